"""GPU: every instantiation of the post-solve list kernels -- qsc_sinfo, qsc_scheck, qsc_qfit_*,
qsc_sfit, qsc_sfit_smooth, qsc_cfit_* (QSC_LAYOUT_DISPATCH x QSC_RP_DISPATCH x QSC_INFO_DISPATCH,
csrc/qsc_info.cuh) and the rank pad x link x log x criterion matrix of qsc_sgain -- against the fp64
references, on the 30 cells of tests/list_matrix_ref.py (rank pad 4 / 8 / 16 x probit / logit x
narrow-linear, narrow-log, wide-linear, wide-log, signed rows), each for both kinds.  Every test
first asserts that it reached the instantiation it is about.

Tolerances.  The pure sums (blocks, check statistics, the calibration's g and H, the gains):
max(1e-5, 10 floor), floor the same metric of the fp32 numpy evaluation of the same sums, in the
metric of the kernel's own test file.  The step comparisons (sfit, sfit_smooth, cfit: one undamped
step from list_matrix_ref.START x the truth): max(1e-5, 10 floor) in the per-pixel (per-bin) norm
sfit_smooth_ref.pixel_rel over the compared set -- the pixels (bins) where the fp32 and the fp64
reference take the same accept decision, fixed from the references alone; the 10x allows for the
kernel's other summation order and its fma's, and tests/test_list_matrix_host.py caps floor at 1e-4
so that the margin cannot hide a wrong term.  Every measured error is printed next to its floor
(lines that start with "lm "; profiles/list_matrix/errors.txt has those of one run)."""
import numpy as np
import pytest
import torch

import check_ref as ckr
import design_ref as dr
import info_ref as ir
import list_matrix_ref as lm
import qfit_ref as qr
import sfit_smooth_ref as ssr
from conftest import rel_fro

pytestmark = pytest.mark.gpu

P, TILE = lm.P, lm.TILE
CELL_IDS = sorted(lm.CELLS)
ULP = 2.0 ** -23
SMOOTH_RIDGE = 1e-2
CHECK_RIDGE = 1.0  # (at 1e-2 the log model's I* / Ixx sits inside the guard's window)
_OBS = {}


def bound(floor):
    return max(1e-5, 10 * floor)


def cell_obs(cell):
    """(problem, packed observations) of a cell, packed once, with the facts the cell is about."""
    from quantized_spectrum_cartography_amd.obs import Observations
    d = lm.problem(cell)
    if cell not in _OBS:
        _OBS[cell] = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                                  log_model=d["log_model"], tile=TILE, R_hint=d["R"],
                                  loss=d["loss"])
    obs = _OBS[cell]
    assert obs.desc.wide == d["wide"] and obs.desc.rowfmt == d["rowfmt"]
    assert obs.rank_pad(d["R"]) == d["RP"]
    assert obs.loss == d["loss"] and bool(obs.log_model) == d["log_model"]
    assert obs.Pp == 192 and obs.desc.ntiles == 3 and int((obs.perm < 0).sum()) == 57
    assert obs.nnz == int(d["Wx"].sum())
    return d, obs


def device_inputs(d, obs, S=None, C=None):
    """(S_pos (Pp, RP), C (R, K)) on the device from (R, P) / (R, K) arrays (default: the truth)."""
    R = d["R"]
    S = d["S"].reshape(R, P) if S is None else torch.as_tensor(S, dtype=torch.float32)
    C = d["C"] if C is None else torch.as_tensor(C, dtype=torch.float32)
    return obs.to_positions(S.reshape(R, P)), C.to(torch.float32).cuda().contiguous()


def to_pixels(obs, x_pos):
    return x_pos[obs.iperm().long()]


# ---------------------------------------------------------------------------------------
# qsc_sinfo
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", CELL_IDS)
def test_sinfo_blocks(cell, kind):
    from quantized_spectrum_cartography_amd import fits
    d, obs = cell_obs(cell)
    R = d["R"]
    S_pos, Cd = device_inputs(d, obs)
    Jb = fits._info_blocks_pos(obs, S_pos, Cd, R, kind)
    assert tuple(Jb.shape) == (192, d["RP"], d["RP"]) and not torch.isnan(Jb).any()
    J64, J32 = lm.blocks(cell, kind), lm.blocks(cell, kind, np.float32)
    floor = rel_fro(J32, J64)
    e = rel_fro(to_pixels(obs, Jb)[:, :R, :R].cpu().numpy(), J64)
    print("lm sinfo %s %s: rel_fro %.2e floor %.2e" % (cell, kind, e, floor))
    assert e <= bound(floor)
    assert (Jb[:, R:, :] == 0).all() and (Jb[:, :, R:] == 0).all()
    assert (Jb[obs.perm < 0] == 0).all()
    assert (to_pixels(obs, Jb)[0] == 0).all()
    assert torch.equal(Jb, Jb.transpose(1, 2))


# ---------------------------------------------------------------------------------------
# qsc_scheck
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fitted", [0, 1])
@pytest.mark.parametrize("cell", CELL_IDS)
def test_scheck_statistics_counts_and_flags(cell, fitted):
    from quantized_spectrum_cartography_amd import fits
    d, obs = cell_obs(cell)
    S_pos, Cd = device_inputs(d, obs)
    bufs = (torch.full((obs.Pp, 4), float("nan"), device="cuda"),
            torch.full((obs.Pp,), -1, dtype=torch.int32, device="cuda"),
            torch.full((obs.Pp,), -1, dtype=torch.int32, device="cuda"))
    stat, count, flags = fits._check_pos(obs, S_pos, Cd, d["R"], fitted, CHECK_RIDGE, *bufs)
    assert not torch.isnan(stat).any() and (count >= 0).all() and (flags >= 0).all()
    pads = obs.perm < 0
    assert (stat[pads] == 0).all() and (count[pads] == 0).all() and (flags[pads] == 0).all()
    st = to_pixels(obs, stat).double().cpu().numpy()
    got = dict(D=st[:, 0], V=st[:, 1], u=st[:, 2], info=st[:, 3],
               n=to_pixels(obs, count).cpu().numpy().astype(np.int64),
               flags=to_pixels(obs, flags).cpu().numpy().astype(np.int64))
    ref = lm.check_stats(cell, fitted, CHECK_RIDGE, np.float64)
    flo = lm.check_stats(cell, fitted, CHECK_RIDGE, np.float32)
    # the integers: exact, the 1 .. 5 ladder among them
    assert np.array_equal(got["n"], ref["n"])
    assert got["n"][0] == 0 and [int(got["n"][n]) for n in lm.LADDER] == [1, 2, 3, 4, 5]
    ex = lm.check_excluded(ref)
    assert lm.check_excluded_ok(ex)
    assert np.array_equal(got["flags"][~ex], ref["flags"][~ex])
    unt = (ref["flags"] & ckr.UNTESTABLE != 0) & ~ex
    assert (got["u"][unt] == 0).all() and (got["info"][unt] == 0).all()
    assert all(got[k][0] == 0 for k in ("D", "V", "u", "info"))
    valid = np.ones(P, bool)
    testable = (ref["flags"] & 3 == 0) & (got["flags"] & 3 == 0) & (ref["n"] > 0)
    for key, keep in (("D", valid), ("V", valid), ("u", testable), ("info", testable)):
        if not keep.any() or np.max(np.abs(ref[key][keep])) == 0:
            assert key in ("u", "info") and fitted == 1
            print("lm scheck %s fitted %d %s: no testable pixel" % (cell, fitted, key))
            continue
        e = ckr.max_err(got[key], ref[key], keep)
        floor = ckr.max_err(flo[key], ref[key],
                            keep & (flo["flags"] & (2 if key in ("D", "V") else 3) == 0))
        print("lm scheck %s fitted %d %s: err %.2e floor %.2e pixels %d"
              % (cell, fitted, key, e, floor, int(keep.sum())))
        assert e <= bound(floor), key


# ---------------------------------------------------------------------------------------
# qsc_qfit_begin / _finish
# ---------------------------------------------------------------------------------------
def _rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", CELL_IDS)
def test_qfit_sums_at_a_point(cell, kind):
    from quantized_spectrum_cartography_amd import fits
    d, obs = cell_obs(cell)
    R = d["R"]
    m = qr.model_of(d)
    S_pos, Cd = device_inputs(d, obs)
    # model_nll: the begin + finish pair at the packed model
    F0, _, _ = qr.evaluate(np.zeros(2), kind="observed", dtype=np.float64, **m)
    v = fits.model_nll(obs, d["S"], d["C"])
    e0 = abs(v - F0) / abs(F0)
    print("lm qfit %s model_nll: err %.2e (fp32 ulps %.2f)" % (cell, e0, e0 / ULP))
    assert e0 <= 8 * ULP
    # one evaluation away from the packed model, with both priors
    start = np.array([0.15, 0.3 * d["sigma"]])
    prior = (0.7, 1.3)
    F64, g64, H64 = qr.evaluate(start, kind=kind, prior=prior, dtype=np.float64, **m)
    F32, g32, H32 = qr.evaluate(start, kind=kind, prior=prior, dtype=np.float32, **m)
    theta, f, cov, gh, info = fits._fit_noise_pos(obs, S_pos, Cd, R, kind, 3, prior, tuple(start),
                                                  1, 1e-6, 0.0, iterate=False)
    f, gh = f.cpu().numpy(), gh.cpu().numpy()
    assert info.tolist()[0] == 0 and (theta.cpu().numpy() == start).all() and f[0] == f[1]
    eF = abs(f[1] - F64) / abs(F64)
    print("lm qfit %s %s F: err %.2e (fp32 ulps %.2f)" % (cell, kind, eF, eF / ULP))
    assert eF <= 8 * ULP
    for what, got, r64, r32 in (("g", gh[:2], g64, g32), ("H", gh[2:], H64, H32)):
        floor = _rel_max(r32, r64)
        e = _rel_max(got, r64)
        print("lm qfit %s %s %s: err %.2e floor %.2e" % (cell, kind, what, e, floor))
        assert e <= bound(floor), what


# ---------------------------------------------------------------------------------------
# qsc_sfit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", lm.RIDGES)
@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", CELL_IDS)
def test_sfit_one_step(cell, kind, ridge):
    from quantized_spectrum_cartography_amd import fits
    d, obs = cell_obs(cell)
    R = d["R"]
    S0 = lm.s_start(d)
    r64, r32 = (lm.sfit_step(cell, kind, ridge, t) for t in (np.float64, np.float32))
    keep, acc = lm.compared(r64, r32, S0, lm.observed_pixels(d))
    floor = lm.pixel_rel(r32["S"], r64["S"], keep)
    S_pos, Cd = device_inputs(d, obs, S=S0)
    S_out, f, steps, counters = fits._fit_s_pos(obs, S_pos, Cd, R, kind, ridge, 1, 1e-5, 0.0,
                                                d["log_model"])
    assert not torch.isnan(S_out).any() and not torch.isnan(f).any()
    assert (S_out[obs.perm < 0] == 0).all() and (S_out[:, R:] == 0).all()
    S = obs.to_pixels(S_out, R).double().cpu().numpy()
    e = lm.pixel_rel(S, r64["S"], keep)
    print("lm sfit %s %s ridge %g: err %.2e floor %.2e compared %d accepted %d"
          % (cell, kind, ridge, e, floor, int(keep.sum()), int(acc.sum())))
    assert (to_pixels(obs, steps).cpu().numpy()[keep] == 1).all()
    assert e <= bound(floor)


# ---------------------------------------------------------------------------------------
# qsc_sfit_smooth
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", ssr.KINDS, ids=[k for k, _ in ssr.KINDS])
@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", CELL_IDS)
def test_sfit_smooth_one_visit_of_each_colour(cell, kind, smooth):
    from quantized_spectrum_cartography_amd import fits
    d, obs = cell_obs(cell)
    R = d["R"]
    sk, dl = smooth
    code, delta = fits._kind_code(sk, dl)
    S0 = lm.s_start(d)
    colour = torch.as_tensor(ssr.colors(lm.I, lm.J))
    perm = obs.perm.cpu().long()
    for color in (0, 1):
        r64, r32 = (lm.smooth_visit(cell, kind, SMOOTH_RIDGE, sk, dl, color, t)
                    for t in (np.float64, np.float32))
        keep, acc = lm.compared(r64, r32, S0, r64["own"])
        floor = lm.pixel_rel(r32["S"], r64["S"], keep)
        S_pos, Cd = device_inputs(d, obs, S=S0)
        before = S_pos.clone()
        f, nll, steps, counters, ws = fits._sfit_smooth_bufs(obs, R, 1)
        fits._sfit_smooth_visit(obs, S_pos, Cd, R, color, kind, SMOOTH_RIDGE, 1, 1e-5, 0.0,
                                d["log_model"], code, delta, ssr.WEIGHT, f, nll, steps,
                                counters[0, color], ws)
        assert not torch.isnan(S_pos).any()
        # the other colour's rows and the padding rows: the bits they had
        other = (perm < 0) | (colour[perm.clamp(min=0)] != color)
        assert int(other.sum()) == 57 + int((~r64["own"]).sum())
        assert torch.equal(S_pos.cpu()[other], before.cpu()[other])
        S = obs.to_pixels(S_pos, R).double().cpu().numpy()
        e = lm.pixel_rel(S, r64["S"], keep)
        print("lm smooth %s %s %s colour %d: err %.2e floor %.2e compared %d accepted %d"
              % (cell, kind, sk, color, e, floor, int(keep.sum()), int(acc.sum())))
        assert (to_pixels(obs, steps).cpu().numpy()[keep] == 1).all()
        assert e <= bound(floor)


# ---------------------------------------------------------------------------------------
# qsc_cfit_begin / _iterate / _finish
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", lm.RIDGES)
@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", CELL_IDS)
def test_cfit_one_step(cell, kind, ridge):
    from quantized_spectrum_cartography_amd import _lib, fits
    d, obs = cell_obs(cell)
    R = d["R"]
    desc, _, _ = obs.layout(R)
    assert _lib.lib().qsc_cfit_groups(desc, R) == 3  # the fixed-order sum over groups is in play
    C0 = lm.c_start(d)
    r64, r32 = (lm.cfit_step(cell, kind, ridge, t) for t in (np.float64, np.float32))
    keep, acc = lm.compared(r64, r32, C0, lm.observed_bins(d), "C")
    floor = lm.pixel_rel(r32["C"], r64["C"], keep)
    S_pos, Cd = device_inputs(d, obs, C=C0)
    run = lambda: fits._fit_c_pos(obs, S_pos, Cd, R, kind, ridge, 1, 1e-5, 0.0, True)
    C_out, f, steps, counters, _ = run()
    C2, f2, steps2, counters2, _ = run()
    assert torch.equal(C_out, C2) and torch.equal(f, f2) and torch.equal(steps, steps2)
    assert torch.equal(counters, counters2)
    assert not torch.isnan(C_out).any() and not torch.isnan(f).any()
    e = lm.pixel_rel(C_out.double().cpu().numpy(), r64["C"], keep)
    print("lm cfit %s %s ridge %g: err %.2e floor %.2e compared %d accepted %d"
          % (cell, kind, ridge, e, floor, int(keep.sum()), int(acc.sum())))
    assert (steps.cpu().numpy()[keep] == 1).all()
    assert e <= bound(floor)


# ---------------------------------------------------------------------------------------
# qsc_sgain: rank pad x link x log x criterion (no layout axis)
# ---------------------------------------------------------------------------------------
GAIN_CELLS = [c for c in CELL_IDS if lm.CELLS[c][2] in ("narrow-lin", "narrow-log")]


@pytest.mark.parametrize("crit", dr.CRITERIA)
@pytest.mark.parametrize("cell", GAIN_CELLS)
def test_sgain_of_the_full_plan(cell, crit):
    from quantized_spectrum_cartography_amd import fits
    d, obs = cell_obs(cell)
    ridge = 1e-2
    S, C = lm.flat(d)
    model = (d["b"].double().numpy(), d["sigma"], d["offset"], d["log_model"], d["loss"])
    J64 = lm.blocks(cell, "expected")
    A = lm.cached(("plan", cell), lambda: dr.plan_blocks(S, C, None, *model))
    ref, first, bad, piv0, piv1 = dr.gains(J64, A, C, ridge, crit)
    assert not first.any() and not bad.any() and piv0.min() > 1e-4 and piv1.min() > 1e-4
    keep = np.ones(P, bool)
    flo = dr.gains_fp32(J64, S, C, None, ridge, crit, *model).astype(np.float64)
    r = fits.design(obs, d["S"], d["C"], criterion=crit, kind="expected", ridge=ridge)
    got = r.gain.reshape(P).double().cpu().numpy()
    assert (r.first_look, r.degenerate) == (0, 0) and np.isfinite(got).all() and (got >= 0).all()

    def errors(x):
        x, y = x[keep], ref[keep]
        return (float(np.max(np.abs(x - y)) / np.max(np.abs(y))),
                float(np.max(np.abs(x - y) / np.abs(y))))
    (e_max, e_pix), (f_max, f_pix) = errors(got), errors(flo)
    print("lm sgain %s %s: err %.2e floor %.2e per-pixel err %.2e floor %.2e"
          % (cell, crit, e_max, f_max, e_pix, f_pix))
    assert e_max <= bound(f_max)
    assert e_pix <= bound(f_pix)


# ---------------------------------------------------------------------------------------
# qsc_entry_info, qsc_entry_check, qsc_entry_calib: link x log x kind on one short vector
# ---------------------------------------------------------------------------------------
ENTRY_CELLS = ["R3-%s-%s" % (loss, ds) for loss in lm.LINKS for ds in ("narrow-lin", "narrow-log")]


def entry_vector(d):
    """(Y, t fp32, valid, saturated): every code at the middle of its bin and exactly on its
    lower edge, values 60 link scales past the outermost finite edges (every edge saturated) and,
    under the log model, t + offset <= 0 and t = -offset."""
    e = ir.edges_of(d["b"].double().numpy(), d["log_model"])
    # (60 a: z = 60 for the probit, which saturates at 14; z = 110 for the logit, at 100 -- and
    # e^x stays inside fp32 under the log model)
    a = ir.link_scale(d["sigma"], d["loss"]) * (110.0 / 60.0 if d["loss"] == "logit" else 1.0)
    nb = d["nbins"]
    inner = e[1:-1]
    lo = np.r_[inner[0] - 2 * d["sigma"], inner]
    hi = np.r_[inner, inner[-1] + 2 * d["sigma"]]
    x = np.r_[0.5 * (lo + hi), lo[1:]]
    Y = np.r_[np.arange(nb), np.arange(1, nb)]
    n_sat = 2 if not d["log_model"] else 1
    x = np.r_[x, inner[-1] + 60 * a, (inner[0] - 60 * a,) if not d["log_model"] else ()]
    Y = np.r_[Y, nb - 1, (0,) if not d["log_model"] else ()]
    t = np.exp(x) - d["offset"] if d["log_model"] else x
    sat = np.r_[np.zeros(len(t) - n_sat, bool), np.ones(n_sat, bool)]
    valid = np.ones(len(t), bool)
    if d["log_model"]:
        t = np.r_[t, -0.5, -d["offset"]]
        Y = np.r_[Y, 1, 2]
        sat = np.r_[sat, False, False]
        valid = np.r_[valid, False, False]
    t = t.astype(np.float32)
    if d["log_model"]:
        assert (t[~valid] + np.float32(d["offset"]) <= 0).all()
    return Y.astype(np.int64), t, valid, sat


@pytest.mark.parametrize("kind", lm.KINDS)
@pytest.mark.parametrize("cell", ENTRY_CELLS)
def test_entry_ops_on_the_edge_vector(cell, kind):
    from quantized_spectrum_cartography_amd import utils
    d, obs = cell_obs(cell)
    Y, t, valid, sat = entry_vector(d)
    b = d["b"].double().numpy()
    args = (b, d["sigma"], d["offset"], d["log_model"], d["loss"])
    Yd, td = torch.from_numpy(Y).cuda(), torch.from_numpy(t).cuda()
    ok = valid & ~sat
    t64 = t.astype(np.float64)
    # qsc_entry_info
    h = utils.entry_information(td, Yd, d["b"], d["sigma"], offset=d["offset"],
                                log_model=d["log_model"], loss=d["loss"], kind=kind).cpu().numpy()
    assert not np.isnan(h[valid]).any()
    hr = ir.curvature(t64[ok], Y[ok], *args, kind)
    e = _rel_max(h[ok], hr)
    print("lm entry_info %s %s: err %.2e" % (cell, kind, e))
    assert e <= 1e-5
    assert (h[sat] == 0).all()
    # qsc_entry_check (no kind axis: run once per cell)
    if kind == "expected":
        out = utils.entry_check(Yd, td, obs).cpu().numpy()
        et = ckr.entry_terms(t64, Y, [float(v) for v in d["b"]], *args[1:])
        assert np.isfinite(out).all() and (out[:, ~valid] == 0).all()
        for i, key in enumerate(("dl", "var", "gx", "hx", "dxdt")):
            e = _rel_max(out[i][ok], et[key][ok])
            print("lm entry_check %s %s: err %.2e" % (cell, key, e))
            assert e <= 1e-5, key
        assert (out[2][sat] == 0).all() and (out[3][sat] == 0).all()
    # qsc_entry_calib
    tau, beta = 0.2, 0.3 * d["sigma"]
    cal = utils.entry_calibration(Yd, td, obs, tau, beta, kind).cpu().numpy()
    cargs = (b, d["sigma"], tau, beta, d["offset"], d["log_model"], d["loss"], kind)
    f64, g64, H64, neg = qr.terms(t64, Y, *cargs, dtype=np.float64)
    f32, g32, H32, _ = qr.terms(t, Y, *cargs, dtype=np.float32)
    assert np.array_equal(neg, ~valid) and np.isposinf(cal[0][~valid]).all()
    assert np.isfinite(cal[:, valid]).all()
    ref = np.vstack([f64[None], g64, H64])[:, ok]
    ref32 = np.vstack([f32[None], g32, H32]).astype(np.float64)[:, ok]
    for i, term in enumerate(("f", "g_tau", "g_beta", "H_tt", "H_tb", "H_bb")):
        floor = _rel_max(ref32[i], ref[i])
        e = _rel_max(cal[i][ok], ref[i])
        print("lm entry_calib %s %s %s: err %.2e floor %.2e" % (cell, kind, term, e, floor))
        assert e <= bound(floor), term
