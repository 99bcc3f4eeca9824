"""GPU: the expected information gain of planned readings -- qsc_sgain and qmc.design -- against
the fp64 reference of tests/design_ref.py.

Shapes, draws and cases are those of tests/test_gpu_info.py (its problem(), observations() and
reference blocks are shared): 9 x 15 pixels with tile 64 (Pp = 192, six slices, 57 padding
positions), R = 3 / 8 at K = 37 and R = 16 at K = 70 (K odd and even: the two lane halves of a
position take unequal and equal shares of the bins), pixel 0 unobserved, sampling rate 0.7.

Tolerance (per case, criterion and ridge): the metric is max|got - ref| / max|ref| over the
identified pixels and, for the full plan w = 1, also the largest per-pixel relative error.  Each
is held to max(1e-5, 10 floor): 1e-5 is the project's pass tolerance, floor the same metric of an
fp32 numpy evaluation of the same formulas (design_ref.gains_fp32: fp32 map, sums, Cholesky and
inverse factor from the fp32-rounded reference J, S and C), measured here and independent of the
code under test; the factor 10 is the allowance of tests/test_gpu_info.py for fp32 summation error
amplified by the condition number (DESIGN.md section 7s has the measured errors)."""
import ctypes

import numpy as np
import pytest
import torch

import design_ref as dr
import test_gpu_info as gi
from conftest import rel_fro

pytestmark = pytest.mark.gpu

I, J, P = gi.I, gi.J, gi.P
CASES = list(gi.CASES)
SPARSE = {5: 1.0, 17: 2.0, 30: 0.5}  # bin: planned readings

_PLAN, _GAINS = {}, {}


def model_args(d):
    return (d["b"].double().numpy(), d["sigma"], d["offset"], d["log_model"], d["loss"])


def s64(d):
    return d["S"].reshape(d["R"], -1).double().numpy()


def plan_blocks(name, w=None):
    """(P, R, R) fp64 blocks of the plan, computed once per (case, plan) and left unchanged."""
    key = (name, None if w is None else tuple(w))
    if key not in _PLAN:
        d = gi.problem(name)
        _PLAN[key] = dr.plan_blocks(s64(d), d["C"].double().numpy(), w, *model_args(d))
        _PLAN[key].setflags(write=False)
    return _PLAN[key]


def ref_gains(name, crit, ridge, kind="expected", w=None):
    key = (name, crit, ridge, kind, None if w is None else tuple(w))
    if key not in _GAINS:
        d = gi.problem(name)
        _GAINS[key] = dr.gains(gi.ref_blocks(name, kind), plan_blocks(name, w),
                               d["C"].double().numpy(), ridge, crit)
    return _GAINS[key]


def floor_gains(name, crit, ridge, kind="expected", w=None, keep=None):
    d = gi.problem(name)
    return dr.gains_fp32(gi.ref_blocks(name, kind), s64(d), d["C"].double().numpy(), w, ridge,
                         crit, *model_args(d), keep=keep).astype(np.float64)


def errors(got, ref, keep):
    """(max|got - ref| / max|ref|, max per-pixel relative error) over the pixels `keep`."""
    got, ref = np.asarray(got, np.float64)[keep], np.asarray(ref, np.float64)[keep]
    return (float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))),
            float(np.max(np.abs(got - ref) / np.abs(ref))))


def raw_gain(obs, d, crit, ridge, w=None, Jb=None):
    """qsc_sgain through the ABI into a NaN-filled gain (Pp,): (gain, n_first, n_bad)."""
    from quantized_spectrum_cartography_amd import _lib, qmc
    R = d["R"]
    RP = obs.rank_pad(R)
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = d["C"].cuda().contiguous()
    if Jb is None:
        Jb = gi.raw_blocks(obs, d, "expected")
    G = torch.zeros((RP, RP), device="cuda")
    G[:R, :R] = Cd @ Cd.t()
    wd = None if w is None else torch.tensor(w, dtype=torch.float32, device="cuda")
    gain = torch.full((obs.Pp,), float("nan"), device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    _lib.call("qsc_sgain", _lib.ptr(S_pos), _lib.ptr(Cd), _lib.ptr(Jb), _lib.ptr(obs.perm),
              _lib.ptr(wd), _lib.ptr(G), obs.model, R, obs.K, obs.P, obs.Pp,
              qmc.DESIGN_CRITERIA[crit], float(ridge), _lib.ptr(gain), _lib.ptr(cnt[0:1]),
              _lib.ptr(cnt[1:2]), _lib.stream())
    n_first, n_bad = cnt.tolist()
    return gain, n_first, n_bad


# ---------------------------------------------------------------------------------------
# (i) the raw ABI
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", dr.CRITERIA)
@pytest.mark.parametrize("name", CASES)
def test_raw_gain_is_fully_written_and_two_calls_agree_bit_for_bit(name, crit):
    d = gi.problem(name)
    obs = gi.observations(name)
    Jb = gi.raw_blocks(obs, d, "expected")
    a, fa, ba = raw_gain(obs, d, crit, 0.0, Jb=Jb)
    b, fb, bb = raw_gain(obs, d, crit, 0.0, Jb=Jb)
    assert not torch.isnan(a).any()
    pads = obs.perm < 0
    assert int(pads.sum()) == obs.Pp - P == 57
    assert (a[pads] == 0).all()
    assert torch.equal(a, b) and (fa, ba) == (fb, bb) == (1, 0)
    assert int(torch.isinf(a).sum()) == 1 and (a >= 0).all()
    # the default plan is the plan of ones
    c, fc, bc = raw_gain(obs, d, crit, 0.0, w=[1.0] * d["K"], Jb=Jb)
    assert torch.equal(a, c) and (fc, bc) == (1, 0)
    # the zero plan is worth exactly nothing and leaves the unobserved pixel degenerate
    z, fz, bz = raw_gain(obs, d, crit, 0.0, w=[0.0] * d["K"], Jb=Jb)
    assert (z == 0).all() and (fz, bz) == (0, 1)


# ---------------------------------------------------------------------------------------
# (ii) parity with the reference: the full plan
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 1e-2])
@pytest.mark.parametrize("crit", dr.CRITERIA)
@pytest.mark.parametrize("name", CASES)
def test_gain_of_the_full_plan_vs_reference(name, crit, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d = gi.problem(name)
    obs = gi.observations(name)
    ref, first, bad, piv0, piv1 = ref_gains(name, crit, ridge)
    keep = np.ones(P, bool)
    if ridge == 0.0:
        # the unobserved pixel: J exactly 0, so the pivot of M0 is exactly 0; M1 sums K >= R bins
        keep[0] = False
        assert first[0] and first.sum() == 1 and piv0[0] == 0.0
    else:
        assert not first.any()
    assert not bad.any()
    # no pivot of an identified pixel is near the classification threshold
    assert piv0[keep].min() > 1e-4 and piv1.min() > 1e-4, (piv0[keep].min(), piv1.min())
    f_max, f_pix = errors(floor_gains(name, crit, ridge, keep=keep), ref, keep)
    r = qmc.design(obs, d["S"], d["C"], criterion=crit, kind="expected", ridge=ridge)
    assert tuple(r.gain.shape) == (1, I, J) and r.entry_gain is None
    got = r.gain.reshape(P).cpu().numpy()
    e_max, e_pix = errors(got, ref, keep)
    print("case", name, crit, "ridge", ridge, "err", e_max, "floor", f_max, "per-pixel err", e_pix,
          "floor", f_pix, "min pivots", piv0[keep].min(), piv1.min())
    assert not np.isnan(got).any() and (got >= 0).all()
    assert r.degenerate == 0
    if ridge == 0.0:
        assert r.first_look == 1 and got[0] == np.inf and np.isfinite(got[1:]).all()
        assert r.best(1).tolist() == [[0, 0]]
    else:
        assert r.first_look == 0 and np.isfinite(got).all()
    assert e_max <= max(1e-5, 10 * f_max)
    assert e_pix <= max(1e-5, 10 * f_pix)


# ---------------------------------------------------------------------------------------
# (iii) blocks of kind "observed"; a sparse plan
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit", dr.CRITERIA)
def test_gain_on_observed_blocks_vs_reference(crit):
    """Linear probit, R = 8: the likelihood is log-concave, so the observed J is positive
    semidefinite."""
    from quantized_spectrum_cartography_amd import qmc
    name, ridge = "onebit8", 1e-2
    d = gi.problem(name)
    ref, first, bad, piv0, piv1 = ref_gains(name, crit, ridge, kind="observed")
    assert not first.any() and not bad.any() and piv0.min() > 1e-4 and piv1.min() > 1e-4
    keep = np.ones(P, bool)
    f_max, f_pix = errors(floor_gains(name, crit, ridge, kind="observed"), ref, keep)
    r = qmc.design(gi.observations(name), d["S"], d["C"], criterion=crit, kind="observed",
                   ridge=ridge)
    e_max, e_pix = errors(r.gain.reshape(P).cpu().numpy(), ref, keep)
    print("case", name, crit, "observed blocks, err", e_max, "floor", f_max, "per-pixel err",
          e_pix, "floor", f_pix)
    assert (r.first_look, r.degenerate) == (0, 0)
    assert e_max <= max(1e-5, 10 * f_max)
    assert e_pix <= max(1e-5, 10 * f_pix)


@pytest.mark.parametrize("crit", dr.CRITERIA)
def test_gain_of_a_sparse_plan_vs_reference(crit):
    """Three bins with 1, 2 and 0.5 readings, R = 8, ridge 1e-2 (at ridge 0 the unobserved pixel's
    M1 would be singular by rank: a rounding-level pivot, whose classification is not tested)."""
    from quantized_spectrum_cartography_amd import qmc
    name, ridge = "onebit8", 1e-2
    d = gi.problem(name)
    w = [SPARSE.get(k, 0.0) for k in range(d["K"])]
    ref, first, bad, piv0, piv1 = ref_gains(name, crit, ridge, w=w)
    assert not first.any() and not bad.any() and piv0.min() > 1e-4 and piv1.min() > 1e-4
    keep = np.ones(P, bool)
    f_max, _ = errors(floor_gains(name, crit, ridge, w=w), ref, keep)
    r = qmc.design(gi.observations(name), d["S"], d["C"], weights=torch.tensor(w), criterion=crit,
                   ridge=ridge)
    got = r.gain.reshape(P).cpu().numpy()
    e_max, _ = errors(got, ref, keep)
    print("case", name, crit, "sparse plan, err", e_max, "floor", f_max)
    assert (r.first_look, r.degenerate) == (0, 0)
    assert (got > 0).all() and np.isfinite(got).all()
    assert e_max <= max(1e-5, 10 * f_max)
    # fewer readings are worth less than the full plan
    full = ref_gains(name, crit, ridge)[0]
    assert (got < full).all()


# ---------------------------------------------------------------------------------------
# (iv) additivity through the public API: planned readings against readings taken
# ---------------------------------------------------------------------------------------
def test_design_gain_equals_the_logdet_change_when_the_readings_are_added():
    """D-gain of the full plan at a pixel = 1/2 (logdet(info2 + ridge I) - logdet(info + ridge I))
    with info2 the expected blocks after one reading of every bin is added at that pixel
    (Observations.from_readings; at an observed pixel cells repeat).
    Bound: both sides come from fp32 blocks held to rel_fro <= eps = 1e-5 (the pass tolerance of
    tests/test_gpu_info.py); a relative perturbation eps of a block moves its logdet by at most
    R kappa eps, kappa the block's condition number, and two logdets enter each side:
    |difference| <= 4 R kappa eps, kappa taken from the fp64 reference blocks in the test."""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    name, ridge = "onebit3", 1e-2
    d = gi.problem(name)
    R, K = d["R"], d["K"]
    obs = gi.observations(name)
    pixels = [(0, 0), (4, 7), (8, 14)]  # the unobserved pixel and two observed ones
    Wx = d["Wx"].reshape(K, I, J)
    assert Wx[:, 4, 7].sum() > 0 and Wx[:, 8, 14].sum() > 0 and Wx[:, 0, 0].sum() == 0
    k0, i0, j0 = torch.nonzero(Wx, as_tuple=True)
    c0 = d["Y"].reshape(K, I, J)[k0, i0, j0]
    ks = torch.arange(K).repeat(len(pixels))
    is_ = torch.tensor([p[0] for p in pixels]).repeat_interleave(K)
    js = torch.tensor([p[1] for p in pixels]).repeat_interleave(K)
    cs = (torch.arange(K * len(pixels)) % 2)  # (the codes do not matter to the expected blocks)
    obs2 = Observations.from_readings(torch.cat([k0, ks]), torch.cat([i0, is_]),
                                      torch.cat([j0, js]), torch.cat([c0, cs]), (K, I, J), d["b"],
                                      d["sigma"], tile=gi.TILE, R_hint=R, loss=d["loss"])
    assert obs2.max_repeat == 2
    info = qmc.confidence(obs, d["S"], d["C"], kind="expected").info.double().cpu().numpy()
    info2 = qmc.confidence(obs2, d["S"], d["C"], kind="expected").info.double().cpu().numpy()
    r = qmc.design(obs, d["S"], d["C"], criterion="D", ridge=ridge)
    Jr = gi.ref_blocks(name, "expected")
    eye = ridge * np.eye(R)
    for (i, j) in pixels:
        p = i * J + j
        want = 0.5 * (np.linalg.slogdet(info2[p] + eye)[1] - np.linalg.slogdet(info[p] + eye)[1])
        got = float(r.gain[0, i, j])
        kappa = max(np.linalg.cond(Jr[p] + eye), np.linalg.cond(Jr[p] + plan_blocks(name)[p] + eye))
        bound = 4 * R * kappa * 1e-5
        print("pixel", (i, j), "design", got, "logdet change", want, "diff", abs(got - want),
              "bound", bound)
        assert abs(got - want) <= bound
    # elsewhere nothing was added: the same blocks up to the summation order of the new packing
    others = np.ones(P, bool)
    others[[i * J + j for i, j in pixels]] = False
    assert rel_fro(info2[others], info[others]) <= 1e-5


# ---------------------------------------------------------------------------------------
# (v) the "which bin" companion and the ranking
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["onebit3", "bins16"])
def test_entry_gain_and_best_vs_reference(name):
    from quantized_spectrum_cartography_amd import qmc
    import info_ref as ir
    d = gi.problem(name)
    obs = gi.observations(name)
    R, K = d["R"], d["K"]
    ridge = 1e-2
    Jr = gi.ref_blocks(name, "expected")
    C64 = d["C"].double().numpy()
    ref = dr.entry_gain(Jr, s64(d), C64, None, ridge, *model_args(d))
    # the fp32 floor: fp32 std_T (info_ref.stds_fp32) and fp32 h, log1p in fp32
    _, sT32 = ir.stds_fp32(Jr, C64, ridge)
    h32 = dr.expected_information(s64(d), C64, *model_args(d)).astype(np.float32)
    fl = np.float32(0.5) * np.log1p(h32 * sT32 * sT32)
    floor = float(np.max(np.abs(fl.astype(np.float64) - ref)) / np.max(ref))
    r = qmc.design(obs, d["S"], d["C"], criterion="D", ridge=ridge, entry_gain=True)
    assert tuple(r.entry_gain.shape) == (K, 1, I, J)
    got = r.entry_gain.reshape(K, P).cpu().numpy()
    e = float(np.max(np.abs(got - ref)) / np.max(ref))
    tol = max(1e-5, 10 * floor)
    print("case", name, "entry_gain err", e, "floor", floor)
    assert np.isfinite(got).all() and (got >= 0).all()
    assert e <= tol
    # without a ridge the unobserved pixel's entries are first looks
    r0 = qmc.design(obs, d["S"], d["C"], criterion="D", ridge=0.0, entry_gain=True)
    eg0 = r0.entry_gain.reshape(K, P)
    assert torch.isinf(eg0[:, 0]).all() and torch.isfinite(eg0[:, 1:]).all()
    assert not torch.isnan(eg0).any()
    # best(n): +inf first, then the reference's order wherever its gains differ by more than the
    # tolerance of the parity test
    gref = ref_gains(name, "D", 0.0)[0]
    best = r0.best(P)
    idx = (best[:, 0] * J + best[:, 1]).cpu().numpy()
    assert sorted(idx.tolist()) == list(range(P)) and idx[0] == 0 and gref[0] == np.inf
    scale = np.max(gref[1:])
    ident = np.arange(P) != 0
    f_max, _ = errors(floor_gains(name, "D", 0.0, keep=ident), gref, ident)
    slack = 2 * max(1e-5, 10 * f_max) * scale
    seq = gref[idx]
    assert (seq[1:-1] >= seq[2:] - slack).all()
    assert dr.order(gref)[0] == 0
    assert tuple(r0.best(5).shape) == (5, 2) and torch.equal(r0.best(5), best[:5])


# ---------------------------------------------------------------------------------------
# (vi) the ABI's argument checks
# ---------------------------------------------------------------------------------------
def test_abi_rejects_what_it_cannot_compute():
    from quantized_spectrum_cartography_amd import _lib
    L = _lib.lib()
    d = gi.problem("onebit3")
    R = d["R"]
    obs = gi.observations("onebit3")
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = d["C"].cuda().contiguous()
    Jb = torch.zeros((obs.Pp, 4, 4), device="cuda")
    G = torch.zeros((4, 4), device="cuda")
    gain = torch.zeros(obs.Pp, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = _lib.ptr

    def sgain(model=obs.model, R_=R, K_=obs.K, P_=obs.P, Pp_=obs.Pp, crit=0, ridge=0.1, G_=G,
              gain_=gain, nf=cnt[0:1], nb=cnt[1:2], J_=Jb):
        return L.qsc_sgain(p(S_pos), p(Cd), p(J_), p(obs.perm), None, p(G_), model, R_, K_, P_,
                           Pp_, crit, ctypes.c_float(ridge), p(gain_), p(nf), p(nb), None)

    assert sgain() == 0 and sgain(crit=1) == 0 and sgain(crit=2) == 0
    assert sgain(crit=0, G_=None) == 0 and sgain(crit=1, G_=None) == 0
    sq = _lib.make_model(d["b"], d["sigma"], loss="squared")
    assert sgain(model=sq) == _lib.QSC_EINVAL
    assert sgain(model=None) == _lib.QSC_EINVAL
    assert sgain(ridge=-1.0) == _lib.QSC_EINVAL
    assert sgain(ridge=float("nan")) == _lib.QSC_EINVAL
    assert sgain(crit=3) == _lib.QSC_EINVAL and sgain(crit=-1) == _lib.QSC_EINVAL
    assert sgain(crit=2, G_=None) == _lib.QSC_EINVAL
    assert sgain(R_=0) == _lib.QSC_EINVAL and sgain(R_=17) == _lib.QSC_EINVAL
    assert sgain(K_=0) == _lib.QSC_EINVAL and sgain(P_=0) == _lib.QSC_EINVAL
    assert sgain(Pp_=obs.P - 1) == _lib.QSC_EINVAL and sgain(Pp_=obs.Pp + 1) == _lib.QSC_EINVAL
    assert sgain(gain_=None) == _lib.QSC_EINVAL and sgain(nf=None) == _lib.QSC_EINVAL
    assert sgain(nb=None) == _lib.QSC_EINVAL and sgain(J_=None) == _lib.QSC_EINVAL
    # C^T, the edges and w beyond the LDS: refused before any launch (the buffers stay tiny).
    # At rank 16 a row of C^T takes 20 floats and w one more: 84 K + 16 bytes against 163840.
    k_fit = (160 * 1024 - 16) // 84
    assert sgain(R_=16, K_=k_fit + 1) == _lib.QSC_EUNSUPPORTED
    assert sgain(R_=16, K_=4096) == _lib.QSC_EUNSUPPORTED
    torch.cuda.synchronize()
