"""GPU: observations packed from a list of readings (Observations.from_readings,
qsc_obs_readings_*), repeated readings per cell through the passes and the solver.

Shapes: 9 x 15 pixels (P = 135, ragged), K = 37 / 70 (one / two k-slices, both ragged), tile 64
(Pp = 192, three tiles -- odd, for the snake deal -- and 57 padding positions) or 128.
Inputs and references come from tests/test_readings_host.py, which also checks them on the CPU;
the numpy packer is tests/readings_ref.py."""
import numpy as np
import pytest
import torch

import readings_ref as rr
from test_pass_matrix_host import errors, make_case
from test_readings_host import (F, I, J, M, P, RANKS, SETS, TILE, case, readings,
                                summed_reference)

pytestmark = pytest.mark.gpu

TOL = 1e-5
FIELDS = ("perm", "counts", "s_width", "s_off", "c_width", "c_off", "c_kmap", "s_entries",
          "c_entries")


def _dense(d, R, tile, schedule, perm=None, loss="probit"):
    from quantized_spectrum_cartography_amd.obs import Observations
    return Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                        log_model=d["log_model"], R_hint=R, tile=tile, schedule=schedule,
                        perm=perm, loss=loss)


def _from(d, kijc, shape, R, tile, schedule=False, perm=None, loss="probit"):
    from quantized_spectrum_cartography_amd.obs import Observations
    return Observations.from_readings(*kijc, shape, d["b"], d["sigma"], offset=d["offset"],
                                      log_model=d["log_model"], R_hint=R, tile=tile,
                                      schedule=schedule, perm=perm, loss=loss)


def _kijc(k, p, c, Jw, order=None, code_dtype=torch.int64):
    if order is not None:
        k, p, c = k[order], p[order], c[order]
    return (torch.from_numpy(k), torch.from_numpy(p // Jw), torch.from_numpy(p % Jw),
            torch.from_numpy(c).to(code_dtype))


def _desc(obs):
    return {name: getattr(obs.desc, name) for name, _ in obs.desc._fields_}


def _assert_same_packing(a, b):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert _desc(a) == _desc(b)


def _arrays(obs, s_entries=None, c_entries=None, desc=None):
    """The packing as the dict readings_ref.pack returns."""
    et = np.uint32 if obs.desc.wide else np.uint16
    g = lambda t: t.cpu().numpy()  # noqa: E731
    d = desc if desc is not None else obs.desc
    return dict(counts=g(obs.counts), perm=g(obs.perm), s_width=g(obs.s_width),
                s_off=g(obs.s_off), c_width=g(obs.c_width), c_off=g(obs.c_off),
                c_kmap=g(obs.c_kmap),
                s_entries=g(obs.s_entries if s_entries is None else s_entries).view(et),
                c_entries=g(obs.c_entries if c_entries is None else c_entries).view(et),
                desc={name: getattr(d, name) for name, _ in d._fields_ if name != "reserved_"})


def _assert_bytes_equal_numpy(obs, want):
    got = _arrays(obs)
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
    assert got["desc"] == want["desc"]


# ---- packing, no repeats ------------------------------------------------------------------
# name -> (K, bins, R_hint, tile, I, J, f)
NOREPEAT = {"onebit-sr": (37, 2, 8, 64, I, J, F), "lin4": (70, 4, 8, 64, I, J, F),
            "wide16": (37, 16, 8, 64, I, J, F), "lin4-tile128": (70, 4, 8, 128, I, J, F),
            "onebit-tile128": (37, 2, 8, 128, I, J, F),
            "many-tiles": (3, 2, 8, 64, 220, 320, 0.01)}


@pytest.mark.parametrize("schedule", [False, True])
@pytest.mark.parametrize("name", sorted(NOREPEAT))
def test_repeat_free_packing_is_bit_identical(name, schedule):
    K, nbins, R, tile, Ih, Jw, f = NOREPEAT[name]
    d = make_case(5200 + sorted(NOREPEAT).index(name), 3, Ih, Jw, K, f, nbins, False)
    dense = _dense(d, R, tile, schedule)
    assert dense.desc.wide == int(nbins > 15) and dense.desc.rowfmt == int(nbins == 2)
    if name == "many-tiles":
        assert dense.desc.ntiles == 1100 and (dense.c_width == 0).any()
    k, p, c = rr.dense_readings(d["Y"].numpy(), d["Wx"].numpy())
    shape = (K, Ih, Jw)
    shuffled = np.random.RandomState(7).permutation(k.size)
    for order, dt in ((shuffled, torch.int64), (None, torch.uint8), (shuffled[::-1].copy(),
                                                                      torch.int32)):
        obs = _from(d, _kijc(k, p, c, Jw, order, dt), shape, R, tile, schedule)
        assert obs.codes is None and obs.nnz == k.size and obs.stats()["max_repeat"] == 1
        _assert_same_packing(dense, obs)
    if not schedule:
        want = rr.pack(k, p, c, K, Ih * Jw, tile, nbins, rowfmt=dense.desc.rowfmt)
        _assert_bytes_equal_numpy(obs, want)
    assert "max_repeat" not in dense.stats()


def test_repeat_free_packing_with_a_callers_perm():
    K, nbins, R, tile = 70, 4, 8, 64
    d = make_case(5300, 3, I, J, K, F, nbins, False)
    g = torch.Generator().manual_seed(3)
    perm = torch.cat([torch.randperm(P, generator=g), -torch.ones(192 - P, dtype=torch.int64)])
    perm = perm[torch.randperm(192, generator=g)].to(torch.int32)  # padding anywhere
    dense = _dense(d, R, tile, False, perm=perm)
    k, p, c = rr.dense_readings(d["Y"].numpy(), d["Wx"].numpy())
    order = np.random.RandomState(8).permutation(k.size)
    obs = _from(d, _kijc(k, p, c, J, order), (K, I, J), R, tile, perm=perm)
    _assert_same_packing(dense, obs)
    _assert_bytes_equal_numpy(obs, rr.pack(k, p, c, K, P, tile, nbins, perm=perm.numpy()))


@pytest.mark.parametrize("schedule", [False, True])
def test_code_field_copy_of_a_readings_object(schedule):
    """One-bit signed rows at R_hint 8; at R = 16 with K = 500 the passes' doubled tables do not
    fit, so layout(16) packs a code-field copy -- from the kept sorted readings."""
    K, R = 500, 8
    d = make_case(5400, 3, I, J, K, 0.05, 2, False)
    dense = _dense(d, R, TILE, schedule)
    k, p, c = rr.dense_readings(d["Y"].numpy(), d["Wx"].numpy())
    obs = _from(d, _kijc(k, p, c, J, np.random.RandomState(9).permutation(k.size)), (K, I, J), R,
                TILE, schedule)
    assert dense.desc.rowfmt == 1 and not dense.signed_rows_ok(16)
    _assert_same_packing(dense, obs)
    dd, ds, dc = dense.layout(16)
    od, os_, oc = obs.layout(16)
    assert dd.rowfmt == 0 and od.rowfmt == 0 and obs.codes is None
    assert torch.equal(ds, os_) and torch.equal(dc, oc)
    assert not torch.equal(ds, dense.s_entries)
    if not schedule:
        want = rr.pack(k, p, c, K, P, TILE, 2, rowfmt=0)
        got = _arrays(obs, os_, oc, od)
        assert np.array_equal(got["s_entries"], want["s_entries"])
        assert np.array_equal(got["c_entries"], want["c_entries"])


# ---- packing, repeats ---------------------------------------------------------------------
def _multiset(lists):
    return {key: sorted(v) for key, v in lists.items()}


def _check_repeats(d, k, p, c, K, nbins, R, tile=TILE, Ih=I, Jw=J):
    shape = (K, Ih, Jw)
    kijc = _kijc(k, p, c, Jw)
    obs = _from(d, kijc, shape, R, tile)
    assert obs.desc.nnz == obs.nnz == k.size
    assert np.array_equal(obs.counts.cpu().numpy(), np.bincount(p, minlength=Ih * Jw))
    mult = np.bincount(k * (Ih * Jw) + p)
    assert obs.stats()["max_repeat"] == mult.max()
    a = _arrays(obs)
    want = rr.expected_lists(k, p, c, a["perm"], tile)
    assert rr.decode_lists(a) == want  # multisets, ascending keys, ties in input order
    _assert_bytes_equal_numpy(obs, rr.pack(k, p, c, K, Ih * Jw, tile, nbins,
                                           rowfmt=obs.desc.rowfmt))
    again = _from(d, kijc, shape, R, tile)
    _assert_same_packing(obs, again)
    sched = _from(d, kijc, shape, R, tile, schedule=True)
    got = rr.decode_lists(_arrays(sched))
    assert _multiset(got[0]) == _multiset(want[0]) and _multiset(got[1]) == _multiset(want[1])
    for f in FIELDS[:7]:
        assert torch.equal(getattr(obs, f), getattr(sched, f)), f
    return obs


@pytest.mark.parametrize("name", ["onebit", "lin4"])
def test_repeated_readings_packing(name):
    """Cells carry 0 - 3 readings with differing codes, the list shuffled."""
    K, nbins = SETS[name][:2]
    d, _ = case(name, 8)
    kt, it, jt, ct = readings(name, 8)
    k, p, c = kt.numpy(), (it * J + jt).numpy(), ct.numpy()
    obs = _check_repeats(d, k, p, c, K, nbins, 8)
    assert obs.stats()["max_repeat"] == M and obs.desc.rowfmt == int(nbins == 2)


def test_pixel_list_longer_than_K():
    """K = 5, four readings of every cell of 40 pixels (a list of 20 > K), one of the rest."""
    K, nbins = 5, 4
    d = make_case(5500, 3, I, J, K, 1.0, nbins, False)
    rs = np.random.RandomState(10)
    kk, pp = np.meshgrid(np.arange(K), np.arange(P), indexing="ij")
    kk, pp = kk.ravel(), pp.ravel()
    heavy = np.isin(pp, rs.permutation(P)[:40])
    k = np.concatenate([kk, np.repeat(kk[heavy], 3)])
    p = np.concatenate([pp, np.repeat(pp[heavy], 3)])
    o = rs.permutation(k.size)
    k, p = k[o], p[o]
    c = rs.randint(0, nbins, k.size)
    obs = _check_repeats(d, k, p, c, K, nbins, 3)
    assert int(obs.s_width.max()) == 20 and int(obs.counts.max()) == 20 > K


def test_bin_list_longer_than_the_tile():
    """One bin read three times at every pixel of a 64-pixel tile: a (tile, bin) list of
    192 > PT = 64 (8 x 8 pixels, one tile)."""
    K, nbins, Ih, Jw = 37, 2, 8, 8
    d = make_case(5600, 3, Ih, Jw, K, 0.2, nbins, False)
    rs = np.random.RandomState(11)
    k0, p0, c0 = rr.dense_readings(d["Y"].numpy(), d["Wx"].numpy())
    keep = k0 != 11
    k = np.concatenate([k0[keep], np.full(192, 11)])
    p = np.concatenate([p0[keep], np.tile(np.arange(64), 3)])
    c = np.concatenate([c0[keep], rs.randint(0, nbins, 192)])
    o = rs.permutation(k.size)
    k, p, c = k[o], p[o], c[o]
    obs = _check_repeats(d, k, p, c, K, nbins, 8, tile=64, Ih=Ih, Jw=Jw)
    assert obs.desc.ntiles == 1 and int(obs.c_width.max()) == 192 > obs.desc.PT
    assert int(obs.c_kmap[0]) == 11


# ---- passes with repeats ------------------------------------------------------------------
def _pass(d, obs, R):
    from quantized_spectrum_cartography_amd import fused
    S = d["S0"].cuda().requires_grad_(True)
    C = d["C0"].cuda().requires_grad_(True)
    v = fused.ProbitNLL.apply(S, C, obs)
    v.backward()
    return v.item(), S.grad.cpu().reshape(R, -1).numpy(), C.grad.cpu().numpy()


def _readings_obs(name, R, schedule=None):
    K, nbins, _, loss = SETS[name]
    d, _ = case(name, R)
    obs = _from(d, readings(name, R), (K, I, J), R, TILE, schedule=schedule, loss=loss)
    assert obs.stats()["max_repeat"] == M and obs.desc.rowfmt == int(nbins == 2)
    return d, obs, loss


@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_passes_with_repeats_vs_summed_oracle(name, R):
    """qsc_spass, qsc_cpass + qsc_cfinish (fused.ProbitNLL.apply) on the stacked readings against
    the fp64 closed form summed over the M dense snapshots."""
    d, obs, _ = _readings_obs(name, R)
    e = errors(_pass(d, obs, R), summed_reference(name, R))
    print("readings pass %s R=%d rowfmt=%d: value %.2e dS %.2e dC %.2e"
          % ((name, R, obs.desc.rowfmt) + e))
    assert e[0] < TOL
    assert e[1] < TOL
    assert e[2] < TOL


LAMBDA = 100.0


def _costs_reference(name, R, C1):
    """The first recorded costs, NLL + lambda_c ||C||_F + lambda_s ||S||_F: the C-step's at
    (S0, C0), the S-step's at (S0, C1), C1 the C after its first step."""
    d, _ = case(name, R)
    reg_s = LAMBDA * float(d["S0"].double().norm())
    c0 = summed_reference(name, R)[0] + LAMBDA * float(d["C0"].double().norm()) + reg_s
    s0 = summed_reference(name, R, C=C1)[0] + LAMBDA * float(C1.double().norm()) + reg_s
    return c0, s0


@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_fused_launch_with_repeats(name, R):
    """qsc_scpass where it is supported: the fused S-step + C-pass launch reproduces the launch
    pair bit for bit on the stacked readings (eager and hipGraph), and the first costs are the
    summed oracle's NLL plus the regulariser.  The fused launch's gradients meet the summed oracle
    through that chain, not directly: the launch pair's gradients are checked against it in
    test_passes_with_repeats_vs_summed_oracle, and S and C after 5 fused iterations are the launch
    pair's bit for bit."""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.fused import PassEngine
    d, obs, loss = _readings_obs(name, R)
    supported = PassEngine(obs, R).scpass_supported()
    kw = dict(S_init=d["S0"], C_init=d["C0"], obs=obs, project_s=False, lambda_c=LAMBDA,
              lambda_s=LAMBDA)
    one = qmc.solve(None, None, d["b"], d["sigma"], max_iter=1, fuse=False, **kw)
    c0, s0 = _costs_reference(name, R, one.C.cpu())
    e = (abs(one.costs_c[0] - c0) / abs(c0), abs(one.costs_s[0] - s0) / abs(s0))
    print("readings costs %s R=%d fused=%d: costs_c %.2e costs_s %.2e" % ((name, R, supported) + e))
    assert e[0] < TOL
    assert e[1] < TOL
    a = qmc.solve(None, None, d["b"], d["sigma"], max_iter=5, fuse=False, **kw)
    assert not a.fused
    for g in (False, True):
        b = qmc.solve(None, None, d["b"], d["sigma"], max_iter=5, fuse=True, use_graph=g, **kw)
        assert b.fused == supported
        assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
        assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
        assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


# ---- solver ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["onebit", "lin4"])
def test_solve_on_repeat_free_readings_is_bit_identical(name):
    from quantized_spectrum_cartography_amd import qmc
    K, nbins = SETS[name][:2]
    R = 8
    d, snaps = case(name, R)
    k, p, c = rr.dense_readings(d["Y"].numpy(), d["Wx"].numpy())
    order = np.random.RandomState(12).permutation(k.size)
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=5, project_s=False)
    for fuse in (False, True):
        for g in (False, True):
            obs = _from(d, _kijc(k, p, c, J, order), (K, I, J), R, TILE, schedule=None)
            a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], tile=TILE, fuse=fuse, use_graph=g,
                          **kw)
            b = qmc.solve(None, None, d["b"], d["sigma"], obs=obs, fuse=fuse, use_graph=g, **kw)
            assert a.fused == b.fused
            assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
            assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
            assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


def test_solve_with_repeats_descends():
    """M = 3 snapshots of a 4-bin map: 20 iterations stay finite and the NLL on the readings
    goes down."""
    from quantized_spectrum_cartography_amd import qmc
    name, R = "lin4", 8
    K = SETS[name][0]
    d, obs, _ = _readings_obs(name, R)
    res = qmc.solve(None, None, d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"], max_iter=20,
                    obs=obs, project_s=False)
    assert res.S.shape == (R, 1, I, J) and res.C.shape == (R, K)
    assert torch.isfinite(res.S).all() and torch.isfinite(res.C).all()
    assert np.isfinite(res.costs_c).all() and np.isfinite(res.costs_s).all()
    nll0 = summed_reference(name, R)[0]
    nll = summed_reference(name, R, S=res.S.cpu(), C=res.C.cpu())[0]
    print("readings solve: NLL %.6g -> %.6g" % (nll0, nll))
    assert nll < nll0


def test_solve_readings_holdout_is_deterministic():
    from quantized_spectrum_cartography_amd import qmc
    name, R = "lin4", 8
    K = SETS[name][0]
    d, _ = case(name, R)
    kijc = readings(name, R)
    n = kijc[0].numel()
    kw = dict(R=R, S_init=d["S0"], C_init=d["C0"], max_iter=20, check_every=5, tile=TILE,
              holdout=0.2, holdout_seed=4, project_s=False)
    a = qmc.solve_readings(*kijc, (K, I, J), d["b"], d["sigma"], **kw)
    b = qmc.solve_readings(*kijc, (K, I, J), d["b"], d["sigma"], **kw)
    assert torch.equal(a.fit_index, b.fit_index) and torch.equal(a.held_index, b.held_index)
    assert torch.equal(torch.sort(torch.cat([a.fit_index, a.held_index])).values,
                       torch.arange(n))
    assert a.obs.nnz + a.obs_holdout.nnz == n and a.obs_holdout.nnz == round(0.2 * n)
    assert torch.equal(a.obs.perm, a.obs_holdout.perm)
    assert torch.equal(a.S, b.S) and torch.equal(a.C, b.C)
    assert a.costs_c == b.costs_c and a.holdout_nll == b.holdout_nll
    assert a.best_iter in (5, 10, 15, 20) and len(a.holdout_nll) >= 1
    assert all(np.isfinite(v) for _, v in a.holdout_nll)
    other = qmc.solve_readings(*kijc, (K, I, J), d["b"], d["sigma"], **dict(kw, holdout_seed=5))
    assert not torch.equal(other.held_index, a.held_index)


# ---- errors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["k", "p", "code"])
def test_bad_readings_are_counted_and_refused(what):
    K, nbins = 37, 2
    d = make_case(5700, 3, I, J, K, F, nbins, False)
    k, p, c = rr.dense_readings(d["Y"].numpy(), d["Wx"].numpy())
    kt, it, jt, ct = _kijc(k, p, c, J)
    if what == "k":
        kt[3] = K
        kt[10] = K
    elif what == "p":
        it[5] = -1  # p = -1 ... -J: outside the grid
    else:
        ct[0] = nbins
        ct[1] = nbins
        ct[2] = -1
    nbad = {"k": 2, "p": 1, "code": 3}[what]
    with pytest.raises(ValueError, match=r"^%d of %d readings" % (nbad, k.size)):
        _from(d, (kt, it, jt, ct), (K, I, J), 8, TILE)
