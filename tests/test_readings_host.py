"""CPU: the readings front door (Observations.from_readings, qmc.solve(obs=), qmc.solve_readings)
as far as it runs without a device, and the inputs of tests/test_gpu_readings.py.

1. the numpy packer of tests/readings_ref.py, given the readings of a dense (Y, Wx), produces a
   packing that the independent decode of tests/test_gpu_packing.py (written from include/qsc.h)
   accepts against the dense codes -- so the GPU test may compare bytes with it;
2. host-side argument errors are raised before any library call;
3. split_readings is a seeded partition;
4. the snapshot data sets of the GPU pass tests are conditioned as the pass matrix's are: the
   reference's own fp32 formulation, summed over the snapshots, stays within 3e-6 of the summed
   fp64 closed form, so the 1e-5 bound is left to the kernels.  A set that misses gets another
   seed in _RESEED; the bound stays;
5. the inputs of tests/test_gpu_readings_fits.py (confidence, fit_S, fit_C, fit_S_smooth on
   repeated readings): the dense stacked problems equal the sums over the snapshots, and the
   numpy references converge on them (see the end of this file)."""
import types

import numpy as np
import pytest
import torch

import cfit_ref as cr
import info_ref as ir
import logit_ref as lr
import readings_fit_ref as rf
import readings_ref as rr
import sfit_ref as sr
from oracle import explicit, reference_ops as ro
from test_pass_matrix_host import errors, make_case

I, J, TILE = 9, 15, 64
P = I * J
M = 3  # snapshots = the largest number of readings of one cell
F = 0.3
RANKS = (3, 8, 16)
# name -> (K, bins, log model, loss)
SETS = {"onebit": (37, 2, False, "probit"), "lin4": (70, 4, False, "probit"),
        "log4": (37, 4, True, "probit"), "logit-onebit": (37, 2, False, "logit"),
        "logit-lin4": (70, 4, False, "logit")}
_RESEED = {}
_CASES, _REFS = {}, {}


def case(name, R):
    """Problem `name` at rank R: d (model, S0, C0 as make_case gives them) and M dense snapshots
    [(Y_m, Wx_m)], each with at most one reading per cell; snapshot m > 0 takes the codes and the
    mask of a later draw (any codes in range are a valid observation of the same model)."""
    key = (name, R)
    if key not in _CASES:
        K, nbins, log_model, _ = SETS[name]
        seed = 31000 + 1000 * sorted(SETS).index(name) + 10 * R + 100000 * _RESEED.get(key, 0)
        d = make_case(seed, R, I, J, K, F, nbins, log_model)
        snaps = [(d["Y"], d["Wx"])]
        for m in range(1, M):
            e = make_case(seed + m, R, I, J, K, F, nbins, log_model)
            snaps.append((e["Y"], e["Wx"]))
        _CASES[key] = (d, snaps)
    return _CASES[key]


def readings(name, R, shuffle_seed=5):
    """(k, i, j, code) int64 tensors of the case's stacked snapshots, shuffled."""
    _, snaps = case(name, R)
    k, p, c = rr.stack_readings([(Y.numpy(), W.numpy()) for Y, W in snaps])
    o = np.random.RandomState(shuffle_seed).permutation(k.size)
    k, p, c = k[o], p[o], c[o]
    return tuple(torch.from_numpy(a) for a in (k, p // J, p % J, c))


def _nll_grad(loss):
    return lr.nll_grad if loss == "logit" else explicit.nll_grad


def summed_reference(name, R, S=None, C=None):
    """(value, dS (R,P), dC (R,K)): the fp64 closed form summed over the snapshots (at the
    case's S0, C0 unless given)."""
    d, snaps = case(name, R)
    K, loss = SETS[name][0], SETS[name][3]
    key = (name, R)
    if S is None and C is None and key in _REFS:
        return _REFS[key]
    Sn = (d["S0"] if S is None else S).reshape(R, P).numpy().astype(np.float32)
    Cn = (d["C0"] if C is None else C).numpy().astype(np.float32)
    tot = None
    for Y, W in snaps:
        r = _nll_grad(loss)(Sn, Cn, Y.reshape(K, P).numpy(), W.reshape(K, P).numpy(),
                            d["b"].numpy(), d["sigma"], d["offset"], d["log_model"])
        tot = r if tot is None else tuple(a + b for a, b in zip(tot, r))
    if S is None and C is None:
        _REFS[key] = tot
    return tot


def summed_fp32(name, R):
    d, snaps = case(name, R)
    loss = SETS[name][3]
    S = d["S0"].clone().requires_grad_(True)
    C = d["C0"].clone().requires_grad_(True)
    f = lr.masked_nll if loss == "logit" else ro.masked_nll
    v = sum(f(S, C, Y, W, d["b"], d["sigma"], d["offset"], d["log_model"]) for Y, W in snaps)
    v.backward()
    return v.item(), S.grad.reshape(R, -1).numpy(), C.grad.numpy()


@pytest.mark.parametrize("R", RANKS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_snapshot_sets_are_well_conditioned(name, R):
    e = errors(summed_fp32(name, R), summed_reference(name, R))
    print("conditioning %s R=%d: value %.2e dS %.2e dC %.2e" % ((name, R) + e))
    assert max(e) < 3e-6


def test_snapshot_sets_repeat_cells():
    """The stacked snapshots read cells 0 to M times, with differing codes on some cell."""
    for name in SETS:
        d, snaps = case(name, 3)
        K = SETS[name][0]
        mult = sum(W.reshape(K, P) for _, W in snaps).numpy()
        assert set(np.unique(mult)) == set(range(M + 1))
        Y0, Y1 = snaps[0][0].reshape(K, P).numpy(), snaps[1][0].reshape(K, P).numpy()
        both = (snaps[0][1].reshape(K, P).numpy() != 0) & (snaps[1][1].reshape(K, P).numpy() != 0)
        assert (Y0[both] != Y1[both]).any()


def _fake_obs(a, codes):
    """The attributes tests/test_gpu_packing.check_packing reads, from a numpy packing."""
    d = types.SimpleNamespace(**a["desc"])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    signed = np.int32 if d.wide else np.int16
    return types.SimpleNamespace(
        desc=d, K=d.K, P=d.P, codes=t(codes), counts=t(a["counts"]), perm=t(a["perm"]),
        s_width=t(a["s_width"]), s_off=t(a["s_off"]), c_width=t(a["c_width"]), c_off=t(a["c_off"]),
        c_kmap=t(a["c_kmap"]), s_entries=t(a["s_entries"].view(signed)),
        c_entries=t(a["c_entries"].view(signed)))


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("K,nbins,rowfmt,tile", [(37, 2, 1, 64), (37, 2, 0, 64), (70, 4, 0, 64),
                                                 (70, 4, 0, 128), (37, 16, 0, 64)])
def test_numpy_packer_reproduces_the_dense_packing(K, nbins, rowfmt, tile, shuffle):
    """Repeat-free input: the decode of test_gpu_packing.py (descriptor, pixel order, both
    formats' lists in ascending order with pads last, c_kmap, the tail) accepts the numpy
    packing against the dense codes, whatever the order of the list."""
    from test_gpu_packing import check_packing
    d = make_case(4100 + K + nbins, 3, I, J, K, F, nbins, False)
    Y, W = d["Y"].reshape(K, P).numpy(), d["Wx"].reshape(K, P).numpy()
    k, p, c = rr.dense_readings(Y, W)
    if shuffle:
        o = np.random.RandomState(1).permutation(k.size)
        k, p, c = k[o], p[o], c[o]
    a = rr.pack(k, p, c, K, P, tile, nbins, rowfmt=rowfmt)
    assert a["desc"]["wide"] == int(nbins > 15)
    codes = np.where(W != 0, Y, 0xFF).astype(np.uint8)
    check_packing(_fake_obs(a, codes), natural_order=True)
    # and the decode of readings_ref itself agrees with its own expectation
    got = rr.decode_lists(a)
    assert got == rr.expected_lists(k, p, c, a["perm"], tile)


def test_numpy_packer_keeps_equal_keys_in_input_order():
    k = np.array([2, 0, 2, 2, 0])
    p = np.array([5, 5, 5, 5, 5])
    c = np.array([1, 0, 0, 1, 1])
    a = rr.pack(k, p, c, 3, 40, 64, 2)
    per_pixel, per_bin = rr.decode_lists(a)
    assert per_pixel == {5: [(0, 0), (0, 1), (2, 1), (2, 0), (2, 1)]}
    assert per_bin == {(0, 0): [(0, 0), (0, 1)], (0, 2): [(0, 1), (0, 0), (0, 1)]}
    assert a["s_width"].tolist() == [8, 0] and a["desc"]["nnz"] == 5


# ---- errors raised on the host, before any library call -------------------------------------
def _no_library(monkeypatch):
    from quantized_spectrum_cartography_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "lib", boom)


_B = [-1e5, 0.5, 1e5]


def _good():
    return [torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]),
            torch.tensor([0, 1, 0])]


@pytest.mark.parametrize("what", ["lengths", "float", "empty", "tile", "shape"])
def test_from_readings_host_errors(monkeypatch, what):
    from quantized_spectrum_cartography_amd.obs import Observations
    _no_library(monkeypatch)
    a, kw, shape = _good(), {}, (4, 3, 3)
    if what == "lengths":
        a[3] = torch.tensor([0, 1])
    elif what == "float":
        a[1] = torch.tensor([0.0, 1.0, 2.0])
    elif what == "empty":
        a = [torch.zeros(0, dtype=torch.int64)] * 4
    elif what == "tile":
        kw["tile"] = 96
    else:
        shape = (4, 3)
    with pytest.raises(ValueError):
        Observations.from_readings(*a, shape, _B, 1.0, **kw)
    with pytest.raises(ValueError):
        from quantized_spectrum_cartography_amd import qmc
        qmc.solve_readings(*a, shape, _B, 1.0, R=2, **kw)


def test_solve_without_y_needs_obs(monkeypatch):
    from quantized_spectrum_cartography_amd import qmc
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="obs"):
        qmc.solve(None, None, _B, 1.0, R=2)


def test_split_readings_is_a_seeded_partition():
    from quantized_spectrum_cartography_amd import qmc
    fit, held = qmc.split_readings(1000, 0.2, seed=3)
    assert held.numel() == 200 and fit.numel() == 800
    assert torch.equal(torch.sort(torch.cat([fit, held])).values, torch.arange(1000))
    assert (fit[1:] > fit[:-1]).all() and (held[1:] > held[:-1]).all()
    again = qmc.split_readings(1000, 0.2, seed=3)
    assert torch.equal(fit, again[0]) and torch.equal(held, again[1])
    other = qmc.split_readings(1000, 0.2, seed=4)
    assert not torch.equal(held, other[1])
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            qmc.split_readings(10, bad)


# ---- the second-order consumers' inputs (tests/test_gpu_readings_fits.py) ------------------
# 5. the stacked-bin / stacked-pixel dense problems of tests/readings_fit_ref.py are, term for
#    term, the sums over the snapshots; and the existing numpy references, unchanged, converge on
#    them within their step limits in fp32 and in fp64 -- what makes `unconverged == 0` in the GPU
#    tests a condition the references alone meet (the rule of tests/test_sfit_host.py).
@pytest.mark.parametrize("name", rf.CASES)
def test_stacked_problems_sum_the_snapshots(name):
    d, snaps = rf.problem(name)
    R, K = d["R"], d["K"]
    mult = sum(W for _, W in rf.snapshots(name, "s"))
    assert set(np.unique(mult)) == set(range(rf.M + 1)) and (mult[:, 0] == 0).all()
    kind = sr.default_kind(d["log_model"])
    S = 0.8 * d["S"].reshape(R, P).double().numpy()
    f, g, Jb = sr.evaluate(S, kind=kind, **rf.stacked_bins(name))
    parts = [sr.evaluate(S, kind=kind, **rf.snapshot_model(name, "s", m)) for m in range(rf.M)]
    for got, want in zip((f, g, Jb), (sum(q[a] for q in parts) for a in range(3))):
        assert got.shape == want.shape and np.allclose(got, want, rtol=1e-12, atol=1e-12)
    C = 0.8 * d["C"].double().numpy()
    f, g, Jb = cr.evaluate(C, kind=kind, **rf.stacked_pixels(name))
    parts = [cr.evaluate(C, kind=kind, **rf.snapshot_model(name, "c", m)) for m in range(rf.M)]
    for got, want in zip((f, g, Jb), (sum(q[a] for q in parts) for a in range(3))):
        assert got.shape == want.shape and np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert f.shape == (K,) and f[0] == 0  # bin 0 is unobserved on the C side


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_sfit_reference_converges_on_the_stacked_bins(name, ridge):
    d, _ = rf.problem(name)
    m = rf.stacked_bins(name)
    obsd = sr.observed_pixels(m["Wx"])
    assert int((~obsd).sum()) == 1 and not obsd[0]
    S0 = (np.ones if d["log_model"] else np.zeros)((d["R"], P))
    for dtype in (np.float64, np.float32):
        r = sr.fit(S0, ridge=ridge, max_steps=30, dtype=dtype, **m)
        print(name, ridge, dtype.__name__, "sfit steps max", int(r["steps"].max()))
        assert r["converged"].all() and r["identified"].all()
    mn = sr.minimise_fp64(S0, ridge=ridge, **m)
    g = sr.gradient_fp64(mn["S"], ridge=ridge, project=d["log_model"], **m)
    assert np.abs(g[:, obsd]).max() <= 1e-9


@pytest.mark.parametrize("ridge", rf.RIDGES)
@pytest.mark.parametrize("name", rf.CASES)
def test_cfit_reference_converges_on_the_stacked_pixels(name, ridge):
    d, _ = rf.problem(name)
    m = rf.stacked_pixels(name)
    o = cr.observed_bins(m["Wx"])
    assert int((~o).sum()) == 1 and not o[0]
    C0 = cr.default_start(d)
    for dtype in (np.float64, np.float32):
        r = cr.fit(C0, ridge=ridge, max_steps=cr.MAX_STEPS, dtype=dtype, **m)
        print(name, ridge, dtype.__name__, "cfit steps max", int(r["steps"].max()))
        assert r["converged"].all() and r["identified"].all()
    t = cr.fit(C0, ridge=ridge, max_steps=300, tol=1e-12, dtype=np.float64, **m)
    assert t["converged"][o].all()


@pytest.mark.parametrize("name", rf.CASES)
def test_information_blocks_of_the_stacked_bins_are_positive_definite_with_a_ridge(name):
    d, _ = rf.problem(name)
    m = rf.stacked_bins(name)
    for kind in ("expected", "observed"):
        Jr = ir.blocks(d["S"].reshape(d["R"], P).double().numpy(), m["C"], m["Y"], m["Wx"], m["b"],
                       m["sigma"], m["offset"], m["log_model"], m["loss"], kind)
        for ridge in rf.RIDGES:
            assert ir.stds(Jr, d["C"].double().numpy(), ridge, map_std=False)[2] == 0
