"""CPU: the range arithmetic of Observations.split / folds, the argument checks of select / split /
folds / cross_validate (raised before any device call: there is no GPU here), the inputs of
tests/test_gpu_select.py and the properties of the reference (tests/select_ref.py) that the GPU
tests rely on: fold sizes at the fixed seed, and the ranking of two ridges by held-out NLL in fp64
(tests/sfit_ref.py)."""
import numpy as np
import pytest
import torch

import draw_ref as dr
import select_ref as sl
import sfit_ref as sr
from quantized_spectrum_cartography_amd import fits, qmc
from quantized_spectrum_cartography_amd.obs import Observations

RIDGES = (1e-2, 1e3)   # cross_validate must rank the first below the second in every fold
CV_FOLDS, CV_SEED = 5, 9


@pytest.mark.parametrize("n", [2, 3, 5, 7, 65536])
def test_fold_ranges_tile_the_range(n):
    r = [Observations.fold_range(f, n) for f in range(n)]
    assert r == [sl.fold_range(f, n) for f in range(n)]
    assert r[0][0] == 0 and r[-1][1] == 1 << 24
    assert all(a[1] == b[0] for a, b in zip(r, r[1:]))   # no gap, no overlap
    assert all(lo < hi for lo, hi in r)                   # none empty (n <= 2^16)
    widths = {hi - lo for lo, hi in r}
    assert max(widths) - min(widths) <= 1


def test_frac_range_rounds_and_clamps():
    f = Observations.frac_range
    assert f(0.5) == 1 << 23 and f(0.1) == round(0.1 * 2 ** 24) == sl.frac_range(0.1)
    assert f(1e-12) == 1 and f(1 - 1e-12) == (1 << 24) - 1
    assert f(2.0 ** -24) == 1 and f(1.5 * 2.0 ** -24) == 2
    for x in (0.01, 0.2, 0.25, 0.9):
        assert f(x) == sl.frac_range(x) and abs(f(x) / 2 ** 24 - x) <= 2.0 ** -25


def test_known_answer_and_stream():
    # the generator is draw_ref's (known answer checked there); the rule's stream is word 3 = 2^31
    assert tuple(int(v) for v in dr.philox4x32_10(0, 0, 0, 0, 0, 0)) == dr.KAT_ZERO
    k, p, j = np.arange(50), np.arange(50) * 3, np.arange(50) % 3
    assert not np.array_equal(sl.u24(k, p, j, 7), dr.n24(k, p, j, 0, 7))
    assert np.array_equal(sl.u24(k, p, j, 7), dr.n24(k, p, j, 0x80000000, 7))
    assert sl.u24(k, p, j, 7).max() < 1 << 24


def _fake(K=4, I=3, J=5, loss="probit"):
    """An Observations with a shape and no device state: any device call would fail here."""
    o = Observations.__new__(Observations)
    o.K, o.I, o.J, o.P, o.loss = K, I, J, I * J, loss
    return o


def test_select_checks_raise_before_any_device_call():
    o = _fake()
    ok_p, ok_b = torch.ones(3, 5, dtype=torch.bool), torch.ones(4, dtype=torch.bool)
    Observations.check_select(4, 3, 5, ok_p, ok_b, "keep")
    Observations.check_select(4, 3, 5, None, None, "fresh")
    for kw in (dict(pixels=torch.ones(5, 3, dtype=torch.bool)),
               dict(pixels=torch.ones(15, dtype=torch.bool)),
               dict(pixels=torch.ones(3, 5)),
               dict(pixels=np.ones((3, 5), bool)),
               dict(bins=torch.ones(5, dtype=torch.bool)),
               dict(bins=torch.ones(4, dtype=torch.uint8)),
               dict(bins=ok_b, perm="sorted")):
        with pytest.raises(ValueError):
            o.select(**kw)


def test_split_and_folds_checks_raise_before_any_device_call():
    o = _fake()
    for frac in (0.0, 1.0, -0.1, 1.5, float("nan"), None, "half"):
        with pytest.raises(ValueError):
            o.split(frac)
    for seed in (2 ** 64, -2 ** 63 - 1, 1.5, None):
        with pytest.raises(ValueError):
            o.split(0.5, seed=seed)
        with pytest.raises(ValueError):
            o.folds(5, seed=seed)
    with pytest.raises(ValueError):
        o.split(0.5, perm="other")
    for n in (1, 0, -3, 65537, 2.0, None, True):
        with pytest.raises(ValueError):
            o.folds(n)
    # the accepted ends: seeds map to resample's signed 64-bit value
    assert Observations.check_split(frac=0.5, seed=2 ** 64 - 1) == -1
    assert Observations.check_split(seed=-2 ** 63, n=2) == -2 ** 63
    assert Observations.check_split(seed=0, n=65536) == 0


def test_cross_validate_checks_raise_before_any_device_call():
    assert qmc.cross_validate is fits.cross_validate
    fit = lambda tr: None  # noqa: E731
    with pytest.raises(ValueError, match="squared"):
        fits.cross_validate(_fake(loss="squared"), fit)
    with pytest.raises(ValueError):
        fits.cross_validate(_fake(), "not callable")
    for n in (1, 65537, 2.5):
        with pytest.raises(ValueError):
            fits.cross_validate(_fake(), fit, folds=n)
    with pytest.raises(ValueError):
        fits.cross_validate(_fake(), fit, seed=2 ** 64)


def test_solve_with_obs_and_holdout_checks_the_fraction_first():
    o = _fake()
    with pytest.raises(ValueError, match="fraction"):
        qmc.solve(None, None, [0.0, 1.0, 2.0], 0.5, R=2, obs=o, holdout=1.5)


def test_problem_lists_are_what_the_gpu_tests_assume():
    for name, (K, I, J) in sl.SHAPES.items():
        for nbins in (2, 4):
            d = sl.problem(name, nbins, 1)
            cell = d["k"] * d["P"] + d["p"]
            assert np.unique(cell).size == cell.size and d["c"].max() == nbins - 1
            d5 = sl.problem(name, nbins, 5)
            assert np.bincount(dr.occurrence(d5["k"], d5["p"], d5["P"])).size == 5
    assert sl.SHAPES["small"][1] * sl.SHAPES["small"][2] < 64
    assert (sl.SHAPES["ragged"][1] * sl.SHAPES["ragged"][2]) % 16 != 0 and sl.SHAPES["ragged"][0] > 64
    assert (sl.SHAPES["vec"][1] * sl.SHAPES["vec"][2]) % 16 == 0


def test_fold_sizes_at_the_fixed_seed():
    """483 x 70, 5 folds: every fold's size within 5 binomial standard deviations of n / 5."""
    for rep in (1, 5):
        d = sl.problem("ragged", 2, rep)
        n = d["k"].size
        fold = sl.fold_of(d["k"], d["p"], d["P"], 5, sl.FOLD_SEED)
        sizes = np.bincount(fold, minlength=5)
        assert sizes.sum() == n and fold.min() == 0 and fold.max() == 4
        sd = np.sqrt(n * 0.2 * 0.8)
        print("fold sizes", sizes.tolist(), "n/5", n / 5, "sd", sd)
        assert np.all(np.abs(sizes - n / 5) <= 5 * sd)
        # keep() with a fold's range and with its complement says the same
        lo, hi = sl.fold_range(2, 5)
        t = sl.keep(d["k"], d["p"], d["P"], sl.FOLD_SEED, lo, hi)
        assert np.array_equal(t, fold == 2)
        assert np.array_equal(sl.keep(d["k"], d["p"], d["P"], sl.FOLD_SEED, lo, hi, True), ~t)


def cv_reference(ridge):
    """Per-fold held-out NLL per reading of the fp64 Newton fit of S at the true C on
    draw_ref.boot_problem(), folds by the reference rule."""
    c, d = dr.BOOT, dr.boot_problem()
    b, sigma = d["b"], c["sigma"]
    k, p = np.nonzero(d["Wx"])
    fold = sl.fold_of(k, p, d["P"], CV_FOLDS, CV_SEED, j=np.zeros(k.size, np.int64))
    out = []
    for f in range(CV_FOLDS):
        tr, te = np.zeros_like(d["Wx"]), np.zeros_like(d["Wx"])
        tr[k[fold != f], p[fold != f]] = True
        te[k[fold == f], p[fold == f]] = True
        S = sr.fit(np.zeros_like(d["S"]), d["C"], d["Y"], tr, b, sigma, ridge=ridge)["S"]
        out.append(dr.nll(S, d["C"], d["Y"], te, d["model"]) / int(te.sum()))
    return out


_CV = {}


def cv_reference_cached(ridge):
    if ridge not in _CV:
        _CV[ridge] = cv_reference(ridge)
    return _CV[ridge]


def test_reference_ranks_the_two_ridges_in_every_fold():
    small, big = (cv_reference_cached(r) for r in RIDGES)
    print("fp64 held-out NLL per reading: ridge %g" % RIDGES[0], small, "ridge %g" % RIDGES[1], big)
    assert all(a < b for a, b in zip(small, big))
