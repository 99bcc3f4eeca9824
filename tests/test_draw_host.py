"""CPU: what tests/test_gpu_draw.py rests on -- the generator's definition, the reference draw's
rules, the conditions the GPU file sets on its inputs (checked here on the reference's own draws),
the argument checks of Observations.resample and fits.bootstrap, and the Welford helper."""
import numpy as np
import pytest
import torch

import draw_ref as dr
import test_gpu_check as tgc

SEED = 11


def test_philox_known_answer_and_u_range():
    got = tuple(int(w) for w in dr.philox4x32_10(0, 0, 0, 0, 0, 0))
    assert got == dr.KAT_ZERO
    # a second published vector: counter and key all ones
    got = tuple(int(w) for w in dr.philox4x32_10(*(4 * [0xFFFFFFFF]), 0xFFFFFFFF, 0xFFFFFFFF))
    assert got == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    # u = (n + 1/2) 2^-24 lies strictly inside (0, 1) for every 24-bit n (fp64 holds it exactly)
    for n in (0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 24 - 1):
        u = (n + 0.5) * 2.0 ** -24
        assert 0.0 < u < 1.0 and u * 2.0 ** 25 == 2 * n + 1
    # ... but n + 1/2 has 25 bits: as an fp32 number the largest u rounds to 1, which is why the
    # kernel forms thr = fma(n, Z 2^-24, Z 2^-25) (one rounding of u Z) and never u itself
    assert np.float32((2 ** 24 - 1 + 0.5) * 2.0 ** -24) == np.float32(1.0)
    g = np.random.default_rng(0)
    k, p = g.integers(0, 5000, 4000), g.integers(0, 2 ** 20, 4000)
    u = dr.uniform(k, p, np.zeros(4000, np.int64), 3, SEED)
    assert (u > 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * 4000)


def test_u_is_a_function_of_the_key_only():
    g = np.random.default_rng(1)
    k, p = g.integers(0, 7, 300), g.integers(0, 9, 300)     # 63 cells: many repeats
    j = dr.occurrence(k, p, 9)
    cell = k * 9 + p
    for c in np.unique(cell):
        assert np.array_equal(j[cell == c], np.arange((cell == c).sum()))
    u = dr.uniform(k, p, j, 2, SEED)
    o = g.permutation(300)
    j2 = dr.occurrence(k[o], p[o], 9)
    u2 = dr.uniform(k[o], p[o], j2, 2, SEED)
    key = lambda kk, pp, jj: np.lexsort((jj, pp, kk))
    assert np.array_equal(u[key(k, p, j)], u2[key(k[o], p[o], j2)])
    # another seed, replicate or occurrence: other numbers
    assert not np.array_equal(u, dr.uniform(k, p, j, 2, SEED + 1))
    assert not np.array_equal(u, dr.uniform(k, p, j, 3, SEED))
    assert not np.array_equal(u, dr.uniform(k, p, j + 1, 2, SEED))
    assert dr.key_of(-1) == (0xFFFFFFFF, 0xFFFFFFFF) and dr.key_of(2 ** 32 + 5) == (5, 1)


@pytest.mark.parametrize("name", list(tgc.CASES))
def test_reference_draw_rules_and_the_window_condition(name):
    """The reference never draws a bin of probability 0, keeps invalid readings, and on each of the
    seven cases at most 1e-3 of the readings lie inside the comparison window."""
    d = tgc.problem(name)
    r = dr.resample_readings(d["S"], d["C"], d["k"], d["p"], d["y"], d["model"], SEED, 0)
    ok = ~r["invalid"]
    n = len(d["k"])
    Pd = r["Pb"][r["code"], np.arange(n)]
    assert (Pd[ok] > 0).all()
    assert np.array_equal(r["code"][~ok], d["y"][~ok])
    assert (r["code"] >= 0).all() and (r["code"] < len(d["b"]) - 1).all()
    inside = (r["margin"] <= dr.WINDOW).sum()
    print(name, "readings", n, "inside the window", int(inside), "invalid", int((~ok).sum()))
    assert inside <= 1e-3 * n
    if "underflow" in d["planted"]:
        # every reading of the planted pixel sits where all bins but the last have P == 0
        at = d["p"] == d["planted"]["underflow"]
        assert (r["Pb"][:-1, at] == 0).all() and (r["code"][at] == len(d["b"]) - 2).all()
    if "negative" in d["planted"]:
        assert r["invalid"].any() and set(d["p"][r["invalid"]]) == {d["planted"]["negative"]}
    if d["packing"] == "readings":
        assert r["j"].max() == 2


def test_reference_draws_meet_the_distribution_conditions():
    """Counts per bin within 5 binomial standard deviations of sum P_b, and section 7u's null
    moments of z_fit and z_shift, on the reference's draws at the GPU test's seed."""
    import check_ref as cr
    d = tgc.null_problem()
    P = d["P"]
    Yn, r = dr.resample_dense(d["S"], d["C"], d["Y"], d["Wx"], d["model"], SEED, 0)
    for b in range(2):
        pb = r["Pb"][b]
        dev = abs((r["code"] == b).sum() - pb.sum()) / np.sqrt((pb * (1 - pb)).sum())
        print("bin", b, "deviation", dev)
        assert dev <= 5.0
    st = cr.stats(d["S"], d["C"], r["k"], r["p"], r["code"], *d["model"], fitted=False)
    assert st["flags"].max() == 0
    zf, zs, _ = cr.zscores(st)
    for z in (zf, zs):
        mean, var, kappa = tgc.moments(z)
        assert abs(mean) <= 5.0 / np.sqrt(P)
        assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / P) * kappa


def test_reference_bootstrap_meets_the_conditions_of_the_gpu_test():
    """On draw_ref.boot_problem(), with refit = ("S",): the median over the pixels with >= 40
    readings of std_S / the Cramer-Rao bound lies in [0.7, 1.5], p_fit lies in [0.05, 0.95] for the
    data drawn at the model's noise and is 1 / (n + 1) for the data drawn at twice that."""
    import info_ref as ir
    c, d = dr.BOOT, dr.boot_problem()
    n = c["n"]
    ref = dr.bootstrap(d["S"], d["C"], d["Y"], d["Wx"], d["model"], n=n, seed=c["draw_seed"],
                       refit_=("S",))
    J = ir.blocks(d["S"], d["C"], d["Y"], d["Wx"], *d["model"], kind="expected")
    many = d["Wx"].sum(axis=0) >= 40
    bound = ir.stds(J, d["C"], 0.0, map_std=False)[0]
    ratio = float(np.median((ref["std_S"] / bound)[:, many]))
    print("pixels", int(many.sum()), "median ratio", ratio, "p_fit", ref["p_fit"])
    assert many.sum() > 100 and 0.7 <= ratio <= 1.5
    assert 0.05 <= ref["p_fit"] <= 0.95
    noisy = dr.bootstrap(d["S"], d["C"], d["Y2"], d["Wx"], d["model"], n=n, seed=c["draw_seed"],
                         refit_=("S",))
    assert noisy["p_fit"] == 1.0 / (n + 1)


def test_bootstrap_and_resample_arguments_are_checked_before_any_device_call(monkeypatch):
    from quantized_spectrum_cartography_amd import _lib, fits, qmc
    from quantized_spectrum_cartography_amd.obs import Observations

    def boom(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    assert qmc.bootstrap is fits.bootstrap
    ok = dict(n=8, refit=("C", "S"), rounds=1, ridge_s=0.0, ridge_c=0.0, max_steps=30,
              loss="probit")
    assert fits.check_bootstrap(**ok) == (8, ("C", "S"), 1)
    assert fits.check_bootstrap(**dict(ok, refit="S"))[1] == ("S",)
    for bad in (dict(n=1), dict(refit=()), dict(refit=("S", "noise")), dict(ridge_s=-1.0),
                dict(ridge_c=float("nan")), dict(loss="squared"), dict(rounds=0),
                dict(max_steps=0)):
        with pytest.raises(ValueError):
            fits.check_bootstrap(**dict(ok, **bad))
    obs = Observations.__new__(Observations)
    obs.loss, obs.K, obs.I, obs.J, obs.P = "probit", 5, 4, 3, 12
    S, C = torch.zeros(2, 1, 4, 3), torch.zeros(2, 5)
    assert Observations.check_resample("probit", 5, 4, 3, S, C, 2 ** 64 - 1, 0) == (2, -1)
    assert Observations.check_resample("logit", 5, 4, 3, S[:, 0], C) == (2, 0)
    for s, c in ((torch.zeros(2, 1, 3, 4), C), (S, torch.zeros(3, 5)), (S, torch.zeros(2, 6)),
                 (torch.zeros(17, 1, 4, 3), torch.zeros(17, 5)), (torch.zeros(12), C)):
        with pytest.raises(ValueError):
            obs.resample(s, c)
        with pytest.raises(ValueError):
            fits.bootstrap(obs, s, c, n=4)
    with pytest.raises(ValueError):
        obs.resample(S, C, replicate=-1)
    with pytest.raises(ValueError):
        obs.resample(S, C, seed=2 ** 64)
    with pytest.raises(ValueError):
        fits.bootstrap(obs, S, C, n=1)
    obs.loss = "squared"
    with pytest.raises(ValueError):
        obs.resample(S, C)
    with pytest.raises(ValueError):
        fits.bootstrap(obs, S, C)


def test_welford_and_the_scale_gauge_against_numpy():
    from quantized_spectrum_cartography_amd import fits
    g = np.random.default_rng(5)
    x = 1e3 + g.standard_normal((9, 4, 7))        # a large mean: the two-pass form's weak spot
    w = fits.Welford()
    for s in x:
        w.add(torch.from_numpy(s).float())
    x32 = x.astype(np.float32).astype(np.float64)
    assert w.count == 9 and w.mean.dtype == torch.float64
    assert np.allclose(w.mean.numpy(), x32.mean(axis=0), rtol=1e-14)
    assert np.allclose(w.std().numpy(), x32.std(axis=0, ddof=1), rtol=1e-11)
    S, C = g.random((3, 10)), g.random((3, 6))
    C[2] = 0.0
    norms = np.array([2.0, 0.5, 1.0])
    Sg, Cg = fits.scale_gauge(torch.from_numpy(S), torch.from_numpy(C), torch.from_numpy(norms))
    Sr, Cr = dr.scale_gauge(S, C, norms)
    assert np.allclose(Sg.numpy(), Sr, rtol=1e-14) and np.allclose(Cg.numpy(), Cr, rtol=1e-14)
    assert np.allclose(np.linalg.norm(Cr[:2], axis=1), norms[:2])
    assert np.allclose(Cr.T @ Sr, C.T @ S, rtol=1e-12)
