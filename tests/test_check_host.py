"""CPU: the fp64 reference of the per-position fit checks (tests/check_ref.py) against its own
defining identities -- the null moments per entry by enumeration of the bins, the score as the
derivative of the NLL in the shift, I* as the Schur complement of the (R + 1) x (R + 1) expected
information assembled from tests/info_ref.py -- the thresholds of CheckResult.flagged, and the
argument checks of qmc.check_fit, which need no device."""
import types

import numpy as np
import pytest
import torch

import check_ref as cr
import info_ref as ir

K, I, J, R = 9, 3, 5, 2
P = I * J
RIDGE = 1e-3

# (bin boundaries, sigma, offset, log_model, loss)
MODELS = {
    "onebit": ([0.0, 0.6, 2.0], 0.4, 0.0, False, "probit"),
    "log4": ([-23.025850296020508, -1.0, -0.4, 0.1, 30.0], 0.6, 1e-3, True, "probit"),
    "logit3": ([0.0, 0.4, 0.9, 2.0], 0.3, 0.0, False, "logit"),
    # (the log model does not clamp its outer edges: they are set wide, so that the bins carry all
    # of the probability and the null moments are exact)
    "logit_log4": ([-23.025850296020508, -1.0, -0.4, 0.1, 30.0], 0.5, 1e-3, True, "logit"),
}


def _problem(name, seed=7):
    b, sigma, offset, log_model, loss = MODELS[name]
    g = np.random.default_rng(seed)
    S = 0.2 + 0.8 * g.random((R, P))
    C = 0.1 + 0.9 * g.random((R, K))
    Y = g.integers(0, len(b) - 1, (K, P))
    Wx = (g.random((K, P)) < 0.8).astype(np.float64)
    Wx[:, 0] = 0  # an unobserved pixel
    return dict(S=S, C=C, Y=Y, Wx=Wx, model=(b, sigma, offset, log_model, loss))


@pytest.mark.parametrize("name", list(MODELS))
def test_per_entry_null_moments_by_enumerating_the_bins(name):
    """sum_b P_b (l_b - H) = 0, sum_b P_b (l_b - H)^2 = var, sum_b P_b g_x,b = 0 and
    sum_b P_b g_x,b^2 = h_x: the exact null mean and variance of D and u, entry by entry."""
    model = MODELS[name]
    nb = len(model[0]) - 1
    T = np.linspace(0.05, 1.6, 41)
    Pb = ir.bin_probabilities(T[None, :], model[0], model[1], model[2], model[3], model[4])[:, 0]
    assert np.allclose(Pb.sum(0), 1.0, atol=1e-12)
    m1 = m2 = s1 = s2 = 0.0
    for c in range(nb):
        et = cr.entry_terms(T, np.full(T.shape, c), *model)
        assert not et["sat"].any() and not et["neg"].any()
        m1 = m1 + Pb[c] * et["dl"]
        m2 = m2 + Pb[c] * et["dl"] ** 2
        s1 = s1 + Pb[c] * et["gx"]
        s2 = s2 + Pb[c] * et["gx"] ** 2
    et = cr.entry_terms(T, np.zeros(T.shape, int), *model)
    assert np.max(np.abs(m1)) <= 1e-12
    assert np.max(np.abs(m2 - et["var"])) <= 1e-12 * max(1.0, np.max(et["var"]))
    assert np.max(np.abs(s1)) <= 1e-10 * max(1.0, np.max(np.sqrt(et["hx"])))
    assert np.max(np.abs(s2 - et["hx"]) / et["hx"]) <= 1e-9


@pytest.mark.parametrize("name", list(MODELS))
def test_score_is_the_derivative_of_the_nll_in_the_shift(name):
    d = _problem(name)
    k, p, y = cr.dense_readings(d["Y"], d["Wx"])
    st = cr.stats(d["S"], d["C"], k, p, y, *d["model"], fitted=False)
    eps = 1e-5
    fd = (cr.nll(d["S"], d["C"], k, p, y, *d["model"], delta=eps)
          - cr.nll(d["S"], d["C"], k, p, y, *d["model"], delta=-eps)) / (2 * eps)
    assert st["flags"].max() == 0
    assert np.max(np.abs(fd - st["u"])) <= 1e-7 * max(1.0, np.max(np.abs(st["u"])))
    assert st["u"][0] == 0 and st["n"][0] == 0 and st["info"][0] == 0
    assert np.array_equal(st["n"], d["Wx"].sum(0).astype(int))


@pytest.mark.parametrize("ridge", [0.0, RIDGE])
@pytest.mark.parametrize("name", list(MODELS))
def test_info_is_the_schur_complement_of_the_joint_expected_information(name, ridge):
    """(s, delta) has the expected information [[J + ridge I, v], [v^T, Ixx]] with, in terms of
    info_ref's per-entry h (in t): J = sum h c c^T, v = sum (h / dxdt) c, Ixx = sum h / dxdt^2."""
    d = _problem(name)
    b, sigma, offset, log_model, loss = d["model"]
    k, p, y = cr.dense_readings(d["Y"], d["Wx"])
    st = cr.stats(d["S"], d["C"], k, p, y, *d["model"], fitted=True, ridge=ridge)
    T = d["C"].T @ d["S"]
    h = ir.curvature(T, d["Y"], b, sigma, offset, log_model, loss, "expected") * d["Wx"]
    dxdt = 1.0 / (T + offset) if log_model else np.ones_like(T)
    Jb = ir.blocks(d["S"], d["C"], d["Y"], d["Wx"], b, sigma, offset, log_model, loss, "expected")
    for q in range(1, P):
        M = np.zeros((R + 1, R + 1))
        M[:R, :R] = Jb[q] + ridge * np.eye(R)
        M[:R, R] = M[R, :R] = d["C"] @ (h[:, q] / dxdt[:, q])
        M[R, R] = np.sum(h[:, q] / dxdt[:, q] ** 2)
        want = 1.0 / np.linalg.inv(M)[R, R]
        assert abs(st["Istar"][q] - want) <= 1e-9 * M[R, R], (q, st["Istar"][q], want)
        if not log_model:
            assert st["flags"][q] == 0 and st["info"][q] == st["Istar"][q]
        elif ridge == 0.0:
            # a shift of x = log(t + offset) is a common gain on s but for the offset (1e-3 of t):
            # confounded with the fit of s, I* ~ (offset / t)^2 Ixx
            assert st["flags"][q] == cr.UNTESTABLE and st["info"][q] == 0
            assert st["ratio"][q] < 1e-4
    # the unobserved pixel: nothing to test, with or without the ridge
    assert st["flags"][0] == cr.UNTESTABLE and st["info"][0] == 0 and st["u"][0] == 0


def test_reference_rules_for_edge_positions():
    """n < R without a ridge is untestable (the shift is confounded with s); a log-model reading
    with t + offset <= 0 makes the position invalid; an underflowing P saturates."""
    b, sigma, offset, log_model, loss = MODELS["log4"]
    S = np.array([[0.5, 0.4, -1.0], [0.3, 0.6, 0.5]])
    C = np.array([[0.9, 0.2, 0.5], [0.1, 0.8, 0.4]])
    k = np.array([0, 0, 1, 2, 0, 1])
    p = np.array([0, 1, 1, 1, 2, 2])
    y = np.array([1, 2, 0, 3, 1, 2])
    st = cr.stats(S, C, k, p, y, b, sigma, offset, log_model, loss, fitted=True, ridge=0.0)
    # (under the log model position 1, with n >= R, is untestable too: a shift of log t is a gain
    # on s)
    assert st["flags"].tolist() == [cr.UNTESTABLE, cr.UNTESTABLE, cr.INVALID]
    assert st["n"].tolist() == [1, 3, 1]
    assert st["u"][0] == 0 and st["info"][0] == 0 and st["V"][0] > 0
    assert [st[key][2] for key in ("D", "V", "u", "info")] == [0, 0, 0, 0]
    # the linear model: n = 1 < R = 2 is untestable, n = 3 is not
    lin = cr.stats(S[:, :2], C, k[:4], p[:4], y[:4] % 2, *MODELS["onebit"], fitted=True, ridge=0.0)
    assert lin["flags"].tolist() == [cr.UNTESTABLE, 0] and lin["n"].tolist() == [1, 3]
    assert lin["info"][0] == 0 and lin["u"][0] == 0 and lin["info"][1] > 0 and lin["ratio"][0] < 1e-6
    # one-bit probit far in the tail: P(code 1 | t = -9 sigma below the threshold) underflows fp32
    ob = MODELS["onebit"]
    st = cr.stats(np.array([[0.0], [0.0]]), C, [0, 1], [0, 0], [1, 0], [0.0, 12.0, 20.0], 0.4,
                  fitted=False)
    assert st["flags"].tolist() == [cr.SATURATED] and st["n"].tolist() == [2]
    et = cr.entry_terms(np.zeros(1), np.ones(1, int), [0.0, 12.0, 20.0], 0.4)
    assert et["gx"][0] == 0 and et["l"][0] == -np.log(cr.FLT_MIN) and ob[1] == 0.4


# ---------------------------------------------------------------------------------------
# the package's host side
# ---------------------------------------------------------------------------------------
def _result(z_shift, z_fit, flags):
    from quantized_spectrum_cartography_amd import fits
    z_shift = torch.as_tensor(z_shift, dtype=torch.float32)
    z_fit = torch.as_tensor(z_fit, dtype=torch.float32)
    flags = torch.as_tensor(flags, dtype=torch.int32)
    one = torch.ones_like(z_shift)
    # unit variances: D = z_fit, u = -z_shift
    return fits.check_result(z_fit, one.clone(), -z_shift, one.clone(), one.to(torch.int32), flags)


def test_flagged_thresholds_on_hand_made_z_arrays():
    from scipy.special import ndtri
    n = 10
    crit = -ndtri(0.01 / (2 * n))  # 3.2905
    z = np.zeros((2, 5))
    z[0, 0], z[0, 1], z[0, 2], z[1, 0] = crit * 1.001, -crit * 1.001, crit * 0.999, -crit * 0.999
    r = _result(z, np.zeros((2, 5)), np.zeros((2, 5), int))
    assert torch.allclose(r.z_shift, torch.as_tensor(z, dtype=torch.float32))
    want = np.zeros((2, 5), bool)
    want[0, 0] = want[0, 1] = True
    assert r.flagged(0.01, "shift").numpy().tolist() == want.tolist()
    assert not r.flagged(0.01, "fit").any()
    # "either" tests both at alpha / 2: a larger critical value
    crit2 = -ndtri(0.005 / (2 * n))
    assert crit2 > crit * 1.001 and not r.flagged(0.01, "either").any()
    zf = np.zeros((2, 5))
    zf[1, 4] = crit2 * 1.001
    r = _result(z, zf, np.zeros((2, 5), int))
    assert r.flagged(0.01, "either").numpy().tolist() == (zf != 0).tolist()
    assert r.flagged(0.01, "fit").numpy().tolist() == (zf != 0).tolist()
    # untestable and invalid pixels are never flagged and leave the family: m = 8
    fl = np.zeros((2, 5), int)
    fl[0, 0], fl[1, 1] = 1, 2
    crit8 = -ndtri(0.01 / (2 * 8))
    z[0, 2] = crit8 * 1.001
    assert crit8 * 1.001 < crit
    r = _result(z, zf, fl)
    want = np.zeros((2, 5), bool)
    want[0, 1] = want[0, 2] = want[1, 0] = True  # (0.999 crit exceeds the smaller family's crit8)
    assert crit8 * 1.001 < crit * 0.999
    assert r.flagged(0.01, "shift").numpy().tolist() == want.tolist()
    assert (r.untestable, r.invalid, r.saturated) == (1, 1, 0)
    assert int(r.testable("shift").sum()) == 8 and int(r.testable("fit").sum()) == 9
    with pytest.raises(ValueError):
        r.flagged(0.01, "both")
    with pytest.raises(ValueError):
        r.flagged(0.01, "shift", method="holm")
    with pytest.raises(ValueError):
        r.flagged(0.0)


def test_check_result_forms_the_z_in_one_place():
    from quantized_spectrum_cartography_amd import fits
    D = torch.tensor([[1.0, -2.0, 3.0]])
    V = torch.tensor([[4.0, 0.0, 9.0]])
    u = torch.tensor([[-2.0, 1.0, 0.0]])
    info = torch.tensor([[16.0, 0.0, 0.0]])
    flags = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    r = fits.check_result(D, V, u, info, torch.tensor([[3, 0, 2]], dtype=torch.int32), flags)
    assert r.z_fit.tolist() == [[0.5, 0.0, 1.0]]
    assert r.z_shift.tolist() == [[0.5, 0.0, 0.0]] and r.shift.tolist() == [[0.125, 0.0, 0.0]]
    # the total leaves the invalid pixel out: (1 - 2) / sqrt(4 + 0)
    assert r.z_fit_total == pytest.approx(-0.5)
    assert not any(torch.isnan(t).any() for t in (r.z_fit, r.z_shift, r.shift))


def test_arguments_are_checked_before_any_device_call(monkeypatch):
    from quantized_spectrum_cartography_amd import _lib, fits, qmc, utils

    def boom(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    obs = types.SimpleNamespace(loss="probit", K=4, P=6, I=2, J=3)
    S, C = torch.zeros(2, 1, 2, 3), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="squared"):
        qmc.check_fit(types.SimpleNamespace(loss="squared", K=4, P=6), S, C)
    with pytest.raises(ValueError, match="ridge"):
        qmc.check_fit(obs, S, C, ridge=-1.0)
    with pytest.raises(ValueError, match="ridge"):
        qmc.check_fit(obs, S, C, ridge=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        qmc.check_fit(obs, torch.zeros(2, 1, 2, 4), C)
    with pytest.raises(ValueError, match="shape"):
        qmc.check_fit(obs, S, torch.zeros(2, 5))
    with pytest.raises(ValueError, match="shape"):
        qmc.check_fit(obs, S, torch.zeros(3, 4))
    # solve(check=True): refused in generator mode and for the squared loss
    with pytest.raises(ValueError, match="check"):
        fits.check_post_solve(object(), "probit", 0.0, check=True)
    with pytest.raises(ValueError, match="check"):
        fits.check_post_solve(None, "squared", 0.0, check=True)
    assert fits.check_post_solve(None, "probit", 0.0, check=True).check is True
    assert fits.check_post_solve(None, "probit", 0.0).check is False
    assert fits.check_post_solve(object(), "squared", 0.0).check is False
    sq = _lib.make_model([0.0, 1.0, 2.0], 0.5, loss="squared")
    with pytest.raises(ValueError, match="squared"):
        utils.entry_check(torch.zeros(3, dtype=torch.int64), torch.zeros(3), sq)
    with pytest.raises(ValueError, match="Observations"):
        utils.entry_check(torch.zeros(3, dtype=torch.int64), torch.zeros(3), "model")
    assert qmc.check_fit is fits.check_fit and qmc.CheckResult is fits.CheckResult
