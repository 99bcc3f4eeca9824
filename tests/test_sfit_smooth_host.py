"""CPU: the numpy reference of the red-black Newton fit of S under the smoothness prior
(tests/sfit_smooth_ref.py) against torch autograd, its monotonicity, its convergence on the inputs
of the GPU cases, and the argument checks of qmc.fit_S_smooth / solve(polish_smooth=...), which
all fire before a device is touched."""
import numpy as np
import pytest
import torch

import sfit_ref as sr
import sfit_smooth_ref as ssr
import smooth_ref

I, J, P = sr.I, sr.J, sr.P


def start(d):
    return (np.ones if d["log_model"] else np.zeros)((d["R"], P))


def torch_objective(d, ridge, weight, kind, delta):
    """S (R, P) fp64 torch -> oracle NLL + ridge / 2 |S|^2 + weight * smooth_ref.penalty_t."""
    data = smooth_ref._data_term(d["Y"], d["Wx"], d["b"], d["sigma"], d["offset"], d["log_model"],
                                 d["loss"], torch.float64)
    C = d["C"].double()
    R = d["R"]
    return lambda S: (data(S, C) + 0.5 * ridge * (S * S).sum()
                      + weight * smooth_ref.penalty_t(S.reshape(R, I, J), kind, delta))


@pytest.mark.parametrize("kind,delta", [("quad", None), ("huber", ssr.DELTA)])
@pytest.mark.parametrize("name", ["bins16", "logit", "log8"])
def test_gradient_and_curvature_additions_match_autograd(name, kind, delta):
    d = sr.problem(name)
    m = sr.model_of(d)
    ridge, w = 0.05, 0.7
    S = 0.8 * d["S"].reshape(d["R"], P).double().numpy() + 0.1
    F = torch_objective(d, ridge, w, kind, delta)
    X = torch.tensor(S, requires_grad=True)
    F(X).backward()
    # the likelihood part with the oracle's fp64 link scale (exact_scale, as tests/test_sfit_host.py
    # compares it), plus the reference's prior additions
    f, g, Jb = sr.evaluate(S, kind="observed", ridge=ridge, exact_scale=True, **m)
    val, pg, pk = ssr.prior_terms(S, I, J, kind, delta)
    g = g + ridge * S + w * pg
    assert np.abs(g - X.grad.numpy()).max() <= 1e-9 * max(1.0, np.abs(g).max())
    # the value, each edge once
    F0 = float(F(X).detach())
    assert np.isclose(f.sum() + 0.5 * w * val.sum(), F0, rtol=1e-12)
    assert np.isclose(ssr.objective(S, I, J, m, ridge, w, kind, delta), F0, rtol=1e-6)
    assert np.abs(ssr.gradient_fp64(S, I, J, m, ridge, w, kind, delta) - g).max() <= 1e-5
    if kind == "quad":
        # the diagonal blocks of the Hessian: observed J + ridge I + w * (number of neighbours) I
        for p in (0, 7, J + 3, P - 1):  # corner, border, interior, corner
            def fp(col, p=p):
                Z = torch.tensor(S).clone()
                Z[:, p] = col
                return F(Z)
            H = torch.autograd.functional.hessian(fp, torch.tensor(S[:, p])).numpy()
            ref = Jb[p] + ridge * np.eye(d["R"]) + w * np.diag(pk[:, p])
            assert np.abs(H - ref).max() <= 1e-9 * max(1.0, np.abs(H).max())
            assert pk[0, p] == (2 if p in (0, P - 1) else 3 if p == 7 else 4)


@pytest.mark.parametrize("name,ridge,kind,delta", ssr.CONVERGED)
def test_objective_is_monotone_and_the_references_converge_on_the_gpu_inputs(name, ridge, kind,
                                                                             delta):
    d = sr.problem(name)
    m = sr.model_of(d)
    S0 = ssr.near_start(d)
    mn = ssr.minimiser(name, ridge, kind, delta)
    assert mn["moved"] == 0
    nb = ssr.budget(name, ridge, kind)
    for dtype in (np.float64, np.float32):
        tr = []
        r = ssr.fit(S0, I, J, m, ssr.WEIGHT, kind, delta, ridge=ridge, dtype=dtype, trace=tr,
                    sweeps=nb)
        tr = np.array(tr)
        # a step is accepted on a pixel's phi rounded to `dtype`, and the trace is a separately
        # rounded fp64 sum over the 135 pixels: allow 64 eps of F
        slack = 64 * float(np.finfo(dtype).eps) * np.abs(tr).max()
        assert (np.diff(tr) <= slack).all(), (name, ridge, dtype, np.diff(tr).max())
        assert r["moved"] == 0 and r["sweeps"] <= nb, (name, ridge, dtype, r["moved"])
        assert r["unidentified"] == 0 and np.isfinite(r["S"]).all()
        # `moved` == 0 because the fit arrived, not because every trial was rejected (a stall
        # leaves errors of 0.4 to 1.8).  A sweep that moves a pixel by less than tol (1 + |s|) at a
        # linear rate rho leaves tol (1 + |s|) / (1 - rho) of distance: 4e-3 at the rho = 0.99 of
        # the crawling cases; the fp32 accept test adds its 1e-3
        e = ssr.pixel_rel(r["S"], mn["S"])
        assert e <= 1e-2, (name, ridge, dtype, e)


def test_huber_delta_splits_the_differences_at_the_minimiser():
    for name, ridge, kind, delta in ssr.CONVERGED:
        if kind != "huber":
            continue
        d = sr.problem(name)
        mn = ssr.minimiser(name, ridge, kind, delta)
        X = mn["S"].reshape(-1, I, J)
        a = np.concatenate([np.abs(X[:, :, 1:] - X[:, :, :-1]).ravel(),
                            np.abs(X[:, 1:] - X[:, :-1]).ravel()])
        assert (a <= delta).any() and (a > delta).any(), name


def test_a_masked_pixel_lands_on_the_mean_of_its_neighbours():
    d = dict(sr.problem("bins16"))
    Wx = d["Wx"].clone()
    pi = 4 * J + 6  # interior, colour 0; the corner pixel 0 is unobserved already
    Wx.reshape(d["K"], P)[:, pi] = 0
    d["Wx"] = Wx
    m = sr.model_of(d)
    S0 = 0.8 * d["S"].reshape(d["R"], P).double().numpy()
    assert ssr.colors(I, J)[pi] == 0 and ssr.colors(I, J)[0] == 0
    r = ssr.visit(S0, 0, I, J, m, ssr.WEIGHT, "quad", None, ridge=0.0, inner_steps=1, mu0=0.0)
    assert np.allclose(r["S"][:, pi], S0[:, [pi - 1, pi + 1, pi - J, pi + J]].mean(axis=1),
                       rtol=0, atol=1e-12)
    assert np.allclose(r["S"][:, 0], S0[:, [1, J]].mean(axis=1), rtol=0, atol=1e-12)
    assert r["identified"][pi] and r["identified"][0]


# ---------------------------------------------------------------------------------------
# argument checks: before a device is touched (no GPU in this test run)
# ---------------------------------------------------------------------------------------
class _Obs:
    loss, log_model = "probit", False


def test_fit_s_smooth_rejects_bad_arguments_before_any_gpu_call():
    from quantized_spectrum_cartography_amd import qmc
    C = torch.ones(3, 5)
    ok = dict(smooth=0.1)
    for kw in (dict(smooth=0.0), dict(smooth=-1.0), dict(sweeps=0), dict(inner_steps=0),
               dict(smooth_kind="tv"), dict(smooth_kind="huber"),
               dict(smooth_kind="huber", smooth_delta=0.0), dict(ridge=-1.0), dict(mu0=-1.0),
               dict(tol=0.0), dict(kind="fisher")):
        with pytest.raises(ValueError):
            qmc.fit_S_smooth(_Obs(), C, **dict(ok, **kw))
    sq = _Obs()
    sq.loss = "squared"
    with pytest.raises(ValueError):
        qmc.fit_S_smooth(sq, C, 0.1)
    with pytest.raises(ValueError, match="fit_S"):
        qmc.fit_S_smooth(_Obs(), C, 0.0)


def test_solve_polish_smooth_rejects_bad_arguments_before_any_gpu_call():
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem("logit")
    args = (d["Y"], d["Wx"], d["b"], d["sigma"])
    kw = dict(R=3, max_iter=1, loss="logit")
    with pytest.raises(ValueError, match="smooth > 0"):
        qmc.solve(*args, polish_smooth=3, **kw)
    with pytest.raises(ValueError):
        qmc.solve(*args, polish_smooth=-1, smooth=0.1, **kw)
    with pytest.raises(ValueError):
        qmc.solve(*args, polish_smooth=3, smooth=0.1, R=3, max_iter=1, loss="squared")
    with pytest.raises(ValueError):  # (smooth > 0 with a generator raises by itself)
        qmc.solve(*args, polish_smooth=3, smooth=0.1, generator=object(), **kw)
    with pytest.raises(ValueError, match="polish_smooth"):
        qmc.solve(*args, polish_smooth=3, generator=object(), **kw)
    # polish_s with the prior keeps raising
    with pytest.raises(ValueError, match="couples pixels"):
        qmc.solve(*args, polish_s=3, smooth=0.1, **kw)
