"""CPU: the numpy reference of the per-pixel Newton fit (tests/sfit_ref.py) against torch fp64
autograd of the project's oracle NLL, its own invariants, the argument checks of qmc.fit_S /
solve(polish_s=...) (which need no device), the header's declarations, and -- on exactly the
inputs of tests/test_gpu_sfit.py -- that the reference alone converges every observed pixel
within the default 30 steps, in fp32 and in fp64."""
import types

import numpy as np
import pytest
import torch

import sfit_ref as sr
from test_info_host import MODELS, P, R, _oracle_nll, _problem

RIDGE = 0.3


@pytest.mark.parametrize("loss", ["probit", "logit"])
@pytest.mark.parametrize("name", ["onebit", "log4"])
def test_reference_gradient_and_blocks_equal_autograd_of_the_oracle_nll(name, loss):
    S, C, Y, Wx, b, sigma, offset, log_model = _problem(name)

    def cost(s):
        return (_oracle_nll(s, C, Y, Wx.double(), b, sigma, offset, log_model, loss)
                + 0.5 * RIDGE * (s * s).sum())

    g_t = torch.autograd.functional.jacobian(cost, S).numpy()        # (R, P)
    H_t = torch.autograd.functional.hessian(cost, S).numpy()         # (R, P, R, P)
    f, g, Jb = sr.evaluate(S.numpy(), C.numpy(), Y.numpy(), Wx.numpy(), b, sigma, offset,
                           log_model, loss, "observed", RIDGE, exact_scale=True)
    g = g + RIDGE * S.numpy()
    assert np.allclose(g, g_t, rtol=1e-9, atol=1e-9 * np.abs(g_t).max())
    for p in range(P):
        blk = Jb[p] + RIDGE * np.eye(R)
        assert np.allclose(blk, H_t[:, p, :, p], rtol=1e-9, atol=1e-9 * np.abs(Jb).max())
    assert np.isclose(f.sum(), float(cost(S)), rtol=1e-12)
    assert np.all(g[:, 0] == RIDGE * S.numpy()[:, 0]) and np.all(Jb[0] == 0)  # the empty pixel


@pytest.mark.parametrize("name", list(sr.CASES))
def test_minimiser_is_stationary_and_the_trajectory_descends(name):
    d = sr.problem(name)
    m = sr.model_of(d)
    obsd = sr.observed_pixels(m["Wx"])
    S0 = (np.ones if d["log_model"] else np.zeros)((d["R"], sr.P))
    mn = sr.minimise_fp64(S0, ridge=1e-2, **m)
    g = sr.gradient_fp64(mn["S"], ridge=1e-2, project=d["log_model"], **m)
    assert np.abs(g[:, obsd]).max() <= 1e-9
    for dtype in (np.float64, np.float32):
        tr = []
        sr.fit(S0, ridge=1e-2, dtype=dtype, trace=tr, **m)
        tr = np.array(tr)
        assert len(tr) >= 3 and (np.diff(tr, axis=0) <= 0).all()


@pytest.mark.parametrize("ridge", sr.RIDGES)
@pytest.mark.parametrize("name", list(sr.CASES))
def test_reference_converges_on_every_gpu_case_within_the_default_steps(name, ridge):
    """What makes `unconverged == 0` in tests/test_gpu_sfit.py a condition the reference alone
    meets: the same inputs, the same start, max_steps = 30, in both precisions."""
    d = sr.problem(name)
    m = sr.model_of(d)
    obsd = sr.observed_pixels(m["Wx"])
    assert int((~obsd).sum()) == 1
    S0 = (np.ones if d["log_model"] else np.zeros)((d["R"], sr.P))
    for dtype in (np.float64, np.float32):
        r = sr.fit(S0, ridge=ridge, max_steps=30, dtype=dtype, **m)
        print(name, ridge, dtype.__name__, "steps max", int(r["steps"].max()))
        assert r["converged"][obsd].all()
        assert r["converged"][~obsd].all() and r["identified"].all()
        assert r["steps"].max() <= 30
    # without a ridge the empty pixel alone is unidentified, and it keeps its start
    r0 = sr.fit(S0, ridge=0.0, max_steps=3, dtype=np.float32, **m)
    assert (~r0["identified"]).sum() == 1 and not r0["identified"][0]
    assert np.array_equal(r0["S"][:, 0], S0[:, 0])


def test_fit_s_rejects_bad_arguments_before_touching_a_device():
    from quantized_spectrum_cartography_amd import qmc
    C = torch.zeros(2, 4)
    obs = types.SimpleNamespace(loss="probit", log_model=False)  # (never reached)
    with pytest.raises(ValueError, match="squared"):
        qmc.fit_S(types.SimpleNamespace(loss="squared"), C)
    with pytest.raises(ValueError, match="ridge"):
        qmc.fit_S(obs, C, ridge=-1e-3)
    with pytest.raises(ValueError, match="mu0"):
        qmc.fit_S(obs, C, mu0=-1.0)
    with pytest.raises(ValueError, match="tol"):
        qmc.fit_S(obs, C, tol=0.0)
    with pytest.raises(ValueError, match="max_steps"):
        qmc.fit_S(obs, C, max_steps=0)
    with pytest.raises(ValueError, match="kind"):
        qmc.fit_S(obs, C, kind="laplace")
    r = qmc.FitSResult(S=None, nll=0.0, steps=torch.zeros(1, 1), unconverged=0, unidentified=0)
    assert r.S is None
    assert qmc.SolveResult(S=None, C=None, costs_c=[], costs_s=[]).polish is None


def test_solve_validates_polish_s():
    from quantized_spectrum_cartography_amd import qmc
    Y = torch.zeros(4, 1, 6, 6, dtype=torch.int64)
    Wx = torch.ones(4, 1, 6, 6)
    b = torch.tensor([0.0, 0.5, 1.0])
    kw = dict(R=2, max_iter=1)
    with pytest.raises(ValueError, match="generator"):
        qmc.solve(Y, Wx, b, 0.1, polish_s=5, generator=torch.nn.Identity(),
                  Z_init=torch.zeros(2, 36), **kw)
    with pytest.raises(ValueError, match="squared"):
        qmc.solve(Y, Wx, b, 0.1, polish_s=5, loss="squared", **kw)
    with pytest.raises(ValueError, match="couples pixels"):
        qmc.solve(Y, Wx, b, 0.1, polish_s=5, smooth=0.1, **kw)
    with pytest.raises(ValueError, match="polish_s"):
        qmc.solve(Y, Wx, b, 0.1, polish_s=-1, **kw)


def test_header_declares_the_entry_points():
    from quantized_spectrum_cartography_amd import _lib
    h = _lib.parse_header()
    assert "qsc_sfit" in h and "qsc_sfit_workspace_bytes" in h
    assert len(h["qsc_sfit"][1]) == 23 and len(h["qsc_sfit_workspace_bytes"][1]) == 2
