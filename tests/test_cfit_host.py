"""CPU: the numpy reference of the per-bin projected Newton fit of C (tests/cfit_ref.py) against
tests/sfit_ref.py on transposed inputs, against torch fp64 autograd of the project's oracle NLL,
the argument checks of qmc.fit_C / solve(polish_c=...) (which need no device), the header's
declarations, and -- on exactly the inputs of tests/test_gpu_cfit.py -- that the reference alone
converges every observed bin within 40 steps, in fp32 and in fp64."""
import types

import numpy as np
import pytest
import torch

import cfit_ref as cr
import sfit_ref as sr
from test_info_host import P, R, _oracle_nll, _problem

RIDGE = 0.3


@pytest.mark.parametrize("name", list(cr.CASES))
def test_without_the_bound_the_reference_is_sfit_ref_on_transposed_inputs(name):
    d = cr.problem(name)
    m = cr.model_of(d)
    C0 = cr.default_start(d)
    S = m["S"]
    for dtype in (np.float64, np.float32):
        a = cr.fit(C0, ridge=1e-2, max_steps=6, project=False, dtype=dtype, **m)
        b = sr.fit(C0, S, m["Y"].T, m["Wx"].T, m["b"], m["sigma"], m["offset"], m["log_model"],
                   m["loss"], ridge=1e-2, max_steps=6, project=False, dtype=dtype)
        assert np.array_equal(a["C"], b["S"]) and np.array_equal(a["f"], b["f"], equal_nan=True)
        assert np.array_equal(a["steps"], b["steps"])
        assert np.array_equal(a["converged"], b["converged"])
        assert np.array_equal(a["identified"], b["identified"])
        assert not a["held"].any()


@pytest.mark.parametrize("loss", ["probit", "logit"])
@pytest.mark.parametrize("name", ["onebit", "log4"])
def test_reference_gradient_and_blocks_equal_autograd_of_the_oracle_nll_in_c(name, loss):
    S, C, Y, Wx, b, sigma, offset, log_model = _problem(name)

    def cost(c):
        return (_oracle_nll(S, c, Y, Wx.double(), b, sigma, offset, log_model, loss)
                + 0.5 * RIDGE * (c * c).sum())

    g_t = torch.autograd.functional.jacobian(cost, C).numpy()        # (R, K)
    H_t = torch.autograd.functional.hessian(cost, C).numpy()         # (R, K, R, K)
    K = C.shape[1]
    f, g, Jb = sr.evaluate(C.numpy(), S.numpy(), Y.numpy().T, Wx.numpy().T, b, sigma, offset,
                           log_model, loss, "observed", RIDGE, exact_scale=True)
    g = g + RIDGE * C.numpy()
    assert np.allclose(g, g_t, rtol=1e-9, atol=1e-9 * np.abs(g_t).max())
    for k in range(K):
        blk = Jb[k] + RIDGE * np.eye(R)
        assert np.allclose(blk, H_t[:, k, :, k], rtol=1e-9, atol=1e-9 * np.abs(Jb).max())
    assert np.isclose(f.sum(), float(cost(C)), rtol=1e-12)
    # cfit_ref.evaluate is that call (with the nominal link scale)
    f2, g2, J2 = cr.evaluate(C.numpy(), S.numpy(), Y.numpy(), Wx.numpy(), b, sigma, offset,
                             log_model, loss, "observed", RIDGE)
    f3, g3, J3 = sr.evaluate(C.numpy(), S.numpy(), Y.numpy().T, Wx.numpy().T, b, sigma, offset,
                             log_model, loss, "observed", RIDGE)
    assert np.array_equal(f2, f3) and np.array_equal(g2, g3) and np.array_equal(J2, J3)
    assert f.shape == (K,) and g.shape == (R, K) and Jb.shape == (K, R, R) and S.shape[1] == P


@pytest.mark.parametrize("ridge", cr.RIDGES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_projected_reference_converges_on_every_gpu_case_within_40_steps(name, ridge):
    """What makes `unconverged == 0` in tests/test_gpu_cfit.py a condition the reference alone
    meets: the same inputs, the same start, max_steps = 40, in both precisions."""
    d = cr.problem(name)
    m = cr.model_of(d)
    obsd = cr.observed_bins(m["Wx"])
    assert int((~obsd).sum()) == 1 and not obsd[0]
    C0 = cr.default_start(d)
    for dtype in (np.float64, np.float32):
        tr = []
        r = cr.fit(C0, ridge=ridge, max_steps=cr.MAX_STEPS, dtype=dtype, trace=tr, **m)
        g = cr.gradient_fp64(r["C"], ridge=ridge, **m)
        n_held = int(((r["C"] <= 0) & obsd[None, :]).sum())
        print(name, ridge, dtype.__name__, "steps max", int(r["steps"].max()), "at the bound",
              n_held, "projected gradient", float(np.abs(g[:, obsd]).max()))
        assert r["converged"][obsd].all() and r["steps"].max() <= cr.MAX_STEPS
        assert (r["C"] >= 0).all() and np.isfinite(r["f"]).all()
        assert (np.diff(np.array(tr), axis=0) <= 0).all()
        if dtype is np.float64:
            assert np.abs(g[:, obsd]).max() <= (1e-2 if d["log_model"] else 1e-5)
    # without a ridge the empty bin alone is unidentified, and it keeps its start
    r0 = cr.fit(C0, ridge=0.0, max_steps=3, dtype=np.float32, **m)
    assert (~r0["identified"]).sum() == 1 and not r0["identified"][0]
    assert np.array_equal(r0["C"][:, 0], C0[:, 0])
    # with a ridge, from zeros, it stays exactly 0 and is identified
    rz = cr.fit(np.zeros_like(C0), ridge=ridge, max_steps=3, dtype=np.float32, **m)
    assert (rz["C"][:, 0] == 0).all() and rz["identified"][0] and rz["converged"][0]


def test_fit_c_rejects_bad_arguments_before_touching_a_device():
    from quantized_spectrum_cartography_amd import qmc
    S = torch.zeros(2, 1, 3, 3)
    obs = types.SimpleNamespace(loss="probit", log_model=False)  # (never reached)
    with pytest.raises(ValueError, match="squared"):
        qmc.fit_C(types.SimpleNamespace(loss="squared"), S)
    with pytest.raises(ValueError, match="ridge"):
        qmc.fit_C(obs, S, ridge=-1e-3)
    with pytest.raises(ValueError, match="mu0"):
        qmc.fit_C(obs, S, mu0=-1.0)
    with pytest.raises(ValueError, match="tol"):
        qmc.fit_C(obs, S, tol=0.0)
    with pytest.raises(ValueError, match="max_steps"):
        qmc.fit_C(obs, S, max_steps=0)
    with pytest.raises(ValueError, match="kind"):
        qmc.fit_C(obs, S, kind="laplace")
    r = qmc.FitCResult(C=None, nll=0.0, steps=torch.zeros(1), unconverged=0, unidentified=0)
    assert r.C is None and r.std_C is None
    assert qmc.SolveResult(S=None, C=None, costs_c=[], costs_s=[]).polish_c is None


def test_solve_validates_polish_c():
    from quantized_spectrum_cartography_amd import qmc
    Y = torch.zeros(4, 1, 6, 6, dtype=torch.int64)
    Wx = torch.ones(4, 1, 6, 6)
    b = torch.tensor([0.0, 0.5, 1.0])
    kw = dict(R=2, max_iter=1)
    with pytest.raises(ValueError, match="generator"):
        qmc.solve(Y, Wx, b, 0.1, polish_c=5, generator=torch.nn.Identity(),
                  Z_init=torch.zeros(2, 36), **kw)
    with pytest.raises(ValueError, match="squared"):
        qmc.solve(Y, Wx, b, 0.1, polish_c=5, loss="squared", **kw)
    with pytest.raises(ValueError, match="polish_c"):
        qmc.solve(Y, Wx, b, 0.1, polish_c=-1, **kw)
    # the smoothness prior does not involve C: accepted
    assert qmc.check_polish_c(5, None, "probit") == 5 and qmc.check_polish_c(0, object(), "squared") == 0


def test_header_declares_the_entry_points():
    from quantized_spectrum_cartography_amd import _lib
    h = _lib.parse_header()
    for name in ("qsc_cfit_workspace_bytes", "qsc_cfit_groups", "qsc_cfit_active_offset", "qsc_cfit_begin",
                 "qsc_cfit_iterate", "qsc_cfit_finish"):
        assert name in h
    assert len(h["qsc_cfit_begin"][1]) == 18 and len(h["qsc_cfit_iterate"][1]) == 12
    assert len(h["qsc_cfit_finish"][1]) == 12
