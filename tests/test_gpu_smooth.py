"""GPU: the spatial smoothness prior on the loss fields -- qsc_smooth_neighbors / qsc_smooth_grad,
utils.smooth_penalty and solve(smooth=...) -- against the fp64 reference of tests/smooth_ref.py.

Tolerances are the project's own for the same comparisons (stated in the header of
tests/test_gpu_logit.py): 1e-5 relative (Frobenius) for passes and solves, rtol 1e-5 for values
and cost histories.  Shapes: (24,20) leaves padding positions, (33,7) is odd and non-square,
(1,70) / (70,1) have edges in one direction only; R in {3, 8, 16} covers the padded rank rows and
the three rank templates; tile=64 gives several tiles."""
import numpy as np
import pytest
import torch

import smooth_ref as sr
from conftest import rel_fro
from oracle import reference_ops as ro

pytestmark = pytest.mark.gpu

SHAPES = [(24, 20), (33, 7), (1, 70), (70, 1)]
KINDS = [("quad", None), ("huber", 0.25)]  # S in [0, 1): differences on both sides of 0.25


def _obs(I, J, K=6, R=4, tile=None, seed=0, f=0.4):
    """A small one-bit observation set (its count-sorted pixel order is what matters here)."""
    from quantized_spectrum_cartography_amd.obs import Observations
    g = torch.Generator().manual_seed(seed)
    Y = torch.randint(0, 2, (K, 1, I, J), generator=g)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), f), generator=g)
    return Observations(Y, Wx, torch.tensor([0.0, 0.5, 1.0]), 0.3, R_hint=R, tile=tile)


def _field(seed, R, I, J):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(R, 1, I, J, generator=g)


_PEN = {}


def _ref(seed, R, I, J, kind, delta):
    """(S, value, grad) of the fp64 reference, computed once per case."""
    key = (seed, R, I, J, kind, delta)
    if key not in _PEN:
        S = _field(seed, R, I, J)
        v, g = sr.penalty(S.double().numpy(), kind, delta)
        _PEN[key] = (S, v, g)
    return _PEN[key]


def _engine(obs, R):
    from quantized_spectrum_cartography_amd.fused import PassEngine
    return PassEngine(obs, R, hist_cap=4)


# ---------------------------------------------------------------------------------------
# 1. neighbour table
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,J,tile", [(24, 20, None), (24, 20, 64), (33, 7, None), (1, 70, None),
                                      (70, 1, None)])
def test_neighbour_table_of_the_count_sorted_order(I, J, tile):
    obs = _obs(I, J, tile=tile)
    if tile:
        assert obs.desc.ntiles > 1
    perm = obs.perm.cpu().numpy()
    assert (perm < 0).sum() == obs.Pp - I * J
    nbr = obs.neighbors()
    assert nbr.dtype == torch.int32 and tuple(nbr.shape) == (obs.Pp, 4)
    assert np.array_equal(nbr.cpu().numpy(), sr.neighbor_table(perm, I, J))
    assert obs.neighbors() is nbr  # cached


@pytest.mark.parametrize("I,J,pads", [(24, 20, 32), (33, 7, 25), (1, 70, 1), (70, 1, 0)])
def test_neighbour_table_of_a_random_order_with_pads(I, J, pads):
    from quantized_spectrum_cartography_amd.obs import neighbor_table
    rng = np.random.default_rng(I * 100 + J)
    perm = np.concatenate([rng.permutation(I * J), np.full(pads, -1)]).astype(np.int32)
    rng.shuffle(perm)  # pads anywhere, not only at the end
    nbr = neighbor_table(torch.from_numpy(perm).cuda(), I, J)
    assert np.array_equal(nbr.cpu().numpy(), sr.neighbor_table(perm, I, J))


# ---------------------------------------------------------------------------------------
# 2. gradient and value, 3. determinism
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,delta", KINDS)
@pytest.mark.parametrize("I,J,R,tile", [(24, 20, 3, None), (24, 20, 8, 64), (33, 7, 16, None),
                                        (33, 7, 3, None), (1, 70, 8, None), (70, 1, 16, None)])
def test_smooth_grad_vs_reference(I, J, R, tile, kind, delta):
    S, v_ref, g_ref = _ref(21, R, I, J, kind, delta)
    if kind == "huber":
        X = S.reshape(R, I, J)
        d = (X[:, :, 1:] - X[:, :, :-1]).abs() if J > 1 else (X[:, 1:] - X[:, :-1]).abs()
        assert (d < delta).any() and (d > delta).any(), "both huber branches must occur"
    obs = _obs(I, J, R=R, tile=tile)
    eng = _engine(obs, R)
    S_pos = obs.to_positions(S.reshape(R, -1))
    RP = S_pos.shape[1]
    gen = torch.Generator().manual_seed(5)
    prefill = torch.randn(obs.Pp, RP, generator=gen).cuda()
    weight = 0.75
    dS = prefill.clone()
    pen = eng.smooth_grad(S_pos, dS, kind, delta, weight, record=False).clone()
    # value
    e_v = abs(pen.item() - v_ref) / abs(v_ref)
    # accumulation: dS = prefill + weight * grad, in pixel order against the fp64 reference
    got = obs.to_pixels(dS - prefill, R).cpu().numpy() / weight
    # (dS - prefill re-rounds at |prefill| ~ 1: 6e-8 absolute against gradients of order 1; the
    # exact-accumulation check below uses a zero prefill)
    dS0 = torch.zeros_like(prefill)
    eng.smooth_grad(S_pos, dS0, kind, delta, 1.0, record=False)
    e_g = rel_fro(obs.to_pixels(dS0, R).cpu().numpy(), g_ref.reshape(R, -1))
    print("case", (I, J, R, tile, kind), "value", e_v, "grad", e_g)
    assert e_v < 1e-5
    assert e_g < 1e-5
    assert rel_fro(got, g_ref.reshape(R, -1)) < 1e-5
    expect = prefill + weight * dS0  # fma(weight, g, prefill) against a separate multiply-add:
    assert torch.allclose(dS, expect, rtol=0, atol=2e-6)  # one ulp of values below 16 (1.9e-6)
    # rows r >= R and padding positions keep the prefill's bits
    assert torch.equal(dS[:, R:], prefill[:, R:])
    pads = obs.perm < 0
    assert int(pads.sum()) == obs.Pp - I * J
    assert torch.equal(dS[pads], prefill[pads])
    # a null dS gives the same value
    pen2 = eng.smooth_grad(S_pos, None, kind, delta, weight, record=False)
    assert torch.equal(pen2, pen)
    # determinism: a second call on the same input gives the same bits
    dS_b = prefill.clone()
    pen_b = eng.smooth_grad(S_pos, dS_b, kind, delta, weight, record=False)
    assert torch.equal(dS_b, dS) and torch.equal(pen_b, pen)


def test_penalty_history_rows_and_counter():
    """The device-side step counter picks the history row; rows past the capacity are dropped."""
    I, J, R = 24, 20, 3
    obs = _obs(I, J, R=R)
    eng = _engine(obs, R)  # hist_cap = 4
    vals = []
    for k in range(6):
        S_pos = obs.to_positions(_field(30 + k, R, I, J).reshape(R, -1))
        vals.append(eng.smooth_grad(S_pos, None, "quad").item())
        eng.smooth_grad(S_pos, None, "quad", record=False)  # does not advance the history
    assert eng.smooth_history() == vals[:4]
    assert int(eng.smooth_ws[:4].view(torch.int32).item()) == 6


def test_smooth_grad_rejects_bad_arguments():
    from quantized_spectrum_cartography_amd import _lib
    L = _lib.lib()
    x = torch.zeros(64, 4, device="cuda")
    nbr = torch.full((64, 4), -1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(int(L.qsc_smooth_workspace_bytes(64)), dtype=torch.uint8, device="cuda")
    pen = torch.zeros(1, device="cuda")
    p = _lib.ptr

    def call(R=3, Pp=64, kind=0, delta=0.0, nbytes=None, pen_=pen):
        return L.qsc_smooth_grad(p(x), p(nbr), R, Pp, kind, delta, 1.0, p(x), p(pen_), None, 0,
                                 p(ws), ws.numel() if nbytes is None else nbytes, None)

    assert call() == 0
    assert call(R=0) == _lib.QSC_EINVAL and call(R=17) == _lib.QSC_EINVAL
    assert call(Pp=0) == _lib.QSC_EINVAL
    assert call(kind=2) == _lib.QSC_EINVAL
    assert call(kind=1, delta=0.0) == _lib.QSC_EINVAL
    assert call(nbytes=16) == _lib.QSC_EINVAL
    assert call(pen_=None) == _lib.QSC_EINVAL
    assert call(Pp=(1 << 28) + 64) == _lib.QSC_EUNSUPPORTED
    assert L.qsc_smooth_workspace_bytes(0) == 0
    assert L.qsc_smooth_workspace_bytes((1 << 28) + 1) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# 4. smooth_penalty (pixel order)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,delta", KINDS)
@pytest.mark.parametrize("I,J,R", [(24, 20, 3), (33, 7, 8), (1, 70, 16), (70, 1, 3)])
def test_smooth_penalty_pixel_order(I, J, R, kind, delta):
    from quantized_spectrum_cartography_amd import utils
    S, v_ref, g_ref = _ref(21, R, I, J, kind, delta)
    v, g = utils.smooth_penalty(S.cuda(), kind, delta)
    assert g.shape == S.shape
    assert abs(v.item() - v_ref) / abs(v_ref) < 1e-5
    assert rel_fro(g.cpu().numpy(), g_ref) < 1e-5
    with pytest.raises(ValueError):
        utils.smooth_penalty(S.cuda(), "huber")
    with pytest.raises(ValueError):
        utils.smooth_penalty(S.cuda(), "tv")


# ---------------------------------------------------------------------------------------
# 5. solver against the fp64 reference
# ---------------------------------------------------------------------------------------
def solver_case(name):
    """Inputs of the solver tests: random strictly positive S_init / C_init and sampling density
    0.3, so that no Adam step is taken on a gradient that is zero up to rounding."""
    seed, R, I, J, K, nbins, log_model, loss, smooth, kind, delta, tile, project_s, s_lo, s_hi = {
        "onebit": (101, 3, 24, 20, 16, 2, False, "probit", 5.0, "quad", None, None, False, 0.05, 0.5),
        # (the log model is well conditioned in fp32 only away from T_hat = 0: S_init >= 0.25, as
        # the log cases of tests/test_gpu_fused.py)
        "log4": (102, 3, 33, 7, 16, 4, True, "probit", 3.0, "huber", 0.1, None, True, 0.25, 0.5),
        "logit": (103, 8, 24, 20, 16, 2, False, "logit", 3.0, "huber", 0.1, 64, False, 0.05, 0.5),
        # S_init above the truth and from 0.001 up: S decreases, entries cross zero within the run
        # and the projection zeroes them
        "onebit_proj": (104, 3, 33, 7, 16, 2, False, "probit", 0.2, "quad", None, None, True,
                        0.001, 2.0),
    }[name]
    g = torch.Generator().manual_seed(seed)
    S = torch.rand(R, 1, I, J, generator=g)
    C = torch.rand(R, K, generator=g)
    Tt = ro.get_tensor(S, C)
    if log_model:
        b = torch.tensor([-23.025850296020508, -1.5, -0.5, 0.3, 3.0])
        sigma, off = 0.7, 1e-3
        Y = ro.quantize(Tt, sigma, b, offset=off, log_model=True,
                        noise=torch.randn(Tt.shape, generator=g))
    else:
        off = 0.0
        b = torch.quantile(Tt.reshape(-1), torch.linspace(0, 1, nbins + 1))
        sigma = (float(Tt.max()) - float(Tt.min())) / 4
        Y = ro.quantize(Tt, sigma, b, noise=torch.randn(Tt.shape, generator=g))
    Wx = torch.bernoulli(torch.full((K, 1, I, J), 0.3), generator=g)
    S0 = s_lo + s_hi * torch.rand(R, 1, I, J, generator=g)
    C0 = 0.05 + 0.5 * torch.rand(R, K, generator=g)
    return dict(Y=Y.unsqueeze(1), Wx=Wx, b=b, sigma=sigma, offset=off, S0=S0, C0=C0,
                log_model=log_model, loss=loss, smooth=smooth, kind=kind, delta=delta, tile=tile,
                project_s=project_s, R=R, n_iter=6)


def solver_ref(d, dtype=torch.float64):
    return sr.free_s_solve_smooth(d["S0"], d["C0"], d["Y"], d["Wx"], d["b"], d["sigma"],
                                  d["offset"], d["log_model"], n_iter=d["n_iter"], loss=d["loss"],
                                  project_s=d["project_s"], smooth=d["smooth"], kind=d["kind"],
                                  delta=d["delta"], dtype=dtype)


@pytest.mark.parametrize("name", ["onebit", "log4", "logit", "onebit_proj"])
def test_smooth_solver_vs_reference_and_graph(name):
    """solve(smooth=...) for 6 iterations against smooth_ref.free_s_solve_smooth in fp64: linear
    one-bit (quad), log-model 4-bin with project_s (huber), loss="logit" (huber, R = 8, eight
    tiles), and a linear one-bit case whose S starts above the truth and from 0.001 up, so that
    the S >= 0 projection zeroes entries within the run (qsc_supdate's project_nonneg; the
    smoothness prior itself pulls small entries up, hence the weak prior there).  The hipGraph
    replay gives the eager run's bits.

    The tolerance was checked to be attainable in fp32 on these inputs before relying on it: the
    fp32 restatement of the reference (solver_ref(d, torch.float32), torch CPU) agrees with the
    fp64 reference to 6.4e-8 / 6.5e-8 / 5.8e-8 / 5.5e-8 (S), 5.4e-8 / 5.8e-8 / 6.4e-8 / 4.8e-8 (C)
    relative Frobenius and 1.2e-7 / 6.0e-8 / 1.2e-7 / 1.1e-7 (costs, relative) for onebit / log4 /
    logit / onebit_proj, and clips the same 5 entries in onebit_proj.  (Log-model inputs with
    S_init from 0.02 up were tried first and dropped: there the fp32 restatement itself is 3e-6 to
    1e-5 from fp64.)"""
    from quantized_spectrum_cartography_amd import qmc
    d = solver_case(name)
    ref = solver_ref(d)
    if name == "onebit_proj":
        assert ref["clipped"] > 0, "the case is meant to exercise the S >= 0 projection"
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=d["n_iter"], loss=d["loss"],
              offset=d["offset"], log_model=d["log_model"], project_s=d["project_s"],
              tile=d["tile"], smooth=d["smooth"], smooth_kind=d["kind"], smooth_delta=d["delta"])
    a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], **kw)
    assert not a.fused
    e_s = rel_fro(a.S.cpu().numpy(), ref["S"].numpy())
    e_c = rel_fro(a.C.cpu().numpy(), ref["C"].numpy())
    e_cc = np.max(np.abs(np.asarray(a.costs_c) / np.asarray(ref["costs_c"]) - 1))
    e_cs = np.max(np.abs(np.asarray(a.costs_s) / np.asarray(ref["costs_s"]) - 1))
    print("case", name, "S", e_s, "C", e_c, "costs_c", e_cc, "costs_s", e_cs)
    assert len(a.costs_c) == len(a.costs_s) == d["n_iter"]
    assert e_s < 1e-5
    assert e_c < 1e-5
    assert np.allclose(a.costs_c, ref["costs_c"], rtol=1e-5)
    assert np.allclose(a.costs_s, ref["costs_s"], rtol=1e-5)
    b = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], use_graph=True, **kw)
    assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
    assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
    assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


def test_smooth_solver_prepare_then_graph_runs():
    """FreeSSolver(smooth>0): prepare(n) then run(n, use_graph=True) twice equals one eager
    run(2n); no fused launch, no chaining."""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    d = solver_case("onebit")
    out = []
    for graph in (False, True):
        obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], R_hint=d["R"])
        sol = qmc.FreeSSolver(obs, d["S0"], d["C0"], hist_cap=8, smooth=d["smooth"])
        assert not sol.fuse and not sol.chain
        if graph:
            sol.prepare(3)
            sol.run(3, use_graph=True)
            sol.run(3, use_graph=True)
        else:
            sol.run(6)
        assert not sol.ahead()
        out.append((sol.S_pixels().cpu().numpy(), sol.C.cpu().numpy(), sol.history()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and len(out[0][2][0]) == 6


# ---------------------------------------------------------------------------------------
# 6. smooth = 0 is the unregularised path
# ---------------------------------------------------------------------------------------
def test_smooth_zero_is_the_default_path():
    from quantized_spectrum_cartography_amd import qmc
    d = solver_case("onebit")
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=5)
    a = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], **kw)
    b = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], smooth=0.0, **kw)
    assert a.fused and b.fused, "the fused S-step + C-pass launch runs with smooth = 0"
    assert np.array_equal(a.S.cpu().numpy(), b.S.cpu().numpy())
    assert np.array_equal(a.C.cpu().numpy(), b.C.cpu().numpy())
    assert a.costs_c == b.costs_c and a.costs_s == b.costs_s


# ---------------------------------------------------------------------------------------
# 7. holdout, 8. validation
# ---------------------------------------------------------------------------------------
def test_smooth_solver_holdout_runs():
    from quantized_spectrum_cartography_amd import qmc
    d = solver_case("onebit")
    r = qmc.solve(d["Y"], d["Wx"], d["b"], d["sigma"], S_init=d["S0"], C_init=d["C0"],
                  max_iter=20, holdout=0.1, check_every=5, patience=10, smooth=d["smooth"])
    assert not r.fused
    assert 1 <= r.best_iter <= 20
    assert len(r.holdout_nll) >= 1
    assert np.isfinite(np.asarray([v for _, v in r.holdout_nll], np.float64)).all()
    assert np.isfinite(r.S.cpu().numpy()).all() and np.isfinite(r.C.cpu().numpy()).all()
    assert len(r.costs_c) == r.iters


def test_smooth_validation_errors():
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    d = solver_case("onebit")
    args = (d["Y"], d["Wx"], d["b"], d["sigma"])
    kw = dict(S_init=d["S0"], C_init=d["C0"], max_iter=1)
    with pytest.raises(ValueError):
        qmc.solve(*args, smooth=-0.5, **kw)
    with pytest.raises(ValueError):
        qmc.solve(*args, smooth=1.0, smooth_kind="tv", **kw)
    with pytest.raises(ValueError):
        qmc.solve(*args, smooth=1.0, smooth_kind="huber", **kw)
    with pytest.raises(ValueError):
        qmc.solve(*args, smooth=1.0, smooth_kind="huber", smooth_delta=-1.0, **kw)
    with pytest.raises(ValueError):
        qmc.solve(*args, smooth=1.0, generator=torch.nn.Identity(), Z_init=d["S0"].reshape(3, -1),
                  C_init=d["C0"], max_iter=1)
    obs = Observations(*args, R_hint=3)
    with pytest.raises(ValueError):
        qmc.FreeSSolver(obs, d["S0"], d["C0"], smooth=1.0, smooth_kind="huber")
