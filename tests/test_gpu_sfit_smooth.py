"""GPU: the red-black Newton fit of S under the smoothness prior -- qsc_sfit_smooth,
qmc.fit_S_smooth and solve(polish_smooth=...) -- against the numpy reference of
tests/sfit_smooth_ref.py.

Shapes: tests/test_gpu_sfit.py's 9 x 15 pixels at tile 64 (Pp = 192: both colours, corners with 2
neighbours, border pixels with 3, 57 padding positions) and its five layouts / models at ridge
1e-2 and 1; 1 x 40 and 40 x 1 grids; 260 x 260 at R 16 (more slices than the workspace grid has
waves).  Weight, Huber delta and the sweep budget are sfit_smooth_ref's (chosen on the CPU,
tests/test_sfit_smooth_host.py).

Bounds: maximum relative error over all pixels (every pixel is observed or has neighbours)
against the fp64 reference within max(1e-5, 10 floor), floor the same figure of the fp32 numpy
reference (the rule of tests/test_gpu_sfit.py).  The relative error is taken per pixel, of the
pixel's row s in the infinity norm: |s - s_ref|_inf / |s_ref|_inf (sfit_smooth_ref.pixel_rel).
The element-wise figure (tests/test_gpu_sfit.py's max_rel) is printed next to it.
Element by element it is not a property of the arithmetic here: under the prior with a small
ridge the R = 16 rows have entries of both signs and sizes up to 4, some of the 2160 entries lie
within 1e-3 of zero, and the ordinary fp32 error of 3e-6 there reads as 1e-4 to 2e-3 depending on
the order of summation alone (measured on the CPU: the fp32 reference against fp64 with the
entries of one pixel listed in six other orders gave 5e-4 to 8e-4 where the natural order gives
1.2e-4, all at one entry of value 4.7e-4).  DESIGN.md section 7n has the measured figures.
"""
import ctypes

import numpy as np
import pytest
import torch

import sfit_ref as sr
import sfit_smooth_ref as ssr
from test_gpu_sfit import max_rel as elem_rel, observations, observed, raw_fit, start

pytestmark = pytest.mark.gpu

I, J, P, TILE = sr.I, sr.J, sr.P, sr.TILE
W, DELTA = ssr.WEIGHT, ssr.DELTA
ULP = 2.0 ** -23
_REF = {}
max_rel = ssr.pixel_rel
KINDS = ssr.KINDS


def cached(key, fn):
    if key not in _REF:
        r = fn()
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def visits(obs, d, S0, colors, ridge, weight=W, kind="quad", delta=None, inner_steps=1, tol=1e-5,
           mu0=1e-3, S_pos=None, grid=(I, J)):
    """qsc_sfit_smooth, one launch per entry of `colors`, through qmc._sfit_smooth_visit with the
    defaults of fit_S_smooth: pixel-order numpy S, steps, per-visit counters and the position-order
    S after every launch."""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.fused import smooth_kind
    R = d["R"]
    ikind = "expected" if d["log_model"] else "observed"
    if S_pos is None:
        S_pos = obs.to_positions(torch.as_tensor(S0, dtype=torch.float32))
    Cd = d["C"].cuda().contiguous()
    code, dl = smooth_kind(kind, delta)
    f, nll, steps, cnt, ws = qmc._sfit_smooth_bufs(obs, R, len(colors))
    cnt = cnt.reshape(-1, 3)[:len(colors)]
    after = []
    for i, c in enumerate(colors):
        qmc._sfit_smooth_visit(obs, S_pos, Cd, R, c, ikind, ridge, inner_steps, tol, mu0,
                               d["log_model"], code, dl, weight, f, nll, steps, cnt[i], ws)
        after.append(S_pos.clone())
    ip = obs.iperm().long()
    return dict(S=obs.to_pixels(S_pos, R).double().cpu().numpy(), steps=steps[ip].cpu().numpy(),
                counters=cnt.cpu().numpy(), after=after, S_pos=S_pos, f_pos=f, nll_pos=nll,
                steps_pos=steps)


def ref_visits(name, d, S0, colors, ridge, dtype, weight=W, kind="quad", delta=None,
               inner_steps=1, mu0=1e-3, grid=(I, J)):
    def run():
        s, out = np.array(S0, np.float64), []
        for c in colors:
            r = ssr.visit(s, c, grid[0], grid[1], sr.model_of(d), weight, kind, delta, ridge=ridge,
                          inner_steps=inner_steps, mu0=mu0, dtype=dtype)
            s = r["S"]
            out.append(r)
        return dict(S=np.asarray(s, np.float64), last=out[-1],
                    moved=np.array([r["moved"] for r in out]))
    return cached(("visits", name, tuple(colors), ridge, dtype, weight, kind, delta, inner_steps,
                   mu0), run)


# ---------------------------------------------------------------------------------------
# (i) one visit of each colour
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,delta", KINDS)
@pytest.mark.parametrize("ridge", sr.RIDGES)
@pytest.mark.parametrize("name", list(sr.CASES))
def test_one_visit_of_each_colour_vs_reference(name, ridge, kind, delta):
    d = sr.problem(name)
    obs = observations(name)
    assert obs.Pp == 192
    S0 = start(d, "near")
    r64 = ref_visits(name, d, S0, (0, 1), ridge, np.float64, kind=kind, delta=delta)
    r32 = ref_visits(name, d, S0, (0, 1), ridge, np.float32, kind=kind, delta=delta)
    floor = max_rel(r32["S"], r64["S"])
    tol = max(1e-5, 10 * floor)
    S_in = obs.to_positions(torch.as_tensor(S0, dtype=torch.float32))
    before = S_in.clone()
    g = visits(obs, d, S0, (0, 1), ridge, kind=kind, delta=delta, S_pos=S_in)
    e = max_rel(g["S"], r64["S"])
    print("case", name, "ridge", ridge, kind, "two visits", e, "floor", floor, "tol", tol,
          "| element-wise", elem_rel(g["S"], r64["S"]), "floor", elem_rel(r32["S"], r64["S"]))
    # the rows of the other colour and the padding rows: bit-identical after each launch
    perm = obs.perm.cpu().numpy()
    col = np.where(perm >= 0, ssr.colors(I, J)[np.maximum(perm, 0)], -1)
    prev = before
    for c, now in zip((0, 1), g["after"]):
        keep = torch.as_tensor(col != c, device=now.device)
        assert torch.equal(now[keep], prev[keep])
        assert not torch.equal(now[~keep], prev[~keep])
        prev = now
    assert not np.isnan(g["S"]).any() and not torch.isnan(g["f_pos"]).any()
    assert (g["steps"] == 1).all()
    assert e <= tol
    assert (g["counters"][:, 1:] >= 0).all() and g["counters"][:, 2].sum() == 0


@pytest.mark.parametrize("name", list(sr.CASES))
def test_weight_zero_is_qsc_sfit(name):
    d = sr.problem(name)
    obs = observations(name)
    o = observed(d)
    ridge, n = 1e-2, 3
    S0 = start(d, "near")
    r64 = sr.fit(S0, ridge=ridge, max_steps=n, dtype=np.float64, **sr.model_of(d))
    r32 = sr.fit(S0, ridge=ridge, max_steps=n, dtype=np.float32, **sr.model_of(d))
    tol = max(1e-5, 10 * max_rel(r32["S"][:, o], r64["S"][:, o]))
    a = raw_fit(obs, d, S0, ridge, max_steps=n)
    g = visits(obs, d, S0, (0, 1), ridge, weight=0.0, inner_steps=n)
    e = max_rel(g["S"][:, o], a["S"][:, o])
    print("case", name, "weight 0 vs qsc_sfit", e, "tol", tol)
    assert e <= tol
    assert (g["steps"] == a["steps"]).all()


def test_masked_pixels_land_on_the_mean_of_their_neighbours():
    from quantized_spectrum_cartography_amd.obs import Observations
    d = dict(sr.problem("bins16"))
    R = d["R"]
    pi = 4 * J + 6  # interior, colour 0; pixel 0 (corner, colour 0) is unobserved already
    Wx = d["Wx"].clone()
    Wx.reshape(d["K"], P)[:, pi] = 0
    d["Wx"] = Wx
    obs = Observations(d["Y"], Wx, d["b"], d["sigma"], tile=TILE, R_hint=R)
    S0 = start(d, "near")
    # ridge 0, quad: phi is exactly quadratic there, and with mu0 = 0 the step is the Newton step
    g = visits(obs, d, S0, (0,), 0.0, inner_steps=1, mu0=0.0)
    S0f = np.float32(S0).astype(np.float64)
    for p, nb in ((pi, [pi - 1, pi + 1, pi - J, pi + J]), (0, [1, J])):
        mean = S0f[:, nb].mean(axis=1)
        assert (np.abs(g["S"][:, p] - mean) <= 1e-6 * (1 + np.abs(mean))).all(), p
    assert g["counters"][0, 2] == 0  # identified through their neighbours
    a = raw_fit(obs, d, S0, 0.0, max_steps=1, mu0=0.0)
    assert a["unidentified"] == 2


# ---------------------------------------------------------------------------------------
# (ii) the converged fit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ridge,kind,delta", ssr.CONVERGED)
def test_converged_fit_vs_minimiser(name, ridge, kind, delta):
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem(name)
    m = sr.model_of(d)
    obs = observations(name)
    R = d["R"]
    S0 = ssr.near_start(d)
    mn = ssr.minimiser(name, ridge, kind, delta)
    nb = ssr.budget(name, ridge, kind)
    r32 = cached(("fit32", name, ridge, kind), lambda: ssr.fit(
        S0, I, J, m, W, kind, delta, ridge=ridge, dtype=np.float32, sweeps=nb))
    floor = max_rel(r32["S"], mn["S"])
    gr = lambda S: np.abs(ssr.gradient_fp64(S, I, J, m, ridge, W, kind, delta,
                                            project=d["log_model"])).max()
    res = qmc.fit_S_smooth(obs, d["C"], W, smooth_kind=kind, smooth_delta=delta, ridge=ridge,
                           sweeps=nb, S_init=torch.as_tensor(S0, dtype=torch.float32))
    S = res.S.reshape(R, P).double().cpu().numpy()
    e = max_rel(S, mn["S"])
    print("case", name, "ridge", ridge, kind, "S error", e, "floor", floor, "gradient", gr(S),
          "floor", gr(r32["S"]), "sweeps", res.sweeps, "moved", res.moved, "unconverged",
          res.unconverged, "| element-wise", elem_rel(S, mn["S"]), "floor", elem_rel(r32["S"], mn["S"]))
    assert tuple(res.S.shape) == (R, 1, I, J) and tuple(res.steps.shape) == (I, J)
    assert torch.isfinite(res.S).all() and np.isfinite(res.objective)
    assert res.moved == 0 and res.unidentified == 0
    assert e <= max(1e-5, 10 * floor)
    F = ssr.objective(S, I, J, m, ridge, W, kind, delta)
    assert np.isclose(res.objective, F, rtol=1e-5)
    f64, _, _ = sr.evaluate(S, ridge=0.0, kind="observed", **m)
    assert np.isclose(res.nll, f64.sum(), rtol=1e-5)


def test_a_stall_is_told_apart_from_convergence():
    """From S = 0 under the logistic link the two trials of a visit are rejected in the link's
    tail: nothing moves, and the result says so in `unconverged`; from 0.8 S_true it arrives."""
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem("logit")
    obs = observations("logit")
    stalled = qmc.fit_S_smooth(obs, d["C"], W, ridge=1e-2, sweeps=8)
    assert stalled.moved == 0 and stalled.unconverged > 0
    near = qmc.fit_S_smooth(obs, d["C"], W, ridge=1e-2, sweeps=ssr.SWEEPS,
                            S_init=torch.as_tensor(ssr.near_start(d), dtype=torch.float32))
    print("stall: unconverged", stalled.unconverged, "arrived: unconverged", near.unconverged)
    assert near.moved == 0 and near.unconverged < stalled.unconverged


@pytest.mark.parametrize("kind,delta", KINDS)
@pytest.mark.parametrize("name", list(sr.CASES))
def test_objective_is_monotone_in_sweeps(name, kind, delta):
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem(name)
    m = sr.model_of(d)
    obs = observations(name)
    ridge = 1e-2
    S0 = start(d, "default")
    F0 = ssr.objective(S0, I, J, m, ridge, W, kind, delta)
    prev = F0 + 8 * ULP * abs(F0)
    for n in (1, 2, 3, 5):
        res = qmc.fit_S_smooth(obs, d["C"], W, smooth_kind=kind, smooth_delta=delta, ridge=ridge,
                               sweeps=n, sync_every=0)
        F = ssr.objective(res.S.reshape(d["R"], P).double().cpu().numpy(), I, J, m, ridge, W, kind,
                          delta)
        assert np.isfinite(F) and F <= prev, (n, F - prev)
        assert F <= F0 + 8 * ULP * abs(F0) and res.sweeps == n
        assert not torch.isnan(res.S).any()
        prev = F + 8 * ULP * abs(F)


# ---------------------------------------------------------------------------------------
# (iii) determinism
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["onebit16", "bins4", "log8"])
def test_determinism_graph_and_sync_every(name):
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem(name)
    obs = observations(name)
    S0 = start(d, "near")
    a = visits(obs, d, S0, (0, 1, 0, 1), 1e-2, inner_steps=2)
    b = visits(obs, d, S0, (0, 1, 0, 1), 1e-2, inner_steps=2)
    for k in ("S_pos", "f_pos", "nll_pos", "steps_pos"):
        assert torch.equal(a[k], b[k])
    assert (a["counters"] == b["counters"]).all()
    # the same 2-sweep sequence captured into a hipGraph replays to the eager bits
    from quantized_spectrum_cartography_amd.fused import smooth_kind
    R = d["R"]
    ikind = "expected" if d["log_model"] else "observed"
    Cd = d["C"].cuda().contiguous()
    S_pos = obs.to_positions(torch.as_tensor(S0, dtype=torch.float32))
    init = S_pos.clone()
    f, nll, steps, cnt, ws = qmc._sfit_smooth_bufs(obs, R, 2)
    obs.neighbors()
    code, dl = smooth_kind("quad", None)

    def seq():
        for i in range(2):
            for c in (0, 1):
                qmc._sfit_smooth_visit(obs, S_pos, Cd, R, c, ikind, 1e-2, 2, 1e-5, 1e-3,
                                       d["log_model"], code, dl, W, f, nll, steps, cnt[i, c], ws)
    seq()  # (eager once: everything lazily built exists before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        with torch.cuda.graph(g, stream=st):
            seq()
    torch.cuda.current_stream().wait_stream(st)
    S_pos.copy_(init)
    steps.zero_()
    cnt.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(S_pos, a["S_pos"]) and torch.equal(steps, a["steps_pos"])
    assert (cnt.reshape(-1, 3).cpu().numpy() == a["counters"]).all()
    # sync_every 0 / 1 / 4: the same bits when none stops early
    rs = [qmc.fit_S_smooth(obs, d["C"], W, ridge=1e-2, sweeps=3, sync_every=s) for s in (0, 1, 4)]
    assert all(r.sweeps == 3 for r in rs)
    assert torch.equal(rs[0].S, rs[1].S) and torch.equal(rs[0].S, rs[2].S)
    assert rs[0].objective == rs[1].objective == rs[2].objective


@pytest.mark.parametrize("name", ["bins4", "bins16", "logit"])
def test_natural_and_scheduled_list_order_agree(name):
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem(name)
    m = sr.model_of(d)
    ridge = 1e-2
    obs, nat = observations(name), observations(name, schedule=False)
    assert obs.schedule and not nat.schedule
    S0 = ssr.near_start(d)
    mn = ssr.minimiser(name, ridge, "quad", None)
    fit = lambda o: qmc.fit_S_smooth(
        o, d["C"], W, ridge=ridge, sweeps=ssr.SWEEPS,
        S_init=torch.as_tensor(S0, dtype=torch.float32)).S.reshape(d["R"], P).double().cpu().numpy()
    a, n = fit(obs), fit(nat)
    ea, en = max_rel(a, mn["S"]), max_rel(n, mn["S"])
    print("case", name, "scheduled", ea, "natural", en)
    # each within its distance of the minimiser, hence within their sum of each other (relative
    # errors of values of order 1; 1.25: the denominators differ)
    assert max_rel(n, a) <= 1.25 * (ea + en) + 1e-7


# ---------------------------------------------------------------------------------------
# (iv) degenerate and large grids
# ---------------------------------------------------------------------------------------
def grid_problem(Ig, Jg, R, K, f, seed):
    """A one-bit probit problem on an Ig x Jg grid (sfit_ref.problem's recipe)."""
    from oracle import reference_ops as ro
    g = torch.Generator().manual_seed(seed)
    S = 0.2 + 0.8 * torch.rand(R, 1, Ig, Jg, generator=g)
    C = 0.1 + 0.9 * torch.rand(R, K, generator=g)
    T = ro.get_tensor(S, C)
    b = torch.tensor([0.0, float(T.median()), float(T.max()) + 1.0])
    Y = ro.quantize(T, 0.5, b, noise=torch.randn(T.shape, generator=g)).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, Ig, Jg), f), generator=g)
    return dict(name="grid%dx%d" % (Ig, Jg), R=R, K=K, S=S, C=C, Y=Y, Wx=Wx, b=b, sigma=0.5,
                offset=0.0, log_model=False, loss="probit", nbins=2)


@pytest.mark.parametrize("shape", [(1, 40), (40, 1)])
def test_degenerate_grids(shape):
    from quantized_spectrum_cartography_amd.obs import Observations
    Ig, Jg = shape
    d = grid_problem(Ig, Jg, 3, 37, 0.7, 21)
    obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], tile=TILE, R_hint=3)
    S0 = 0.8 * d["S"].reshape(3, -1).double().numpy()
    ridge = 1e-2
    out = {}
    for dt in (np.float64, np.float32):
        s = S0
        for c in (0, 1):
            s = ssr.visit(s, c, Ig, Jg, sr.model_of(d), W, ridge=ridge, inner_steps=1, dtype=dt)["S"]
        out[dt] = np.asarray(s, np.float64)
    tol = max(1e-5, 10 * max_rel(out[np.float32], out[np.float64]))
    g = visits(obs, d, S0, (0, 1), ridge)
    e = max_rel(g["S"], out[np.float64])
    print("grid", shape, "error", e, "tol", tol)
    assert e <= tol and (g["steps"] == 1).all()


def test_more_slices_than_waves_in_the_grid():
    from quantized_spectrum_cartography_amd.obs import Observations
    Ig = Jg = 260
    d = grid_problem(Ig, Jg, 16, 20, 0.3, 22)
    obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], R_hint=16)
    assert obs.Pp >= 67600 > 65536
    S0 = 0.8 * d["S"].reshape(16, -1).double().numpy()
    ridge = 1.0
    m = sr.model_of(d)
    cols = (0, 1, 0, 1)
    g = visits(obs, d, S0, cols, ridge, grid=(Ig, Jg))
    h = visits(obs, d, S0, cols, ridge, grid=(Ig, Jg))
    assert torch.equal(g["S_pos"], h["S_pos"]) and (g["counters"] == h["counters"]).all()
    # per visit against the fp32 reference started from the kernel's own previous rows: the
    # one-step bound (max(1e-5, 10 floor), floor the fp32 reference against the fp64 one)
    prev = obs.to_positions(torch.as_tensor(S0, dtype=torch.float32))
    for c, now in zip(cols, g["after"]):
        s_in = obs.to_pixels(prev, 16).double().cpu().numpy()
        r32 = ssr.visit(s_in, c, Ig, Jg, m, W, ridge=ridge, inner_steps=1, dtype=np.float32)
        r64 = ssr.visit(s_in, c, Ig, Jg, m, W, ridge=ridge, inner_steps=1, dtype=np.float64)
        tol = max(1e-5, 10 * max_rel(r32["S"], r64["S"]))
        e = max_rel(obs.to_pixels(now, 16).double().cpu().numpy(), r32["S"])
        print("260 x 260 colour", c, "error vs fp32 reference", e, "tol", tol)
        assert e <= tol
        prev = now
    assert not torch.isnan(g["S_pos"]).any()


# ---------------------------------------------------------------------------------------
# (v) the C ABI's refusals and solve(polish_smooth=...)
# ---------------------------------------------------------------------------------------
def test_abi_rejects_what_it_cannot_compute():
    from quantized_spectrum_cartography_amd import _lib
    L = _lib.lib()
    d = sr.problem("bins16")
    R = d["R"]
    obs = observations("bins16")
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    keep = S_pos.clone()
    Cd = d["C"].cuda().contiguous()
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    nbr = obs.neighbors()
    p, cf = _lib.ptr, ctypes.c_float

    def call(color=0, weight=0.1, sk=0, delta=0.0, inner=1, Ig=I, ridge=0.1, kind=1, tol=1e-5):
        desc, ent, _ = obs.layout(R)
        return L.qsc_sfit_smooth(desc, p(ent), p(obs.s_width), p(obs.s_off), p(obs.perm), p(nbr),
                                 Ig, J, color, obs.model, R, p(Cd), p(S_pos), kind, cf(ridge),
                                 cf(1e-3), cf(tol), inner, 0, sk, cf(delta), cf(weight), None, None,
                                 None, p(cnt[0:1]), p(cnt[1:2]), p(cnt[2:3]), None, 0, None)

    E = _lib.QSC_EINVAL
    assert call(color=2) == E and call(color=-1) == E and call(weight=-1.0) == E
    assert call(sk=2) == E and call(sk=1, delta=0.0) == E and call(inner=0) == E
    assert call(Ig=I + 1) == E and call(ridge=-1.0) == E and call(kind=2) == E and call(tol=0.0) == E
    torch.cuda.synchronize()
    assert torch.equal(S_pos, keep)
    assert call() == 0 and call(sk=1, delta=0.1, color=1) == 0
    desc, _, _ = obs.layout(R)
    assert L.qsc_sfit_smooth_workspace_bytes(desc, R) == 0
    assert L.qsc_sfit_smooth_workspace_bytes(desc, 16) > 0
    torch.cuda.synchronize()


def test_solve_polish_smooth():
    from quantized_spectrum_cartography_amd import qmc
    d = sr.problem("logit")
    R, K = d["R"], d["K"]
    g = torch.Generator().manual_seed(5)
    S0 = 0.2 + 0.5 * torch.rand(R, 1, I, J, generator=g)
    C0 = 0.1 + 0.5 * torch.rand(R, K, generator=g)
    kw = dict(S_init=S0, C_init=C0, max_iter=3, tile=TILE, loss="logit", smooth=0.1)
    args = (d["Y"], d["Wx"], d["b"], d["sigma"])
    plain = qmc.solve(*args, **kw)
    zero = qmc.solve(*args, polish_smooth=0, **kw)
    assert torch.equal(zero.S, plain.S) and torch.equal(zero.C, plain.C)
    assert zero.costs_c == plain.costs_c and zero.costs_s == plain.costs_s
    assert zero.polish_smooth is None and plain.polish_smooth is None
    res = qmc.solve(*args, polish_smooth=3, **kw)
    assert torch.equal(res.C, plain.C) and res.polish_smooth.S is None
    assert res.polish_smooth.sweeps == 3
    ridge = qmc.default_confidence_ridge(plain.S, 100.0)
    m = dict(sr.model_of(d), C=plain.C.double().cpu().numpy())
    F = lambda S: ssr.objective(S.reshape(R, P).double().cpu().numpy(), I, J, m, ridge, 0.1)
    F_plain, F_pol = F(plain.S), F(res.S)
    print("objective at the solver's S", F_plain, "polished", F_pol, res.polish_smooth.objective)
    assert np.isclose(res.polish_smooth.objective, F_pol, rtol=1e-5)
    assert F_pol < F_plain
    with pytest.raises(ValueError):
        qmc.solve(*args, polish_smooth=3, **dict(kw, smooth=0.0))
