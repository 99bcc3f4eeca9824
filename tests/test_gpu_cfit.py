"""GPU: the per-bin projected Newton fit of C for known S -- qsc_cfit_begin / _iterate / _finish,
qmc.fit_C and solve(polish_c=...) -- against the numpy reference of tests/cfit_ref.py.

Shapes (tests/test_gpu_sfit.py's): 9 x 15 pixels with tile 64 (Pp = 192: three tiles, 57 padding
positions), K = 37 / 70 (one and two k-slices, 27 / 58 empty padding bins), R = 3 / 8 / 16, the
five layouts / models of sfit_ref.CASES (one-bit signed rows, 4-bin code field, wide 16-bin, log
model, logit), bin 0 unobserved, S = S_true ~ U(0.2, 1); ridge 1e-2 and 1; max_steps = 40.

Bounds.  One step from C_init: max relative error against the fp64 reference step within
max(1e-5, 10 floor), floor the error of the fp32 numpy reference step on the same inputs.
Minimiser: against the fp64 reference run to tol = 1e-12 (300 steps) within 10 floor, floor the
error of the fp32 reference's own converged result (40 steps, default tol) against that target.
The fp32 reference evaluates f in fp32, so its accept test stops it short of the minimiser; the
kernel sums f in fp64 and lands inside that floor (DESIGN.md section 7m has the measured
figures).  std_C: against the fp64 Cholesky inverse at the returned C within max(1e-5, 10 floor),
floor the same computation in fp32 (tests/test_gpu_info.py's rule).  f at C_init: 8 fp32 ulps of
f (the device forms the link scale and the edges in fp32).  The unobserved bin is left out of the
relative errors (its exact value is 0 or C_init) and checked on its own; a check of "exactly 0
with a ridge" starts from zeros, since from C_init = 1 (the log model's default) the damped step
c <- c mu / (ridge + mu) only approaches 0.  List order, tile size and the cross-tile fold (a
layout with more tiles than tile groups) are checked on f at C_init, which every layout sums in
fp64 from the same terms: agreement to 2 n 2^-53 for n terms, where a dropped or doubled entry
would show at 1 / n.
"""
import ctypes

import numpy as np
import pytest
import torch

import cfit_ref as cr

pytestmark = pytest.mark.gpu

P, TILE, STEPS = cr.P, cr.TILE, cr.MAX_STEPS
_OBS, _REF = {}, {}
ULP = 2.0 ** -23


def observations(name, schedule=None, tile=TILE):
    from quantized_spectrum_cartography_amd.obs import Observations
    key = (name, schedule, tile)
    if key not in _OBS:
        d = cr.problem(name)
        _OBS[key] = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], offset=d["offset"],
                                 log_model=d["log_model"], tile=tile, R_hint=d["R"], loss=d["loss"],
                                 schedule=schedule)
    return _OBS[key]


def start(d, what):
    if what == "default":
        return cr.default_start(d)
    if what == "zeros":
        return np.zeros((d["R"], d["K"]))
    return 0.8 * d["C"].double().numpy()  # "near"


def reference(name, ridge, what, dtype, **kw):
    """cr.fit, computed once per key and left unchanged."""
    key = (name, ridge, what, dtype, tuple(sorted(kw.items())))
    if key not in _REF:
        d = cr.problem(name)
        r = cr.fit(start(d, what), ridge=ridge, dtype=dtype, **cr.model_of(d), **kw)
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def target(name, ridge, project=True):
    return reference(name, ridge, "default", np.float64, max_steps=300, tol=1e-12, project=project)


def raw_fit(obs, d, C0, ridge, max_steps=STEPS, tol=1e-5, mu0=1e-3, project=True, std=False,
            sync_every=4, alias=False):
    """The three calls through qmc._fit_c_pos with the defaults of fit_C: numpy C (R, K), f (K,),
    steps (K,), the counters, and the device tensors."""
    from quantized_spectrum_cartography_amd import qmc
    R = d["R"]
    kind = "expected" if d["log_model"] else "observed"
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = torch.as_tensor(C0, dtype=torch.float32).cuda().contiguous()
    C_out, f, steps, counters, std_C = qmc._fit_c_pos(
        obs, S_pos, Cd, R, kind, ridge, max_steps, tol, mu0, project, std=std,
        sync_every=sync_every, C_out=Cd if alias else None)
    unconv, unident = counters.tolist()
    return dict(C=C_out.double().cpu().numpy(), f=f.cpu().numpy(), steps=steps.cpu().numpy(),
                unconverged=unconv, unidentified=unident, C_dev=C_out, f_dev=f, steps_dev=steps,
                std=None if std_C is None else std_C.double().cpu().numpy())


def max_rel(a, b):
    """Relative error where the reference is not 0; where it is exactly 0 (an entry at the bound)
    the absolute error, C being of order 1."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    z = b == 0
    return float(np.max(np.where(z, np.abs(a - b), np.abs(a - b) / np.where(z, 1.0, np.abs(b)))))


def observed(d):
    return cr.observed_bins(d["Wx"].reshape(d["K"], P).numpy())


# ---------------------------------------------------------------------------------------
# (i) one projected Newton step
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", cr.RIDGES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_one_newton_step_vs_reference(name, ridge):
    d = cr.problem(name)
    obs = observations(name)
    assert obs.Pp == 192 and obs.desc.ntiles == 3 and obs.desc.nks == (1 if d["K"] == 37 else 2)
    assert bool(obs.desc.wide) == (d["nbins"] > 15)
    if name == "onebit16":
        assert obs.desc.rowfmt == 1, "the one-bit linear case is meant to run on signed rows"
    o = observed(d)
    r64 = reference(name, ridge, "near", np.float64, max_steps=1, mu0=0.0)
    r32 = reference(name, ridge, "near", np.float32, max_steps=1, mu0=0.0)
    floor = max_rel(r32["C"][:, o], r64["C"][:, o])
    tol = max(1e-5, 10 * floor)
    g = raw_fit(obs, d, start(d, "near"), ridge, max_steps=1, mu0=0.0)
    e = max_rel(g["C"][:, o], r64["C"][:, o])
    print("case", name, "ridge", ridge, "one step", e, "floor", floor, "tol", tol)
    assert not np.isnan(g["C"]).any() and (g["steps"][o] == 1).all()
    assert e <= tol


# ---------------------------------------------------------------------------------------
# (ii) the minimiser, with and without the bound
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", cr.RIDGES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_minimiser_vs_reference(name, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d = cr.problem(name)
    m = cr.model_of(d)
    obs = observations(name)
    o = observed(d)
    R, K = d["R"], d["K"]
    mn = target(name, ridge)
    r32 = reference(name, ridge, "default", np.float32, max_steps=STEPS)
    floor = max_rel(r32["C"][:, o], mn["C"][:, o])
    g_floor = np.abs(cr.gradient_fp64(r32["C"], ridge=ridge, **m)[:, o]).max()
    res = qmc.fit_C(obs, d["S"], ridge=ridge, max_steps=STEPS)
    C = res.C.double().cpu().numpy()
    e = max_rel(C[:, o], mn["C"][:, o])
    gn = np.abs(cr.gradient_fp64(C, ridge=ridge, **m)[:, o]).max()
    steps = res.steps.cpu().numpy()
    at_zero = (mn["C"] == 0) & o[None, :]
    print("case", name, "ridge", ridge, "C error", e, "floor", floor, "projected gradient", gn,
          "of the fp32 reference", g_floor, "steps max", int(steps.max()), "hist",
          np.bincount(steps).tolist(), "held at 0", int(at_zero.sum()))
    assert tuple(res.C.shape) == (R, K) and tuple(res.steps.shape) == (K,)
    assert torch.isfinite(res.C).all() and np.isfinite(res.nll) and (res.C >= 0).all()
    assert res.unconverged == 0 and res.unidentified == 0 and res.std_C is None
    assert e <= 10 * floor
    # what the fp64 minimiser holds at the bound comes back as exactly 0
    assert (C[at_zero] == 0).all()
    # the NLL at C without the ridge term (fp64 reference at the returned C)
    f64, _, _ = cr.evaluate(C, ridge=0.0, kind="observed", **m)
    assert np.isclose(res.nll, f64.sum(), rtol=1e-5)


@pytest.mark.parametrize("ridge", cr.RIDGES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_without_the_bound_the_fit_matches_the_unprojected_reference(name, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d = cr.problem(name)
    obs = observations(name)
    o = observed(d)
    mn = target(name, ridge, project=False)
    r32 = reference(name, ridge, "default", np.float32, max_steps=STEPS, project=False)
    floor = max_rel(r32["C"][:, o], mn["C"][:, o])
    res = qmc.fit_C(obs, d["S"], ridge=ridge, max_steps=STEPS, project=False)
    C = res.C.double().cpu().numpy()
    e = max_rel(C[:, o], mn["C"][:, o])
    print("case", name, "ridge", ridge, "unprojected C error", e, "floor", floor, "negative entries",
          int((mn["C"] < 0).sum()))
    assert res.unconverged == 0 and e <= 10 * floor


@pytest.mark.parametrize("name", list(cr.CASES))
def test_f_is_monotone_in_max_steps(name):
    d = cr.problem(name)
    m = cr.model_of(d)
    obs = observations(name)
    ridge = 1e-2
    C0 = start(d, "default")
    f0, _, _ = cr.evaluate(C0, ridge=ridge, kind=cr.sr.default_kind(d["log_model"]), **m)
    prev = f0 + 8 * ULP * np.abs(f0)
    for n in (1, 2, 3, 5):
        g = raw_fit(obs, d, C0, ridge, max_steps=n)
        assert np.isfinite(g["f"]).all()
        assert (g["f"] <= prev).all(), (n, np.max(g["f"] - prev))
        assert (g["steps"] <= n).all()
        prev = g["f"]


# ---------------------------------------------------------------------------------------
# (iii) structure, determinism, graphs, list order, tiles
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cr.CASES))
def test_structure_and_determinism(name):
    from quantized_spectrum_cartography_amd import qmc
    d = cr.problem(name)
    obs = observations(name)
    R, K = d["R"], d["K"]
    assert int((obs.perm < 0).sum()) == obs.Pp - P == 57
    assert 64 * obs.desc.nks - K in (27, 58)
    a = raw_fit(obs, d, start(d, "zeros"), 1e-2)
    # the unobserved bin with a ridge: exactly 0, converged at once, counted nowhere
    assert (a["C"][:, 0] == 0).all() and a["f"][0] == 0 and a["steps"][0] == 1
    assert a["unidentified"] == 0 and a["unconverged"] == 0
    assert not np.isnan(a["C"]).any() and not np.isnan(a["f"]).any()
    # two calls, every sync_every, and C_out aliasing C_init: the same bits
    runs = [raw_fit(obs, d, start(d, "zeros"), 1e-2, sync_every=s) for s in (4, 0, 1)]
    runs.append(raw_fit(obs, d, start(d, "zeros"), 1e-2, alias=True))
    for b in runs:
        for k in ("C_dev", "f_dev", "steps_dev"):
            assert torch.equal(a[k], b[k]), k
        assert (a["unconverged"], a["unidentified"]) == (b["unconverged"], b["unidentified"])
    # without a ridge the unobserved bin returns C_init and is counted once; no NaN
    C1 = np.full((R, K), 0.5)
    e = raw_fit(obs, d, C1, 0.0, max_steps=2, std=True)
    assert (e["C"][:, 0] == 0.5).all() and e["unidentified"] == 1
    assert not np.isnan(e["C"]).any() and not np.isnan(e["std"]).any()
    assert np.isinf(e["std"][:, 0]).all()  # its block is not positive definite: +inf, not NaN
    # the sequence captured in a hipGraph and replayed: the bits of the eager run
    kind = "expected" if d["log_model"] else "observed"
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = torch.zeros((R, K), dtype=torch.float32, device="cuda")
    run = lambda: qmc._fit_c_pos(obs, S_pos, Cd, R, kind, 1e-2, 6, 1e-5, 1e-3, True, std=True,
                                 sync_every=0)
    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = run()
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, out):
        assert torch.equal(x, y)


def f_at(obs, R, S, C0, kind, ridge=0.0):
    """f_k(C0) (K,) fp64 on the device: qsc_cfit_begin's walk at C_init settled by qsc_cfit_finish
    with no step in between (every sum of f is fp64, so layouts differ by fp64 rounding only)."""
    from quantized_spectrum_cartography_amd import _lib, qmc
    L, p, cf = _lib.lib(), _lib.ptr, ctypes.c_float
    desc, _, ent = obs.layout(R)
    S_pos = obs.to_positions(S.reshape(R, -1))
    Cd = torch.as_tensor(C0, dtype=torch.float32).cuda().contiguous()
    nws = int(L.qsc_cfit_workspace_bytes(desc, R))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    C_out = torch.empty_like(Cd)
    f = torch.empty(obs.K, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    _lib.call("qsc_cfit_begin", desc, p(ent), p(obs.c_width), p(obs.c_off), p(obs.c_kmap),
              obs.model, R, p(S_pos), p(Cd), qmc.INFO_KINDS[kind], cf(ridge), cf(1e-3), cf(1e-5), 1,
              1, p(ws), nws, _lib.stream())
    _lib.call("qsc_cfit_finish", desc, obs.model, R, p(C_out), p(f), None, None, p(cnt[0:1]),
              p(cnt[1:2]), p(ws), nws, _lib.stream())
    assert torch.equal(C_out, Cd)
    return f.cpu().numpy()


@pytest.mark.parametrize("name", list(cr.CASES))
def test_list_order_and_tile_size_change_nothing_but_the_order_of_the_sums(name):
    """Scheduled / natural list order and tile 64 / 128 (other padding positions, other tiles,
    other bin orders) are the same problem.  (a) f at C_init is a sum of fp64 terms of the same
    fp32 inputs, so the layouts agree to the rounding of an fp64 sum, n 2^-53 relative for n terms
    (a dropped or doubled entry changes f by 1 / n of itself).  (b) One step from 0.8 C_true: each
    layout within the one-step bound max(1e-5, 10 floor) of the fp64 step.  (c) The converged
    results: each within 10 floor of the fp64 minimiser, and of one another within the sum of their
    own measured distances from it plus 4 fp32 ulps."""
    d = cr.problem(name)
    m = cr.model_of(d)
    R, ridge = d["R"], 1e-2
    o = observed(d)
    kind = cr.sr.default_kind(d["log_model"])
    layouts = {"scheduled": observations(name), "natural": observations(name, schedule=False),
               "tile128": observations(name, tile=128)}
    assert layouts["scheduled"].schedule and not layouts["natural"].schedule
    assert layouts["tile128"].desc.ntiles == 2 and layouts["tile128"].Pp == 256
    # (a) f at C_init
    C0 = start(d, "near")
    f64, _, _ = cr.evaluate(C0, ridge=0.0, kind=kind, **m)
    fs = {k: f_at(v, R, d["S"], C0, kind) for k, v in layouts.items()}
    n_terms = int((m["Wx"] != 0).sum(axis=1).max())
    for k, f in fs.items():
        assert np.isfinite(f).all() and f[0] == 0
        dev = np.abs(f - fs["scheduled"]).max() / np.abs(fs["scheduled"]).max()
        print("case", name, k, "f at C_init against scheduled", dev, "against fp64 numpy",
              np.abs(f - f64).max() / np.abs(f64).max())
        assert dev <= 2 * n_terms * 2.0 ** -53  # (two orders of an n-term fp64 sum)
        assert np.allclose(f, f64, rtol=8 * ULP, atol=0)  # (the device's link scale is fp32)
    # (b) one step
    r64 = reference(name, ridge, "near", np.float64, max_steps=1, mu0=0.0)
    r32 = reference(name, ridge, "near", np.float32, max_steps=1, mu0=0.0)
    tol1 = max(1e-5, 10 * max_rel(r32["C"][:, o], r64["C"][:, o]))
    for k, v in layouts.items():
        g = raw_fit(v, d, C0, ridge, max_steps=1, mu0=0.0)
        e = max_rel(g["C"][:, o], r64["C"][:, o])
        print("case", name, k, "one step", e, "tol", tol1)
        assert e <= tol1
    # (c) the converged results
    mn = target(name, ridge)
    r32 = reference(name, ridge, "default", np.float32, max_steps=STEPS)
    bound = 10 * max_rel(r32["C"][:, o], mn["C"][:, o])
    runs = {k: raw_fit(v, d, start(d, "default"), ridge) for k, v in layouts.items()}
    err = {k: np.abs(v["C"][:, o] - mn["C"][:, o]).max() for k, v in runs.items()}
    print("case", name, "distance from the minimiser", err, "bound (relative)", bound)
    for k, v in runs.items():
        assert max_rel(v["C"][:, o], mn["C"][:, o]) <= bound
        assert v["unconverged"] == 0 and v["unidentified"] == 0
        for k2, v2 in runs.items():
            pair = np.abs(v["C"][:, o] - v2["C"][:, o]).max()
            assert pair <= err[k] + err[k2] + 4 * ULP * np.abs(mn["C"]).max(), (k, k2, pair)
        if not d["log_model"]:
            assert (v["C"][:, 0] == 0).all()


# ---------------------------------------------------------------------------------------
# (iii-b) more tiles than groups: the cross-tile fold
# ---------------------------------------------------------------------------------------
_MANY = {}


def many_tiles_problem():
    """220 x 320 pixels, K = 3, R = 2, one-bit probit, rate 0.5 (the smallest shape with more
    tiles than groups): at tile 64 the layout has 1100 tiles, more than the 1024 groups the library
    forms, so the split is uneven -- 76 workgroups walk 2 tiles and fold the second into the
    partial rows of the first (the bins sit on other lanes there), 948 walk one; at tile 1024 it
    has 69 tiles and as many groups (no fold)."""
    if not _MANY:
        from oracle import reference_ops as ro
        R, K, I, J = 2, 3, 220, 320
        g = torch.Generator().manual_seed(31)
        S = 0.2 + 0.8 * torch.rand(R, 1, I, J, generator=g)
        C = 0.1 + 0.9 * torch.rand(R, K, generator=g)
        T = ro.get_tensor(S, C)
        b = torch.tensor([0.0, float(T.median()), float(T.max()) + 1.0])
        Y = ro.quantize(T, 0.5, b, noise=torch.randn(T.shape, generator=g)).unsqueeze(1)
        Wx = torch.bernoulli(torch.full((K, 1, I, J), 0.5), generator=g)
        _MANY.update(name="many", R=R, K=K, S=S, C=C, Y=Y, Wx=Wx, b=b, sigma=0.5, offset=0.0,
                     log_model=False, loss="probit", nbins=2)
    return _MANY


def test_more_tiles_than_groups_fold_across_tiles():
    from quantized_spectrum_cartography_amd import _lib
    from quantized_spectrum_cartography_amd.obs import Observations
    d = many_tiles_problem()
    m = cr.model_of(d)
    R, K, ridge = d["R"], d["K"], 1e-2
    mk = lambda tile: Observations(d["Y"], d["Wx"], d["b"], d["sigma"], tile=tile, R_hint=R)
    small, big = mk(64), mk(1024)
    L = _lib.lib()
    assert small.desc.ntiles == 1100 and L.qsc_cfit_groups(small.desc, R) == 1024
    assert big.desc.ntiles == 69 and L.qsc_cfit_groups(big.desc, R) == 69
    # f at C_init: the folded partials against the unfolded ones and against fp64 numpy
    C0 = 0.8 * d["C"].double().numpy()
    f64, _, _ = cr.evaluate(C0, ridge=0.0, kind="observed", **m)
    fa, fb = f_at(small, R, d["S"], C0, "observed"), f_at(big, R, d["S"], C0, "observed")
    n_terms = int((m["Wx"] != 0).sum(axis=1).max())
    dev = np.abs(fa - fb).max() / np.abs(fb).max()
    print("many tiles: f folded against unfolded", dev, "terms", n_terms, "against fp64 numpy",
          np.abs(fa - f64).max() / np.abs(f64).max())
    assert dev <= 2 * n_terms * 2.0 ** -53  # (two orders of an n-term fp64 sum)
    assert np.allclose(fa, f64, rtol=8 * ULP, atol=0)
    # one step and the converged result against the reference; two calls bit for bit
    C1 = np.zeros((R, K))
    r64 = cr.fit(C0, ridge=ridge, max_steps=1, mu0=0.0, **m)
    r32 = cr.fit(C0, ridge=ridge, max_steps=1, mu0=0.0, dtype=np.float32, **m)
    tol1 = max(1e-5, 10 * max_rel(r32["C"], r64["C"]))
    mn = cr.fit(C1, ridge=ridge, max_steps=300, tol=1e-12, **m)
    r32 = cr.fit(C1, ridge=ridge, max_steps=STEPS, dtype=np.float32, **m)
    bound = 10 * max_rel(r32["C"], mn["C"])
    runs = {}
    for k, obs in (("tile64", small), ("tile1024", big)):
        e1 = max_rel(raw_fit(obs, d, C0, ridge, max_steps=1, mu0=0.0)["C"], r64["C"])
        a = raw_fit(obs, d, C1, ridge)
        b2 = raw_fit(obs, d, C1, ridge, sync_every=0)
        for key in ("C_dev", "f_dev", "steps_dev"):
            assert torch.equal(a[key], b2[key]), key
        e = max_rel(a["C"], mn["C"])
        print("many tiles:", k, "one step", e1, "tol", tol1, "C error", e, "bound", bound,
              "steps max", int(a["steps"].max()))
        assert e1 <= tol1 and e <= bound and a["unconverged"] == 0 and a["unidentified"] == 0
        runs[k] = a
    err = {k: np.abs(v["C"] - mn["C"]).max() for k, v in runs.items()}
    pair = np.abs(runs["tile64"]["C"] - runs["tile1024"]["C"]).max()
    assert pair <= err["tile64"] + err["tile1024"] + 4 * ULP * np.abs(mn["C"]).max()


# ---------------------------------------------------------------------------------------
# (iv) std_C
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", cr.RIDGES)
@pytest.mark.parametrize("name", list(cr.CASES))
def test_std_c_vs_fp64_cholesky_inverse(name, ridge):
    from quantized_spectrum_cartography_amd import qmc
    d = cr.problem(name)
    m = cr.model_of(d)
    obs = observations(name)
    kind = cr.sr.default_kind(d["log_model"])
    res = qmc.fit_C(obs, d["S"], ridge=ridge, max_steps=STEPS, std=True)
    C = res.C.double().cpu().numpy()
    s64 = cr.std_fp64(C, kind=kind, ridge=ridge, **m)
    s32 = cr.std_fp64(C, kind=kind, ridge=ridge, dtype=np.float32, **m)
    floor = max_rel(s32, s64)
    tol = max(1e-5, 10 * floor)
    e = max_rel(res.std_C.double().cpu().numpy(), s64)
    print("case", name, "ridge", ridge, "std_C error", e, "floor", floor, "tol", tol)
    assert tuple(res.std_C.shape) == (d["R"], d["K"]) and torch.isfinite(res.std_C).all()
    assert e <= tol
    # the unobserved bin: J = 0, so the prior's 1 / sqrt(ridge)
    assert np.allclose(res.std_C[:, 0].cpu().numpy(), ridge ** -0.5, rtol=1e-6)


def test_abi_rejects_what_it_cannot_compute():
    from quantized_spectrum_cartography_amd import _lib
    from quantized_spectrum_cartography_amd.obs import Observations
    L = _lib.lib()
    d = cr.problem("bins16")
    R = d["R"]
    obs = observations("bins16")
    S_pos = obs.to_positions(d["S"].reshape(R, -1))
    Cd = d["C"].cuda().contiguous()
    p, cf = _lib.ptr, ctypes.c_float

    def begin(o=obs, kind=1, ridge=0.1, mu0=1e-3, tol=1e-5, max_steps=2, short=0):
        desc, _, ent = o.layout(R)
        nws = int(L.qsc_cfit_workspace_bytes(desc, R))
        assert nws > 0
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
        return L.qsc_cfit_begin(desc, p(ent), p(o.c_width), p(o.c_off), p(o.c_kmap), o.model, R,
                                p(S_pos), p(Cd), kind, cf(ridge), cf(mu0), cf(tol), max_steps, 1,
                                p(ws), nws - short, None)

    assert begin() == 0
    sq = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], tile=TILE, R_hint=R, loss="squared")
    assert begin(o=sq) == _lib.QSC_EINVAL  # the squared loss is not a likelihood
    assert begin(kind=2) == _lib.QSC_EINVAL
    assert begin(ridge=-1.0) == _lib.QSC_EINVAL and begin(mu0=-1.0) == _lib.QSC_EINVAL
    assert begin(tol=0.0) == _lib.QSC_EINVAL and begin(max_steps=0) == _lib.QSC_EINVAL
    assert begin(short=1) == _lib.QSC_EINVAL
    # a tile whose S rows do not fit the LDS at this rank (a descriptor only: nothing is launched)
    desc = _lib.QscObsDesc()
    ctypes.memmove(ctypes.byref(desc), ctypes.byref(obs.desc), ctypes.sizeof(desc))
    desc.wide, desc.PT, desc.ntiles, desc.Pp = 1, 64 * 1024, 1, 64 * 1024
    nws = int(L.qsc_cfit_workspace_bytes(desc, R))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    wide = observations("bins16")
    assert wide.desc.wide
    rc = L.qsc_cfit_begin(desc, p(wide.c_entries), p(obs.c_width), p(obs.c_off), p(obs.c_kmap),
                          obs.model, R, p(S_pos), p(Cd), 1, cf(0.1), cf(1e-3), cf(1e-5), 2, 1, p(ws),
                          nws, None)
    assert rc == _lib.QSC_EUNSUPPORTED
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# (v) solve(polish_c=...)
# ---------------------------------------------------------------------------------------
def test_solve_polish_c_runs_fit_c_on_the_result_and_zero_changes_nothing():
    from quantized_spectrum_cartography_amd import qmc
    d = cr.problem("logit")  # the small one-bit case (R = 3, K = 37)
    R, K = d["R"], d["K"]
    m = cr.model_of(d)
    g = torch.Generator().manual_seed(5)
    S0 = 0.2 + 0.5 * torch.rand(R, 1, cr.I, cr.J, generator=g)
    C0 = 0.1 + 0.5 * torch.rand(R, K, generator=g)
    kw = dict(S_init=S0, C_init=C0, max_iter=3, tile=TILE, loss="logit")
    args = (d["Y"], d["Wx"], d["b"], d["sigma"])
    plain = qmc.solve(*args, **kw)
    zero = qmc.solve(*args, polish_c=0, **kw)
    assert torch.equal(zero.S, plain.S) and torch.equal(zero.C, plain.C)
    assert zero.costs_c == plain.costs_c and zero.costs_s == plain.costs_s
    assert zero.polish_c is None and plain.polish_c is None
    res = qmc.solve(*args, polish_c=5, **kw)
    assert torch.equal(res.S, plain.S) and res.costs_c == plain.costs_c
    obs = observations("logit")
    ridge = qmc.default_confidence_ridge(plain.C, 100.0)
    fit = qmc.fit_C(obs, plain.S, C_init=plain.C, ridge=ridge, max_steps=5, project=True)
    assert torch.equal(res.C, fit.C)
    assert res.polish_c.C is None and res.polish_c.nll == fit.nll
    assert torch.equal(res.polish_c.steps, fit.steps)
    # the polished NLL against the unpolished C at the same S (fp64 reference, no ridge term)
    m = dict(m, S=plain.S.reshape(R, P).double().cpu().numpy())
    f_plain, _, _ = cr.evaluate(plain.C.double().cpu().numpy(), ridge=0.0, **m)
    f_pol, _, _ = cr.evaluate(res.C.double().cpu().numpy(), ridge=0.0, **m)
    print("nll unpolished", f_plain.sum(), "polished", res.polish_c.nll, "ridge", ridge)
    assert np.isclose(res.polish_c.nll, f_pol.sum(), rtol=1e-5)
    assert res.polish_c.nll <= f_plain.sum()
    # polish_s after polish_c fits S at the polished C
    both = qmc.solve(*args, polish_c=5, polish_s=5, **kw)
    assert torch.equal(both.C, res.C) and both.polish is not None and both.polish_c is not None
    fs = qmc.fit_S(obs, res.C, S_init=plain.S, ridge=qmc.default_confidence_ridge(plain.S, 100.0),
                   max_steps=5)
    assert torch.equal(both.S, fs.S)
