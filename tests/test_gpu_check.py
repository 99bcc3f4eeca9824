"""GPU: per-sensor goodness of fit and level-shift score tests -- qsc_scheck, qsc_entry_check,
qmc.check_fit and solve(check=True) -- against the fp64 reference of tests/check_ref.py.

Shapes: I x J = 10 x 13 (P = 130) with tile 64: Pp = 192, six slices, 62 padding positions;
R = 2 / 5 / 11 (rank pads 4 / 8 / 16) at K = 21 / 21 / 40; sampling rate 0.7; one wide case
(K = 4100, P = 64).  Planted positions: pixel 0 has no readings, pixel 1 a single one (n < R),
pixel 2 (log model) a row of S with mixed signs so that some t + offset <= 0, pixel 3 (linear
model) a huge S and one reading of the opposite code, whose P underflows.  Inputs: S ~ U(0.2, 1)
(log model: U(3, 10), so that with the ridge I* / Ixx lies above the guard's window),
C ~ U(0.1, 1), thresholds at the quantiles of the map, codes drawn from the model.

Tolerance: max|got - ref| / max|ref| per statistic over the positions where the reference is
testable (D, V: valid), held to max(1e-5, 10 floor) -- the bound of tests/test_gpu_design.py --
floor the same metric of the fp32 evaluation check_ref.stats(dtype=float32).  n must be equal
everywhere; the flag words wherever the reference's I* / Ixx lies outside [1e-5, 1e-3] and no
small pivot meets a large ratio: at most 2 % of the positions (3 of 130) may be left out, and the
test asserts the count (1 position in bins4_11 at ridge 1e-2, 0 in every other case).  DESIGN.md section 7u has the measured errors.
"""
import numpy as np
import pytest
import torch

import check_ref as cr

pytestmark = pytest.mark.gpu

TILE = 64
RIDGES = [0.0, 1e-2]

# name: (R, K, I, J, model, loss, sigma, rate, packing, seed)
CASES = {
    "onebit2": (2, 21, 10, 13, "onebit", "probit", 0.4, 0.7, "dense", 1),
    "logit5": (5, 21, 10, 13, "onebit", "logit", 0.3, 0.7, "dense", 2),
    "bins4_11": (11, 40, 10, 13, "bins4", "probit", 0.5, 0.7, "dense", 3),
    "log4_5": (5, 21, 10, 13, "log4", "probit", 0.5, 0.7, "dense", 4),
    "logit_log4_2": (2, 21, 10, 13, "log4", "logit", 0.3, 0.7, "dense", 5),
    "readings11": (11, 40, 10, 13, "onebit", "probit", 0.6, 0.5, "readings", 6),
    "wide": (2, 4100, 8, 8, "bins4", "probit", 0.5, 0.02, "dense", 7),
}
_PROB, _REF, _OBS = {}, {}, {}


def draw_codes(g, x, b, sigma, loss, log_model):
    """Codes of x + noise against the interior edges (the outer ones: clamped, or set wide)."""
    if loss == "logit":
        u = g.random(x.shape)
        noise = sigma * (np.log(u) - np.log1p(-u))
    else:
        noise = sigma * g.standard_normal(x.shape)
    return np.searchsorted(np.asarray(b[1:-1], np.float64), x + noise).astype(np.int64)


def problem(name):
    """Inputs of a case (numpy; fp32-representable S, C and edges), built once."""
    if name in _PROB:
        return _PROB[name]
    R, K, I, J, model, loss, sigma, rate, packing, seed = CASES[name]
    P = I * J
    g = np.random.default_rng(seed)
    log_model = model == "log4"
    offset = 1e-3 if log_model else 0.0
    S = (3.0 + 7.0 * g.random((R, P)) if log_model else 0.2 + 0.8 * g.random((R, P)))
    C = 0.1 + 0.9 * g.random((R, K))
    S, C = S.astype(np.float32).astype(np.float64), C.astype(np.float32).astype(np.float64)
    T = C.T @ S
    x = np.log(T + offset) if log_model else T
    if model == "onebit":
        b = [0.0, float(np.median(T)), float(T.max()) + 1.0]
    elif model == "bins4":
        q = np.quantile(T, [0.25, 0.5, 0.75])
        b = [0.0, float(q[0]), float(q[1]), float(q[2]), float(T.max()) + 1.0]
    else:
        q = np.quantile(x, [0.25, 0.5, 0.75])
        b = [-23.025850296020508, float(q[0]), float(q[1]), float(q[2]), float(x.max()) + 0.5]
    b = [float(np.float32(v)) for v in b]
    Y = draw_codes(g, x, b, sigma, loss, log_model)
    Wx = (g.random((K, P)) < rate)
    planted = {}
    if P == 130:
        Wx[:, 0] = False                      # no readings
        Wx[:, 1] = False
        Wx[3, 1] = True                       # a single reading: n < R
        planted = {"empty": 0, "single": 1}
        if log_model:
            S[:, 2] = np.where(np.arange(R) % 2 == 0, -1.0, 1.0)  # t = sum +-c: both signs
            Wx[:, 2] = True
            planted["negative"] = 2
        else:
            S[:, 3] = 2000.0                  # every edge saturated; one reading says code 0
            Wx[:, 3] = True
            Y[:, 3] = len(b) - 2
            Y[5, 3] = 0
            planted["underflow"] = 3
    k, p = np.nonzero(Wx)
    y = Y[k, p]
    if packing == "readings":
        # every fifth cell is read twice more, with codes of their own
        rep = np.arange(len(k)) % 5 == 0
        k2, p2 = np.repeat(k[rep], 2), np.repeat(p[rep], 2)
        y2 = draw_codes(g, x[k2, p2], b, sigma, loss, log_model)
        k, p, y = np.concatenate([k, k2]), np.concatenate([p, p2]), np.concatenate([y, y2])
    d = dict(name=name, R=R, K=K, I=I, J=J, P=P, S=S, C=C, Y=Y, Wx=Wx, k=k, p=p, y=y, b=b,
             sigma=sigma, offset=offset, log_model=log_model, loss=loss, packing=packing,
             planted=planted, model=(b, sigma, offset, log_model, loss))
    _PROB[name] = d
    return d


def reference(name, fitted, ridge, dtype=np.float64):
    """check_ref.stats of a case, computed once per (case, fitted, ridge, dtype), read-only."""
    key = (name, fitted, ridge, np.dtype(dtype).name)
    if key not in _REF:
        d = problem(name)
        st = cr.stats(d["S"], d["C"], d["k"], d["p"], d["y"], *d["model"], fitted=bool(fitted),
                      ridge=ridge, dtype=dtype)
        for v in st.values():
            v.setflags(write=False)
        _REF[key] = st
    return _REF[key]


def excluded(ref):
    """Positions whose flag word is not compared: I* / Ixx inside the guard's window
    [1e-5, 1e-3], or a pivot within 1e-5 of the threshold together with a ratio above the
    window (a rank-deficient block, whose ratio is rounding noise below it, is compared)."""
    r = ref["ratio"]
    return ((r >= 1e-5) & (r <= 1e-3)) | ((np.abs(ref["minpiv"]) < 1e-5) & (r > 1e-3))


def observations(name):
    from quantized_spectrum_cartography_amd.obs import Observations
    if name not in _OBS:
        d = problem(name)
        K, I, J = d["K"], d["I"], d["J"]
        kw = dict(offset=d["offset"], log_model=d["log_model"], tile=TILE, R_hint=d["R"],
                  loss=d["loss"])
        if d["packing"] == "readings":
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
            _OBS[name] = Observations.from_readings(t(d["k"]), t(d["p"] // J), t(d["p"] % J),
                                                    t(d["y"]), (K, I, J), torch.tensor(d["b"]),
                                                    d["sigma"], **kw)
        else:
            Y = torch.from_numpy(d["Y"]).reshape(K, 1, I, J)
            Wx = torch.from_numpy(d["Wx"].astype(np.float32)).reshape(K, 1, I, J)
            _OBS[name] = Observations(Y, Wx, torch.tensor(d["b"]), d["sigma"], **kw)
    return _OBS[name]


def tensors(d):
    return (torch.from_numpy(d["S"]).float().reshape(d["R"], 1, d["I"], d["J"]),
            torch.from_numpy(d["C"]).float())


def raw_check(obs, d, fitted, ridge, bufs=None):
    """qsc_scheck through the ABI into NaN- / -1-filled buffers: every element must be written.
    -> (stat (Pp, 4), count (Pp,), flags (Pp,)) in position order."""
    from quantized_spectrum_cartography_amd import fits
    R = d["R"]
    S, C = tensors(d)
    S_pos = obs.to_positions(S.reshape(R, -1))
    Cd = C.cuda().contiguous()
    if bufs is None:
        bufs = (torch.full((obs.Pp, 4), float("nan"), device="cuda"),
                torch.full((obs.Pp,), -1, dtype=torch.int32, device="cuda"),
                torch.full((obs.Pp,), -1, dtype=torch.int32, device="cuda"))
    return fits._check_pos(obs, S_pos, Cd, R, fitted, ridge, *bufs)


def pixels(obs, stat, count, flags):
    ip = obs.iperm().long()
    st = stat[ip].double().cpu().numpy()
    return dict(D=st[:, 0], V=st[:, 1], u=st[:, 2], info=st[:, 3],
                n=count[ip].cpu().numpy().astype(np.int64),
                flags=flags[ip].cpu().numpy().astype(np.int64))


# ---------------------------------------------------------------------------------------
# (i) the case matrix against the reference
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", RIDGES)
@pytest.mark.parametrize("fitted", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_statistics_counts_and_flags_vs_reference(name, fitted, ridge):
    d = problem(name)
    obs = observations(name)
    P = d["P"]
    if name == "wide":
        assert obs.desc.wide == 1 and obs.Pp == 64
    else:
        assert obs.Pp == 192 and int((obs.perm < 0).sum()) == 62
        if d["packing"] == "dense":
            assert obs.desc.rowfmt == (1 if name in ("onebit2", "logit5") else 0)
    if d["packing"] == "readings":
        assert obs.max_repeat == 3
    ref = reference(name, fitted, ridge)
    flo = reference(name, fitted, ridge, np.float32)
    stat, count, flags = raw_check(obs, d, fitted, ridge)
    assert not torch.isnan(stat).any() and (count >= 0).all() and (flags >= 0).all()
    pads = obs.perm < 0
    assert (stat[pads] == 0).all() and (count[pads] == 0).all() and (flags[pads] == 0).all()
    got = pixels(obs, stat, count, flags)
    # the integers
    assert np.array_equal(got["n"], ref["n"])
    ex = excluded(ref)
    print("case", name, "fitted", fitted, "ridge", ridge, "flag words not compared:", int(ex.sum()),
          "of", P, "untestable", int((ref["flags"] & 1 != 0).sum()))
    assert ex.sum() <= 0.02 * P
    assert np.array_equal(got["flags"][~ex], ref["flags"][~ex])
    # zeros exactly where the rules write them
    inv = ref["flags"] & cr.INVALID != 0
    unt = (ref["flags"] & cr.UNTESTABLE != 0) & ~ex
    for key in ("D", "V", "u", "info"):
        assert (got[key][inv] == 0).all()
    assert (got["u"][unt] == 0).all() and (got["info"][unt] == 0).all()
    # the statistics
    valid = ~inv
    testable = (ref["flags"] & 3 == 0) & (got["flags"] & 3 == 0) & (ref["n"] > 0)
    for key, keep in (("D", valid), ("V", valid), ("u", testable), ("info", testable)):
        if not keep.any() or np.max(np.abs(ref[key][keep])) == 0:
            assert key in ("u", "info") and fitted == 1
            continue
        err = cr.max_err(got[key], ref[key], keep)
        floor = cr.max_err(flo[key], ref[key],
                           keep & (flo["flags"] & (2 if key in ("D", "V") else 3) == 0))
        print("   ", key, "err", err, "floor", floor, "positions", int(keep.sum()))
        assert err <= max(1e-5, 10 * floor)
    # the planted positions
    pl = d["planted"]
    if pl:
        f = got["flags"]
        assert got["n"][pl["empty"]] == 0 and f[pl["empty"]] == (cr.UNTESTABLE if fitted else 0)
        assert all(got[key][pl["empty"]] == 0 for key in ("D", "V", "u", "info"))
        assert got["n"][pl["single"]] == 1
        if fitted and ridge == 0.0:
            assert f[pl["single"]] & cr.UNTESTABLE
            assert got["u"][pl["single"]] == 0 and got["info"][pl["single"]] == 0
        if "negative" in pl:
            q = pl["negative"]
            assert f[q] == cr.INVALID and 0 < got["n"][q] < int(d["Wx"][:, q].sum())
            assert all(got[key][q] == 0 for key in ("D", "V", "u", "info"))
        if "underflow" in pl:
            q = pl["underflow"]
            assert f[q] == cr.SATURATED | (cr.UNTESTABLE if fitted else 0)
            assert got["u"][q] == 0 and got["info"][q] == 0
            assert ref["D"][q] >= -np.log(cr.FLT_MIN) - 1e-9
            assert abs(got["D"][q] - ref["D"][q]) <= 1e-6 * ref["D"][q]


def test_two_calls_agree_bit_for_bit_and_a_graph_replay_equals_the_eager_call():
    from quantized_spectrum_cartography_amd import fits
    name = "bins4_11"
    d = problem(name)
    obs = observations(name)
    R = d["R"]
    a = [t.clone() for t in raw_check(obs, d, 1, 1e-2)]
    b = raw_check(obs, d, 1, 1e-2)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # (the inputs are on the device before the capture: it holds the one launch and nothing else)
    S, C = tensors(d)
    S_pos = obs.to_positions(S.reshape(R, -1))
    Cd = C.cuda().contiguous()
    obs.layout(R)
    bufs = (torch.zeros((obs.Pp, 4), device="cuda"),
            torch.zeros(obs.Pp, dtype=torch.int32, device="cuda"),
            torch.zeros(obs.Pp, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fits._check_pos(obs, S_pos, Cd, R, True, 1e-2, *bufs)
    torch.cuda.current_stream().wait_stream(s)
    for t in bufs:
        t.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, bufs))


def test_check_fit_is_the_raw_call_in_pixel_order():
    from quantized_spectrum_cartography_amd import qmc
    name = "log4_5"
    d = problem(name)
    obs = observations(name)
    S, C = tensors(d)
    r = qmc.check_fit(obs, S, C, fitted=True, ridge=1e-2)
    got = pixels(obs, *raw_check(obs, d, 1, 1e-2))
    I, J = d["I"], d["J"]
    for key, t in (("D", r.D), ("V", r.V), ("u", r.u), ("info", r.info), ("n", r.n),
                   ("flags", r.flags)):
        assert tuple(t.shape) == (I, J)
        assert np.array_equal(t.reshape(-1).double().cpu().numpy(), got[key].astype(np.float64))
    ref = reference(name, 1, 1e-2)
    zf, zs, sh = cr.zscores({k: got[k] for k in ("D", "V", "u", "info")})
    assert np.allclose(r.z_fit.reshape(-1).cpu().numpy(), zf, rtol=1e-5, atol=1e-6)
    assert np.allclose(r.z_shift.reshape(-1).cpu().numpy(), zs, rtol=1e-5, atol=1e-6)
    assert np.allclose(r.shift.reshape(-1).cpu().numpy(), sh, rtol=1e-5, atol=1e-6)
    assert r.invalid == 1 and r.saturated == int((ref["flags"] & 4 != 0).sum())
    assert r.untestable == int((got["flags"] & 1 != 0).sum())
    valid = got["flags"] & 2 == 0
    assert r.z_fit_total == pytest.approx(got["D"][valid].sum() / np.sqrt(got["V"][valid].sum()),
                                          rel=1e-9)
    assert not any(torch.isnan(t).any() for t in (r.z_fit, r.z_shift, r.shift))


# ---------------------------------------------------------------------------------------
# (ii) the elementwise op
# ---------------------------------------------------------------------------------------
# (name, b, sigma, offset, log_model, loss, map values): moderate |z| <= 8.5 and saturated edges
# |z| >= 25 (between them the fp32 P is denormal or 0 where the fp64 one is not)
def _grid(lo, hi, far):
    return np.concatenate([np.linspace(lo, hi, 33), far]).astype(np.float32).astype(np.float64)


ENTRY = [
    ("onebit", [0.0, 1.0, 5.0], 0.4, 0.0, False, "probit",
     _grid(1.0 - 4.5, 1.0 + 4.5, [-40.0, -20.0, 20.0, 40.0])),
    ("logit3", [0.0, 0.5, 1.5, 5.0], 0.25, 0.0, False, "logit",
     _grid(0.5 - 2.0, 1.5 + 2.0, [-200.0, -60.0, 60.0, 200.0])),
    ("log4", [-23.025850296020508, -1.0, 0.0, 1.0, 40.0], 0.5, 1e-3, True, "probit",
     np.concatenate([np.exp(_grid(-5.0, 5.0, [])), [-1.0, -1e-3, -2e-3]])),
]


@pytest.mark.parametrize("case", ENTRY, ids=[c[0] for c in ENTRY])
def test_entry_check_vs_reference_on_a_grid_with_saturated_edges(case):
    from quantized_spectrum_cartography_amd import _lib, utils
    name, b, sigma, offset, log_model, loss, t = case
    nb = len(b) - 1
    T = np.repeat(t.astype(np.float32)[None, :], nb, 0)
    Y = np.repeat(np.arange(nb)[:, None], len(t), 1)
    m = _lib.make_model(b, sigma, offset, log_model, loss=loss)
    out = utils.entry_check(torch.from_numpy(Y).cuda(), torch.from_numpy(T).cuda(), m)
    assert tuple(out.shape) == (5, nb, len(t)) and not torch.isnan(out).any()
    got = out.double().cpu().numpy()
    et = cr.entry_terms(T.astype(np.float64), Y, b, sigma, np.float32(offset), log_model, loss)
    if name != "log4":
        assert et["sat"].any()
    for i, key in enumerate(("dl", "var", "gx", "hx", "dxdt")):
        err = float(np.max(np.abs(got[i] - et[key])) / np.max(np.abs(et[key])))
        print("entry_check", name, key, "err", err)
        assert err <= 1e-5
    assert (got[2][et["sat"]] == 0).all()
    if log_model:
        assert et["neg"].sum() == 3 * nb and (got[:, et["neg"]] == 0).all()


# ---------------------------------------------------------------------------------------
# (iii) what the ABI refuses
# ---------------------------------------------------------------------------------------
def test_abi_rejects_what_it_cannot_compute_and_launches_nothing():
    import ctypes
    from quantized_spectrum_cartography_amd import _lib
    L = _lib.lib()
    name = "onebit2"
    d = problem(name)
    obs = observations(name)
    R = d["R"]
    desc, s_entries, _ = obs.layout(R)
    S, C = tensors(d)
    S_pos = obs.to_positions(S.reshape(R, -1))
    Cd = C.cuda().contiguous()
    stat = torch.full((obs.Pp, 4), float("nan"), device="cuda")
    count = torch.full((obs.Pp,), -1, dtype=torch.int32, device="cuda")
    flags = torch.full((obs.Pp,), -1, dtype=torch.int32, device="cuda")
    p = _lib.ptr

    def scheck(desc_=desc, model=obs.model, R_=R, fitted=1, ridge=0.0, stat_=stat):
        return L.qsc_scheck(desc_, p(s_entries), p(obs.s_width), p(obs.s_off), p(obs.perm), model,
                            R_, p(S_pos), p(Cd), fitted, ctypes.c_float(ridge), p(stat_), p(count),
                            p(flags), None)

    sq = _lib.make_model(d["b"], d["sigma"], loss="squared")
    assert scheck(model=sq) == _lib.QSC_EINVAL
    assert scheck(model=None) == _lib.QSC_EINVAL
    assert scheck(ridge=-1.0) == _lib.QSC_EINVAL
    assert scheck(ridge=float("nan")) == _lib.QSC_EINVAL
    assert scheck(fitted=2) == _lib.QSC_EINVAL and scheck(fitted=-1) == _lib.QSC_EINVAL
    assert scheck(R_=0) == _lib.QSC_EINVAL and scheck(R_=17) == _lib.QSC_EINVAL
    assert scheck(stat_=None) == _lib.QSC_EINVAL
    four = _lib.make_model([0.0, 1.0, 2.0, 3.0, 4.0], d["sigma"])
    assert scheck(model=four) == _lib.QSC_EINVAL        # the layout holds two bins
    # C^T beyond the LDS: at rank 16 a row takes 20 floats, 80 K + 16 bytes against 163840.
    # Refused before any launch: nothing is written and no buffer is read.
    big = _lib.QscObsDesc.from_buffer_copy(desc)
    big.K = 3000
    assert scheck(desc_=big, R_=16) == _lib.QSC_EUNSUPPORTED
    with pytest.raises(_lib.QscError):
        _lib.call("qsc_scheck", big, p(s_entries), p(obs.s_width), p(obs.s_off), p(obs.perm),
                  obs.model, 16, p(S_pos), p(Cd), 1, 0.0, p(stat), p(count), p(flags), None)
    torch.cuda.synchronize()
    assert torch.isnan(stat).all() and (count == -1).all() and (flags == -1).all()
    assert scheck() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(stat).any()


# ---------------------------------------------------------------------------------------
# (iv) the null moments, fitted = 0
# ---------------------------------------------------------------------------------------
NULL = dict(I=64, J=64, K=32, R=3, sigma=0.4, rate=0.5, seed=2024)


def null_problem():
    """One-bit probit readings drawn from the model at the true (S, C), P = 4096."""
    if "null" in _PROB:
        return _PROB["null"]
    c = NULL
    P = c["I"] * c["J"]
    g = np.random.default_rng(c["seed"])
    S = (0.2 + 0.8 * g.random((c["R"], P))).astype(np.float32).astype(np.float64)
    C = (0.1 + 0.9 * g.random((c["R"], c["K"]))).astype(np.float32).astype(np.float64)
    T = C.T @ S
    b = [0.0, float(np.float32(np.median(T))), float(np.float32(T.max() + 1.0))]
    Y = draw_codes(g, T, b, c["sigma"], "probit", False)
    Wx = g.random(T.shape) < c["rate"]
    k, p = np.nonzero(Wx)
    d = dict(S=S, C=C, Y=Y, Wx=Wx, k=k, p=p, y=Y[k, p], b=b, P=P,
             model=(b, c["sigma"], 0.0, False, "probit"))
    d["ref"] = cr.stats(S, C, k, p, d["y"], *d["model"], fitted=False)
    _PROB["null"] = d
    return d


def moments(z):
    """(mean, variance about 0, kappa): kappa = sqrt((m4 - 1) / 2) scales the standard deviation
    sqrt(2 / P) of the sample variance of P unit normals to that of variables with fourth moment
    m4 (var(z^2) = m4 - 1 at unit variance)."""
    z = np.asarray(z, np.float64)
    return float(z.mean()), float((z * z).mean()), float(np.sqrt((np.mean(z ** 4) - 1.0) / 2.0))


def test_null_moments_of_z_fit_and_z_shift():
    """Under the model at the true (S, C) and fitted = 0, D has mean 0 and variance V and u mean 0
    and variance Ixx exactly, so each z has mean 0 and variance 1 at every pixel: the mean of P of
    them has standard deviation 1 / sqrt(P), their mean square sqrt(2 / P) kappa.  (The reference
    passes with this seed: z_fit mean -0.0176, mean square 1.0075, kappa 1.122; z_shift mean
    0.0329, mean square 1.0095, kappa 1.011; the bounds are 0.078 and 0.124 / 0.112.)"""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    c, d = NULL, null_problem()
    P, K, I, J = d["P"], c["K"], c["I"], c["J"]
    ref = d["ref"]
    assert ref["flags"].max() == 0 and ref["n"].min() > 0
    zf_r, zs_r, _ = cr.zscores(ref)
    obs = Observations(torch.from_numpy(d["Y"]).reshape(K, 1, I, J),
                       torch.from_numpy(d["Wx"].astype(np.float32)).reshape(K, 1, I, J),
                       torch.tensor(d["b"]), c["sigma"], R_hint=c["R"])
    r = qmc.check_fit(obs, torch.from_numpy(d["S"]).float().reshape(c["R"], 1, I, J),
                      torch.from_numpy(d["C"]).float(), fitted=False)
    assert r.untestable == 0 and r.invalid == 0 and r.saturated == 0
    assert np.array_equal(r.n.reshape(-1).cpu().numpy(), ref["n"])
    for label, z, z_ref in (("z_fit", r.z_fit, zf_r), ("z_shift", r.z_shift, zs_r)):
        mean, var, _ = moments(z.reshape(-1).cpu().numpy())
        mean_r, var_r, kappa = moments(z_ref)
        print(label, "mean", mean, "var", var, "reference", mean_r, var_r, "kappa", kappa)
        for m, v in ((mean_r, var_r), (mean, var)):
            assert abs(m) <= 5.0 / np.sqrt(P)
            assert abs(v - 1.0) <= 5.0 * np.sqrt(2.0 / P) * kappa
    assert abs(r.z_fit_total) <= 5.0


# ---------------------------------------------------------------------------------------
# (v) planted faults, fitted = 1
# ---------------------------------------------------------------------------------------
FAULT = dict(I=32, J=32, K=64, R=2, sigma=0.5, rate=0.75, delta=1.5, seed=77, n_bad=8)


def fault_problem():
    """One-bit probit readings around a threshold at 0 with S, C ~ U(-1, 1) (a shift is then far
    from the span of the spectra: I* ~ Ixx), about 48 per pixel; 8 pixels read with x + delta."""
    if "fault" in _PROB:
        return _PROB["fault"]
    c = FAULT
    P = c["I"] * c["J"]
    g = np.random.default_rng(c["seed"])
    S = (2.0 * g.random((c["R"], P)) - 1.0).astype(np.float32).astype(np.float64)
    C = (2.0 * g.random((c["R"], c["K"])) - 1.0).astype(np.float32).astype(np.float64)
    T = C.T @ S
    b = [-10.0, 0.0, 10.0]
    bad = np.sort(g.choice(P, c["n_bad"], replace=False))
    shift = np.zeros(P)
    shift[bad] = c["delta"]
    Y = draw_codes(g, T + shift[None, :], b, c["sigma"], "probit", False)
    Wx = g.random(T.shape) < c["rate"]
    k, p = np.nonzero(Wx)
    d = dict(S=S, C=C, Y=Y, Wx=Wx, k=k, p=p, y=Y[k, p], b=b, P=P, bad=bad,
             model=(b, c["sigma"], 0.0, False, "probit"))
    _PROB["fault"] = d
    return d


def fault_reference(d, S_fit):
    """The reference's statistics, Bonferroni mask and the margin of the nearest |z| to the
    critical value, at the fitted S."""
    st = cr.stats(S_fit, d["C"], d["k"], d["p"], d["y"], *d["model"], fitted=True, ridge=0.0)
    _, zs, sh = cr.zscores(st)
    mask, crit = cr.flagged(zs, st["flags"] & 3 == 0, 0.01)
    return st, zs, sh, mask, float(np.min(np.abs(np.abs(zs) / crit - 1.0)))


def test_planted_level_shifts_are_the_flagged_pixels():
    """(delta and the seed were picked on the CPU with S from tests/sfit_ref.py's Newton fit: the
    reference then flags exactly the 8 planted pixels -- their z between 6.1 and 7.3, the largest
    null |z| 3.23, against the critical value 4.42 -- and no |z| lies within 1 % of it (the nearest
    is 27 % away); both are asserted here at the S that fit_S returns.)"""
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    c, d = FAULT, fault_problem()
    K, I, J, R = c["K"], c["I"], c["J"], c["R"]
    obs = Observations(torch.from_numpy(d["Y"]).reshape(K, 1, I, J),
                       torch.from_numpy(d["Wx"].astype(np.float32)).reshape(K, 1, I, J),
                       torch.tensor(d["b"]), c["sigma"], R_hint=R)
    assert 44 < len(d["k"]) / d["P"] < 52
    Ct = torch.from_numpy(d["C"]).float()
    fit = qmc.fit_S(obs, Ct, ridge=0.0)
    S_fit = fit.S.reshape(R, -1).double().cpu().numpy()
    st, zs, sh, mask, margin = fault_reference(d, S_fit)
    print("reference: flagged", np.nonzero(mask)[0].tolist(), "planted", d["bad"].tolist(),
          "margin", margin, "z at planted", zs[d["bad"]].tolist())
    assert np.array_equal(np.nonzero(mask)[0], d["bad"]) and margin > 0.01
    r = qmc.check_fit(obs, fit.S, Ct, fitted=True, ridge=0.0)
    got = r.flagged(0.01, "shift").reshape(-1).cpu().numpy()
    assert np.array_equal(got, mask)
    assert (r.shift.reshape(-1).cpu().numpy()[d["bad"]] > 0).all() and (sh[d["bad"]] > 0).all()
    assert r.untestable == 0 and np.array_equal(r.flags.reshape(-1).cpu().numpy(), st["flags"])


# ---------------------------------------------------------------------------------------
# (vi) solve(check=True)
# ---------------------------------------------------------------------------------------
def test_solve_attaches_the_result_of_the_direct_call():
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    K = I = J = 16
    R = 2
    g = torch.Generator().manual_seed(5)
    S0 = 0.2 + 0.8 * torch.rand(R, 1, I, J, generator=g)
    C0 = 0.1 + 0.9 * torch.rand(R, K, generator=g)
    T = torch.einsum("rp,rk->kp", S0.reshape(R, -1), C0)
    b = torch.tensor([0.0, float(T.median()), float(T.max()) + 1.0])
    Y = (T + 0.3 * torch.randn(T.shape, generator=g) > b[1]).long().reshape(K, 1, I, J)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), 0.7), generator=g)
    obs = Observations(Y, Wx, b, 0.3, R_hint=R)
    res = qmc.solve(None, None, b, 0.3, R=R, S_init=S0, C_init=C0, max_iter=5, obs=obs,
                    check=True)
    assert isinstance(res.check, qmc.CheckResult)
    ridge = qmc.default_confidence_ridge(res.S, 100.0)
    direct = qmc.check_fit(obs, res.S, res.C, fitted=True, ridge=ridge)
    for key in ("D", "V", "u", "info", "n", "flags", "z_fit", "z_shift", "shift"):
        assert torch.equal(getattr(res.check, key), getattr(direct, key)), key
    assert tuple(res.check.z_shift.shape) == (I, J)
    assert qmc.solve(None, None, b, 0.3, R=R, S_init=S0, C_init=C0, max_iter=2, obs=obs).check is None
