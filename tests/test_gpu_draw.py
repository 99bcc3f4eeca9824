"""GPU: the draw of readings from the model (qsc_draw_codes, qsc_draw_readings,
Observations.resample) and fits.bootstrap against the fp64 reference of tests/draw_ref.py.

Inputs: the seven cases of tests/test_gpu_check.py (R 2 / 5 / 11, probit and logit, linear and
log, two bins with signed rows, 4 bins, K = 4100 wide entries, a readings list with cells read
three times; P = 130 with tile 64, so padding positions exist), with its planted pixels: one whose
every bin but the last has P == 0 and one (log model) with t + offset <= 0.  The 16-bin case is the
bins4 map cut at 15 quantiles (wide entries).  Codes are compared exactly outside the window
draw_ref.WINDOW (u Z within 1e-5 of a cumulative sum: ten times the 1e-6 to which fp32
probabilities agree with fp64), which may hold at most 1e-3 of the readings
(tests/test_draw_host.py checks the inputs).  The bootstrap input is draw_ref.boot_problem()."""
import numpy as np
import pytest
import torch

import check_ref as cr
import draw_ref as dr
import readings_ref as rr
import test_gpu_check as tgc

pytestmark = pytest.mark.gpu

SEED = 11
t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def packed_dict(obs):
    """The packing of `obs` as tests/readings_ref.py's decode_lists takes it."""
    d = obs.desc
    desc = dict(K=d.K, P=d.P, Pp=d.Pp, PT=d.PT, ntiles=d.ntiles, nks=d.nks, wide=d.wide,
                nbins=d.nbins, rowfmt=d.rowfmt)
    n = lambda x: x.cpu().numpy()
    view = (lambda e: n(e.view(torch.int32)).view(np.uint32)) if d.wide else \
        (lambda e: n(e).view(np.uint16))
    return dict(desc=desc, s_entries=view(obs.s_entries), c_entries=view(obs.c_entries),
                s_width=n(obs.s_width), s_off=n(obs.s_off), c_width=n(obs.c_width),
                c_off=n(obs.c_off), c_kmap=n(obs.c_kmap), perm=n(obs.perm))


def cell_codes(obs):
    """{(k, p): sorted codes} of both formats of a packed Observations."""
    a = packed_dict(obs)
    per_pixel, per_bin = rr.decode_lists(a)
    s_side, c_side = {}, {}
    for p, lst in per_pixel.items():
        for k, c in lst:
            s_side.setdefault((k, p), []).append(c)
    nt, perm = a["desc"]["ntiles"], a["perm"]
    for (t, k), lst in per_bin.items():
        for ql, c in lst:
            i = ql // 32
            g = i * nt + ((nt - 1 - t) if i & 1 else t)
            c_side.setdefault((k, int(perm[g * 32 + ql % 32])), []).append(c)
    srt = lambda m: {key: sorted(v) for key, v in m.items()}
    return srt(s_side), srt(c_side)


def reference_cells(d, r, keep_all=False):
    """{(k, p): sorted reference codes} and the set of cells with a reading inside the window."""
    cells, near = {}, set()
    for k, p, c, m in zip(d["k"].tolist(), d["p"].tolist(), r["code"].tolist(), r["margin"]):
        cells.setdefault((k, p), []).append(c)
        if m <= dr.WINDOW:
            near.add((k, p))
    return {key: sorted(v) for key, v in cells.items()}, near


def sc(d):
    return tgc.tensors(d)


# ---------------------------------------------------------------------------------------
# parity of the codes, the pattern, the argument left untouched
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tgc.CASES))
def test_drawn_codes_equal_the_reference_outside_the_window(name):
    d = tgc.problem(name)
    obs = tgc.observations(name)
    S, C = sc(d)
    r = dr.resample_readings(d["S"], d["C"], d["k"], d["p"], d["y"], d["model"], SEED, 0)
    ref, near = reference_cells(d, r)
    assert len(near) <= 1e-3 * len(d["k"])
    kept = [t.clone() for t in (obs.s_entries, obs.c_entries, obs.perm, obs.counts, obs.s_width,
                                obs.s_off, obs.c_width, obs.c_off, obs.c_kmap)]
    kept_codes = (obs.codes if obs.codes is not None else obs._packed).clone()
    new = obs.resample(S, C, seed=SEED, replicate=0)
    # the pattern is shared, the codes are new arrays, the argument is bit-unchanged
    for key in ("perm", "counts", "s_width", "s_off", "c_width", "c_off", "c_kmap", "model"):
        assert getattr(new, key) is getattr(obs, key)
    assert new.nnz == obs.nnz and new.desc is not obs.desc and new.desc.rowfmt == obs.desc.rowfmt
    assert new.s_entries.data_ptr() != obs.s_entries.data_ptr()
    assert new._engines == 0 and new._code_field is None
    now = (obs.s_entries, obs.c_entries, obs.perm, obs.counts, obs.s_width, obs.s_off,
           obs.c_width, obs.c_off, obs.c_kmap)
    assert all(torch.equal(a, b) for a, b in zip(kept, now))
    assert torch.equal(kept_codes, obs.codes if obs.codes is not None else obs._packed)
    if obs.codes is not None:
        codes = new.codes.cpu().numpy()
        assert np.array_equal(codes == 0xFF, ~d["Wx"])
        got = codes[d["k"], d["p"]].astype(np.int64)
        cmp = r["margin"] > dr.WINDOW
        print(name, "compared", int(cmp.sum()), "of", cmp.size, "differing",
              int((got[cmp] != r["code"][cmp]).sum()))
        assert np.array_equal(got[cmp], r["code"][cmp])
    # both entry formats hold, per cell, the reference's codes
    s_side, c_side = cell_codes(new)
    assert set(s_side) == set(ref) and set(c_side) == set(ref)
    for cell, want in ref.items():
        if cell not in near:
            assert s_side[cell] == want and c_side[cell] == want, cell
    # invalid: the readings with t + offset <= 0 keep their codes and are counted
    assert int(new.invalid.item()) == int(r["invalid"].sum())
    if "negative" in d["planted"]:
        assert r["invalid"].any()
    if "underflow" in d["planted"]:
        assert all(set(v) == {len(d["b"]) - 2} for (k, p), v in s_side.items()
                   if p == d["planted"]["underflow"])
    # drawn data never saturate the likelihood (flag bit 4), wherever the input did
    from quantized_spectrum_cartography_amd import qmc
    chk = qmc.check_fit(new, S, C, fitted=False)
    assert int((chk.flags & 4).sum()) == 0


def test_sixteen_bins_wide_entries():
    d = dict(tgc.problem("bins4_11"))
    T = d["C"].T @ d["S"]
    q = np.quantile(T[:, 4:], np.arange(1, 16) / 16.0)
    b = [float(np.float32(v)) for v in [0.0] + q.tolist() + [float(T.max()) + 1.0]]
    model = (b, d["sigma"], 0.0, False, "probit")
    from quantized_spectrum_cartography_amd.obs import Observations
    K, I, J = d["K"], d["I"], d["J"]
    Y = np.minimum(d["Y"], 3)
    obs = Observations(t_(Y).reshape(K, 1, I, J), t_(d["Wx"].astype(np.float32)).reshape(K, 1, I, J),
                       torch.tensor(b), d["sigma"], tile=tgc.TILE, R_hint=d["R"])
    assert obs.desc.wide == 1 and obs.desc.nbins == 16
    S, C = sc(d)
    new = obs.resample(S, C, seed=SEED, replicate=1)
    r = dr.resample_readings(d["S"], d["C"], d["k"], d["p"], Y[d["k"], d["p"]], model, SEED, 1)
    cmp = r["margin"] > dr.WINDOW
    assert (~cmp).sum() <= 1e-3 * cmp.size
    got = new.codes.cpu().numpy()[d["k"], d["p"]].astype(np.int64)
    assert np.array_equal(got[cmp], r["code"][cmp]) and len(np.unique(got)) >= 8


# ---------------------------------------------------------------------------------------
# one definition, two inputs; repeats; keys
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["onebit2", "bins4_11"])
def test_readings_input_gives_the_dense_input_s_entries(name):
    from quantized_spectrum_cartography_amd.obs import Observations
    d = tgc.problem(name)
    dense = tgc.observations(name)
    K, I, J = d["K"], d["I"], d["J"]
    o = np.random.default_rng(3).permutation(len(d["k"]))
    lst = Observations.from_readings(t_(d["k"][o]), t_(d["p"][o] // J), t_(d["p"][o] % J),
                                     t_(d["y"][o]), (K, I, J), torch.tensor(d["b"]), d["sigma"],
                                     tile=tgc.TILE, R_hint=d["R"], loss=d["loss"])
    assert lst.desc.rowfmt == dense.desc.rowfmt == (1 if name == "onebit2" else 0)
    S, C = sc(d)
    a, b = dense.resample(S, C, seed=SEED), lst.resample(S, C, seed=SEED)
    assert torch.equal(a.s_entries, b.s_entries) and torch.equal(a.c_entries, b.c_entries)
    assert not torch.equal(a.s_entries, dense.s_entries)


def test_repeated_cells_get_one_draw_per_occurrence_in_both_formats():
    name = "readings11"
    d = tgc.problem(name)
    obs = tgc.observations(name)
    assert obs.max_repeat == 3
    S, C = sc(d)
    new = obs.resample(S, C, seed=SEED, replicate=2)
    r = dr.resample_readings(d["S"], d["C"], d["k"], d["p"], d["y"], d["model"], SEED, 2)
    assert set(r["j"].tolist()) == {0, 1, 2}
    ref, near = reference_cells(d, r)
    s_side, c_side = cell_codes(new)
    triples = [c for c in ref if len(ref[c]) == 3 and c not in near]
    assert len(triples) > 100
    assert all(s_side[c] == c_side[c] == ref[c] for c in triples)
    assert any(len(set(ref[c])) > 1 for c in triples)      # the occurrences are drawn separately


def test_keys_seed_replicate_tile_perm_and_schedule():
    from quantized_spectrum_cartography_amd.obs import Observations
    name = "bins4_11"
    d = tgc.problem(name)
    obs = tgc.observations(name)
    S, C = sc(d)
    K, I, J = d["K"], d["I"], d["J"]
    a = obs.resample(S, C, seed=SEED, replicate=3)
    b = obs.resample(S, C, seed=SEED, replicate=3)
    assert torch.equal(a.codes, b.codes) and torch.equal(a.s_entries, b.s_entries)
    assert torch.equal(a.c_entries, b.c_entries)
    assert not torch.equal(a.codes, obs.resample(S, C, seed=SEED + 1, replicate=3).codes)
    assert not torch.equal(a.codes, obs.resample(S, C, seed=SEED, replicate=4).codes)
    base, _ = cell_codes(a)
    perm = torch.full((256,), -1, dtype=torch.int32)
    perm[:130] = torch.from_numpy(np.random.default_rng(9).permutation(130).astype(np.int32))
    args = (t_(d["Y"]).reshape(K, 1, I, J), t_(d["Wx"].astype(np.float32)).reshape(K, 1, I, J),
            torch.tensor(d["b"]), d["sigma"])
    for kw in (dict(tile=128), dict(tile=128, perm=perm), dict(tile=64, schedule=False)):
        other = Observations(*args, R_hint=d["R"], **kw).resample(S, C, seed=SEED, replicate=3)
        assert torch.equal(other.codes, a.codes)
        s_side, c_side = cell_codes(other)
        assert s_side == base and c_side == base


# ---------------------------------------------------------------------------------------
# the distribution of the draws
# ---------------------------------------------------------------------------------------
def test_drawn_data_follow_the_model():
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    c, d = tgc.NULL, tgc.null_problem()
    P, K, I, J, R = d["P"], c["K"], c["I"], c["J"], c["R"]
    obs = Observations(t_(d["Y"]).reshape(K, 1, I, J),
                       t_(d["Wx"].astype(np.float32)).reshape(K, 1, I, J),
                       torch.tensor(d["b"]), c["sigma"], R_hint=R)
    S, C = t_(d["S"]).float().reshape(R, 1, I, J), t_(d["C"]).float()
    new = obs.resample(S, C, seed=SEED)
    _, r = dr.resample_dense(d["S"], d["C"], d["Y"], d["Wx"], d["model"], SEED, 0)
    got = new.codes.cpu().numpy()[r["k"], r["p"]]
    for b in range(2):
        pb = r["Pb"][b]
        dev = abs((got == b).sum() - pb.sum()) / np.sqrt((pb * (1 - pb)).sum())
        print("bin", b, "count", int((got == b).sum()), "expected", pb.sum(), "deviation", dev)
        assert dev <= 5.0
    st = cr.stats(d["S"], d["C"], r["k"], r["p"], r["code"], *d["model"], fitted=False)
    chk = qmc.check_fit(new, S, C, fitted=False)
    assert chk.saturated == 0 and chk.invalid == 0
    for label, z, z_ref in (("z_fit", chk.z_fit, cr.zscores(st)[0]),
                            ("z_shift", chk.z_shift, cr.zscores(st)[1])):
        mean, var, _ = tgc.moments(z.reshape(-1).cpu().numpy())
        kappa = tgc.moments(z_ref)[2]
        print(label, "mean", mean, "mean square", var, "kappa", kappa)
        assert abs(mean) <= 5.0 / np.sqrt(P)
        assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / P) * kappa


# ---------------------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------------------
def test_a_graph_replay_of_the_draw_equals_the_eager_call():
    from quantized_spectrum_cartography_amd import _lib
    d = tgc.problem("bins4_11")
    obs = tgc.observations("bins4_11")
    R = d["R"]
    S, C = sc(d)
    Sd, Cd = S.reshape(R, -1).cuda().contiguous(), C.cuda().contiguous()
    eager = obs.resample(S, C, seed=SEED, replicate=5).codes
    out = torch.zeros_like(obs.codes)
    inv = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _lib.call("qsc_draw_codes", _lib.ptr(obs.codes), obs.K, obs.P, obs.model, R,
                      _lib.ptr(Sd), _lib.ptr(Cd), SEED, 5, _lib.ptr(out), _lib.ptr(inv),
                      _lib.stream())
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_abi_rejects_what_it_cannot_draw_from():
    from quantized_spectrum_cartography_amd import _lib
    d = tgc.problem("bins4_11")
    obs = tgc.observations("bins4_11")
    R = d["R"]
    S, C = sc(d)
    Sd, Cd = S.reshape(R, -1).cuda().contiguous(), C.cuda().contiguous()
    out = torch.full_like(obs.codes, 9)
    inv = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    sq = _lib.make_model(d["b"], d["sigma"], loss="squared")
    p = _lib.ptr
    call = lambda m, r, o: L.qsc_draw_codes(p(obs.codes), obs.K, obs.P, m, r, p(Sd), p(Cd), SEED, 0,
                                            o, p(inv), _lib.stream())
    assert call(sq, R, p(out)) == _lib.QSC_EINVAL
    assert call(obs.model, 0, p(out)) == _lib.QSC_EINVAL
    assert call(obs.model, 17, p(out)) == _lib.QSC_EINVAL
    assert call(obs.model, R, p(None)) == _lib.QSC_EINVAL
    torch.cuda.synchronize()
    assert (out == 9).all()


# ---------------------------------------------------------------------------------------
# bootstrap
# ---------------------------------------------------------------------------------------
def boot_obs(Y):
    from quantized_spectrum_cartography_amd.obs import Observations
    c, d = dr.BOOT, dr.boot_problem()
    K, I, J = c["K"], c["I"], c["J"]
    return Observations(t_(Y).reshape(K, 1, I, J),
                        t_(d["Wx"].astype(np.float32)).reshape(K, 1, I, J), torch.tensor(d["b"]),
                        c["sigma"], R_hint=c["R"])


def boot_tensors():
    c, d = dr.BOOT, dr.boot_problem()
    return t_(d["S"]).float().reshape(c["R"], 1, c["I"], c["J"]), t_(d["C"]).float()


def test_bootstrap_replicates_and_spread_vs_reference():
    """Each replicate's refitted S, C and NLL, and std_S / std_C over the replicates, against the
    fp64 reference on the codes the GPU drew: max|got - ref| / max|ref| <= max(1e-5, 10 floor),
    floor the same metric of the reference's own fp32 run, over the pixels (bins) whose fit
    converged in both the fp32 and the fp64 reference in every replicate (at most 10 % left out).
    A converged fit ends at the minimiser whatever sequence of accepted and rejected steps led
    there, so the step counts themselves need not agree (they do at 18 of 1024 pixels only); a
    fit that ran into max_steps in one precision stopped at a point the accept decisions chose."""
    from quantized_spectrum_cartography_amd import fits, qmc
    c, d = dr.BOOT, dr.boot_problem()
    n, R, P = 6, c["R"], d["P"]
    obs = boot_obs(d["Y"])
    S, C = boot_tensors()
    codes = []
    for b in range(n):
        y = obs.resample(S, C, seed=c["draw_seed"], replicate=b).codes.cpu().numpy().astype(np.int64)
        codes.append(np.where(d["Wx"], y, 0))
    ref = dr.bootstrap(d["S"], d["C"], d["Y"], d["Wx"], d["model"], n=n, codes=codes)
    flo = dr.bootstrap(d["S"], d["C"], d["Y"], d["Wx"], d["model"], n=n, codes=codes,
                       dtype=np.float32)
    same_s = np.all([a[("S", 0)] & b[("S", 0)] for a, b in zip(ref["steps"], flo["steps"])], axis=0)
    same_c = np.all([a[("C", 0)] & b[("C", 0)] for a, b in zip(ref["steps"], flo["steps"])], axis=0)
    print("pixels kept", int(same_s.sum()), "of", P, "bins kept", int(same_c.sum()), "of", c["K"])
    assert same_s.sum() >= 0.9 * P and same_c.sum() >= 0.9 * c["K"]
    err = lambda got, want, keep: float(np.max(np.abs(got - want)[..., keep]) /
                                        np.max(np.abs(want[..., keep])))
    res = qmc.bootstrap(obs, S, C, n=n, seed=c["draw_seed"])
    assert res.n == n and res.invalid == 0 and res.std_map is None
    pairs = [("std_S", res.std_S.reshape(R, P).double().cpu().numpy(), ref["std_S"], flo["std_S"], same_s),
             ("std_C", res.std_C.double().cpu().numpy(), ref["std_C"], flo["std_C"], same_c),
             ("mean_S", res.mean_S.reshape(R, P).double().cpu().numpy(), ref["mean_S"], flo["mean_S"], same_s),
             ("mean_C", res.mean_C.double().cpu().numpy(), ref["mean_C"], flo["mean_C"], same_c)]
    for label, got, want, floor_v, keep in pairs:
        e, f = err(got, want, keep), err(floor_v, want, keep)
        print(label, "err", e, "floor", f)
        assert e <= max(1e-5, 10 * f)
    e = float(np.max(np.abs(res.nll.numpy() - ref["nll"]) / np.abs(ref["nll"])))
    f = float(np.max(np.abs(flo["nll"] - ref["nll"]) / np.abs(ref["nll"])))
    print("nll err", e, "floor", f, "observed", res.nll_observed, ref["nll_observed"])
    assert e <= max(1e-5, 10 * f)
    assert abs(res.nll_observed - ref["nll_observed"]) <= max(1e-5, 10 * f) * abs(ref["nll_observed"])
    assert res.p_fit == (1 + int((res.nll.numpy() >= res.nll_observed).sum())) / (n + 1)


def test_bootstrap_spread_matches_confidence_and_p_fit_tells_a_wrong_noise_scale():
    from quantized_spectrum_cartography_amd import qmc
    c, d = dr.BOOT, dr.boot_problem()
    n, R, P = c["n"], c["R"], d["P"]
    S, C = boot_tensors()
    obs = boot_obs(d["Y"])
    res = qmc.bootstrap(obs, S, C, n=n, seed=c["draw_seed"], refit=("S",), map_std=True)
    conf = qmc.confidence(obs, S, C, kind="expected")
    many = (d["Wx"].sum(axis=0) >= 40)
    ratio = (res.std_S / conf.std_S).reshape(R, P).cpu().numpy()[:, many]
    print("pixels with >= 40 readings", int(many.sum()), "median std_S / confidence",
          float(np.median(ratio)))
    assert many.sum() > 100 and 0.7 <= np.median(ratio) <= 1.5
    assert res.std_map.shape == (c["K"], 1, c["I"], c["J"]) and bool((res.std_map > 0).all())
    assert torch.equal(res.mean_C, C.cuda()) and bool((res.std_C == 0).all())
    print("p_fit at the model's noise", res.p_fit)
    assert 0.05 <= res.p_fit <= 0.95
    noisy = qmc.bootstrap(boot_obs(d["Y2"]), S, C, n=n, seed=c["draw_seed"], refit=("S",))
    print("p_fit at twice the noise", noisy.p_fit, noisy.nll_observed, float(noisy.nll.max()))
    assert noisy.p_fit == 1.0 / (n + 1)
