"""GPU: growing packed observations (qsc_obs_cell_counts, qsc_draw_list, qsc_obs_readings_merge;
Observations.occurrences / draw / append; qmc.draw_readings, qmc.acquire) against the integer
reference of tests/append_ref.py and the fp64 references tests/info_ref.py, tests/design_ref.py.

Shapes are the packing tests' own (select_ref.SHAPES: (5, 9, 7), (70, 23, 21), (8, 32, 32)), tiles 64
and 128, 2 and 4 bins, list parents with up to 5 readings per cell.  The parent of the middle shape
holds about 35 k readings: no multiple of the merge chunk of 1024, with runs of equal keys that
cross chunk boundaries in both sorted arrays (asserted below).  An append is compared bit for bit
with the re-sort it replaces, from_readings(cat(obs.readings(), batch), perm=obs.perm): counts,
descriptor, tables, the five arrays of `_packed` (the alignment gaps between them are never
written by either route), both entry arrays and max_repeat."""
import numpy as np
import pytest
import torch

import append_ref as ap
import design_ref as de
import draw_ref as dr
import select_ref as sl
import test_gpu_check as tgc
import test_gpu_info as gi

pytestmark = pytest.mark.gpu

SEED = 11
TABLES = ("perm", "counts", "s_width", "s_off", "c_width", "c_off", "c_kmap", "s_entries",
          "c_entries")
t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
n_ = lambda t: t.cpu().numpy().astype(np.int64)  # noqa: E731


SITES = ap.SITES
_ACQ = {}


def acquire_problem():
    """(d, list parent, S (2,1,I,J), C (2,K)) of append_ref.acquire_inputs(), built once."""
    d, S, C = ap.acquire_inputs()
    if not _ACQ:
        _ACQ["obs"] = from_list(d, d["k"], d["p"], d["c"], None, R_hint=2)
        _ACQ["S"], _ACQ["C"] = t_(S).reshape(2, 1, d["I"], d["J"]), t_(C)
    return d, _ACQ["obs"], _ACQ["S"], _ACQ["C"]


def from_list(d, k, p, c, tile, perm=None, schedule=None, R_hint=8):
    from quantized_spectrum_cartography_amd.obs import Observations
    J = d["J"]
    return Observations.from_readings(t_(k), t_(p // J), t_(p % J), t_(c), (d["K"], d["I"], J),
                                      d["b"], d["sigma"], tile=tile, perm=perm, R_hint=R_hint,
                                      schedule=schedule)


def kijc(d, b):
    k, p, c = b
    return t_(k), t_(p // d["J"]), t_(p % d["J"]), t_(c)


def resort(obs, d, batch, perm="keep"):
    """The route an append replaces: export, concatenate, pack again."""
    from quantized_spectrum_cartography_amd.obs import Observations
    parts = [torch.cat((a, b.to(a.device).to(a.dtype))) for a, b in zip(obs.readings(), kijc(d, batch))]
    return Observations.from_readings(*parts, (d["K"], d["I"], d["J"]), d["b"], d["sigma"],
                                      perm=obs.perm if perm == "keep" else None, tile=obs.desc.PT,
                                      R_hint=obs.R_hint, schedule=obs.schedule)


def desc_of(obs):
    return {name: getattr(obs.desc, name) for name, _ in obs.desc._fields_}


def packed_of(obs):
    return ap.packed_views(obs._packed.cpu().numpy(), obs.nnz, obs.K, obs.P, obs.desc.PT)


def assert_same(a, b):
    assert desc_of(a) == desc_of(b)
    for f in TABLES:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.codes is None and b.codes is None and a._n == b._n == a.nnz
    assert a._packed.numel() == b._packed.numel()
    pa, pb = packed_of(a), packed_of(b)
    for f in pa:
        assert pa[f].tobytes() == pb[f].tobytes(), f
    assert a.max_repeat == b.max_repeat
    assert (a.loss, a.R_hint, a.schedule, a.noise_std) == (b.loss, b.R_hint, b.schedule, b.noise_std)


def assert_is_reference(obs, k, p, c):
    """`_packed`, the counts and max_repeat against the numpy reference on the full list."""
    want = ap.sorted_arrays(k, p, c, obs.K, obs.P, obs.desc.PT, obs.perm.cpu().numpy())
    got = packed_of(obs)
    for f in want:
        assert np.array_equal(got[f], want[f]), f
    assert np.array_equal(n_(obs.counts), np.bincount(p, minlength=obs.P))
    assert obs.max_repeat == np.bincount(k * obs.P + p).max() and obs.nnz == k.size


def snapshot(obs):
    arrays = [getattr(obs, f) for f in TABLES] + [obs.codes if obs.codes is not None else obs._packed]
    return arrays, [a.clone() for a in arrays], desc_of(obs)


def assert_untouched(obs, snap):
    arrays, copies, desc = snap
    now = [getattr(obs, f) for f in TABLES] + [obs.codes if obs.codes is not None else obs._packed]
    assert all(a is b for a, b in zip(arrays, now))
    assert all(torch.equal(a, b) for a, b in zip(now, copies))
    assert desc_of(obs) == desc


def parent_lists(d, without=None):
    k, p, c = d["k"], d["p"], d["c"]
    if without is not None:
        m = ~np.isin(p, without)
        k, p, c = k[m], p[m], c[m]
    return k, p, c


CASES = [(name, tile, nbins) for name in sl.SHAPES for tile in (64, 128) for nbins in (2, 4)]


# ---------------------------------------------------------------------------------------
# append is the re-sort, bit for bit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tile,nbins", CASES)
def test_append_equals_the_resort_bit_for_bit(name, tile, nbins):
    d = sl.problem(name, nbins, 5)
    obs = from_list(d, d["k"], d["p"], d["c"], tile)
    snap = snapshot(obs)
    n = obs.nnz
    assert obs.desc.rowfmt == int(nbins == 2) and obs.max_repeat == 5
    if name == "ragged":
        assert n > 30000 and n % ap.CHUNK != 0
        pk = packed_of(obs)
        sk, ck, _ = ap.sort_keys(d["k"], d["p"], d["K"], d["P"], tile, obs.perm.cpu().numpy())
        for key in (np.sort(sk), np.sort(ck)):  # runs of equal keys cross merge chunk boundaries
            assert any(key[e - 1] == key[e] for e in range(ap.CHUNK, n, ap.CHUNK))
        assert pk["s_rd"].size == n
    order = ap.exported(d["k"], d["p"], obs.perm.cpu().numpy())
    B = ap.batches(name, nbins)
    got = {}
    for b in ("single", "m1000", "larger", "one_pixel", "repeats", "shuffled"):
        k, p, c = B[b]
        new = obs.append(*kijc(d, B[b]))
        assert new.perm is obs.perm and new.nnz == n + k.size and new.desc.PT == tile
        assert_same(new, resort(obs, d, B[b]))
        assert_is_reference(new, *(np.r_[x[order], y] for x, y in zip((d["k"], d["p"], d["c"]), B[b])))
        assert_untouched(obs, snap)
        got[b] = new
    assert got["larger"].nnz > 2 * n and got["repeats"].max_repeat >= 5 + 3
    assert int(got["one_pixel"].counts.max()) >= 300
    # the order of the batch changes nothing but the stable order of equal keys
    a, b = got["m1000"], got["shuffled"]
    for f in TABLES[:7]:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    pa, pb = packed_of(a), packed_of(b)
    for f in ("s_seg", "c_seg", "c_kinv"):
        assert np.array_equal(pa[f], pb[f])
    for f in ("s_rd", "c_rd"):
        assert np.array_equal(pa[f] & 0xFFFFFF, pb[f] & 0xFFFFFF)
    # readings only into pixels the parent never saw
    unseen = ap.unseen_pixels(name)
    k0, p0, c0 = parent_lists(d, unseen)
    par = from_list(d, k0, p0, c0, tile)
    assert int(par.counts[t_(unseen)].sum()) == 0
    new = par.append(*kijc(d, B["unseen"]))
    assert_same(new, resort(par, d, B["unseen"]))
    o = ap.exported(k0, p0, par.perm.cpu().numpy())
    assert_is_reference(new, *(np.r_[x[o], y] for x, y in zip((k0, p0, c0), B["unseen"])))


@pytest.mark.parametrize("name,tile,nbins", [c for c in CASES if c[1] == 64])
def test_two_appends_equal_one_and_a_dense_or_fresh_append_is_the_resort(name, tile, nbins):
    from quantized_spectrum_cartography_amd.obs import Observations
    d = sl.problem(name, nbins, 5)
    obs = from_list(d, d["k"], d["p"], d["c"], tile)
    B = ap.batches(name, nbins)
    both = tuple(np.r_[x, y] for x, y in zip(B["m1000"], B["repeats"]))
    two = obs.append(*kijc(d, B["m1000"])).append(*kijc(d, B["repeats"]))
    assert_same(two, obs.append(*kijc(d, both)))
    # perm="fresh": the pixels ordered by the new counts -- from_readings without a perm
    fresh = obs.append(*kijc(d, B["one_pixel"]), perm="fresh")
    assert_same(fresh, resort(obs, d, B["one_pixel"], perm="fresh"))
    assert int(fresh.perm[0]) == int(d["p"][0])
    # a dense parent: exported, concatenated and packed as a list (its pixel order kept)
    d1 = sl.problem(name, nbins, 1)
    Y, Wx = sl.dense_of(d1)
    shape = (d1["K"], 1, d1["I"], d1["J"])
    dense = Observations(t_(Y).reshape(shape), t_(Wx.astype(np.float32)).reshape(shape), d1["b"],
                         d1["sigma"], tile=tile)
    snap = snapshot(dense)
    new = dense.append(*kijc(d1, B["repeats"]))
    assert new.codes is None and new.perm is not None and torch.equal(new.perm, dense.perm)
    assert_same(new, resort(dense, d1, B["repeats"]))
    assert_untouched(dense, snap)
    assert_same(new.append(*kijc(d1, B["single"])), resort(new, d1, B["single"]))  # then it merges


def test_an_invalid_batch_raises_with_its_count_and_builds_nothing():
    d = sl.problem("ragged", 4, 5)
    obs = from_list(d, d["k"], d["p"], d["c"], 64)
    snap = snapshot(obs)
    k, i, j, c = kijc(d, tuple(a[:10].copy() for a in ap.batches("ragged", 4)["m1000"]))
    k[3], i[5], c[7] = d["K"], -1, 4
    for perm in ("keep", "fresh"):
        with pytest.raises(ValueError, match=r"^3 of 10 readings"):
            obs.append(k, i, j, c, perm=perm)
    with pytest.raises(ValueError, match="one length"):
        obs.append(k[:9], i, j, c)
    with pytest.raises(ValueError, match="perm must be"):
        obs.append(k, i, j, c, perm="sorted")
    assert_untouched(obs, snap)
    from quantized_spectrum_cartography_amd import _lib
    L = _lib.lib()
    K, P = d["K"], d["P"]
    assert L.qsc_obs_readings_merge_packed_bytes(2 ** 30, 2 ** 30, K, P, 64) == 0
    assert L.qsc_obs_readings_merge_workspace_bytes(2 ** 30, 2 ** 30, K, P, 64) == 0
    assert L.qsc_obs_readings_merge_packed_bytes(obs.nnz, 0, K, P, 64) == 0
    assert L.qsc_obs_readings_merge_packed_bytes(obs.nnz, 5, K, P, 65) == 0
    # the workspace follows m, not n
    small = L.qsc_obs_readings_merge_workspace_bytes(obs.nnz, 100, K, P, 64)
    assert 0 < small == L.qsc_obs_readings_merge_workspace_bytes(100 * obs.nnz, 100, K, P, 64)


def test_a_graph_captured_on_the_parent_replays_unchanged_after_append():
    from quantized_spectrum_cartography_amd.obs import Observations
    from quantized_spectrum_cartography_amd.qmc import FreeSSolver
    from test_gpu_fused import _random_case
    d = _random_case(83, 4, 32, 32, 8, f=0.3)
    k, _, i, j = torch.nonzero(d["Wx"], as_tuple=True)
    mk = lambda: Observations.from_readings(k, i, j, d["Y"][k, 0, i, j], (8, 32, 32), d["b"],  # noqa: E731
                                            d["sigma"], R_hint=4, tile=256)
    obs = mk()
    sol = FreeSSolver(obs, d["S0"], d["C0"], hist_cap=64)
    sol.run(3, use_graph=True)
    snap = snapshot(obs)
    obs.append(k[:500], i[:500], j[:500], d["Y"][k, 0, i, j][:500])
    obs.occurrences(k[:50], i[:50], j[:50])
    assert_untouched(obs, snap)
    sol.run(3, use_graph=True)
    ref = FreeSSolver(mk(), d["S0"], d["C0"], hist_cap=64)
    ref.run(6, use_graph=False)
    assert torch.equal(ref.S, sol.S) and torch.equal(ref.C, sol.C)


# ---------------------------------------------------------------------------------------
# draws are the resample's draws; occurrences
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tgc.CASES))
def test_draws_at_listed_cells_are_the_resamples_draws(name):
    """Dense and list parents; probit, log-model and logit (test_gpu_check's cases, with their
    planted pixels).  Bit for bit against resample; against the fp64 reference outside the window
    draw_ref.WINDOW, which may hold at most 1e-3 of the readings."""
    from quantized_spectrum_cartography_amd import qmc
    d = tgc.problem(name)
    obs = tgc.observations(name)
    S, C = tgc.tensors(d)
    K, I, J, P = obs.K, obs.I, obs.J, obs.P
    b, sigma, offset, log_model, loss = d["model"]
    k, i, j, c_old = obs.readings()
    kk, pp = n_(k), n_(i) * J + n_(j)
    occ = dr.occurrence(kk, pp, P)  # (the exported order is (.., occurrence): list order counts it)
    assert occ.max() == (2 if d["packing"] == "readings" else 0)
    for rep in (3, 0):  # (replicate 0 last: the reference comparison below is at tgc's own draw)
        new = obs.resample(S, C, seed=SEED, replicate=rep)
        kn, in_, jn, c_new = new.readings()
        assert torch.equal(k, kn) and torch.equal(i, in_) and torch.equal(j, jn)
        args = (k, i, j, S, C, (K, I, J), b, sigma, offset, log_model, loss, SEED, rep)
        code = qmc.draw_readings(*args, occurrence=t_(occ), allow_invalid=True)
        assert code.dtype == torch.uint8 and code.is_cuda and code.numel() == obs.nnz
        undrawn = code == 0xFF
        assert torch.equal(code[~undrawn], c_new[~undrawn])
        assert torch.equal(c_new[undrawn], c_old[undrawn])   # resample keeps what it cannot draw
        assert int(undrawn.sum()) == int(new.invalid.item())
    # replicate 0 at SEED: the draw whose window condition tests/test_draw_host.py checks
    ref = ap.draw_list(d["S"], d["C"], kk, pp, occ, d["model"], SEED, 0)
    assert int(undrawn.sum()) == int(ref["invalid"].sum())
    assert np.array_equal(undrawn.cpu().numpy(), ref["invalid"])
    cmp = ref["margin"] > dr.WINDOW
    assert (~cmp).sum() <= 1e-3 * cmp.size
    assert np.array_equal(n_(code)[cmp], ref["code"][cmp])
    if "negative" in d["planted"]:   # the log model's invalid readings: counted and flagged
        assert ref["invalid"].any()
        with pytest.raises(ValueError, match=r"^%d of %d readings cannot be drawn \(%d with"
                           % (int(undrawn.sum()), obs.nnz, int(undrawn.sum()))):
            qmc.draw_readings(*args, occurrence=t_(occ))
    else:
        assert not undrawn.any()
        assert torch.equal(qmc.draw_readings(*args, occurrence=t_(occ)), code)
    if occ.max() == 0:  # occurrence=None means 0
        assert torch.equal(qmc.draw_readings(*args, allow_invalid=True), code)


@pytest.mark.parametrize("form", ["dense", "list"])
@pytest.mark.parametrize("name", list(sl.SHAPES))
def test_occurrences_equal_the_reference_count(name, form):
    from quantized_spectrum_cartography_amd.obs import Observations
    d = sl.problem(name, 2, 5 if form == "list" else 1)
    K, P, J = d["K"], d["P"], d["J"]
    if form == "list":
        obs = from_list(d, d["k"], d["p"], d["c"], 64)
    else:
        Y, Wx = sl.dense_of(d)
        shape = (K, 1, d["I"], J)
        obs = Observations(t_(Y).reshape(shape), t_(Wx.astype(np.float32)).reshape(shape), d["b"],
                           d["sigma"], tile=64)
    mult = np.bincount(d["k"] * P + d["p"], minlength=K * P)
    cells = [int(np.flatnonzero(mult == m)[0]) for m in ((0, 1, 5) if form == "list" else (0, 1))]
    g = np.random.default_rng(3)
    q = np.r_[np.repeat(cells, 3), g.integers(0, K * P, 500)]   # absent, once, five times; repeats
    q = q[g.permutation(q.size)]
    k, p = q // P, q % P
    got = obs.occurrences(t_(k), t_(p // J), t_(p % J))
    assert got.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(n_(got), ap.occurrences(d["k"], d["p"], k, p, P))
    for cell, m in zip(cells, (0, 1, 5)):
        assert sorted(n_(got)[q == cell].tolist())[:3] == [m, m + 1, m + 2]
    with pytest.raises(ValueError, match=r"^2 of 3 cells"):
        obs.occurrences(t_(np.array([0, K, 1])), t_(np.array([0, 0, -1])), t_(np.array([0, 0, 0])))


def test_drawing_a_plan_in_one_batch_or_in_three_gives_the_same_bytes():
    d, obs, S, C = acquire_problem()
    g = np.random.default_rng(5)
    sites = np.stack(np.unravel_index(g.choice(d["P"], SITES, replace=False), (d["I"], d["J"])), 1)
    w = np.ones(d["K"], np.int64)
    w[2], w[5] = 3, 0                                   # cells repeated inside the plan
    k, p = ap.plan(sites, w, d["J"])
    assert ap.cell_counts(d["k"], d["p"], k, p, d["P"]).max() >= 1   # and held by the parent too
    kij = lambda m: (t_(k[m]), t_(p[m] // d["J"]), t_(p[m] % d["J"]))  # noqa: E731
    every = np.ones(k.size, bool)
    one = obs.append(*kij(every), obs.draw(*kij(every), S, C, seed=SEED, replicate=1))
    three = obs
    for part in np.array_split(np.arange(k.size), [k.size // 5, k.size // 2]):
        m = np.zeros(k.size, bool)
        m[part] = True
        three = three.append(*kij(m), three.draw(*kij(m), S, C, seed=SEED, replicate=1))
    assert_same(one, three)
    # and the data are the reference's draw at the occurrence numbers of the whole plan
    occ = ap.occurrences(d["k"], d["p"], k, p, d["P"])
    ref = ap.draw_list(S.reshape(2, -1).double().numpy(), C.double().numpy(), k, p, occ, d["model"],
                       SEED, 1)
    code = n_(obs.draw(*kij(every), S, C, seed=SEED, replicate=1))
    cmp = ref["margin"] > dr.WINDOW
    assert np.array_equal(code[cmp], ref["code"][cmp]) and (~cmp).sum() <= 1e-3 * cmp.size + 1


# ---------------------------------------------------------------------------------------
# the loop closes: planned gain = realised drop
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [False, None])
def test_planned_gain_equals_the_realised_drop_when_the_plan_is_appended(schedule):
    """At fixed (S, C), kind="expected": after the plan (one reading of every bin) is appended at
    the pixels B, sum_r var(S_r) drops by design("A")'s gain and 1/2 logdet(J + ridge I) rises by
    design("D")'s, at every p in B.
    The bound, for design's gains against the fp64 reference and for the realised drops against
    both design's gain and the fp64 reference, is the one tests/test_gpu_design.py applies to these
    gains: max(1e-5, 10 x the fp32 floor) relative to the reference gain (the floor: design_ref's
    fp32 evaluation of the same formulas).  No wider bound is used for the difference of the two
    fp32 variances: none is needed (about 1e-6 relative is measured).
    Every pixel outside B: with schedule=False its block and std_S are the same bits; with the
    default schedule the lists of a slice whose width changed are re-ordered, which moves the
    blocks of B's slice neighbours by summation order, so the blocks are held to rel_fro <= 1e-5,
    as tests/test_gpu_design.py holds them after its re-packing."""
    from conftest import rel_fro
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    name, ridge = "onebit3", 1e-2
    d = gi.problem(name)
    R, K, I, J, P = d["R"], d["K"], gi.I, gi.J, gi.P
    model = (d["b"].double().numpy(), d["sigma"], d["offset"], d["log_model"], d["loss"])
    S64, C64 = d["S"].reshape(R, -1).double().numpy(), d["C"].double().numpy()
    Wx = d["Wx"].reshape(K, I, J)
    k0, i0, j0 = torch.nonzero(Wx, as_tuple=True)
    obs = Observations.from_readings(k0, i0, j0, d["Y"].reshape(K, I, J)[k0, i0, j0], (K, I, J),
                                     d["b"], d["sigma"], tile=gi.TILE, R_hint=R, loss=d["loss"],
                                     schedule=schedule)
    assert obs.schedule == (schedule is None)
    B = [(4, 7), (8, 14), (2, 3)]
    assert all(Wx[:, i, j].sum() > 0 for i, j in B)
    pB = np.array([i * J + j for i, j in B])
    k, p = ap.plan(np.array(B), np.ones(K, np.int64), J)
    before = qmc.confidence(obs, d["S"], d["C"], kind="expected", ridge=ridge)
    gA = qmc.design(obs, d["S"], d["C"], criterion="A", ridge=ridge).gain.reshape(P).cpu().numpy()
    gD = qmc.design(obs, d["S"], d["C"], criterion="D", ridge=ridge).gain.reshape(P).cpu().numpy()
    new = obs.append(t_(k), t_(p // J), t_(p % J), obs.draw(t_(k), t_(p // J), t_(p % J), d["S"],
                                                           d["C"], seed=SEED))
    assert new.schedule == obs.schedule
    after = qmc.confidence(new, d["S"], d["C"], kind="expected", ridge=ridge)
    # fp64 references at the same points
    J0 = ap.expected_blocks(S64, C64, n_(k0), n_(i0) * J + n_(j0), model)
    A = de.plan_blocks(S64, C64, None, *model)
    assert np.allclose(ap.expected_blocks(S64, C64, np.r_[n_(k0), k], np.r_[n_(i0) * J + n_(j0), p],
                                          model)[pB], (J0 + A)[pB], rtol=1e-12)
    keep = np.zeros(P, bool)
    keep[pB] = True
    v0 = (before.std_S.reshape(R, P).double().cpu().numpy() ** 2).sum(0)
    v1 = (after.std_S.reshape(R, P).double().cpu().numpy() ** 2).sum(0)
    i0_, i1_ = (x.info.double().cpu().numpy() for x in (before, after))
    eye = ridge * np.eye(R)
    for crit, got in (("A", gA), ("D", gD)):
        ref, first, bad, piv0, piv1 = de.gains(J0, A, C64, ridge, crit)
        assert not first[pB].any() and not bad[pB].any()
        floor = de.gains_fp32(J0, S64, C64, None, ridge, crit, *model, keep=keep).astype(np.float64)
        f = np.max(np.abs(floor[pB] - ref[pB]) / np.abs(ref[pB]))
        tol = max(1e-5, 10 * f)
        for q in pB:
            if crit == "A":
                drop = v0[q] - v1[q]
            else:
                drop = 0.5 * (np.linalg.slogdet(i1_[q] + eye)[1] - np.linalg.slogdet(i0_[q] + eye)[1])
            e = [abs(got[q] - ref[q]) / abs(ref[q]), abs(drop - got[q]) / abs(ref[q]),
                 abs(drop - ref[q]) / abs(ref[q])]
            print("schedule", obs.schedule, "pixel", q, crit, "gain", got[q], "fp64", ref[q],
                  "realised", drop, "rel err design, drop vs design, drop vs fp64", e, "bound", tol)
            assert e[0] <= tol
            assert e[1] <= tol
            assert e[2] <= tol
    others = t_(~keep)
    if not obs.schedule:
        assert torch.equal(after.info.cpu()[others], before.info.cpu()[others])
        assert torch.equal(after.std_S.reshape(R, P).cpu()[:, others],
                           before.std_S.reshape(R, P).cpu()[:, others])
    e = rel_fro(i1_[~keep], i0_[~keep])
    print("schedule", obs.schedule, "blocks outside B rel_fro", e)
    assert e <= 1e-5
    assert not torch.equal(after.info.cpu()[~others], before.info.cpu()[~others])


# ---------------------------------------------------------------------------------------
# acquire
# ---------------------------------------------------------------------------------------
def test_acquire_bookkeeping_reproducibility_and_refit():
    from quantized_spectrum_cartography_amd import qmc
    d, obs, S, C = acquire_problem()
    K, I, J = d["K"], d["I"], d["J"]
    snap = snapshot(obs)
    w = torch.ones(K)
    w[1] = 2.0
    measure = qmc.acquire.simulate(S, C, seed=SEED)
    run = lambda ridge, **kw: qmc.acquire(obs, S, C, measure, rounds=3, sites=SITES,  # noqa: E731
                                          weights=w, ridge=ridge, **kw)
    # ridge 0: a pixel read in fewer than R bins is a first look (gain +inf), chosen first
    a, b = run(0.0, refit=()), run(0.0, refit=())
    per_round = SITES * (K + 1)
    assert len(a.rounds) == 3 and [r.added for r in a.rounds] == [per_round] * 3
    assert a.obs.nnz == obs.nnz + 3 * per_round and a.obs.codes is None
    assert a.S is S and a.C is C                                   # refit=(): untouched
    assert_untouched(obs, snap)
    assert_same(a.obs, b.obs)                                      # reproducible from the seed
    # the sites are design's best at every stage; the unobserved pixels (gain +inf) come first
    cur = obs
    for r in a.rounds:
        want = qmc.design(cur, S, C, weights=w, ridge=0.0)
        assert tuple(r.sites.shape) == (SITES, 2) and r.sites.dtype == torch.int64
        assert torch.equal(r.sites, want.best(SITES).cpu())
        assert torch.equal(r.gain, want.gain.reshape(-1).cpu()[r.sites[:, 0] * J + r.sites[:, 1]])
        k, p = ap.plan(r.sites.numpy(), w.long().numpy(), J)
        kij = (t_(k), t_(p // J), t_(p % J))
        cur = cur.append(*kij, cur.draw(*kij, S, C, seed=SEED))
    assert_same(cur, a.obs)
    first = a.rounds[0]
    assert qmc.design(obs, S, C, weights=w, ridge=0.0).first_look >= SITES
    assert torch.isinf(first.gain).all()
    pix = first.sites[:, 0] * J + first.sites[:, 1]
    assert (pix[1:] > pix[:-1]).all()                 # equal gains: in pixel order
    # refit: S (and C) move, from the same data; with a ridge every gain is finite
    c = run(1e-2, refit=("S", "C"), ridge_s=1e-2, ridge_c=1e-2)
    c2 = run(1e-2, refit=("S", "C"), ridge_s=1e-2, ridge_c=1e-2)
    assert all(torch.isfinite(r.gain).all() and (r.gain[:-1] >= r.gain[1:]).all() for r in c.rounds)
    assert torch.equal(c.S, c2.S) and torch.equal(c.C, c2.C)
    assert tuple(c.S.shape) == (2, 1, I, J) and tuple(c.C.shape) == (2, K)
    assert torch.isfinite(c.S).all() and torch.isfinite(c.C).all()
    assert not torch.equal(c.S.cpu(), S.reshape(2, 1, I, J)) and c.obs.nnz == a.obs.nnz
