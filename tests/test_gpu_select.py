"""GPU: subsets of packed observations (qsc_select_codes, qsc_export_codes, qsc_export_readings;
Observations.select / split / folds / readings; solve(obs=, holdout=); qmc.cross_validate) against
the integer reference of tests/select_ref.py.

Shapes (select_ref.SHAPES): (5, 9, 7) one partial tile, P < 64; (70, 23, 21) two bin slices, P = 483
(byte loads, a partial last tile); (8, 32, 32) 16-byte loads.  Each with tiles 64 and 128, 2 and 4
quantiser bins (both row formats), a dense parent and a list parent with up to 5 readings per
cell.  The list of the (70, 23, 21) problem has 35 k readings, no multiple of the compaction chunk
of 1024, and runs of equal keys that cross chunk boundaries (asserted below).  Packings are
compared bit for bit with the packing of the reference-filtered input."""
import numpy as np
import pytest
import torch

import draw_ref as dr
import select_ref as sl
from test_select_host import CV_FOLDS, CV_SEED, RIDGES, cv_reference_cached

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SEED = sl.FOLD_SEED
TABLES = ("perm", "counts", "s_width", "s_off", "c_width", "c_off", "c_kmap", "s_entries",
          "c_entries")
t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def from_list(d, k, p, c, tile, perm=None, schedule=None, R_hint=8):
    from quantized_spectrum_cartography_amd.obs import Observations
    J = d["J"]
    return Observations.from_readings(t_(k), t_(p // J), t_(p % J), t_(c), (d["K"], d["I"], J),
                                      d["b"], d["sigma"], tile=tile, perm=perm, R_hint=R_hint,
                                      schedule=schedule)


def from_dense(d, Y, Wx, tile, perm=None, schedule=None, R_hint=8):
    from quantized_spectrum_cartography_amd.obs import Observations
    shape = (d["K"], 1, d["I"], d["J"])
    return Observations(t_(Y).reshape(shape), t_(Wx.astype(np.float32)).reshape(shape), d["b"],
                        d["sigma"], tile=tile, perm=perm, R_hint=R_hint, schedule=schedule)


def desc_of(obs):
    return {name: getattr(obs.desc, name) for name, _ in obs.desc._fields_}


def assert_same_packing(a, b):
    for f in TABLES:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert desc_of(a) == desc_of(b)
    assert (a.codes is None) == (b.codes is None)
    if a.codes is not None:
        assert torch.equal(a.codes, b.codes)
    else:
        # (the kept sorted readings through their export: `_packed` has unwritten alignment gaps)
        assert all(torch.equal(x, y) for x, y in zip(a.readings(), b.readings()))
        assert a.max_repeat == b.max_repeat


def snapshot(obs):
    arrays = [getattr(obs, f) for f in TABLES] + [obs.codes if obs.codes is not None else obs._packed]
    return arrays, [a.clone() for a in arrays], desc_of(obs)


def assert_untouched(obs, snap):
    arrays, copies, desc = snap
    now = [getattr(obs, f) for f in TABLES] + [obs.codes if obs.codes is not None else obs._packed]
    assert all(a is b for a, b in zip(arrays, now))
    assert all(torch.equal(a, b) for a, b in zip(now, copies))
    assert desc_of(obs) == desc


def parent_of(name, nbins, tile, form, **kw):
    """(problem, parent Observations, pack): pack(mask) packs the readings of the original input
    that `mask` (over the problem's list) keeps, with the parent's perm and tile."""
    d = sl.problem(name, nbins, 5 if form == "list" else 1)
    if form == "list":
        obs = from_list(d, d["k"], d["p"], d["c"], tile, **kw)
        pack = lambda m: from_list(d, d["k"][m], d["p"][m], d["c"][m], tile, perm=obs.perm)  # noqa: E731
    else:
        Y, Wx = sl.dense_of(d)
        obs = from_dense(d, Y, Wx, tile, **kw)

        def pack(m):
            W = np.zeros_like(Wx)
            W[d["k"][m], d["p"][m]] = True
            return from_dense(d, Y, W, tile, perm=obs.perm)
    return d, obs, pack


def masks_of(d, seed=0):
    g = np.random.default_rng(50 + seed)
    return g.random((d["I"], d["J"])) < 0.7, g.random(d["K"]) < 0.8


CASES = [(name, tile, nbins, form) for name in sl.SHAPES for tile in (64, 128) for nbins in (2, 4)
         for form in ("dense", "list")]


@pytest.mark.parametrize("name,tile,nbins,form", CASES)
def test_select_split_folds_are_bit_identical_to_packing_the_filtered_input(name, tile, nbins, form):
    d, obs, pack = parent_of(name, nbins, tile, form)
    assert obs.desc.rowfmt == int(nbins == 2) and obs.desc.PT == tile
    k, p, P = d["k"], d["p"], d["P"]
    snap = snapshot(obs)
    # select: pixel mask, bin mask
    mp, mb = masks_of(d)
    ref = sl.keep(k, p, P, keep_pixel=mp, keep_bin=mb)
    got = obs.select(pixels=t_(mp), bins=t_(mb))
    assert got.nnz == int(ref.sum()) and got.perm is obs.perm
    assert got.loss == obs.loss and got.R_hint == obs.R_hint and got.schedule == obs.schedule
    assert_same_packing(got, pack(ref))
    assert_untouched(obs, snap)
    # split: the two halves partition the parent
    hi = sl.frac_range(0.3)
    held_ref = sl.keep(k, p, P, SEED, 0, hi)
    fit, held = obs.split(0.3, seed=SEED)
    assert held.nnz == int(held_ref.sum()) and fit.nnz + held.nnz == obs.nnz
    assert_same_packing(held, pack(held_ref))
    assert_same_packing(fit, pack(~held_ref))
    assert torch.equal(fit.counts + held.counts, obs.counts)
    assert_untouched(obs, snap)
    # folds: fold 1 of 3, train and test
    folds = obs.folds(3, seed=SEED)
    assert len(folds) == 3
    lo, hi = sl.fold_range(1, 3)
    test_ref = sl.keep(k, p, P, SEED, lo, hi)
    train, test = folds[1]
    assert_same_packing(test, pack(test_ref))
    assert_same_packing(train, pack(~test_ref))
    assert torch.equal(train.counts + test.counts, obs.counts)
    assert_untouched(obs, snap)
    # everything combined: masks and a range, through the rule's own entry
    both = sl.keep(k, p, P, SEED, lo, hi, True, mp, mb)
    kp, kb = obs._masks(t_(mp), t_(mb))
    got = obs._subset(kp, kb, SEED, lo, hi, 1, obs.perm)
    assert_same_packing(got, pack(both))
    assert_untouched(obs, snap)


def exported(obs):
    k, i, j, c = obs.readings()
    assert (k.dtype, i.dtype, j.dtype, c.dtype) == (torch.int32,) * 3 + (torch.uint8,)
    assert k.is_cuda and k.numel() == obs.nnz
    return (k.cpu().numpy().astype(np.int64),
            (i.cpu().numpy().astype(np.int64) * obs.J + j.cpu().numpy()), c.cpu().numpy().astype(np.int64))


@pytest.mark.parametrize("name,tile,nbins,form", CASES)
def test_export_round_trip_and_order(name, tile, nbins, form):
    from quantized_spectrum_cartography_amd.obs import Observations
    d, obs, _ = parent_of(name, nbins, tile, form)
    snap = snapshot(obs)
    k, p, c = exported(obs)
    if form == "dense":
        order = np.argsort(d["k"] * d["P"] + d["p"], kind="stable")          # ascending (k, p)
    else:
        order = sl.sorted_by_position(d["k"], d["p"], obs.perm.cpu().numpy())  # (position, k, occ.)
        n = order.size
        assert n % 1024 != 0
        if name == "ragged":  # a run of equal keys crosses a compaction chunk boundary
            cell = (d["k"] * d["P"] + d["p"])[order]
            assert any(cell[e - 1] == cell[e] for e in range(1024, n, 1024))
    assert np.array_equal(k, d["k"][order]) and np.array_equal(p, d["p"][order])
    assert np.array_equal(c, d["c"][order])
    back = Observations.from_readings(*obs.readings(), (d["K"], d["I"], d["J"]), d["b"], d["sigma"],
                                      perm=obs.perm, tile=obs.desc.PT)
    for f in TABLES:
        assert torch.equal(getattr(back, f), getattr(obs, f)), f
    assert desc_of(back) == desc_of(obs)
    if form == "list":  # (a dense parent exports in (k, p) order, its list twin in position order)
        assert all(torch.equal(x, y) for x, y in zip(back.readings(), obs.readings()))
    assert_untouched(obs, snap)


def test_folds_partition_the_parent_as_exported_sequences():
    for form in ("dense", "list"):
        d, obs, _ = parent_of("ragged", 4, 64, form)
        want = sl.fold_of(d["k"], d["p"], d["P"], 5, SEED)
        key = lambda k, p: k * d["P"] + p  # noqa: E731
        parts, sizes = [], []
        for f, (train, test) in enumerate(obs.folds(5, seed=SEED)):
            k, p, c = exported(test)
            m = want == f
            o = np.argsort(key(k, p), kind="stable")
            r = np.argsort(key(d["k"][m], d["p"][m]), kind="stable")
            assert np.array_equal(k[o], d["k"][m][r]) and np.array_equal(p[o], d["p"][m][r])
            assert np.array_equal(c[o], d["c"][m][r])      # (within a cell: occurrence order)
            assert train.nnz + test.nnz == obs.nnz
            parts.append(test.counts)
            sizes.append(test.nnz)
        assert sum(sizes) == obs.nnz and sizes == np.bincount(want, minlength=5).tolist()
        assert torch.equal(sum(parts[1:], parts[0]), obs.counts)


def test_a_readings_fold_does_not_depend_on_the_packing():
    """Tile, a caller's perm, schedule off, both row formats, dense and list input: the same fold
    for every reading."""
    name, n = "ragged", 3
    d2, d4 = sl.problem(name, 2, 1), sl.problem(name, 4, 1)
    K, P = d2["K"], d2["P"]
    g = torch.Generator().manual_seed(4)
    Pp = -(-P // 64) * 64
    perm = torch.cat([torch.randperm(P, generator=g), -torch.ones(Pp - P, dtype=torch.int64)])
    perm = perm[torch.randperm(Pp, generator=g)].to(torch.int32)
    for d in (d2, d4):
        Y, Wx = sl.dense_of(d)
        want = np.full((K, P), -1, np.int64)
        want[d["k"], d["p"]] = sl.fold_of(d["k"], d["p"], P, n, SEED)
        variants = [from_dense(d, Y, Wx, 64), from_dense(d, Y, Wx, 128),
                    from_dense(d, Y, Wx, 64, perm=perm), from_dense(d, Y, Wx, 64, schedule=False),
                    from_list(d, d["k"], d["p"], d["c"], 64),
                    from_list(d, d["k"], d["p"], d["c"], 128, schedule=False),
                    from_list(d, d["k"], d["p"], d["c"], 64, perm=perm)]
        assert {v.desc.rowfmt for v in variants} == {int(d["nbins"] == 2)}
        for obs in variants:
            got = np.full((K, P), -1, np.int64)
            for f, (_, test) in enumerate(obs.folds(n, seed=SEED)):
                k, p, _c = exported(test)
                assert (got[k, p] == -1).all()
                got[k, p] = f
            assert np.array_equal(got, want)
    # repeated readings: the occurrence number is the list's, whatever the packing
    d = sl.problem(name, 2, 5)
    want = sl.fold_of(d["k"], d["p"], P, n, SEED)
    for obs in (from_list(d, d["k"], d["p"], d["c"], 64), from_list(d, d["k"], d["p"], d["c"], 128),
                from_list(d, d["k"], d["p"], d["c"], 64, perm=perm, schedule=False)):
        held = obs.folds(n, seed=SEED)[2][1]
        k, p, c = exported(held)
        m = want == 2
        o = np.argsort(k * P + p, kind="stable")
        r = np.argsort(d["k"][m] * P + d["p"][m], kind="stable")
        assert np.array_equal(k[o], d["k"][m][r]) and np.array_equal(p[o], d["p"][m][r])
        assert np.array_equal(c[o], d["c"][m][r])


@pytest.mark.parametrize("form", ["dense", "list"])
@pytest.mark.parametrize("name", list(sl.SHAPES))
def test_edges(name, form):
    d, obs, pack = parent_of(name, 2, 64, form)
    k, p, P = d["k"], d["p"], d["P"]
    ones_p = torch.ones(d["I"], d["J"], dtype=torch.bool)
    ones_b = torch.ones(d["K"], dtype=torch.bool)
    # all kept: the parent's own packing; an all-ones mask equals no mask
    a, b = obs.select(), obs.select(pixels=ones_p, bins=ones_b)
    assert_same_packing(a, b)
    assert_same_packing(a, pack(np.ones(k.size, bool)))
    for f in TABLES:
        assert torch.equal(getattr(a, f), getattr(obs, f)), f
    assert a.nnz == obs.nnz == k.size
    # one pixel kept (the most read one)
    px = int(np.bincount(p, minlength=P).argmax())
    one = torch.zeros(P, dtype=torch.bool)
    one[px] = True
    got = obs.select(pixels=one.reshape(d["I"], d["J"]))
    assert got.nnz == int((p == px).sum())
    assert_same_packing(got, pack(p == px))
    # perm="fresh": the order the constructor itself finds for the kept readings
    fresh = obs.select(pixels=one.reshape(d["I"], d["J"]), perm="fresh")
    assert fresh.nnz == got.nnz and torch.equal(fresh.counts, got.counts)
    # nothing left
    with pytest.raises(ValueError, match="no reading"):
        obs.select(bins=torch.zeros(d["K"], dtype=torch.bool))
    with pytest.raises(ValueError, match="no reading"):
        obs.select(pixels=~ones_p)
    # the device counters equal the reference count (the export's n_out through _export)
    mp, mb = masks_of(d, 1)
    lo, hi = sl.fold_range(3, 7)
    ref = sl.keep(k, p, P, 21, lo, hi, False, mp, mb)
    kp, kb = obs._masks(t_(mp), t_(mb))
    assert obs._export(kp, kb, 21, lo, hi, 0)[3] == int(ref.sum())
    assert obs._export(kp, kb, 21, lo, hi, 1)[3] == int(sl.keep(k, p, P, 21, lo, hi, True, mp, mb).sum())
    assert obs._export(None, None, 21, 5, 5, 0)[3] == 0   # an empty range
    if form == "dense":
        # qsc_select_codes' own counter: *kept += the kept cells (masks and a range; "ragged"
        # takes the byte loads, "vec" the 16-byte loads), and the masked codes themselves
        from quantized_spectrum_cartography_amd import _lib
        out = torch.empty_like(obs.codes)
        kept = torch.zeros(1, dtype=torch.int64, device=obs.device)
        assert (P % 16 == 0) == (name == "vec") and out.data_ptr() % 16 == 0
        for invert, want in ((0, ref), (1, sl.keep(k, p, P, 21, lo, hi, True, mp, mb))):
            before = int(kept.item())
            for rep in (1, 2):  # the second call adds the same amount to the un-zeroed counter
                _lib.call("qsc_select_codes", _lib.ptr(obs.codes), d["K"], P, _lib.ptr(kp),
                          _lib.ptr(kb), 21, lo, hi, invert, _lib.ptr(out), _lib.ptr(kept),
                          _lib.stream())
                assert int(kept.item()) == before + rep * int(want.sum())
            codes = np.full((d["K"], P), 0xFF, np.uint8)
            codes[k[want], p[want]] = d["c"][want]
            assert np.array_equal(out.cpu().numpy(), codes)
        # no masks, the range rule off: everything is kept and counted
        kept.zero_()
        _lib.call("qsc_select_codes", _lib.ptr(obs.codes), d["K"], P, None, None, 0, 0, 1 << 24, 0,
                  _lib.ptr(out), _lib.ptr(kept), _lib.stream())
        assert int(kept.item()) == k.size and torch.equal(out, obs.codes)
    # a 64-bit seed with the top bit set
    big = 2 ** 64 - 12345
    fit, held = obs.split(0.5, seed=big)
    assert held.nnz == int(sl.keep(k, p, P, big, 0, sl.frac_range(0.5)).sum())


def test_works_on_resampled_and_remodelled_parents_and_squared_loss():
    from quantized_spectrum_cartography_amd.obs import Observations
    d, obs, _ = parent_of("vec", 2, 64, "dense")
    g = torch.Generator().manual_seed(1)
    S, C = torch.rand(2, 1, d["I"], d["J"], generator=g) + 0.5, torch.rand(2, d["K"], generator=g) + 0.5
    for parent in (obs.resample(S, C, seed=3), obs.with_model(noise_std=0.9)):
        fit, held = parent.split(0.25, seed=SEED)
        ref = sl.keep(d["k"], d["p"], d["P"], SEED, 0, sl.frac_range(0.25))
        assert held.nnz == int(ref.sum()) and torch.equal(fit.counts + held.counts, parent.counts)
        assert held.noise_std == parent.noise_std and held.model is parent.model
        m = np.zeros((d["K"], d["P"]), bool)
        m[d["k"][ref], d["p"][ref]] = True
        assert torch.equal(held.codes.cpu() != 0xFF, t_(m))
        assert torch.equal(held.codes.cpu()[t_(m)], parent.codes.cpu()[t_(m)])
    Y, Wx = sl.dense_of(d)
    shape = (d["K"], 1, d["I"], d["J"])
    sq = Observations(t_(Y).reshape(shape), t_(Wx.astype(np.float32)).reshape(shape), d["b"],
                      d["sigma"], tile=64, loss="squared")
    fit, held = sq.split(0.25, seed=SEED)
    assert held.loss == "squared" and held.nnz == int(ref.sum())
    # a calibrate result: the split carries the calibrated model
    from quantized_spectrum_cartography_amd import qmc
    bd = dr.boot_problem()
    bobs, S, C = boot_obs()
    cal = qmc.calibrate(bobs, S, C, rounds=1, ridge_s=1e-3, ridge_c=1e-3).obs
    assert cal is not bobs and cal.noise_std != bobs.noise_std
    k, p = np.nonzero(bd["Wx"])
    ref = sl.keep(k, p, bd["P"], SEED, 0, sl.frac_range(0.25), j=np.zeros(k.size, np.int64))
    fit, held = cal.split(0.25, seed=SEED)
    assert held.nnz == int(ref.sum()) and torch.equal(fit.counts + held.counts, cal.counts)
    assert held.noise_std == cal.noise_std and held.bin_boundaries == cal.bin_boundaries
    assert held.model is cal.model and fit.perm is cal.perm
    assert np.isfinite(qmc.model_nll(held, S, C))


def test_graph_captured_on_the_parent_replays_unchanged_after_select():
    from quantized_spectrum_cartography_amd.obs import Observations
    from quantized_spectrum_cartography_amd.qmc import FreeSSolver
    from test_gpu_fused import _random_case
    d = _random_case(81, 4, 32, 32, 8, f=0.3)
    mk = lambda: Observations(d["Y"], d["Wx"], d["b"], d["sigma"], R_hint=4, tile=256)  # noqa: E731
    obs = mk()
    sol = FreeSSolver(obs, d["S0"], d["C0"], hist_cap=64)
    sol.run(3, use_graph=True)
    snap = snapshot(obs)
    obs.select(bins=torch.arange(8) % 2 == 0)
    obs.split(0.3, seed=1)
    obs.folds(4)[2]
    obs.readings()
    assert_untouched(obs, snap)
    sol.run(3, use_graph=True)
    ref = FreeSSolver(mk(), d["S0"], d["C0"], hist_cap=64)
    ref.run(6, use_graph=False)
    assert np.array_equal(ref.S.cpu().numpy(), sol.S.cpu().numpy())
    assert np.array_equal(ref.C.cpu().numpy(), sol.C.cpu().numpy())


@pytest.mark.parametrize("form", ["dense", "list"])
def test_solve_with_obs_and_holdout_equals_the_split_by_hand(form):
    from quantized_spectrum_cartography_amd import qmc
    from quantized_spectrum_cartography_amd.obs import Observations
    from test_gpu_fused import _random_case
    d = _random_case(82, 3, 32, 32, 8, f=0.5)
    if form == "dense":
        obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], R_hint=3)
    else:
        k, _, i, j = torch.nonzero(d["Wx"], as_tuple=True)
        obs = Observations.from_readings(k, i, j, d["Y"][k, 0, i, j], (8, 32, 32), d["b"],
                                         d["sigma"], R_hint=3)
    kw = dict(R=3, S_init=d["S0"], C_init=d["C0"], max_iter=40, check_every=5, patience=2)
    a = qmc.solve(None, None, d["b"], d["sigma"], obs=obs, holdout=0.2, holdout_seed=5, **kw)
    fit, held = obs.split(0.2, seed=5)
    b = qmc.solve(None, None, d["b"], d["sigma"], obs=fit, obs_holdout=held, **kw)
    assert a.obs.nnz == fit.nnz and a.obs_holdout.nnz == held.nnz
    assert_same_packing(a.obs, fit)
    assert_same_packing(a.obs_holdout, held)
    assert torch.equal(a.S, b.S) and torch.equal(a.C, b.C)
    assert a.best_iter == b.best_iter and a.holdout_nll == b.holdout_nll and len(a.holdout_nll) >= 2


def boot_obs():
    from quantized_spectrum_cartography_amd.obs import Observations
    c, d = dr.BOOT, dr.boot_problem()
    shape = (c["K"], 1, c["I"], c["J"])
    obs = Observations(t_(d["Y"]).reshape(shape), t_(d["Wx"].astype(np.float32)).reshape(shape),
                       torch.tensor(d["b"]), c["sigma"], R_hint=c["R"])
    S = t_(d["S"]).float().reshape(c["R"], 1, c["I"], c["J"])
    return obs, S, t_(d["C"]).float()


def test_cross_validate_equals_the_manual_loop_and_ranks_two_ridges():
    from quantized_spectrum_cartography_amd import qmc
    c, d = dr.BOOT, dr.boot_problem()
    obs, S, C = boot_obs()
    fits = {r: (lambda tr, r=r: (qmc.fit_S(tr, C, ridge=r).S, C)) for r in RIDGES}
    cv = {r: qmc.cross_validate(obs, fits[r], folds=CV_FOLDS, seed=CV_SEED) for r in RIDGES}
    # the manual loop, exactly
    k, p = np.nonzero(d["Wx"])
    want_fold = sl.fold_of(k, p, d["P"], CV_FOLDS, CV_SEED)
    r0 = RIDGES[0]
    manual = []
    for f, (train, test) in enumerate(obs.folds(CV_FOLDS, seed=CV_SEED)):
        assert test.nnz == int((want_fold == f).sum()) == cv[r0].n_test[f]
        assert train.nnz == cv[r0].n_train[f] == obs.nnz - test.nnz
        manual.append(qmc.model_nll(test, qmc.fit_S(train, C, ridge=r0).S, C) / test.nnz)
        # model_nll of a subset against fp64, at the existing model_nll test's tolerance
        te = np.zeros_like(d["Wx"])
        te[k[want_fold == f], p[want_fold == f]] = True
        ref = dr.nll(d["S"], d["C"], d["Y"], te, d["model"])
        got = qmc.model_nll(test, S, C)
        print("fold %d model_nll rel err %.2e" % (f, abs(got - ref) / abs(ref)))
        assert abs(got - ref) <= 8 * ULP * abs(ref)
    assert manual == cv[r0].nll
    assert cv[r0].mean == sum(manual) / CV_FOLDS
    var = sum((v - cv[r0].mean) ** 2 for v in manual) / (CV_FOLDS - 1)
    assert cv[r0].stderr == (var / CV_FOLDS) ** 0.5
    # the ranking the fp64 reference has (tests/test_select_host.py): the small ridge in every fold
    print("held-out NLL per reading", {r: cv[r].nll for r in RIDGES},
          "fp64", {r: cv_reference_cached(r) for r in RIDGES})
    assert all(a < b for a, b in zip(cv[RIDGES[0]].nll, cv[RIDGES[1]].nll))
    assert cv[RIDGES[0]].mean < cv[RIDGES[1]].mean
    # a solve as the recipe: an object with .S and .C is accepted
    res = qmc.cross_validate(obs, lambda tr: qmc.solve(
        None, None, d["b"], c["sigma"], R=c["R"], obs=tr, S_init=S, C_init=C, max_iter=5), folds=2)
    assert len(res.nll) == 2 and all(np.isfinite(res.nll))
    with pytest.raises(IndexError):
        obs.folds(2)[2]
