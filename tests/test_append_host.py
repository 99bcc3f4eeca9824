"""CPU: what tests/test_gpu_append.py rests on -- the merge rule of include/qsc.h ("Growing a list
packing") on the reference's sorted arrays, the inputs of the GPU tests (chunk-crossing runs, the
batches), the occurrence numbers, and the argument checks of Observations.append / occurrences,
qmc.draw_readings and qmc.acquire, which raise before any device call (there is no GPU here)."""
import numpy as np
import pytest
import torch

import append_ref as ap
import draw_ref as dr
import readings_ref as rr
import select_ref as sl
from quantized_spectrum_cartography_amd import fits, qmc
from quantized_spectrum_cartography_amd.obs import Observations, check_draw_readings


def natural_perm(P, PT):
    Pp = -(-P // PT) * PT
    return np.r_[np.arange(P)[::-1], -np.ones(Pp - P, np.int64)]  # (any order will do)


@pytest.mark.parametrize("name", list(sl.SHAPES))
@pytest.mark.parametrize("tile", [64, 128])
def test_the_merge_rule_gives_the_sorted_arrays_of_the_concatenated_list(name, tile):
    d = sl.problem(name, 4, 5)
    K, P = d["K"], d["P"]
    perm = natural_perm(P, tile)
    order = ap.exported(d["k"], d["p"], perm)
    pk, pp, pc = d["k"][order], d["p"][order], d["c"][order]
    par = ap.sorted_arrays(pk, pp, pc, K, P, tile, perm)
    psk, pck, _ = ap.sort_keys(pk, pp, K, P, tile, perm)
    for bname, (k, p, c) in ap.batches(name, 4).items():
        if bname == "unseen":
            continue
        want = ap.sorted_arrays(np.r_[pk, k], np.r_[pp, p], np.r_[pc, c], K, P, tile, perm)
        bat = ap.sorted_arrays(k, p, c, K, P, tile, perm)
        bsk, bck, _ = ap.sort_keys(k, p, K, P, tile, perm)
        for fmt, par_key, bat_key in (("s_rd", psk, bsk), ("c_rd", pck, bck)):
            out, ins, rank = ap.merge_sorted(np.sort(par_key), par[fmt], np.sort(bat_key), bat[fmt])
            assert np.array_equal(out, want[fmt]), (bname, fmt)
            assert (np.diff(ins) >= 0).all() and ins.max() <= pk.size and rank.max() <= k.size
        # the new segment tables are the parent's plus the scan of the batch's per-list counts
        assert np.array_equal(want["s_seg"], par["s_seg"] + bat["s_seg"])
        assert np.array_equal(want["c_seg"], par["c_seg"] + bat["c_seg"])
        # ... and the entries are the packer's on the concatenated list
        a = rr.pack(np.r_[pk, k], np.r_[pp, p], np.r_[pc, c], K, P, tile, 4, perm=perm)
        assert a["desc"]["nnz"] == pk.size + k.size
        assert np.array_equal(np.diff(want["s_seg"]), np.bincount(
            ap.positions(np.r_[pp, p], perm, P), minlength=a["desc"]["Pp"]))


def test_the_inputs_are_what_the_gpu_tests_assume():
    d = sl.problem("ragged", 2, 5)
    n = d["k"].size
    assert n > 30000 and n % ap.CHUNK != 0
    for nbins in (2, 4):
        for name in sl.SHAPES:
            dd = sl.problem(name, nbins, 5)
            B = ap.batches(name, nbins)
            assert set(B) == {"single", "m1000", "larger", "one_pixel", "unseen", "repeats",
                              "shuffled"}
            assert B["single"][0].size == 1 and B["larger"][0].size > dd["k"].size
            assert np.unique(B["one_pixel"][1]).size == 1
            assert np.isin(B["unseen"][1], ap.unseen_pixels(name)).all()
            cnt = ap.cell_counts(dd["k"], dd["p"], B["repeats"][0], B["repeats"][1], dd["P"])
            assert (cnt >= 1).all() and dr.occurrence(B["repeats"][0], B["repeats"][1],
                                                      dd["P"]).max() >= 2
            a, b = B["m1000"], B["shuffled"]
            assert not np.array_equal(a[0], b[0])
            key = lambda x: np.lexsort((x[2], x[1], x[0]))  # noqa: E731
            assert all(np.array_equal(u[key(a)], v[key(b)]) for u, v in zip(a, b))
            assert all(x.max() < hi for x, hi in zip(B["larger"], (dd["K"], dd["P"], nbins)))


def test_the_acquire_inputs_are_model_draws_over_the_vec_pattern():
    d, S, C = ap.acquire_inputs()
    src = sl.problem("vec", 2, 5)
    assert (d["K"], d["I"], d["J"]) == sl.SHAPES["vec"] and S.shape == (2, d["P"]) and C.shape == (2, 8)
    assert np.array_equal(d["k"], src["k"]) and np.array_equal(d["p"], src["p"])
    assert set(np.unique(d["c"])) == {0, 1} and 0.2 < d["c"].mean() < 0.8
    assert ap.SITES * 3 <= d["P"]


def test_occurrence_numbers_continue_the_parents():
    d = sl.problem("small", 2, 5)
    P = d["P"]
    k, p = np.r_[d["k"][:20], d["k"][:20], 0], np.r_[d["p"][:20], d["p"][:20], P - 1]
    occ = ap.occurrences(d["k"], d["p"], k, p, P)
    full = dr.occurrence(np.r_[d["k"], k], np.r_[d["p"], p], P)[d["k"].size:]
    assert np.array_equal(occ, full)       # j_occ of the appended readings, by list order
    assert np.array_equal(ap.cell_counts(d["k"], d["p"], d["k"], d["p"], P),
                          np.bincount(d["k"] * P + d["p"])[d["k"] * P + d["p"]])
    w = np.array([1, 0, 2])
    kk, pp = ap.plan(np.array([[1, 2], [0, 3]]), w, 7)
    assert kk.tolist() == [0, 2, 2, 0, 2, 2] and pp.tolist() == [9, 9, 9, 3, 3, 3]


def _fake(K=4, I=3, J=5, loss="probit"):
    """An Observations with a shape and no device state: any device call would fail here."""
    o = Observations.__new__(Observations)
    o.K, o.I, o.J, o.P, o.loss = K, I, J, I * J, loss
    return o


def test_append_and_occurrences_check_the_batch_before_any_device_call():
    o = _fake()
    k = torch.tensor([0, 1])
    for bad in ((k, k, k, k[:1]), (k, k[:1], k, k), (k.float(), k, k, k), (k, k, k, k.float()),
                (k[:0], k[:0], k[:0], k[:0]), (k.reshape(1, 2), k, k, k), ([0, 1], k, k, k)):
        with pytest.raises(ValueError):
            o.append(*bad)
        with pytest.raises(ValueError):
            Observations.check_readings(*bad, (4, 3, 5))
    for bad in ((k, k, k[:1]), (k.float(), k, k), (k[:0], k[:0], k[:0])):
        with pytest.raises(ValueError):
            o.occurrences(*bad)
    assert Observations.check_readings(k, k, k, k, (4, 3, 5)) == (4, 3, 5, 2)


def test_draw_readings_checks_before_any_device_call():
    assert qmc.draw_readings is not None and qmc.check_draw_readings is check_draw_readings
    k = torch.tensor([0, 1, 3])
    S, C = torch.ones(2, 1, 3, 5), torch.ones(2, 4)
    shape, b = (4, 3, 5), [0.0, 1.0, 2.0]
    assert check_draw_readings(k, k, k, S, C, shape, seed=2 ** 64 - 1) == (4, 3, 5, 3, 2, -1)
    assert check_draw_readings(k, k, k, S.reshape(2, 15), C, shape, occurrence=k)[3] == 3
    with pytest.raises(ValueError, match="squared"):
        qmc.draw_readings(k, k, k, S, C, shape, b, 0.5, loss="squared")
    for kw in (dict(seed=2 ** 64), dict(replicate=-1), dict(replicate=2 ** 31),
               dict(occurrence=k[:2]), dict(occurrence=k.float())):
        with pytest.raises(ValueError):
            qmc.draw_readings(k, k, k, S, C, shape, b, 0.5, **kw)
    with pytest.raises(ValueError):
        qmc.draw_readings(k, k, k[:2], S, C, shape, b, 0.5)
    with pytest.raises(ValueError):
        qmc.draw_readings(k, k, k, S, torch.ones(2, 5), shape, b, 0.5)
    with pytest.raises(ValueError):
        qmc.draw_readings(k, k, k, torch.ones(2, 1, 5, 3), C, shape, b, 0.5)
    with pytest.raises(ValueError, match="squared"):
        check_draw_readings(k, k, k, S, C, shape, loss="squared")
    assert callable(_fake().draw) and callable(_fake().occurrences)


def test_acquire_checks_raise_before_any_device_call():
    assert qmc.acquire is fits.acquire and qmc.check_acquire is fits.check_acquire
    assert callable(qmc.acquire.simulate(None, None, 0))
    S, C = torch.ones(2, 1, 3, 5), torch.ones(2, 4)
    measure = lambda k, i, j, obs: k * 0  # noqa: E731
    with pytest.raises(ValueError, match="squared"):
        qmc.acquire(_fake(loss="squared"), S, C, measure, rounds=1, sites=1)
    with pytest.raises(ValueError, match="generator"):
        qmc.acquire(_fake(), S, C, measure, rounds=1, sites=1, generator=torch.nn.Identity())
    for kw in (dict(rounds=0), dict(rounds=1.5), dict(sites=0), dict(sites=16), dict(sites=True),
               dict(criterion="E"), dict(kind="both"), dict(ridge=-1.0), dict(refit=("Z",)),
               dict(weights=torch.ones(3)), dict(weights=torch.tensor([1.0, 0.5, 0.0, 1.0])),
               dict(weights=torch.zeros(4)), dict(weights=torch.tensor([1.0, -1.0, 1.0, 1.0])),
               dict(measure="not callable")):
        args = dict(measure=measure, rounds=1, sites=1)
        args.update(kw)
        with pytest.raises(ValueError):
            qmc.acquire(_fake(), S, C, **args)
    w, refit = fits.check_acquire("probit", measure, 2, 15, [2, 0, 1, 1], 4, refit="S", P=15)
    assert w.tolist() == [2, 0, 1, 1] and w.dtype == torch.int64 and refit == ("S",)
    w, refit = fits.check_acquire("logit", measure, 1, 1, None, 4, refit=())
    assert w.tolist() == [1, 1, 1, 1] and refit == ()
