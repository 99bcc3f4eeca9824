"""GPU: the shared tile, walks and occurrence rule of the observation-container kernels
(qsc_obs_tile.cuh, qsc_obs_readings.cuh) at the two sizes the other suites do not reach, against
the CPU references draw_ref / select_ref.

Dense, more than one tile per bin: tests/test_gpu_check.py's cases stop at P = 130 and
select_ref.SHAPES at P = 1024, so neither the dense draw nor the dense select has run a second
tile of a bin, nor a ragged one.  (3, 66, 64): P = 4224, 16-byte loads, 128 cells in the second
tile; (3, 63, 67): P = 4221, byte loads.  Two bins, and four bins with the log model.

A run of equal cells across chunk boundaries: a list packing whose pixel 17 holds 3 bins x 700
readings and a few dozen single readings elsewhere (n = 2140 > 2048).  With pixel 17 at position 0
the runs are [0, 700), [700, 1400), [1400, 2100): the export's chunk boundaries 1024 and 2048 fall
inside runs (asserted from the reference's order before anything runs), and the one wave that
walks slice 0 looks back along runs 700 long.

(A wave past the last slice of the slice walk is reached already: tests/test_gpu_draw.py's
"readings11" is a list packing with Pp = 192 and tile 64, six slices in workgroups of four waves,
filled and resampled.)"""
import numpy as np
import pytest
import torch

import draw_ref as dr
import select_ref as sl
import test_gpu_check as tgc
from test_gpu_draw import cell_codes
from test_gpu_select import TABLES, assert_same_packing, desc_of, exported, from_list

pytestmark = pytest.mark.gpu

SEED = 11
TILE_CELLS = 4096     # QSC_EXPORT_CHUNK_CODES: cells per workgroup of the dense kernels
CHUNK = 1024          # QSC_EXPORT_CHUNK_READINGS
SHAPES = {"vec": (3, 66, 64), "bytes": (3, 63, 67)}
t_ = lambda a: torch.from_numpy(np.array(a))  # noqa: E731  (a copy: the shared inputs are read-only)
_DENSE = {}


def dense_problem(shape, model):
    """test_gpu_check.problem's recipe at R = 3 and a shape of SHAPES, 30 % of the cells read;
    with the fp64 reference of resample(seed=SEED).  Built once, read-only."""
    if (shape, model) in _DENSE:
        return _DENSE[(shape, model)]
    (K, I, J), R, sigma = SHAPES[shape], 3, 0.5
    P = I * J
    g = np.random.default_rng(40 + 2 * sorted(SHAPES).index(shape) + (model == "log4"))
    log_model = model == "log4"
    offset = 1e-3 if log_model else 0.0
    S = 3.0 + 7.0 * g.random((R, P)) if log_model else 0.2 + 0.8 * g.random((R, P))
    C = 0.1 + 0.9 * g.random((R, K))
    S, C = S.astype(np.float32).astype(np.float64), C.astype(np.float32).astype(np.float64)
    T = C.T @ S
    if log_model:
        x = np.log(T + offset)
        q = np.quantile(x, [0.25, 0.5, 0.75])
        b = [-23.025850296020508, float(q[0]), float(q[1]), float(q[2]), float(x.max()) + 0.5]
        S[:, P - 1] = [-1.0, 1.0, -1.0]  # t + offset <= 0 for some bins: in the last, ragged tile
    else:
        x = T
        b = [0.0, float(np.median(T)), float(T.max()) + 1.0]
    b = [float(np.float32(v)) for v in b]
    Y = tgc.draw_codes(g, x, b, sigma, "probit", log_model)
    Wx = g.random((K, P)) < 0.3
    Wx[:, P - 1] = True
    mdl = (b, sigma, offset, log_model, "probit")
    Yn, ref = dr.resample_dense(S, C, Y, Wx, mdl, SEED, 0)
    for a in (S, C, Y, Wx, Yn):
        a.setflags(write=False)
    d = dict(K=K, I=I, J=J, P=P, R=R, S=S, C=C, Y=Y, Wx=Wx, b=b, sigma=sigma, offset=offset,
             log_model=log_model, model=mdl, ref=ref)
    _DENSE[(shape, model)] = d
    return d


@pytest.mark.parametrize("model", ["onebit", "log4"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_dense_draw_and_split_over_two_tiles_per_bin_with_a_ragged_last_tile(shape, model):
    from quantized_spectrum_cartography_amd.obs import Observations
    d = dense_problem(shape, model)
    K, I, J, P, R, Wx, r = d["K"], d["I"], d["J"], d["P"], d["R"], d["Wx"], d["ref"]
    assert TILE_CELLS < P < 2 * TILE_CELLS and (P % 16 == 0) == (shape == "vec")
    assert Wx[:, TILE_CELLS:].any(axis=1).all()       # every bin has readings in its second tile
    obs = Observations(t_(d["Y"]).reshape(K, 1, I, J), t_(Wx.astype(np.float32)).reshape(K, 1, I, J),
                       torch.tensor(d["b"]), d["sigma"], offset=d["offset"],
                       log_model=d["log_model"], tile=256, R_hint=R)
    kept = obs.codes.clone()
    # the draw against draw_ref, outside its window
    S, C = t_(d["S"]).float().reshape(R, 1, I, J), t_(d["C"]).float()
    new = obs.resample(S, C, seed=SEED, replicate=0)
    codes = new.codes.cpu().numpy()
    assert np.array_equal(codes == 0xFF, ~Wx)
    cmp = r["margin"] > dr.WINDOW
    got = codes[r["k"], r["p"]].astype(np.int64)
    print(shape, model, "compared", int(cmp.sum()), "of", cmp.size, "differing",
          int((got[cmp] != r["code"][cmp]).sum()), "invalid", int(r["invalid"].sum()))
    assert (~cmp).sum() <= 1e-3 * cmp.size
    assert np.array_equal(got[cmp], r["code"][cmp])
    assert int(new.invalid.item()) == int(r["invalid"].sum())
    assert r["invalid"].any() == d["log_model"]
    assert (got[r["p"] >= TILE_CELLS] != d["Y"][r["k"], r["p"]][r["p"] >= TILE_CELLS]).any()
    # the split against select_ref: the two halves' codes, cell by cell
    held_ref = np.zeros((K, P), bool)
    held_ref[r["k"], r["p"]] = sl.keep(r["k"], r["p"], P, SEED, 0, sl.frac_range(0.3))
    fit, held = obs.split(0.3, seed=SEED)
    Yc = d["Y"].astype(np.uint8)
    assert np.array_equal(held.codes.cpu().numpy(), np.where(Wx & held_ref, Yc, 0xFF))
    assert np.array_equal(fit.codes.cpu().numpy(), np.where(Wx & ~held_ref, Yc, 0xFF))
    assert held.nnz == int((Wx & held_ref).sum()) and fit.nnz + held.nnz == obs.nnz
    assert held_ref[:, TILE_CELLS:].any() and (Wx & ~held_ref)[:, TILE_CELLS:].any()
    assert torch.equal(fit.counts + held.counts, obs.counts) and torch.equal(obs.codes, kept)


def straddle_problem():
    """(problem dict as select_ref's, perm): K = 3 bins x 700 readings at pixel 17, one reading at
    each of 40 other cells, shuffled; perm puts pixel 17 at position 0."""
    K, I, J, big, reps = 3, 9, 7, 17, 700
    P = I * J
    g = np.random.default_rng(5)
    others = np.setdiff1d(np.arange(P), [big])
    k = np.r_[np.repeat(np.arange(K), reps), g.integers(0, K, 40)]
    p = np.r_[np.full(K * reps, big), g.choice(others, 40, replace=False)]
    o = g.permutation(k.size)
    k, p = k[o].astype(np.int64), p[o].astype(np.int64)
    c = g.integers(0, 2, k.size).astype(np.int64)
    perm = np.full(64, -1, np.int32)
    perm[:P] = np.r_[big, others]
    return dict(k=k, p=p, c=c, K=K, I=I, J=J, P=P, b=[0.0, 1.0, 3.0], sigma=0.5, nbins=2), perm


def test_a_run_of_equal_cells_across_chunk_boundaries_of_the_export_and_the_slice_walk():
    from quantized_spectrum_cartography_amd.obs import Observations
    d, perm = straddle_problem()
    k, p, c, P, n = d["k"], d["p"], d["c"], d["P"], d["k"].size
    # the condition on the input, from the reference's order alone
    order = sl.sorted_by_position(k, p, perm)
    cell = (k * P + p)[order]
    inside = [e for e in range(CHUNK, n, CHUNK) if cell[e - 1] == cell[e]]
    assert n > 2 * CHUNK and inside == [CHUNK, 2 * CHUNK]
    obs = from_list(d, k, p, c, 64, perm=t_(perm))
    assert obs.max_repeat == 700 and obs.Pp == 64
    # readings() round-trips, in (position, k, occurrence) order
    ek, ep, ec = exported(obs)
    assert np.array_equal(ek, k[order]) and np.array_equal(ep, p[order])
    assert np.array_equal(ec, c[order])
    back = Observations.from_readings(*obs.readings(), (d["K"], d["I"], d["J"]), d["b"], d["sigma"],
                                      perm=obs.perm, tile=64)
    assert all(torch.equal(getattr(back, f), getattr(obs, f)) for f in TABLES)
    assert desc_of(back) == desc_of(obs)
    assert all(torch.equal(x, y) for x, y in zip(back.readings(), obs.readings()))
    # split(0.5) partitions the parent exactly as select_ref says
    held_ref = sl.keep(k, p, P, SEED, 0, sl.frac_range(0.5))
    assert 0.4 * n < held_ref.sum() < 0.6 * n
    fit, held = obs.split(0.5, seed=SEED)
    pack = lambda m: from_list(d, k[m], p[m], c[m], 64, perm=obs.perm)  # noqa: E731
    assert_same_packing(held, pack(held_ref))
    assert_same_packing(fit, pack(~held_ref))
    assert fit.nnz + held.nnz == n
    # resample: occurrence j of a cell gets draw_ref's code, and the same one in both formats
    g = np.random.default_rng(6)
    S = (0.2 + 0.8 * g.random((2, P))).astype(np.float32)
    C = (0.5 + 1.5 * g.random((2, d["K"]))).astype(np.float32)
    r = dr.resample_readings(S, C, k, p, c, (d["b"], d["sigma"], 0.0, False, "probit"), SEED, 2)
    assert r["j"].max() == 699
    new = obs.resample(t_(S).reshape(2, 1, d["I"], d["J"]), t_(C), seed=SEED, replicate=2)
    nk, np_, nc = exported(new)
    cmp = r["margin"][order] > dr.WINDOW
    assert np.array_equal(nk, ek) and np.array_equal(np_, ep) and (~cmp).sum() <= 1e-3 * n
    assert np.array_equal(nc[cmp], r["code"][order][cmp])
    assert len(set(nc[cell == cell[CHUNK]].tolist())) == 2   # the occurrences are drawn separately
    s_side, c_side = cell_codes(new)
    assert s_side == c_side and sum(len(v) for v in s_side.values()) == n
