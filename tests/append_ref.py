"""CPU reference (numpy, exact integer arithmetic) of growing a list packing -- a helper for
tests/test_append_host.py and tests/test_gpu_append.py, not a test file.  Written from include/qsc.h
("Growing a list packing", qsc_draw_list); it imports nothing of the package and is built on
tests/readings_ref.py (the packer), tests/draw_ref.py (Philox, occurrence, the draw) and
tests/select_ref.py (the problems and the exported order).

The reference of an append IS the packing of the concatenated list: readings_ref.pack(parent in
exported order + batch).  Beside it stand the caller-kept sorted readings (sorted_arrays: what
`_packed` holds), the merge rule on them (merge_sorted: i + ins[i], e + #{ins <= e}), the cell
counts and occurrence numbers, the draw at listed cells and the plan of an acquisition round."""
import numpy as np

import draw_ref as dr
import readings_ref as rr
import select_ref as sl

CHUNK = 1024          # QSC_MERGE_CHUNK: parent readings per workgroup of the merge
IDX_BITS = 24
ALIGN = 256           # every array of `_packed` starts on a multiple of it


def _up(x, m):
    return -(-x // m) * m


def dims(K, P, PT):
    Pp = _up(P, PT)
    nt, nks = Pp // PT, -(-K // 64)
    return dict(Pp=Pp, nt=nt, nks=nks, Kp=nks * 64, nb=nt * nks * 64)


def positions(p, perm, P):
    perm = np.asarray(perm, np.int64)
    iperm = np.full(P, -1, np.int64)
    iperm[perm[perm >= 0]] = np.flatnonzero(perm >= 0)
    return iperm[np.asarray(p, np.int64)]


def sort_keys(k, p, K, P, PT, perm):
    """(S-format key, C-format key, qlocal) of every reading: (position, k) and (tile, bin, qlocal)
    as single integers."""
    d = dims(K, P, PT)
    k = np.asarray(k, np.int64)
    pos = positions(p, perm, P)
    t, ql = rr.tile_of(pos, d["nt"])
    return pos * K + k, (t * d["Kp"] + k) * PT + ql, ql


def sorted_arrays(k, p, c, K, P, PT, perm):
    """The caller-kept sorted readings of a list, in list order on equal keys: dict(s_rd, c_rd
    uint32 (idx | code << 24), s_seg, c_seg, c_kinv int32)."""
    d = dims(K, P, PT)
    k, c = np.asarray(k, np.int64), np.asarray(c, np.int64)
    sk, ck, ql = sort_keys(k, p, K, P, PT, perm)
    so, co = np.argsort(sk, kind="stable"), np.argsort(ck, kind="stable")
    poscnt = np.bincount(sk // K, minlength=d["Pp"])
    ccount = np.bincount(ck // PT, minlength=d["nb"]).reshape(d["nt"], d["Kp"])
    order_cnt = ccount.copy()
    order_cnt[:, K:] = -1
    kmap = np.argsort(-order_cnt, axis=1, kind="stable")
    kinv = np.empty_like(kmap)
    np.put_along_axis(kinv, kmap, np.broadcast_to(np.arange(d["Kp"]), kmap.shape), axis=1)
    return dict(s_rd=(k[so] | (c[so] << IDX_BITS)).astype(np.uint32),
                c_rd=(ql[co] | (c[co] << IDX_BITS)).astype(np.uint32),
                s_seg=np.r_[0, np.cumsum(poscnt)].astype(np.int32),
                c_seg=np.r_[0, np.cumsum(ccount.reshape(-1))].astype(np.int32),
                c_kinv=kinv.reshape(-1).astype(np.int32))


def packed_views(raw, n, K, P, PT):
    """The five arrays of a `_packed` byte array (numpy uint8) for n readings."""
    d = dims(K, P, PT)
    out, o = {}, 0
    for name, count, dt in (("s_rd", n, np.uint32), ("c_rd", n, np.uint32),
                            ("s_seg", d["Pp"] + 1, np.int32), ("c_seg", d["nb"] + 1, np.int32),
                            ("c_kinv", d["nb"], np.int32)):
        out[name] = raw[o:o + 4 * count].view(dt)
        o += _up(4 * count, ALIGN)
    assert o == raw.size
    return out


def merge_sorted(par_key, par_val, bat_key, bat_val):
    """The merge rule of include/qsc.h on one sorted array: parent (keys ascending) and sorted batch
    -> (merged values, ins, rank of every parent reading)."""
    ins = np.searchsorted(par_key, bat_key, side="right")      # parent readings with key <= it
    rank = np.searchsorted(ins, np.arange(par_key.size), side="right")  # batch readings in front
    out = np.empty(par_key.size + bat_key.size, par_val.dtype)
    out[np.arange(bat_key.size) + ins] = bat_val
    out[np.arange(par_key.size) + rank] = par_val
    return out, ins, rank


def exported(k, p, perm):
    """A list in the order Observations.readings() gives for its list packing."""
    return sl.sorted_by_position(k, p, perm)


def cell_counts(pk, pp, k, p, P):
    """How often the parent list (pk, pp) holds every cell (k, p)."""
    cells, cnt = np.unique(np.asarray(pk, np.int64) * P + np.asarray(pp, np.int64),
                           return_counts=True)
    q = np.asarray(k, np.int64) * P + np.asarray(p, np.int64)
    at = np.searchsorted(cells, q)
    hit = (at < cells.size) & (cells[np.minimum(at, cells.size - 1)] == q)
    return np.where(hit, cnt[np.minimum(at, cells.size - 1)], 0)


def occurrences(pk, pp, k, p, P):
    """j_occ of every reading of the batch (k, p) once appended to the parent list."""
    return cell_counts(pk, pp, k, p, P) + dr.occurrence(k, p, P)


def draw_list(S, C, k, p, occ, model, seed=0, replicate=0):
    """qsc_draw_list in fp64: dict(code (0xFF where nothing is drawn), invalid, margin)."""
    S, C = np.asarray(S, np.float64), np.asarray(C, np.float64)
    k, p = np.asarray(k, np.int64), np.asarray(p, np.int64)
    u = dr.uniform(k, p, np.asarray(occ, np.int64), replicate, seed)
    t = np.einsum("rn,rn->n", S[:, p], C[:, k])
    code, inv, margin, _ = dr.draw(t, u, np.full(k.size, 0xFF, np.int64), *model)
    return dict(code=code, invalid=inv, margin=margin)


def plan(sites, weights, J):
    """(k, p) of an acquisition round: weights[k] readings of bin k at every site (rows (i, j)),
    site by site, bins ascending."""
    w = np.asarray(weights, np.int64)
    bins = np.repeat(np.arange(w.size), w)
    sites = np.asarray(sites, np.int64)
    pix = sites[:, 0] * J + sites[:, 1]
    return np.tile(bins, pix.size), np.repeat(pix, bins.size)


SITES = 16            # sites per round of the acquire tests
_ACQ = {}


def acquire_inputs():
    """The (8, 32, 32), R = 2 synthetic problem of the acquire tests: (d, S (2, P), C (2, K)), fp32
    numpy.  The pattern is select_ref's "vec" list (up to 5 readings per cell), the codes are this
    reference's draws from the truth (S, C), one-bit probit."""
    if not _ACQ:
        src = sl.problem("vec", 2, 5)
        K, I, J, P = src["K"], src["I"], src["J"], src["P"]
        g = np.random.default_rng(321)
        S = (0.2 + 0.8 * g.random((2, P))).astype(np.float32)
        C = (0.1 + 0.9 * g.random((2, K))).astype(np.float32)
        T = C.astype(np.float64).T @ S.astype(np.float64)
        b = [0.0, float(np.float32(np.median(T))), float(np.float32(T.max() + 1.0))]
        model = (b, 0.4, 0.0, False, "probit")
        occ = dr.occurrence(src["k"], src["p"], P)
        c = draw_list(S, C, src["k"], src["p"], occ, model, seed=99)["code"]
        _ACQ.update(d=dict(k=src["k"], p=src["p"], c=c, K=K, I=I, J=J, P=P, b=b, sigma=0.4,
                           model=model), S=S, C=C)
    return _ACQ["d"], _ACQ["S"], _ACQ["C"]


_BATCHES = {}


def batches(name, nbins, seed=0):
    """The batches of the append tests for the list parent sl.problem(name, nbins, 5): name ->
    (k, p, c) int64.  `single` one reading; `m1000`; `larger` m > n; `one_pixel` every reading into
    one pixel; `unseen` only pixels the parent never saw (the parent used with it is the problem
    without those pixels: see unseen_pixels); `repeats` cells repeated inside the batch that the
    parent holds too; `shuffled` the m1000 batch in another order."""
    key = (name, nbins, seed)
    if key not in _BATCHES:
        d = sl.problem(name, nbins, 5)
        K, P, n = d["K"], d["P"], d["k"].size
        g = np.random.default_rng(7000 + 13 * sorted(sl.SHAPES).index(name) + nbins + seed)

        def rand(m):
            return g.integers(0, K, m), g.integers(0, P, m), g.integers(0, nbins, m)
        out = {"single": rand(1), "m1000": rand(1000), "larger": rand(n + 37)}
        k, _, c = rand(300)
        out["one_pixel"] = (k, np.full(300, int(d["p"][0])), c)
        k, _, c = rand(200)
        out["unseen"] = (k, g.choice(unseen_pixels(name), 200), c)
        pick = g.integers(0, n, 40)                       # cells the parent holds ...
        k, p = np.repeat(d["k"][pick], 3), np.repeat(d["p"][pick], 3)   # ... three times each
        o = g.permutation(k.size)
        out["repeats"] = (k[o], p[o], g.integers(0, nbins, k.size))
        o = g.permutation(1000)
        out["shuffled"] = tuple(a[o] for a in out["m1000"])
        _BATCHES[key] = {b: tuple(np.asarray(a, np.int64) for a in v) for b, v in out.items()}
    return _BATCHES[key]


def unseen_pixels(name):
    """The pixels the `unseen` batch goes to (every seventh): its parent is the problem's list
    without their readings."""
    K, I, J = sl.SHAPES[name]
    return np.arange(0, I * J, 7)


def expected_blocks(S, C, k, p, model):
    """J (P, R, R) in fp64 of kind "expected" for a LIST of readings (cells may repeat): every
    reading of cell (k, p) adds h_exp(t_kp) c_k c_k^T, whatever its code (design_ref's h_exp)."""
    import design_ref as de
    S, C = np.asarray(S, np.float64), np.asarray(C, np.float64)
    h = de.expected_information(S, C, *model)                     # (K, P)
    n = np.zeros_like(h)
    np.add.at(n, (np.asarray(k, np.int64), np.asarray(p, np.int64)), 1.0)
    return np.einsum("kp,rk,sk->prs", n * h, C, C)
