"""CPU reference (numpy, integer arithmetic only) of the keep rule of include/qsc.h
(qsc_select_codes / qsc_export_codes / qsc_export_readings) and of the range arithmetic of
Observations.split / folds -- a helper for tests/test_select_host.py and tests/test_gpu_select.py,
not a test file.  It imports nothing of the package and is built on tests/draw_ref.py's n24 and
occurrence with the replicate word 0x80000000.

Reading (k, p, j_occ) is kept iff
    keep_pixel[p] != 0  and  keep_bin[k] != 0  and  ((lo <= u24 < hi) != invert)
    u24 = philox4x32_10(counter (k, p, j_occ, 0x80000000), key (seed lo, seed hi))[0] >> 8
"""
import numpy as np

import draw_ref as dr

STREAM = 0x80000000
RANGE = 1 << 24
# (K, I, J) of the GPU tests: one partial tile with P < 64; two bin slices with P = 483 (no
# multiple of 16: byte loads, a partial last tile); P a multiple of 16 (16-byte loads)
SHAPES = {"small": (5, 9, 7), "ragged": (70, 23, 21), "vec": (8, 32, 32)}
FOLD_SEED = 3  # test_select_host.py checks the fold sizes of the ragged problem at this seed


def u24(k, p, j, seed):
    return dr.n24(np.asarray(k, np.int64), np.asarray(p, np.int64), np.asarray(j, np.int64),
                  STREAM, seed)


def frac_range(frac):
    """hi of split(frac)'s held-out range [0, hi)."""
    return min(max(int(round(float(frac) * RANGE)), 1), RANGE - 1)


def fold_range(f, n):
    return (f << 24) // n, ((f + 1) << 24) // n


def keep(k, p, P, seed=0, lo=0, hi=RANGE, invert=False, keep_pixel=None, keep_bin=None, j=None):
    """The kept mask of the readings (k, p) in list order (j: their occurrence numbers; default
    by list order)."""
    k, p = np.asarray(k, np.int64), np.asarray(p, np.int64)
    j = dr.occurrence(k, p, P) if j is None else np.asarray(j, np.int64)
    u = u24(k, p, j, seed)
    out = ((u >= lo) & (u < hi)) != bool(invert)
    if keep_pixel is not None:
        out &= np.asarray(keep_pixel).reshape(-1)[p] != 0
    if keep_bin is not None:
        out &= np.asarray(keep_bin).reshape(-1)[k] != 0
    return out


def fold_of(k, p, P, n, seed=0, j=None):
    """The fold 0 .. n - 1 whose test range holds every reading's u24."""
    k, p = np.asarray(k, np.int64), np.asarray(p, np.int64)
    j = dr.occurrence(k, p, P) if j is None else np.asarray(j, np.int64)
    u = u24(k, p, j, seed)
    edges = np.array([fold_range(f, n)[0] for f in range(n)] + [RANGE], np.int64)
    return np.searchsorted(edges, u, side="right") - 1


_PROBLEMS = {}


def problem(name, nbins=2, max_repeat=1, rate=0.35):
    """A list of readings over SHAPES[name]: every cell is read with probability `rate`, a read
    cell 1 .. max_repeat times; the list is shuffled.  -> dict(k, p, c (int64, list order), K, I,
    J, P, b (bin boundaries), sigma)."""
    key = (name, nbins, max_repeat, rate)
    if key not in _PROBLEMS:
        K, I, J = SHAPES[name]
        P = I * J
        g = np.random.default_rng(1000 + 10 * sorted(SHAPES).index(name) + nbins + 100 * max_repeat)
        read = g.random((K, P)) < rate
        times = np.where(read, g.integers(1, max_repeat + 1, (K, P)), 0)
        k, p = np.nonzero(times)
        reps = times[k, p]
        k, p = np.repeat(k, reps), np.repeat(p, reps)
        order = g.permutation(k.size)
        k, p = k[order], p[order]
        c = g.integers(0, nbins, k.size)
        b = [0.0] + [float(v) for v in np.arange(1, nbins)] + [float(nbins) + 1.0]
        _PROBLEMS[key] = dict(k=k.astype(np.int64), p=p.astype(np.int64), c=c.astype(np.int64),
                              K=K, I=I, J=J, P=P, b=b, sigma=0.5, nbins=nbins)
    return _PROBLEMS[key]


def dense_of(d):
    """(Y, Wx) (K, P) of a problem without repeats."""
    Y = np.zeros((d["K"], d["P"]), np.int64)
    Wx = np.zeros((d["K"], d["P"]), bool)
    Y[d["k"], d["p"]] = d["c"]
    Wx[d["k"], d["p"]] = True
    return Y, Wx


def sorted_by_position(k, p, perm):
    """The indices that put a list into the exported order of a list packing: (position, k,
    occurrence) with position = the place of p in perm."""
    perm = np.asarray(perm, np.int64)
    pos_of = np.full(int(perm.max()) + 1, -1, np.int64)
    pos_of[perm[perm >= 0]] = np.flatnonzero(perm >= 0)
    key = pos_of[np.asarray(p, np.int64)] * (int(np.max(k)) + 1) + np.asarray(k, np.int64)
    return np.argsort(key, kind="stable")
