"""CPU reference (numpy, integer arithmetic and fp64) of the draw of readings from the model and of
the parametric bootstrap -- a helper for tests/test_draw_host.py and tests/test_gpu_draw.py, not a
test file.  Written from include/qsc.h (qsc_draw_codes / qsc_draw_readings); it imports nothing of
the package and reuses tests/info_ref.py's bin_probabilities and the Newton references
tests/cfit_ref.py / tests/sfit_ref.py.

One reading at bin k, pixel p, occurrence j (its place among the readings of its cell, in list
order), replicate rep:
    n = philox4x32_10(counter (k, p, j, rep), key (seed & 0xFFFFFFFF, seed >> 32))[0] >> 8
    u = (n + 1/2) 2^-24;  P_b at t = s_p . c_k;  Z = sum_b P_b
    code = the smallest b with u Z < P_0 + ... + P_b, else the last b with P_b > 0
    log model with t + offset <= 0: the reading keeps its code and is counted invalid
"""
import numpy as np

import cfit_ref as cf
import info_ref as ir
import sfit_ref as sr

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KAT_ZERO = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
# a drawn code may differ from an fp32 implementation's only where u Z lies this close to a
# cumulative sum: ten times the 1e-6 to which fp32 probabilities agree with fp64
WINDOW = 1e-5


BOOT = dict(I=32, J=32, K=64, R=2, sigma=0.4, rate=0.75, seed=77, n=16, draw_seed=5)
_BOOT = {}


def boot_problem():
    """The bootstrap tests' input: a 32 x 32 map, K = 64, R = 2, one-bit probit readings drawn at
    the true (S, C) (Y) and at twice the model's noise_std (Y2) over one 0.75 mask."""
    if not _BOOT:
        c = BOOT
        P = c["I"] * c["J"]
        g = np.random.default_rng(c["seed"])
        S = (0.2 + 0.8 * g.random((c["R"], P))).astype(np.float32).astype(np.float64)
        C = (0.1 + 0.9 * g.random((c["R"], c["K"]))).astype(np.float32).astype(np.float64)
        T = C.T @ S
        b = [0.0, float(np.float32(np.median(T))), float(np.float32(T.max() + 1.0))]
        z = g.standard_normal(T.shape)
        Y = (T + c["sigma"] * z > b[1]).astype(np.int64)
        Y2 = (T + 2.0 * c["sigma"] * z > b[1]).astype(np.int64)
        Wx = g.random(T.shape) < c["rate"]
        _BOOT.update(S=S, C=C, Y=Y, Y2=Y2, Wx=Wx, b=b, P=P,
                     model=(b, c["sigma"], 0.0, False, "probit"))
    return _BOOT


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of Philox4x32-10."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m32 = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # < 2^64: both factors hold 32 bits
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & m32
        hi1, lo1 = p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def key_of(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & MASK, s >> 32


def n24(k, p, j, replicate, seed):
    """The 24-bit integer of every reading's draw."""
    k0, k1 = key_of(seed)
    x0 = philox4x32_10(k, p, j, np.full(np.shape(k), int(replicate), np.uint64), k0, k1)[0]
    return (x0 >> np.uint64(8)).astype(np.int64)


def uniform(k, p, j, replicate, seed):
    """u = (n + 1/2) 2^-24 in fp64: 0 < u < 1 exactly."""
    return (n24(k, p, j, replicate, seed).astype(np.float64) + 0.5) * 2.0 ** -24


def occurrence(k, p, P):
    """j_occ of every reading: its index among the readings of its cell, in list order."""
    k, p = np.asarray(k, np.int64), np.asarray(p, np.int64)
    cell = k * int(P) + p
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    first = np.r_[True, sc[1:] != sc[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(sc)), 0))
    j = np.empty(len(sc), np.int64)
    j[order] = np.arange(len(sc)) - start
    return j


def draw(t, u, keep, b, sigma, offset=0.0, log_model=False, loss="probit"):
    """The drawn code of every reading at map value t (fp64), uniform u and present code keep.
    -> (code, invalid mask, margin, P_b (nbins, n)): margin = min_b |u Z - cum_b|, the distance of
    the threshold from the nearest cumulative sum (inf for an invalid reading)."""
    t, u = np.asarray(t, np.float64), np.asarray(u, np.float64)
    keep = np.asarray(keep, np.int64)
    inv = (t + offset <= 0) if log_model else np.zeros(t.shape, bool)
    Pb = ir.bin_probabilities(np.where(inv, 1.0, t), b, sigma, offset, log_model, loss)  # (nb, n)
    cum = np.cumsum(Pb, axis=0)
    thr = u * cum[-1]
    passed = thr[None, :] < cum
    first = np.argmax(passed, axis=0)
    nb = Pb.shape[0]
    last = nb - 1 - np.argmax((Pb > 0)[::-1], axis=0)
    code = np.where(passed.any(axis=0), first, last)
    code = np.where(inv | ~(Pb > 0).any(axis=0), keep, code)
    margin = np.where(inv, np.inf, np.min(np.abs(thr[None, :] - cum), axis=0))
    return code.astype(np.int64), inv, margin, Pb


def resample_readings(S, C, k, p, y, model, seed=0, replicate=0):
    """Drawn codes of the readings (k, p, y) (1-D; cells may repeat; j_occ by list order) from the
    model at S (R, P), C (R, K); model = (b, sigma, offset, log_model, loss).
    -> dict(code, invalid, margin, Pb, u, j)."""
    S, C = np.asarray(S, np.float64), np.asarray(C, np.float64)
    k, p = np.asarray(k, np.int64), np.asarray(p, np.int64)
    j = occurrence(k, p, S.shape[1])
    u = uniform(k, p, j, replicate, seed)
    t = np.einsum("rn,rn->n", S[:, p], C[:, k])
    code, inv, margin, Pb = draw(t, u, y, *model)
    return dict(code=code, invalid=inv, margin=margin, Pb=Pb, u=u, j=j)


def resample_dense(S, C, Y, Wx, model, seed=0, replicate=0):
    """(Y_new (K, P) with the unobserved cells left as they are, the readings dict) for dense
    Y, Wx (K, P)."""
    k, p = np.nonzero(np.asarray(Wx) != 0)
    r = resample_readings(S, C, k, p, np.asarray(Y)[k, p], model, seed, replicate)
    Yn = np.array(Y, np.int64)
    Yn[k, p] = r["code"]
    r["k"], r["p"] = k, p
    return Yn, r


def scale_gauge(S, C, norms):
    """|c_r|_2 = norms[r], s_r inversely (a zero c_r is left as it is)."""
    cur = np.linalg.norm(C, axis=1)
    a = np.where(cur > 0, norms / np.where(cur > 0, cur, 1.0), 1.0)
    return S / a[:, None], C * a[:, None]


def nll(S, C, Y, Wx, model):
    """-sum log max(P, FLT_MIN) over the observed cells, fp64."""
    b, sigma, offset, log_model, loss = model
    Pb = ir.bin_probabilities(C.T @ S, b, sigma, offset, log_model, loss)
    k, p = np.nonzero(np.asarray(Wx) != 0)
    Py = Pb[np.asarray(Y)[k, p], k, p]
    return float(-np.log(np.maximum(Py, np.finfo(np.float32).tiny)).sum())


def refit(S, C, Y, Wx, model, refit_=("C", "S"), rounds=1, ridge_s=0.0, ridge_c=0.0, max_steps=30,
          project_s=None, dtype=np.float64):
    """The bootstrap's recipe on dense data: `rounds` times cfit_ref.fit then sfit_ref.fit from
    (S, C).  -> (S, C, nll (fp64 at the result), dict of the per-bin / per-pixel `converged` masks
    of every fit)."""
    b, sigma, offset, log_model, loss = model
    S, C = np.array(S, dtype), np.array(C, dtype)
    steps = {}
    for r in range(rounds):
        if "C" in refit_:
            out = cf.fit(C, S, Y, Wx, b, sigma, offset, log_model, loss, ridge=ridge_c,
                         max_steps=max_steps, dtype=dtype)
            C, steps[("C", r)] = out["C"], out["converged"]
        if "S" in refit_:
            out = sr.fit(S, C, Y, Wx, b, sigma, offset, log_model, loss, ridge=ridge_s,
                         max_steps=max_steps, project=project_s, dtype=dtype)
            S, steps[("S", r)] = out["S"], out["converged"]
    return S, C, nll(S.astype(np.float64), C.astype(np.float64), Y, Wx, model), steps


def bootstrap(S, C, Y, Wx, model, n=32, seed=0, dtype=np.float64, codes=None, **recipe):
    """The bootstrap over the references.  codes: optional list of n drawn Y (K, P) to refit
    instead of the reference's own draws.  -> dict(std_S, std_C, mean_S, mean_C, nll (n,),
    nll_observed, p_fit, S (n, R, P), C (n, R, K), steps)."""
    S0, C0 = np.asarray(S, np.float64), np.asarray(C, np.float64)
    norms = np.linalg.norm(C0, axis=1)
    nll_obs = refit(S0, C0, Y, Wx, model, dtype=dtype, **recipe)[2]
    Ss, Cs, nlls, steps = [], [], [], []
    for rep in range(n):
        Yb = codes[rep] if codes is not None else resample_dense(S0, C0, Y, Wx, model, seed, rep)[0]
        Sb, Cb, f, st = refit(S0, C0, Yb, Wx, model, dtype=dtype, **recipe)
        Sb, Cb = scale_gauge(Sb.astype(np.float64), Cb.astype(np.float64), norms)
        Ss.append(Sb)
        Cs.append(Cb)
        nlls.append(f)
        steps.append(st)
    Ss, Cs, nlls = np.array(Ss), np.array(Cs), np.array(nlls)
    return dict(std_S=Ss.std(axis=0, ddof=1), std_C=Cs.std(axis=0, ddof=1), mean_S=Ss.mean(axis=0),
                mean_C=Cs.mean(axis=0), nll=nlls, nll_observed=nll_obs,
                p_fit=(1 + int((nlls >= nll_obs).sum())) / (n + 1), S=Ss, C=Cs, steps=steps)
