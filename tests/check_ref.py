"""CPU reference (numpy fp64) of the per-position goodness-of-fit and level-shift statistics -- a
helper for tests/test_check_host.py and tests/test_gpu_check.py, not a test file.  Written from
the formulas of include/qsc.h (qsc_scheck); it imports nothing of the package and reuses
tests/info_ref.py's bin_terms.

Per reading (k, p, y), t = s_p . c_k, x = t or log(t + offset) (+ delta), dxdt = 1 or 1 / (t + offset):
    l = -log max(P_y, FLT_MIN),  H = -sum_b P_b log P_b,  var = max(sum_b P_b log^2 P_b - H^2, 0)
    g_x = -P_y'/P_y (0 where P_y underflows),  h_x = sum_b P_b'^2 / P_b   (bins with P_b == 0 dropped)
Per position: D = sum (l - H), V = sum var, u = sum g_x, Ixx = sum h_x,
    g = sum g_x dxdt c_k + ridge s, v = sum h_x dxdt c_k, J = sum h_x dxdt^2 c_k c_k^T + ridge I,
    fitted: u* = u - v^T J^-1 g, I* = Ixx - v^T J^-1 v through J = L L^T, a = L^-1 v, b = L^-1 g.
Flags: 1 untestable (fitted: a pivot <= 0 or I* <= 1e-4 Ixx; u*, I* = 0), 2 invalid (log model,
t + offset <= 0: all four 0, bit 1 clear), 4 saturated (P_y below what fp32 holds).
"""
import numpy as np

import info_ref as ir

FLT_MIN = float(np.finfo(np.float32).tiny)
# the fp32 P of a code is 0 below about 2^-150; the tests keep P_y well away from this
SAT_P = 2.0 ** -150
GUARD = 1e-4
UNTESTABLE, INVALID, SATURATED = 1, 2, 4


def entry_terms(T, Y, b, sigma, offset=0.0, log_model=False, loss="probit", delta=0.0):
    """Per-entry terms in fp64 at the map values T and codes Y (same shape): a dict of dl = l - H,
    l, H, var, gx, hx, dxdt, sat, neg.  Entries with neg (t + offset <= 0) hold zeros."""
    T = np.asarray(T, np.float64)
    Y = np.asarray(Y).astype(np.int64)
    e = ir.edges_of(b, log_model)
    a = ir.link_scale(sigma, loss)
    nb = len(e) - 1
    neg = (T + offset <= 0) if log_model else np.zeros(T.shape, bool)
    tp = np.where(neg, 1.0, T + offset) if log_model else None
    x = (np.log(tp) if log_model else T) + delta
    dxdt = 1.0 / tp if log_model else np.ones_like(T)
    H = np.zeros_like(x)
    M2 = np.zeros_like(x)
    hx = np.zeros_like(x)
    Py = np.zeros_like(x)
    P1y = np.zeros_like(x)
    for c in range(nb):
        P, P1, _ = ir.bin_terms(x, e[c], e[c + 1], a, loss)
        on = P > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            lp = np.where(on, np.log(np.where(on, P, 1.0)), 0.0)
            H -= np.where(on, P * lp, 0.0)
            M2 += np.where(on, P * lp * lp, 0.0)
            hx += np.where(on, P1 * P1 / np.where(on, P, 1.0), 0.0)
        Py = np.where(Y == c, P, Py)
        P1y = np.where(Y == c, P1, P1y)
    sat = Py < SAT_P
    with np.errstate(divide="ignore", invalid="ignore"):
        gx = np.where(sat, 0.0, -P1y / np.where(sat, 1.0, Py))
    l = -np.log(np.maximum(Py, FLT_MIN))
    out = dict(dl=l - H, l=l, H=H, var=np.maximum(M2 - H * H, 0.0), gx=gx, hx=hx, dxdt=dxdt)
    for k in out:
        out[k] = np.where(neg, 0.0, out[k])
    out["sat"] = sat & ~neg
    out["neg"] = neg
    return out


def chol(A):
    """Cholesky of A by the pivot rule of qsc_info_std: (L, relative pivots piv_j / A_jj, bad);
    a pivot that is not positive is replaced by 1 and sets bad."""
    n = A.shape[0]
    L = np.zeros_like(A)
    rel = np.ones(n, np.float64)
    bad = False
    for j in range(n):
        piv = A[j, j] - np.dot(L[j, :j], L[j, :j])
        rel[j] = float(piv) / float(A[j, j]) if A[j, j] > 0 else 0.0
        if not piv > 0:
            bad = True
            piv = A.dtype.type(1.0)
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L, rel, bad


def forward(L, r):
    y = np.zeros_like(r)
    for i in range(L.shape[0]):
        y[i] = (r[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    return y


def stats(S, C, k, p, y, b, sigma, offset=0.0, log_model=False, loss="probit", fitted=True,
          ridge=0.0, dtype=np.float64, delta=0.0):
    """The statistics of every position from the readings (k, p, y) (1-D integer arrays; a cell may
    repeat), S (R, P), C (R, K).  -> dict of D, V, u, info (the four outputs, the zeroing rules
    applied), n, flags and, for the tests' exclusions, Ixx, Istar and ratio (I* and I* / Ixx before
    the rules; ratio is 1 where fitted is off, 0 where Ixx is 0) and minpiv (the smallest relative pivot of J; 1 without).
    dtype=np.float32: the rounding floor -- the map value from the fp32-rounded S and C in fp32,
    the per-entry terms evaluated in fp64 at it and rounded once, D and V summed in fp64 and the
    rest, the factorisation and the substitutions in fp32, as the kernel is specified."""
    f = np.dtype(dtype).type
    S = np.asarray(S, np.float64).astype(dtype)
    C = np.asarray(C, np.float64).astype(dtype)
    k, p, y = (np.asarray(v).astype(np.int64).reshape(-1) for v in (k, p, y))
    R, P = S.shape
    sp, ck = S[:, p], C[:, k]                      # (R, n)
    t = np.zeros(len(k), dtype)
    for r in range(R):
        t = t + sp[r] * ck[r]
    assert t.dtype == np.dtype(dtype)
    et = entry_terms(t, y, b, sigma, f(offset) if dtype == np.float32 else offset, log_model,
                     loss, delta)
    on = ~et["neg"]
    dl, var = et["dl"].astype(dtype), et["var"].astype(dtype)
    gx, hx, dx = et["gx"].astype(dtype), et["hx"].astype(dtype), et["dxdt"].astype(dtype)
    D, V = np.zeros(P), np.zeros(P)
    np.add.at(D, p, dl.astype(np.float64))
    np.add.at(V, p, var.astype(np.float64))
    u, Ixx = np.zeros(P, dtype), np.zeros(P, dtype)
    np.add.at(u, p, gx)
    np.add.at(Ixx, p, hx)
    n = np.bincount(p[on], minlength=P).astype(np.int64)
    inv = np.bincount(p[et["neg"]], minlength=P) > 0
    sat = np.bincount(p[et["sat"]], minlength=P) > 0
    us, Is = u.copy(), Ixx.copy()
    ratio, minpiv = np.ones(P), np.ones(P)
    untest = np.zeros(P, bool)
    if fitted:
        g = np.zeros((P, R), dtype)
        v = np.zeros((P, R), dtype)
        J = np.zeros((P, R, R), dtype)
        ge, hv = gx * dx, hx * dx
        hj = hv * dx
        np.add.at(g, p, (ge * ck).T)
        np.add.at(v, p, (hv * ck).T)
        np.add.at(J, p, np.einsum("n,rn,sn->nrs", hj, ck, ck))
        assert J.dtype == np.dtype(dtype)
        for q in range(P):
            A = J[q] + f(ridge) * np.eye(R, dtype=dtype)
            L, rel, bad = chol(A)
            a = forward(L, v[q])
            bb = forward(L, g[q] + f(ridge) * S[:, q])
            Is[q] = Ixx[q] - np.dot(a, a)
            us[q] = u[q] - np.dot(a, bb)
            minpiv[q] = rel.min()
            ratio[q] = float(Is[q]) / float(Ixx[q]) if Ixx[q] > 0 else 0.0
            untest[q] = bad or not Is[q] > f(GUARD) * Ixx[q]
    flags = (np.where(untest & ~inv, UNTESTABLE, 0) | np.where(inv, INVALID, 0)
             | np.where(sat, SATURATED, 0)).astype(np.int64)
    zs = untest | inv
    return dict(D=np.where(inv, 0.0, D), V=np.where(inv, 0.0, V),
                u=np.where(zs, 0.0, us.astype(np.float64)),
                info=np.where(zs, 0.0, Is.astype(np.float64)), n=n, flags=flags,
                Ixx=Ixx.astype(np.float64), Istar=Is.astype(np.float64), ratio=ratio,
                minpiv=minpiv)


def dense_readings(Y, Wx):
    """(k, p, y) of the observed cells of Y (K, P), Wx (K, P), in (k, p) order."""
    k, p = np.nonzero(np.asarray(Wx) != 0)
    return k, p, np.asarray(Y)[k, p]


def nll(S, C, k, p, y, b, sigma, offset=0.0, log_model=False, loss="probit", delta=0.0):
    """Per-position sum of l at x + delta (P,), fp64."""
    S, C = np.asarray(S, np.float64), np.asarray(C, np.float64)
    t = np.einsum("rn,rn->n", S[:, p], C[:, k])
    et = entry_terms(t, y, b, sigma, offset, log_model, loss, delta)
    out = np.zeros(S.shape[1])
    np.add.at(out, p, et["l"])
    return out


def zscores(st):
    """(z_fit, z_shift, shift) of a stats dict by check_fit's rule: 0 where the variance is 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        zf = np.where(st["V"] > 0, st["D"] / np.sqrt(st["V"]), 0.0)
        zs = np.where(st["info"] > 0, -st["u"] / np.sqrt(st["info"]), 0.0)
        sh = np.where(st["info"] > 0, -st["u"] / st["info"], 0.0)
    return zf, zs, sh


def flagged(z, testable, alpha):
    """Two-sided Bonferroni mask and the critical value: |z| > -ndtri(alpha / (2 m))."""
    from scipy.special import ndtri
    m = int(np.sum(testable))
    if m == 0:
        return np.zeros(z.shape, bool), np.inf
    crit = -ndtri(alpha / (2.0 * m))
    return testable & (np.abs(z) > crit), crit


def max_err(got, ref, keep):
    """max|got - ref| / max|ref| over the positions keep."""
    got, ref = np.asarray(got, np.float64)[keep], np.asarray(ref, np.float64)[keep]
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
