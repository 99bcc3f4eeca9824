"""CPU reference (numpy fp64) of the per-pixel Fisher information -- a helper for
tests/test_info_host.py and tests/test_gpu_info.py, not a test file.  Written from the formulas
of include/qsc.h (qsc_sinfo); it imports nothing of the package.

Per entry, in the model domain x (x = t, or log(t + offset)), phi = F':
    P = F(hi - x) - F(lo - x),  P' = -(phi(hi - x) - phi(lo - x)),  P'' = phi'(hi - x) - phi'(lo - x)
    g_x = -P'/P;   observed h_x = (P'/P)^2 - P''/P;   expected h_x = sum_b (P_b')^2 / P_b
    probit: a = fp32(sigma * 1.414213), phi(y) = exp(-(y/a)^2) / (a sqrt(pi)), phi' = -2 (y/a) phi / a
    logit:  phi = F (1 - F) / s, phi' = phi (1 - 2F) / s
    linear: h = h_x;  log model: observed h = (h_x - g_x) / (t + offset)^2, expected h_x / (t + offset)^2
Blocks J_p = sum_{k observed at p} h(k, p) c_k c_k^T; std_S = sqrt(diag((J_p + ridge I)^-1));
std_T[k, p] = sqrt(c_k^T (J_p + ridge I)^-1 c_k); a block that is not positive definite gives +inf.
"""
import math

import numpy as np
from scipy.special import erfc


def edges_of(b, log_model):
    """prob_probit's edges: the linear model clamps b[0], b[-1] to -/+1e5, the log model does not."""
    e = np.asarray(b, dtype=np.float64).copy()
    if not log_model:
        e[0], e[-1] = -1e5, 1e5
    return e


def link_scale(sigma, loss, exact=False):
    """The divisor of the link: fp32(sigma * 1.414213) (probit) or sigma (logit).  exact=True
    keeps sigma * 1.414213 in fp64 (the oracle NLL's own constant)."""
    if loss == "logit":
        return float(sigma)
    a = float(sigma) * 1.414213
    return a if exact else float(np.float32(a))


def _edge_terms(y, a, loss):
    """F, phi, phi' at y = edge - x (arrays); a saturated or infinite edge gives phi = phi' = 0."""
    fin = np.isfinite(y)
    z = np.where(fin, y, 0.0) / a
    if loss == "logit":
        e = np.exp(-np.abs(z))
        r = 1.0 / (1.0 + e)
        F = np.where(z < 0, e * r, r)
        f = e * r * r
        phi = f / a
        dphi = phi * np.where(z < 0, 1.0, -1.0) * (1.0 - e) * r / a  # phi (1 - 2F) / s
    else:
        F = 0.5 * erfc(-z)
        phi = np.exp(-z * z) / (a * math.sqrt(math.pi))
        dphi = -2.0 * z * phi / a
    F = np.where(fin, F, np.where(y > 0, 1.0, 0.0))
    return F, np.where(fin, phi, 0.0), np.where(fin, dphi, 0.0)


def bin_terms(x, lo, hi, a, loss):
    """(P, P', P'') of the bin (lo, hi) at x."""
    Fu, pu, du = _edge_terms(hi - x, a, loss)
    Fw, pw, dw = _edge_terms(lo - x, a, loss)
    # the difference of the two lower tails where both are past the median (no cancellation)
    Fu_c, _, _ = _edge_terms(-(hi - x), a, loss)
    Fw_c, _, _ = _edge_terms(-(lo - x), a, loss)
    P = np.where((hi - x) + (lo - x) > 0, Fw_c - Fu_c, Fu - Fw)
    return P, -(pu - pw), du - dw


def curvature(T, Y, b, sigma, offset=0.0, log_model=False, loss="probit", kind="expected",
              exact_scale=False):
    """h (K, P) in fp64: the curvature of every entry's -log P in the map value T[k, p]."""
    T = np.asarray(T, np.float64)
    Y = np.asarray(Y).astype(np.int64)
    e = edges_of(b, log_model)
    a = link_scale(sigma, loss, exact_scale)
    tp = T + offset if log_model else None
    x = np.log(tp) if log_model else T
    if kind == "observed":
        P, P1, P2 = bin_terms(x, e[Y], e[Y + 1], a, loss)
        gx = -P1 / P
        h = gx * gx - P2 / P
        if log_model:
            h = h - gx
    elif kind == "expected":
        h = np.zeros_like(x)
        for c in range(len(e) - 1):
            P, P1, _ = bin_terms(x, e[c], e[c + 1], a, loss)
            with np.errstate(divide="ignore", invalid="ignore"):
                h += np.where(P > 0, P1 * P1 / P, 0.0)
    else:
        raise ValueError(kind)
    return h / (tp * tp) if log_model else h


def bin_probabilities(T, b, sigma, offset=0.0, log_model=False, loss="probit"):
    """P_b (nbins, K, P) of every bin at every entry."""
    T = np.asarray(T, np.float64)
    e = edges_of(b, log_model)
    a = link_scale(sigma, loss)
    x = np.log(T + offset) if log_model else T
    return np.stack([bin_terms(x, e[c], e[c + 1], a, loss)[0] for c in range(len(e) - 1)])


def blocks(S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", kind="expected",
           exact_scale=False):
    """J (P, R, R) in fp64 from dense S (R, P), C (R, K), Y (K, P), Wx (K, P)."""
    S = np.asarray(S, np.float64)
    C = np.asarray(C, np.float64)
    W = (np.asarray(Wx, np.float64) != 0).astype(np.float64)
    h = curvature(C.T @ S, Y, b, sigma, offset, log_model, loss, kind, exact_scale)
    return np.einsum("kp,rk,sk->prs", W * h, C, C)


def stds(J, C, ridge, map_std=True):
    """(std_S (R, P), std_T (K, P) or None, unidentified) in fp64; a block J_p + ridge I that is
    not positive definite gives +inf and is counted."""
    J = np.asarray(J, np.float64)
    C = np.asarray(C, np.float64)
    P, R, _ = J.shape
    K = C.shape[1]
    std_S = np.full((R, P), np.inf)
    std_T = np.full((K, P), np.inf) if map_std else None
    bad = 0
    for p in range(P):
        A = J[p] + ridge * np.eye(R)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            bad += 1
            continue
        M = np.linalg.solve(L, np.eye(R))  # L^-1
        std_S[:, p] = np.sqrt((M * M).sum(axis=0))
        if map_std:
            std_T[:, p] = np.sqrt(((M @ C) ** 2).sum(axis=0))
    return std_S, std_T, bad


def stds_fp32(J, C, ridge):
    """The same figures from an fp32 numpy Cholesky inverse of the fp32-rounded blocks (every
    block must be positive definite): the rounding floor an fp32 implementation is measured
    against."""
    J32 = np.asarray(J, np.float64).astype(np.float32)
    C32 = np.asarray(C, np.float64).astype(np.float32)
    P, R, _ = J32.shape
    std_S = np.empty((R, P), np.float32)
    std_T = np.empty((C32.shape[1], P), np.float32)
    eye = np.eye(R, dtype=np.float32)
    for p in range(P):
        L = np.linalg.cholesky(J32[p] + np.float32(ridge) * eye)
        M = np.linalg.inv(L)
        assert M.dtype == np.float32
        std_S[:, p] = np.sqrt((M * M).sum(axis=0))
        std_T[:, p] = np.sqrt(((M @ C32) ** 2).sum(axis=0))
    return std_S, std_T


def max_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))
