"""CPU reference (numpy fp64) of the expected information gain of planned readings -- a helper
for tests/test_design_host.py and tests/test_gpu_design.py, not a test file.  Written from the
definitions of include/qsc.h (qsc_sgain) on top of tests/info_ref.py; it imports nothing of the
package.

    t_kp = S[:, p] . c_k,   A_p = sum_k w_k h_exp(t_kp) c_k c_k^T   (h_exp: info_ref's expected kind;
                                                                     log model: 0 where t + offset <= 0)
    M0 = J_p + ridge I,  M1 = M0 + A_p
    D: 1/2 (logdet M1 - logdet M0)    A: tr(M0^-1) - tr(M1^-1)    V: tr(G M0^-1) - tr(G M1^-1), G = C C^T
    M0 not positive definite, M1 positive definite: +inf (a first look);  M1 not: 0 (degenerate)
"""
import numpy as np

import info_ref as ir

CRITERIA = ("D", "A", "V")


def expected_information(S, C, b, sigma, offset=0.0, log_model=False, loss="probit"):
    """h_exp (K, P) in fp64 at the map C^T S: the Fisher information of one reading of every
    entry; under the log model 0 where t + offset <= 0."""
    T = np.asarray(C, np.float64).T @ np.asarray(S, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = ir.curvature(T, np.zeros(T.shape, np.int64), b, sigma, offset, log_model, loss,
                         "expected")
    if log_model:
        h = np.where(T + offset > 0.0, h, 0.0)
    return h


def plan_blocks(S, C, w, b, sigma, offset=0.0, log_model=False, loss="probit"):
    """A (P, R, R) in fp64 of the plan w (K,) (None: ones)."""
    C = np.asarray(C, np.float64)
    w = np.ones(C.shape[1]) if w is None else np.asarray(w, np.float64)
    h = expected_information(S, C, b, sigma, offset, log_model, loss)
    return np.einsum("k,kp,rk,sk->prs", w, h, C, C)


def pivots(M):
    """The Cholesky pivots of the symmetric M (fp64), in order; the factorisation stops at the
    first pivot that is not positive (the rest are returned as that pivot)."""
    n = M.shape[0]
    L = np.zeros_like(M)
    piv = np.empty(n)
    for j in range(n):
        pj = M[j, j] - L[j, :j] @ L[j, :j]
        piv[j] = pj
        if not pj > 0.0:
            piv[j:] = pj
            break
        L[j, j] = np.sqrt(pj)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return piv


def rel_pivot(M):
    """The smallest Cholesky pivot of M relative to its largest diagonal entry (<= 0: M is not
    positive definite; an all-zero M gives 0)."""
    d = float(np.max(np.diag(M)))
    p = float(np.min(pivots(M)))
    return p / d if d > 0.0 else min(p, 0.0)


def _figure(M, G, criterion):
    if criterion == "D":
        sign, ld = np.linalg.slogdet(M)
        assert sign > 0
        return 0.5 * ld
    Mi = np.linalg.inv(M)
    return -float(np.trace(Mi)) if criterion == "A" else -float(np.trace(G @ Mi))


def gains(J, A, C, ridge, criterion):
    """(gain (P,), first (P,) bool, bad (P,) bool, piv0 (P,), piv1 (P,)) in fp64 from the blocks
    J (P, R, R) and the plan's A (P, R, R); piv0 / piv1 the relative smallest pivots of M0 / M1."""
    assert criterion in CRITERIA
    J = np.asarray(J, np.float64)
    A = np.asarray(A, np.float64)
    C = np.asarray(C, np.float64)
    P, R, _ = J.shape
    G = C @ C.T
    gain = np.zeros(P)
    first = np.zeros(P, bool)
    bad = np.zeros(P, bool)
    piv0 = np.empty(P)
    piv1 = np.empty(P)
    for p in range(P):
        M0 = J[p] + ridge * np.eye(R)
        M1 = M0 + A[p]
        piv0[p], piv1[p] = rel_pivot(M0), rel_pivot(M1)
        if not piv1[p] > 0.0:
            bad[p] = True
        elif not piv0[p] > 0.0:
            first[p] = True
            gain[p] = np.inf
        else:
            gain[p] = _figure(M1, G, criterion) - _figure(M0, G, criterion)
    return gain, first, bad, piv0, piv1


def gains_fp32(J, S, C, w, ridge, criterion, b, sigma, offset=0.0, log_model=False,
               loss="probit", keep=None):
    """The same figures from an fp32 numpy evaluation of the same formulas -- fp32 map, plan
    block, sums, Cholesky and inverse factor -- from the fp32-rounded J, S and C (every M0 and
    M1 of the pixels `keep`, default all, must be positive definite; the others get NaN): the
    rounding floor an fp32 implementation is measured against.
    (The link terms of h_exp are evaluated in fp64 at the fp32 map value and rounded once.)"""
    J32 = np.asarray(J, np.float64).astype(np.float32)
    S32 = np.asarray(S, np.float64).astype(np.float32)
    C32 = np.asarray(C, np.float64).astype(np.float32)
    K = C32.shape[1]
    w32 = np.ones(K, np.float32) if w is None else np.asarray(w, np.float64).astype(np.float32)
    T32 = C32.T @ S32
    assert T32.dtype == np.float32
    h = ir.curvature(T32, np.zeros(T32.shape, np.int64), b, sigma, offset, log_model, loss,
                     "expected")
    if log_model:
        h = np.where(T32 + np.float32(offset) > 0.0, h, 0.0)
    wh = w32[:, None] * h.astype(np.float32)
    A32 = np.einsum("kp,rk,sk->prs", wh, C32, C32)
    assert A32.dtype == np.float32
    P, R, _ = J32.shape
    G32 = C32 @ C32.T
    eye = np.eye(R, dtype=np.float32)
    out = np.full(P, np.nan, np.float32)
    keep = np.ones(P, bool) if keep is None else np.asarray(keep, bool)

    def figure(M):
        L = np.linalg.cholesky(M)
        assert L.dtype == np.float32
        if criterion == "D":
            return np.sum(np.log(np.diag(L)), dtype=np.float32)
        Li = np.linalg.inv(L)
        if criterion == "A":
            return -np.sum(Li * Li, dtype=np.float32)
        return -np.sum((Li @ G32) * Li, dtype=np.float32)

    for p in np.nonzero(keep)[0]:
        M0 = J32[p] + np.float32(ridge) * eye
        M1 = M0 + A32[p]
        out[p] = figure(M1) - figure(M0)
    return out


def entry_gain(J, S, C, w, ridge, b, sigma, offset=0.0, log_model=False, loss="probit"):
    """1/2 log1p(w_k h_exp(t_kp) c_k^T (J_p + ridge I)^-1 c_k) (K, P) in fp64; +inf where the block
    is not positive definite."""
    C = np.asarray(C, np.float64)
    wv = np.ones(C.shape[1]) if w is None else np.asarray(w, np.float64)
    h = expected_information(S, C, b, sigma, offset, log_model, loss)
    _, std_T, _ = ir.stds(J, C, ridge)
    with np.errstate(invalid="ignore"):
        eg = 0.5 * np.log1p(wv[:, None] * h * std_T * std_T)
    return np.where(np.isinf(std_T), np.inf, eg)


def order(gain):
    """Pixel indices by descending gain, +inf first, equal gains in pixel order."""
    return np.argsort(-np.asarray(gain, np.float64), kind="stable")
