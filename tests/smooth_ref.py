"""CPU reference of the spatial smoothness prior on the loss fields -- a helper for
tests/test_smooth_host.py and tests/test_gpu_smooth.py, not a test file.

    R(S) = sum_r sum_{4-neighbour edges {p,p'}} rho(S_r(p) - S_r(p'))     (each edge once)
    quad:  rho(d) = d^2 / 2          huber:  rho(d) = d^2 / (2 delta) if |d| <= delta else |d| - delta/2
written as plain sums over S[:, :, 1:] - S[:, :, :-1] and the row analogue (torch, fp64 by
default), with its autograd gradient; a host neighbour table built from a pixel order `perm`; and
free_s_solve_smooth, the loop of oracle/solver.free_s_solve with + smooth * R(S) in both costs.
"""
import numpy as np
import torch

import logit_ref
from oracle import explicit
from oracle import reference_ops as ro


# ---------------------------------------------------------------------------------------
# penalty
# ---------------------------------------------------------------------------------------
def _rho(d, kind, delta):
    if kind == "quad":
        return 0.5 * d * d
    if kind == "huber":
        a = d.abs()
        return torch.where(a <= delta, d * d / (2.0 * delta), a - 0.5 * delta)
    raise ValueError(kind)


def penalty_t(S, kind="quad", delta=None):
    """R(S) as a 0-dim torch tensor of S's dtype; S (R,1,I,J) or (R,I,J), differentiable."""
    X = S.reshape(S.shape[0], S.shape[-2], S.shape[-1])
    dh = X[:, :, 1:] - X[:, :, :-1]
    dv = X[:, 1:, :] - X[:, :-1, :]
    return _rho(dh, kind, delta).sum() + _rho(dv, kind, delta).sum()


def penalty(S, kind="quad", delta=None):
    """(value, grad) in fp64: the autograd gradient of penalty_t, shaped like S (numpy)."""
    X = torch.as_tensor(np.asarray(S), dtype=torch.float64).clone().requires_grad_(True)
    v = penalty_t(X, kind, delta)
    v.backward()
    return float(v.item()), X.grad.numpy()


# ---------------------------------------------------------------------------------------
# neighbour table
# ---------------------------------------------------------------------------------------
def neighbor_table(perm, I, J):
    """(Pp, 4) int32: positions of the left, right, upper, lower neighbour of position q's pixel
    p = perm[q] = i*J + j; -1 outside the grid and for padding positions (perm[q] == -1)."""
    perm = np.asarray(perm).astype(np.int64)
    Pp, P = perm.shape[0], I * J
    iperm = np.full(P, -1, np.int64)
    valid = perm >= 0
    iperm[perm[valid]] = np.nonzero(valid)[0]
    nbr = np.full((Pp, 4), -1, np.int32)
    for q in range(Pp):
        p = perm[q]
        if p < 0:
            continue
        i, j = divmod(int(p), J)
        if j > 0:
            nbr[q, 0] = iperm[p - 1]
        if j + 1 < J:
            nbr[q, 1] = iperm[p + 1]
        if i > 0:
            nbr[q, 2] = iperm[p - J]
        if i + 1 < I:
            nbr[q, 3] = iperm[p + J]
    return nbr


# ---------------------------------------------------------------------------------------
# solver
# ---------------------------------------------------------------------------------------
def _data_term(Y, Wx, b, sigma, offset, log_model, loss, dtype):
    """-sum(Wx log P(Y | T_hat(S, C))) as a function of (S, C).  fp32: the oracle's own
    reference-formulation functions (reference_ops.masked_nll, logit_ref.masked_nll); fp64: the
    same expressions (explicit.edges_of's edges, the reference's 1.414213) in float64."""
    if dtype == torch.float32:
        if loss == "logit":
            return lambda S, C: logit_ref.masked_nll(S, C, Y, Wx, b, sigma, offset, log_model)
        return lambda S, C: ro.masked_nll(S, C, Y, Wx, b, sigma, offset, log_model)
    e = torch.tensor(explicit.edges_of(np.asarray(b, np.float64), log_model))
    Yl = Y.reshape(Y.shape[0], -1).long()
    W = Wx.reshape(Yl.shape).double()
    lo, hi = e[Yl], e[Yl + 1]

    def F(y):
        if loss == "logit":
            return torch.sigmoid(y / sigma)
        return 0.5 * (1 + torch.erf(y / (sigma * ro.SQRT2_REF)))

    def term(S, C):
        T = C.t() @ S.reshape(S.shape[0], -1)  # (K, P)
        x = torch.log(T + offset) if log_model else T
        P = F(hi - x) - F(lo - x)
        # (unobserved entries are excluded before the log, so a saturated P there is harmless)
        return -torch.sum(torch.log(torch.where(W != 0, P, torch.ones_like(P))))

    return term


def free_s_solve_smooth(S0, C0, Y, Wx, b, sigma, offset=0.0, log_model=False, n_iter=6,
                        lambda_c=100.0, lambda_s=100.0, lr_c=5e-3, lr_s=1e-2, loss="probit",
                        project_s=False, smooth=0.0, kind="quad", delta=None,
                        dtype=torch.float64):
    """oracle/solver.free_s_solve's loop (qmc/qmc.ipynb :559-634, free S; torch autograd and
    torch.optim.Adam, C[C<0] = 0, optional S[S<0] = 0) with + smooth * R(S) in the cost of both
    steps.  dtype float64: the reference; float32: its fp32 restatement on the oracle's own
    functions.  Returns dict(S, C, costs_c, costs_s, clipped) -- clipped: how many S entries the
    projection zeroed over the run."""
    data = _data_term(Y, Wx, b, sigma, offset, log_model, loss, dtype)
    S = S0.detach().to(dtype).clone().requires_grad_(True)
    C = C0.detach().to(dtype).clone().requires_grad_(True)
    optC = torch.optim.Adam([C], lr=lr_c)
    optS = torch.optim.Adam([S], lr=lr_s)
    costs_c, costs_s, clipped = [], [], 0
    for _ in range(n_iter):
        Sc = S.detach().clone()
        optC.zero_grad()
        cost = (data(Sc, C) + lambda_c * torch.norm(C, "fro") + lambda_s * torch.norm(Sc, "fro")
                + smooth * penalty_t(Sc, kind, delta))
        cost.backward()
        optC.step()
        with torch.no_grad():
            C[C < 0] = 0
        costs_c.append(cost.item())
        optS.zero_grad()
        cost = (data(S, C) + lambda_c * torch.norm(C, "fro") + lambda_s * torch.norm(S, "fro")
                + smooth * penalty_t(S, kind, delta))
        cost.backward()
        optS.step()
        if project_s:
            with torch.no_grad():
                clipped += int((S < 0).sum())
                S[S < 0] = 0
        costs_s.append(cost.item())
    return dict(S=S.detach(), C=C.detach(), costs_c=costs_c, costs_s=costs_s, clipped=clipped)
