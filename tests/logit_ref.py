"""CPU restatement of the logistic (ordered-logit) observation model -- a helper for
tests/test_logit_host.py and tests/test_gpu_logit.py, not a test file.

Reference formulation (torch CPU, fp32): the op sequence of oracle/reference_ops.prob_probit and
masked_nll with the reference's F_sigmoid (qmc/quantization_model.py:43-47, 1/(1+exp(-y))) in
place of F_probit, applied to (edge - X) / s:
    P = F((b[Y+1] - X)/s) - F((b[Y] - X)/s)          linear model: b[0] = -1e5, b[-1] = 1e5
This is what tools/make_golden_logit.py ran on the reference's own functions.

Explicit formulation (numpy fp64): the closed forms the HIP passes implement,
    u = (b[y+1] - x)/s, w = (b[y] - x)/s, F = logistic CDF, f = F (1 - F)
    P = F(u) - F(w);  nll = -sum log P;  g = (f(u) - f(w)) / (s P) * (1/(t + offset) if log)
evaluated without cancellation (the pair (u, w) is mirrored into the lower half first), so they
stay exact far into the tails.
"""
import numpy as np
import torch

from oracle import explicit
from oracle import reference_ops as ro


# ---------------------------------------------------------------------------------------
# reference formulation (torch, fp32, autograd)
# ---------------------------------------------------------------------------------------
def F_sigmoid(y):
    return 1 / (1 + torch.exp(-y))


def F_logit(y, s):
    return F_sigmoid(y / s)


def guarded(z):
    """F_sigmoid(z) with the same values; where exp(-z) overflows (the linear model's -1e5 clamp
    edge, F == 0 exactly) plain autograd forms 0 * inf = nan, so that constant term is evaluated
    detached (tools/make_golden_logit.py does the same on the reference's function)."""
    sat = torch.isinf(torch.exp(-z.detach()))
    return torch.where(sat, F_sigmoid(z.detach()),
                       F_sigmoid(torch.where(sat, torch.zeros_like(z), z)))


def prob_logit(Y, X_hat, b, s, log_model=False):
    edges = torch.as_tensor(b, dtype=torch.float32).clone()
    if not log_model:
        edges[0] = -100000
        edges[-1] = 100000
    lo, hi = edges[Y], edges[Y + 1]
    return guarded((hi - X_hat) / s) - guarded((lo - X_hat) / s)


def masked_nll(S, C, Y, Wx, b, s, offset=0.0, log_model=False):
    """-sum(Wx * log(prob_logit(Y, T_hat, b, s))) with T_hat = get_tensor(S, C)."""
    T_hat = ro.get_tensor(S, C).unsqueeze(1)
    if log_model:
        T_hat = torch.log(T_hat + offset)
    return -torch.sum(Wx * torch.log(prob_logit(Y, T_hat, b, s, log_model)))


def free_s_solve(S0, C0, Y, Wx, b, s, offset=0.0, log_model=False, n_iter=10, lambda_c=100.0,
                 lambda_s=100.0, lr_c=5e-3, lr_s=1e-2, snapshots=()):
    """oracle/solver.free_s_solve's loop (qmc/qmc.ipynb :559-634, free S) on the logistic NLL."""
    S = S0.clone().requires_grad_(True)
    C = C0.clone().requires_grad_(True)
    optC = torch.optim.Adam([C], lr=lr_c)
    optS = torch.optim.Adam([S], lr=lr_s)
    costs_c, costs_s, snaps = [], [], {}
    for i in range(n_iter):
        Sc = S.detach().clone()
        optC.zero_grad()
        nll = masked_nll(Sc, C, Y, Wx, b, s, offset, log_model)
        cost = nll + lambda_c * torch.norm(C, "fro") + lambda_s * torch.norm(Sc, "fro")
        cost.backward()
        optC.step()
        with torch.no_grad():
            C[C < 0] = 0
        costs_c.append(cost.item())
        optS.zero_grad()
        nll = masked_nll(S, C, Y, Wx, b, s, offset, log_model)
        cost = nll + lambda_c * torch.norm(C, "fro") + lambda_s * torch.norm(S, "fro")
        cost.backward()
        optS.step()
        costs_s.append(cost.item())
        if i + 1 in snapshots:
            snaps[i + 1] = (S.detach().clone(), C.detach().clone())
    return dict(S=S.detach(), C=C.detach(), costs_c=costs_c, costs_s=costs_s, snaps=snaps)


# ---------------------------------------------------------------------------------------
# explicit formulation (numpy, fp64)
# ---------------------------------------------------------------------------------------
def _Ff(z):
    """F(z) and f(z) = F (1 - F) from exp(-|z|) only (full relative precision in both tails)."""
    e = np.exp(-np.abs(z))
    r = 1.0 / (1.0 + e)
    return np.where(z < 0, e * r, r), e * r * r


def prob_grad(x, lo, hi, s):
    """P = F((hi-x)/s) - F((lo-x)/s) and gx = d(-log P)/dx, fp64, cancellation-free."""
    u = (hi - x) / s
    w = (lo - x) / s
    mir = (u + w) > 0
    uu = np.where(mir, -w, u)
    ww = np.where(mir, -u, w)
    Fu, fu = _Ff(uu)
    Fw, fw = _Ff(ww)
    P = Fu - Fw
    with np.errstate(divide="ignore", invalid="ignore"):
        gx = np.where(mir, -1.0, 1.0) * (fu - fw) / (s * P)
    return P, gx


def nll_grad(S, C, Y, Wx, b, s, offset=0.0, log_model=False):
    """S (R,P), C (R,K), Y (K,P) int, Wx (K,P) 0/1 -> (nll, dS (R,P), dC (R,K)) in fp64."""
    S = np.asarray(S, np.float64)
    C = np.asarray(C, np.float64)
    Y = np.asarray(Y).astype(np.int64)
    Wx = np.asarray(Wx, np.float64)
    e = explicit.edges_of(b, log_model)
    T = C.T @ S  # (K, P)
    x = np.log(T + offset) if log_model else T
    P, gx = prob_grad(x, e[Y], e[Y + 1], float(s))
    obs = Wx != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        nll = -np.sum(np.log(P[obs]))
    g = np.where(obs, gx * (1.0 / (T + offset) if log_model else 1.0), 0.0)
    return nll, C @ g, S @ g.T


def explicit_solve(S0, C0, Y, Wx, b, s, offset=0.0, log_model=False, n_iter=3, lambda_c=100.0,
                   lambda_s=100.0, lr_c=5e-3, lr_s=1e-2):
    """oracle/explicit.explicit_solve's loop (closed-form fp64 gradients, explicit.adam_step) on
    the logistic NLL.  S0 (R,P), C0 (R,K), Y / Wx (K,P).  Returns (S, C, costs_c, costs_s)."""
    S = np.asarray(S0, np.float64).copy()
    C = np.asarray(C0, np.float64).copy()
    mS, vS, mC, vC = (np.zeros_like(S), np.zeros_like(S), np.zeros_like(C), np.zeros_like(C))
    costs_c, costs_s = [], []

    def reg(X, lam):
        n = float(np.linalg.norm(X))
        return lam * n, (lam * X / n if n > 0 else np.zeros_like(X))

    for it in range(1, n_iter + 1):
        nll, _, dC = nll_grad(S, C, Y, Wx, b, s, offset, log_model)
        rc, gc = reg(C, lambda_c)
        rs, _ = reg(S, lambda_s)
        costs_c.append(nll + rc + rs)
        C, mC, vC = explicit.adam_step(C, mC, vC, dC + gc, it, lr_c)
        C = np.maximum(C, 0.0)
        nll, dS, _ = nll_grad(S, C, Y, Wx, b, s, offset, log_model)
        rc, _ = reg(C, lambda_c)
        rs, gs = reg(S, lambda_s)
        costs_s.append(nll + rc + rs)
        S, mS, vS = explicit.adam_step(S, mS, vS, dS + gs, it, lr_s)
    return S, C, costs_c, costs_s
