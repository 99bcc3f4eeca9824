"""CPU reference (numpy, fp64 or fp32) of the per-pixel damped Newton fit of S for known C
(include/qsc.h: qsc_sfit) -- a helper for tests/test_sfit_host.py and tests/test_gpu_sfit.py, not
a test file.  Written from the header's statement of the iteration; it imports nothing of the
package.  The link terms come from tests/info_ref.py (bin_terms), evaluated in the chosen dtype.

Per position p, s = S[:, p], entries k with Wx[k, p] != 0, t = s . c_k, x = t or log(t + offset):
    f = sum -log max(P, FLT_MIN) + ridge / 2 |s|^2
    g = sum g_t c_k,       g_t = -P'/P (linear) or -P'/P / (t + offset) (log model)
    J = sum h c_k c_k^T,   h of info_ref.curvature (observed / expected)
An entry with P == 0 adds 0 to g and J; t + offset <= 0 makes f = +inf.  The iteration:
    evaluate at S_init, mu = mu0; up to max_steps times: Cholesky of J + (ridge + mu) I, delta from
    g + ridge s, s' = s - delta (projected onto s' >= 0 if project); a pivot <= 0 rejects the step;
    accept iff f' <= f and finite (mu <- max(mu / 10, 0 if mu0 == 0 else MU_MIN)), else
    mu <- max(10 mu, MU_MIN); converged once an accepted step has
    |s' - s|_inf <= tol (1 + |s|_inf).  A position is identified once a factorisation has every
    pivot > mu (J + ridge I itself then has positive pivots).

Also the inputs of the GPU cases (`problem`), so that the CPU test can check that this reference
converges on exactly those inputs.
"""
import numpy as np
import torch

import info_ref as ir
from oracle import reference_ops as ro

MU_MIN = 1e-6
FLT_MIN = float(np.finfo(np.float32).tiny)

I, J, TILE = 9, 15, 64
P = I * J
RATE = 0.7
RIDGES = (1e-2, 1.0)

# name: (R, K, model, threshold, sigma, loss, seed) -- the five layouts / models of
# tests/test_gpu_info.py: one-bit signed rows, 4-bin code field, wide 16-bin, log model, logit
CASES = {
    "onebit16": (16, 70, "onebit", 3.5, 0.8, "probit", 13),
    "bins4": (8, 37, "bins4", None, 0.6, "probit", 12),
    "bins16": (3, 37, "bins16", None, 0.3, "probit", 17),
    "log8": (3, 70, "log8", None, 0.2, "probit", 14),
    "logit": (3, 37, "onebit", 0.9, 0.4, "logit", 15),
}
# (Chosen on the CPU so that this reference, in fp32 and in fp64, converges every observed pixel
# within 30 steps from the default start (tests/test_sfit_host.py): the log model with 8 bins and
# sigma 0.2 at R = 3, K = 70 -- with 4 bins or more noise the minimiser sits on the bound s = 0,
# where the clipped Newton step stalls -- and the logistic link at R = 3, where the walk through
# its tail from S = 0 takes fewer steps than at R = 16.)

_PROB = {}


def problem(name):
    """Inputs of a case (CPU tensors), built once: S_true ~ U(0.2, 1), C ~ U(0.1, 1), Y drawn from
    the model, sampling rate 0.7, pixel 0 unobserved (as tests/test_gpu_info.py's)."""
    if name in _PROB:
        return _PROB[name]
    R, K, model, thr, sigma, loss, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    S = 0.2 + 0.8 * torch.rand(R, 1, I, J, generator=g)
    C = 0.1 + 0.9 * torch.rand(R, K, generator=g)
    T = ro.get_tensor(S, C)
    if loss == "logit":
        u = torch.rand(T.shape, generator=g)
        noise = torch.log(u) - torch.log1p(-u)
    else:
        noise = torch.randn(T.shape, generator=g)
    offset, log_model = 0.0, False
    if model == "onebit":
        b = torch.tensor([0.0, thr, float(T.max()) + 1.0])
    elif model in ("bins16", "bins4"):
        b = torch.quantile(T.reshape(-1), torch.linspace(0, 1, 17 if model == "bins16" else 5))
    else:
        # the log model: NB bins with the inner edges at the quantiles of log(T + offset)
        nb = int(model[3:])
        offset, log_model = 1e-3, True
        x = torch.log(T + offset).reshape(-1)
        q = torch.quantile(x, torch.linspace(0, 1, nb + 1)[1:-1])
        b = torch.tensor([-23.025850296020508] + [float(v) for v in q] + [float(x.max()) + 0.5])
    Y = ro.quantize(T, sigma, b, offset=offset, log_model=log_model, noise=noise).unsqueeze(1)
    Wx = torch.bernoulli(torch.full((K, 1, I, J), RATE), generator=g)
    Wx[:, :, 0, 0] = 0  # pixel 0 is unobserved
    d = dict(name=name, R=R, K=K, S=S, C=C, Y=Y, Wx=Wx, b=b, sigma=sigma, offset=offset,
             log_model=log_model, loss=loss, nbins=len(b) - 1)
    _PROB[name] = d
    return d


def model_of(d):
    """The numpy-side model arguments of a problem dict."""
    return dict(C=d["C"].double().numpy(), Y=d["Y"].reshape(d["K"], -1).numpy(),
                Wx=d["Wx"].reshape(d["K"], -1).numpy(), b=d["b"].double().numpy(),
                sigma=d["sigma"], offset=d["offset"], log_model=d["log_model"], loss=d["loss"])


def default_kind(log_model):
    return "expected" if log_model else "observed"


def evaluate(S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", kind="observed",
             ridge=0.0, dtype=np.float64, exact_scale=False):
    """(f (P,), g (R, P), J (P, R, R)) at S (R, P), every operation in `dtype`."""
    S = np.asarray(S, dtype)
    C = np.asarray(C, dtype)
    Y = np.asarray(Y).astype(np.int64)
    W = np.asarray(Wx) != 0
    e = ir.edges_of(b, log_model).astype(dtype)
    a = ir.link_scale(sigma, loss, exact_scale)
    T = (C.T @ S).astype(dtype)
    one = dtype(1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if log_model:
            tp = T + dtype(offset)
            neg = W & ~(tp > 0)
            x = np.log(np.where(tp > 0, tp, one))
            ti = one / np.where(tp > 0, tp, one)
        else:
            neg = np.zeros_like(W)
            x, ti = T, np.ones_like(T)
        Pr, P1, P2 = ir.bin_terms(x, e[Y], e[Y + 1], a, loss)
        use = W & (Pr > 0) & ~neg
        Ps = np.where(Pr > 0, Pr, one)
        gx = -P1 / Ps
        if kind == "observed":
            h = gx * gx - P2 / Ps
            if log_model:
                h = h - gx
        elif kind == "expected":
            h = np.zeros_like(x)
            for c in range(len(e) - 1):
                Pb, Pb1, _ = ir.bin_terms(x, e[c], e[c + 1], a, loss)
                h = h + np.where(Pb > 0, Pb1 * Pb1 / np.where(Pb > 0, Pb, one), 0)
        else:
            raise ValueError(kind)
        h = (h * ti * ti).astype(dtype)
        gt = (gx * ti).astype(dtype)
        fe = -np.log(np.maximum(Pr, dtype(FLT_MIN)))
    fe = np.where(W, fe, 0).astype(dtype)
    gt = np.where(use, gt, 0).astype(dtype)
    h = np.where(use, h, 0).astype(dtype)
    f = fe.sum(axis=0) + dtype(0.5 * ridge) * (S * S).sum(axis=0)
    f = np.where(neg.any(axis=0), dtype(np.inf), f).astype(dtype)
    g = (C @ gt).astype(dtype)
    Jb = np.einsum("kp,rk,sk->prs", h, C, C).astype(dtype)
    assert f.dtype == dtype and g.dtype == dtype and Jb.dtype == dtype
    return f, g, Jb


def chol_solve(A, rhs, mu):
    """Batched Cholesky solve of A (P, R, R) x = rhs (P, R) in A's dtype: (x, ok, ident) with ok
    False where a pivot was not positive (replaced by 1) and ident True where every pivot > mu."""
    n, R, _ = A.shape
    dt = A.dtype
    L = np.zeros_like(A)
    ok = np.ones(n, bool)
    ident = np.ones(n, bool)
    for j in range(R):
        piv = A[:, j, j] - (L[:, j, :j] * L[:, j, :j]).sum(axis=1, dtype=dt)
        ident &= piv > mu
        bad = ~(piv > 0)
        ok &= ~bad
        d = np.sqrt(np.where(bad, dt.type(1), piv))
        L[:, j, j] = d
        for i in range(j + 1, R):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1, dtype=dt)) / d
    y = np.zeros_like(rhs)
    for i in range(R):
        y[:, i] = (rhs[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1, dtype=dt)) / L[:, i, i]
    x = np.zeros_like(rhs)
    for i in range(R - 1, -1, -1):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1, dtype=dt)) / L[:, i, i]
    return x, ok, ident


def fit(S_init, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", kind=None,
        ridge=0.0, max_steps=30, tol=1e-5, mu0=1e-3, project=None, dtype=np.float64,
        trace=None):
    """The iteration of qsc_sfit on dense inputs.  Returns a dict: S (R, P), f (P,), steps (P,),
    converged (P,) bool, identified (P,) bool.  `trace` (a list) receives the accepted f (P,) after
    the evaluation at S_init and after every step."""
    kind = default_kind(log_model) if kind is None else kind
    project = bool(log_model) if project is None else bool(project)
    ev = lambda S: evaluate(S, C, Y, Wx, b, sigma, offset, log_model, loss, kind, ridge, dtype)
    s = np.array(S_init, dtype)
    R, n = s.shape
    f, g, Jb = ev(s)
    mu = np.full(n, mu0, dtype)
    mu_floor = dtype(0.0 if mu0 == 0 else MU_MIN)
    done = np.zeros(n, bool)
    ident = np.zeros(n, bool)
    steps = np.zeros(n, np.int32)
    eye = np.eye(R, dtype=dtype)
    if trace is not None:
        trace.append(f.copy())
    for _ in range(int(max_steps)):
        if done.all():
            break
        A = Jb + (dtype(ridge) + mu)[:, None, None] * eye
        rhs = (g + dtype(ridge) * s).T.copy()
        delta, ok, idn = chol_solve(A.astype(dtype), rhs.astype(dtype), mu)
        ident |= ok & idn & ~done
        st = s - delta.T
        if project:
            st = np.maximum(st, dtype(0))
        move = ok & ~done
        st = np.where(move[None, :], st, s).astype(dtype)
        ft, gt, Jt = ev(st)
        acc = ok & (ft <= f) & np.isfinite(ft) & ~done
        rej = ~acc & ~done
        dmax = np.abs(st - s).max(axis=0)
        conv = acc & (dmax <= dtype(tol) * (dtype(1) + np.abs(s).max(axis=0)))
        steps += (~done).astype(np.int32)
        s = np.where(acc[None, :], st, s)
        g = np.where(acc[None, :], gt, g)
        Jb = np.where(acc[:, None, None], Jt, Jb)
        f = np.where(acc, ft, f)
        mu = np.where(acc, np.maximum(mu / dtype(10), mu_floor), mu)
        mu = np.where(rej, np.maximum(dtype(10) * mu, dtype(MU_MIN)), mu).astype(dtype)
        done |= conv
        if trace is not None:
            trace.append(f.copy())
    return dict(S=s, f=f, steps=steps, converged=done, identified=ident)


def minimise_fp64(S_init, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit",
                  kind=None, ridge=0.0, project=None):
    """The minimiser in fp64: the same iteration run to tol = 1e-12, then plain Newton steps on
    the stationarity condition (the f' <= f test cannot see a decrease below one ulp of f, which
    leaves a gradient of about sqrt(ulp(f) lambda)); with project, on the variables that are not
    held at the bound s = 0 by an outward gradient."""
    project = bool(log_model) if project is None else bool(project)
    r = fit(S_init, C, Y, Wx, b, sigma, offset, log_model, loss, kind, ridge, max_steps=500,
            tol=1e-12, mu0=1e-3, project=project, dtype=np.float64)
    s = r["S"].copy()
    obsd = observed_pixels(Wx)
    for _ in range(20):
        _, g, Jb = evaluate(s, C, Y, Wx, b, sigma, offset, log_model, loss, "observed", ridge)
        g = g + ridge * s
        held = (s <= 0) & (g > 0) if project else np.zeros(s.shape, bool)
        if np.abs(np.where(held, 0.0, g)[:, obsd]).max(initial=0.0) < 1e-12:
            break
        for p in np.flatnonzero(obsd):
            fr = ~held[:, p]
            A = Jb[p][np.ix_(fr, fr)] + ridge * np.eye(int(fr.sum()))
            s[fr, p] -= np.linalg.solve(A, g[fr, p])
        if project:
            s = np.maximum(s, 0.0)
    r["S"] = s
    return r


def gradient_fp64(S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", ridge=0.0,
                  project=False):
    """g + ridge s (R, P) in fp64 at S; with project the projected gradient (components at the
    bound s = 0 that point outwards, g > 0, are 0)."""
    S = np.asarray(S, np.float64)
    _, g, _ = evaluate(S, C, Y, Wx, b, sigma, offset, log_model, loss, "observed", ridge)
    g = g + ridge * S
    if project:
        g = np.where((S <= 0) & (g > 0), 0.0, g)
    return g


def observed_pixels(Wx):
    return (np.asarray(Wx) != 0).any(axis=0)
