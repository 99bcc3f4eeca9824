"""CPU reference (numpy, fp64 or fp32) of the calibration fit of the observation model's own
parameters (include/qsc.h: qsc_qfit_*, qsc_entry_calib) -- a helper for tests/test_qfit_host.py
and tests/test_gpu_qfit.py, not a test file.  Written from the header's statement of the problem
and the iteration; it imports nothing of the package.  P comes from tests/info_ref.py (bin_terms).

theta = (tau, beta): the link's divisor a = a0 e^tau (a0 = fp32(sigma0 * 1.414213) probit, s0
logit) and every interior, finite edge b_i + beta (the linear model's clamp edges -1e5, +1e5 stay).
Per entry at x (x = t or log(t + offset)), with u = (hi - x) / a, w = (lo - x) / a on the shifted
edges, psi the density in z-units, du/dtau = -u, du/dbeta = 1 / a (0 for an unshifted edge):
    P_tau = -(u psi(u) - w psi(w))               P_beta = (psi(u) - psi(w)) / a
    P_tt  = (z psi + z^2 psi')(u) - (...)(w)     P_tb   = -((psi + z psi')(u) - (...)(w)) / a
    P_bb  = (psi'(u) - psi'(w)) / a^2
    f = -log max(P, FLT_MIN),  g_i = -P_i / P
    observed H_ij = P_i P_j / P^2 - P_ij / P;  expected H_ij = sum_b P_i,b P_j,b / P_b (P_b > 0)
A saturated (|z| >= 14 probit, 100 logit) or infinite edge contributes exactly 0; an entry with
P == 0 adds 0 to g and H; t + offset <= 0 makes F = +inf.
F = sum f + prior_scale / 2 tau^2 + prior_shift / 2 beta^2.  The iteration:
    evaluate at start, mu = mu0; up to max_steps times: solve (H + diag(prior) + mu I) delta =
    g + prior * theta with a parameter that is not fitted an identity row; theta' = theta - delta;
    a pivot <= 0 rejects the step; accept iff F' <= F and finite (mu <- max(mu / 10, 0 if mu0 == 0
    else MU_MIN)), else mu <- max(10 mu, MU_MIN); converged once an accepted step has
    |theta' - theta|_inf <= tol (1 + |theta|_inf); identified once a factorisation has every pivot
    of a fitted row > mu.

The cases are tests/sfit_ref.py's five (shapes, S, C, edges, sigma0, mask), with the codes drawn
anew at sigma_true = 1.5 sigma0 and the interior edges moved by shift_true = a quarter of the
median bin width, so that the minimiser is well away from the start (0, 0).
"""
import math

import numpy as np
import torch

import info_ref as ir
import sfit_ref as sr
from oracle import reference_ops as ro

MU_MIN = 1e-6
FLT_MIN = float(np.finfo(np.float32).tiny)
SAT = {"probit": 14.0, "logit": 100.0}
SCALE_TRUE = 1.5
CASES = sr.CASES
P, TILE = sr.P, sr.TILE
MAX_STEPS = 30
# The start of every case is (0, 0), the packed model, but for the one-bit probit case: its
# threshold 3.5 sits at the lower end of the map values (3.0 .. 8.9), so few entries inform the
# two parameters, the scoring steps from (0, 0) are rejected over and over while mu climbs, and the
# fp64 reference needs exactly the 30 steps allowed (the fp32 one 30 as well): no margin for an
# implementation that rounds differently.  From (0, 0.5), still 0.7 from the minimiser
# (0.42, 1.23), both need 15.
START = {"onebit16": (0.0, 0.5)}

_PROB = {}


def start_of(name):
    return START.get(name, (0.0, 0.0))


def shifted_bounds(b, beta, log_model):
    """The boundary list at beta (fp64): interior edges (linear model) or every finite edge (log
    model) + beta."""
    b = np.asarray(b, np.float64).copy()
    if log_model:
        fin = np.isfinite(b)
        b[fin] += beta
    else:
        b[1:-1] += beta
    return b


def problem(name):
    """sfit_ref.problem(name) with Y drawn at SCALE_TRUE sigma0 on edges shifted by shift_true
    (built once; Y of the original is not used)."""
    if name in _PROB:
        return _PROB[name]
    d = dict(sr.problem(name))
    seed = CASES[name][6]
    g = torch.Generator().manual_seed(1000 + seed)
    T = ro.get_tensor(d["S"], d["C"])
    if d["loss"] == "logit":
        u = torch.rand(T.shape, generator=g)
        noise = torch.log(u) - torch.log1p(-u)
    else:
        noise = torch.randn(T.shape, generator=g)
    b = d["b"].double().numpy()
    shift = 0.25 * float(np.median(np.diff(b)))
    bs = torch.tensor(shifted_bounds(b, shift, d["log_model"]), dtype=torch.float32)
    d["Y"] = ro.quantize(T, SCALE_TRUE * d["sigma"], bs, offset=d["offset"],
                         log_model=d["log_model"], noise=noise).unsqueeze(1)
    d["tau_true"], d["shift_true"] = math.log(SCALE_TRUE), shift
    _PROB[name] = d
    return d


def model_of(d):
    """The numpy-side arguments of a problem dict (S, C in fp64 from their fp32 values)."""
    R, K = d["R"], d["K"]
    return dict(S=d["S"].reshape(R, -1).double().numpy(), C=d["C"].double().numpy(),
                Y=d["Y"].reshape(K, -1).numpy(), Wx=d["Wx"].reshape(K, -1).numpy(),
                b=d["b"].double().numpy(), sigma=d["sigma"], offset=d["offset"],
                log_model=d["log_model"], loss=d["loss"])


def edge_table(b, beta, log_model, dtype):
    """(lo, hi, slo, shi) per bin at beta in `dtype`: the edges (clamped in the linear model,
    shifted where they are) and whether each is shifted."""
    nb = len(b) - 1
    e = ir.edges_of(np.asarray(b, np.float32).astype(np.float64), log_model)
    sh = np.isfinite(e) if log_model else np.r_[False, np.ones(nb - 1, bool), False]
    e = np.where(sh, e + beta, e).astype(dtype)
    # (an infinite edge is unshifted and contributes 0 either way)
    return e[:-1], e[1:], sh[:-1], sh[1:]


def _edge(z, loss):
    """psi, z psi, psi', z psi', z^2 psi' at z (an array in its own dtype); exactly 0 when
    saturated or infinite."""
    dt = z.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.abs(z) < dt(SAT[loss])
        zs = np.where(fin, z, dt(0))
        if loss == "logit":
            E = np.where(fin, np.exp(-np.abs(zs)), dt(0))
            r = dt(1) / (dt(1) + E)
            A = E * r * r
            D = A * (np.where(zs < 0, dt(1), dt(-1)) * (dt(1) - E) * r)
        else:
            A = np.where(fin, np.exp(-zs * zs) * dt(1.0 / math.sqrt(math.pi)), dt(0))
            D = dt(-2) * (zs * A)
    return A, zs * A, D, zs * D, zs * zs * D


def bin_calib(x, lo, hi, slo, shi, a, loss):
    """(P, (P_tau, P_beta), (P_tt, P_tb, P_bb)) of the bin (lo, hi) at x, all in x's dtype."""
    dt = x.dtype.type
    a = dt(a)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        P = ir.bin_terms(x, lo, hi, float(a), loss)[0].astype(x.dtype)
        Au, Bu, Du, zDu, zzDu = _edge(((hi - x) / a).astype(x.dtype), loss)
        Aw, Bw, Dw, zDw, zzDw = _edge(((lo - x) / a).astype(x.dtype), loss)
    hu, hw = np.where(shi, dt(1), dt(0)), np.where(slo, dt(1), dt(0))
    ia = dt(1) / a
    P1 = (-(Bu - Bw), (hu * Au - hw * Aw) * ia)
    P2 = ((Bu + zzDu) - (Bw + zzDw), -(hu * (Au + zDu) - hw * (Aw + zDw)) * ia,
          (hu * Du - hw * Dw) * (ia * ia))
    return P, P1, P2


def link_scale(sigma, loss, tau, dtype):
    a0 = ir.link_scale(sigma, loss)  # fp32(sigma * 1.414213), or s
    return dtype(a0 * math.exp(float(tau)))


def terms(T, Y, b, sigma, tau, beta, offset=0.0, log_model=False, loss="probit", kind="expected",
          dtype=np.float64):
    """Per-entry (f, g (2, ...), H (3, ...), neg) at the map values T and codes Y, every operation
    in `dtype`.  neg marks t + offset <= 0 (f there is +inf)."""
    T = np.asarray(T, dtype)
    Y = np.asarray(Y).astype(np.int64)
    lo, hi, slo, shi = edge_table(b, beta, log_model, dtype)
    a = link_scale(sigma, loss, tau, dtype)
    one = dtype(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if log_model:
            tp = T + dtype(offset)
            neg = ~(tp > 0)
            x = np.log(np.where(neg, one, tp)).astype(dtype)
        else:
            neg = np.zeros(T.shape, bool)
            x = T
        Pr, P1, P2 = bin_calib(x, lo[Y], hi[Y], slo[Y], shi[Y], a, loss)
        use = (Pr > 0) & ~neg
        Ps = np.where(Pr > 0, Pr, one)
        g = [-P1[0] / Ps, -P1[1] / Ps]
        if kind == "observed":
            H = [g[0] * g[0] - P2[0] / Ps, g[0] * g[1] - P2[1] / Ps, g[1] * g[1] - P2[2] / Ps]
        elif kind == "expected":
            H = [np.zeros_like(x) for _ in range(3)]
            for c in range(len(lo)):
                Pb, Q1, _ = bin_calib(x, lo[c], hi[c], slo[c], shi[c], a, loss)
                on = Pb > 0
                Pd = np.where(on, Pb, one)
                qt, qb = Q1[0] / Pd, Q1[1] / Pd
                H[0] = H[0] + np.where(on, Q1[0] * qt, 0)
                H[1] = H[1] + np.where(on, Q1[1] * qt, 0)
                H[2] = H[2] + np.where(on, Q1[1] * qb, 0)
        else:
            raise ValueError(kind)
        f = -np.log(np.maximum(Pr, dtype(FLT_MIN)))
    f = np.where(neg, dtype(np.inf), f).astype(dtype)
    g = np.stack([np.where(use, v, 0) for v in g]).astype(dtype)
    H = np.stack([np.where(use, v, 0) for v in H]).astype(dtype)
    return f, g, H, neg


def evaluate(theta, S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit",
             kind="expected", prior=(0.0, 0.0), dtype=np.float64):
    """(F, g (2,), H (3,)) over the dense masked problem at theta, in `dtype`; F includes the
    prior, g and H do not."""
    W = np.asarray(Wx) != 0
    T = (np.asarray(C, dtype).T @ np.asarray(S, dtype)).astype(dtype)
    f, g, H, _ = terms(T, Y, b, sigma, theta[0], theta[1], offset, log_model, loss, kind, dtype)
    F = np.where(W, f, 0).sum(dtype=dtype)
    F = dtype(F + dtype(0.5 * prior[0]) * dtype(theta[0]) ** 2
              + dtype(0.5 * prior[1]) * dtype(theta[1]) ** 2)
    g = np.where(W[None], g, 0).reshape(2, -1).sum(axis=1, dtype=dtype)
    H = np.where(W[None], H, 0).reshape(3, -1).sum(axis=1, dtype=dtype)
    return F, g, H


def solve2(A, free, mu, rhs):
    """delta of the damped 2 x 2 system (a held row the identity): (delta, ok, ident)."""
    dt = rhs.dtype.type
    ok = ident = True
    p0 = A[0]
    if free[0]:
        ident = ident and bool(p0 > mu)
        if not p0 > 0:
            ok, p0 = False, dt(1)
    l10 = A[1] / p0
    p1 = A[2] - l10 * A[1]
    if free[1]:
        ident = ident and bool(p1 > mu)
        if not p1 > 0:
            ok, p1 = False, dt(1)
    d1 = (rhs[1] - l10 * rhs[0]) / p1
    return np.array([rhs[0] / p0 - l10 * d1, d1], rhs.dtype), ok, ident


def fit(S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", fit=(True, True),
        kind="expected", prior=(0.0, 0.0), start=(0.0, 0.0), max_steps=MAX_STEPS, tol=1e-6,
        mu0=1e-3, dtype=np.float64, trace=None):
    """The iteration of qsc_qfit_* on dense inputs.  Returns a dict: theta (2,), F, F_start, g, H
    (the accepted ones), steps, converged, identified."""
    ev = lambda th: evaluate(th, S, C, Y, Wx, b, sigma, offset, log_model, loss, kind, prior, dtype)
    free = (bool(fit[0]), bool(fit[1]))
    pr = np.array(prior, dtype)
    th = np.array(start, dtype)
    F, g, H = ev(th)
    F0 = F
    mu, mu_floor = dtype(mu0), dtype(0.0 if mu0 == 0 else MU_MIN)
    done = ident = False
    step_ok = True
    steps = 0
    if trace is not None:
        trace.append(float(F))
    while steps < int(max_steps) and not done:
        A = np.array([H[0] + pr[0] + mu if free[0] else 1, H[1] if all(free) else 0,
                      H[2] + pr[1] + mu if free[1] else 1], dtype)
        rhs = np.where(free, g + pr * th, 0).astype(dtype)
        delta, ok, idn = solve2(A, free, mu, rhs)
        ident = ident or (ok and idn)
        step_ok = ok
        tt = np.where(np.array(free) & ok, th - delta, th).astype(dtype)
        Ft, gt, Ht = ev(tt)
        steps += 1
        acc = step_ok and bool(Ft <= F) and bool(np.isfinite(Ft))
        if acc:
            done = bool(np.abs(tt - th).max() <= dtype(tol) * (dtype(1) + np.abs(th).max()))
            th, F, g, H = tt, Ft, gt, Ht
            mu = max(mu / dtype(10), mu_floor)
        else:
            mu = max(dtype(10) * mu, dtype(MU_MIN))
        if trace is not None:
            trace.append(float(F))
    return dict(theta=th, F=F, F_start=F0, g=g, H=H, steps=steps, converged=done,
                identified=ident)


def gradient_fp64(theta, S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit",
                  prior=(0.0, 0.0), fit=(True, True)):
    """g + prior * theta (2,) in fp64 at theta; 0 for a parameter that is not fitted."""
    th = np.asarray(theta, np.float64)
    _, g, _ = evaluate(th, S, C, Y, Wx, b, sigma, offset, log_model, loss, "observed", prior)
    return np.where(fit, g + np.asarray(prior) * th, 0.0)


def minimise_fp64(S, C, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit",
                  fit=(True, True), prior=(0.0, 0.0), start=(0.0, 0.0)):
    """The minimiser in fp64: the iteration at tol = 1e-12, then plain Newton steps on the
    stationarity condition with the observed Hessian (the F' <= F test cannot see a decrease
    below one ulp of F)."""
    m = dict(S=S, C=C, Y=Y, Wx=Wx, b=b, sigma=sigma, offset=offset, log_model=log_model, loss=loss)
    r = globals()["fit"](fit=fit, kind="expected", prior=prior, start=start, max_steps=500,
                         tol=1e-12, **m)
    th = r["theta"].copy()
    free = np.array(fit, bool)
    for _ in range(20):
        _, g, H = evaluate(th, kind="observed", prior=prior, **m)
        g = np.where(free, g + np.asarray(prior) * th, 0.0)
        if np.abs(g).max() < 1e-10:
            break
        A = np.array([[H[0] + prior[0], H[1]], [H[1], H[2] + prior[1]]])
        A = np.where(np.outer(free, free), A, np.eye(2))
        th = th - np.linalg.solve(A, g)
    r["theta"] = th
    return r
