"""CPU reference (numpy, fp64 or fp32) of the per-bin projected Newton fit of C for known S
(include/qsc.h: qsc_cfit_begin / _iterate / _finish) -- a helper for tests/test_cfit_host.py and
tests/test_gpu_cfit.py, not a test file.  Written from the header's statement of the iteration on
top of tests/sfit_ref.py: the problem is sfit_ref's with the roles of S and C exchanged, so the
evaluation is sfit_ref.evaluate with the arguments transposed (S as the "spectra", Y.T, Wx.T) and
the solve is sfit_ref.chol_solve.

Per bin k, c = C[:, k], entries p with Wx[k, p] != 0, t = S[:, p] . c:
    f = sum -log max(P, FLT_MIN) + ridge / 2 |c|^2,   g = sum g_t s_p,   J = sum h s_p s_p^T
The iteration: evaluate at C_init, mu = mu0; up to max_steps times: gamma = g + ridge c; with
project the held set A = {r : c_r <= 0 and gamma_r > 0}; Cholesky of J + (ridge + mu) I with the
rows and columns of A replaced by the identity and gamma_A = 0; c' = c - delta (clipped at 0 with
project); a pivot <= 0 rejects the step; accept iff f' <= f and finite
(mu <- max(mu / 10, 0 if mu0 == 0 else MU_MIN)), else mu <- max(10 mu, MU_MIN); converged once an
accepted step has |c' - c|_inf <= tol (1 + |c|_inf).  A bin is identified once a factorisation has
every pivot of its free rows > mu.  With project = False no operation differs from sfit_ref.fit
on the transposed inputs (tests/test_cfit_host.py checks equality).
"""
import numpy as np

import sfit_ref as sr

MU_MIN = sr.MU_MIN
CASES = sr.CASES
RIDGES = sr.RIDGES
I, J, P, TILE = sr.I, sr.J, sr.P, sr.TILE
MAX_STEPS = 40

_PROB = {}


def problem(name):
    """sfit_ref.problem(name) with bin 0 of Wx cleared: an unobserved bin."""
    if name not in _PROB:
        d = dict(sr.problem(name))
        Wx = d["Wx"].clone()
        Wx[0] = 0
        d["Wx"] = Wx
        _PROB[name] = d
    return _PROB[name]


def model_of(d):
    """The numpy-side arguments of a problem dict: S (R, P) known, Y / Wx (K, P)."""
    return dict(S=d["S"].reshape(d["R"], -1).double().numpy(), Y=d["Y"].reshape(d["K"], -1).numpy(),
                Wx=d["Wx"].reshape(d["K"], -1).numpy(), b=d["b"].double().numpy(),
                sigma=d["sigma"], offset=d["offset"], log_model=d["log_model"], loss=d["loss"])


def default_start(d):
    return (np.ones if d["log_model"] else np.zeros)((d["R"], d["K"]))


def evaluate(C, S, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", kind="observed",
             ridge=0.0, dtype=np.float64):
    """(f (K,), g (R, K), J (K, R, R)) at C (R, K): sfit_ref.evaluate, transposed."""
    return sr.evaluate(C, S, np.asarray(Y).T, np.asarray(Wx).T, b, sigma, offset, log_model, loss,
                       kind, ridge, dtype)


def fit(C_init, S, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", kind=None,
        ridge=0.0, max_steps=30, tol=1e-5, mu0=1e-3, project=True, dtype=np.float64, trace=None):
    """The iteration on dense inputs.  Returns a dict: C (R, K), f (K,), steps (K,), converged
    (K,) bool, identified (K,) bool, held (R, K) bool (the held set of the last factorisation)."""
    kind = sr.default_kind(log_model) if kind is None else kind
    ev = lambda C: evaluate(C, S, Y, Wx, b, sigma, offset, log_model, loss, kind, ridge, dtype)
    c = np.array(C_init, dtype)
    R, n = c.shape
    f, g, Jb = ev(c)
    mu = np.full(n, mu0, dtype)
    mu_floor = dtype(0.0 if mu0 == 0 else MU_MIN)
    done = np.zeros(n, bool)
    ident = np.zeros(n, bool)
    steps = np.zeros(n, np.int32)
    held = np.zeros((R, n), bool)
    eye = np.eye(R, dtype=dtype)
    if trace is not None:
        trace.append(f.copy())
    for _ in range(int(max_steps)):
        if done.all():
            break
        A = Jb + (dtype(ridge) + mu)[:, None, None] * eye
        gam = g + dtype(ridge) * c
        held = (c <= 0) & (gam > 0) if project else np.zeros((R, n), bool)
        h = held.T  # (n, R)
        # rows and columns of the held set: the identity (scaled above mu, so that the pivot test
        # of the identification only sees the free rows; the held delta is 0 either way)
        A = np.where(h[:, :, None] | h[:, None, :], dtype(0), A)
        A = np.where(h[:, :, None] & eye.astype(bool)[None], (dtype(1) + dtype(2) * mu)[:, None, None],
                     A)
        rhs = np.where(h, dtype(0), gam.T).copy()
        delta, ok, idn = sr.chol_solve(A.astype(dtype), rhs.astype(dtype), mu)
        ident |= ok & idn & ~done
        ct = c - delta.T
        if project:
            ct = np.maximum(ct, dtype(0))
        move = ok & ~done
        ct = np.where(move[None, :], ct, c).astype(dtype)
        ft, gt, Jt = ev(ct)
        acc = ok & (ft <= f) & np.isfinite(ft) & ~done
        rej = ~acc & ~done
        dmax = np.abs(ct - c).max(axis=0)
        conv = acc & (dmax <= dtype(tol) * (dtype(1) + np.abs(c).max(axis=0)))
        steps += (~done).astype(np.int32)
        c = np.where(acc[None, :], ct, c)
        g = np.where(acc[None, :], gt, g)
        Jb = np.where(acc[:, None, None], Jt, Jb)
        f = np.where(acc, ft, f)
        mu = np.where(acc, np.maximum(mu / dtype(10), mu_floor), mu)
        mu = np.where(rej, np.maximum(dtype(10) * mu, dtype(MU_MIN)), mu).astype(dtype)
        done |= conv
        if trace is not None:
            trace.append(f.copy())
    return dict(C=c, f=f, steps=steps, converged=done, identified=ident, held=held)


def gradient_fp64(C, S, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", ridge=0.0,
                  project=True):
    """g + ridge c (R, K) in fp64 at C; with project the projected gradient (components at the
    bound c = 0 that point outwards, gamma > 0, are 0)."""
    C = np.asarray(C, np.float64)
    _, g, _ = evaluate(C, S, Y, Wx, b, sigma, offset, log_model, loss, "observed", ridge)
    g = g + ridge * C
    if project:
        g = np.where((C <= 0) & (g > 0), 0.0, g)
    return g


def std_fp64(C, S, Y, Wx, b, sigma, offset=0.0, log_model=False, loss="probit", kind="observed",
             ridge=0.0, dtype=np.float64):
    """sqrt(diag((J + ridge I)^-1)) (R, K) of the blocks at C, every operation in `dtype`; +inf
    for a bin whose block is not positive definite."""
    _, _, Jb = evaluate(C, S, Y, Wx, b, sigma, offset, log_model, loss, kind, 0.0, dtype)
    R = Jb.shape[1]
    out = np.full((R, Jb.shape[0]), np.inf)
    for k in range(Jb.shape[0]):
        A = (Jb[k] + dtype(ridge) * np.eye(R, dtype=dtype)).astype(dtype)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        M = np.linalg.inv(L).astype(dtype)
        out[:, k] = np.sqrt((M * M).sum(axis=0))
    return out


def observed_bins(Wx):
    return (np.asarray(Wx) != 0).any(axis=1)
