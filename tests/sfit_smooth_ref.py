"""CPU reference (numpy, fp64 or fp32) of the red-black Newton fit of S under the smoothness prior
(include/qsc.h: qsc_sfit_smooth; qmc.fit_S_smooth) -- a helper for tests/test_sfit_smooth_host.py
and tests/test_gpu_sfit_smooth.py, not a test file.  Written from the header's statement of the
visit; it imports nothing of the package.  The likelihood terms are tests/sfit_ref.py's
(evaluate, chol_solve), the prior's value is checked against tests/smooth_ref.py by the host test.

A visit of colour c on S (R, P), pixels p = i*J + j of colour (i + j) & 1 == c, the others fixed:
    phi_p(s) = f_p(s) + w sum_{n in N(p)} sum_r rho(s_r - S[r, n])
    g_r  += w rho'(d)     quad: d;  huber: clamp(d / delta, -1, 1)
    J_rr += w kappa(d)    quad: 1;  huber: 1 / max(|d|, delta)
then sfit_ref.fit's iteration on (phi, g, J) for up to inner_steps trial evaluations, mu from mu0.
All pixels are evaluated at once (an own-colour pixel's neighbours are all of the other colour, so
its prior terms see fixed rows only); the pixels of the other colour are `done` from the start.
"""
import numpy as np

import sfit_ref as sr

MU_MIN = sr.MU_MIN
I_, J_ = sr.I, sr.J

# the weight, the Huber delta, the start and the sweep budget of the GPU cases, chosen on the CPU
# (tests/test_sfit_smooth_host.py checks that both references bring `moved` to 0 within SWEEPS on
# every converged-fit case, that the fp64 one then sits at minimise_fp64's point, and that DELTA
# splits the differences at the minimiser).  Measured with these references:
# * at weight 0.3 the Huber cases at ridge 1e-2 need 60 sweeps and more; at 0.05 most end within 20;
# * the start is 0.8 S_true.  From S = 0 the logit and log-model cases stall: a visit restarts mu at
#   mu0 and has inner_steps = 2 trials, which does not raise the damping far enough to get a step
#   accepted in the link's tail, so the pixel does not move, `moved` reads 0 and the fit stops
#   short of the minimiser (fit_S's 30 steps in one launch do raise it);
# * four cases need more than the 30 sweeps that serve the rest (sweeps until `moved` == 0 from
#   0.8 S_true at inner_steps = 2, fp64 / fp32 reference):
#     one-bit R 16, ridge 1e-2, quad    29 /  43   about 49 one-bit samples for 16 unknowns leave
#     one-bit R 16, ridge 1e-2, huber  207 / 279   directions that only the ridge holds
#     4-bin,        ridge 1e-2, huber   61 /  59   the pixel without observations has only
#     logit,        ridge 1e-2, huber  105 / 105   ridge / 2 |s|^2 and the prior's linear branch
#   (inner_steps = 6 brings the last two to 23 and 37 and does not help the first two).  Their
#   budgets below are those counts with a margin; the second case is left out (see CONVERGED).
WEIGHT = 0.05
DELTA = 0.1
SWEEPS = 30
INNER = 2
KINDS = [("quad", None), ("huber", DELTA)]
BUDGET = {("onebit16", 1e-2, "quad"): 60, ("bins4", 1e-2, "huber"): 80,
          ("logit", 1e-2, "huber"): 130}
# one-bit R 16 at ridge 1e-2 with huber is the one case of the twenty left out: 207 / 279 sweeps
# of this reference, with its fp64 minimiser, take more than three minutes of CPU per test
CONVERGED = [(n, r, k, dl) for n in sr.CASES for r in sr.RIDGES for k, dl in KINDS
             if (n, r, k) != ("onebit16", 1e-2, "huber")]


def budget(name, ridge, kind):
    """The sweep budget of a converged-fit case."""
    return BUDGET.get((name, ridge, kind), SWEEPS)


_MIN = {}


def minimiser(name, ridge, kind, delta):
    """minimise_fp64 of a converged-fit case from near_start, computed once and left unchanged."""
    key = (name, ridge, kind)
    if key not in _MIN:
        d = sr.problem(name)
        r = minimise_fp64(near_start(d), I_, J_, sr.model_of(d), WEIGHT, kind, delta, ridge=ridge,
                          max_sweeps=4 * budget(name, ridge, kind))
        r["S"].setflags(write=False)
        _MIN[key] = r
    return _MIN[key]


def near_start(d):
    """0.8 S_true as (R, P) fp64: the start of the converged-fit cases."""
    return 0.8 * d["S"].reshape(d["R"], -1).double().numpy()


def pixel_rel(a, b):
    """Maximum over pixels of the relative error of the pixel's row in the infinity norm:
    max_p |a[:, p] - b[:, p]|_inf / |b[:, p]|_inf (the absolute error where the reference row is
    exactly 0); a, b (R, n)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num, den = np.abs(a - b).max(axis=0), np.abs(b).max(axis=0)
    return float(np.max(num / np.where(den == 0, 1.0, den)))


def colors(I, J):
    i, j = np.divmod(np.arange(I * J), J)
    return (i + j) & 1


def _pairs(I, J):
    """The four neighbour directions (left, right, up, down) as (own slice, neighbour slice) of an
    (R, I, J) array."""
    a = slice(None)
    return [((a, a, slice(1, None)), (a, a, slice(None, -1))),
            ((a, a, slice(None, -1)), (a, a, slice(1, None))),
            ((a, slice(1, None), a), (a, slice(None, -1), a)),
            ((a, slice(None, -1), a), (a, slice(1, None), a))]


def prior_terms(S, I, J, kind="quad", delta=None, dtype=np.float64):
    """Per pixel, summed over its existing neighbours: (val (P,), g (R, P), kdiag (R, P)) =
    (sum_n sum_r rho(d), sum_n rho'(d), sum_n kappa(d)), d = S[r, p] - S[r, n], in `dtype`."""
    X = np.asarray(S, dtype).reshape(-1, I, J)
    R = X.shape[0]
    val = np.zeros((R, I, J), dtype)
    g = np.zeros((R, I, J), dtype)
    k = np.zeros((R, I, J), dtype)
    for own, nb in _pairs(I, J):
        d = X[own] - X[nb]
        if kind == "quad":
            v, dg, dk = dtype(0.5) * d * d, d, np.ones_like(d)
        elif kind == "huber":
            dl = dtype(delta)
            a = np.abs(d)
            v = np.where(a <= dl, d * d / (dtype(2) * dl), a - dtype(0.5) * dl)
            dg = np.clip(d / dl, dtype(-1), dtype(1))
            dk = dtype(1) / np.maximum(a, dl)
        else:
            raise ValueError(kind)
        val[own] += v.astype(dtype)
        g[own] += dg.astype(dtype)
        k[own] += dk.astype(dtype)
    return val.sum(axis=0).reshape(-1), g.reshape(R, -1), k.reshape(R, -1)


def evaluate(S, I, J, model, kind, ridge, weight, smooth_kind, delta, dtype):
    """(phi (P,), nll (P,), g (R, P), J (P, R, R)) at S, every pixel with its prior terms."""
    f, g, Jb = sr.evaluate(S, kind=kind, ridge=ridge, dtype=dtype, **model)
    nll, _, _ = (f, None, None) if ridge == 0 else sr.evaluate(S, kind=kind, ridge=0.0,
                                                               dtype=dtype, **model)
    v, pg, pk = prior_terms(S, I, J, smooth_kind, delta, dtype)
    w = dtype(weight)
    R = g.shape[0]
    Jb = Jb.copy()
    Jb[:, np.arange(R), np.arange(R)] += (w * pk).T
    return (f + w * v).astype(dtype), nll, (g + w * pg).astype(dtype), Jb.astype(dtype)


def objective(S, I, J, model, ridge, weight, smooth_kind="quad", delta=None):
    """F(S) = NLL + ridge / 2 |S|^2 + weight R(S) in fp64, each edge once."""
    S = np.asarray(S, np.float64)
    f, _, _ = sr.evaluate(S, kind="observed", ridge=ridge, **model)
    v, _, _ = prior_terms(S, I, J, smooth_kind, delta)
    return float(f.sum() + 0.5 * weight * v.sum())


def gradient_fp64(S, I, J, model, ridge, weight, smooth_kind="quad", delta=None, project=False):
    """dF/dS (R, P) in fp64; with project the projected gradient (sfit_ref.gradient_fp64's rule)."""
    S = np.asarray(S, np.float64)
    _, g, _ = sr.evaluate(S, kind="observed", ridge=ridge, **model)
    _, pg, _ = prior_terms(S, I, J, smooth_kind, delta)
    g = g + ridge * S + weight * pg
    if project:
        g = np.where((S <= 0) & (g > 0), 0.0, g)
    return g


def visit(S, color, I, J, model, weight, smooth_kind="quad", delta=None, ridge=0.0, kind=None,
          inner_steps=2, tol=1e-5, mu0=1e-3, project=None, dtype=np.float64):
    """One visit of one colour from S (R, P).  Returns a dict: S (R, P), phi (P,), nll (P,),
    steps (P,), own (P,) bool, moved, unconverged (ints) and identified (P,) bool."""
    log_model = model["log_model"]
    kind = sr.default_kind(log_model) if kind is None else kind
    project = bool(log_model) if project is None else bool(project)
    ev = lambda X: evaluate(X, I, J, model, kind, ridge, weight, smooth_kind, delta, dtype)
    s = np.array(S, dtype)
    s0 = s.copy()
    R, n = s.shape
    own = colors(I, J) == color
    f, nll, g, Jb = ev(s)
    mu = np.full(n, mu0, dtype)
    mu_floor = dtype(0.0 if mu0 == 0 else MU_MIN)
    done = ~own
    ident = np.zeros(n, bool)
    steps = np.zeros(n, np.int32)
    eye = np.eye(R, dtype=dtype)
    for _ in range(int(inner_steps)):
        if done.all():
            break
        A = Jb + (dtype(ridge) + mu)[:, None, None] * eye
        rhs = (g + dtype(ridge) * s).T.copy()
        delta_s, ok, idn = sr.chol_solve(A.astype(dtype), rhs.astype(dtype), mu)
        ident |= ok & idn & ~done
        st = s - delta_s.T
        if project:
            st = np.maximum(st, dtype(0))
        move = ok & ~done
        st = np.where(move[None, :], st, s).astype(dtype)
        ft, nt, gt, Jt = ev(st)
        acc = ok & (ft <= f) & np.isfinite(ft) & ~done
        rej = ~acc & ~done
        dmax = np.abs(st - s).max(axis=0)
        conv = acc & (dmax <= dtype(tol) * (dtype(1) + np.abs(s).max(axis=0)))
        steps += (~done).astype(np.int32)
        s = np.where(acc[None, :], st, s)
        g = np.where(acc[None, :], gt, g)
        Jb = np.where(acc[:, None, None], Jt, Jb)
        f = np.where(acc, ft, f)
        nll = np.where(acc, nt, nll)
        mu = np.where(acc, np.maximum(mu / dtype(10), mu_floor), mu)
        mu = np.where(rej, np.maximum(dtype(10) * mu, dtype(MU_MIN)), mu).astype(dtype)
        done = done | conv
    d0 = np.abs(s - s0).max(axis=0)
    moved = own & (d0 > dtype(tol) * (dtype(1) + np.abs(s0).max(axis=0)))
    return dict(S=s, phi=f, nll=nll, steps=steps, own=own, moved=int(moved.sum()),
                unconverged=int((own & ~done).sum()), identified=ident)


def fit(S_init, I, J, model, weight, smooth_kind="quad", delta=None, ridge=0.0, kind=None,
        sweeps=SWEEPS, inner_steps=INNER, tol=1e-5, mu0=1e-3, project=None, dtype=np.float64,
        stop=True, trace=None):
    """The sweep loop of qmc.fit_S_smooth (colour 0, then colour 1; with `stop` it ends after
    the first sweep in which neither colour moved).  Returns a dict: S (R, P), nll, sweeps, steps
    (P,), moved, unidentified (both of the last sweep).  `trace` (a list) receives F in fp64 at
    S_init and after every half-sweep."""
    s = np.array(S_init, dtype)
    n = s.shape[1]
    steps = np.zeros(n, np.int32)
    nll = np.zeros(n, dtype)
    if trace is not None:
        trace.append(objective(s, I, J, model, ridge, weight, smooth_kind, delta))
    done, moved, unident = 0, 0, 0
    for _ in range(int(sweeps)):
        moved, unident = 0, 0
        for color in (0, 1):
            r = visit(s, color, I, J, model, weight, smooth_kind, delta, ridge, kind, inner_steps,
                      tol, mu0, project, dtype)
            s = r["S"]
            steps += r["steps"]
            nll = np.where(r["own"], r["nll"], nll)
            moved += r["moved"]
            unident += int((r["own"] & ~r["identified"]).sum())
            if trace is not None:
                trace.append(objective(s, I, J, model, ridge, weight, smooth_kind, delta))
        done += 1
        if stop and moved == 0:
            break
    return dict(S=s, nll=float(nll.astype(np.float64).sum()), sweeps=done, steps=steps,
                moved=moved, unidentified=unident)


def minimise_fp64(S_init, I, J, model, weight, smooth_kind="quad", delta=None, ridge=0.0,
                  kind=None, project=None, max_sweeps=400):
    """The minimiser of F in fp64: sweeps at tol = 1e-12 (inner_steps 3) until none moves or
    max_sweeps.  (The accept test cannot see a decrease below one ulp of phi, which leaves a
    gradient of about sqrt(ulp(phi) lambda) ~ 1e-8: three orders below the fp32 floor.)"""
    return fit(S_init, I, J, model, weight, smooth_kind, delta, ridge, kind, sweeps=max_sweeps,
               inner_steps=3, tol=1e-12, mu0=1e-3, project=project, dtype=np.float64)
