"""The post-solve estimators (not in the reference): confidence, design, check_fit, the Newton
fits fit_S, fit_C, fit_S_smooth and fit_noise, model_nll, calibrate, bootstrap, cross_validate,
acquire (the sequential-sensing loop over design, Observations.append and the fits), and the
stage of solve() that runs them on its
result (check_post_solve, post_solve).  Every public function validates its arguments before
anything touches a device; the `_*_pos` drivers take a position-order S (Pp, RP) and device
tensors.  qmc re-exports the names: qmc.fit_S etc. stay the user-facing spellings.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import _lib
from ._model import _dev
from .fused import check_smooth, smooth_kind as _kind_code
from .obs import Observations

INFO_KINDS = {"expected": 0, "observed": 1}  # QSC_INFO_EXPECTED, QSC_INFO_OBSERVED


def _check_newton(name, loss, kind, ridge, mu0, tol, max_steps, kind_optional=True):
    """Validate the arguments every Newton fit takes; `name` is the fit's, for the messages.
    ridge=None: the fit has none.  kind=None (the fit picks the model's default) passes where
    kind_optional."""
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: %s has nothing to fit' % name)
    if not (kind is None and kind_optional) and kind not in INFO_KINDS:
        raise ValueError("%s kind must be one of %s, got %r" % (name, sorted(INFO_KINDS), kind))
    if ridge is not None and not float(ridge) >= 0.0:
        raise ValueError("the %s ridge must be >= 0, got %r" % (name, ridge))
    if not float(mu0) >= 0.0:
        raise ValueError("mu0 must be >= 0, got %r" % (mu0,))
    if not float(tol) > 0.0:
        raise ValueError("tol must be > 0, got %r" % (tol,))
    if int(max_steps) < 1:
        raise ValueError("max_steps must be >= 1, got %r" % (max_steps,))


def _defaults(obs, kind, project):
    """(kind, project) with None replaced by the model's default: Fisher scoring and S >= 0
    under the log model, Newton and no projection otherwise."""
    log_model = bool(getattr(obs, "log_model", False))
    if kind is None:
        kind = "expected" if log_model else "observed"
    if project is None:
        project = log_model
    return kind, project


def _start(obs, X_init, R, n):
    """X_init, or the default start (R, n): ones under the log model, zeros otherwise."""
    if X_init is None:
        log_model = bool(getattr(obs, "log_model", False))
        X_init = (torch.ones if log_model else torch.zeros)(R, n)
    return X_init


def _inputs(obs, S, C, R):
    """(S_pos (Pp, RP) in position order, Cd (R, K) contiguous), fp32 on the device."""
    S_pos = obs.to_positions(S.detach().to(torch.float32).reshape(R, -1))
    Cd = _dev(C.detach().to(torch.float32)).reshape(R, obs.K).contiguous()
    return S_pos, Cd


def _iterate(step, n, sync_every, active):
    """Call step() up to n times; after every sync_every-th call evaluate active() (the one
    device read-back) and stop where it is 0.  With sync_every = 0 active() is never called:
    nothing is read back and the sequence can be captured into a hipGraph.  -> the calls made."""
    for i in range(1, n + 1):
        step()
        if sync_every and i % int(sync_every) == 0 and int(active()) == 0:
            return i
    return n


@dataclass
class ConfidenceResult:
    std_S: torch.Tensor                 # (R, 1, I, J), pixel order; +inf where unidentified
    std_T: Optional[torch.Tensor]       # (K, 1, I, J) or None (map_std=False)
    info: torch.Tensor                  # (P, R, R) information blocks J_p, pixel order
    unidentified: int                   # pixels whose J_p + ridge I is not positive definite


def check_confidence(kind, ridge, loss):
    """Validate the confidence arguments (before anything touches a device)."""
    if kind not in INFO_KINDS:
        raise ValueError("confidence kind must be one of %s, got %r" % (sorted(INFO_KINDS), kind))
    if ridge is not None and not float(ridge) >= 0.0:
        raise ValueError("the confidence ridge must be >= 0, got %r" % (ridge,))
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: it has no Fisher information')


def _info_blocks_pos(obs, S_pos, C, R, kind):
    """qsc_sinfo on a position-order S (Pp, RP) and a device C (R, K): J (Pp, RP, RP)."""
    desc, s_entries, _ = obs.layout(R)
    RP = obs.rank_pad(R)
    J = torch.empty((obs.Pp, RP, RP), dtype=torch.float32, device=S_pos.device)
    _lib.call("qsc_sinfo", desc, _lib.ptr(s_entries), _lib.ptr(obs.s_width), _lib.ptr(obs.s_off),
              obs.model, R, _lib.ptr(S_pos), _lib.ptr(C), INFO_KINDS[kind], _lib.ptr(J),
              _lib.stream())
    return J


def _confidence_pos(obs, S_pos, C, R, kind, ridge, map_std):
    """confidence() on a position-order S (Pp, RP) and a device C (R, K)."""
    RP = obs.rank_pad(R)
    dev = S_pos.device
    J = _info_blocks_pos(obs, S_pos, C, R, kind)
    std_pos = torch.empty((obs.Pp, RP), dtype=torch.float32, device=dev)
    std_T = torch.empty((obs.K, obs.P), dtype=torch.float32, device=dev) if map_std else None
    nbad = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("qsc_info_std", _lib.ptr(J), _lib.ptr(obs.perm), R, obs.P, obs.Pp, _lib.ptr(C),
              obs.K, float(ridge), _lib.ptr(std_pos), _lib.ptr(std_T), _lib.ptr(nbad),
              _lib.stream())
    std_S = obs.to_pixels(std_pos, R).reshape(R, 1, obs.I, obs.J)
    info = J[obs.iperm().long()][:, :R, :R].contiguous()
    if std_T is not None:
        std_T = std_T.reshape(obs.K, 1, obs.I, obs.J)
    return ConfidenceResult(std_S=std_S, std_T=std_T, info=info, unidentified=int(nbad.item()))


def confidence(obs, S, C, kind="expected", ridge=0.0, map_std=False):
    """Laplace / Cramer-Rao confidence of the loss fields S and of the map at (S, C).

    Conditional on C, the Hessian of the NLL in S is block diagonal: pixel p has the R x R block
    J_p = sum_{k observed at p} h(k, p) c_k c_k^T, c_k = C[:, k], with h the curvature of one
    entry's -log P in T_hat[k, p] (include/qsc.h, qsc_sinfo, has the formulas).  kind="expected"
    takes the Fisher information of each entry (independent of the observed code, J_p >= 0: the
    Cramer-Rao bound); kind="observed" the curvature at the observed code (the Hessian a double
    backward of the NLL gives; under the log model it may be indefinite).  Then
      std_S[r, p] = sqrt(((J_p + ridge I)^-1)[r, r]),
      std_T[k, p] = sqrt(c_k^T (J_p + ridge I)^-1 c_k)   (map_std=True; delta method, for every
                    map entry, observed or not).
    A pixel whose J_p + ridge I is not positive definite (no observations and ridge = 0, say) is
    unidentified: its standard deviations are +inf and it is counted in `unidentified`.
    C is treated as known -- its R K parameters are informed by all observations, a pixel's R
    values of S by that pixel's few -- so the C-side information and the S-C covariance are not
    included: the figures are lower bounds on the joint uncertainty.
    obs: the Observations the solve ran on; S (R,1,I,J) or (R,P), C (R,K).  Returns a
    ConfidenceResult(std_S (R,1,I,J), std_T (K,1,I,J) or None, info (P,R,R), unidentified).
    Raises ValueError for an unknown kind, ridge < 0 or obs.loss == "squared"."""
    check_confidence(kind, ridge, getattr(obs, "loss", None))
    R = S.shape[0]
    S_pos, Cd = _inputs(obs, S, C, R)
    return _confidence_pos(obs, S_pos, Cd, R, kind, ridge, map_std)


def default_confidence_ridge(S, lambda_s):
    """lambda_s / ||S||_F: the isotropic part of the Hessian of the solver's lambda_s ||S||_F
    regulariser, (lambda_s / ||S||) (I - s s^T / ||S||^2) with s = vec(S); its rank-one part
    couples all pixels and is dropped.  0 for S = 0."""
    n = float(torch.linalg.norm(S.detach().to(torch.float32)))
    return float(lambda_s) / n if n > 0.0 else 0.0


DESIGN_CRITERIA = {"D": 0, "A": 1, "V": 2}  # QSC_DESIGN_D, QSC_DESIGN_A, QSC_DESIGN_V


@dataclass
class DesignResult:
    gain: torch.Tensor                  # (1, I, J), pixel order; +inf for a first look
    first_look: int                     # pixels whose J_p + ridge I is not positive definite
    degenerate: int                     # pixels whose block with the plan is not positive definite
    entry_gain: Optional[torch.Tensor] = None  # (K, 1, I, J) or None (entry_gain=False)

    def best(self, n):
        """The n best sites: (n, 2) int64 rows (i, j) by descending gain, first looks (+inf)
        first; equal gains in pixel order."""
        flat = self.gain.reshape(-1)
        n = int(n)
        if not 1 <= n <= flat.numel():
            raise ValueError("n must be in [1, %d], got %r" % (flat.numel(), n))
        idx = torch.argsort(flat, descending=True, stable=True)[:n].to(torch.int64)
        ncol = self.gain.shape[-1]
        return torch.stack((idx // ncol, idx % ncol), dim=1)


def check_design(criterion, kind, ridge, loss, weights, K):
    """Validate the design arguments (before anything touches a device); the plan as an fp32
    CPU tensor (K,) or None."""
    if criterion not in DESIGN_CRITERIA:
        raise ValueError("design criterion must be one of %s, got %r"
                         % (sorted(DESIGN_CRITERIA), criterion))
    if kind not in INFO_KINDS:
        raise ValueError("design kind must be one of %s, got %r" % (sorted(INFO_KINDS), kind))
    if not float(ridge) >= 0.0:
        raise ValueError("the design ridge must be >= 0, got %r" % (ridge,))
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: it has no Fisher information')
    if weights is None:
        return None
    w = torch.as_tensor(weights).detach().to("cpu", torch.float32)
    if tuple(w.shape) != (int(K),):
        raise ValueError("weights must have shape (%d,), got %s" % (int(K), tuple(w.shape)))
    if not bool((w >= 0).all()) or not bool(torch.isfinite(w).all()):
        raise ValueError("the design weights must be finite and >= 0")
    return w.contiguous()


def _gain_pos(obs, S_pos, C, J, R, w, criterion, ridge):
    """qsc_sgain on a position-order S (Pp, RP), a device C (R, K), the blocks J (Pp, RP, RP) and
    a device plan w (K,) or None: (gain (Pp,), counters (2,) int32: first looks, degenerate)."""
    RP = obs.rank_pad(R)
    dev = S_pos.device
    G = None
    if criterion == "V":
        G = torch.zeros((RP, RP), dtype=torch.float32, device=dev)
        G[:R, :R] = C @ C.t()
    gain = torch.empty(obs.Pp, dtype=torch.float32, device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.call("qsc_sgain", _lib.ptr(S_pos), _lib.ptr(C), _lib.ptr(J), _lib.ptr(obs.perm),
              _lib.ptr(w), _lib.ptr(G), obs.model, R, obs.K, obs.P, obs.Pp,
              DESIGN_CRITERIA[criterion], float(ridge), _lib.ptr(gain), _lib.ptr(counters[0:1]),
              _lib.ptr(counters[1:2]), _lib.stream())
    return gain, counters


def _entry_gain_pos(obs, S, C, J, R, w, ridge):
    """1/2 log1p(w_k h_exp(t_kp) std_T[k, p]^2) (K, P), pixel order: the D gain of one reading of
    bin k at pixel p, from qsc_info_std's std_T and qsc_entry_info (expected kind)."""
    from ._model import get_tensor
    from .utils import entry_information
    dev = J.device
    std_pos = torch.empty((obs.Pp, obs.rank_pad(R)), dtype=torch.float32, device=dev)
    std_T = torch.empty((obs.K, obs.P), dtype=torch.float32, device=dev)
    nbad = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("qsc_info_std", _lib.ptr(J), _lib.ptr(obs.perm), R, obs.P, obs.Pp, _lib.ptr(C),
              obs.K, float(ridge), _lib.ptr(std_pos), _lib.ptr(std_T), _lib.ptr(nbad),
              _lib.stream())
    T = get_tensor(S.reshape(R, 1, obs.I, obs.J), C).reshape(obs.K, obs.P)
    h = entry_information(T, torch.zeros((), dtype=torch.int64, device=dev), obs.bin_boundaries,
                          obs.noise_std, offset=obs.offset, log_model=obs.log_model,
                          loss=obs.loss, kind="expected")
    if obs.log_model:  # (an entry with t + offset <= 0 adds 0: qsc_sgain's rule)
        h = torch.where(T + float(obs.offset) > 0.0, h, torch.zeros_like(h))
    if w is not None:
        h = h * w[:, None]
    eg = 0.5 * torch.log1p(h * std_T * std_T)
    return torch.where(torch.isinf(std_T), torch.full_like(eg, float("inf")), eg)


def design(obs, S, C, weights=None, criterion="D", kind="expected", ridge=0.0, entry_gain=False):
    """Where to measure next: the expected information gain, per pixel, of a planned batch of
    readings at (S, C).

    A plan is `weights` (K,), w_k >= 0 the number of readings planned in bin k (default: one of
    every bin, "a sensor that reads every bin once").  With J_p the information block of the
    readings already held (qmc.confidence's; `kind` selects how it is formed) and h_exp the Fisher
    information of one reading, which does not depend on the code it will return,
      A_p = sum_k w_k h_exp(T_hat[k, p]) c_k c_k^T,   M0 = J_p + ridge I,   M1 = M0 + A_p
      criterion "D":  1/2 (logdet M1 - logdet M0)        the expected entropy reduction in nats
                "A":  tr(M0^-1) - tr(M1^-1)              the reduction of sum_r var(S[r, p])
                "V":  tr(G M0^-1) - tr(G M1^-1), G = C C^T: the reduction of sum_k var(T_hat[k, p]),
                      the map's variance at the pixel
    one HIP walk (qsc_sgain, include/qsc.h) after the one qsc_sinfo call that forms J.
    Conditional on C the pixels are independent, so the gain of placing the plan at a pixel is
    that pixel's figure alone and the best n distinct sites are the top n: result.best(n).
    A pixel whose J_p + ridge I is not positive definite (no readings yet and ridge = 0) has gain
    +inf, a first look, and is counted in first_look; one whose block is not positive definite
    even with the plan has gain 0 and is counted in degenerate.  As in qmc.confidence, C is
    treated as known.
    entry_gain=True adds the "which bin" companion (K, 1, I, J): for a single extra reading of
    bin k at pixel p, w_k of them, 1/2 log1p(w_k h_exp std_T[k, p]^2), the rank-one case of "D"
    (+inf where std_T is); it materialises K x P values like confidence(map_std=True).
    obs: the Observations; S (R,1,I,J) or (R,P), C (R,K).  Returns DesignResult(gain (1,I,J),
    first_look, degenerate, entry_gain or None).  Raises ValueError for an unknown criterion or
    kind, ridge < 0, negative weights or weights of another shape than (K,), or
    obs.loss == "squared", before any GPU call."""
    w = check_design(criterion, kind, ridge, getattr(obs, "loss", None), weights,
                     getattr(obs, "K", C.shape[-1]))
    R = S.shape[0]
    Cd = _dev(C.detach().to(torch.float32)).reshape(R, obs.K).contiguous()
    S_pos = obs.to_positions(S.detach().to(torch.float32).reshape(R, -1))
    wd = w.to(Cd.device) if w is not None else None
    J = _info_blocks_pos(obs, S_pos, Cd, R, kind)
    gain, counters = _gain_pos(obs, S_pos, Cd, J, R, wd, criterion, ridge)
    eg = None
    if entry_gain:
        Sd = _dev(S.detach().to(torch.float32)).reshape(R, obs.P)
        eg = _entry_gain_pos(obs, Sd, Cd, J, R, wd, ridge).reshape(obs.K, 1, obs.I, obs.J)
    first, bad = counters.tolist()
    return DesignResult(gain=gain[obs.iperm().long()].reshape(1, obs.I, obs.J),
                        first_look=first, degenerate=bad, entry_gain=eg)


CHECK_UNTESTABLE, CHECK_INVALID, CHECK_SATURATED = 1, 2, 4  # QSC_CHECK_* (include/qsc.h)
FLAG_WHICH = ("shift", "fit", "either")


def _z(num, den):
    """num / sqrt(den) where den > 0, else 0: the one rule every z of CheckResult is formed by."""
    ok = den > 0
    return torch.where(ok, num / torch.sqrt(torch.where(ok, den, torch.ones_like(den))),
                       torch.zeros_like(num))


@dataclass
class CheckResult:
    n: torch.Tensor                     # (I, J) int32: readings used at the pixel
    z_fit: torch.Tensor                 # (I, J) D / sqrt(V) (0 where V == 0)
    z_shift: torch.Tensor               # (I, J) -u* / sqrt(I*): positive, the sensor reads high
    shift: torch.Tensor                 # (I, J) -u* / I*: one-step estimate of delta, model domain
    flags: torch.Tensor                 # (I, J) int32: 1 untestable, 2 invalid, 4 saturated
    D: torch.Tensor                     # (I, J) sum (l - H)
    V: torch.Tensor                     # (I, J) sum var
    u: torch.Tensor                     # (I, J) u* (the efficient score with fitted=True)
    info: torch.Tensor                  # (I, J) I*
    untestable: int = 0                 # pixels with flag bit 1
    invalid: int = 0                    # ... bit 2
    saturated: int = 0                  # ... bit 4
    z_fit_total: float = 0.0            # sum D / sqrt(sum V) over the valid pixels

    def testable(self, which="shift"):
        """(I, J) bool: the pixels the `which` test can judge -- never an untestable (shift) or
        invalid one, and only where the statistic's variance is positive."""
        if which not in FLAG_WHICH:
            raise ValueError("which must be one of %s, got %r" % (FLAG_WHICH, which))
        valid = (self.flags & CHECK_INVALID) == 0
        t_shift = valid & ((self.flags & CHECK_UNTESTABLE) == 0) & (self.info > 0)
        t_fit = valid & (self.V > 0)
        return {"shift": t_shift, "fit": t_fit, "either": t_shift | t_fit}[which]

    def flagged(self, alpha=0.01, which="shift", method="bonferroni"):
        """(I, J) bool mask of the pixels whose statistic rejects the model at family-wise level
        alpha: a two-sided normal test, |z| > -ndtri(alpha / (2 m)), m the number of testable
        pixels (Bonferroni).  which="shift" tests z_shift, "fit" z_fit, "either" both at alpha / 2
        each.  Untestable and invalid pixels are never flagged."""
        if method != "bonferroni":
            raise ValueError('method must be "bonferroni", got %r' % (method,))
        if not 0.0 < float(alpha) < 1.0:
            raise ValueError("alpha must be in (0, 1), got %r" % (alpha,))
        if which not in FLAG_WHICH:
            raise ValueError("which must be one of %s, got %r" % (FLAG_WHICH, which))
        if which == "either":
            return (self.flagged(float(alpha) / 2, "shift", method)
                    | self.flagged(float(alpha) / 2, "fit", method))
        ok = self.testable(which)
        m = int(ok.sum())
        if m == 0:
            return torch.zeros_like(ok)
        z = self.z_shift if which == "shift" else self.z_fit
        crit = -torch.special.ndtri(torch.tensor(float(alpha) / (2.0 * m), dtype=torch.float64))
        return ok & (z.double().abs() > crit.to(z.device))


def check_check_fit(loss, ridge):
    """Validate the check_fit arguments (before anything touches a device)."""
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: there is no model to check')
    if not float(ridge) >= 0.0:
        raise ValueError("the check_fit ridge must be >= 0, got %r" % (ridge,))


def _check_pos(obs, S_pos, C, R, fitted, ridge, stat=None, count=None, flags=None):
    """qsc_scheck on a position-order S (Pp, RP) and a device C (R, K): (stat (Pp, 4) = D, V, u*,
    I*, count (Pp,) int32, flags (Pp,) int32), all on the device; nothing is read back."""
    desc, s_entries, _ = obs.layout(R)
    dev = S_pos.device
    if stat is None:
        stat = torch.empty((obs.Pp, 4), dtype=torch.float32, device=dev)
        count = torch.empty(obs.Pp, dtype=torch.int32, device=dev)
        flags = torch.empty(obs.Pp, dtype=torch.int32, device=dev)
    _lib.call("qsc_scheck", desc, _lib.ptr(s_entries), _lib.ptr(obs.s_width), _lib.ptr(obs.s_off),
              _lib.ptr(obs.perm), obs.model, R, _lib.ptr(S_pos), _lib.ptr(C), 1 if fitted else 0,
              float(ridge), _lib.ptr(stat), _lib.ptr(count), _lib.ptr(flags), _lib.stream())
    return stat, count, flags


def check_result(D, V, u, info, n, flags):
    """CheckResult from the four statistics, the counts and the flag words (same-shaped tensors):
    the z's, the one-step shift, the flag counts and the total are formed here and nowhere else."""
    ok = info > 0
    shift = torch.where(ok, -u / torch.where(ok, info, torch.ones_like(info)),
                        torch.zeros_like(u))
    valid = (flags & CHECK_INVALID) == 0
    sD = float((D.double() * valid).sum())
    sV = float((V.double() * valid).sum())
    return CheckResult(
        n=n, z_fit=_z(D, V), z_shift=_z(-u, info), shift=shift, flags=flags, D=D, V=V, u=u,
        info=info, untestable=int(((flags & CHECK_UNTESTABLE) != 0).sum()),
        invalid=int(((flags & CHECK_INVALID) != 0).sum()),
        saturated=int(((flags & CHECK_SATURATED) != 0).sum()),
        z_fit_total=sD / math.sqrt(sV) if sV > 0.0 else 0.0)


def check_fit(obs, S, C, fitted=True, ridge=0.0):
    """Are the readings consistent with the fitted model, and which sensors are not?  Per pixel
    (a pixel of the map is a physical sensor) a goodness-of-fit statistic and a score test for a
    level shift of that sensor alone, from one HIP walk over the packed lists (qsc_scheck;
    include/qsc.h has every formula).

    Per reading, with P_b the model's probability of code b at the map value: l = -log P_y, its
    expectation H = -sum_b P_b log P_b and variance var under the model, the score g_x = -P_y'/P_y
    in the model domain x and its Fisher information h_x.  Per pixel
      D = sum (l - H),  V = sum var:            z_fit = D / sqrt(V); large: the readings are less
                                                likely than the model itself expects
      u = sum g_x,  Ixx = sum h_x:              the score and information of a shift x -> x + delta
                                                of the sensor's received level
    fitted=False takes u* = u, I* = Ixx: exact under the model at the true (S, C) -- D has mean 0
    and variance V, u mean 0 and variance Ixx, for any number of readings.  This is the form for
    held-out readings: after solve_readings(holdout=...),
    check_fit(res.obs_holdout, res.S, res.C, fitted=False) (that packing shares obs.perm).
    fitted=True (default; S was fitted to these readings) removes what the fit of the pixel's own
    s absorbs: u* = u - v^T J^-1 g, I* = Ixx - v^T J^-1 v, with J the expected information block of
    s (qmc.confidence's, plus ridge I), v the cross information and g the S-gradient at S -- Neyman's
    C(alpha) statistic, valid to first order even where S is not exactly the conditional MLE.
    z_shift = -u* / sqrt(I*) (positive: the sensor reads high) and shift = -u* / I* is the
    one-step estimate of delta in model-domain units.  D is NOT corrected for the fit: on the
    fitted readings z_fit is biased low by about R / 2 in D; held-out readings with fitted=False
    give the exact form.  C is treated as known, as in qmc.confidence.  `ridge` is the ridge the
    fit of S carried (solve(check=True) passes default_confidence_ridge).
    flags (bits): 1 untestable -- fitted and J is not positive definite or I* <= 1e-4 Ixx (the
    shift is confounded with s: fewer readings than R, say; u*, I* are 0); 2 invalid -- log model
    and a reading with T_hat + offset <= 0 (all four statistics 0); 4 saturated -- a reading whose
    P underflows (it enters l as -log FLT_MIN and adds 0 to the score).  Nothing is ever NaN.
    Under the log model a shift of x = log(T_hat + offset) is a common gain on the pixel's s but
    for the offset: with fitted=True and ridge = 0 it is confounded with the fit and every pixel is
    untestable; the ridge of the fit, or held-out readings with fitted=False, make the test live.
    Returns CheckResult(n, z_fit, z_shift, shift, flags, D, V, u, info (each (I, J)), untestable,
    invalid, saturated (counts), z_fit_total = sum D / sqrt(sum V) over the valid pixels); its
    .flagged(alpha, which) is the Bonferroni mask.  To re-solve without the flagged sensors:
      keep = ~r.flagged(0.01, "either")
      obs2 = Observations(Y, Wx * keep, ...)      # or filter the readings by keep[i, j] and re-pack
    obs: the Observations; S (R,1,I,J) or (R,P), C (R,K).  Raises ValueError for
    obs.loss == "squared", ridge < 0 or shapes that do not match obs, before any GPU call."""
    check_check_fit(getattr(obs, "loss", None), ridge)
    R = S.shape[0]
    if S.numel() != R * obs.P or tuple(C.shape) != (R, obs.K):
        raise ValueError("check_fit needs S (R,1,I,J) or (R,P) and C (R,K) of obs's shape "
                         "(P = %d, K = %d), got %s and %s"
                         % (obs.P, obs.K, tuple(S.shape), tuple(C.shape)))
    S_pos, Cd = _inputs(obs, S, C, R)
    stat, count, flags = _check_pos(obs, S_pos, Cd, R, bool(fitted), ridge)
    ip = obs.iperm().long()
    st = stat[ip].reshape(obs.I, obs.J, 4)
    return check_result(st[..., 0].contiguous(), st[..., 1].contiguous(), st[..., 2].contiguous(),
                        st[..., 3].contiguous(), count[ip].reshape(obs.I, obs.J),
                        flags[ip].reshape(obs.I, obs.J))


@dataclass
class FitSResult:
    S: Optional[torch.Tensor]           # (R, 1, I, J), pixel order (None in SolveResult.polish)
    nll: float                          # -sum log P at S over the observed entries (no ridge term)
    steps: torch.Tensor                 # (I, J) int32: trial evaluations each pixel used
    unconverged: int                    # pixels not converged within max_steps
    unidentified: int                   # pixels whose J_p + ridge I never had positive pivots


def check_fit_s(loss, ridge, kind, max_steps, tol, mu0):
    """Validate the fit_S arguments (before anything touches a device)."""
    _check_newton("fit_S", loss, kind, ridge, mu0, tol, max_steps)


def _fit_s_pos(obs, S_pos, C, R, kind, ridge, max_steps, tol, mu0, project, S_out=None):
    """qsc_sfit on a position-order S (Pp, RP) and a device C (R, K): (S_out, f (Pp,),
    steps (Pp,) int32, counters (2,) int32: unconverged, unidentified), all on the device."""
    desc, s_entries, _ = obs.layout(R)
    dev = S_pos.device
    if S_out is None:
        S_out = torch.empty_like(S_pos)
    f = torch.empty(obs.Pp, dtype=torch.float32, device=dev)
    steps = torch.empty(obs.Pp, dtype=torch.int32, device=dev)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    nws = int(_lib.lib().qsc_sfit_workspace_bytes(desc, R))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    _lib.call("qsc_sfit", desc, _lib.ptr(s_entries), _lib.ptr(obs.s_width), _lib.ptr(obs.s_off),
              _lib.ptr(obs.perm), obs.model, R, _lib.ptr(C), _lib.ptr(S_pos), INFO_KINDS[kind],
              float(ridge), float(mu0), float(tol), int(max_steps), 1 if project else 0,
              _lib.ptr(S_out), _lib.ptr(f), _lib.ptr(steps), _lib.ptr(counters[0:1]),
              _lib.ptr(counters[1:2]), _lib.ptr(ws), nws, _lib.stream())
    return S_out, f, steps, counters


def fit_S(obs, C, S_init=None, ridge=0.0, kind=None, max_steps=30, tol=1e-5, mu0=1e-3,
          project=None):
    """The loss fields S for known spectra C: per pixel, a damped Newton / Fisher-scoring fit.

    Given C the likelihood separates over pixels; pixel p minimises
      f_p(s) = sum_{k observed at p} -log P(Y[k, p] | s . c_k) + ridge / 2 |s|^2,
    convex under the linear model (both links are log-concave).  One HIP launch (qsc_sfit,
    include/qsc.h has the iteration) evaluates f, its gradient and the R x R curvature block of
    every pixel from the packed lists, solves (J + (ridge + mu) I) delta = g + ridge s in
    registers, accepts the step when f does not increase (else raises the damping mu), and
    repeats until |delta|_inf <= tol (1 + |s|_inf) or max_steps -- a handful of steps where the
    alternating solver's Adam S-step needs hundreds.  The point it returns is the conditional MLE
    (MAP with the ridge) that qmc.confidence's standard deviations are defined at.
    obs: the Observations; C (R, K) from an earlier solve, spa / gram.nnls_spectra or a
    catalogue.  S_init (R,1,I,J) or (R,P): default zeros (linear model) or ones (log model).
    kind "observed" (Newton; default for the linear model) or "expected" (Fisher scoring, always
    positive semidefinite; default for the log model, whose observed Hessian may be indefinite).
    project: keep S >= 0 (default: obs.log_model, as solve's project_s).  mu0: initial damping
    (0: pure Newton steps while they are accepted).
    Returns FitSResult(S (R,1,I,J), nll, steps (I,J), unconverged, unidentified): nll is the NLL
    at S without the ridge term, summed in fp64 in a fixed order; unidentified counts pixels
    whose J_p + ridge I never had all pivots positive (no observations and ridge = 0: such a
    pixel keeps S_init).  Raises ValueError for loss="squared", negative ridge / mu0, tol <= 0,
    max_steps < 1 or an unknown kind, before any GPU call."""
    check_fit_s(getattr(obs, "loss", None), ridge, kind, max_steps, tol, mu0)
    kind, project = _defaults(obs, kind, project)
    R = C.shape[0]
    S_pos, Cd = _inputs(obs, _start(obs, S_init, R, obs.P), C, R)
    S_out, f, steps, counters = _fit_s_pos(obs, S_pos, Cd, R, kind, ridge, max_steps, tol, mu0,
                                           project)
    nll = float(f.double().sum() - 0.5 * float(ridge) * (S_out.double() ** 2).sum())
    unconverged, unidentified = counters.tolist()
    return FitSResult(S=obs.to_pixels(S_out, R).reshape(R, 1, obs.I, obs.J), nll=nll,
                      steps=steps[obs.iperm().long()].reshape(obs.I, obs.J),
                      unconverged=unconverged, unidentified=unidentified)


@dataclass
class FitCResult:
    C: Optional[torch.Tensor]           # (R, K) (None in SolveResult.polish_c)
    nll: float                          # -sum log P at C over the observed entries (no ridge term)
    steps: torch.Tensor                 # (K,) int32: trial evaluations each bin used
    unconverged: int                    # bins not converged within max_steps
    unidentified: int                   # bins whose J_k + ridge I never had positive pivots
    std_C: Optional[torch.Tensor] = None  # (R, K) sqrt(diag((J_k + ridge I)^-1)) (std=True)


def check_fit_c(loss, ridge, kind, max_steps, tol, mu0):
    """Validate the fit_C arguments (before anything touches a device)."""
    _check_newton("fit_C", loss, kind, ridge, mu0, tol, max_steps)


def _fit_c_pos(obs, S_pos, C_init, R, kind, ridge, max_steps, tol, mu0, project, std=False,
               sync_every=4, C_out=None, ws=None):
    """qsc_cfit_begin / _iterate / _finish on a position-order S (Pp, RP) and a device C_init
    (R, K): (C_out, f (K,) fp64, steps (K,) int32, counters (2,) int32: unconverged,
    unidentified, std_C or None), all on the device.  With sync_every = 0 nothing is read back
    (the sequence can be captured into a hipGraph)."""
    desc, _, c_entries = obs.layout(R)
    dev = S_pos.device
    K = obs.K
    if C_out is None:
        C_out = torch.empty((R, K), dtype=torch.float32, device=dev)
    f = torch.empty(K, dtype=torch.float64, device=dev)
    steps = torch.empty(K, dtype=torch.int32, device=dev)
    std_C = torch.empty((R, K), dtype=torch.float32, device=dev) if std else None
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    nws = int(_lib.lib().qsc_cfit_workspace_bytes(desc, R))
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    lists = (desc, _lib.ptr(c_entries), _lib.ptr(obs.c_width), _lib.ptr(obs.c_off),
             _lib.ptr(obs.c_kmap), obs.model, R, _lib.ptr(S_pos))
    _lib.call("qsc_cfit_begin", *lists, _lib.ptr(C_init), INFO_KINDS[kind], float(ridge),
              float(mu0), float(tol), int(max_steps), 1 if project else 0, _lib.ptr(ws), nws,
              _lib.stream())
    o = int(_lib.lib().qsc_cfit_active_offset())
    active = ws[o:o + 4].view(torch.int32)
    _iterate(lambda: _lib.call("qsc_cfit_iterate", *lists, INFO_KINDS[kind], _lib.ptr(ws), nws,
                               _lib.stream()),
             int(max_steps), sync_every, active.item)
    _lib.call("qsc_cfit_finish", desc, obs.model, R, _lib.ptr(C_out), _lib.ptr(f), _lib.ptr(steps),
              _lib.ptr(std_C), _lib.ptr(counters[0:1]), _lib.ptr(counters[1:2]), _lib.ptr(ws), nws,
              _lib.stream())
    return C_out, f, steps, counters, std_C


def fit_C(obs, S, C_init=None, ridge=0.0, kind=None, max_steps=30, tol=1e-5, mu0=1e-3,
          project=True, std=False, sync_every=4):
    """The spectra C for known loss fields S: per frequency bin, a projected damped Newton /
    Fisher-scoring fit of the quantized likelihood -- the mirror image of fit_S.

    Given S the likelihood separates over bins; bin k minimises over c = C[:, k]
      f_k(c) = sum_{p observed in bin k} -log P(Y[k, p] | S[:, p] . c) + ridge / 2 |c|^2,
    R unknowns informed by every observed pixel of the bin.  A HIP walk over the packed
    C-format lists (qsc_cfit.hip, include/qsc.h has the iteration) evaluates f, its gradient and
    the R x R curvature block of every bin at a trial C; a second kernel accepts the trial when
    f does not increase (else raises the damping mu), solves (J + (ridge + mu) I) delta =
    g + ridge c on the entries that are not held at the bound, and proposes the next trial, until
    |delta|_inf <= tol (1 + |c|_inf) or max_steps.  project=True (default: C >= 0 is the
    solver's standing constraint) makes it a two-metric projected Newton method: entries at 0
    whose gradient points outwards are held, the rest take the Newton step and are clipped.
    obs: the Observations; S (R,1,I,J) or (R,P) from a propagation model, a survey or an earlier
    solve.  C_init (R,K): default zeros (linear model) or ones (log model).  kind "observed"
    (default for the linear model) or "expected" (default for the log model).  std=True also
    returns std_C = sqrt(diag((J_k + ridge I)^-1)) at the result (the bound ignored; +inf for a
    bin whose block is not positive definite).  sync_every: every so many steps the count of
    active bins is read back and the loop stops at 0 (0: never; the result is the same bits).
    Returns FitCResult(C (R,K), nll, steps (K,), unconverged, unidentified, std_C or None): nll is
    the NLL at C without the ridge term (fp64 sums in a fixed order); unidentified counts bins
    whose J_k + ridge I never had all pivots positive (no observations and ridge = 0: such a bin
    keeps C_init).  Raises ValueError for loss="squared", negative ridge / mu0, tol <= 0,
    max_steps < 1 or an unknown kind, before any GPU call."""
    check_fit_c(getattr(obs, "loss", None), ridge, kind, max_steps, tol, mu0)
    kind, project = _defaults(obs, kind, project)
    R = S.shape[0]
    S_pos, Cd = _inputs(obs, S, _start(obs, C_init, R, obs.K), R)
    C_out, f, steps, counters, std_C = _fit_c_pos(obs, S_pos, Cd, R, kind, ridge, max_steps, tol,
                                                  mu0, project, std=std, sync_every=sync_every)
    nll = float(f.sum() - 0.5 * float(ridge) * (C_out.double() ** 2).sum())
    unconverged, unidentified = counters.tolist()
    return FitCResult(C=C_out, nll=nll, steps=steps, unconverged=unconverged,
                      unidentified=unidentified, std_C=std_C)


@dataclass
class FitNoiseResult:
    noise_std: float                    # sigma0 e^tau (for loss="logit" the logistic scale)
    shift: float                        # beta, the common shift of the interior edges
    bin_boundaries: List[float]         # the shifted list (Observations.with_model takes it)
    nll: float                          # -sum log P at the result, without the prior terms
    nll_start: float                    # ... at the start
    std_log_scale: Optional[float]      # sqrt(cov[tau, tau]); None where the scale is not fitted
    std_shift: Optional[float]          # sqrt(cov[beta, beta]); None where the shift is not fitted
    corr: Optional[float]               # their correlation; None unless both are fitted
    steps: int                          # trial evaluations used
    converged: bool
    unidentified: bool                  # H + prior never had positive pivots on the fitted set


FIT_PARAMS = {"scale": 1, "shift": 2}  # QSC_QFIT_SCALE, QSC_QFIT_SHIFT


def check_fit_noise(loss, fit, kind, prior, start, max_steps, tol, mu0):
    """Validate the fit_noise arguments (before anything touches a device); the fit mask."""
    _check_newton("fit_noise", loss, kind, None, mu0, tol, max_steps, kind_optional=False)
    fit = (fit,) if isinstance(fit, str) else tuple(fit)
    if not fit or any(p not in FIT_PARAMS for p in fit):
        raise ValueError("fit must name one or both of %s, got %r" % (sorted(FIT_PARAMS), fit))
    for name, pair in (("prior", prior), ("start", start)):
        try:
            ok = len(pair) == 2 and all(math.isfinite(float(x)) for x in pair)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError("%s must be two finite numbers (scale, shift), got %r" % (name, pair))
    if any(float(x) < 0.0 for x in prior):
        raise ValueError("the fit_noise prior weights must be >= 0, got %r" % (prior,))
    mask = 0
    for p in fit:
        mask |= FIT_PARAMS[p]
    return mask


def shifted_boundaries(bin_boundaries, shift, log_model):
    """The boundary list with every interior edge (linear model: all but the first and last, which
    the likelihood clamps) or every finite edge (log model) moved by `shift`: the edges qsc_qfit
    evaluates, fp64 sums of the fp32 boundaries."""
    b = torch.as_tensor(bin_boundaries, dtype=torch.float32).double()
    moved = torch.isfinite(b) if log_model else torch.ones_like(b, dtype=torch.bool)
    if not log_model:
        moved[0] = moved[-1] = False
    return torch.where(moved, b + float(shift), b).tolist()


def _fit_noise_pos(obs, S_pos, C, R, kind, mask, prior, start, max_steps, tol, mu0, sync_every=4,
                   iterate=True):
    """qsc_qfit_begin / _iterate / _finish on a position-order S (Pp, RP) and a device C (R, K):
    device tensors theta (2,), f (2,: F at the result and at the start, priors included),
    cov (3,), gh (5,: g, H), all fp64, and info (2,) int32: steps, flags.  With sync_every = 0
    nothing is read back (the sequence can be captured into a hipGraph)."""
    desc, s_entries, _ = obs.layout(R)
    dev = S_pos.device
    out = torch.empty(12, dtype=torch.float64, device=dev)
    theta, f, cov, gh = out[0:2], out[2:4], out[4:7], out[7:12]
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    nws = int(_lib.lib().qsc_qfit_workspace_bytes(desc, R))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    lists = (desc, _lib.ptr(s_entries), _lib.ptr(obs.s_width), _lib.ptr(obs.s_off), obs.model, R,
             _lib.ptr(S_pos), _lib.ptr(C), INFO_KINDS[kind])
    _lib.call("qsc_qfit_begin", *lists, int(mask), float(prior[0]), float(prior[1]),
              float(start[0]), float(start[1]), float(mu0), float(tol), int(max_steps),
              _lib.ptr(ws), nws, _lib.stream())
    o = int(_lib.lib().qsc_qfit_active_offset())
    active = ws[o:o + 4].view(torch.int32)
    _iterate(lambda: _lib.call("qsc_qfit_iterate", *lists, _lib.ptr(ws), nws, _lib.stream()),
             int(max_steps) if iterate else 0, sync_every, active.item)
    _lib.call("qsc_qfit_finish", desc, obs.model, R, _lib.ptr(theta), _lib.ptr(f), _lib.ptr(cov),
              _lib.ptr(gh), _lib.ptr(info[0:1]), _lib.ptr(info[1:2]), _lib.ptr(ws), nws,
              _lib.stream())
    return theta, f, cov, gh, info


def fit_noise(obs, S, C, fit=("scale", "shift"), kind="expected", prior=(0.0, 0.0),
              start=(0.0, 0.0), max_steps=30, tol=1e-6, mu0=1e-3, sync_every=4):
    """Calibrate the quantiser from the readings themselves: the noise scale and a common shift
    of the levels, for known S and C -- the one block of the likelihood's parameters the other
    fits take as given.

    Two parameters: sigma = obs.noise_std * exp(tau) (for loss="logit" the logistic scale) and a
    shift beta added to every interior edge of obs.bin_boundaries (the two outer edges of the
    linear model, which the likelihood clamps, stay; under the log model every finite edge moves,
    a common gain).  With the map T_hat = S, C fixed they minimise
      F(tau, beta) = -sum log P(Y | T_hat; sigma, edges + beta)
                     + prior[0] / 2 tau^2 + prior[1] / 2 beta^2
    by damped Newton steps on a 2 x 2 system: a HIP walk over the packed S-format lists
    (qsc_qfit.hip, include/qsc.h has the derivatives and the iteration) sums F, its gradient and
    curvature at a trial point in a fixed order, one workgroup accepts the trial when F does not
    increase (else raises the damping mu), solves and proposes the next, until
    |delta|_inf <= tol (1 + |theta|_inf) or max_steps.  The whole fit is stream-ordered; every
    sync_every steps one flag is read back to stop early (0: never; the result is the same bits).
    obs: the Observations; S (R,1,I,J) or (R,P) and C (R,K) from a solve or the other fits.
    fit: ("scale", "shift"), ("scale",) or ("shift",): the other parameter stays at `start`.
    kind "expected" (Fisher scoring, the default for both models: positive semidefinite) or
    "observed" (Newton).  prior: the weights of the quadratic priors on (tau, beta); start: where
    the iteration begins, (0, 0) being obs's own model.
    Returns FitNoiseResult(noise_std, shift, bin_boundaries (the shifted list), nll, nll_start
    (both without the prior terms), std_log_scale, std_shift, corr, steps, converged,
    unidentified); hand the model on with obs.with_model(r.noise_std, r.bin_boundaries).
    The standard errors come from the inverse of the accepted curvature plus the prior and are
    conditional on S and C: as qmc.confidence treats C as known, they leave out the uncertainty
    of the map itself and are lower bounds on the joint one; they are +inf where the curvature is
    not positive definite.  unidentified: the data do not determine the fitted parameters (every
    term saturated and no prior, say); the result is then `start`.
    Raises ValueError for loss="squared", an empty or unknown `fit`, an unknown kind, negative
    prior weights or mu0, tol <= 0 or max_steps < 1, before any GPU call."""
    mask = check_fit_noise(getattr(obs, "loss", None), fit, kind, prior, start, max_steps, tol,
                           mu0)
    R = S.shape[0]
    S_pos, Cd = _inputs(obs, S, C, R)
    theta, f, cov, _, info = _fit_noise_pos(obs, S_pos, Cd, R, kind, mask, prior, start,
                                            max_steps, tol, mu0, sync_every)
    (tau, beta), (F, F0), (ctt, ctb, cbb) = theta.tolist(), f.tolist(), cov.tolist()
    steps, flags = info.tolist()
    pen = lambda t, b: 0.5 * float(prior[0]) * t * t + 0.5 * float(prior[1]) * b * b
    has_s, has_b = bool(mask & 1), bool(mask & 2)
    corr = None
    if has_s and has_b:
        corr = ctb / math.sqrt(ctt * cbb) if math.isfinite(ctt) and math.isfinite(cbb) else 0.0
    return FitNoiseResult(
        noise_std=obs.noise_std * math.exp(tau), shift=beta,
        bin_boundaries=shifted_boundaries(obs.bin_boundaries, beta, obs.log_model),
        nll=F - pen(tau, beta), nll_start=F0 - pen(float(start[0]), float(start[1])),
        std_log_scale=math.sqrt(ctt) if has_s else None,
        std_shift=math.sqrt(cbb) if has_b else None, corr=corr, steps=steps,
        converged=not flags & 1, unidentified=bool(flags & 2))


def model_nll(obs, S, C):
    """-sum log P(Y | T_hat(S, C)) over the packed entries under obs's own model: the walk of
    fit_noise at its start (qsc_qfit_begin, settled by qsc_qfit_finish with no step between),
    fp64 sums in a fixed order."""
    check_fit_noise(getattr(obs, "loss", None), ("scale",), "expected", (0.0, 0.0), (0.0, 0.0), 1,
                    1e-6, 0.0)
    R = S.shape[0]
    S_pos, Cd = _inputs(obs, S, C, R)
    # (the observed kind: f is the same and its walk does not loop over the bins)
    _, f, _, _, _ = _fit_noise_pos(obs, S_pos, Cd, R, "observed", 1, (0.0, 0.0), (0.0, 0.0), 1,
                                   1e-6, 0.0, iterate=False)
    return float(f[1])


@dataclass
class CrossValidateResult:
    nll: List[float]        # per fold: model_nll(test, S, C) / test.nnz at the fit on train
    mean: float             # their mean
    stderr: float           # standard error of the mean over the folds
    n_test: List[int]       # readings of every test part
    n_train: List[int]      # readings of every train part


def check_cross_validate(loss, fit, folds=5, seed=0):
    """Host-side checks of cross_validate's arguments, before any device call.  -> None."""
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: there is no held-out NLL to score')
    if not callable(fit):
        raise ValueError("fit must be a callable: train Observations -> (S, C)")
    Observations.check_split(seed=seed, n=0 if folds is None else folds)


def cross_validate(obs, fit, folds=5, seed=0):
    """K-fold cross-validation of any fitting recipe by held-out likelihood.  obs.folds(folds,
    seed) splits the packed readings on the device (every reading is in exactly one test part);
    for each fold S, C = fit(train) -- any callable that returns (S, C) or an object with .S and
    .C -- and the score is model_nll(test, S, C) / test.nnz, the held-out NLL per reading.
    -> CrossValidateResult (per-fold scores, their mean, the standard error over folds, sizes).
    The intended uses, a grid over the smoothness weight and over the rank:
        for w in (0.0, 0.1, 1.0):
            cv[w] = cross_validate(obs, lambda tr: solve(None, None, b, sigma, R=R, obs=tr,
                                                         smooth=w, max_iter=200))
        for R in (2, 3, 4):
            cv[R] = cross_validate(obs, lambda tr: solve(None, None, b, sigma, R=R, obs=tr))
    and the one with the smallest mean wins (differences inside stderr are ties; the folds share
    a seed, so two recipes are scored on the same parts and may be compared fold by fold).
    Raises ValueError for loss="squared" (no likelihood), folds outside [2, 65536] or a seed out
    of range, before any device call, and when a part is empty."""
    check_cross_validate(getattr(obs, "loss", None), fit, folds, seed)
    nll, n_test, n_train = [], [], []
    for train, test in obs.folds(folds, seed):
        out = fit(train)
        S, C = (out.S, out.C) if hasattr(out, "S") and hasattr(out, "C") else out
        nll.append(model_nll(test, S, C) / test.nnz)
        n_test.append(test.nnz)
        n_train.append(train.nnz)
    mean = sum(nll) / len(nll)
    var = sum((v - mean) ** 2 for v in nll) / (len(nll) - 1)
    return CrossValidateResult(nll=nll, mean=mean, stderr=math.sqrt(var / len(nll)),
                               n_test=n_test, n_train=n_train)


@dataclass
class CalibrateResult:
    S: Optional[torch.Tensor]           # (R, 1, I, J) (None in SolveResult.calibration)
    C: Optional[torch.Tensor]           # (R, K) (None in SolveResult.calibration)
    obs: Observations                   # the observations under the calibrated model
    noise_std: float
    shift: float
    # per round the objective NLL + ridges after each block: (fit_noise, fit_C, fit_S)
    objective: List[tuple] = field(default_factory=list)
    fits: List[FitNoiseResult] = field(default_factory=list)


def check_calibrate(rounds, loss, ridge_s, ridge_c):
    """Validate the calibrate arguments (before anything touches a device); the round count."""
    n = int(rounds)
    if n < 1:
        raise ValueError("rounds must be >= 1, got %r" % (rounds,))
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: there is nothing to calibrate')
    if not float(ridge_s) >= 0.0 or not float(ridge_c) >= 0.0:
        raise ValueError("the calibrate ridges must be >= 0, got %r, %r" % (ridge_s, ridge_c))
    return n


def calibrate(obs, S, C, rounds=2, ridge_s=0.0, ridge_c=0.0, fit=("scale", "shift"),
              max_steps=30, project_s=None):
    """Joint calibration by block-coordinate descent on NLL + ridge_s / 2 |S|^2 + ridge_c / 2 |C|^2
    over (noise scale and shift), C and S.  Per round: fit_noise at the current S, C; the model is
    handed on with Observations.with_model; fit_C at the current S; fit_S at the new C -- each a
    conditional minimisation started from the current point, so the objective does not increase
    from block to block.  Thin Python over the three fits; every argument is theirs.
    The scale of the map and the noise scale are only jointly determined through the edges: with
    a single threshold at 0 (or none) a common factor of T_hat and sigma leaves the likelihood
    unchanged, and the ridges alone then pick the scale.
    Returns CalibrateResult(S, C, obs (under the calibrated model; the packed arrays are shared
    with the argument), noise_std, shift (the total, relative to the argument's boundaries),
    objective (per round the three values after fit_noise, fit_C, fit_S), fits)."""
    n = check_calibrate(rounds, getattr(obs, "loss", None), ridge_s, ridge_c)
    check_fit_noise(obs.loss, fit, "expected", (0.0, 0.0), (0.0, 0.0), max_steps, 1e-6, 1e-3)
    R = S.shape[0]
    S = _dev(S.detach().to(torch.float32)).reshape(R, 1, obs.I, obs.J)
    C = _dev(C.detach().to(torch.float32)).reshape(R, obs.K)
    pen = lambda: (0.5 * float(ridge_s) * float((S.double() ** 2).sum())
                   + 0.5 * float(ridge_c) * float((C.double() ** 2).sum()))
    out = CalibrateResult(S=None, C=None, obs=obs, noise_std=obs.noise_std, shift=0.0)
    for _ in range(n):
        q = fit_noise(obs, S, C, fit=fit, max_steps=max_steps)
        obs = obs.with_model(q.noise_std, q.bin_boundaries)
        out.shift += q.shift
        o1 = q.nll + pen()
        c = fit_C(obs, S, C_init=C, ridge=ridge_c, max_steps=max_steps)
        C = c.C
        o2 = c.nll + pen()
        s = fit_S(obs, C, S_init=S, ridge=ridge_s, max_steps=max_steps, project=project_s)
        S = s.S
        # (fit_S reports every pixel's f rounded to fp32; the walk of fit_noise sums the same
        # terms in fp64, so the three values of a round compare to summation order)
        out.objective.append((o1, o2, model_nll(obs, S, C) + pen()))
        out.fits.append(q)
    out.S, out.C, out.obs, out.noise_std = S, C, obs, obs.noise_std
    return out


@dataclass
class AcquireRound:
    sites: torch.Tensor     # (sites, 2) int64 rows (i, j), CPU: the pixels chosen, best first
    gain: torch.Tensor      # (sites,) fp32, CPU: their predicted gains (+inf: a first look)
    added: int              # readings appended in the round


@dataclass
class AcquireResult:
    obs: Observations       # the observations after the last round
    S: torch.Tensor         # the loss fields after the last refit (the input where refit=())
    C: torch.Tensor         # the spectra likewise
    rounds: List[AcquireRound]


ACQUIRE_REFIT = ("S", "C")


def check_acquire(loss, measure, rounds, sites, weights, K, criterion="D", kind="expected",
                  ridge=0.0, refit=("S",), generator=None, P=None):
    """Validate acquire's arguments (before anything touches a device): a likelihood and a free S
    (no generator), a callable `measure`, rounds >= 1, 1 <= sites (<= P where given), check_design's
    rules with whole numbers of readings as weights, refit a subset of ("S", "C").
    -> (the plan as an int64 CPU tensor (K,), refit as a tuple).  Raises ValueError."""
    if generator is not None:
        raise ValueError("acquire applies to free S only: with a generator S is not a free "
                         "parameter")
    w = check_design(criterion, kind, ridge, loss, weights, K)
    if not callable(measure):
        raise ValueError("measure must be a callable: (k, i, j, obs) -> codes")
    if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 1:
        raise ValueError("rounds must be an int >= 1, got %r" % (rounds,))
    if isinstance(sites, bool) or not isinstance(sites, int) or sites < 1 or \
            (P is not None and sites > int(P)):
        raise ValueError("sites must be an int in [1, number of pixels], got %r" % (sites,))
    refit = (refit,) if isinstance(refit, str) else tuple(refit)
    if any(b not in ACQUIRE_REFIT for b in refit):
        raise ValueError("refit may name %s, got %r" % (list(ACQUIRE_REFIT), refit))
    if w is None:
        w = torch.ones(int(K), dtype=torch.float32)
    if not bool((w == w.round()).all()) or float(w.sum()) < 1.0:
        raise ValueError("acquire plans whole readings: the weights must be whole numbers with "
                         "at least one reading")
    return w.to(torch.int64), refit


def acquire(obs, S, C, measure, rounds, sites, weights=None, criterion="D", kind="expected",
            ridge=0.0, refit=("S",), ridge_s=0.0, ridge_c=0.0, max_steps=30, generator=None):
    """Sequential sensing: design -> measure -> append -> refit, `rounds` times.

    Each round runs design(obs, S, C, weights, criterion, kind, ridge), takes result.best(sites)
    (first looks, gain +inf, come first), plans weights[k] readings of bin k at each chosen pixel
    (default: one of every bin), asks code = measure(k, i, j, obs) for them (int64 lists on obs.device,
    site by site in the order chosen, bins ascending; -> an integer tensor of codes), appends them
    (obs.append: a list parent is merged, not re-sorted) and refits: fit_S(obs, C, S_init=S,
    ridge=ridge_s) where "S" is in refit, then fit_C(obs, S, C_init=C, ridge=ridge_c) where "C" is.
    refit=() leaves S and C as given.  acquire.simulate(S_true, C_true, seed) is a `measure` that
    draws the readings from a truth (obs.draw: the data do not depend on how the acquisition is
    cut into rounds).  The input obs is left untouched.
    -> AcquireResult(obs, S, C, rounds: per round the sites, their predicted gains and the number
    of readings added).  Raises ValueError for loss="squared", a generator, or arguments out of
    range, before any device call."""
    w, refit = check_acquire(getattr(obs, "loss", None), measure, rounds, sites, weights,
                             getattr(obs, "K", C.shape[-1]), criterion, kind, ridge, refit,
                             generator, getattr(obs, "P", None))
    plan = torch.repeat_interleave(torch.arange(w.numel()), w)  # one site's bins, ascending
    wf = w.to(torch.float32)
    log = []
    for _ in range(rounds):
        d = design(obs, S, C, weights=wf, criterion=criterion, kind=kind, ridge=ridge)
        ij = d.best(sites).to(obs.device)
        gain = d.gain.reshape(-1)[ij[:, 0] * obs.J + ij[:, 1]]
        k = plan.to(obs.device).repeat(sites)
        i = ij[:, 0].repeat_interleave(plan.numel())
        j = ij[:, 1].repeat_interleave(plan.numel())
        obs = obs.append(k, i, j, measure(k, i, j, obs))
        if "S" in refit:
            S = fit_S(obs, C, S_init=S, ridge=ridge_s, max_steps=max_steps).S
        if "C" in refit:
            C = fit_C(obs, S, C_init=C, ridge=ridge_c, max_steps=max_steps).C
        log.append(AcquireRound(sites=ij.cpu(), gain=gain.cpu(), added=int(k.numel())))
    return AcquireResult(obs=obs, S=S, C=C, rounds=log)


def _simulate(S_true, C_true, seed=0, replicate=0):
    """A `measure` for acquire that draws every planned reading from the model of the
    observations at the truth (S_true, C_true): obs.draw with the given seed and replicate."""
    def measure(k, i, j, obs):
        return obs.draw(k, i, j, S_true, C_true, seed=seed, replicate=replicate)
    return measure


acquire.simulate = _simulate


@dataclass
class BootstrapResult:
    std_S: torch.Tensor                 # (R, 1, I, J) spread of the refitted S over the replicates
    std_C: torch.Tensor                 # (R, K)       ... of the refitted C
    mean_S: torch.Tensor                # (R, 1, I, J) their means (mean - start: the fit's bias)
    mean_C: torch.Tensor                # (R, K)
    std_map: Optional[torch.Tensor]     # (K, 1, I, J) spread of T_hat, gauge free (map_std=True)
    nll: torch.Tensor                   # (n,) fp64, CPU: every replicate's NLL at its refitted point
    nll_observed: float                 # the NLL of obs at the point the same recipe gives on obs
    p_fit: float                        # (1 + #{nll_b >= nll_observed}) / (n + 1)
    n: int
    invalid: int                        # readings left undrawn (log model, T_hat + offset <= 0)


BOOT_REFIT = ("C", "S")


def check_bootstrap(n, refit, rounds, ridge_s, ridge_c, max_steps, loss):
    """Validate the bootstrap arguments (before anything touches a device).
    -> (n, refit as a tuple, rounds)."""
    if loss == "squared":
        raise ValueError('loss="squared" is not a likelihood: there is nothing to draw from')
    if int(n) < 2:
        raise ValueError("a spread needs n >= 2 replicates, got %r" % (n,))
    refit = (refit,) if isinstance(refit, str) else tuple(refit)
    if not refit or any(b not in BOOT_REFIT for b in refit):
        raise ValueError("refit must name one or both of %s, got %r" % (list(BOOT_REFIT), refit))
    if int(rounds) < 1:
        raise ValueError("rounds must be >= 1, got %r" % (rounds,))
    if not float(ridge_s) >= 0.0 or not float(ridge_c) >= 0.0:
        raise ValueError("the bootstrap ridges must be >= 0, got %r, %r" % (ridge_s, ridge_c))
    if int(max_steps) < 1:
        raise ValueError("max_steps must be >= 1, got %r" % (max_steps,))
    return int(n), refit, int(rounds)


class Welford:
    """Running mean and sum of squared deviations (M2) of equally shaped tensors, in fp64 on the
    tensors' device: add(x) per sample; mean, and std() = sqrt(M2 / (count - 1)), the sample
    standard deviation (the bootstrap's standard error).  No sample is kept."""

    def __init__(self):
        self.count, self.mean, self.m2 = 0, None, None

    def add(self, x):
        x = x.detach().double()
        if self.mean is None:
            self.mean, self.m2 = torch.zeros_like(x), torch.zeros_like(x)
        self.count += 1
        d = x - self.mean
        self.mean += d / self.count
        self.m2 += d * (x - self.mean)

    def std(self):
        return (self.m2 / (self.count - 1)).sqrt()


def scale_gauge(S, C, norms):
    """(S, C) (R, P), (R, K) rescaled per component so that |c_r|_2 = norms[r] (s_r inversely):
    the map S^T C is unchanged.  A component whose c_r is 0 is left as it is."""
    cur = torch.linalg.vector_norm(C.double(), dim=1)
    a = torch.where(cur > 0, norms.double() / cur, torch.ones_like(cur))
    a = torch.where(a > 0, a, torch.ones_like(a))
    return ((S.double() / a[:, None]).to(S.dtype), (C.double() * a[:, None]).to(C.dtype))


def _refit_pos(obs, S_pos, C, R, refit, rounds, ridge_s, ridge_c, max_steps, project_s):
    """The bootstrap's refit recipe on a position-order S (Pp, RP) and a device C (R, K): `rounds`
    times fit_C then fit_S (those of `refit`), calibrate's own calls, each from the current point;
    then the NLL there (model_nll's walk).  -> (S_pos, C, nll (1,) fp64), all on the device:
    nothing is read back (fit_C runs with sync_every = 0)."""
    kind_s, project_s = _defaults(obs, None, project_s)
    kind_c, _ = _defaults(obs, None, True)
    for _ in range(rounds):
        if "C" in refit:
            C = _fit_c_pos(obs, S_pos, C, R, kind_c, ridge_c, max_steps, 1e-5, 1e-3, True,
                           sync_every=0)[0]
        if "S" in refit:
            S_pos = _fit_s_pos(obs, S_pos, C, R, kind_s, ridge_s, max_steps, 1e-5, 1e-3,
                               project_s)[0]
    f = _fit_noise_pos(obs, S_pos, C, R, "observed", 1, (0.0, 0.0), (0.0, 0.0), 1, 1e-6, 0.0,
                       sync_every=0, iterate=False)[1]
    return S_pos, C, f[1:2]


def bootstrap(obs, S, C, n=32, seed=0, refit=("C", "S"), rounds=1, ridge_s=0.0, ridge_c=0.0,
              max_steps=30, project_s=None, map_std=False):
    """Parametric bootstrap of the fit at (S, C): the joint uncertainty of S and C, and whether
    the whole fit is consistent with its data.

    confidence, fit_C's std_C and check_fit are conditional on the other factor and bound the joint
    uncertainty from below; model_nll is one number without a scale.  Here n replicates of the
    readings are drawn from the fitted model over the same sampling pattern
    (obs.resample(S, C, seed, b), b = 0 .. n - 1: the very P_b the likelihood evaluates, at the
    observed cells only), and every replicate is refitted by the recipe
        `rounds` times from (S, C):  fit_C(C_init=...) if "C" in refit, then fit_S(S_init=...) if
        "S" in refit
    -- calibrate's own calls, with ridge_c, ridge_s, max_steps and project_s meaning what they
    mean there.  The same recipe runs once on obs itself for nll_observed.  The NLLs are model_nll
    of the refitted points, and p_fit = (1 + #{nll_b >= nll_observed}) / (n + 1): small when the
    data are less likely than data from the model are (1 / (n + 1) is the smallest value).
    The spread is accumulated by Welford's update in fp64 on the device (sample standard deviation
    over the n replicates); one replicate's Observations is held at a time, and the host waits
    once per replicate, to read its NLL.  The model sees only S^T C, so before a replicate enters
    the sums its scale gauge is fixed: each component is rescaled so that |c_r|_2 equals the
    start's (s_r inversely; the reference's ColumnNormalization idea).  The refit starts inside
    the start's basin, so components are not re-matched by permutation.  std_map, the spread of
    T_hat itself, needs no gauge; it is the only K x P output and is opt-in (map_std=True).
    With refit=("S",) and ridge_s = 0, std_S estimates what confidence(kind="expected").std_S
    bounds.  Not done here: refitting the quantiser (fit_noise), the Adam solver as the refit,
    the generator / DIP modes, sharded solvers.
    obs: the Observations; S (R,1,I,J) or (R,I,J), C (R,K).  Returns BootstrapResult(std_S, std_C,
    mean_S, mean_C, std_map, nll (n,), nll_observed, p_fit, n, invalid).  Raises ValueError for
    n < 2, an empty refit or an unknown name in it, rounds < 1, negative ridges, max_steps < 1,
    obs.loss == "squared" or shapes that do not match obs, before any GPU call."""
    n, refit, rounds = check_bootstrap(n, refit, rounds, ridge_s, ridge_c, max_steps,
                                       getattr(obs, "loss", None))
    R, _ = Observations.check_resample(obs.loss, obs.K, obs.I, obs.J, S, C, seed, 0)
    S0 = _dev(S.detach().to(torch.float32)).reshape(R, obs.P).contiguous()
    S_pos0, C0 = _inputs(obs, S0, C, R)
    norms = torch.linalg.vector_norm(C0.double(), dim=1)
    recipe = (R, refit, rounds, ridge_s, ridge_c, max_steps, project_s)
    nll_observed = float(_refit_pos(obs, S_pos0, C0, *recipe)[2])
    acc_s, acc_c, acc_t = Welford(), Welford(), Welford()
    nll = torch.empty(n, dtype=torch.float64)
    invalid = torch.zeros(1, dtype=torch.int32, device=S_pos0.device)
    for b in range(n):
        rep = obs.resample(S0, C0, seed, b)
        S_pos, Cb, f = _refit_pos(rep, S_pos0, C0, *recipe)
        invalid += rep.invalid
        Sb, Cb = scale_gauge(obs.to_pixels(S_pos, R), Cb, norms)
        acc_s.add(Sb)
        acc_c.add(Cb)
        if map_std:
            from ._model import get_tensor
            acc_t.add(get_tensor(Sb.reshape(R, 1, obs.I, obs.J), Cb))
        nll[b] = float(f)  # the one wait of this replicate
        del rep
    shape_s = (R, 1, obs.I, obs.J)
    return BootstrapResult(
        std_S=acc_s.std().float().reshape(shape_s), std_C=acc_c.std().float(),
        mean_S=acc_s.mean.float().reshape(shape_s), mean_C=acc_c.mean.float(),
        std_map=acc_t.std().float().reshape(obs.K, 1, obs.I, obs.J) if map_std else None,
        nll=nll, nll_observed=nll_observed,
        p_fit=(1 + int((nll >= nll_observed).sum())) / (n + 1), n=n, invalid=int(invalid.item()))


@dataclass
class FitSSmoothResult:
    S: Optional[torch.Tensor]           # (R, 1, I, J), pixel order (None in SolveResult.polish_smooth)
    nll: float                          # -sum log P at S over the observed entries
    penalty: float                      # R(S), unweighted (qsc_smooth_grad)
    objective: float                    # nll + ridge / 2 |S|^2 + smooth * penalty
    sweeps: int                         # sweeps run (a sweep: colour 0, then colour 1)
    steps: torch.Tensor                 # (I, J) int32: trial evaluations each pixel used in all
    moved: int                          # pixels the last sweep moved by more than tol (1 + |s|_inf)
    unconverged: int                    # pixels of the last sweep whose last trial was not an
                                        # accepted step within tol (stalled pixels among them)
    unidentified: int                   # pixels of the last sweep whose J + prior + ridge never
                                        # had positive pivots


def check_fit_s_smooth(loss, smooth, smooth_kind, smooth_delta, ridge, kind, sweeps, inner_steps,
                       tol, mu0):
    """Validate the fit_S_smooth arguments (before anything touches a device); float(smooth)."""
    if int(inner_steps) < 1:
        raise ValueError("inner_steps must be >= 1, got %r" % (inner_steps,))
    check_fit_s(loss, ridge, kind, inner_steps, tol, mu0)
    smooth = check_smooth(smooth, smooth_kind, smooth_delta)
    if not smooth > 0.0:
        raise ValueError("fit_S_smooth needs smooth > 0, got %r: without the prior the pixels are "
                         "independent and fit_S fits them in one launch" % (smooth,))
    if int(sweeps) < 1:
        raise ValueError("sweeps must be >= 1, got %r" % (sweeps,))
    return smooth


def _sfit_smooth_bufs(obs, R, sweeps):
    """The device buffers of a run of visits: (f, nll, steps (zeroed), counters (sweeps, 2, 3)
    int32 zeroed -- one (n_moved, n_unconverged, n_unidentified) triple per visit, so that no
    launch waits for a reset -- and the workspace or None)."""
    desc, _, _ = obs.layout(R)
    dev = obs.device
    f = torch.zeros(obs.Pp, dtype=torch.float32, device=dev)
    nll = torch.zeros(obs.Pp, dtype=torch.float32, device=dev)
    steps = torch.zeros(obs.Pp, dtype=torch.int32, device=dev)
    counters = torch.zeros((int(sweeps), 2, 3), dtype=torch.int32, device=dev)
    nws = int(_lib.lib().qsc_sfit_smooth_workspace_bytes(desc, R))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
    return f, nll, steps, counters, ws


def _sfit_smooth_visit(obs, S_pos, C, R, color, kind, ridge, inner_steps, tol, mu0, project,
                       smooth_code, delta, weight, f, nll, steps, cnt, ws):
    """qsc_sfit_smooth: one visit of one colour, in place on the position-order S_pos (Pp, RP);
    cnt a (3,) int32 device view (n_moved, n_unconverged, n_unidentified) the call adds to."""
    desc, s_entries, _ = obs.layout(R)
    _lib.call("qsc_sfit_smooth", desc, _lib.ptr(s_entries), _lib.ptr(obs.s_width),
              _lib.ptr(obs.s_off), _lib.ptr(obs.perm), _lib.ptr(obs.neighbors()), obs.I, obs.J,
              int(color), obs.model, R, _lib.ptr(C), _lib.ptr(S_pos), INFO_KINDS[kind],
              float(ridge), float(mu0), float(tol), int(inner_steps), 1 if project else 0,
              smooth_code, float(delta), float(weight), _lib.ptr(f), _lib.ptr(nll),
              _lib.ptr(steps), _lib.ptr(cnt[0:1]), _lib.ptr(cnt[1:2]), _lib.ptr(cnt[2:3]),
              _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream())


def _fit_s_smooth_pos(obs, S_pos, C, R, kind, ridge, sweeps, inner_steps, tol, mu0, project,
                      smooth_kind_, smooth_delta, weight, sync_every=4):
    """Red-black sweeps of qsc_sfit_smooth in place on S_pos: (nll (Pp,), steps (Pp,),
    counters (sweeps, 2, 3), sweeps run).  With sync_every = 0 nothing is read back."""
    code, delta = _kind_code(smooth_kind_, smooth_delta)
    f, nll, steps, counters, ws = _sfit_smooth_bufs(obs, R, sweeps)
    # (not _iterate: a sweep writes, and the read-back sums, its own row of the counters)
    n = 0
    for i in range(int(sweeps)):
        for color in (0, 1):
            _sfit_smooth_visit(obs, S_pos, C, R, color, kind, ridge, inner_steps, tol, mu0,
                               project, code, delta, weight, f, nll, steps, counters[i, color], ws)
        n = i + 1
        if sync_every and n % int(sync_every) == 0 and int(counters[i, :, 0].sum().item()) == 0:
            break
    return nll, steps, counters, n


def _smooth_penalty_pos(obs, S_pos, R, smooth_kind_, smooth_delta):
    """R(S), unweighted, of a position-order S (qsc_smooth_grad with dS = NULL); synchronises."""
    code, delta = _kind_code(smooth_kind_, smooth_delta)
    dev = S_pos.device
    nb = int(_lib.lib().qsc_smooth_workspace_bytes(obs.Pp))
    if nb == 0:
        raise _lib.QscError("the smoothness prior does not support Pp = %d" % obs.Pp)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    pen = torch.zeros(1, dtype=torch.float32, device=dev)
    _lib.call("qsc_smooth_grad", _lib.ptr(S_pos), _lib.ptr(obs.neighbors()), R, obs.Pp, code,
              delta, 1.0, None, _lib.ptr(pen), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream())
    return float(pen.item())


def fit_S_smooth(obs, C, smooth, smooth_kind="quad", smooth_delta=None, S_init=None, ridge=0.0,
                 kind=None, sweeps=20, inner_steps=2, tol=1e-5, mu0=1e-3, project=None,
                 sync_every=4):
    """The loss fields S for known spectra C under the smoothness prior: red-black Newton sweeps.

    Minimises F(S) = NLL(S) + ridge / 2 |S|^2 + smooth * R(S), R the prior of solve(smooth=...)
    ("quad" or "huber" with smooth_delta).  The prior couples each pixel to its 4 grid neighbours
    only, and that graph is bipartite in the colour (i + j) & 1: with one colour held fixed the
    pixels of the other are independent, and each takes up to inner_steps damped Newton steps of
    fit_S's iteration on its own phi = f + smooth * (prior terms of its edges) in one HIP launch
    (qsc_sfit_smooth, include/qsc.h).  A sweep is colour 0 then colour 1; every accepted step
    lowers its pixel's phi, so F never increases (block coordinate descent; F is convex under the
    linear model).  A pixel without observations is determined by its neighbours.
    obs, C, S_init, ridge, kind, tol, mu0, project: as fit_S (the same defaults).  Every
    sync_every sweeps the count of pixels the sweep moved by more than tol (1 + |s|_inf) is read
    back and the fit stops at 0 (sync_every=0: never, all sweeps run; the result is the same bits
    where none stops early).  A visit restarts the damping at mu0 and has inner_steps trials: a
    pixel whose trials are all rejected (far in a link's tail, from S = 0 under the logit or log
    model, say) does not move and is not counted in `moved`, so start such fits from a solver's
    S, as polish_smooth does, or raise inner_steps.  `unconverged` counts the pixels whose last
    trial of the last sweep was not an accepted step within tol: every stalled pixel, but also
    the many pixels of a converged fit whose last, rounding-sized step is rejected (117 of 135
    against a stall's 134 on the logit test input), so it is a hint, not a test of convergence.
    Returns FitSSmoothResult(S (R,1,I,J), nll, penalty, objective, sweeps, steps (I,J), moved,
    unconverged, unidentified): nll the fp64 sum of the per-pixel NLL in a fixed order, penalty R(S) unweighted
    (qsc_smooth_grad), objective = nll + ridge / 2 |S|^2 + smooth * penalty, moved and
    unidentified of the last sweep run.  Raises ValueError for smooth <= 0 (use fit_S), sweeps or
    inner_steps < 1, an unknown smooth_kind, huber without delta > 0 and everything fit_S raises
    for, before any GPU call."""
    smooth = check_fit_s_smooth(getattr(obs, "loss", None), smooth, smooth_kind, smooth_delta,
                                ridge, kind, sweeps, inner_steps, tol, mu0)
    kind, project = _defaults(obs, kind, project)
    R = C.shape[0]
    S_pos, Cd = _inputs(obs, _start(obs, S_init, R, obs.P), C, R)
    nll_pos, steps, counters, n = _fit_s_smooth_pos(obs, S_pos, Cd, R, kind, ridge, sweeps,
                                                    inner_steps, tol, mu0, project, smooth_kind,
                                                    smooth_delta, smooth, sync_every=sync_every)
    pen = _smooth_penalty_pos(obs, S_pos, R, smooth_kind, smooth_delta)
    nll = float(nll_pos.double().sum())
    normsq = float((S_pos.double() ** 2).sum())
    moved, unconverged, unidentified = counters[n - 1].sum(dim=0).tolist()
    return FitSSmoothResult(S=obs.to_pixels(S_pos, R).reshape(R, 1, obs.I, obs.J), nll=nll,
                            penalty=pen, objective=nll + 0.5 * float(ridge) * normsq + smooth * pen,
                            sweeps=n, steps=steps[obs.iperm().long()].reshape(obs.I, obs.J),
                            moved=int(moved), unconverged=int(unconverged),
                            unidentified=int(unidentified))


@dataclass
class PostSolve:
    """solve()'s validated post-solve options (check_post_solve): the four counts, 0 = off, the
    confidence kind (None = off) with its ridge (None = default_confidence_ridge), and whether
    check_fit runs."""
    polish_c: int = 0
    polish_s: int = 0
    polish_smooth: int = 0
    calibrate: int = 0
    confidence: Optional[str] = None
    confidence_ridge: Optional[float] = None
    check: bool = False


def _check_option(name, value, generator, loss):
    """The rules every post-solve option of solve() shares: a count >= 0 and, where it is on, a
    free S and a likelihood.  -> the count."""
    n = int(value)
    if n < 0:
        raise ValueError("%s must be >= 0, got %r" % (name, value))
    if n > 0:
        if generator is not None:
            raise ValueError("%s applies to free S only: with a generator S is not a free "
                             "parameter" % name)
        if loss == "squared":
            raise ValueError('%s needs a likelihood: loss="squared" has none' % name)
    return n


def check_polish_c(polish_c, generator, loss):
    """Validate solve(polish_c=...) (before anything touches a device); the step count.  The
    smoothness prior is allowed: it does not involve C."""
    return _check_option("polish_c", polish_c, generator, loss)


def check_post_solve(generator, loss, smooth, polish_s=0, polish_c=0, polish_smooth=0, calibrate=0,
                     confidence=None, confidence_ridge=None, check=False):
    """Validate solve(polish_s=, polish_c=, polish_smooth=, calibrate=, confidence=,
    confidence_ridge=, check=) (before anything touches a device) -> PostSolve.  `smooth` is solve's
    checked weight of the smoothness prior."""
    n_s = _check_option("polish_s", polish_s, generator, loss)
    if n_s and smooth > 0.0:
        raise ValueError("polish_s fits every pixel on its own; the smoothness prior "
                         "(smooth > 0) couples pixels")
    n_c = check_polish_c(polish_c, generator, loss)
    n_smooth = _check_option("polish_smooth", polish_smooth, generator, loss)
    if n_smooth and not smooth > 0.0:
        raise ValueError("polish_smooth fits S under the smoothness prior: it needs "
                         "smooth > 0 (without the prior, polish_s fits every pixel on its own)")
    n_cal = _check_option("calibrate", calibrate, generator, loss)
    if _check_option("confidence", confidence is not None, generator, loss):
        check_confidence(confidence, confidence_ridge, loss)
    do_check = bool(_check_option("check", bool(check), generator, loss))
    return PostSolve(polish_c=n_c, polish_s=n_s, polish_smooth=n_smooth, calibrate=n_cal,
                     confidence=confidence, confidence_ridge=confidence_ridge, check=do_check)


def post_solve(res, obs, opts, lambda_s, lambda_c, project_s, smooth, smooth_kind, smooth_delta):
    """solve()'s post-solve stage on the SolveResult `res` of a free-S or holdout solve on `obs`,
    in this order, each step started from the S, C the one before left in `res`:
      polish_c       C <- fit_C at S, ridge lambda_c / ||C||_F; res.polish_c (without C)
      polish_s       S <- fit_S at C, ridge lambda_s / ||S||_F; res.polish (without S)
      polish_smooth  S <- that many sweeps of fit_S_smooth at C under the solve's prior, the
                     ridge of polish_s; res.polish_smooth (without S)
      calibrate      S, C <- that many rounds of calibrate with both ridges; res.calibration
                     (without S, C); what follows runs on its .obs, the calibrated model
      confidence     res.std_S and res.unidentified at the returned S, C, the ridge
                     opts.confidence_ridge or lambda_s / ||S||_F
      check          res.check = check_fit at the returned S, C, fitted, the ridge
                     lambda_s / ||S||_F
    opts: check_post_solve's PostSolve; a step that is off is skipped.  -> res."""
    if opts.polish_c:
        r = fit_C(obs, res.S, C_init=res.C, ridge=default_confidence_ridge(res.C, lambda_c),
                  max_steps=opts.polish_c, project=True)
        res.C, r.C = r.C, None
        res.polish_c = r
    if opts.polish_s:
        r = fit_S(obs, res.C, S_init=res.S, ridge=default_confidence_ridge(res.S, lambda_s),
                  max_steps=opts.polish_s, project=project_s)
        res.S, r.S = r.S, None
        res.polish = r
    if opts.polish_smooth:
        r = fit_S_smooth(obs, res.C, smooth, smooth_kind=smooth_kind, smooth_delta=smooth_delta,
                         S_init=res.S, ridge=default_confidence_ridge(res.S, lambda_s),
                         sweeps=opts.polish_smooth, project=project_s)
        res.S, r.S = r.S, None
        res.polish_smooth = r
    if opts.calibrate:
        r = calibrate(obs, res.S, res.C, rounds=opts.calibrate,
                      ridge_s=default_confidence_ridge(res.S, lambda_s),
                      ridge_c=default_confidence_ridge(res.C, lambda_c), project_s=project_s)
        res.S, res.C, r.S, r.C = r.S, r.C, None, None
        res.calibration = r
        obs = r.obs
    if opts.confidence is not None:
        ridge = (default_confidence_ridge(res.S, lambda_s) if opts.confidence_ridge is None
                 else float(opts.confidence_ridge))
        c = confidence(obs, res.S, res.C, kind=opts.confidence, ridge=ridge)
        res.std_S, res.unidentified = c.std_S, c.unidentified
    if opts.check:
        res.check = check_fit(obs, res.S, res.C, fitted=True,
                              ridge=default_confidence_ridge(res.S, lambda_s))
    return res
