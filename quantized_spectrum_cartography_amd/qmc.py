"""Alternating S/C maximum-likelihood solver — the drop-in for the qmc.py / qmc.ipynb solver.

The reference's solver is the notebook cell qmc/qmc.ipynb cell 1 (raw-JSON lines :422-653,
loop at :559-645); qmc/qmc.py is only its import preamble.  Per outer iteration it runs
  C-step (cinnerIter = 1):  cost = -sum(Wx log P(Y | T_hat(S, C))) + lambda_c ||C||_F
                            + lambda_s ||Z||_F;  Adam(lr 5e-3) on C;  C[C<0] = 0      (:562-579)
  S-step (sinnerIter = 1):  same cost;  Adam(lr 1e-2) on Z with S = G(Z)            (:622-634)
`solve` reproduces that loop in two modes:
  * free S (generator=None): S itself is the Adam variable with lambda_s ||S||_F, the form of
    backup/notebooks/onebit_lowrank.ipynb:1230-1236 (needed for maps that are not 51x51);
    every grad-step is a fused HIP pass with the Adam update on the device, no host sync.
  * generator (S = generator(Z)): the C-step is the fused HIP C-step; the S-step gets dS from
    the fused HIP S-pass and back-propagates it through the torch generator to Z (the
    reference's GAN path, Z optimised, network frozen: :547-550).
"""
import math
import warnings
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import _lib
from ._model import _dev, map_nmse
# the post-solve estimators live in fits.py; qmc.fit_S etc. stay the user-facing spellings
from .fits import (  # noqa: F401
    DESIGN_CRITERIA, INFO_KINDS, BootstrapResult, CalibrateResult, CheckResult, ConfidenceResult,
    CrossValidateResult, DesignResult, FitCResult, bootstrap, check_bootstrap,
    check_cross_validate, cross_validate,
    AcquireResult, AcquireRound, acquire, check_acquire,
    FitNoiseResult, FitSResult, FitSSmoothResult, _fit_c_pos, _fit_noise_pos, _fit_s_pos,
    _fit_s_smooth_pos, _sfit_smooth_bufs, _sfit_smooth_visit, calibrate, check_confidence, check_design,
    check_fit, check_fit_noise, check_polish_c, check_post_solve, confidence, default_confidence_ridge,
    design, fit_C, fit_noise,
    fit_S, fit_S_smooth, model_nll, post_solve, shifted_boundaries)
from .fused import PassEngine, check_smooth
from .obs import Observations, check_draw_readings, draw_readings  # noqa: F401
# the run driver and the hipGraph mechanics live in runs.py; these spellings stay importable
from .runs import (  # noqa: F401
    GRAPH_MAX_ITERS, AlternatingSolver, abandon_capture, capture_stream, cost_history,
    graph_chunks, quiesce_collectives, stream_capture_status)
from .utils import LOG_OFFSET_7_ADJUSTED as LOG_OFFSET


@dataclass
class SolveResult:
    S: torch.Tensor                     # (R, 1, I, J), natural pixel order
    C: torch.Tensor                     # (R, K)
    costs_c: List[float]                # cost evaluated in each C-step (before the update)
    costs_s: List[float]                # cost evaluated in each S-step (before the update)
    nmse: List[float] = field(default_factory=list)  # map NMSE after each tracked iteration
    Z: Optional[torch.Tensor] = None
    iters: int = 0
    fused: bool = False                 # S-step + next C-pass ran as one launch (qsc_scpass)
    std_S: Optional[torch.Tensor] = None  # (R, 1, I, J) standard deviations (solve(confidence=...))
    unidentified: Optional[int] = None  # pixels whose information block is not positive definite
    polish: Optional["FitSResult"] = None  # solve(polish_s=n): the fit_S run on S (without S)
    polish_c: Optional["FitCResult"] = None  # solve(polish_c=n): the fit_C run on C (without C)
    # solve(polish_smooth=n): the fit_S_smooth run on S (without S)
    polish_smooth: Optional["FitSSmoothResult"] = None
    # solve(calibrate=n): the qmc.calibrate run on S, C (without them; .obs is the calibrated one)
    calibration: Optional["CalibrateResult"] = None
    check: Optional["CheckResult"] = None  # solve(check=True): qmc.check_fit at the returned S, C
    # solve(obs=, holdout=) and solve_readings: the packed observations the fit ran on, and the
    # held-out ones it early-stopped on (None without a holdout)
    obs: Optional[Observations] = None
    obs_holdout: Optional[Observations] = None


class FreeSSolver(AlternatingSolver):
    """Device-resident free-S alternating solver over one Observations set.

    State (position-ordered S, Adam moments, step counters, ||S||^2, NLLs) lives on the GPU.
    An iteration is cpass, cfinish (C-step) then spass (S-step).  With `fuse` (default where
    qsc_scpass_supported) `run(n)` issues the same kernel sequence with each S-step and the
    following C-pass in one launch: cpass, cfinish, (scpass, cfinish) x (n-1), spass -- two
    launches per iteration.  With `use_graph` the whole sequence of run(n) is captured once per
    n in a hipGraph (torch.cuda.CUDAGraph) and replayed; `prepare(n)` captures it ahead.
    """

    graph_state = ("S", "C", "mS", "vS", "mC", "vC")

    def __init__(self, obs, S_init, C_init, lambda_c=100.0, lambda_s=100.0, lr_c=5e-3, lr_s=1e-2,
                 betas=(0.9, 0.999), eps=1e-8, project_c=True, hist_cap=1024, fuse=True,
                 T_true=None, nmse_every=0, project_s=None, chain=True, smooth=0.0,
                 smooth_kind="quad", smooth_delta=None):
        super().__init__()
        self.smooth = check_smooth(smooth, smooth_kind, smooth_delta)
        self.smooth_kind, self.smooth_delta = smooth_kind, smooth_delta
        self.obs = obs
        R = S_init.shape[0]
        self.R = R
        self.engine = PassEngine(obs, R, hist_cap=hist_cap)
        self.S = obs.to_positions(S_init.reshape(R, -1))
        self.C = _dev(C_init.detach().to(torch.float32)).reshape(R, obs.K).clone()
        self.mS, self.vS = torch.zeros_like(self.S), torch.zeros_like(self.S)
        self.mC, self.vC = torch.zeros_like(self.C), torch.zeros_like(self.C)
        self.adam_c = _lib.make_adam(lr_c, betas, eps, project_nonneg=project_c)
        # project_s: S >= 0 after every S-step (S[S<0] = 0, fused into the S-side Adam), the
        # domain of the reference's generator / decoder S (sigmoid outputs, deep_prior/networks/
        # dip.py:80).  Default (None): on under the log model, where T_hat + offset must stay > 0
        # -- unprojected free S drives T_hat + offset <= 0 within ~200 iterations at C5
        # (log of a non-positive value: a non-finite cost and S); off otherwise
        if project_s is None:
            project_s = bool(getattr(obs, "log_model", False))
        self.project_s = bool(project_s)
        self.adam_s = _lib.make_adam(lr_s, betas, eps, project_nonneg=self.project_s)
        self.lambda_c, self.lambda_s = float(lambda_c), float(lambda_s)
        self.engine.init_state(self.S)
        self.fuse = bool(fuse) and self.engine.scpass_supported()
        # chain: runs end with the fused launch (AlternatingSolver.issue); `_ahead` says that the
        # workspace holds the C-pass of the next iteration at the current S, C (valid while
        # neither tensor was modified by torch since: their version counters)
        self.chain = bool(chain)
        self._ahead, self._ahead_ver = False, None
        if self.smooth > 0.0:
            # smoothness prior smooth * R(S) (qsc_smooth_grad): the S-step becomes gradient pass
            # -> prior gradient -> Adam (three launches and a one-block finish), so neither the
            # fused launch (its S-step takes no external gradient term) nor run chaining applies
            self.fuse = False
            self.chain = False
            self.dS_buf = torch.zeros_like(self.S)
            self.graph_state += ("dS_buf",)
            obs.neighbors()  # (built here, outside any capture)
            self.engine._smooth_bufs()
        # map NMSE after every `nmse_every`-th S-step, on the device inside the iteration
        # sequence (qsc_map_nmse_track; the reference evaluates it every iteration, :582, :637)
        self.nmse_every = int(nmse_every) if T_true is not None else 0
        if self.nmse_every:
            K, P = obs.K, obs.P
            self._T = _dev(T_true.detach().to(torch.float32)).reshape(K, P).contiguous()
            self._iperm = obs.iperm()
            self._nmse_hist = torch.zeros((max(hist_cap // self.nmse_every, 1), 2),
                                          dtype=torch.float64, device=self.S.device)
            self._nmse_ws = torch.empty(_lib.lib().qsc_reduce_workspace_bytes(0),
                                        dtype=torch.uint8, device=self.S.device)
    # one outer iteration = C grad-step + S grad-step
    def c_step(self):
        e = self.engine
        self._ahead = False
        e.cpass(self.S, self.C)
        e.cfinish(self.C, 1, mC=self.mC, vC=self.vC, adam=self.adam_c, lambda_c=self.lambda_c)

    def s_step(self):
        e = self.engine
        self._ahead = False
        if self.smooth > 0.0:
            # dS = NLL gradient, += smooth * grad R(S) (R(S) into the penalty history), then
            # qsc_supdate: + lambda_s S/||S||, Adam, the S >= 0 projection
            e.spass(self.S, self.C, 0, dS=self.dS_buf)
            e.smooth_grad(self.S, self.dS_buf, self.smooth_kind, self.smooth_delta, self.smooth)
            e.supdate(self.S, self.mS, self.vS, self.dS_buf, self.adam_s, self.lambda_s)
            self._track()
            return
        e.spass(self.S, self.C, 1, mS=self.mS, vS=self.vS, adam=self.adam_s, lambda_s=self.lambda_s)
        self._track()

    # ---- run chaining (AlternatingSolver.issue) ----
    def _chain_key(self):
        """What a C-pass left ahead depends on: S and C (their storage and torch version
        counters: an in-place torch write, or a fresh tensor swapped in) and the workspace it
        sits in (the engine's launch generation: any pass or finish launched on the engine since,
        by this solver or by a caller such as bench.time_kernel, may have overwritten it)."""
        return (self.S.data_ptr(), self.S._version, self.C.data_ptr(), self.C._version,
                self.engine.gen)

    def ahead(self):
        """True when the workspace holds the next iteration's C-pass at the current S, C."""
        return self.chain and self._ahead and self._ahead_ver == self._chain_key()

    def c_finish(self):
        """The C-step on the C-pass a previous run left ahead (its finish only)."""
        self._ahead = False
        self.engine.cfinish(self.C, 1, mC=self.mC, vC=self.vC, adam=self.adam_c,
                            lambda_c=self.lambda_c)

    def fused_last(self):
        """The run's last S-step, fused with the next iteration's C-pass (left ahead)."""
        e = self.engine
        e.scpass(self.S, self.C, self.mS, self.vS, self.adam_s, self.lambda_s)
        self._track()
        self.chain_replayed()

    def chain_replayed(self):
        """(after a replayed or issued chaining run: its last fused launch left a C-pass ahead)"""
        if self.chain and self.fuse:
            self._ahead, self._ahead_ver = True, self._chain_key()

    def capture_mark(self):
        return (self._ahead, self._ahead_ver, self.engine.gen)

    def capture_restore(self, mark):
        # (a capture issues launches without executing them: the engine's generation returns to
        # its value before the capture, so the captured run does not invalidate the state)
        self._ahead, self._ahead_ver, self.engine.gen = mark

    def chain_force(self, ahead):
        """Set the chaining state run() starts from (prepare: capture both entry forms)."""
        if ahead:
            self.chain_replayed()
        else:
            self._ahead = False
        return self.ahead() == bool(ahead)

    def graph_key(self, n):
        return (n, self.ahead())

    def fused_body(self):
        """S-step i fused with C-pass i+1, then C-step i+1's finish (needs a C-step before)."""
        e = self.engine
        self._ahead = False
        e.scpass(self.S, self.C, self.mS, self.vS, self.adam_s, self.lambda_s)
        self._track()  # (S_{i+1}, C_{i+1}): C is updated by the cfinish below
        e.cfinish(self.C, 1, mC=self.mC, vC=self.vC, adam=self.adam_c, lambda_c=self.lambda_c)

    def _track(self):
        if not self.nmse_every:
            return
        o = self.obs
        _lib.call("qsc_map_nmse_track", _lib.ptr(self.S), _lib.ptr(self._iperm), self.S.shape[1],
                  _lib.ptr(self.C), _lib.ptr(self._T), self.R, o.P, o.K, 0, 0.0,
                  _lib.ptr(self.engine.state), self.nmse_every, _lib.ptr(self._nmse_hist),
                  self._nmse_hist.shape[0], _lib.ptr(self._nmse_ws), self._nmse_ws.numel(),
                  _lib.stream())

    def nmse_history(self):
        """Map NMSE after S-steps nmse_every, 2 nmse_every, ... recorded so far."""
        if not self.nmse_every:
            return []
        n = min(int(self.state()["iter"]) // self.nmse_every, self._nmse_hist.shape[0])
        h = self._nmse_hist[:n].cpu()
        return [float((a / b) ** 0.5) if b > 0 else float("nan") for a, b in h.tolist()]

    # ---- results --------------------------------------------------------------------------
    def S_pixels(self):
        return self.obs.to_pixels(self.S, self.R).reshape(self.R, 1, self.obs.I, self.obs.J)

    def history(self):
        self.engine.flush()  # settle the last S-pass (its history row)
        st = self.state()
        n = min(int(st["iter"]), self.engine.hist_cap)
        rows = self.engine.hist[: 4 * n].view(n, 4).double().cpu().tolist()
        nsq_c_final = float((self.C.double() ** 2).sum().item())
        # smooth * R(S) at the S both steps of iteration i were evaluated with (the S before
        # S-step i), recorded by that S-step's qsc_smooth_grad
        pen = self.engine.smooth_history() if self.smooth > 0.0 else []
        return cost_history(rows, nsq_c_final, self.lambda_c,
                            [(self.lambda_s * math.sqrt(r[3]),
                              self.smooth * pen[i] if i < len(pen) else 0.0)
                             for i, r in enumerate(rows)])


def solve(Y, Wx, bin_boundaries, noise_std, R=None, S_init=None, C_init=None, offset=None,
          log_model=False, lambda_c=100.0, lambda_s=100.0, lr_c=5e-3, lr_s=1e-2, max_iter=500,
          betas=(0.9, 0.999), eps=1e-8, project_c=True, generator=None, Z_init=None,
          restart=False, restart_samples=(200, 200), T_true=None, nmse_every=0,
          use_graph=False, obs=None, tile=None, callback=None, loss="probit", fuse=True,
          project_s=None, holdout=0.0, check_every=10, patience=5, holdout_seed=0,
          smooth=0.0, smooth_kind="quad", smooth_delta=None, confidence=None,
          confidence_ridge=None, polish_s=0, polish_c=0, polish_smooth=0, obs_holdout=None,
          calibrate=0, check=False):
    """Alternating S/C probit-MLE (qmc/qmc.ipynb :559-645).

    Args mirror the notebook globals: Y (K,1,I,J) bin indices, Wx (K,1,I,J) 0/1 mask,
    bin_boundaries / noise_std / offset of the model, lambda_c = lambda_s = 100,
    lr_c = 5e-3, lr_s = 1e-2, max_iter = 500.  With `generator` the S-step optimises Z_init
    through S = generator(Z) (Adam on Z, the network frozen); otherwise S is free.
    loss="squared" replaces the probit likelihood by the Euclidean criterion
    ||Wx (T_hat - Obs)||_F^2 of qmc/qmc_dowjons.ipynb :142-162 (Obs = bin midpoints,
    get_quantized_obs_from_ordinal); the cost history then holds that criterion.
    loss="logit" replaces the probit link by the logistic one, F(y) = 1 / (1 + exp(-y / s)) with
    s = noise_std (the reference's F_sigmoid at s = 1; noise standard deviation s pi / sqrt(3)):
    every path below (free S, generator, holdout, graphs) runs the same fused passes on it.
    project_s=True keeps free S >= 0 (S[S<0] = 0 after each S-step, as C at :579).  The
    default (None) is True for the log model: it needs T_hat + offset > 0 (log at
    qmc/quantization_model_log.py:14, qmc/qmc.ipynb:571), which unprojected free S leaves within
    a few hundred steps, and the reference's own S is a sigmoid output (>= 0); False otherwise.
    project_s=False under the log model is accepted (the caller's choice) and warns.
    holdout > 0 (free S only; not in the reference, which runs a fixed iteration count): that
    fraction of the observed entries (seeded by holdout_seed) is held out of the fit; every
    `check_every` iterations their NLL at the current S, C is evaluated (fused HIP S-pass on
    the held-out set, same pixel order), and the run stops once it has not improved for
    `patience` checks, returning the S, C of the best check (result.best_iter, .holdout_nll).
    With obs= the packed readings are split on the device by obs.split(holdout, holdout_seed)
    (a counter-based split: other entries than the Y, Wx path's host draw holds out) and the
    result gains `obs` and `obs_holdout`, the two halves; qmc.cross_validate repeats this over
    K folds.  With ~6 one-bit samples per pixel (C2) the unregularised free-S MLE over-fits: the map
    NMSE is best after ~50 iterations and grows after.
    smooth > 0 (free S only; not in the reference, whose spatial prior is the generator): adds
    the smoothness prior smooth * R(S) on the loss fields to the cost of both steps, R summed
    over the 4-neighbour edges {p, p'} of the I x J grid (each once, none across the border) and
    over the emitters r:  smooth_kind="quad": R = 1/2 sum (S_r(p) - S_r(p'))^2 (Tikhonov);
    "huber": R = sum h(S_r(p) - S_r(p')), h(d) = d^2 / (2 delta) for |d| <= delta else
    |d| - delta / 2, delta = smooth_delta > 0 (a smoothed anisotropic TV that keeps edges).  The
    S-step then runs as gradient pass -> prior gradient (qsc_smooth_grad, a HIP kernel in the
    solver's pixel order) -> Adam, without the fused S-step + C-pass launch (result.fused is
    False); the cost histories include the prior.  Pixels without observations then follow
    their neighbours instead of only shrinking.  holdout= is a natural way to pick `smooth`.
    Raises ValueError for smooth < 0, an unknown kind, huber without delta > 0, or smooth > 0
    with a generator (which is itself the prior).  smooth = 0 (default) is the unregularised
    path, unchanged.
    confidence="expected" | "observed" (free S and holdout solves; not in the reference): the
    result gains std_S (R,1,I,J), the per-pixel standard deviations of the returned S from the
    Fisher information conditional on C, and `unidentified` (see qmc.confidence, which also
    gives the map's standard deviations).  The ridge added to every pixel's information block is
    confidence_ridge, or by default lambda_s / ||S||_F: the isotropic part of the Hessian of the
    lambda_s ||S||_F regulariser (its rank-one part, -lambda_s s s^T / ||S||^3, couples all
    pixels and is dropped).  Raises ValueError with a generator (the generator is the prior and
    S is not free), with loss="squared", for an unknown kind or a negative ridge.  The default
    None leaves every path and result as it is.
    polish_s=n > 0 (free S and holdout solves; not in the reference): after the loop -- and after
    the holdout's best-check restore -- S is replaced by qmc.fit_S started from it at the returned
    C, for up to n damped Newton steps per pixel, with the ridge lambda_s / ||S||_F of
    default_confidence_ridge: the conditional MLE, where the Adam iterate is not stationary in S.
    It runs before confidence= is attached, so std_S is evaluated at the point the theory is
    about; result.polish is the FitSResult (without S).  Raises ValueError with a generator, with
    loss="squared" and with smooth > 0: the fit treats every pixel on its own, and the
    smoothness prior couples pixels.  The default 0 leaves every path and result bit-identical.
    polish_c=n > 0 (free S and holdout solves; not in the reference): after the loop and the
    holdout restore, and before polish_s, C is replaced by qmc.fit_C started from it at the
    returned S, for up to n projected Newton steps per bin with the ridge lambda_c / ||C||_F --
    so a following polish_s fits S at the polished C.  result.polish_c is the FitCResult (without
    C).  Raises ValueError with a generator and with loss="squared"; smooth > 0 is allowed (the
    prior does not involve C).  The default 0 leaves every path and result bit-identical.
    polish_smooth=n > 0 (free S and holdout solves with smooth > 0; not in the reference): after
    polish_c and before confidence=, S is replaced by n red-black sweeps of qmc.fit_S_smooth
    started from it at the returned C, under the solve's own smooth, smooth_kind and smooth_delta
    and the ridge lambda_s / ||S||_F of polish_s: the second-order fit for the solves polish_s
    refuses.  result.polish_smooth is the FitSSmoothResult (without S).  Raises ValueError with
    smooth = 0, with a generator and with loss="squared".  The default 0 leaves every path and
    result bit-identical.
    calibrate=n > 0 (free S and holdout solves; not in the reference, which hard-codes sigma): after
    the polish steps and before confidence= is attached, n rounds of qmc.calibrate (fit_noise, then
    fit_C, then fit_S under the re-estimated noise scale and level shift) run from the returned S,
    C with the ridges lambda_s / ||S||_F and lambda_c / ||C||_F of the polish steps; S and C are
    replaced, the confidence is then evaluated under the calibrated model, and result.calibration
    is the CalibrateResult (without S, C; its .obs carries the calibrated model).  Raises
    ValueError with a generator and with loss="squared".  The default 0 leaves every path and
    result bit-identical.
    check=True (free S and holdout solves; not in the reference): last of all, on the calibrated
    observations if calibrate= ran, result.check = qmc.check_fit(obs, S, C, fitted=True) with the
    ridge lambda_s / ||S||_F: per-pixel goodness of fit and level-shift score tests of the readings
    the solve ran on.  Raises ValueError with a generator and with loss="squared".  The default
    False leaves every path and result as it is.
    obs= gives the packed observations (an Observations, e.g. Observations.from_readings for a
    list of sensor reports); Y and Wx may then be None, and K, I, J, the model and the loss are
    obs's.  obs_holdout= (with obs=, free S only) is a second Observations packed with obs.perm and
    obs's tile: the run then early-stops on its NLL exactly as holdout > 0 does on the entries it
    splits off itself (solve_readings(holdout=...) splits a list of readings this way).  Its loss
    and model (bin boundaries, noise_std, offset, log_model) must be obs's.
    Returns a SolveResult with S (R,1,I,J) and C (R,K) on the GPU.
    """
    if Y is None and obs is None:
        raise ValueError("Y=None needs obs=: the packed observations (Observations, "
                         "Observations.from_readings)")
    if obs_holdout is not None:
        if obs is None or generator is not None:
            raise ValueError("obs_holdout goes with obs= and free S")
        if (obs_holdout.Pp != obs.Pp or obs_holdout.desc.PT != obs.desc.PT
                or obs_holdout.K != obs.K or not torch.equal(obs_holdout.perm, obs.perm)):
            raise ValueError("obs_holdout must be packed with obs.perm and obs's tile")
        if any(getattr(obs_holdout, a) != getattr(obs, a)
               for a in ("loss", "log_model", "noise_std", "offset", "bin_boundaries")):
            raise ValueError("obs_holdout must carry obs's loss and model (bin boundaries, "
                             "noise_std, offset, log_model)")
    smooth = check_smooth(smooth, smooth_kind, smooth_delta)
    if smooth > 0.0 and generator is not None:
        raise ValueError("smooth > 0 applies to free S only: a generator already carries the "
                         "spatial prior")
    post = check_post_solve(generator, obs.loss if obs is not None else loss, smooth,
                            polish_s=polish_s, polish_c=polish_c, polish_smooth=polish_smooth,
                            calibrate=calibrate, confidence=confidence,
                            confidence_ridge=confidence_ridge, check=check)
    if log_model and obs is None:
        # the reference log model's default offset (qmc/quantization_model_log.py:7, 9)
        offset = LOG_OFFSET if offset is None else float(offset)
        if not offset > 0.0:
            raise ValueError("the log model needs offset > 0 (log(T_hat + offset) at T_hat = 0)")
    if Y is None:
        K, I, J = obs.K, obs.I, obs.J
    else:
        K = Y.shape[0]
        I, J = Y.shape[-2], Y.shape[-1]
    if R is None:
        R = (S_init.shape[0] if S_init is not None else
             (C_init.shape[0] if C_init is not None else Z_init.shape[0]))
    obs_h = obs_holdout
    split_obs = False
    if holdout and generator is None and obs_h is None and obs is not None:
        # packed observations are split on the device, in obs's pixel order (obs.split)
        obs, obs_h = obs.split(float(holdout), holdout_seed)
        split_obs = True
    elif holdout and generator is None and obs_h is None:
        Wx_fit, Wx_h = split_holdout(Y, Wx, float(holdout), holdout_seed)
        obs = Observations(Y, Wx_fit, bin_boundaries, noise_std, offset=offset or 0.0,
                           log_model=log_model, tile=tile, R_hint=R, loss=loss)
        # the held-out entries in the SAME position order (perm) and tiles, so the solver's
        # position-order S is evaluated on them as it is
        obs_h = Observations(Y, Wx_h, bin_boundaries, noise_std, offset=offset or 0.0,
                             log_model=log_model, tile=obs.desc.PT, R_hint=R, loss=loss,
                             perm=obs.perm)
    if obs is None:
        obs = Observations(Y, Wx, bin_boundaries, noise_std, offset=offset or 0.0,
                           log_model=log_model, tile=tile, R_hint=R, loss=loss)
    if C_init is None:
        C_init = torch.zeros(R, K)
    if generator is None and obs_h is not None:
        res = _solve_holdout(obs, obs_h, S_init, C_init, R, lambda_c, lambda_s, lr_c, lr_s,
                             max_iter, betas, eps, project_c, fuse, project_s, use_graph,
                             int(check_every), int(patience), smooth, smooth_kind, smooth_delta)
        # (on the fitted entries, the held-out ones excluded)
        res = post_solve(res, obs, post, lambda_s, lambda_c, project_s, smooth, smooth_kind,
                         smooth_delta)
        if split_obs:
            res.obs, res.obs_holdout = obs, obs_h
        return res
    if generator is None:
        if S_init is None:
            S_init = torch.zeros(R, 1, I, J)
        if project_s is None:
            project_s = bool(obs.log_model)
        elif log_model and not project_s:
            warnings.warn("free S under the log model without project_s: T_hat + offset can "
                          "reach <= 0 (a non-finite cost)", RuntimeWarning)
        # the NMSE history is recorded on the device inside the run (no host round trips);
        # a callback still gets control every nmse_every iterations (or once at the end)
        sol = FreeSSolver(obs, S_init, C_init, lambda_c, lambda_s, lr_c, lr_s, betas, eps,
                          project_c, hist_cap=max_iter, fuse=fuse,
                          T_true=T_true if nmse_every else None, nmse_every=nmse_every,
                          project_s=project_s, smooth=smooth, smooth_kind=smooth_kind,
                          smooth_delta=smooth_delta)
        done = 0
        chunk = nmse_every if (callback is not None and nmse_every) else max_iter
        while done < max_iter:
            n = min(chunk, max_iter - done)
            sol.run(n, use_graph=use_graph)
            done += n
            if callback is not None:
                callback(done, sol)
        nmse = sol.nmse_history()
        costs_c, costs_s = sol.history()
        res = SolveResult(S=sol.S_pixels(), C=sol.C.clone(), costs_c=costs_c, costs_s=costs_s,
                          nmse=nmse, iters=max_iter, fused=sol.fuse)
        return post_solve(res, obs, post, lambda_s, lambda_c, project_s, smooth, smooth_kind,
                          smooth_delta)
    return _solve_generator(obs, generator, Z_init, C_init, R, lambda_c, lambda_s, lr_c, lr_s,
                            max_iter, betas, eps, project_c, restart, restart_samples, T_true,
                            nmse_every, callback, use_graph=use_graph)


# iterations per captured hipGraph of the generator / DIP solver (GeneratorSolver): every
# iteration is ~100 graph nodes (the torch decoder's forward and backward, its optimizer step and
# the HIP passes), so long runs replay a chunk graph instead of one graph of the whole run
GEN_GRAPH_ITERS = 32


class GeneratorSolver(AlternatingSolver):
    """S = generator(Z) alternating solver (qmc/qmc.ipynb :541-634) as a device-resident op
    sequence that is captured in hipGraphs (the DIP solver of dip.solve, the GAN path of solve).

    One iteration, no host synchronisation anywhere:
      C-step  fused HIP C-pass at S_pos (the S of the previous S-step, :564) + qsc_cfinish (Adam on
              C, C >= 0, :576-579); the step's NLL / ||C||^2 stay in the engine's history rows;
      S-step  S = generator(Z) (torch, MIOpen convs), S -> position order (qsc_perm_gather into
              the persistent S_pos), fused HIP S-pass in gradient mode (dS), qsc_state_flush
              (the S-step NLL into the history row), dS -> pixel order, the surrogate
              <S, dS> + lambda_s ||Z||_F back-propagated through the generator (:626-633), the
              optimizer step (:634) -- qsc_adam_flat over the flat parameter buffer, its step
              the engine state's S-step count; lambda_s ||Z|| recorded on the device.
    run(n, use_graph=True) replays captured chunk graphs of GEN_GRAPH_ITERS iterations (sharing
    one memory pool) after WARMUP eager iterations, which create the autograd / MIOpen
    workspaces outside capture.  The optimised tensors live in one flat buffer and take their
    Adam step in one launch (qsc_adam_flat: torch.optim.Adam's update bit for bit, the step
    count from the engine state).  Graph replay and eager issue run the same
    kernels on the same buffers, so the results are bitwise equal
    (tests/test_gpu_fused.py::test_generator_solver_graph_equals_eager).  A capture that fails
    (a library call that cannot be captured) is recorded in `graph_error` and the solver runs
    eagerly from then on."""

    WARMUP = 1
    graph_tolerant = True
    graph_iters = GEN_GRAPH_ITERS

    def __init__(self, obs, generator, Z_init, C_init, R, lambda_c=100.0, lambda_s=100.0,
                 lr_c=5e-3, lr_s=1e-2, betas=(0.9, 0.999), eps=1e-8, project_c=True,
                 params=None, optimize_z=True, hist_cap=1024):
        super().__init__()
        dev = obs.device
        self.obs, self.net, self.R = obs, generator, R
        self.I, self.J = obs.I, obs.J
        self.engine = PassEngine(obs, R, hist_cap=max(int(hist_cap), 1))
        self.C = _dev(C_init.detach().to(torch.float32)).reshape(R, obs.K).clone()
        self.mC, self.vC = torch.zeros_like(self.C), torch.zeros_like(self.C)
        self.adam_c = _lib.make_adam(lr_c, betas, eps, project_nonneg=project_c)
        self.lambda_c, self.lambda_s = float(lambda_c), float(lambda_s)
        # The optimised tensors (Z and / or the decoder's parameters) live in ONE flat buffer
        # (each a view into it), so the S-step's Adam is one qsc_adam_flat launch over all of
        # them -- torch.optim.Adam's update bit for bit, at the step the engine state counts --
        # instead of torch's per-tensor launches (its capturable foreach path divides every
        # tensor by its 0-dim bias corrections in a launch of its own: ~150 launches of a few us
        # per iteration for the 256^2 decoder, round 6's profile).
        Z = Z_init.detach().to(dev, torch.float32)
        plist = list(params or [])
        sizes = ([Z.numel()] if optimize_z else []) + [q.numel() for q in plist]
        self.flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        o = 0
        if optimize_z:
            self.flat[:Z.numel()] = Z.reshape(-1)
            self.Z = self.flat[:Z.numel()].view(Z.shape).detach().requires_grad_(True)
            o = Z.numel()
        else:
            self.Z = Z.clone()
        for q in plist:
            n = q.numel()
            with torch.no_grad():
                self.flat[o:o + n] = q.detach().reshape(-1).to(dev, torch.float32)
                q.data = self.flat[o:o + n].view(q.shape)
            o += n
        self.plist = ([self.Z] if optimize_z else []) + plist
        self.m_flat = torch.zeros_like(self.flat)
        self.v_flat = torch.zeros_like(self.flat)
        self.g_flat = torch.zeros_like(self.flat)
        self.adam_s = _lib.make_adam(lr_s, betas, eps, project_nonneg=False)
        with torch.no_grad():
            S0 = generator(self.Z).reshape(R, 1, self.I, self.J)
        self.S_pos = obs.to_positions(S0.reshape(R, -1))
        self.engine.init_state(self.S_pos)
        self.dS_pos = torch.zeros_like(self.S_pos)
        self.dS_pix = torch.zeros((R, obs.P), dtype=torch.float32, device=dev)
        self.hist_cap = self.engine.hist_cap
        self.zreg = torch.zeros(self.hist_cap, dtype=torch.float32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self.S_last = S0.detach()
        self.done = 0
        self._eager_done = 0
        # (the chunk graphs share one memory pool)
        self.graph_pool = torch.cuda.graph_pool_handle() if self.C.is_cuda else None

    # ---- one iteration (capturable) -----------------------------------------------------
    def c_step(self):
        e = self.engine
        e.cpass(self.S_pos, self.C)
        e.cfinish(self.C, 1, mC=self.mC, vC=self.vC, adam=self.adam_c, lambda_c=self.lambda_c)

    def s_step(self):
        e, R = self.engine, self.R
        # gradients set to None: backward then writes each one instead of zeroing and adding to
        # it (two elementwise launches per parameter tensor); inside a capture the new gradients
        # live in the graph's pool
        for q in self.plist:
            q.grad = None
        S = self.net(self.Z).reshape(R, 1, self.I, self.J)
        self.obs.to_positions(S.detach().reshape(R, -1), out=self.S_pos)
        e.spass(self.S_pos, self.C, 0, dS=self.dS_pos)
        e.flush(record=True)  # the S-step NLL -> this iteration's history row
        self.obs.to_pixels(self.dS_pos, R, out=self.dS_pix)
        reg = self.lambda_s * torch.norm(self.Z, "fro")
        surrogate = (S * self.dS_pix.reshape(R, 1, self.I, self.J)).sum() + reg
        surrogate.backward()
        if self.plist:
            # the gradients into the flat buffer (one batched copy), then Adam on all of them
            torch.cat([q.grad.reshape(-1) for q in self.plist], out=self.g_flat)
            _lib.call("qsc_adam_flat", _lib.ptr(self.flat), _lib.ptr(self.m_flat),
                      _lib.ptr(self.v_flat), _lib.ptr(self.g_flat), self.flat.numel(),
                      self.adam_s, _lib.ptr(e.state), _lib.stream())
        with torch.no_grad():
            self.zreg.index_copy_(0, self.ctr.clamp(max=self.hist_cap - 1),
                                  reg.detach().reshape(1))
            self.ctr += 1
        self.S_last = S.detach()

    # ---- runs ---------------------------------------------------------------------------
    def prepare(self, n):
        """Capture (without executing) the chunk graphs run(n) will replay.  Needs the WARMUP
        eager iterations done (they create the optimizer state outside capture)."""
        if self._eager_done < self.WARMUP:
            raise RuntimeError("prepare() after %d eager iterations (run them first)" % self.WARMUP)
        super().prepare(n)

    def run(self, n, use_graph=True):
        """Enqueue n iterations (no host sync): the WARMUP iterations still to do (all n
        without use_graph) eagerly, the rest as chunk-graph replays."""
        use_graph = use_graph and self._on_gpu()
        eager = min(n, max(self.WARMUP - self._eager_done, 0)) if use_graph else n
        super().run(eager)
        self._eager_done += eager
        super().run(n - eager, use_graph=True)
        self.done += n

    def capture_mark(self):
        return self.engine.gen

    def capture_restore(self, mark):
        self.engine.gen = mark  # (a capture issues launches without executing them)

    # ---- results --------------------------------------------------------------------------
    def S_pixels(self):
        """The last S-step's generator output S (R, 1, I, J)."""
        return self.S_last

    def history(self):
        """Per-iteration costs (qmc/qmc.ipynb :573, :631): C-step cost at the C it
        differentiates, S-step cost at the updated C (both with lambda_s ||Z|| of the S-step's
        Z), from the device history rows (one synchronisation)."""
        n = min(self.done, self.hist_cap)
        rows = self.engine.hist[: 4 * n].view(n, 4).double().cpu().tolist()
        z = self.zreg[:n].double().cpu().tolist()
        nsq_c_final = float((self.C.double() ** 2).sum().item())
        return cost_history(rows, nsq_c_final, self.lambda_c, [(zi,) for zi in z])


def split_holdout(Y, Wx, frac, seed=0):
    """(Wx_fit, Wx_holdout): a seeded random `frac` of the observed entries (Wx == 1, or all
    entries when Wx is None) moved to the held-out mask."""
    W = (Wx if Wx is not None else torch.ones(Y.shape)).to(torch.float32)
    g = torch.Generator().manual_seed(int(seed))
    u = torch.rand(W.shape, generator=g).to(W.device)
    hold = (W > 0) & (u < frac)
    return W * (~hold).to(W.dtype), W * hold.to(W.dtype)


def split_readings(n, frac, seed=0):
    """(fit, held): two int64 index tensors that partition range(n), `held` a seeded random
    round(frac n) of the readings (at least one of each part), both ascending so that each part
    keeps the list's order.  The same (n, frac, seed) gives the same split."""
    n = int(n)
    if not 0.0 < float(frac) < 1.0:
        raise ValueError("the held-out fraction must be in (0, 1)")
    if n < 2:
        raise ValueError("need at least two readings to hold some out")
    g = torch.Generator().manual_seed(int(seed))
    order = torch.randperm(n, generator=g)
    nh = min(max(int(round(float(frac) * n)), 1), n - 1)
    return torch.sort(order[nh:]).values, torch.sort(order[:nh]).values


def solve_readings(k, i, j, code, shape, bin_boundaries, noise_std, R=None, offset=None,
                   log_model=False, tile=None, loss="probit", holdout=0.0, holdout_seed=0,
                   **solve_kw):
    """solve() on a list of readings (see Observations.from_readings: reading e = bin k[e] at
    pixel (i[e], j[e]) of the shape = (K, I, J) map observed with code code[e]; any order, a cell
    may be read any number of times).  The readings are packed without a dense Y / Wx and handed
    to solve(obs=...); solve_kw are solve's other keywords (S_init, C_init, max_iter, use_graph,
    smooth, confidence, polish_*, ...).  holdout > 0 holds out that fraction of the READINGS
    (split_readings, seeded by holdout_seed; a cell read three times may keep two readings in the
    fit and lend one to the check), packs them with the fit part's pixel order and tile, and
    early-stops on their NLL as solve(holdout=...) does.  The result gains `obs` (and
    `obs_holdout`, `fit_index`, `held_index` with a holdout)."""
    for name in ("obs", "obs_holdout", "generator", "Z_init"):
        if solve_kw.get(name) is not None:
            raise ValueError("solve_readings packs the readings itself and fits free S: %s= is "
                             "not accepted" % name)
    K, I, J, n = Observations.check_readings(k, i, j, code, shape, tile)
    if R is None:
        init = solve_kw.get("S_init") if solve_kw.get("S_init") is not None else \
            solve_kw.get("C_init")
        if init is None:
            raise ValueError("give R, S_init or C_init")
        R = init.shape[0]
    if log_model:
        offset = LOG_OFFSET if offset is None else float(offset)
        if not offset > 0.0:
            raise ValueError("the log model needs offset > 0 (log(T_hat + offset) at T_hat = 0)")
    kw = dict(offset=offset or 0.0, log_model=log_model, R_hint=R, loss=loss)
    if not holdout:
        obs = Observations.from_readings(k, i, j, code, (K, I, J), bin_boundaries, noise_std,
                                         tile=tile, **kw)
        res = solve(None, None, bin_boundaries, noise_std, R=R, obs=obs, **solve_kw)
        res.obs = obs
        return res
    fit, held = split_readings(n, float(holdout), holdout_seed)
    fit_d, held_d = fit.to(k.device), held.to(k.device)
    obs = Observations.from_readings(k[fit_d], i[fit_d], j[fit_d], code[fit_d], (K, I, J),
                                     bin_boundaries, noise_std, tile=tile, **kw)
    # the held-out readings in the SAME position order (perm) and tiles, so the solver's
    # position-order S is evaluated on them as it is
    obs_h = Observations.from_readings(k[held_d], i[held_d], j[held_d], code[held_d], (K, I, J),
                                       bin_boundaries, noise_std, tile=obs.desc.PT,
                                       perm=obs.perm, **kw)
    res = solve(None, None, bin_boundaries, noise_std, R=R, obs=obs, obs_holdout=obs_h,
                **solve_kw)
    res.obs, res.obs_holdout, res.fit_index, res.held_index = obs, obs_h, fit, held
    return res


def _solve_holdout(obs, obs_h, S_init, C_init, R, lambda_c, lambda_s, lr_c, lr_s, max_iter,
                   betas, eps, project_c, fuse, project_s, use_graph, check_every, patience,
                   smooth=0.0, smooth_kind="quad", smooth_delta=None):
    """Free-S solve with early stopping on the held-out NLL (solve(holdout=...)); the held-out
    criterion is the NLL alone, also with a smoothness prior on the fit."""
    I, J = obs.I, obs.J
    if S_init is None:
        S_init = torch.zeros(R, 1, I, J)
    sol = FreeSSolver(obs, S_init, C_init, lambda_c, lambda_s, lr_c, lr_s, betas, eps, project_c,
                      hist_cap=max_iter, fuse=fuse, project_s=project_s, smooth=smooth,
                      smooth_kind=smooth_kind, smooth_delta=smooth_delta)
    eng_h = PassEngine(obs_h, R)
    eng_h.init_state(sol.S)
    dS_h = torch.empty_like(sol.S)
    hist_h, best, best_iter, best_SC = [], float("inf"), 0, None
    done = 0
    while done < max_iter:
        n = min(check_every, max_iter - done)
        sol.run(n, use_graph=use_graph)
        done += n
        eng_h.spass(sol.S, sol.C, 0, dS=dS_h)
        eng_h.flush(record=False)
        v = float(eng_h.read_state()["nll_s"])
        hist_h.append((done, v))
        if v < best:
            best, best_iter = v, done
            best_SC = (sol.S.clone(), sol.C.clone())
        elif done - best_iter >= patience * check_every:
            break
    costs_c, costs_s = sol.history()
    S_pos, C = best_SC if best_SC is not None else (sol.S, sol.C)
    res = SolveResult(S=obs.to_pixels(S_pos, R).reshape(R, 1, I, J), C=C.clone(),
                      costs_c=costs_c, costs_s=costs_s, iters=done, fused=sol.fuse)
    res.best_iter = best_iter
    res.holdout_nll = hist_h
    return res


def _solve_generator(obs, generator, Z_init, C_init, R, lambda_c, lambda_s, lr_c, lr_s, max_iter,
                     betas, eps, project_c, restart, restart_samples, T_true, nmse_every,
                     callback, params=None, optimize_z=True, use_graph=True):
    """S = generator(Z) variant (qmc/qmc.ipynb :541-634) on a GeneratorSolver.  The S-step
    optimises Z (optimize_z) plus any extra `params` -- the DIP solver passes the decoder
    weights.  The one-time random restart of Z (:590-619, i == 1) runs eagerly between the
    C-step and the S-step of iteration 1; the rest runs as captured hipGraph chunks (use_graph).
    With `callback` or NMSE tracking the run is split into chunks of `nmse_every` iterations
    (callback(i, dict(S, C, Z)) after each, S the last S-step's generator output)."""
    sol = GeneratorSolver(obs, generator, Z_init, C_init, R, lambda_c, lambda_s, lr_c, lr_s,
                          betas, eps, project_c, params=params, optimize_z=optimize_z,
                          hist_cap=max_iter)
    return drive_generator(sol, max_iter, restart, restart_samples, T_true, nmse_every, callback,
                           use_graph)


def drive_generator(sol, max_iter, restart=False, restart_samples=(200, 200), T_true=None,
                    nmse_every=0, callback=None, use_graph=True):
    """Run a fresh GeneratorSolver for max_iter iterations (the loop of qmc/qmc.ipynb :559-645)
    and collect its SolveResult."""
    obs, generator, R = sol.obs, sol.net, sol.R
    lambda_c, lambda_s = sol.lambda_c, sol.lambda_s
    nmse = []
    chunk = max(int(nmse_every), 1) if (callback is not None or (T_true is not None and nmse_every)) \
        else max_iter
    done = 0

    def after(k):
        if T_true is not None and nmse_every and k % nmse_every == 0:
            nmse.append(map_nmse(sol.S_last, sol.C, T_true))
        if callback is not None:
            callback(k, dict(S=sol.S_last, C=sol.C, Z=sol.Z))

    if restart and max_iter >= 2:
        # iteration 0, then iteration 1's C-step, the restart, and its S-step (eager)
        sol.run(1, use_graph=False)
        after(1)
        sol.c_step()
        _restart_z(sol, obs, generator, R, lambda_c, lambda_s, restart_samples)
        sol.s_step()
        sol._eager_done += 1
        sol.done += 1
        after(2)
        done = 2
    while done < max_iter:
        n = min(chunk - (done % chunk), max_iter - done)
        sol.run(n, use_graph=use_graph)
        done += n
        if callback is not None or (T_true is not None and nmse_every):
            after(done)
    costs_c, costs_s = sol.history()
    res = SolveResult(S=sol.S_last, C=sol.C, costs_c=costs_c, costs_s=costs_s, nmse=nmse,
                      Z=sol.Z.detach(), iters=max_iter)
    res.graph_error = sol.graph_error
    res.solver = sol
    return res


def _restart_z(sol, obs, generator, R, lambda_c, lambda_s, restart_samples):
    """The notebook's one-time random restart of Z at i == 1 (:590-619): 200 random candidates,
    the best by its full cost, then 200 perturbations of it -- whose cost the reference
    evaluates at the LAST first-round sample (temp_out, :611: a reference quirk kept as is).
    Candidates are scored on a separate pass engine (its own state), so the solver's step
    counters and history rows are untouched."""
    dev = obs.device
    I, J = obs.I, obs.J
    eng = PassEngine(obs, R, hist_cap=0)
    Sp = torch.empty_like(sol.S_pos)
    dSp = torch.empty_like(sol.S_pos)
    eng.init_state(Sp.zero_())
    Z = sol.Z

    def nll_of(S_cand):
        obs.to_positions(S_cand.reshape(R, -1), out=Sp)
        eng.spass(Sp, sol.C, 0, dS=dSp)
        eng.flush(record=False)
        return eng.read_state()["nll_s"]

    S_now = sol.S_last
    best = float("inf")
    n1, n2 = restart_samples
    last = None
    for _ in range(n1):
        cand = torch.randn((R, Z.shape[1]), dtype=torch.float32)
        with torch.no_grad():
            out = generator(cand.to(dev)).reshape(R, 1, I, J)
        crit = nll_of(out) + lambda_c * float(torch.norm(sol.C)) + lambda_s * float(torch.norm(S_now))
        last = out
        if crit < best:
            with torch.no_grad():
                Z.copy_(cand.to(dev))
            best = crit
    for _ in range(n2):
        cand = 0.2 * torch.randn((R, Z.shape[1]), dtype=torch.float32) + Z.detach().cpu()
        crit = nll_of(last) + lambda_c * float(torch.norm(sol.C)) + lambda_s * float(torch.norm(S_now))
        if crit < best:
            with torch.no_grad():
                Z.copy_(cand.to(dev))
            best = crit
