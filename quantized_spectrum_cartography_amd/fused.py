"""Fused likelihood + gradient passes over packed observations (the hot path).

One *grad-step*  is one pass plus the update of the block it
differentiates:
  C-step:  qsc_cpass (per-tile dC partials)  ->  qsc_cfinish (fixed-order reduction,
           + lambda_c C/||C||, Adam, C[C<0] = 0)               qmc/qmc.ipynb :562-579
  S-step:  qsc_spass (dS in registers, + lambda_s S/||S||, Adam fused in the epilogue)
                                                                qmc/qmc.ipynb :622-634
Scalars (step counters, ||S||^2, NLLs, the cost history) stay on the device and their
book-keeping rides on those same kernels (qsc_state protocol in include/qsc.h), so an outer
iteration is three launches with no host synchronisation and is captured in one hipGraph.
qsc_scpass runs an S-step and the following C-pass as one launch (the C-pass of iteration i+1
reads only its tile's S_i, handed over in LDS), so solvers issue two launches per iteration.
"""
import torch

from . import _lib
from ._model import _dev, _ws


SMOOTH_KINDS = {"quad": 0, "huber": 1}  # QSC_SMOOTH_QUAD, QSC_SMOOTH_HUBER


def smooth_kind(kind, delta):
    """(kind code, delta) of the smoothness prior, validated: kind "quad" or "huber", the latter
    with delta > 0."""
    if kind not in SMOOTH_KINDS:
        raise ValueError("smooth_kind must be one of %s, got %r" % (sorted(SMOOTH_KINDS), kind))
    if kind == "huber":
        if delta is None or not float(delta) > 0.0:
            raise ValueError("smooth_kind='huber' needs smooth_delta > 0")
        return SMOOTH_KINDS[kind], float(delta)
    return SMOOTH_KINDS[kind], 0.0


def check_smooth(smooth, kind, delta):
    """Validate the solver's smoothness arguments; returns float(smooth)."""
    smooth = float(smooth)
    if not smooth >= 0.0:
        raise ValueError("smooth must be >= 0, got %r" % (smooth,))
    smooth_kind(kind, delta)
    return smooth


class PassEngine:
    """Workspace + device state for running the fused passes on one Observations set."""

    def __init__(self, obs, R, hist_cap=0):
        if not 1 <= R <= _lib.QSC_MAX_R:
            raise ValueError("rank R must be in [1, %d]" % _lib.QSC_MAX_R)
        self.obs, self.R = obs, R
        # the packed entries at this rank (signed rows, or a code-field copy: obs.layout)
        self.desc, self.s_entries, self.c_entries = obs.layout(R)
        dev = obs.device
        nb = _lib.lib().qsc_pass_workspace_bytes(self.desc, R)
        if nb == 0:
            raise _lib.QscError("invalid observation descriptor")
        # zeroed once: the S-pass keeps its slice scheduler words in the workspace and leaves
        # them zero at exit (include/qsc.h, qsc_pass_workspace_bytes)
        self.ws = torch.zeros(max(int(nb), 1), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(_lib.STATE_BYTES, dtype=torch.uint8, device=dev)
        self.hist_cap = int(hist_cap)
        self.hist = torch.zeros(max(4 * self.hist_cap, 4), dtype=torch.float32, device=dev)
        # workspace generation: bumped by every launch that writes the workspace's pass partials
        # (slab, NLL / norm partials, cnsq) or C, so a solver can tell that a C-pass it left
        # ahead in the workspace was overwritten since (qmc.FreeSSolver.ahead)
        self.gen = 0

    # ---- state --------------------------------------------------------------------------
    def init_state(self, S_pos):
        ws = _ws(256 * 8, S_pos.device)
        _lib.call("qsc_state_init", _lib.ptr(self.state), _lib.ptr(S_pos), self.R, self.obs.Pp,
                  _lib.ptr(ws), ws.numel(), _lib.stream())

    def read_state(self):
        return _lib.read_state(self.state)

    def field(self, name):
        return _lib.state_field(self.state, name)

    # ---- passes -------------------------------------------------------------------------
    def cpass(self, S_pos, C):
        self.gen += 1
        o = self.obs
        _lib.call("qsc_cpass", self.desc, _lib.ptr(self.c_entries), _lib.ptr(o.c_width), _lib.ptr(o.c_off),
                  _lib.ptr(o.c_kmap), o.model, self.R, _lib.ptr(S_pos), _lib.ptr(C),
                  _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    def cpass_nsq(self, S_pos, C):
        """cpass that also writes every slice's ||S||^2 partial (qsc_cpass_nsq: the K-slab
        C-pass after the all-gather of S, in place of a qsc_slice_nsq launch)."""
        self.gen += 1
        o = self.obs
        _lib.call("qsc_cpass_nsq", self.desc, _lib.ptr(self.c_entries), _lib.ptr(o.c_width),
                  _lib.ptr(o.c_off), _lib.ptr(o.c_kmap), o.model, self.R, _lib.ptr(S_pos),
                  _lib.ptr(C), _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    def cnsq(self):
        """A 1-float view of the workspace slot where the C-pass leaves ||C||^2 of the C it
        read (qsc_pass_cnsq_offset): all-reduced in place by the K-slab solver."""
        off = int(_lib.lib().qsc_pass_cnsq_offset(self.desc, self.R))
        if off < 0 or off % 4:
            raise _lib.QscError("qsc_pass_cnsq_offset failed")
        return self.ws[off:off + 4].view(torch.float32)

    def cfinish(self, C, mode, dC=None, mC=None, vC=None, adam=None, lambda_c=0.0,
                normsq_ext=None, record=True):
        self.gen += 1
        hist, cap = (self.hist, self.hist_cap) if (record and self.hist_cap) else (None, 0)
        _lib.call("qsc_cfinish", self.desc, self.R, _lib.ptr(C), int(mode), _lib.ptr(dC),
                  _lib.ptr(mC), _lib.ptr(vC), adam, float(lambda_c), _lib.ptr(normsq_ext),
                  _lib.ptr(self.state), _lib.ptr(hist), cap, _lib.ptr(self.ws), self.ws.numel(),
                  _lib.stream())

    def spass(self, S_pos, C, mode, dS=None, mS=None, vS=None, adam=None, lambda_s=0.0):
        self.gen += 1
        o = self.obs
        _lib.call("qsc_spass", self.desc, _lib.ptr(self.s_entries), _lib.ptr(o.s_width), _lib.ptr(o.s_off),
                  o.model, self.R, _lib.ptr(S_pos), _lib.ptr(C), int(mode), _lib.ptr(dS),
                  _lib.ptr(mS), _lib.ptr(vS), adam, float(lambda_s), _lib.ptr(self.state),
                  _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    def spass_kslab(self, S_pos, C, dS_rs, chunk_rows, nranks):
        """K-slab S-pass (qsc_spass_kslab): the partial dS into the reduce-scatter buffer dS_rs
        (nranks chunks of chunk_rows rows, each followed by one extra slice holding this slab's
        ||C||^2 in its first element)."""
        self.gen += 1
        o = self.obs
        u = _lib.QSC_SLICE
        if chunk_rows % u:
            raise ValueError("K-slab chunks must be whole position slices")
        _lib.call("qsc_spass_kslab", self.desc, _lib.ptr(self.s_entries), _lib.ptr(o.s_width),
                  _lib.ptr(o.s_off), o.model, self.R, _lib.ptr(S_pos), _lib.ptr(C),
                  _lib.ptr(dS_rs), chunk_rows // u, int(nranks), _lib.ptr(self.state),
                  _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    def scpass_supported(self):
        return bool(_lib.lib().qsc_scpass_supported(self.desc, self.R))

    def scpass(self, S_pos, C, mS, vS, adam, lambda_s):
        """spass (mode 1, Adam) fused with the next cpass at the updated S (qsc_scpass)."""
        self.gen += 1
        o = self.obs
        _lib.call("qsc_scpass", self.desc, _lib.ptr(self.s_entries), _lib.ptr(o.s_width),
                  _lib.ptr(o.s_off), _lib.ptr(self.c_entries), _lib.ptr(o.c_width),
                  _lib.ptr(o.c_off), _lib.ptr(o.c_kmap), o.model, self.R, _lib.ptr(S_pos),
                  _lib.ptr(C), _lib.ptr(mS),
                  _lib.ptr(vS), adam, float(lambda_s), _lib.ptr(self.state), _lib.ptr(self.ws),
                  self.ws.numel(), _lib.stream())

    def supdate(self, S_pos, mS, vS, g, adam, lambda_s):
        self.gen += 1
        _lib.call("qsc_supdate", self.desc, self.R, _lib.ptr(S_pos), _lib.ptr(mS), _lib.ptr(vS),
                  _lib.ptr(g), adam, float(lambda_s), _lib.ptr(self.state), _lib.ptr(self.ws),
                  self.ws.numel(), _lib.stream())

    # K-slab shards: rows are dealt in whole position slices
    row_unit = _lib.QSC_SLICE

    def supdate_rows(self, S_pos, mS, vS, g_own, adam, lambda_s, r0, r1):
        """Adam on position rows [r0, r1) (multiples of QSC_SLICE) from the shard's gradient
        g_own (its first row is row r0) -- qsc_supdate_slices."""
        self.gen += 1
        u = _lib.QSC_SLICE
        if r0 % u or (r1 % u and r1 != self.obs.Pp):
            raise ValueError("shard rows must be whole position slices")
        _lib.call("qsc_supdate_slices", self.desc, self.R, r0 // u, -(-r1 // u), _lib.ptr(S_pos),
                  _lib.ptr(mS), _lib.ptr(vS), _lib.ptr(g_own), adam, float(lambda_s),
                  _lib.ptr(self.state), _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    def slice_nsq(self, S_pos):
        """Every slice's ||S||^2 partial from the (all-gathered) S -- qsc_slice_nsq."""
        self.gen += 1
        _lib.call("qsc_slice_nsq", self.desc, self.R, _lib.ptr(S_pos), _lib.ptr(self.ws),
                  self.ws.numel(), _lib.stream())

    def cupdate(self, C, mC, vC, g, adam, lambda_c, normsq_s_ext=None):
        """C update from an all-reduced gradient g (R*K [+1]) (IJ-slab sharding)."""
        self.gen += 1
        _lib.call("qsc_cupdate", self.R, self.obs.K, _lib.ptr(C), _lib.ptr(mC), _lib.ptr(vC),
                  _lib.ptr(g), adam, float(lambda_c), _lib.ptr(normsq_s_ext),
                  _lib.ptr(self.state), _lib.stream())

    def sumsq(self, x, out):
        """out[0] = ||x||^2 (fixed order, one workgroup; for small vectors such as C)."""
        _lib.call("qsc_sumsq_small", _lib.ptr(x), x.numel(), _lib.ptr(out), _lib.stream())

    def flush(self, record=True):
        hist, cap = (self.hist, self.hist_cap) if (record and self.hist_cap) else (None, 0)
        _lib.call("qsc_state_flush", self.desc, self.R, _lib.ptr(self.state), _lib.ptr(hist),
                  cap, _lib.ptr(self.ws), self.ws.numel(), _lib.stream())

    # ---- smoothness prior ---------------------------------------------------------------
    def _smooth_bufs(self):
        """The prior's workspace (zeroed: its first word is the history step counter), the
        device scalar R(S) of the last call and the per-iteration history (hist_cap rows)."""
        if getattr(self, "smooth_ws", None) is None:
            dev = self.obs.device
            nb = _lib.lib().qsc_smooth_workspace_bytes(self.obs.Pp)
            if nb == 0:
                raise _lib.QscError("the smoothness prior does not support Pp = %d" % self.obs.Pp)
            self.smooth_ws = torch.zeros(int(nb), dtype=torch.uint8, device=dev)
            self.pen = torch.zeros(1, dtype=torch.float32, device=dev)
            self.pen_hist = torch.zeros(max(self.hist_cap, 1), dtype=torch.float32, device=dev)
        return self.smooth_ws

    def smooth_grad(self, S_pos, dS, kind="quad", delta=None, weight=1.0, record=True):
        """dS += weight * grad R(S) (dS None: value only) and R(S) -> self.pen (qsc_smooth_grad);
        with `record` (and a history) the value is also appended to the penalty history, at the
        row the device-side step counter says."""
        ws = self._smooth_bufs()
        code, delta = smooth_kind(kind, delta)
        hist, cap = (self.pen_hist, self.hist_cap) if (record and self.hist_cap) else (None, 0)
        _lib.call("qsc_smooth_grad", _lib.ptr(S_pos), _lib.ptr(self.obs.neighbors()), self.R,
                  self.obs.Pp, code, delta, float(weight), _lib.ptr(dS), _lib.ptr(self.pen),
                  _lib.ptr(hist), cap, _lib.ptr(ws), ws.numel(), _lib.stream())
        return self.pen

    def smooth_history(self):
        """R(S) of every recorded smooth_grad call so far, in order (fp64 list; synchronises)."""
        if getattr(self, "smooth_ws", None) is None:
            return []
        n = min(int(self.smooth_ws[:4].view(torch.int32).item()), self.hist_cap)
        return self.pen_hist[:n].double().cpu().tolist()

    # ---- composite ----------------------------------------------------------------------
    def nll_grad(self, S_pos, C, need_dS=True, need_dC=True):
        """NLL (device scalar) and its gradients dS (position order) and dC, no regularisers."""
        dS = torch.empty_like(S_pos) if need_dS else None
        dC = torch.empty_like(C) if need_dC else None
        if need_dC or not need_dS:
            self.cpass(S_pos, C)
            self.cfinish(C, 0, dC=dC if need_dC else torch.empty_like(C), record=False)
        if need_dS:
            self.spass(S_pos, C, 0, dS=dS)
            self.flush(record=False)
            nll = self.field("nll_s").clone()[0]
        else:
            nll = self.field("nll_c").clone()[0]
        return nll, dS, dC


class _ProbitNLLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, C, obs):
        R = S.shape[0]
        eng = PassEngine(obs, R)
        Cd = _dev(C.detach().to(torch.float32)).contiguous()
        S_pos = obs.to_positions(S.detach().reshape(R, -1))
        nll, dS_pos, dC = eng.nll_grad(S_pos, Cd, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        dS = obs.to_pixels(dS_pos, R).reshape(S.shape) if dS_pos is not None else None
        ctx.save_for_backward(*(t for t in (dS, dC) if t is not None))
        ctx.has = (dS is not None, dC is not None)
        return nll

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        dS = saved.pop(0) * g if ctx.has[0] else None
        dC = saved.pop(0) * g if ctx.has[1] else None
        return dS, dC, None


class ProbitNLL:
    """-sum(Wx * log(prob_probit(Y, T_hat, b, std))) with T_hat = get_tensor(S, C) (optionally
    log(T_hat + offset)), evaluated by the fused HIP passes over observed entries only.

    Replaces the reference's get_tensor -> log -> prob_probit -> log -> masked sum chain
    (qmc/qmc.ipynb :568-572) and its autograd backward.  The likelihood is the one `obs` was
    packed with (Observations(loss=...)): probit, logit (prob_logit in place of prob_probit) or
    the squared criterion.  Usage:
        nll = ProbitNLL.apply(S, C, obs); (nll + lam*torch.norm(C)).backward()
    """

    @staticmethod
    def apply(S, C, obs):
        if S.dim() == 3:
            S = S.unsqueeze(1)
        return _ProbitNLLFn.apply(S, C, obs)


def smooth_penalty(S, kind="quad", delta=None):
    """(R(S), grad R(S)) of the smoothness prior solve(smooth=...) adds, for loss fields S in
    pixel order, a (R,1,I,J) or (R,I,J) GPU tensor: R(S) a 0-dim fp32 GPU tensor (unweighted), the
    gradient shaped like S.  Runs the solver's own kernel (qsc_smooth_grad) on the identity
    pixel order, so it evaluates exactly the prior the solver applies."""
    from .obs import neighbor_table
    code, delta = smooth_kind(kind, delta)
    _lib.require_device(S)
    R, I, J = S.shape[0], S.shape[-2], S.shape[-1]
    P = I * J
    RP = int(_lib.lib().qsc_rank_pad(R))
    if RP == 0:
        raise ValueError("rank R must be in [1, %d]" % _lib.QSC_MAX_R)
    dev = S.device
    nat = S.detach().to(torch.float32).reshape(R, P).contiguous()
    perm = torch.arange(P, dtype=torch.int32, device=dev)
    nbr = neighbor_table(perm, I, J)
    pos = torch.empty((P, RP), dtype=torch.float32, device=dev)
    _lib.call("qsc_perm_gather", _lib.ptr(nat), _lib.ptr(perm), R, P, P, _lib.ptr(pos),
              _lib.stream())
    g_pos = torch.zeros_like(pos)
    ws = torch.zeros(int(_lib.lib().qsc_smooth_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    pen = torch.zeros(1, dtype=torch.float32, device=dev)
    _lib.call("qsc_smooth_grad", _lib.ptr(pos), _lib.ptr(nbr), R, P, code, delta, 1.0,
              _lib.ptr(g_pos), _lib.ptr(pen), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream())
    grad = torch.empty((R, P), dtype=torch.float32, device=dev)
    _lib.call("qsc_perm_scatter", _lib.ptr(g_pos), _lib.ptr(perm), R, P, P, _lib.ptr(grad),
              _lib.stream())
    return pen[0], grad.reshape(S.shape)
