"""How the alternating solvers issue their runs: the hipGraph mechanics, the one capture routine,
the base class AlternatingSolver that states what the run driver asks of a solver (DESIGN.md has
the table), and the one rule that turns the engine's history rows into costs.  Host code only,
and nothing of the package's own is imported here."""
import ctypes
import math
import time
import warnings

import torch

# Longest run captured as one hipGraph; longer runs replay several (results are identical:
# run(a) then run(b) equals run(a + b) bit for bit, tests/test_gpu_fused.py).
GRAPH_MAX_ITERS = 1024

# RCCL's watchdog thread (torch ProcessGroupNCCL) polls the completion events of the eager
# collectives still on its list every ~100 ms.  Polled while the collectives' stream is being
# captured, such an event fails the query ("operation not permitted on an event last recorded in
# a capturing stream") and the watchdog aborts the process -- seen on MI355X when a capture
# followed an eager collective within milliseconds (profiles/r06/capture_watchdog_abort.log).
# Before capturing collectives: drain the device, then let the watchdog retire its list.
CAPTURE_QUIESCE_S = 0.3


def quiesce_collectives(dist):
    try:
        nccl = dist is not None and dist.is_initialized() and dist.get_backend() == "nccl"
    except (AttributeError, RuntimeError, ValueError):  # (a stand-in process group)
        nccl = False
    if not nccl:
        return
    torch.cuda.synchronize()
    time.sleep(CAPTURE_QUIESCE_S)


_hip = None


def _hip_lib():
    global _hip
    if _hip is None:
        h = ctypes.CDLL("libamdhip64.so")
        h.hipGraphUpload.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        h.hipGraphUpload.restype = ctypes.c_int
        h.hipStreamIsCapturing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        h.hipStreamIsCapturing.restype = ctypes.c_int
        h.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        h.hipStreamEndCapture.restype = ctypes.c_int
        h.hipGraphDestroy.argtypes = [ctypes.c_void_p]
        h.hipGraphDestroy.restype = ctypes.c_int
        h.hipGetLastError.argtypes = []
        h.hipGetLastError.restype = ctypes.c_int
        _hip = h
    return _hip


def capture_stream():
    """A side stream that is not in a capture: torch hands out streams from a fixed pool
    (round robin), and a stream whose capture was invalidated stays invalidated for good
    (abandon_capture), so after a failed capture the pool can return such a stream again;
    skip those."""
    for _ in range(4 * 32 + 1):  # torch's pool holds 32 streams per priority
        s = torch.cuda.Stream()
        if stream_capture_status(s) == 0:
            return s
    raise RuntimeError("no side stream out of capture for hipGraph capture")


def stream_capture_status(stream):
    """0 = not capturing, 1 = capture active, 2 = capture invalidated (hipStreamCaptureStatus)."""
    st = ctypes.c_int(0)
    rc = _hip_lib().hipStreamIsCapturing(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(st))
    return st.value if rc == 0 else -1  # -1: the query itself failed (treated as capturing)


def abandon_capture(side, caller):
    """Clean up after a capture on `side` failed: end (and discard) the capture still open on
    it, clear the HIP error state and synchronise the device.  HIP leaves a stream whose
    capture was invalidated in the invalidated state for good (measured, tools/probe/
    capture_fail.py: hipStreamEndCapture returns an error and the status stays 2), so the side
    stream is abandoned -- captures always use a fresh one -- and only the caller's stream,
    where eager work continues, must be out of capture.  Raises RuntimeError otherwise."""
    h = _hip_lib()
    if stream_capture_status(side) != 0:
        graph = ctypes.c_void_p(None)
        h.hipStreamEndCapture(ctypes.c_void_p(side.cuda_stream), ctypes.byref(graph))
        if graph.value:
            h.hipGraphDestroy(graph)
    h.hipGetLastError()  # clear the (non-sticky) capture error
    if stream_capture_status(caller) != 0:
        raise RuntimeError("a failed hipGraph capture left the caller's stream capturing")
    torch.cuda.synchronize()
    h.hipGetLastError()


def _upload(g):
    """hipGraphUpload the instantiated graph now, so that its first replay does not pay the
    upload (a fixed ~tens of us that would otherwise land in a short timed run)."""
    try:
        ex = g.raw_cuda_graph_exec()
        rc = _hip_lib().hipGraphUpload(ex, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError("hipGraphUpload returned %d" % rc)
        torch.cuda.current_stream().synchronize()
    except (OSError, AttributeError, RuntimeError) as e:  # upload is an optimisation only
        warnings.warn("hipGraphUpload skipped (%s)" % e, RuntimeWarning)


def graph_chunks(n, max_iters=GRAPH_MAX_ITERS):
    """The graph lengths run(n) replays, in order: max_iters-iteration chunks, then the rest."""
    out = []
    while n > 0:
        m = min(n, max_iters)
        out.append(m)
        n -= m
    return out


def capture(solver, n):
    """Capture solver.issue(n)'s kernel sequence into a hipGraph on a side stream (in the
    solver's memory pool, if it shares one among its graphs).

    A capture that fails part-way (an engine error, an illegal synchronisation, a collective
    that cannot be captured) is abandoned cleanly: any capture still open on the side stream or
    the current stream is ended and its graph destroyed, and the device is synchronised, BEFORE
    anything else is issued -- work issued onto a stream that is still capturing would be
    recorded instead of run, and a collective there fails ("operation not permitted when stream
    is capturing").  Then, for a tolerant solver, the failure is recorded in `graph_error`, the
    solver is marked not capturable and runs eagerly from then on; otherwise the error is
    re-raised.  If the capture cannot be ended the error is always raised."""
    quiesce_collectives(solver.dist)
    g = torch.cuda.CUDAGraph()
    s = capture_stream()
    caller = torch.cuda.current_stream()
    s.wait_stream(caller)
    mark = solver.capture_mark()
    try:
        with torch.cuda.stream(s):
            # thread-local capture mode: other threads' HIP calls (RCCL's watchdog queries the
            # events of collectives issued before the capture) must neither fail nor invalidate
            # it -- in the default global mode the watchdog's query errors and aborts the process
            with torch.cuda.graph(g, pool=solver.graph_pool, stream=s,
                                  capture_error_mode="thread_local"):
                solver.issue(n)
    except Exception as e:  # noqa: BLE001 - every failure takes the same clean-up path
        solver.capture_restore(mark)
        err = "%s: %s" % (type(e).__name__, e)
        del g
        abandon_capture(s, caller)  # raises if the caller's stream is left capturing
        if not solver.graph_tolerant:
            raise
        solver.graph_error = err
        solver.graph_capturable = False
        warnings.warn("hipGraph capture failed; running eagerly (%s)" % err, RuntimeWarning)
        return None
    solver.capture_restore(mark)  # (capturing executes nothing: the device state is unchanged)
    torch.cuda.current_stream().wait_stream(s)
    _upload(g)
    return g


class AlternatingSolver:
    """What the run driver below asks of a solver, with the defaults of a plain one.

    A solver has `engine` (read_state) and its spectra `C`, and enqueues (no host sync)
    c_step / s_step; the attributes and hooks select the rest of the issue rule (`issue`)."""

    fuse = False              # fused_body exists: S-step i + C-pass i+1 in one launch
    chain = False             # with fuse: runs end with the fused launch (c_finish, fused_last)
    dist = None               # the process group whose collectives the steps issue
    graph_tolerant = False    # a failed capture: True = warn and run eagerly, False = raise
    graph_capturable = True   # False: run eagerly (the reason is in graph_error)
    graph_error = None
    graph_iters = GRAPH_MAX_ITERS  # longest run captured as one graph
    graph_pool = None         # a memory pool shared by the solver's graphs
    # names of the tensors a captured graph holds the addresses of: a solver whose state tensors
    # were swapped for others (sol.C = ...) captures anew instead of replaying into the old storage
    graph_state = ()

    def __init__(self):
        self._graphs, self._graph_ptrs = {}, None

    # ---- what a solver enqueues ----
    def c_step(self):
        """The C-step: the C-pass at the current S, C and its finish (the update of C)."""
        raise NotImplementedError

    def s_step(self):
        """The stand-alone S-step: the S-pass at the current S, C and the update of S."""
        raise NotImplementedError

    def fused_body(self):
        """(fuse) S-step i and C-pass i+1 in one launch, then C-step i+1's finish."""
        raise NotImplementedError

    def c_finish(self):
        """(chain) The C-step's finish alone, on the C-pass a previous run left ahead."""
        raise NotImplementedError

    def fused_last(self):
        """(chain) The run's last S-step fused with the next run's C-pass, left ahead."""
        raise NotImplementedError

    # ---- hooks ----
    def begin_run(self):
        """(at the start of every issued run)"""

    def ahead(self):
        """True when the workspace holds the next iteration's C-pass at the current S, C."""
        return False

    def chain_replayed(self):
        """(after a replayed chaining run: its last fused launch left a C-pass ahead)"""

    def chain_force(self, ahead):
        """Set the chaining state run() starts from; False if the solver cannot be in it."""
        return not ahead

    def capture_mark(self):
        """The host-side state that issuing a run changes (a capture executes nothing)."""
        return None

    def capture_restore(self, mark):
        """Put back what capture_mark returned."""

    def graph_key(self, n):
        """The key of run(n)'s graph in _graphs, from the solver's current state."""
        return n

    # ---- the driver ----
    def iteration(self):
        self.c_step()
        self.s_step()

    def issue(self, n):
        """Enqueue the kernel sequence of n outer iterations (no host sync): two launches per
        iteration, and with `fuse` c_step, fused_body x (n-1), s_step.

        A solver with `chain` (FreeSSolver) ends a run with the fused launch instead of the
        stand-alone S-step: its last S-step also runs the NEXT iteration's C-pass, whose partials
        wait in the workspace (`ahead()`), and a following run starts with that C-pass's finish
        instead of a C-pass of its own.  The op sequence of run(a) then run(b) is then exactly
        that of run(a + b) -- c_step, fused_body x (a + b - 1), then the last S-step -- and every
        run of n iterations issues n fused launches and n C-step finishes (the steady state),
        where the stand-alone ends cost a C-pass and an S-pass per run."""
        self.begin_run()
        if self.fuse and self.chain and n >= 1:
            if self.ahead():
                self.c_finish()
            else:
                self.c_step()
            for _ in range(n - 1):
                self.fused_body()
            self.fused_last()
        elif self.fuse and n >= 2:
            self.c_step()
            for _ in range(n - 1):
                self.fused_body()
            self.s_step()
        else:
            for _ in range(n):
                self.iteration()

    def _on_gpu(self):
        return torch.cuda.is_available() and self.C.is_cuda

    def _graph(self, n):
        """The hipGraph of the exact kernel sequence of run(n) from the solver's current state
        (captured once per graph_key), or None for a solver that runs eagerly."""
        if not self.graph_capturable:
            return None  # eager (the reason is in graph_error)
        ptrs = tuple(vars(self)[a].data_ptr() for a in self.graph_state)
        if self._graph_ptrs != ptrs:
            self._graphs.clear()
            self._graph_ptrs = ptrs
        key = self.graph_key(n)
        if key not in self._graphs:
            self._graphs[key] = capture(self, n)
        return self._graphs[key]

    def prepare(self, n):
        """Capture (without executing) every graph that run(n, use_graph=True) will replay, so a
        later timed run(n) captures, instantiates and uploads nothing (no-op without a GPU)."""
        if not self._on_gpu():
            return
        # A chaining solver's graphs are keyed by whether a C-pass is ahead: run(n) from the
        # current state replays (m, ahead()) for its first chunk and (m, True) for the later ones,
        # and a later run(n) starts with a C-pass ahead.  Capture every entry form the solver can
        # be in of every chunk size, so no later run(n) captures anything wherever it starts.
        mark = self.capture_mark()
        for m in sorted(set(graph_chunks(n, self.graph_iters))):
            for a in (False, True):
                if self.chain_force(a):
                    self._graph(m)
        self.capture_restore(mark)

    def run(self, n, use_graph=False):
        """Enqueue n outer iterations (no host sync): eager, or as replays of whole-run hipGraphs
        (one replay when n <= graph_iters), so the device work of a timed run(n) does not depend
        on how earlier runs were split."""
        if not (use_graph and self._on_gpu()):
            self.issue(n)
            return
        for m in graph_chunks(n, self.graph_iters):
            g = self._graph(m)
            if g is None:
                self.issue(m)
            else:
                g.replay()
                self.chain_replayed()

    def state(self):
        return self.engine.read_state()


def cost_history(rows, nsq_c_final, lambda_c, s_terms):
    """(costs_c, costs_s) from the engine's history rows (nll_c, nll_s, ||C||^2, ||S||^2), one
    per iteration: the C-step's cost at the C it differentiates, the S-step's at the updated C
    (the next row's ||C||^2; nsq_c_final after the last).  s_terms[i] are the terms iteration i
    adds to both after lambda_c ||C||, added left to right."""
    costs_c, costs_s = [], []
    for i, (nll_c, nll_s, nsq_c, _) in enumerate(rows):
        nsq_c_next = rows[i + 1][2] if i + 1 < len(rows) else nsq_c_final
        cost_c = nll_c + lambda_c * math.sqrt(nsq_c)
        cost_s = nll_s + lambda_c * math.sqrt(nsq_c_next)
        for t in s_terms[i]:
            cost_c, cost_s = cost_c + t, cost_s + t
        costs_c.append(cost_c)
        costs_s.append(cost_s)
    return costs_c, costs_s
