"""GPU: the summation orders of the C-step finish (qsc_cfinish), bit for bit.

qsc_cpass leaves the dC slab [ntiles][R][64 nks] and the NLL partials in the pass workspace; the
S-passes leave their per-slice NLL and ||S||^2 partials there.  qsc_cfinish sums them in two fixed
orders, which every solver form shares and which this file re-sums in numpy float32:

  column order     partial w (of 16) sums tiles w, w + 16, ... from +0; the gradient is
                   p0 + p1 + ... + p15 in that order; then g + p coef and the Adam element update.
  canonical order  thread i of 1024 sums items i, i + 1024, ... from +0; then the xor butterfly
                   over each wave of 64 (offsets 32, 16, ..., 1); then the 16 wave sums in order.

mC, vC, dC, the state and the history row are compared bit for bit, and C bit for bit with one of
the three values the update's hardware square root allows (_adam), at the edges of the finish's
mapping: tile counts around the 16 partials and past one batch of 256, bins around the 16-, 32-
and 64-bin groups, ranks 1..16, the three modes, ||C||^2 given or not, every state of `pending`,
partial counts around the 1024 canonical threads and past one batch of 8192, the history absent,
at its last row and past it, and one replay from a captured graph.  (A layout has an even number
of position slices, Pp being a multiple of 64: the slice counts are 2, 1022, 1024 and 1026, and
the C-pass partial count, which goes through the same sum, takes 1, 1023, 1024 and 1025.)"""
import math

import numpy as np
import pytest
import torch

from test_gpu_fused import _random_case

pytestmark = pytest.mark.gpu

F = np.float32
PEND_C, PEND_SNLL, PEND_SUPD = 1, 2, 4
LAMBDA_C = 0.37


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def _fma(a, b, c):
    """fp32 fused multiply-add, correctly rounded: the exact product plus c in fp64, rounded to
    odd (TwoSum gives the sign of the error), then to fp32."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    t = p + c
    bb = t - p
    e = (p - (t - bb)) + (c - bb)
    even = (t.view(np.int64) & 1) == 0
    t = np.where((e != 0) & even, np.nextafter(t, np.where(e > 0, np.inf, -np.inf)), t)
    return t.astype(F)


def _ipow(b, n):
    r = 1.0
    while n > 0:
        if n & 1:
            r *= b
        b *= b
        n >>= 1
    return r


def _adam(p, m, v, g, ad, step):
    """adam_elem (qsc_common.cuh) on fp32 arrays -> (p candidates, m, v).  The moments are exact.
    The pass kernels run with f32 denormals flushed, where the compiler emits the bare
    v_sqrt_f32 for adam_elem's square root: within 1 ulp, not correctly rounded, and not
    reproducible on the host.  So p is given for the correctly rounded root and its two
    neighbours, and the device's p must be one of the three, bit for bit; every other operation
    of the update is correctly rounded on both sides."""
    step_size = F(ad.lr / (1.0 - _ipow(ad.beta1, step)))
    bc2_sqrt = F(math.sqrt(1.0 - _ipow(ad.beta2, step)))
    w1, w2, beta2, eps = F(1.0 - ad.beta1), F(1.0 - ad.beta2), F(ad.beta2), F(ad.eps)
    m = _fma(w1, g - m, m)
    v = _fma(w2 * g, g, v * beta2)
    root = np.sqrt(v)
    cand = []
    for s in (root, np.nextafter(root, F(0.0)), np.nextafter(root, F(np.inf))):
        q = p + (-step_size * m) / (s / bc2_sqrt + eps)
        cand.append(np.where(q < 0, F(0.0), q) if ad.project_nonneg else q)
    return cand, m, v


def _columns(slab):
    """slab [ntiles][R][Kp] -> [R][Kp] in the column order."""
    part = []
    for w in range(16):
        a = np.zeros(slab.shape[1:], F)
        for t in range(w, slab.shape[0], 16):
            a = a + slab[t]
        part.append(a)
    g = part[0]
    for w in range(1, 16):
        g = g + part[w]
    return g


def _canon(x):
    """the canonical total of the items x"""
    n = -(-max(len(x), 1) // 1024) * 1024
    rows = np.zeros(n, F)
    rows[:len(x)] = x
    a = np.zeros(1024, F)
    for row in rows.reshape(-1, 1024):
        a = a + row
    a = a.reshape(16, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lane ^ o]
    r = F(0.0)
    for w in range(16):
        r = r + a[w, 0]
    return r


class _Case:
    """A packed problem with its engine, and the launches that bring the state to `pend`."""

    def __init__(self, seed, R, I, J, K, tile, hist_cap=4):
        from quantized_spectrum_cartography_amd import _lib
        from quantized_spectrum_cartography_amd.fused import PassEngine
        from quantized_spectrum_cartography_amd.obs import Observations
        d = _random_case(seed, R, I, J, K, f=0.3)
        self.R, self.K = R, K
        self.obs = Observations(d["Y"], d["Wx"], d["b"], d["sigma"], R_hint=R, tile=tile)
        self.e = PassEngine(self.obs, R, hist_cap=hist_cap)
        if hist_cap:  # room behind the last row, to see a write past it
            self.e.hist = torch.full((4 * hist_cap + 8,), -7.0, device="cuda")
        self.S = self.obs.to_positions(d["S0"].reshape(R, -1))
        self.C = d["C0"].reshape(R, K).cuda().contiguous()
        g = torch.Generator().manual_seed(seed)
        self.mC = (0.01 * torch.randn(R, K, generator=g)).cuda()
        self.vC = (1e-4 * torch.rand(R, K, generator=g)).cuda()
        self.mS, self.vS = torch.zeros_like(self.S), torch.zeros_like(self.S)
        self.adam_c = _lib.make_adam(5e-3, project_nonneg=True)
        self.adam_s = _lib.make_adam(1e-2)
        self.e.init_state(self.S)
        dsc = self.e.desc
        self.ntiles, self.nks, self.nslices = dsc.ntiles, dsc.nks, dsc.Pp // 32
        L = _lib.lib()
        self.off = [int(L.qsc_pass_part_offset(dsc, R, w)) for w in range(4)]
        assert all(o >= 0 and o % 4 == 0 for o in self.off)
        assert int(L.qsc_pass_part_offset(dsc, R, 4)) == -1

    def part(self, which, n):
        o = self.off[which]
        return self.e.ws[o:o + 4 * n].view(torch.float32)

    def prepare(self, pend):
        e = self.e
        step = lambda: e.cfinish(self.C, 1, mC=self.mC, vC=self.vC, adam=self.adam_c,
                                 lambda_c=LAMBDA_C)
        if pend == "snll":
            e.spass(self.S, self.C, 0, dS=torch.empty_like(self.S))
        elif pend == "snll2":  # two S-passes: the history row of the second
            for _ in range(2):
                e.spass(self.S, self.C, 0, dS=torch.empty_like(self.S))
        elif pend == "supd":   # a whole iteration first: the Adam scalars come from the cache
            e.cpass(self.S, self.C)
            step()
            e.spass(self.S, self.C, 1, mS=self.mS, vS=self.vS, adam=self.adam_s, lambda_s=0.1)
        elif pend == "c":
            e.cpass(self.S, self.C)
            step()
        e.cpass(self.S, self.C)
        # partials that are not pending must not reach the state: poison them
        if pend in ("none", "c"):
            self.part(2, self.nslices).fill_(float("nan"))
        if pend in ("none", "c", "snll", "snll2"):
            self.part(3, self.nslices).fill_(float("nan"))
        torch.cuda.synchronize()
        want = {"none": 0, "c": PEND_C, "snll": PEND_SNLL, "snll2": PEND_SNLL,
                "supd": PEND_SNLL | PEND_SUPD}[pend]
        assert e.read_state()["pending"] == want


def _check(c, mode, ext, graph=False):
    """Run the finish on the prepared case and compare everything it writes."""
    e, R, K = c.e, c.R, c.K
    Kp = 64 * c.nks
    st = e.read_state()
    slab = c.part(0, c.ntiles * R * Kp).cpu().numpy().reshape(c.ntiles, R, Kp)
    cnll = c.part(1, c.ntiles * c.nks).cpu().numpy()
    snll = c.part(2, c.nslices).cpu().numpy()
    snsq = c.part(3, c.nslices).cpu().numpy()
    C0, m0, v0 = (x.cpu().numpy().copy() for x in (c.C, c.mC, c.vC))
    hist0 = e.hist.cpu().numpy().copy()
    cap = e.hist_cap
    normsq_ext = torch.tensor([3.25], device="cuda") if ext else None
    nsq = F(3.25) if ext else F(e.cnsq().item())
    dC = torch.full((R * K + 1,), -5.0, device="cuda")

    def run():
        if mode == 1:
            e.cfinish(c.C, 1, mC=c.mC, vC=c.vC, adam=c.adam_c, lambda_c=LAMBDA_C,
                      normsq_ext=normsq_ext)
        else:
            e.cfinish(c.C, mode, dC=dC, normsq_ext=normsq_ext)
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run()
        g.replay()
    else:
        run()
    torch.cuda.synchronize()

    # ---- the book-keeping ----
    want = dict(st)
    hist = hist0.copy()
    pend = st["pending"]
    if pend & (PEND_SNLL | PEND_SUPD):
        nll_s = _canon(snll)
        want["nll_s"] = float(nll_s)
        it = st["iter"] - 1
        if cap and 0 <= it < cap:
            hist[4 * it:4 * it + 4] = [st["nll_c"], nll_s, st["normsq_c"], st["normsq_s_prev"]]
        if pend & PEND_SUPD:
            want["normsq_s"] = float(_canon(snsq))
            want["step_s"] = st["step_s"] + 1
        pend &= ~(PEND_SNLL | PEND_SUPD)
    want["nll_c"] = float(_canon(cnll))
    if mode == 1:
        want["normsq_c"] = float(nsq)
        pend |= PEND_C
    want["pending"] = pend
    got = e.read_state()
    for k in want:
        if isinstance(want[k], float):
            assert _bits(got[k]) == _bits(want[k]), (k, got[k], want[k])
        else:
            assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(_bits(e.hist.cpu().numpy()), _bits(hist))

    # ---- the columns ----
    g = _columns(slab)[:, :K]
    if mode == 1:
        nrm = np.sqrt(nsq)
        coef = F(LAMBDA_C) / nrm if nrm > 0 else F(0.0)
        ps, m, v = _adam(C0, m0, v0, g + C0 * coef, c.adam_c, st["step_c"] + 1)
        for name, a, b in (("mC", c.mC, m), ("vC", c.vC, v)):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b)), name
        got_c = _bits(c.C.cpu().numpy())
        assert np.all((got_c == _bits(ps[0])) | (got_c == _bits(ps[1])) | (got_c == _bits(ps[2])))
        print("C: %d of %d elements off the correctly rounded root's value"
              % (int((got_c != _bits(ps[0])).sum()), got_c.size))
        assert bool((dC == -5.0).all())
    else:
        out = dC.cpu().numpy()
        assert np.array_equal(_bits(out[:R * K].reshape(R, K)), _bits(g))
        tail = want["normsq_s"] if mode == 2 else -5.0
        assert _bits(out[R * K]) == _bits(tail)
        for a, b in ((c.C, C0), (c.mC, m0), (c.vC, v0)):
            assert np.array_equal(_bits(a.cpu().numpy()), _bits(b))


# ntiles = I (64-position tiles, J = 64): around the 16 partials; K around the 16-, 32- and
# 64-bin groups; every rank class, mode and state of `pending`
@pytest.mark.parametrize("ntiles,K,R,mode,ext,pend", [
    (1, 1, 1, 1, False, "none"),
    (15, 15, 3, 1, False, "supd"),
    (16, 16, 8, 1, True, "supd"),
    (17, 17, 16, 1, False, "snll"),
    (33, 63, 3, 0, False, "snll"),
    (33, 64, 8, 2, False, "supd"),
    (17, 65, 1, 1, False, "c"),
    (16, 130, 16, 1, True, "none"),
    (15, 130, 3, 2, True, "none"),
    (1, 33, 8, 0, False, "c"),
])
def test_finish_orders_at_the_mapping_edges(ntiles, K, R, mode, ext, pend):
    c = _Case(100 + ntiles + K, R, ntiles, 64, K, 64)
    assert c.ntiles == ntiles
    c.prepare(pend)
    _check(c, mode, ext)


# partial counts around the 1024 canonical threads: slices (S-pass partials) and tiles x k-slices
# (C-pass partials); and past one batch of both sums (8192 slices, 256 tiles)
@pytest.mark.parametrize("I,J,tile,K,R,nslices,nc", [
    (511, 64, 64, 1, 1, 1022, 511),
    (512, 64, 64, 65, 3, 1024, 1024),
    (513, 64, 64, 1, 1, 1026, 513),
    (341, 64, 64, 130, 3, 682, 1023),
    (205, 64, 64, 260, 1, 410, 1025),
    (257, 1024, 1024, 1, 1, 8224, 257),
])
def test_finish_orders_at_the_partial_counts(I, J, tile, K, R, nslices, nc):
    c = _Case(200 + I, R, I, J, K, tile)
    assert (c.nslices, c.ntiles * c.nks) == (nslices, nc)
    c.prepare("supd")
    _check(c, 1, False)


@pytest.mark.parametrize("hist_cap,pend,written", [(0, "snll", False), (1, "snll", True),
                                                   (1, "snll2", False)])
def test_finish_history_absent_last_row_and_past_it(hist_cap, pend, written):
    c = _Case(301, 3, 17, 64, 40, 64, hist_cap=hist_cap)
    c.prepare(pend)
    before = c.e.hist.clone()
    _check(c, 1, False)
    assert bool((c.e.hist != before).any()) == written


def test_finish_replayed_from_a_captured_graph():
    c = _Case(302, 8, 33, 64, 130, 64)
    c.prepare("supd")
    _check(c, 1, False, graph=True)
