"""Observation sets: the quantized, sparsely sampled map packed for the fused HIP passes.

The reference keeps the observation as a dense int64 tensor Y (K,1,I,J) plus a dense float
mask Wx (qmc/qmc.ipynb :493, :537) and evaluates every entry.  `Observations` folds the mask
into uint8 codes (0xFF = unobserved), then packs only the observed entries into the two
sliced formats of include/qsc.h (one per pass), with pixels re-ordered by observation count
so that the 64 lanes of every wavefront carry near-equal work.  Built once per solve.
"""
import ctypes
import os

import torch

from . import _lib
from ._model import _dev, _ws


def ctypes_copy(dst, src):
    """Field-by-field copy of a ctypes Structure."""
    for name, _ in src._fields_:
        setattr(dst, name, getattr(src, name))


def _seed64(seed):  # an int seed in [-2^63, 2^64) as a signed 64-bit value
    if not -2 ** 63 <= seed < 2 ** 64:
        raise ValueError("seed must fit 64 bits, got %r" % (seed,))
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def _check_perm(perm):  # the pixel order of a derived packing: this object's, or by the new counts
    if perm not in ("keep", "fresh"):
        raise ValueError('perm must be "keep" or "fresh", got %r' % (perm,))


def default_tile(P, R, K):
    """C-pass pixel tile (positions, a power of two in [256, 1024]; 128 at rank 16 when LDS
    requires it).

    The C-pass runs one 4-wave workgroup per (tile, 64-bin slice): aim for ~1024 workgroups
    (4 per CU) while keeping tiles large, since the per-bin lists of a tile are padded to their
    longest (bigger tiles -> relatively less padding) and the tile's S rows live in LDS.  At
    least 256 positions: the fused launch (one workgroup per tile) then runs two S-step slices
    per wave and its C-finish sums half as many tiles -- C2 (256^2 x 64) 131.4 k grad-steps/s
    at 256 against 129.8 k at 128 (profiles/r04/fin_small_wg/ab_c2*.log)."""
    if os.environ.get("QSC_CTILE"):  # tuning override (power of two, 64..4096)
        return int(os.environ["QSC_CTILE"])
    Pp = -(-P // 64) * 64
    nks = -(-K // 64)
    if R <= 8:
        # the tile-form C-pass and the fused launch run one workgroup per tile: ~256 tiles (one
        # round on the 256 CUs) whatever K is.  Sizing by tiles x k-slices (the per-slice C-pass
        # form's rule) gave the K-slab shares of C3 (K_loc = 32, 64) 256-position tiles and 4x
        # the slab rows to finish: c3k8 C-finish 6.87 us at 256 positions, 3.26 us at 1024, C-pass
        # 9.81 / 9.57 us (profiles/r06/kslab/c3k8_tiles.log)
        t = 256
        while t * 256 < Pp and t < 1024:
            t *= 2
        return t
    want = max(1, (Pp * nks) // 1024)
    t = 256
    while t * 2 <= want and t < 1024:
        t *= 2
    if R > 8:
        # rank 16: the fused S-step + C-pass launch holds C^T and the S tile at a 20-float
        # pitch in LDS (scfused_lds, qsc_pass_host.cuh); halve the tile until both fit, with the
        # part-sum area of the largest part count it may use
        parts = 1 if nks >= 16 else 16 // nks
        part_sum = 16 * 64 * 4 * nks * parts if parts > 1 else 0
        while t > 128 and 32 + K * 80 + 2048 + t * 80 + part_sum + 64 > 160 * 1024:
            t //= 2
    return t


def neighbor_table(perm, I, J):
    """(Pp, 4) int32 neighbour positions (left, right, up, down; -1 = none) of the pixel order
    `perm` ((Pp,) int32 on the GPU, -1 = padding) over the I x J grid: qsc_smooth_neighbors."""
    _lib.require_device(perm)
    Pp = perm.numel()
    nb = _lib.lib().qsc_smooth_workspace_bytes(Pp)
    if nb == 0:
        raise _lib.QscError("qsc_smooth_workspace_bytes: %d positions are out of range" % Pp)
    ws = _ws(nb, perm.device)
    nbr = torch.empty((Pp, 4), dtype=torch.int32, device=perm.device)
    _lib.call("qsc_smooth_neighbors", _lib.ptr(perm), I * J, Pp, I, J, _lib.ptr(nbr),
              _lib.ptr(ws), ws.numel(), _lib.stream())
    return nbr


class _Folds:
    """Observations.folds: fold f -> (train, test), built on access."""

    def __init__(self, obs, n, seed64):
        self.obs, self.n, self.seed64 = obs, n, seed64

    def __len__(self):
        return self.n

    def __getitem__(self, f):
        if isinstance(f, bool) or not isinstance(f, int):
            raise TypeError("fold index must be an int")
        if f < 0:
            f += self.n
        if not 0 <= f < self.n:
            raise IndexError("fold %d of %d" % (f, self.n))
        o = self.obs
        lo, hi = o.fold_range(f, self.n)
        return (o._subset(None, None, self.seed64, lo, hi, 1, o.perm),
                o._subset(None, None, self.seed64, lo, hi, 0, o.perm))

    def __iter__(self):
        return (self[f] for f in range(self.n))


class Observations:
    """Packed observations of one K-slab.

    Args:
      Y: bin indices, (K,1,I,J) or (K,I,J) integer tensor (quantize output).
      Wx: sampling mask of the same shape (0/1 floats) or None (all observed).
      bin_boundaries, noise_std, offset, log_model: the probit model (see quantization_model*).
      perm: optional (Pp,) int32 pixel order shared across ranks (K-slab sharding).
      tile: optional C-pass tile size (positions, multiple of 64).
      loss: "probit" (the likelihood of qmc/qmc.ipynb), "squared" (the Euclidean criterion
            ||Wx (T_hat - Obs)||^2 of qmc/qmc_dowjons.ipynb :142, Obs the bin midpoints) or
            "logit" (the ordered-logit likelihood: F_probit replaced by the logistic
            F(y) = 1 / (1 + exp(-y / s)); noise_std is then the logistic scale s, the noise
            standard deviation being s pi / sqrt(3)).
      schedule: order every packed list for bank-conflict-free LDS gathers (qsc_obs_schedule;
            default on, QSC_SCHEDULE=0 turns it off).  Results change only by summation order.
    """

    def __init__(self, Y, Wx, bin_boundaries, noise_std, offset=0.0, log_model=False, perm=None,
                 tile=None, R_hint=8, count_hook=None, loss="probit", schedule=None):
        K = Y.shape[0]
        I, J = Y.shape[-2], Y.shape[-1]
        PT, nbins = self._setup(K, I, J, bin_boundaries, noise_std, offset, log_model, tile,
                                R_hint, loss, schedule)
        P = self.P
        Yd = _dev(Y.reshape(K, P).to(torch.int64))
        dev = Yd.device
        self.device = dev
        Wd = _dev(Wx.reshape(K, P).to(torch.float32)) if Wx is not None else None
        codes = torch.empty((K, P), dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("qsc_pack_codes", _lib.ptr(Yd), _lib.ptr(Wd), K * P, nbins, _lib.ptr(codes),
                  _lib.ptr(bad), _lib.stream())
        nbad = int(bad.item())
        if nbad:
            raise ValueError("%d observed entries have a code outside [0, %d) or a sampling "
                             "weight other than 0/1" % (nbad, nbins))
        self._pack_codes(codes, perm, count_hook, PT, nbins, R_hint)

    def _pack_codes(self, codes, perm, count_hook, PT, nbins, R_hint):
        """Construction from the dense codes on (after _setup): count, order, layout, fill."""
        K, P, dev = self.K, self.P, self.device
        self.codes = codes
        s = _lib.stream()
        cnt = torch.empty(P, dtype=torch.int32, device=dev)
        _lib.call("qsc_obs_count", _lib.ptr(codes), K, P, _lib.ptr(cnt), s)
        self.counts = cnt
        perm = self._order(cnt, perm, count_hook)
        self._alloc_tables(PT)
        desc = _lib.QscObsDesc()
        ws = _ws(_lib.lib().qsc_obs_layout_workspace_bytes(K, P, PT), dev)
        _lib.call("qsc_obs_layout", _lib.ptr(codes), K, P, PT, nbins, _lib.ptr(perm), _lib.ptr(cnt),
                  _lib.ptr(self.s_width), _lib.ptr(self.s_off), _lib.ptr(self.c_width),
                  _lib.ptr(self.c_off), _lib.ptr(self.c_kmap), _lib.ptr(ws), ws.numel(), desc, s)
        self._finish(desc, R_hint)

    def _setup(self, K, I, J, bin_boundaries, noise_std, offset, log_model, tile, R_hint, loss,
               schedule):
        """The part of construction that needs no device: shape, tile, model.  -> (PT, nbins)"""
        P = I * J
        if schedule is None:  # QSC_SCHEDULE=0: natural list order (A/B switch)
            schedule = os.environ.get("QSC_SCHEDULE", "1") != "0"
        self.schedule = bool(schedule)
        self.K, self.I, self.J, self.P = K, I, J, P
        self.R_hint = int(R_hint)
        PT = int(tile or default_tile(P, R_hint, K))
        if PT < 64 or PT % 64:
            raise ValueError("tile must be a positive multiple of 64")
        self.Pp = -(-P // PT) * PT  # whole tiles; padding positions carry no observations
        self.model = _lib.make_model(bin_boundaries, noise_std, offset if log_model else 0.0,
                                     log_model, loss=loss)
        self.loss = loss
        self.log_model = bool(log_model)
        self.noise_std = float(noise_std)
        self.offset = float(offset or 0.0)
        self.bin_boundaries = [float(x) for x in (bin_boundaries.tolist() if isinstance(
            bin_boundaries, torch.Tensor) else bin_boundaries)]
        nbins = len(self.bin_boundaries) - 1
        if nbins > 254:
            raise ValueError("at most 254 bins are supported (code 0xFF marks unobserved)")
        return PT, nbins

    def _order(self, cnt, perm, count_hook):
        """The pixel order: by observation count (qsc_obs_order), or the caller's perm."""
        dev, P = self.device, self.P
        if perm is None:
            # count_hook (e.g. an all-reduce over K-slab ranks) makes the pixel order a function
            # of the global counts, so every rank lays S out identically
            order_cnt = count_hook(cnt.clone()) if count_hook is not None else cnt
            perm = torch.empty(self.Pp, dtype=torch.int32, device=dev)
            ws = _ws(_lib.lib().qsc_obs_order_workspace_bytes(P), dev)
            _lib.call("qsc_obs_order", _lib.ptr(order_cnt), P, self.Pp, _lib.ptr(perm), _lib.ptr(ws),
                      ws.numel(), _lib.stream())
        else:
            perm = _dev(perm.to(torch.int32))
            if perm.numel() != self.Pp:
                raise ValueError("perm must have Pp = %d entries" % self.Pp)
        self.perm = perm
        return perm

    def _alloc_tables(self, PT):
        dev = self.device
        ns, nt, nks = self.Pp // _lib.QSC_SLICE, self.Pp // PT, -(-self.K // 64)
        self.s_width = torch.empty(ns, dtype=torch.int32, device=dev)
        self.s_off = torch.empty(ns + 1, dtype=torch.int64, device=dev)
        self.c_width = torch.empty(nt * nks, dtype=torch.int32, device=dev)
        self.c_off = torch.empty(nt * nks + 1, dtype=torch.int64, device=dev)
        self.c_kmap = torch.empty(nt * nks * 64, dtype=torch.int32, device=dev)

    def _finish(self, desc, R_hint):
        dev = self.device
        self.desc = desc
        et = torch.int32 if desc.wide else torch.int16
        self.s_entries = torch.empty(desc.s_entries, dtype=et, device=dev)
        self.c_entries = torch.empty(desc.c_entries, dtype=et, device=dev)
        rowfmt = 1 if self.signed_rows_ok(R_hint) else 0
        desc.rowfmt = rowfmt
        # signed-row entries (include/qsc.h rowfmt 1: the one-bit kind reads each entry's code
        # through the gathered row) wherever the passes' doubled tables fit at this rank
        self._fill(rowfmt)

    @staticmethod
    def check_readings(k, i, j, code, shape, tile=None):
        """Host-side checks of a list of readings, before any device call: four 1-D integer
        tensors of one length n >= 1, shape = (K, I, J) positive, tile a multiple of 64.
        -> (K, I, J, n).  Raises ValueError."""
        try:
            K, I, J = (int(x) for x in shape)
        except (TypeError, ValueError):
            raise ValueError("shape must be (K, I, J), got %r" % (shape,))
        if K < 1 or I < 1 or J < 1 or I * J >= 2 ** 31:
            raise ValueError("shape (K, I, J) must be positive with I * J < 2^31, got %r"
                             % (shape,))
        if tile is not None and (int(tile) < 64 or int(tile) % 64):
            raise ValueError("tile must be a positive multiple of 64")
        ints = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
        for name, t in (("k", k), ("i", i), ("j", j), ("code", code)):
            if not isinstance(t, torch.Tensor) or t.dim() != 1:
                raise ValueError("%s must be a 1-D tensor" % name)
            if t.dtype not in ints:
                raise ValueError("%s must have an integer dtype, got %s" % (name, t.dtype))
        n = k.numel()
        if not (i.numel() == j.numel() == code.numel() == n):
            raise ValueError("k, i, j and code must have one length, got %d, %d, %d, %d"
                             % (n, i.numel(), j.numel(), code.numel()))
        if n < 1:
            raise ValueError("need at least one reading")
        if n >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 readings are supported, got %d" % n)
        return K, I, J, n

    @classmethod
    def from_readings(cls, k, i, j, code, shape, bin_boundaries, noise_std, offset=0.0,
                      log_model=False, perm=None, tile=None, R_hint=8, count_hook=None,
                      loss="probit", schedule=None):
        """Packed observations from a list of readings: reading e says that bin k[e] at pixel
        (i[e], j[e]) of the shape = (K, I, J) map was observed with code code[e].  The four 1-D
        integer tensors may be in any order, and a cell may be read any number of times: every
        reading is one independent observation (its likelihood term is added).  The other
        arguments are the constructor's.  Packing is qsc_obs_readings_* (include/qsc.h): its cost
        follows the number of readings, not K I J, and no dense array is formed; without
        repeated cells the result is bit-identical to the constructor's on the equivalent Y, Wx.
        On the result `codes` is None, `counts` the per-pixel number of readings, `nnz` the
        number of readings, and stats() gains max_repeat.
        Raises ValueError for lists of unequal length, non-integer dtypes, no readings, a shape
        or tile out of range (before any device call), and with the number of readings whose k,
        (i, j) or code is out of range."""
        K, I, J, n = cls.check_readings(k, i, j, code, shape, tile)
        self = cls.__new__(cls)
        PT, nbins = self._setup(K, I, J, bin_boundaries, noise_std, offset, log_model, tile,
                                R_hint, loss, schedule)
        kd, pd, cd = self._device_readings(k, i, j, code, I, J)
        self.device = kd.device
        self._pack_readings(kd, pd, cd, n, perm, count_hook, PT, nbins, R_hint)
        return self

    @staticmethod
    def _device_readings(k, i, j, code, I, J):
        """Checked host or device lists -> the device lists the packing kernels take: int32 k,
        int32 p = i J + j, uint8 or int32 code (None: no codes)."""
        # (values past int32 stay out of range instead of wrapping into it)
        kd = _dev(k).to(torch.int64).clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
        # p = i J + j in int64 with out-of-grid (i, j) mapped to -1 (counted by the device)
        i64, j64 = _dev(i).to(torch.int64), _dev(j).to(torch.int64)
        inside = (i64 >= 0) & (i64 < I) & (j64 >= 0) & (j64 < J)
        pd = torch.where(inside, i64 * J + j64, torch.full_like(i64, -1)).to(torch.int32)
        if code is None:
            return kd, pd, None
        cd = _dev(code)
        cd = (cd if cd.dtype == torch.uint8 else
              cd.to(torch.int64).clamp(-1, 1 << 20).to(torch.int32)).contiguous()
        return kd, pd, cd

    def _pack_readings(self, kd, pd, cd, n, perm, count_hook, PT, nbins, R_hint, cnt=None):
        """from_readings from the device lists on (after _setup): int32 k, int32 p = i J + j,
        uint8 or int32 code, n of each: count, order, layout (two sorts), fill.  cnt: the
        per-pixel counts of a list the caller has counted and found in range already (append)."""
        K, I, J, P, dev = self.K, self.I, self.J, self.P, self.device
        cb = 1 if cd.dtype == torch.uint8 else 4
        s = _lib.stream()
        if cnt is None:
            cnt = torch.empty(P, dtype=torch.int32, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call("qsc_obs_readings_count", _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(cd), cb, n, K,
                      P, nbins, _lib.ptr(cnt), _lib.ptr(bad), s)
            nbad = int(bad.item())
            if nbad:
                raise ValueError("%d of %d readings have k outside [0, %d), (i, j) outside the "
                                 "%d x %d grid or a code outside [0, %d)"
                                 % (nbad, n, K, I, J, nbins))
        self.codes = None
        self.counts = cnt
        perm = self._order(cnt, perm, count_hook)
        self._alloc_tables(PT)
        L = _lib.lib()
        nb = L.qsc_obs_readings_packed_bytes(n, K, P, PT)
        wb = L.qsc_obs_readings_workspace_bytes(n, K, P, PT)
        if nb == 0 or wb == 0:
            raise ValueError("the shape %r with tile %d is out of the packing's range"
                             % ((K, I, J), PT))
        self._packed = torch.empty(nb, dtype=torch.uint8, device=dev)
        self._n = n
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)  # (32 n: not kept in the ws cache)
        desc = _lib.QscObsDesc()
        rep = ctypes.c_int32(0)
        _lib.call("qsc_obs_readings_layout", _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(cd), cb, n, K, P,
                  PT, nbins, _lib.ptr(perm), _lib.ptr(cnt), _lib.ptr(self.s_width),
                  _lib.ptr(self.s_off), _lib.ptr(self.c_width), _lib.ptr(self.c_off),
                  _lib.ptr(self.c_kmap), _lib.ptr(self._packed), nb, _lib.ptr(ws), wb, desc,
                  ctypes.byref(rep), s)
        del ws
        if int(desc.nnz) != n:  # a caller's perm that gives some read pixel no position
            raise ValueError("perm places only %d of the %d readings: every pixel that has a "
                             "reading needs a position" % (int(desc.nnz), n))
        self.max_repeat = int(rep.value)
        self._finish(desc, R_hint)

    def _fill(self, rowfmt, desc=None, s_entries=None, c_entries=None):
        """Pack the entries in format `rowfmt` into (desc, s_entries, c_entries) (default: this
        object's own arrays; only before any pass engine uses them, see layout())."""
        if desc is None:
            if getattr(self, "_engines", 0):
                raise RuntimeError("the packed entries are in use by a pass engine (and maybe a "
                                   "captured hipGraph): re-packing them in place is refused")
            desc, s_entries, c_entries = self.desc, self.s_entries, self.c_entries
        desc.rowfmt = int(rowfmt)
        if self.codes is None:  # from_readings: from the kept sorted readings, no dense codes
            _lib.call("qsc_obs_readings_fill", _lib.ptr(self._packed), self._packed.numel(),
                      self._n, desc, _lib.ptr(self.s_width), _lib.ptr(self.s_off),
                      _lib.ptr(self.c_width), _lib.ptr(self.c_off), _lib.ptr(self.c_kmap),
                      _lib.ptr(s_entries), _lib.ptr(c_entries), _lib.stream())
        else:
            _lib.call("qsc_obs_fill", _lib.ptr(self.codes), desc, _lib.ptr(self.perm),
                      _lib.ptr(self.s_width), _lib.ptr(self.s_off), _lib.ptr(self.c_width),
                      _lib.ptr(self.c_off), _lib.ptr(self.c_kmap), _lib.ptr(s_entries),
                      _lib.ptr(c_entries), _lib.stream())
        if self.schedule:
            # bank-conflict-free list order (include/qsc.h qsc_obs_schedule): the same order for
            # both entry formats (it depends only on the row residues), so their results agree
            ws = _ws(_lib.lib().qsc_obs_schedule_workspace_bytes(desc), self.device)
            _lib.call("qsc_obs_schedule", desc, _lib.ptr(self.s_width), _lib.ptr(self.s_off),
                      _lib.ptr(self.c_width), _lib.ptr(self.c_off), _lib.ptr(s_entries),
                      _lib.ptr(c_entries), _lib.ptr(ws), ws.numel(), _lib.stream())

    def with_model(self, noise_std=None, bin_boundaries=None):
        """The same packed observations under another observation model: a new Observations that
        shares the packed arrays, perm and tile and carries a new qsc_model with `noise_std` (for
        loss="logit" the logistic scale) and / or `bin_boundaries` (None: unchanged) -- what
        qmc.fit_noise's result is handed on with.  Nothing but the model is rebuilt: the codes do
        not depend on it.  The row format is re-evaluated for the new model (signed rows need
        the saturating one-bit likelihood); where it changes, the new object gets entry arrays of
        its own, filled by the packing's own fill.  This object is left untouched.
        Raises ValueError when the number of bins changes or noise_std is not positive."""
        import copy
        b = self.bin_boundaries if bin_boundaries is None else bin_boundaries
        if isinstance(b, torch.Tensor):
            b = b.detach().to("cpu", torch.float64).tolist()
        b = [float(x) for x in b]
        if len(b) != len(self.bin_boundaries):
            raise ValueError("with_model keeps the codes: the number of bins cannot change "
                             "(%d boundaries, got %d)" % (len(self.bin_boundaries), len(b)))
        sigma = self.noise_std if noise_std is None else float(noise_std)
        if not sigma > 0.0:
            raise ValueError("noise_std must be > 0, got %r" % (noise_std,))
        new = copy.copy(self)
        new.model = _lib.make_model(b, sigma, self.offset if self.log_model else 0.0,
                                    self.log_model, loss=self.loss)
        new.noise_std, new.bin_boundaries = sigma, b
        new.desc = _lib.QscObsDesc()
        ctypes_copy(new.desc, self.desc)
        R_hint = getattr(self, "R_hint", None)
        if R_hint is not None:
            rowfmt = 1 if new.signed_rows_ok(R_hint) else 0
            if rowfmt != self.desc.rowfmt:
                new.s_entries = torch.empty_like(self.s_entries)
                new.c_entries = torch.empty_like(self.c_entries)
                new._engines, new._code_field = 0, None
                new._fill(rowfmt, new.desc, new.s_entries, new.c_entries)
        return new

    @staticmethod
    def check_resample(loss, K, I, J, S, C, seed=0, replicate=0):
        """Host-side checks of resample's arguments (ValueError), before any device call: a
        likelihood, S (R,1,I,J), (R,I,J) or (R,I J), C (R,K), R <= 16, replicate.  -> R, seed64."""
        if loss == "squared":
            raise ValueError('loss="squared" is not a likelihood: there is nothing to draw from')
        for name, t in (("S", S), ("C", C)):
            if not isinstance(t, torch.Tensor) or t.dim() < 2:
                raise ValueError("%s must be a tensor of at least two dimensions" % name)
        R = int(S.shape[0])
        if not 1 <= R <= _lib.QSC_MAX_R:
            raise ValueError("rank R must be in [1, %d], got %d" % (_lib.QSC_MAX_R, R))
        if tuple(S.shape) not in ((R, 1, I, J), (R, I, J), (R, I * J)):
            raise ValueError("S must be (R, 1, %d, %d) or (R, %d, %d), got %s"
                             % (I, J, I, J, tuple(S.shape)))
        if tuple(C.shape) != (R, K):
            raise ValueError("C must be (%d, %d), got %s" % (R, K, tuple(C.shape)))
        if not 0 <= int(replicate) < 2 ** 31:
            raise ValueError("replicate must be in [0, 2^31), got %r" % (int(replicate),))
        return R, _seed64(int(seed))

    def resample(self, S, C, seed=0, replicate=0):
        """New readings drawn from the model at (S, C) over the same sampling pattern: the draw of
        the parametric bootstrap (fits.bootstrap), of simulation from a truth and of coverage
        checks.  Every observed reading is replaced by a code drawn from the very P_b the
        likelihood evaluates at its cell (include/qsc.h, qsc_draw_codes / qsc_draw_readings, has
        the rule); the generator is counter based, so a reading's draw depends only on (seed,
        replicate, bin, pixel, occurrence of the cell) -- not on the tile, pixel order, schedule,
        entry format or dense / readings input.
        The result is a new Observations: it shares perm, tile, counts, the width / offset / bin
        order tables and the model with this one (they depend on the pattern, not the codes) and
        owns its codes (or sorted readings), descriptor and entry arrays, filled in the row
        format this object has (the schedule is re-run: row residues depend on the codes).  This
        object is left untouched, so hipGraphs captured on it stay valid.  `result.invalid` is a
        device int32 counter of the readings left as they were because T_hat + offset <= 0 (log
        model).  S (R,1,I,J) or (R,I,J), C (R,K).  Raises ValueError for shapes that do not
        match, loss="squared", or seed / replicate out of range, before any device call."""
        import copy
        R, seed64 = self.check_resample(self.loss, self.K, self.I, self.J, S, C, seed, replicate)
        Cd = _dev(C.detach().to(torch.float32)).reshape(R, self.K).contiguous()
        Sd = _dev(S.detach().to(torch.float32)).reshape(R, self.P).contiguous()
        new = copy.copy(self)
        new.invalid = torch.zeros(1, dtype=torch.int32, device=self.device)
        if self.codes is None:
            S_pos = self.to_positions(Sd)
            new._packed = torch.empty_like(self._packed)
            _lib.call("qsc_draw_readings", _lib.ptr(self._packed), self._packed.numel(), self._n,
                      self.desc, _lib.ptr(self.perm), self.model, R, _lib.ptr(S_pos), _lib.ptr(Cd),
                      seed64, int(replicate), _lib.ptr(new._packed), _lib.ptr(new.invalid),
                      _lib.stream())
        else:
            new.codes = torch.empty_like(self.codes)
            _lib.call("qsc_draw_codes", _lib.ptr(self.codes), self.K, self.P, self.model, R,
                      _lib.ptr(Sd), _lib.ptr(Cd), seed64, int(replicate), _lib.ptr(new.codes),
                      _lib.ptr(new.invalid), _lib.stream())
        new.desc = _lib.QscObsDesc()
        ctypes_copy(new.desc, self.desc)
        new.s_entries = torch.empty_like(self.s_entries)
        new.c_entries = torch.empty_like(self.c_entries)
        new._engines, new._code_field = 0, None
        new._fill(self.desc.rowfmt)
        return new

    # ---- subsets: select, split, folds, readings (include/qsc.h, the keep rule) ------------
    RANGE = 1 << 24  # the keep rule's u24 lies in [0, RANGE)

    @staticmethod
    def frac_range(frac):
        """hi of the held-out range [0, hi) of split(frac): round(frac 2^24) in [1, 2^24 - 1]."""
        return min(max(int(round(float(frac) * Observations.RANGE)), 1), Observations.RANGE - 1)

    @staticmethod
    def fold_range(f, n):
        """(lo, hi) of the test range of fold f of n: the n ranges tile [0, 2^24)."""
        return (int(f) << 24) // int(n), ((int(f) + 1) << 24) // int(n)

    @staticmethod
    def check_select(K, I, J, pixels=None, bins=None, perm="keep"):
        """Host-side checks of select's arguments, before any device call: pixels an (I, J) bool
        tensor or None, bins a (K,) bool tensor or None, a perm.  Raises ValueError."""
        for name, t, shape in (("pixels", pixels, (I, J)), ("bins", bins, (K,))):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.bool:
                raise ValueError("%s must be a bool tensor, got %s"
                                 % (name, t.dtype if isinstance(t, torch.Tensor) else type(t)))
            if tuple(t.shape) != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, shape, tuple(t.shape)))
        _check_perm(perm)

    @staticmethod
    def check_split(frac=None, seed=0, n=None, perm="keep"):
        """Host-side checks of split's (frac) and folds' (n) arguments, before any device call:
        0 < frac < 1, 2 <= n <= 65536, int seed, perm.  -> _seed64(seed).  Raises ValueError."""
        if frac is not None:
            try:
                ok = 0.0 < float(frac) < 1.0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("the held-out fraction must be in (0, 1), got %r" % (frac,))
        if n is not None:
            if isinstance(n, bool) or not isinstance(n, int) or not 2 <= n <= 65536:
                raise ValueError("the number of folds must be an int in [2, 65536], got %r" % (n,))
        _check_perm(perm)
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError("seed must be an int, got %r" % (seed,))
        return _seed64(seed)

    def _child(self):
        """A new Observations with this one's shape, model, loss, tile, R_hint and schedule flag
        and nothing packed yet (what _setup leaves)."""
        new = Observations.__new__(Observations)
        for a in ("K", "I", "J", "P", "Pp", "schedule", "model", "loss", "log_model", "noise_std",
                  "offset", "bin_boundaries", "device"):
            setattr(new, a, getattr(self, a))
        new.R_hint = getattr(self, "R_hint", 8)
        return new

    def _masks(self, pixels, bins):
        kp = None if pixels is None else _dev(pixels.reshape(self.P)).to(torch.uint8).contiguous()
        kb = None if bins is None else _dev(bins.reshape(self.K)).to(torch.uint8).contiguous()
        return kp, kb

    def _export(self, kp, kb, seed64, lo, hi, invert):
        """The kept readings as device lists (int32 k, int32 p, uint8 code) and their number
        (read back): qsc_export_codes (ascending (k, p)) or qsc_export_readings ((position, k,
        occurrence))."""
        dev, nnz = self.device, self.nnz
        k = torch.empty(nnz, dtype=torch.int32, device=dev)
        p = torch.empty(nnz, dtype=torch.int32, device=dev)
        c = torch.empty(nnz, dtype=torch.uint8, device=dev)
        m = torch.zeros(1, dtype=torch.int64, device=dev)
        entries = self.K * self.P if self.codes is not None else self._n
        wb = _lib.lib().qsc_export_workspace_bytes(entries)
        if wb == 0:
            raise ValueError("%d entries are out of the export's range" % entries)
        ws = _ws(wb, dev)
        rule = (_lib.ptr(kp), _lib.ptr(kb), seed64, lo, hi, invert, _lib.ptr(k), _lib.ptr(p),
                _lib.ptr(c), _lib.ptr(m), _lib.ptr(ws), ws.numel(), _lib.stream())
        if self.codes is not None:
            _lib.call("qsc_export_codes", _lib.ptr(self.codes), self.K, self.P, *rule)
        else:
            _lib.call("qsc_export_readings", _lib.ptr(self._packed), self._packed.numel(), self._n,
                      self.desc, _lib.ptr(self.perm), *rule)
        return k, p, c, int(m.item())

    def _subset(self, kp, kb, seed64, lo, hi, invert, perm):
        """The Observations over the readings the rule keeps; perm: a (Pp,) pixel order, or None
        for the order by the new counts."""
        new = self._child()
        PT, nbins = int(self.desc.PT), int(self.desc.nbins)
        if self.codes is not None:
            codes = torch.empty_like(self.codes)
            kept = torch.zeros(1, dtype=torch.int64, device=self.device)
            _lib.call("qsc_select_codes", _lib.ptr(self.codes), self.K, self.P, _lib.ptr(kp),
                      _lib.ptr(kb), seed64, lo, hi, invert, _lib.ptr(codes), _lib.ptr(kept),
                      _lib.stream())
            if not int(kept.item()):
                raise ValueError("the selection leaves no reading")
            new._pack_codes(codes, perm, None, PT, nbins, new.R_hint)
        else:
            k, p, c, m = self._export(kp, kb, seed64, lo, hi, invert)
            if not m:
                raise ValueError("the selection leaves no reading")
            new._pack_readings(k[:m], p[:m], c[:m], m, perm, None, PT, nbins, new.R_hint)
        return new

    def select(self, pixels=None, bins=None, perm="keep"):
        """The readings of the kept pixels and bins as a new Observations with this one's model,
        loss, tile, R_hint and schedule flag: pixels an (I, J) bool mask of the pixels to keep,
        bins a (K,) bool mask (None: all) -- e.g. obs.select(pixels=~check.flagged(...)) drops the
        sensors check_fit flags, also where the raw data are gone (resample, with_model,
        calibrate results).  perm="keep" keeps this object's pixel order, so that position-order
        S, information blocks and captured state stay compatible and the result is a valid
        obs_holdout partner; perm="fresh" orders the pixels by the new counts.  On the device
        (include/qsc.h, the keep rule): dense codes are masked by qsc_select_codes and packed by
        the constructor's own count / layout / fill; a list packing is exported by
        qsc_export_readings and packed as from_readings packs (one re-sort).  This object is left
        untouched.  Raises ValueError for masks of another shape or dtype (before any device
        call) and when no reading is left."""
        self.check_select(self.K, self.I, self.J, pixels, bins, perm)
        kp, kb = self._masks(pixels, bins)
        return self._subset(kp, kb, 0, 0, self.RANGE, 0, self.perm if perm == "keep" else None)

    def split(self, frac, seed=0, perm="keep"):
        """(fit, held): a seeded random split of the readings, `held` about the fraction `frac`
        of them.  A reading goes to `held` iff its u24 (the keep rule's counter-based 24-bit
        number, a function of (seed, bin, pixel, occurrence of the cell) alone) lies in
        [0, round(frac 2^24)) (clamped to [1, 2^24 - 1]), to `fit` otherwise: the halves partition
        this object exactly, and the same reading falls on the same side whatever the tile, pixel
        order, schedule, row format and dense / readings input.  perm="keep": both halves in this
        object's pixel order; "fresh": `fit` ordered by its own counts and `held` packed with
        fit.perm.  Either way `held` is a valid obs_holdout partner of `fit`."""
        seed64 = self.check_split(frac=float("nan") if frac is None else frac, seed=seed, perm=perm)
        h = self.frac_range(frac)
        fit = self._subset(None, None, seed64, 0, h, 1, self.perm if perm == "keep" else None)
        return fit, self._subset(None, None, seed64, 0, h, 0, fit.perm)

    def folds(self, n, seed=0):
        """A sequence of n (train, test) pairs, each built when it is asked for (and not kept):
        fold f's test part holds the readings with u24 in [(f << 24) // n, ((f + 1) << 24) // n),
        its train part the others; the n test parts partition this object.  All in this object's
        pixel order.  2 <= n <= 65536."""
        return _Folds(self, n, self.check_split(seed=seed, n=0 if n is None else n))

    def readings(self):
        """(k, i, j, code): every packed reading as device tensors (int32, int32, int32, uint8),
        in ascending (k, pixel) order for dense input and (position, k, occurrence) order for a
        list packing.  Observations.from_readings(*obs.readings(), shape, ..., perm=obs.perm,
        tile=obs.desc.PT) rebuilds the packing bit for bit."""
        k, p, c, m = self._export(None, None, 0, 0, self.RANGE, 0)
        k, p, c = k[:m], p[:m], c[:m]
        i = torch.div(p, self.J, rounding_mode="floor")
        return k, i, p - i * self.J, c

    # ---- growth: occurrences, draw, append (include/qsc.h, "Growing a list packing") ----------
    def _cells(self, k, i, j):
        """Checked device lists (int32 k, int32 p, their number) of cells given as (k, i, j).
        Raises ValueError with the number of cells outside the map."""
        # (check_readings' rules for three lists: k stands in for the codes)
        K, I, J, m = self.check_readings(k, i, j, k, (self.K, self.I, self.J))
        kd, pd, _ = self._device_readings(k, i, j, None, I, J)
        nbad = int(((kd < 0) | (kd >= K) | (pd < 0)).sum())
        if nbad:
            raise ValueError("%d of %d cells have k outside [0, %d) or (i, j) outside the %d x %d "
                             "grid" % (nbad, m, K, I, J))
        return kd, pd, m

    def occurrences(self, k, i, j):
        """(m,) int32 on the device: the occurrence number j_occ every reading of the list of
        cells (k, i, j) (1-D integer tensors, repeats allowed) will have once appended -- the
        number of readings of its cell this object holds (qsc_obs_cell_counts) plus its place
        among the earlier readings of the same cell in the list.  Raises ValueError for lists of
        unequal length or cells outside the map."""
        kd, pd, m = self._cells(k, i, j)
        cnt = torch.empty(m, dtype=torch.int32, device=self.device)
        if self.codes is not None:
            _lib.call("qsc_obs_cell_counts", _lib.ptr(self.codes), None, 0, 0, self.desc, None,
                      _lib.ptr(kd), _lib.ptr(pd), m, _lib.ptr(cnt), _lib.stream())
        else:
            _lib.call("qsc_obs_cell_counts", None, _lib.ptr(self._packed), self._packed.numel(),
                      self._n, self.desc, _lib.ptr(self.iperm()), _lib.ptr(kd), _lib.ptr(pd), m,
                      _lib.ptr(cnt), _lib.stream())
        # the place inside the list: a stable sort by cell (m is a batch: not the hot path)
        cell, order = torch.sort(kd.to(torch.int64) * self.P + pd, stable=True)
        idx = torch.arange(m, device=self.device)
        first = torch.ones(m, dtype=torch.bool, device=self.device)
        first[1:] = cell[1:] != cell[:-1]
        start = torch.cummax(torch.where(first, idx, torch.zeros_like(idx)), 0).values
        rank = torch.empty(m, dtype=torch.int32, device=self.device)
        rank[order] = (idx - start).to(torch.int32)
        return cnt + rank

    def draw(self, k, i, j, S, C, seed=0, replicate=0, allow_invalid=False):
        """(m,) uint8 codes drawn from this object's model at (S, C) for new readings of the cells
        (k, i, j), observed so far or not: draw_readings with occurrence=self.occurrences(k, i, j),
        so that reading j_occ of a cell gets the same code however an acquisition is cut into
        batches -- the code resample() would give it once it is appended."""
        occ = self.occurrences(k, i, j)
        return draw_readings(k, i, j, S, C, (self.K, self.I, self.J), self.bin_boundaries,
                             self.noise_std, self.offset, self.log_model, self.loss, seed,
                             replicate, occurrence=occ, allow_invalid=allow_invalid)

    def append(self, k, i, j, code, perm="keep"):
        """A new Observations that holds this object's readings followed by the batch (k, i, j,
        code) (from_readings' four lists: any order, repeats allowed), with this one's model, loss,
        tile, R_hint and schedule flag.  The result is a list packing, bit for bit
        from_readings(cat(self.readings(), batch), perm=...); this object is left untouched, so
        hipGraphs captured on it stay valid.
        A list parent with perm="keep" is not re-sorted: the batch alone is sorted and merged into
        the kept sorted readings (qsc_obs_readings_merge), the tables are laid out from the new
        counts, the row format is re-evaluated and the entries are filled and scheduled as
        from_readings does.  perm="fresh" (the pixels ordered by the new counts) changes both sort
        keys, and a dense parent keeps no sorted readings -- its first append is the one that
        forms them: both export, concatenate and re-sort (perm="keep" keeps a dense parent's
        pixel order too), and later appends to the result merge.
        Raises ValueError for lists of unequal length or non-integer dtypes and an unknown perm
        (before any device call), and with the number of readings out of range; nothing is
        built then."""
        K, I, J, m = self.check_readings(k, i, j, code, (self.K, self.I, self.J))
        _check_perm(perm)
        n, P = self.nnz, self.P
        if n + m >= 2 ** 31:
            raise ValueError("at most 2^31 - 1 readings are supported, got %d + %d" % (n, m))
        kd, pd, cd = self._device_readings(k, i, j, code, I, J)
        PT, nbins = int(self.desc.PT), int(self.desc.nbins)
        cb = 1 if cd.dtype == torch.uint8 else 4
        s = _lib.stream()
        bcnt = torch.empty(P, dtype=torch.int32, device=self.device)
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.call("qsc_obs_readings_count", _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(cd), cb, m, K, P,
                  nbins, _lib.ptr(bcnt), _lib.ptr(bad), s)
        nbad = int(bad.item())
        if nbad:
            raise ValueError("%d of %d readings have k outside [0, %d), (i, j) outside the "
                             "%d x %d grid or a code outside [0, %d)" % (nbad, m, K, I, J, nbins))
        new = self._child()
        if self.codes is not None or perm == "fresh":
            pk, pp, pc, n0 = self._export(None, None, 0, 0, self.RANGE, 0)
            new._pack_readings(torch.cat((pk[:n0], kd)), torch.cat((pp[:n0], pd)),
                               torch.cat((pc[:n0], cd.to(torch.uint8))), n0 + m,
                               self.perm if perm == "keep" else None, None, PT, nbins, new.R_hint,
                               cnt=self.counts + bcnt)
            return new
        new.codes = None
        new.counts = self.counts + bcnt
        new.perm = self.perm
        new._alloc_tables(PT)
        L = _lib.lib()
        nb = L.qsc_obs_readings_merge_packed_bytes(n, m, K, P, PT)
        wb = L.qsc_obs_readings_merge_workspace_bytes(n, m, K, P, PT)
        if nb == 0 or wb == 0:
            raise ValueError("%d + %d readings of shape %r with tile %d are out of the merge's "
                             "range" % (n, m, (K, I, J), PT))
        new._packed = torch.empty(nb, dtype=torch.uint8, device=self.device)
        new._n = n + m
        ws = torch.empty(wb, dtype=torch.uint8, device=self.device)  # (follows m; not cached)
        desc = _lib.QscObsDesc()
        rep = ctypes.c_int32(int(self.max_repeat))
        _lib.call("qsc_obs_readings_merge", _lib.ptr(self._packed), self._packed.numel(), n,
                  self.desc, _lib.ptr(self.perm), _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(cd), cb, m,
                  _lib.ptr(new.counts), _lib.ptr(new.s_width), _lib.ptr(new.s_off),
                  _lib.ptr(new.c_width), _lib.ptr(new.c_off), _lib.ptr(new.c_kmap),
                  _lib.ptr(new._packed), nb, _lib.ptr(ws), wb, desc, ctypes.byref(rep), s)
        del ws
        if int(desc.nnz) != n + m:  # a parent's perm that gives some pixel of the batch no position
            raise ValueError("perm places only %d of the %d readings: every pixel that has a "
                             "reading needs a position" % (int(desc.nnz), n + m))
        new.max_repeat = int(rep.value)
        new._finish(desc, new.R_hint)
        return new

    def signed_rows_ok(self, R):
        if os.environ.get("QSC_SIGNED_ROWS", "1") == "0":  # A/B switch (tuning runs)
            return False
        return bool(_lib.lib().qsc_obs_signed_rows_ok(self.desc, int(R), self.model))

    def layout(self, R):
        """(desc, s_entries, c_entries) the passes read at rank R.  The signed-row packing chosen
        for R_hint is used where it applies at R; otherwise a code-field copy is packed once and
        kept (same entry count, other values).  The shared packing is never re-packed in place,
        so hipGraphs captured by other solvers on this object stay valid (their kernels hold the
        descriptor and entry pointers by value)."""
        self._engines = getattr(self, "_engines", 0) + 1
        if self.desc.rowfmt != 1 or self.signed_rows_ok(R):
            return self.desc, self.s_entries, self.c_entries
        if getattr(self, "_code_field", None) is None:
            d = _lib.QscObsDesc()
            ctypes_copy(d, self.desc)
            s_e = torch.empty_like(self.s_entries)
            c_e = torch.empty_like(self.c_entries)
            self._fill(0, d, s_e, c_e)
            self._code_field = (d, s_e, c_e)
        return self._code_field

    # ---- info -----------------------------------------------------------------------
    @property
    def nnz(self):
        return int(self.desc.nnz)

    @property
    def entry_bytes(self):
        return 4 if self.desc.wide else 2

    def stats(self):
        d = self.desc
        out = dict(K=d.K, P=d.P, Pp=d.Pp, tile=d.PT, ntiles=d.ntiles, nks=d.nks, wide=d.wide,
                   nbins=d.nbins, nnz=d.nnz, s_entries=d.s_entries, c_entries=d.c_entries,
                   rowfmt=d.rowfmt,
                   s_padding=d.s_entries / max(d.nnz, 1) - 1.0,
                   c_padding=d.c_entries / max(d.nnz, 1) - 1.0)
        if self.codes is None:  # from_readings: the largest number of readings of one cell
            out["max_repeat"] = self.max_repeat
        return out

    # ---- order conversions -------------------------------------------------------------
    def rank_pad(self, R):
        """Row count RP of the position-order layout for rank R (4, 8 or 16)."""
        rp = int(_lib.lib().qsc_rank_pad(int(R)))
        if rp == 0:
            raise ValueError("rank R must be in [1, %d]" % _lib.QSC_MAX_R)
        return rp

    def iperm(self):
        """(P,) int32: the position of every pixel (inverse of perm; cached)."""
        ip = getattr(self, "_iperm", None)
        if ip is None:
            ip = torch.full((self.P,), -1, dtype=torch.int32, device=self.device)
            valid = self.perm >= 0
            ip[self.perm[valid].long()] = torch.arange(self.Pp, dtype=torch.int32,
                                                       device=self.device)[valid]
            self._iperm = ip
        return ip

    def neighbors(self):
        """(Pp, 4) int32: the positions of every position's left, right, upper and lower grid
        neighbour, -1 outside the grid and for padding positions (qsc_smooth_neighbors; cached).
        The table of the smoothness prior (qsc_smooth_grad)."""
        nb = getattr(self, "_nbr", None)
        if nb is None:
            nb = neighbor_table(self.perm, self.I, self.J)
            self._nbr = nb
        return nb

    def to_positions(self, X, out=None):
        """(R, P) natural pixel order -> (Pp, RP) position order (pixel-major rows, zero padded);
        into `out` when given (a persistent buffer, e.g. inside a captured hipGraph)."""
        R = X.shape[0]
        Xd = _dev(X.detach().to(torch.float32)).reshape(R, self.P).contiguous()
        if out is None:
            out = torch.empty((self.Pp, self.rank_pad(R)), dtype=torch.float32, device=Xd.device)
        elif out.shape != (self.Pp, self.rank_pad(R)) or not out.is_contiguous():
            raise ValueError("out must be a contiguous (%d, %d) tensor" % (self.Pp, self.rank_pad(R)))
        _lib.call("qsc_perm_gather", _lib.ptr(Xd), _lib.ptr(self.perm), R, self.P, self.Pp,
                  _lib.ptr(out), _lib.stream())
        return out

    def to_pixels(self, Xp, R, out=None):
        """(Pp, RP) position order -> (R, P) natural pixel order."""
        if Xp.shape != (self.Pp, self.rank_pad(R)):
            raise ValueError("position-order tensor must be (%d, %d), got %s"
                             % (self.Pp, self.rank_pad(R), tuple(Xp.shape)))
        if out is None:
            out = torch.empty((R, self.P), dtype=torch.float32, device=Xp.device)
        _lib.call("qsc_perm_scatter", _lib.ptr(Xp.contiguous()), _lib.ptr(self.perm), R, self.P,
                  self.Pp, _lib.ptr(out), _lib.stream())
        return out


def check_draw_readings(k, i, j, S, C, shape, loss="probit", seed=0, replicate=0, occurrence=None):
    """Host-side checks of draw_readings' arguments, before any device call: check_readings'
    rules for the three lists of cells, check_resample's for loss, S, C, seed and replicate, and
    `occurrence` a 1-D integer tensor of the lists' length or None.  -> (K, I, J, m, R, seed as
    a signed 64-bit value).  Raises ValueError."""
    K, I, J, m = Observations.check_readings(k, i, j, k, shape)
    R, seed64 = Observations.check_resample(loss, K, I, J, S, C, seed, replicate)
    if occurrence is not None:
        Observations.check_readings(k, i, j, occurrence, shape)  # (one length, an integer dtype)
    return K, I, J, m, R, seed64


def draw_readings(k, i, j, S, C, shape, bin_boundaries, noise_std, offset=0.0, log_model=False,
                  loss="probit", seed=0, replicate=0, occurrence=None, allow_invalid=False):
    """(m,) uint8 codes on the device, drawn from the model at (S, C) at the listed cells: reading
    e is bin k[e] at pixel (i[e], j[e]) of the shape = (K, I, J) map, observed so far or not
    (qsc_draw_list, include/qsc.h).  The rule is Observations.resample's word for word, by the
    same device functions: the Philox counter is (k, p, occurrence, replicate), so with
    occurrence[e] the reading's number in its cell (None: all 0) the code is the one resample
    gives that reading of a packed object.  Observations.draw fills `occurrence` in from what the
    object holds.  A reading nothing can be drawn for (log model with T_hat + offset <= 0; a NaN
    T_hat) gets 0xFF; unless allow_invalid, their number raises ValueError.  S (R,1,I,J) or
    (R,I,J) or (R,I J), C (R,K); the model arguments are Observations'.  Raises ValueError for
    lists of unequal length, shapes that do not match, loss="squared" (not a likelihood) or
    seed / replicate out of range before any device call, and for cells outside the map or a
    negative occurrence."""
    K, I, J, m, R, seed64 = check_draw_readings(k, i, j, S, C, shape, loss, seed, replicate,
                                                occurrence)
    model = _lib.make_model(bin_boundaries, noise_std, offset if log_model else 0.0, log_model,
                            loss=loss)
    kd, pd, _ = Observations._device_readings(k, i, j, None, I, J)
    dev = kd.device
    nbad = int(((kd < 0) | (kd >= K) | (pd < 0)).sum())
    if nbad:
        raise ValueError("%d of %d cells have k outside [0, %d) or (i, j) outside the %d x %d "
                         "grid" % (nbad, m, K, I, J))
    od = None
    if occurrence is not None:
        o64 = _dev(occurrence).to(torch.int64)
        if int(((o64 < 0) | (o64 >= 2 ** 31)).sum()):
            raise ValueError("occurrence numbers must be in [0, 2^31)")
        od = o64.to(torch.int32).contiguous()
    Cd = _dev(C.detach().to(torch.float32)).reshape(R, K).contiguous()
    Sd = _dev(S.detach().to(torch.float32)).reshape(R, I * J).contiguous()
    code = torch.empty(m, dtype=torch.uint8, device=dev)
    invalid = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("qsc_draw_list", _lib.ptr(kd), _lib.ptr(pd), _lib.ptr(od), m, K, I * J, model, R,
              _lib.ptr(Sd), _lib.ptr(Cd), seed64, int(replicate), _lib.ptr(code),
              _lib.ptr(invalid), _lib.stream())
    if not allow_invalid:
        left = int((code == _lib.UNOBSERVED).sum())
        if left:
            raise ValueError("%d of %d readings cannot be drawn (%d with T_hat + offset <= 0 "
                             "under the log model); allow_invalid=True returns them as 0xFF"
                             % (left, m, int(invalid.item())))
    return code
