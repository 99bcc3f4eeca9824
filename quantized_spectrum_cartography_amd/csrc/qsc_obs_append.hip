// qsc_obs_append.hip — growing a list packing (include/qsc.h: qsc_obs_cell_counts,
// qsc_obs_readings_merge): the device side of Observations.occurrences / append.
//
// Both sort keys of the list packing -- (position, k) for the S-format, (tile, bin in k order,
// qlocal) for the C-format -- depend on the pixel order alone, not on the counts.  With the
// parent's perm kept, a batch of m new readings is therefore sorted on its own (the layout's own
// key kernel and stable radix sort, qsc_obs_readings.hip) and each of the two sorted arrays of the
// result is a stable merge of the parent's n with the batch's m, parent readings first on equal
// keys -- what the re-sort of the concatenated list gives, bit for bit.
//
// The merge.  For every sorted batch reading i, ins[i] = the number of parent readings whose key
// is <= its key: an upper bound of its index (k or qlocal) inside the one parent segment
// (position, or (tile, bin)) its key names -- m short searches (ins_kernel).  ins is ascending.
// Then
//     batch reading i   goes to  i + ins[i]
//     parent reading e  goes to  e + #{i : ins[i] <= e}      (an upper bound of e in ins)
// and the parent's readings -- the stream, 4 n bytes in and out per array -- need neither their
// position nor their key: a workgroup takes kChunk consecutive ones, bounds the search range once
// from the chunk's first and last index (two searches of ins per chunk), stages that range of ins
// in LDS where it fits (kStage ints; a global search inside the range otherwise), and a chunk the
// batch does not touch is a shifted copy.  No atomics decide a place: the output bytes are a
// function of the inputs.
//
// max_repeat: only cells the batch touches can have grown.  The first batch reading of every run
// of equal keys adds the run's length to the parent's count of the cell (lower and upper bound
// in the cell's segment: cell_count, which is also qsc_obs_cell_counts' rule) -> atomicMax.
//
// Widths, offsets, bin order and the descriptor come from the new counts by the layout's own
// stages (rd_layout_positions before, rd_layout_finish after the merges): the (tile, bin) counts
// start from the parent's segment lengths instead of zero and the key kernel adds the batch's.
//
// Integer only; integer atomics for the counts and max_repeat.
#include "qsc_common.cuh"
#include "qsc_obs_readings.cuh"

namespace {
using namespace qsc;

constexpr int kBlock = 256;
constexpr int kChunk = 4 * kBlock;  // parent readings per workgroup of the merge
constexpr int kStage = 2048;        // ints of `ins` a workgroup stages in LDS
static_assert(kChunk == QSC_MERGE_CHUNK, "qsc.h");

// number of readings of the sorted run rd[lo, hi) whose index (low 24 bits) is < v / <= v
__device__ __forceinline__ int idx_lower(const uint32_t* __restrict__ rd, int lo, int hi, uint32_t v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((rd[mid] & kIdxMask) < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int idx_upper(const uint32_t* __restrict__ rd, int lo, int hi, uint32_t v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((rd[mid] & kIdxMask) <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// number of a[lo, hi) (ascending) that are <= e, plus lo
__device__ __forceinline__ int upper_le(const int* a, int lo, int hi, int e) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= e) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the bounds of segment q of a table, clamped into [0, n] (a consistent table never needs it)
__device__ __forceinline__ void seg_bounds(const int* __restrict__ seg, int64_t q, int64_t n, int* lo,
                                           int* hi) {
  const int a = seg[q], b = seg[q + 1];
  *lo = (int)min((int64_t)max(a, 0), n);
  *hi = (int)min((int64_t)max(b, *lo), n);
}

// ---- cnt[e] = readings of cell (k[e], p[e]) the parent holds; one thread per query ----
__global__ void __launch_bounds__(kBlock) cell_counts_kernel(
    const uint8_t* __restrict__ codes, const uint32_t* __restrict__ s_rd,
    const int* __restrict__ s_seg, const int* __restrict__ iperm, int64_t n, int K, int P, int Pp,
    const int* __restrict__ k, const int* __restrict__ p, int64_t m, int* __restrict__ cnt) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int kk = k[e], pp = p[e];
  int c = 0;
  if (kk >= 0 && kk < K && pp >= 0 && pp < P) {
    if (codes) {
      c = codes[(int64_t)kk * P + pp] != 0xFFu;
    } else {
      const int q = iperm[pp];
      if (q >= 0 && q < Pp) {
        int lo, hi;
        seg_bounds(s_seg, q, n, &lo, &hi);
        c = idx_upper(s_rd, lo, hi, (uint32_t)kk) - idx_lower(s_rd, lo, hi, (uint32_t)kk);
      }
    }
  }
  cnt[e] = c;
}

// ccount[b] = readings of (tile, bin) b in the parent (its segment's length); ccount[nb] = 0
__global__ void __launch_bounds__(kBlock) ccount_init_kernel(const int* __restrict__ c_seg, int nb,
                                                             int* __restrict__ ccount) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  ccount[b] = b < nb ? c_seg[b + 1] - c_seg[b] : 0;
}

// ins[i] of the sorted batch keys  key = seg * rows + idx  (the S-format: seg = position, rows = K,
// idx = k; the C-format: seg = (tile, bin), rows = PT, idx = qlocal); a key past every valid one
// (a reading no position holds) goes behind the parent.  REPEAT: the S-format call also raises
// *max_repeat to the merged run length of every cell the batch touches.
template <bool REPEAT>
__global__ void __launch_bounds__(kBlock) ins_kernel(const uint64_t* __restrict__ key, int64_t m,
                                                     uint64_t rows, uint64_t nseg,
                                                     const uint32_t* __restrict__ rd,
                                                     const int* __restrict__ seg, int64_t n,
                                                     int* __restrict__ ins,
                                                     int* __restrict__ max_repeat) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t v = key[i];
  if (v >= nseg * rows) {
    ins[i] = (int)n;
    return;
  }
  const uint64_t q = v / rows;
  const uint32_t idx = (uint32_t)(v - q * rows);
  int lo, hi;
  seg_bounds(seg, (int64_t)q, n, &lo, &hi);
  const int ub = idx_upper(rd, lo, hi, idx);
  ins[i] = ub;
  if (REPEAT) {
    if (i > 0 && key[i - 1] == v) return;
    int64_t e = i + 1;
    while (e < m && key[e] == v) ++e;
    atomicMax(max_repeat, (ub - idx_lower(rd, lo, hi, idx)) + (int)(e - i));
  }
}

// One sorted array of the result: workgroups [0, pchunks) move a chunk of the parent's readings,
// the others a chunk of the batch's.
__global__ void __launch_bounds__(kBlock) merge_kernel(const uint32_t* __restrict__ par, int64_t n,
                                                       const uint32_t* __restrict__ bat,
                                                       const int* __restrict__ ins, int64_t m,
                                                       int pchunks, uint32_t* __restrict__ out) {
  __shared__ int stage[kStage];
  __shared__ int range[2];
  if ((int)blockIdx.x >= pchunks) {
    const int64_t i0 = (int64_t)(blockIdx.x - pchunks) * kChunk;
    for (int64_t i = i0 + threadIdx.x; i < min(i0 + kChunk, m); i += kBlock) {
      const int64_t o = i + min(max(ins[i], 0), (int)n);
      out[o] = bat[i];  // o < m + n
    }
    return;
  }
  const int64_t e0 = (int64_t)blockIdx.x * kChunk;
  const int ne = (int)min((int64_t)kChunk, n - e0);
  if (threadIdx.x == 0) range[0] = upper_le(ins, 0, (int)m, (int)e0);
  if (threadIdx.x == 64) range[1] = upper_le(ins, 0, (int)m, (int)(e0 + ne - 1));
  __syncthreads();
  const int lo = range[0], hi = range[1];  // lo <= every reading's rank <= hi <= m
  const int ns = hi - lo;
  if (ns == 0) {
    for (int j = threadIdx.x; j < ne; j += kBlock) out[e0 + j + lo] = par[e0 + j];
    return;
  }
  const bool staged = ns <= kStage;  // (uniform in the workgroup)
  if (staged) {
    for (int j = threadIdx.x; j < ns; j += kBlock) stage[j] = ins[lo + j];
    __syncthreads();
  }
  for (int j = threadIdx.x; j < ne; j += kBlock) {
    const int64_t e = e0 + j;
    const int r = staged ? lo + upper_le(stage, 0, ns, (int)e) : upper_le(ins, lo, hi, (int)e);
    out[e + r] = par[e];  // e < n, r <= m
  }
}

inline bool merge_ok(int64_t n, int64_t m) {
  return n_ok(n) && n_ok(m) && n + m < ((int64_t)1 << 31);
}

// the workspace: the layout's own for m readings, then the batch's sorted values and ins
struct MergeWs {
  RdWs rd;
  uint32_t* val;  // [m]
  int* ins;       // [m]
};
size_t merge_carve(char* b, int64_t m, int32_t K, int32_t P, int32_t PT, MergeWs* w) {
  const size_t base = rd_ws_carve(b, m, K, P, PT, &w->rd);
  if (!base) return 0;
  char* p = b + base;
  w->val = (uint32_t*)p;
  p += align_up((size_t)m * 4);
  w->ins = (int*)p;
  p += align_up((size_t)m * 4);
  return (size_t)(p - b);
}

}  // namespace

extern "C" {

QSC_API int qsc_obs_cell_counts(const uint8_t* codes, const void* packed, size_t packed_bytes,
                                int64_t n, const qsc_obs_desc* d, const int32_t* iperm,
                                const int32_t* k, const int32_t* p, int64_t m, int32_t* cnt,
                                void* stream) {
  Dims dm;
  Packed pk = {};
  if (!k || !p || !cnt || !n_ok(m)) return QSC_EINVAL;
  if (codes ? !desc_dims(d, &dm) : !iperm || !packed_of(packed, packed_bytes, n, d, &dm, &pk))
    return QSC_EINVAL;
  hipLaunchKernelGGL(cell_counts_kernel, dim3((unsigned)ceil_div(m, kBlock)), dim3(kBlock), 0,
                     STREAM(stream), codes, pk.s_rd, pk.s_seg, iperm, n, d->K, d->P, d->Pp, k, p,
                     m, cnt);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API size_t qsc_obs_readings_merge_packed_bytes(int64_t n, int64_t m, int32_t K, int32_t P,
                                                   int32_t PT) {
  Dims d;
  Packed pk;
  if (!merge_ok(n, m) || !dims_of(K, P, PT, &d)) return 0;
  return packed_carve(nullptr, n + m, d, &pk);
}

QSC_API size_t qsc_obs_readings_merge_workspace_bytes(int64_t n, int64_t m, int32_t K, int32_t P,
                                                      int32_t PT) {
  MergeWs w;
  if (!merge_ok(n, m)) return 0;
  return merge_carve(nullptr, m, K, P, PT, &w);
}

QSC_API int qsc_obs_readings_merge(const void* packed, size_t packed_bytes, int64_t n,
                                   const qsc_obs_desc* d, const int32_t* perm, const int32_t* k,
                                   const int32_t* p, const void* code, int32_t code_bytes,
                                   int64_t m, const int32_t* cnt, int32_t* s_width, int64_t* s_off,
                                   int32_t* c_width, int64_t* c_off, int32_t* c_kmap,
                                   void* packed_out, size_t packed_out_bytes, void* ws,
                                   size_t ws_bytes, qsc_obs_desc* desc, int32_t* max_repeat,
                                   void* stream) {
  Dims dm;
  Packed in, out;
  MergeWs w;
  if (!perm || !k || !p || !code || !cnt || !s_width || !s_off || !c_width || !c_off || !c_kmap ||
      !packed_out || packed_out == packed || !ws || !desc || !max_repeat || !merge_ok(n, m) ||
      (code_bytes != 1 && code_bytes != 4) || !packed_of(packed, packed_bytes, n, d, &dm, &in) ||
      d->nbins < 1 || d->nbins > QSC_MAX_BOUNDS - 1)
    return QSC_EINVAL;
  const int32_t K = d->K, P = d->P, PT = d->PT, nbins = d->nbins;
  if (!rd_layout_fits(K, P, PT)) return QSC_EINVAL;
  if (packed_out_bytes < packed_carve((char*)packed_out, n + m, dm, &out)) return QSC_EINVAL;
  const size_t need = merge_carve((char*)ws, m, K, P, PT, &w);
  if (!need || ws_bytes < need) return QSC_EINVAL;
  const int Pp = (int)dm.Pp, nb = (int)dm.nb;
  hipStream_t s = STREAM(stream);
  const int parent_repeat = *max_repeat;

  // new per-position counts, S-format widths, offsets and segments
  int rc = rd_layout_positions(w.rd, K, P, PT, perm, cnt, s_width, s_off, out.s_seg, s);
  if (rc != QSC_OK) return rc;
  // (tile, bin) counts: the parent's, plus the batch's from the key kernel
  hipLaunchKernelGGL(ccount_init_kernel, dim3((unsigned)ceil_div(nb + 1, kBlock)), dim3(kBlock), 0,
                     s, in.c_seg, nb, w.rd.ccount);
  QSC_CHECK_LAUNCH();
  rc = rd_layout_keys(w.rd, k, p, code, code_bytes, m, K, P, PT, nbins, s);
  if (rc != QSC_OK) return rc;

  const dim3 bg((unsigned)ceil_div(m, kBlock)), blk(kBlock);
  const int pchunks = (int)ceil_div(n, kChunk);
  const dim3 mg((unsigned)(pchunks + ceil_div(m, kChunk)));
  int* scal = (int*)(w.rd.totals + 2);  // [0] nnz, [1] max_repeat: rd_layout_finish reads them
  QSC_TRY(hipMemsetAsync(scal, 0, 2 * sizeof(int64_t), s));
  // S-format: sort the batch, place it in the parent, merge
  const uint64_t s_rows = (uint64_t)K, c_rows = (uint64_t)PT;
  rc = rd_sort_pairs(w.rd, w.rd.s_key, w.rd.key_out, w.rd.s_val, w.val, m, (uint64_t)Pp * s_rows, s);
  if (rc != QSC_OK) return rc;
  hipLaunchKernelGGL(ins_kernel<true>, bg, blk, 0, s, w.rd.key_out, m, s_rows, (uint64_t)Pp,
                     in.s_rd, in.s_seg, n, w.ins, scal + 1);
  QSC_CHECK_LAUNCH();
  hipLaunchKernelGGL(merge_kernel, mg, blk, 0, s, in.s_rd, n, w.val, w.ins, m, pchunks, out.s_rd);
  QSC_CHECK_LAUNCH();
  // C-format: the same
  rc = rd_sort_pairs(w.rd, w.rd.c_key, w.rd.key_out, w.rd.c_val, w.val, m, (uint64_t)nb * c_rows, s);
  if (rc != QSC_OK) return rc;
  hipLaunchKernelGGL(ins_kernel<false>, bg, blk, 0, s, w.rd.key_out, m, c_rows, (uint64_t)nb,
                     in.c_rd, in.c_seg, n, w.ins, scal + 1);
  QSC_CHECK_LAUNCH();
  hipLaunchKernelGGL(merge_kernel, mg, blk, 0, s, in.c_rd, n, w.val, w.ins, m, pchunks, out.c_rd);
  QSC_CHECK_LAUNCH();

  // bin order, C-format widths, offsets and segments, totals, descriptor
  int32_t rep = 0;
  rc = rd_layout_finish(w.rd, K, P, PT, nbins, out.s_seg, s_off, c_width, c_off, c_kmap, out.c_seg,
                        out.c_kinv, desc, &rep, s);
  if (rc != QSC_OK) return rc;
  *max_repeat = rep > parent_repeat ? rep : parent_repeat;
  return QSC_OK;
}

}  // extern "C"
