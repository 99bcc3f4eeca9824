// qsc_obs_select.hip — subsets of packed observations (include/qsc.h: qsc_select_codes,
// qsc_export_codes, qsc_export_readings): the device side of Observations.select / split / folds /
// readings.
//
// The keep rule of reading (k, p, j_occ) (include/qsc.h states it; all integer arithmetic):
//     keep_pixel[p] != 0  and  keep_bin[k] != 0  and  ((lo <= u24 < hi) != invert)
//     u24 = philox4x32_10(counter (k, p, j_occ, 0x80000000), key (seed_lo, seed_hi)).x0 >> 8
// Word 3 = 0x80000000 is a stream no draw uses (qsc_draw_* take replicate < 2^31).  With lo = 0,
// hi = 2^24, invert = 0 the range rule is off and no Philox is evaluated.
//
// Dense codes are worked on as one flat array of K P cells in chunks of kTile = 4096 (flat order
// is (k, p) ascending), staged as qsc_obs_tile.cuh's dense tile (see there), so that the rule --
// ten Philox rounds -- runs on full waves of observed cells only.
//
// The exports are stable stream compactions in three steps: (1) the kept count of every chunk,
// (2) one exclusive scan of the chunk counts, (3) the rule again, an in-chunk scan (block_scan /
// scan_pos, see qsc_obs_tile.cuh) and the scatter.  No atomics decide a position: the output bytes
// are a function of the input.
//
// Readings (export_rd_kernel) are read from the S-format sorted array of `packed` in chunks of
// kRdChunk = 1024: the position of a reading from the segment table (the chunk's first and last
// position are searched once, every reading then searches between them), p = perm[position], j_occ
// by occurrence (see qsc_obs_readings.cuh).  Order: (position, k, occurrence), the sorted array's.
//
// Stream-ordered, no allocation; integer atomics for *kept only.
#include <hipcub/hipcub.hpp>

#include "qsc_common.cuh"
#include "qsc_obs_readings.cuh"
#include "qsc_obs_tile.cuh"
#include "qsc_philox.cuh"

namespace {
using namespace qsc;

constexpr int kBlock = kTileBlock;
constexpr int kRdRounds = 4;
constexpr int kRdChunk = kBlock * kRdRounds;  // readings per workgroup
static_assert(kRdChunk == QSC_EXPORT_CHUNK_READINGS, "qsc.h");

struct Rule {
  const uint8_t* keep_pixel;  // [P] or null
  const uint8_t* keep_bin;    // [K] or null
  SeedKey seed;
  uint32_t lo, hi;
  int invert, ranged;         // ranged = 0: lo = 0, hi = 2^24, invert = 0
};

__device__ __forceinline__ bool keep(const Rule& r, uint32_t k, uint32_t p, uint32_t j) {
  if (r.keep_pixel && !r.keep_pixel[p]) return false;
  if (r.keep_bin && !r.keep_bin[k]) return false;
  if (!r.ranged) return true;
  const uint32_t u = philox4x32_10_x0(k, p, j, 0x80000000u, r.seed.lo, r.seed.hi) >> 8;
  return (u >= r.lo && u < r.hi) != (r.invert != 0);
}

// (k, p) of the cell at offset o of a chunk whose first cell is (k0, p0): the chunk's start is
// divided once (64 bits), a cell costs one 32-bit division (p0 + o < P + kTile < 2^32)
struct Cell {
  uint32_t k, p;
};
__device__ __forceinline__ Cell cell_at(uint32_t k0, uint32_t p0, int o, uint32_t P) {
  const uint32_t t = p0 + (uint32_t)o;
  const uint32_t q = t / P;
  return {k0 + q, t - q * P};
}

// ---- dense: out = codes where kept, 0xFF elsewhere; *kept += kept cells ----
template <bool VEC>
__global__ void __launch_bounds__(kBlock) select_codes_kernel(
    const uint8_t* __restrict__ codes, int64_t total, int P, Rule rule, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ kept) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
  __shared__ uint16_t list[kTile];
  __shared__ int wcnt[65];
  __shared__ int nkept;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int nc = (int)min((int64_t)kTile, total - c0);
  const uint32_t k0 = (uint32_t)(c0 / P), p0 = (uint32_t)(c0 - (int64_t)k0 * P);
  if (threadIdx.x == 0) nkept = 0;
  const int nl = stage_observed<VEC>(codes, c0, nc, tile, list, wcnt);
  int nk = 0;
  for (int i = threadIdx.x; i < nl; i += kBlock) {
    const int o = list[i];
    const Cell c = cell_at(k0, p0, o, (uint32_t)P);
    if (keep(rule, c.k, c.p, 0u)) ++nk;
    else tile[o] = 0xFFu;
  }
  if (nk) atomicAdd(&nkept, nk);
  __syncthreads();
  if (threadIdx.x == 0 && nkept) atomicAdd(kept, (unsigned long long)nkept);
  tile_store<VEC>(out, c0, nc, tile);
}

// ---- dense export: COUNT: counts[chunk] = kept cells; else scatter them from offs[chunk] on ----
template <bool VEC, bool COUNT>
__global__ void __launch_bounds__(kBlock) export_codes_kernel(
    const uint8_t* __restrict__ codes, int64_t total, int P, Rule rule,
    int64_t* __restrict__ counts, const int64_t* __restrict__ offs, int* __restrict__ k_out,
    int* __restrict__ p_out, uint8_t* __restrict__ code_out) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
  __shared__ uint16_t list[kTile];
  __shared__ int wcnt[65], wcnt2[65];
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int nc = (int)min((int64_t)kTile, total - c0);
  const uint32_t k0 = (uint32_t)(c0 / P), p0 = (uint32_t)(c0 - (int64_t)k0 * P);
  const int nl = stage_observed<VEC>(codes, c0, nc, tile, list, wcnt);
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < kCells; ++i) {
    const int idx = i * kBlock + threadIdx.x;
    if (idx < nl) {
      const Cell c = cell_at(k0, p0, list[idx], (uint32_t)P);
      if (keep(rule, c.k, c.p, 0u)) mask |= 1u << i;
    }
  }
  const int nk = block_scan<kCells>(mask, wcnt2);
  if (COUNT) {
    if (threadIdx.x == 0) counts[blockIdx.x] = nk;
    return;
  }
  const int64_t base = offs[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kCells; ++i) {
    const int pos = scan_pos(mask, i, wcnt2);
    if ((mask >> i) & 1u) {
      const int o = list[i * kBlock + threadIdx.x];
      const Cell c = cell_at(k0, p0, o, (uint32_t)P);
      k_out[base + pos] = (int)c.k;
      p_out[base + pos] = (int)c.p;
      code_out[base + pos] = tile[o];
    }
  }
}

// ---- readings export, from the S-format sorted array ----
template <bool COUNT>
__global__ void __launch_bounds__(kBlock) export_rd_kernel(
    const uint32_t* __restrict__ rd, const int* __restrict__ seg, int64_t n, int Pp, int K, int P,
    const int* __restrict__ perm, Rule rule, int64_t* __restrict__ counts,
    const int64_t* __restrict__ offs, int* __restrict__ k_out, int* __restrict__ p_out,
    uint8_t* __restrict__ code_out) {
  __shared__ int wcnt[65];
  __shared__ int qr[2];
  const int64_t e0 = (int64_t)blockIdx.x * kRdChunk;
  const int ne = (int)min((int64_t)kRdChunk, n - e0);
  // (seg[0] = 0 <= e and seg[Pp] = n > e for every reading e)
  if (threadIdx.x == 0) qr[0] = seg_find(seg, Pp, (int)e0);
  if (threadIdx.x == 64) qr[1] = seg_find(seg, Pp, (int)(e0 + ne - 1));
  __syncthreads();
  const int qlo = qr[0], qhi = qr[1];
  uint32_t mask = 0;
  int kk[kRdRounds], pp[kRdRounds], cc[kRdRounds];
#pragma unroll
  for (int i = 0; i < kRdRounds; ++i) {
    const int idx = i * kBlock + threadIdx.x;
    kk[i] = pp[i] = cc[i] = 0;
    if (idx < ne) {
      const int64_t e = e0 + idx;
      const int q = qlo + seg_find(seg + qlo, qhi + 1 - qlo, (int)e);
      const uint32_t v = rd[e];
      const uint32_t k = v & kIdxMask;
      const int p = perm[q];
      const uint32_t j = occurrence(rd, e, seg[q], k);
      kk[i] = (int)k;
      pp[i] = p;
      cc[i] = (int)(v >> kIdxBits);
      if (p >= 0 && p < P && (int)k < K && keep(rule, k, (uint32_t)p, j)) mask |= 1u << i;
    }
  }
  const int nk = block_scan<kRdRounds>(mask, wcnt);
  if (COUNT) {
    if (threadIdx.x == 0) counts[blockIdx.x] = nk;
    return;
  }
  const int64_t base = offs[blockIdx.x];
#pragma unroll
  for (int i = 0; i < kRdRounds; ++i) {
    const int pos = scan_pos(mask, i, wcnt);
    if ((mask >> i) & 1u) {
      k_out[base + pos] = kk[i];
      p_out[base + pos] = pp[i];
      code_out[base + pos] = (uint8_t)cc[i];
    }
  }
}

inline bool make_rule(const uint8_t* keep_pixel, const uint8_t* keep_bin, int64_t seed, int32_t lo,
                      int32_t hi, int32_t invert, Rule* r) {
  if (lo < 0 || hi < lo || hi > (1 << 24) || (invert != 0 && invert != 1)) return false;
  r->keep_pixel = keep_pixel;
  r->keep_bin = keep_bin;
  r->seed = split_seed(seed);
  r->lo = (uint32_t)lo;
  r->hi = (uint32_t)hi;
  r->invert = invert;
  r->ranged = !(lo == 0 && hi == (1 << 24) && invert == 0);
  return true;
}

size_t scan_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t*)nullptr, (int64_t*)nullptr, (int)n);
  return b;
}

// the workspace of an export over `chunks` chunks
struct ExportWs {
  int64_t* counts;  // [chunks + 1]  (the last one 0: the scan's total slot)
  int64_t* offs;    // [chunks + 1]
  void* cub;
  size_t cub_bytes;
};
size_t export_carve(char* b, int64_t chunks, ExportWs* w) {
  char* p = b;
  w->counts = (int64_t*)p;
  p += align_up((size_t)(chunks + 1) * 8);
  w->offs = (int64_t*)p;
  p += align_up((size_t)(chunks + 1) * 8);
  w->cub = p;
  w->cub_bytes = align_up(scan_bytes(chunks + 1));
  p += w->cub_bytes;
  return (size_t)(p - b);
}

inline bool entries_ok(int64_t entries) {
  // chunk indices, the scan's length and a grid dimension are ints
  return entries >= 1 && ceil_div(entries, kRdChunk) < ((int64_t)1 << 31) - 1;
}

// steps 2 and the tail of an export: scan the chunk counts, *n_out = their sum
int export_scan(const ExportWs& w, int64_t chunks, int64_t* n_out, hipStream_t s) {
  size_t cb = w.cub_bytes;
  QSC_TRY(hipcub::DeviceScan::ExclusiveSum(w.cub, cb, w.counts, w.offs, (int)(chunks + 1), s));
  QSC_TRY(hipMemcpyAsync(n_out, w.offs + chunks, 8, hipMemcpyDeviceToDevice, s));
  return QSC_OK;
}

}  // namespace

extern "C" {

QSC_API int qsc_select_codes(const uint8_t* codes, int32_t K, int32_t P, const uint8_t* keep_pixel,
                             const uint8_t* keep_bin, int64_t seed, int32_t lo, int32_t hi,
                             int32_t invert, uint8_t* out, int64_t* kept, void* stream) {
  Rule rule;
  if (!codes || !out || !kept || codes == out || K < 1 || P < 1 ||
      !make_rule(keep_pixel, keep_bin, seed, lo, hi, invert, &rule))
    return QSC_EINVAL;
  const int64_t total = (int64_t)K * P, chunks = ceil_div(total, kTile);
  if (chunks >= ((int64_t)1 << 31)) return QSC_EINVAL;
  const bool vec = tile_vec_ok(P, codes, out);
  const dim3 grid((unsigned)chunks), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  if (vec)
    hipLaunchKernelGGL(select_codes_kernel<true>, grid, blk, 0, hs, codes, total, P, rule, out,
                       (unsigned long long*)kept);
  else
    hipLaunchKernelGGL(select_codes_kernel<false>, grid, blk, 0, hs, codes, total, P, rule, out,
                       (unsigned long long*)kept);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API size_t qsc_export_workspace_bytes(int64_t entries) {
  ExportWs w;
  if (!entries_ok(entries)) return 0;
  return export_carve(nullptr, ceil_div(entries, kRdChunk), &w);
}

QSC_API int qsc_export_codes(const uint8_t* codes, int32_t K, int32_t P, const uint8_t* keep_pixel,
                             const uint8_t* keep_bin, int64_t seed, int32_t lo, int32_t hi,
                             int32_t invert, int32_t* k_out, int32_t* p_out, uint8_t* code_out,
                             int64_t* n_out, void* ws, size_t ws_bytes, void* stream) {
  Rule rule;
  if (!codes || !k_out || !p_out || !code_out || !n_out || !ws || K < 1 || P < 1 ||
      !entries_ok((int64_t)K * P) || !make_rule(keep_pixel, keep_bin, seed, lo, hi, invert, &rule))
    return QSC_EINVAL;
  const int64_t total = (int64_t)K * P, chunks = ceil_div(total, kTile);
  ExportWs w;
  if (ws_bytes < export_carve((char*)ws, chunks, &w)) return QSC_EINVAL;
  const bool vec = tile_vec_ok(P, codes);
  const dim3 grid((unsigned)chunks), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  QSC_TRY(hipMemsetAsync(w.counts + chunks, 0, 8, hs));
#define EXPORT_LAUNCH(VC, CNT)                                                               \
  hipLaunchKernelGGL((export_codes_kernel<VC, CNT>), grid, blk, 0, hs, codes, total, P, rule, \
                     w.counts, w.offs, k_out, p_out, code_out)
  if (vec) EXPORT_LAUNCH(true, true); else EXPORT_LAUNCH(false, true);
  QSC_CHECK_LAUNCH();
  const int rc = export_scan(w, chunks, n_out, hs);
  if (rc != QSC_OK) return rc;
  if (vec) EXPORT_LAUNCH(true, false); else EXPORT_LAUNCH(false, false);
#undef EXPORT_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_export_readings(const void* packed, size_t packed_bytes, int64_t n,
                                const qsc_obs_desc* d, const int32_t* perm,
                                const uint8_t* keep_pixel, const uint8_t* keep_bin, int64_t seed,
                                int32_t lo, int32_t hi, int32_t invert, int32_t* k_out,
                                int32_t* p_out, uint8_t* code_out, int64_t* n_out, void* ws,
                                size_t ws_bytes, void* stream) {
  Rule rule;
  Dims dm;
  Packed in;
  if (!perm || !k_out || !p_out || !code_out || !n_out || !ws ||
      !packed_of(packed, packed_bytes, n, d, &dm, &in) ||
      !make_rule(keep_pixel, keep_bin, seed, lo, hi, invert, &rule))
    return QSC_EINVAL;
  const int64_t chunks = ceil_div(n, kRdChunk);
  ExportWs w;
  if (ws_bytes < export_carve((char*)ws, chunks, &w)) return QSC_EINVAL;
  const dim3 grid((unsigned)chunks), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  QSC_TRY(hipMemsetAsync(w.counts + chunks, 0, 8, hs));
  hipLaunchKernelGGL(export_rd_kernel<true>, grid, blk, 0, hs, in.s_rd, in.s_seg, n, (int)dm.Pp,
                     d->K, d->P, perm, rule, w.counts, w.offs, k_out, p_out, code_out);
  QSC_CHECK_LAUNCH();
  const int rc = export_scan(w, chunks, n_out, hs);
  if (rc != QSC_OK) return rc;
  hipLaunchKernelGGL(export_rd_kernel<false>, grid, blk, 0, hs, in.s_rd, in.s_seg, n, (int)dm.Pp,
                     d->K, d->P, perm, rule, w.counts, w.offs, k_out, p_out, code_out);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
