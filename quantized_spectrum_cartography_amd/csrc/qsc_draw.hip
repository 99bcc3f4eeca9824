// qsc_draw.hip — draw readings from the fitted model at the observed cells (include/qsc.h:
// qsc_draw_codes, qsc_draw_readings): the primitive of the parametric bootstrap.
//
// One reading at bin k, pixel p, occurrence j (the j-th reading of its cell), replicate rep:
//     t   = s_p . c_k                     fp32, r ascending, by fma
//     x   = t  or  log(t + offset)        the log model; t + offset <= 0: the reading keeps its
//                                         code and *invalid is incremented
//     P_b = bin_terms<LOGIT>(x, edge_b)   the likelihood's own P, every bin; Z = sum_b P_b, b ascending
//     n   = philox4x32_10(counter (k, p, j, rep), key (seed_lo, seed_hi)).x0 >> 8
//     thr = RN((n + 1/2) 2^-24 Z)         u Z with u = (n + 1/2) 2^-24 in (0, 1), one rounding
//     code = the smallest b with thr < sum_{b' <= b} P_b' (running sum, b ascending); if none,
//            the last b with P_b > 0; if there is none either (a NaN t), the reading keeps its code
// A bin whose fp32 P_b is 0 is never drawn: thr < cum_b with thr >= cum_{b-1} needs P_b > 0.
// The probabilities are evaluated twice (once for Z, once for the running sum: the same
// operations, the same bits) instead of being kept: up to 254 bins do not fit a lane's registers.
// With two bins both are kept and the rule is one comparison.
//
// Dense (draw_codes_kernel).  codes[K][P] holds about one observed cell in ten.  A thread per cell
// with an early exit would run the bin loop with about a tenth of its lanes; the kernel compacts
// instead: a workgroup takes kTile consecutive cells of one bin k as qsc_obs_tile.cuh's dense tile
// (see there: the load, the ascending list of the observed cells' offsets by stage_observed -- the
// ordered scan the exports use, no atomics decide a position: 112.6 us per call at C3 against 161.0
// with an LDS-atomic append, profiles/obswalk/ -- and the write-back), and the threads share the
// list, full waves until its tail.  k is uniform in a workgroup: c_k and the edges sit in LDS and
// are read at uniform addresses.  S is read as natural [R][P] planes: the cells of a tile are
// consecutive pixels, so a plane's reads fall into one 16 KiB window per workgroup; position rows
// would need the inverse permutation and give scattered 16- to 64-byte reads.
//
// Readings (draw_rd_s_kernel, draw_rd_c_kernel).  Both sorted arrays of `packed` are redrawn, each
// from its own keys, by the walks of qsc_obs_readings.cuh (see there): the S-format array by slice
// (walk_s_slice: k from the reading, the pixel from perm), the C-format array by tile (walk_c_tile:
// the position from qlocal by tile_pos, the pixel from perm).  The occurrence index j of a reading
// is `occurrence`'s: reading j of a cell is the same reading in both arrays and gets the same
// code.  S is read in position order [Pp][RP], the order of both arrays' keys.
//
// Listed cells (draw_list_kernel, qsc_draw_list).  A draw at cells given as lists (k, p, occurrence),
// observed or not: one thread per query, the dense kernel's map value (natural planes) and the same
// draw_code, with no present code to keep -- where nothing is drawn the output is 0xFF.
//
// No floating-point atomics, no workspace, no allocation; *invalid is an integer atomic.
#include <hip/hip_runtime.h>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"
#include "qsc_obs_readings.cuh"
#include "qsc_obs_tile.cuh"
#include "qsc_philox.cuh"

namespace {
using namespace qsc;

static_assert(kBlock == kTileBlock, "qsc_obs_tile.cuh");

struct DrawKey {
  SeedKey seed;
  uint32_t replicate;
};

// the drawn code of one reading (the file header's rule); `keep` is the code it has
template <bool LOGIT, bool LOG>
__device__ __forceinline__ int draw_code(float t, int keep, const float2* __restrict__ edges,
                                         const Link& lk, uint32_t k, uint32_t p, uint32_t j,
                                         const DrawKey& key, int& ninvalid) {
  float x = t;
  if (LOG) {
    const float tp = t + lk.offset;
    if (!(tp > 0.0f)) {
      ++ninvalid;
      return keep;
    }
    x = logf(tp);
  }
  const float n = (float)(philox4x32_10_x0(k, p, j, key.replicate, key.seed.lo, key.seed.hi) >> 8);
  float P1_, P2_;
  if (lk.nbins == 2) {
    float P0, P1;
    bin_terms<LOGIT>(x, edges[0].x, edges[0].y, lk, P0, P1_, P2_);
    bin_terms<LOGIT>(x, edges[1].x, edges[1].y, lk, P1, P1_, P2_);
    const float Zs = (P0 + P1) * 0x1p-24f;
    const float thr = __builtin_fmaf(n, Zs, 0.5f * Zs);
    if (thr < P0) return 0;
    if (P1 > 0.0f) return 1;
    return P0 > 0.0f ? 0 : keep;
  }
  float Z = 0.0f;
  for (int b = 0; b < lk.nbins; ++b) {
    const float2 e = edges[b];
    float P;
    bin_terms<LOGIT>(x, e.x, e.y, lk, P, P1_, P2_);
    Z += P;
  }
  const float Zs = Z * 0x1p-24f;
  const float thr = __builtin_fmaf(n, Zs, 0.5f * Zs);
  float cum = 0.0f;
  int last = keep;
  for (int b = 0; b < lk.nbins; ++b) {
    const float2 e = edges[b];
    float P;
    bin_terms<LOGIT>(x, e.x, e.y, lk, P, P1_, P2_);
    cum += P;
    if (thr < cum) return b;
    last = P > 0.0f ? b : last;
  }
  return last;
}

// ---- dense: codes[K][P] -> codes_out[K][P] ----
template <bool LOGIT, bool LOG, bool VEC>
__global__ void __launch_bounds__(kBlock) draw_codes_kernel(
    const uint8_t* __restrict__ codes, int K, int P, int tiles, const float* __restrict__ S,
    const float* __restrict__ C, int R, Link lk, Edges E_, DrawKey key,
    uint8_t* __restrict__ out, int* __restrict__ invalid) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kTile];
  __shared__ uint16_t list[kTile];
  __shared__ float ck[QSC_MAX_R];
  __shared__ int wcnt[65];
  QSC_ENTRYWISE_STAGE(lk, E_.e[b_]);  // (its barrier is repeated below, after the other staging)
  const int k = blockIdx.x / tiles;
  const int p0 = (blockIdx.x - k * tiles) * kTile;
  const int np = min(kTile, P - p0);  // cells of this tile
  const int64_t row = (int64_t)k * P + p0;
  if (threadIdx.x < QSC_MAX_R) ck[threadIdx.x] = threadIdx.x < R ? C[(int64_t)threadIdx.x * K + k] : 0.0f;
  // the tile into LDS, the observed cells' offsets into the list (its barriers cover ck too)
  const int nl = stage_observed<VEC>(codes, row, np, tile, list, wcnt);  // <= np <= kTile
  int ninv = 0;
  for (int i = threadIdx.x; i < nl; i += kBlock) {
    const int o = list[i];
    const int p = p0 + o;
    float t = 0.0f;
    for (int r = 0; r < R; ++r) t = __builtin_fmaf(S[(int64_t)r * P + p], ck[r], t);
    const int keep = tile[o];
    // (a code outside the model's bins is left as it is: nothing is drawn for it)
    if (keep < lk.nbins)
      tile[o] = (uint8_t)draw_code<LOGIT, LOG>(t, keep, se, lk, (uint32_t)k, (uint32_t)p, 0u, key,
                                               ninv);
  }
  if (ninv) atomicAdd(invalid, ninv);
  __syncthreads();
  tile_store<VEC>(out, row, np, tile);
}

// t = S_pos[q] . c_k, r ascending (rows >= R of the position layout are zero and are not read)
__device__ __forceinline__ float map_value(const float* __restrict__ S_pos, int64_t q, int RP,
                                           const float* __restrict__ C, int K, int k, int R) {
  float t = 0.0f;
  for (int r = 0; r < R; ++r) t = __builtin_fmaf(S_pos[q * RP + r], C[(int64_t)r * K + k], t);
  return t;
}

// ---- readings, S-format array: one wave per slice ----
template <bool LOGIT, bool LOG>
__global__ void __launch_bounds__(kBlock) draw_rd_s_kernel(
    const uint32_t* __restrict__ rd, const int* __restrict__ seg_all, int64_t n, int ns, int K,
    int P, int RP, const int* __restrict__ perm, const float* __restrict__ S_pos,
    const float* __restrict__ C, int R, Link lk, Edges E_, DrawKey key,
    uint32_t* __restrict__ rd_out, int* __restrict__ invalid) {
  __shared__ int seg_sh[kWaves][QSC_SLICE + 1];
  QSC_ENTRYWISE_STAGE(lk, E_.e[b_]);
  const int wave = threadIdx.x >> 6;
  const int s = blockIdx.x * kWaves + wave;
  int ninv = 0;
  auto draw = [&](int64_t e, int l, uint32_t v, int e0) {
    const uint32_t k = v & kIdxMask;
    const int keep = (int)(v >> kIdxBits);
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    const uint32_t j = occurrence(rd, e, e0, k);
    int code = keep;
    if (p >= 0 && p < P && (int)k < K && keep < lk.nbins)
      code = draw_code<LOGIT, LOG>(map_value(S_pos, q, RP, C, K, (int)k, R), keep, se, lk, k,
                                   (uint32_t)p, j, key, ninv);
    rd_out[e] = k | ((uint32_t)code << kIdxBits);
  };
  if (!walk_s_slice(rd, seg_all, n, ns, s, seg_sh[wave], draw)) return;
  // (every reading is counted once: by this array's kernel only)
  if (ninv) atomicAdd(invalid, ninv);
}

// ---- readings, C-format array: one workgroup per tile ----
template <bool LOGIT, bool LOG>
__global__ void __launch_bounds__(kBlock) draw_rd_c_kernel(
    const uint32_t* __restrict__ rd, const int* __restrict__ seg_all, int64_t n, int K, int P,
    int Pp, int nt, int nks, int RP, const int* __restrict__ perm,
    const float* __restrict__ S_pos, const float* __restrict__ C, int R, Link lk, Edges E_,
    DrawKey key, uint32_t* __restrict__ rd_out) {
  extern __shared__ int seg[];  // [Kp + 1]
  QSC_ENTRYWISE_STAGE(lk, E_.e[b_]);
  const int Kp = nks * 64;
  const int t = blockIdx.x;
  int ninv = 0;  // (counted by the S-format array's kernel)
  walk_c_tile(rd, seg_all, n, t, Kp, seg, [&](int64_t e, int k, uint32_t v, int e0) {
    const uint32_t ql = v & kIdxMask;
    const int keep = (int)(v >> kIdxBits);
    const int64_t q = tile_pos(t, (int)ql, nt);
    const uint32_t j = occurrence(rd, e, e0, ql);
    int code = keep;
    if (q >= 0 && q < Pp && k < K && keep < lk.nbins) {
      const int p = perm[q];
      if (p >= 0 && p < P)
        code = draw_code<LOGIT, LOG>(map_value(S_pos, q, RP, C, K, k, R), keep, se, lk, (uint32_t)k,
                                     (uint32_t)p, j, key, ninv);
    }
    rd_out[e] = ql | ((uint32_t)code << kIdxBits);
  });
}

// ---- listed cells: one thread per query (k, p, occurrence) -> a code, 0xFF where none is drawn ----
template <bool LOGIT, bool LOG>
__global__ void __launch_bounds__(kBlock) draw_list_kernel(
    const int* __restrict__ k, const int* __restrict__ p, const int* __restrict__ occ, int64_t m,
    int K, int P, const float* __restrict__ S, const float* __restrict__ C, int R, Link lk,
    Edges E_, DrawKey key, uint8_t* __restrict__ code, int* __restrict__ invalid) {
  QSC_ENTRYWISE_STAGE(lk, E_.e[b_]);
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int kk = k[e], pp = p[e];
  int ninv = 0, c = QSC_UNOBSERVED;
  if (kk >= 0 && kk < K && pp >= 0 && pp < P) {
    float t = 0.0f;  // (the dense kernel's sum: S natural planes, r ascending, by fma)
    for (int r = 0; r < R; ++r) t = __builtin_fmaf(S[(int64_t)r * P + pp], C[(int64_t)r * K + kk], t);
    c = draw_code<LOGIT, LOG>(t, QSC_UNOBSERVED, se, lk, (uint32_t)kk, (uint32_t)pp,
                              occ ? (uint32_t)occ[e] : 0u, key, ninv);
  }
  code[e] = (uint8_t)c;
  if (ninv) atomicAdd(invalid, ninv);
}

inline DrawKey make_key(int64_t seed, int32_t replicate) {
  DrawKey k;
  k.seed = split_seed(seed);
  k.replicate = (uint32_t)replicate;
  return k;
}

}  // namespace

// QSC_INFO_DISPATCH for LAUNCH(LOGIT, LOG, KIND): its third axis, the kind, is unused by the draws
#define DRAW_DISPATCH(LAUNCH)                                     \
  do {                                                            \
    const int kind = INFO_EXPECTED;                               \
    QSC_INFO_DISPATCH(LAUNCH);                                    \
  } while (0)

extern "C" {

QSC_API int qsc_draw_codes(const uint8_t* codes, int32_t K, int32_t P, const qsc_model* m,
                           int32_t R, const float* S, const float* C, int64_t seed,
                           int32_t replicate, uint8_t* codes_out, int32_t* invalid, void* stream) {
  if (!codes || !S || !C || !codes_out || !invalid || !info_model_ok(m)) return QSC_EINVAL;
  if (R < 1 || R > QSC_MAX_R || K < 1 || P < 1 || replicate < 0) return QSC_EINVAL;
  const int64_t tiles = ceil_div(P, kTile);
  if (tiles * K >= ((int64_t)1 << 31)) return QSC_EINVAL;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const DrawKey key = make_key(seed, replicate);
  const bool vec = tile_vec_ok(P, codes, codes_out);
  const dim3 grid((unsigned)(tiles * K)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
#define DRAW_LAUNCH_(LGT, LOGV, VC)                                                          \
  hipLaunchKernelGGL((draw_codes_kernel<LGT, LOGV, VC>), grid, blk, 0, hs, codes, K, P,      \
                     (int)tiles, S, C, R, lk, E, key, codes_out, invalid)
#define DRAW_LAUNCH(LGT, LOGV, KD)           \
  do {                                       \
    if (vec) DRAW_LAUNCH_(LGT, LOGV, true);  \
    else DRAW_LAUNCH_(LGT, LOGV, false);     \
  } while (0)
  DRAW_DISPATCH(DRAW_LAUNCH);
#undef DRAW_LAUNCH
#undef DRAW_LAUNCH_
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_draw_readings(const void* packed, size_t packed_bytes, int64_t n,
                              const qsc_obs_desc* d, const int32_t* perm, const qsc_model* m,
                              int32_t R, const float* S, const float* C, int64_t seed,
                              int32_t replicate, void* packed_out, int32_t* invalid,
                              void* stream) {
  Dims dm;
  Packed in, out;
  if (!perm || !S || !C || !packed_out || !invalid || packed == packed_out || !info_model_ok(m) ||
      R < 1 || R > QSC_MAX_R || replicate < 0 || !packed_of(packed, packed_bytes, n, d, &dm, &in) ||
      d->nbins != m->nbounds - 1)
    return QSC_EINVAL;
  packed_carve((char*)packed_out, n, dm, &out);
  // the C-format kernel's segment bounds (Kp + 1 ints) beside its edge table: the LDS a launch
  // gets without asking for more
  const size_t cshm = (size_t)(dm.Kp + 1) * sizeof(int);
  if (cshm + sizeof(float2) * (QSC_MAX_BOUNDS - 1) > 64 * 1024) return QSC_EUNSUPPORTED;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const DrawKey key = make_key(seed, replicate);
  const int RP = qsc_rank_pad(R);
  hipStream_t hs = STREAM(stream);
  // the segment tables (and the codes, replaced below)
  QSC_TRY(hipMemcpyAsync(packed_out, packed, packed_bytes, hipMemcpyDeviceToDevice, hs));
  const dim3 sg((unsigned)ceil_div(dm.ns, kWaves)), cg((unsigned)dm.nt), blk(kBlock);
#define DRAW_RD_LAUNCH(LGT, LOGV, KD)                                                           \
  do {                                                                                          \
    hipLaunchKernelGGL((draw_rd_s_kernel<LGT, LOGV>), sg, blk, 0, hs, in.s_rd, in.s_seg, n,     \
                       (int)dm.ns, d->K, d->P, RP, perm, S, C, R, lk, E, key, out.s_rd,         \
                       invalid);                                                                \
    hipLaunchKernelGGL((draw_rd_c_kernel<LGT, LOGV>), cg, blk, cshm, hs, in.c_rd, in.c_seg, n,  \
                       d->K, d->P, d->Pp, (int)dm.nt, (int)dm.nks, RP, perm, S, C, R, lk, E,    \
                       key, out.c_rd);                                                          \
  } while (0)
  DRAW_DISPATCH(DRAW_RD_LAUNCH);
#undef DRAW_RD_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_draw_list(const int32_t* k, const int32_t* p, const int32_t* occ, int64_t n,
                          int32_t K, int32_t P, const qsc_model* m, int32_t R, const float* S,
                          const float* C, int64_t seed, int32_t replicate, uint8_t* code,
                          int32_t* invalid, void* stream) {
  if (!k || !p || !S || !C || !code || !invalid || !info_model_ok(m)) return QSC_EINVAL;
  if (R < 1 || R > QSC_MAX_R || K < 1 || P < 1 || replicate < 0 || n < 1 ||
      n >= ((int64_t)1 << 31) * kBlock)
    return QSC_EINVAL;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const DrawKey key = make_key(seed, replicate);
  const dim3 grid((unsigned)ceil_div(n, kBlock)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
#define DRAW_LIST_LAUNCH(LGT, LOGV, KD)                                                       \
  hipLaunchKernelGGL((draw_list_kernel<LGT, LOGV>), grid, blk, 0, hs, k, p, occ, n, K, P, S, \
                     C, R, lk, E, key, code, invalid)
  DRAW_DISPATCH(DRAW_LIST_LAUNCH);
#undef DRAW_LIST_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
#undef DRAW_DISPATCH
