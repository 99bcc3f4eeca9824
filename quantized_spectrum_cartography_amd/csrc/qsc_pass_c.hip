// qsc_pass_c.hip — the C-pass of the fused passes (qsc_pass.cuh): cpass_kernel (per 64-bin
// slice) and cpass_tile_kernel (per pixel tile) and their entry points qsc_cpass, qsc_cpass_nsq.
#include "qsc_pass_host.cuh"

namespace {

// ---------------------------------------------------------------------------------------
// C-pass, per-slice form
// ---------------------------------------------------------------------------------------
// One workgroup per (pixel tile, 64-bin frequency slice): kCParts waves, each walking a part of
// the slice's per-bin entry lists (lane = bin k) against the tile's S rows staged in LDS.
// Small workgroups (several resident per CU, dispatched as others retire) let the hardware
// balance the uneven lists and overlap one group's staging with another's arithmetic.  The
// four quarters are summed in LDS in a fixed order and written as the tile's dC slab rows.
// Block -> (tile, slice) map: the nks slices of a tile are given blocks that the round-robin
// dispatcher places on one XCD (b, b+8, b+16, ...), so the tile's S rows are read from that
// XCD's L2 after the first (speed only; any bijection is correct).
template <int RP, typename E, int KIND, bool LOG>
__global__ void __launch_bounds__(kCBlock, (Occ<RP, QSC_CPASS_WAVES>::v)) cpass_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    const int* __restrict__ kmap, int nks, int PT, int xcd_map, Lik lk, Edges E_, int nbins,
    int R, int K,
    const float* __restrict__ S, const float* __restrict__ C, float* __restrict__ slab,
    float* __restrict__ part_nll, float* __restrict__ cnsq) {
  using T = Ent<E>;
  using V4 = typename T::V4;
  constexpr int SP = TP<RP, KIND>::v;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Sl = smem;                                              // [PT][SP] (signed: [2PT+1])
  float2* El = reinterpret_cast<float2*>(Sl + (size_t)table_floats<RP, KIND>(PT));  // [nbins]
  float* Pl = Sl + (size_t)table_floats<RP, KIND>(PT) + 2 * 256;  // [kCParts][R][64]
  float* Nl = Pl + (size_t)kCParts * R * 64;                      // [kCParts]
  int t, ks;
  if (xcd_map) {
    const int j = blockIdx.x >> 3, x = blockIdx.x & 7;
    t = (j / nks) * 8 + x;
    ks = j - (j / nks) * nks;
  } else {
    t = blockIdx.x / nks;
    ks = blockIdx.x - t * nks;
  }
  const int Kp = nks * 64;
  const int part = threadIdx.x >> 6, lane = threadIdx.x & 63;
  [[maybe_unused]] const int wg = blockIdx.x * kCParts + part;  // (diagnostic stamps)
  STAMP(wg, 0);
  RSTAMP(wg, 28);

  // 1. entry read-ahead of this wave's part of the lists and C[:, k], before the staging
  const int64_t wi = (int64_t)t * nks + ks;
  const int W4 = width[wi] >> 2;
  const PartRange pr = part_range(W4, part, kCParts);
  const int j0 = pr.j0, j1 = pr.j1;
  const V4* src = reinterpret_cast<const V4*>(ent + off[wi]);
  const uint32_t lo = (uint32_t)lane * (uint32_t)sizeof(V4);
  V4 buf[kGroup];
  load_group(src, lo, 64, j0, pr.js, max(j1 - 1, 0), buf);
  const int k = kmap[wi * 64 + lane];  // this lane's bin (count-sorted order, include/qsc.h)
  float cv[RP];
#pragma unroll
  for (int r = 0; r < RP; ++r) cv[r] = C[(int64_t)min(r, R - 1) * K + min(k, K - 1)];

  // 2. stage the pixel tile: its rows are whole position slices (qsc_tile_pos, snake-dealt),
  //    each a contiguous run of QSC_SLICE rows in [Pp][RP]; 16-B reads and 16-B LDS writes at
  //    the padded pitch SP
  {
    const float4* __restrict__ src4 = reinterpret_cast<const float4*>(S);
    constexpr int V = RP / 4;  // float4 per row
    const int nt = gridDim.x / nks;
#pragma unroll 4
    for (int i = threadIdx.x; i < PT * V; i += kCBlock) {
      const int ql = i / V, c = i - ql * V;
      put_row4<RP, KIND>(Sl, PT, ql, 4 * c, src4[tile_pos(t, ql, nt) * V + c], lk.ob_thr);
    }
    put_pad_row<RP, KIND>(Sl, PT);
  }
  for (int i = threadIdx.x; i < nbins; i += kCBlock) El[i] = E_.e[i];
  __syncthreads();
  STAMP(wg, 1);

  // 3. likelihood + gradient over the part lists
  const float own_scale = own_scale_of<KIND, LOG>(lk);  // scaled form (lik_grad2)
  f2v own[RP / 2];
#pragma unroll
  for (int j = 0; j < RP / 2; ++j)
    own[j] = f2v{(2 * j < R && k < K) ? cv[2 * j] : 0.0f,
                 (2 * j + 1 < R && k < K) ? cv[2 * j + 1] : 0.0f} * splat2(own_scale);
  f2v accp[RP / 2];
#pragma unroll
  for (int j = 0; j < RP / 2; ++j) accp[j] = splat2(0.0f);
  f2v nll = splat2(0.0f);
  walk_groups<RP, E, KIND, LOG>(src, lo, 64, j0, j1, pr.js, buf, own, Sl, El, lk, accp, nll);
  STAMP(wg, 2);
  const float nll_w = wave_sum_dpp(nll.x + nll.y) * kLn2;
#pragma unroll
  for (int j = 0; j < RP / 2; ++j) {
    if (2 * j < R) Pl[((size_t)part * R + 2 * j) * 64 + lane] = accp[j].x;
    if (2 * j + 1 < R) Pl[((size_t)part * R + 2 * j + 1) * 64 + lane] = accp[j].y;
  }
  if (lane == 0) Nl[part] = nll_w;
  __syncthreads();
  STAMP(wg, 3);

  // 4. fixed-order sum of the parts -> slab rows of this tile / slice
  for (int i = threadIdx.x; i < R * 64; i += kCBlock) {
    float a = Pl[i];
#pragma unroll
    for (int pp = 1; pp < kCParts; ++pp) a += Pl[(size_t)pp * R * 64 + i];
    const int r = i >> 6, l = i & 63;
    slab[((int64_t)t * R + r) * Kp + kmap[wi * 64 + l]] = a;
  }
  if (threadIdx.x == 0) {
    float a = Nl[0];
#pragma unroll
    for (int pp = 1; pp < kCParts; ++pp) a += Nl[pp];
    part_nll[wi] = a;
  }
  if (blockIdx.x == 0) {
    // ||C||^2 for the C update's regulariser (fixed order; C is read-only in this kernel)
    const float nsq = cnorm_sq(C, R * K, Nl);  // Nl's slots are free again
    if (threadIdx.x == 0) *cnsq = nsq;
  }
  STAMP(wg, kStampLast);
  RSTAMP(wg, 29);
}

// ---------------------------------------------------------------------------------------
// C-pass, tile form: one workgroup per pixel tile covering ALL of its k-slices, so the tile's
// S rows are staged in LDS once (not once per 64-bin slice) and the whole grid is resident in
// one round (tiles hold equal mixes of dense and sparse positions, qsc_tile_pos, so the
// workgroups carry equal work).  The NW = blockDim/64 waves take units (k-slice ks, part of
// NP) u = w, w + NW, ...: lane = bin k walks part `part` of the bin's list.  With NP = 1 a
// unit's dC goes straight from registers to the slab; otherwise the NP parts are summed in
// LDS in a fixed order (bitwise deterministic; no atomics).
// ---------------------------------------------------------------------------------------
constexpr int kCTBlock = 1024;
template <int RP>
struct CTBlock {
  static constexpr int w = RP > 8 ? QSC_CTILE_W16 : kCTBlock / 64;  // max waves
  static constexpr int v = 64 * w;
};

template <int RP, typename E, int KIND, bool LOG>
__global__ void __launch_bounds__(CTBlock<RP>::v) cpass_tile_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    const int* __restrict__ kmap, int nks, int NP, int PT, Lik lk, Edges E_, int nbins, int R,
    int K, int ct_in,
    const float* __restrict__ S, const float* __restrict__ C, float* __restrict__ slab,
    float* __restrict__ part_nll, float* __restrict__ cnsq, float* __restrict__ snsq_out) {
  using T = Ent<E>;
  using V4 = typename T::V4;
  constexpr int SP = TP<RP, KIND>::v;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int NW = blockDim.x >> 6;
  const int U = nks * NP;
  float* Sl = smem;                                              // [PT][SP] (signed: [2PT+1])
  float2* El = reinterpret_cast<float2*>(Sl + (size_t)table_floats<RP, KIND>(PT));  // [nbins]
  float* Pl = Sl + (size_t)table_floats<RP, KIND>(PT) + 2 * 256;  // [U][R][64]   (NP > 1)
  float* Nl = Pl + (NP > 1 ? (size_t)U * R * 64 : 0);             // [U] / [NW]
  // (ct) C^T staged next to the tile, [K][RP] (rows r >= R unread), for the units' C columns
  // (not for 32-bit entries below rank 16: their 16-wave walk has no VGPRs to spare)
  float* Ctl = Nl + ((max(U, 16) + 3) & ~3);
  const bool ct = (RP > 8 || sizeof(E) == 2) && ct_in != 0;
  const int t = blockIdx.x;
  const int Kp = nks * 64;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const float own_scale = own_scale_of<KIND, LOG>(lk);  // scaled form (lik_grad2)
  [[maybe_unused]] const int wg = blockIdx.x * CTBlock<RP>::w + w;  // (diagnostic stamps)
  STAMP(wg, 0);
  RSTAMP(wg, 28);

  // 1. read-ahead of the first unit's entries and C column, ahead of the staging
  int u = w;
  V4 buf[kGroup];
  float cv[RP];
  int wi = 0, j0 = 0, j1 = 0, js = 1, k = 0;
  const V4* src = nullptr;
  const uint32_t lo = (uint32_t)lane * (uint32_t)sizeof(V4);
  // the unit's C column: from the staged C^T (ct; after the staging barrier) or from C
  auto unit_cols = [&]() {
    if (ct) {
#pragma unroll
      for (int r = 0; r < RP; r += 4) {
        const float4 q = *reinterpret_cast<const float4*>(Ctl + (size_t)min(k, K - 1) * RP + r);
        cv[r] = q.x;
        cv[r + 1] = q.y;
        cv[r + 2] = q.z;
        cv[r + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int r = 0; r < RP; ++r) cv[r] = C[(int64_t)min(r, R - 1) * K + min(k, K - 1)];
    }
  };
  auto unit_begin = [&](int uu, bool cols) {
    const int ks = uu / NP, part = uu - ks * NP;
    wi = t * nks + ks;
    const int W4 = width[wi] >> 2;
    const PartRange pr = part_range(W4, part, NP);
    j0 = pr.j0;
    j1 = pr.j1;
    js = pr.js;
    src = reinterpret_cast<const V4*>(ent + off[wi]);
    QSC_DCHECK(off[wi] + (int64_t)width[wi] * 64 <= lk.dbg_ent[1]);
    load_group(src, lo, 64, j0, js, max(j1 - 1, 0), buf);
    k = kmap[wi * 64 + lane];  // this lane's bin (count-sorted order)
    QSC_DCHECK(k >= 0 && k < Kp);
    if (cols) unit_cols();
  };
  // the tile's S rows are read first, into registers when they fit QSC_CTILE_SREG float4 per
  // thread: the unit's reads below wait on their own dependent reads (bounds -> entries, bin ->
  // C column), so rows issued after them arrived one round trip later
  const float4* __restrict__ src4 = reinterpret_cast<const float4*>(S);
  constexpr int V = RP / 4;  // float4 per row
  // (not for 32-bit entries below rank 16: their 16-wave walk has no VGPRs to spare)
  constexpr bool kSRok = QSC_CTILE_SREG > 0 && (RP > 8 || sizeof(E) == 2);
  constexpr int kSR = kSRok ? QSC_CTILE_SREG : 1;
  const bool sreg = kSRok && PT * V <= kSR * (int)blockDim.x;
  float4 srow[kSR];
  if (sreg) {
#pragma unroll
    for (int q = 0; q < kSR; ++q) {
      const int i = (int)threadIdx.x + q * (int)blockDim.x;
      const int ql = i / V, c = i - ql * V;
      if (i < PT * V) srow[q] = src4[tile_pos(t, ql, (int)gridDim.x) * V + c];
    }
  }
  // (ct) the C^T reads: no dependency, so they ride with the S rows' round trip
  constexpr int kCT = 4;  // C floats per thread held in registers (R K <= kCT * blockDim)
  float ctv[kCT];
  if (ct) {
#pragma unroll
    for (int q = 0; q < kCT; ++q) {
      const int i = (int)threadIdx.x + q * (int)blockDim.x;
      if (i < R * K) ctv[q] = C[i];
    }
  }
  if (u < U) unit_begin(u, !ct);

  // 2. stage the pixel tile (whole position slices, 16-B reads / writes at pitch SP)
  {
    const int nt = gridDim.x;
    if (ct) {
#pragma unroll
      for (int q = 0; q < kCT; ++q) {
        const int i = (int)threadIdx.x + q * (int)blockDim.x;
        if (i < R * K) {
          const int r = i / K, kk = i - r * K;
          Ctl[(size_t)kk * RP + r] = ctv[q];
        }
      }
    }
    if (sreg) {
#pragma unroll
      for (int q = 0; q < kSR; ++q) {
        const int i = (int)threadIdx.x + q * (int)blockDim.x;
        const int ql = i / V, c = i - ql * V;
        if (i < PT * V) put_row4<RP, KIND>(Sl, PT, ql, 4 * c, srow[q], lk.ob_thr);
      }
    } else {
#pragma unroll 4
      for (int i = threadIdx.x; i < PT * V; i += blockDim.x) {
        const int ql = i / V, c = i - ql * V;
        put_row4<RP, KIND>(Sl, PT, ql, 4 * c, src4[tile_pos(t, ql, nt) * V + c], lk.ob_thr);
      }
    }
    put_pad_row<RP, KIND>(Sl, PT);
  }
  for (int i = threadIdx.x; i < nbins; i += blockDim.x) El[i] = E_.e[i];
  __syncthreads();
  STAMP(wg, 1);
  if (ct && u < U) unit_cols();

  // 3. units: likelihood + gradient over the part lists
  for (; u < U; u += NW) {
    f2v own[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j)
      own[j] = f2v{(2 * j < R && k < K) ? cv[2 * j] : 0.0f,
                   (2 * j + 1 < R && k < K) ? cv[2 * j + 1] : 0.0f} * splat2(own_scale);
    f2v accp[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) accp[j] = splat2(0.0f);
    f2v nll = splat2(0.0f);
    walk_groups<RP, E, KIND, LOG>(src, lo, 64, j0, j1, js, buf, own, Sl, El, lk, accp, nll);
    const float nll_w = wave_sum_dpp(nll.x + nll.y) * kLn2;
    if (NP == 1) {
      // the unit is the whole (tile, k-slice): its slab rows straight from registers
#pragma unroll
      for (int j = 0; j < RP / 2; ++j) {
        if (2 * j < R) slab[((int64_t)t * R + 2 * j) * Kp + k] = accp[j].x;
        if (2 * j + 1 < R) slab[((int64_t)t * R + 2 * j + 1) * Kp + k] = accp[j].y;
      }
      if (lane == 0) part_nll[wi] = nll_w;
    } else {
#pragma unroll
      for (int j = 0; j < RP / 2; ++j) {
        if (2 * j < R) Pl[((size_t)u * R + 2 * j) * 64 + lane] = accp[j].x;
        if (2 * j + 1 < R) Pl[((size_t)u * R + 2 * j + 1) * 64 + lane] = accp[j].y;
      }
      if (lane == 0) Nl[u] = nll_w;
    }
    if (u + NW < U) unit_begin(u + NW, true);
  }
  STAMP(wg, 2);

  // 3b. (qsc_cpass_nsq, K-slab) every slice's ||S||^2 partial from the staged tile, in
  //     slice_nsq_kernel's lane mapping (lane p + 32 h: position p, half row h) and order, so
  //     the values are bit-identical to qsc_slice_nsq's / the shard updates' partials
  if (snsq_out) {
    constexpr int RH = RP / 2;
    const int nsl = PT / QSC_SLICE, nt = gridDim.x;
    const int p = lane & (QSC_SLICE - 1), h = lane >> 5;
    for (int ls = w; ls < nsl; ls += NW) {
      const float* row = Sl + (size_t)(ls * QSC_SLICE + p) * SP + h * RH;
      float nsq = 0.0f;
#pragma unroll
      for (int j = 0; j < RH; ++j) nsq = __builtin_fmaf(row[j], row[j], nsq);
      nsq = wave_sum(nsq);
      if (lane == 0) snsq_out[tile_pos(t, ls * QSC_SLICE, nt) / QSC_SLICE] = nsq;
    }
  }

  // 4. fixed-order sum of the parts -> slab rows of this tile (NP > 1)
  if (NP > 1) {
    __syncthreads();
    STAMP(wg, 3);
    for (int i = threadIdx.x; i < nks * R * 64; i += blockDim.x) {
      const int ks = i / (R * 64), rl = i - ks * (R * 64);
      const float* p = Pl + (size_t)ks * NP * R * 64 + rl;
      float a = p[0];
      for (int pp = 1; pp < NP; ++pp) a += p[(size_t)pp * R * 64];
      const int r = rl >> 6, l = rl & 63;
      slab[((int64_t)t * R + r) * Kp + kmap[((int64_t)t * nks + ks) * 64 + l]] = a;
    }
    for (int ks = threadIdx.x; ks < nks; ks += blockDim.x) {
      float a = Nl[ks * NP];
      for (int pp = 1; pp < NP; ++pp) a += Nl[ks * NP + pp];
      part_nll[t * nks + ks] = a;
    }
  }
  if (blockIdx.x == 0) {
    // ||C||^2 for the C update's regulariser (fixed order; C is read-only in this kernel)
    __syncthreads();
    const float nsq = cnorm_sq(C, R * K, Nl);  // Nl's slots are free again
    if (threadIdx.x == 0) *cnsq = nsq;
  }
  STAMP(wg, kStampLast);
  RSTAMP(wg, 29);
}

// the C-pass launch of qsc_cpass and (nsq: with the per-slice ||S||^2 partials) qsc_cpass_nsq
int cpass_impl(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
               const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m, int32_t R,
               const float* S, const float* C, void* ws, size_t ws_bytes, void* stream, bool nsq) {
  if (!pass_args_ok(d, m, R, ws, ws_bytes) || !S || !C || !c_width || !c_off || !c_kmap ||
      (d->c_entries > 0 && !c_entries))
    return QSC_EINVAL;
  const int RP = rp_of(R);
  const int kind = lik_kind(m);
  const bool sr = d->rowfmt == 1;
  const size_t shm = cpass_lds(d, R, sr);
  PassWs w = carve(d, R, ws);
  Edges E;
  Lik lk;
  pass_lik(d, m, &E, &lk);
  hipStream_t s = STREAM(stream);
  if (QSC_CPASS_TILE) {
    // tile form: up to 16 waves per tile, the partition of tile_parts
    const int nks = d->nks;
    int NP = 1;
    const bool tile = tile_parts(d, R, sr, &NP);
    const int U = nks * NP;
    size_t tshm = cpass_tile_lds(d->PT, R, nks, NP, sr);
    if (tile) {
      const dim3 tb((unsigned)(64 * std::min(U, RP > 8 ? QSC_CTILE_W16 : QSC_CTILE_MAXW)));
      // C^T staged in LDS when it fits next to the tile and in the threads' registers (kCT = 4
      // floats each): the units' C columns then come from LDS, not from a read that depends on
      // the bin map (the partition -- tile_parts -- is sized without it)
      const size_t ct_bytes = 16 + (size_t)d->K * RP * 4;  // [K][RP] (+ alignment)
      const int ct = (QSC_CTILE_CT && (int64_t)R * d->K <= 4 * (int64_t)tb.x &&
                      tshm + ct_bytes <= 160 * 1024) ? 1 : 0;
      if (ct) tshm += ct_bytes;
#define CPASS_TILE_LAUNCH(RPV, ET, KD, LG)                                                     \
  hipLaunchKernelGGL((cpass_tile_kernel<RPV, ET, KD, LG>), dim3((unsigned)d->ntiles), tb, tshm, \
                     s, (const ET*)c_entries, c_width, c_off, c_kmap, nks, NP, d->PT, lk, E,     \
                     d->nbins, R, d->K, ct, S, C, w.slab, w.cnll, w.cnsq,                      \
                     nsq ? w.snsq : nullptr)
      QSC_DISPATCH_PASS(CPASS_TILE_LAUNCH);
#undef CPASS_TILE_LAUNCH
      QSC_CHECK_LAUNCH();
      return QSC_OK;
    }
  }
  if (shm > 160 * 1024) return QSC_EINVAL;
  const int xcd_map = (d->ntiles % 8) == 0 ? 1 : 0;
  const dim3 grid((unsigned)((int64_t)d->ntiles * d->nks));
#define CPASS_LAUNCH(RPV, ET, KD, LG)                                                          \
  hipLaunchKernelGGL((cpass_kernel<RPV, ET, KD, LG>), grid, dim3(kCBlock), shm, s,           \
                     (const ET*)c_entries, c_width, c_off, c_kmap, d->nks, d->PT, xcd_map, lk, \
                     E, d->nbins, R, d->K, S, C, w.slab, w.cnll, w.cnsq)
  QSC_DISPATCH_PASS(CPASS_LAUNCH);
#undef CPASS_LAUNCH
  QSC_CHECK_LAUNCH();
  if (nsq) return qsc_slice_nsq(d, R, S, ws, ws_bytes, stream);  // (per-slice form: unfused)
  return QSC_OK;
}

}  // namespace

#if QSC_DEBUG
int qsc::dbg_line_c(bool clear) { return dbg_line_read(clear); }
#endif

extern "C" {

QSC_API int qsc_cpass(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                      const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m, int32_t R,
                      const float* S, const float* C, void* ws, size_t ws_bytes, void* stream) {
  return cpass_impl(d, c_entries, c_width, c_off, c_kmap, m, R, S, C, ws, ws_bytes, stream,
                    false);
}

QSC_API int qsc_cpass_nsq(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                          const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                          int32_t R, const float* S, const float* C, void* ws, size_t ws_bytes,
                          void* stream) {
  return cpass_impl(d, c_entries, c_width, c_off, c_kmap, m, R, S, C, ws, ws_bytes, stream,
                    true);
}

#if QSC_DIAG_STAMPS
QSC_API int qsc_diag_stamps_c(unsigned long long* host, int n) {
  return diag_stamps_read(host, n);
}
#endif

}  // extern "C"
