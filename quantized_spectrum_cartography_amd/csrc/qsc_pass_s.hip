// qsc_pass_s.hip — the S-pass of the fused passes (qsc_pass.cuh): spass_kernel and its entry
// points qsc_spass, qsc_spass_kslab.
#include "qsc_pass_host.cuh"

namespace {

// Persistent S-pass: a grid sized to the resident waves; each wave reads slice i+1 while it
// computes slice i, so HBM traffic and arithmetic overlap for the whole pass.  Per-slice NLL /
// ||S_new||^2 partials (DPP wave sums) keep the reductions' order independent of the grid.
template <int RP, typename E, int KIND, bool LOG, bool ADAM>
__global__ void __launch_bounds__(kSBlock, (OccS<RP, (int)sizeof(E), QSC_SPASS_WAVES>::v)) spass_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    int nslices, Lik lk, Edges E_, int nbins, int R, int K, int Pp, float* __restrict__ S,
    const float* __restrict__ C, float* __restrict__ dS, float* __restrict__ mS,
    float* __restrict__ vS, qsc_adam ad, float lambda_s, qsc_state* __restrict__ st,
    float* __restrict__ part_nll, float* __restrict__ part_nsq, int* __restrict__ sched,
    AdamCache* __restrict__ acache, int ck, int nck) {
  constexpr int CP = TP<RP, KIND>::v;
  constexpr int RH = RP / 2;  // row elements updated per lane (half row)
  // linear models evaluate the entries in a scaled form (lik_grad2)
  const float own_scale = own_scale_of<KIND, LOG>(lk);
  // all LDS carved from the 16-B aligned dynamic region (no statics ahead of it)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Scalars& sc = *reinterpret_cast<Scalars*>(smem);            // 32 B reserved
  float* Cl = smem + 8;                                        // [K][CP] (signed rows: [2K+1])
  float2* El = reinterpret_cast<float2*>(Cl + (size_t)table_floats<RP, KIND>(K));  // [nbins]

  // a wave = one slice of QSC_SLICE (32) pixel positions at a time, two lanes per pixel: lane
  // half h takes entries 2h, 2h+1 of every 4-entry chunk of the pixel's list; the halves'
  // partial dS are summed by a lane swap and each half then updates its half of the pixel's row
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int p = lane & (QSC_SLICE - 1), h = lane >> 5;
  const int W = gridDim.x * kSWaves;
  const int w = blockIdx.x * kSWaves + wave;
  // Static slice schedule: wave w of W takes slices w, 2W-1-w, 2W+w, 4W-1-w, ... (snake order
  // over the count-sorted slices balances the per-wave work)
  auto slice_of = [&](int t) { return t * W + ((t & 1) ? (W - 1 - w) : w); };
  STAMP(w, 0);
  RSTAMP(w, 28);
#if QSC_DIAG_STAMPS
  if (lane == 0 && w < kStampWaves) {
    g_stamps[w * kStamps + 26] = __builtin_amdgcn_s_getreg(0xF804);  // HW_ID: CU / SIMD / wave slot
    g_stamps[w * kStamps + 27] = __builtin_amdgcn_s_getreg(0xF814);  // XCC_ID
  }
#endif
  int s = slice_of(0);
  // 1. C^T tile reads first (the LDS staging below waits only for them), then the first slice
  const int k0 = threadIdx.x;
  float c0[RP];
#pragma unroll
  for (int r = 0; r < RP; ++r) c0[r] = C[(int64_t)min(r, R - 1) * K + min(k0, K - 1)];
  const float2 e0 = stages_edges<KIND>() ? E_.e[min(k0, nbins - 1)] : float2{};
  __builtin_amdgcn_sched_barrier(0);
  SliceIn<RP, E, ADAM> cur;
  const SliceLane ln = slice_lane<RP, E>(p, h);
  // unconditional (a wave without slices reads slice 0): a static load count lets the C^T
  // staging below wait for its own reads only
  slice_load(cur, ent, width, off, s < nslices ? s : 0, ln, S, mS, vS);
  // 2. stage C^T (rows padded to CP) and the bin edges in LDS
  {
    // branch-free (threads past K rewrite row K-1 with its own values), so the C^T reads stay
    // ahead of the slice reads
    const int kw = min(k0, K - 1);
#pragma unroll
    for (int r = 0; r < RP; r += 4)
      put_row4<RP, KIND>(Cl, K, kw, r,
                         make_float4(r < R ? c0[r] : 0.0f, r + 1 < R ? c0[r + 1] : 0.0f,
                                     r + 2 < R ? c0[r + 2] : 0.0f, r + 3 < R ? c0[r + 3] : 0.0f),
                         lk.ob_thr);
  }
  for (int k = k0 + kSBlock; k < K; k += kSBlock) {
    float v[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) v[r] = (r < R) ? C[(int64_t)r * K + k] : 0.0f;
#pragma unroll
    for (int r = 0; r < RP; r += 4)
      put_row4<RP, KIND>(Cl, K, k, r, make_float4(v[r], v[r + 1], v[r + 2], v[r + 3]), lk.ob_thr);
  }
  put_pad_row<RP, KIND>(Cl, K);
  if constexpr (stages_edges<KIND>()) {
    El[min(k0, nbins - 1)] = e0;  // branch-free like C^T
    for (int b = k0 + kSBlock; b < nbins; b += kSBlock) El[b] = E_.e[b];
  }
  if (threadIdx.x == 0) {
    if (ADAM) {
      const float nrm = sqrtf(st->normsq_s);
      sc.coef = nrm > 0.0f ? lambda_s / nrm : 0.0f;
      const int step = st->step_s + 1;
      sc.as = adam_scalars_cached(acache[step & 1], ad, step);
    }
    if (blockIdx.x == 0) {
      // book-keeping (fields no block of this kernel reads): see qsc_state
      int pend = st->pending;
      if (pend & QSC_PEND_C) st->step_c += 1;
      pend &= ~QSC_PEND_C;
      st->pending = pend | QSC_PEND_SNLL | (ADAM ? QSC_PEND_SUPD : 0);
      st->normsq_s_prev = st->normsq_s;
      st->iter += 1;
    }
  }
  __syncthreads();
  STAMP(w, 1);

  // one slice: the next slice's reads (into q) in flight during this slice's (c) arithmetic;
  // the loop below alternates the two register sets instead of copying q into c
  int i = 0;
  auto one_slice = [&](SliceIn<RP, E, ADAM>& c, SliceIn<RP, E, ADAM>& q) -> bool {
    const int s1 = slice_of(i + 1);
    const bool more = s1 < nslices;  // wave-uniform
    // 3. next slice's reads (unconditional: a last slice re-reads itself, cache-resident, so
    //    the wait counts stay static)
    QSC_DCHECK(s < nslices && off[s] + (int64_t)width[s] * QSC_SLICE <= lk.dbg_ent[0]);
    slice_load(q, ent, width, off, more ? s1 : s, ln, S, mS, vS);
    STAMP(w, 2 + 3 * i);
    const int64_t blk = (int64_t)s * QSC_SLICE * RP;  // the slice's rows (uniform)
    float sv[RP];  // rows >= R are zero in HBM (position-order padding)
#pragma unroll
    for (int r = 0; r < RP; ++r) sv[r] = c.sv[r];
    f2v own[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) own[j] = f2v{sv[2 * j], sv[2 * j + 1]} * splat2(own_scale);

    // 4. likelihood + gradient over the pixel's observed entries
    f2v accp[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) accp[j] = splat2(0.0f);
    f2v nll = splat2(0.0f);
    walk_halves<RP, E, KIND, LOG>(c.src, ln.ent, 2 * QSC_SLICE, c.j1, c.buf, own, Cl, El, lk,
                                  accp, nll);
    STAMP(w, 3 + 3 * i);
    // the two lane halves' partial dS: v_permlane32_swap (VALU) instead of an LDS shuffle
    float acc[RP];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) {
      acc[2 * j] = accp[j].x;
      acc[2 * j + 1] = accp[j].y;
    }

    // 5. epilogue: fused Adam on the lane's half row, or the raw gradient.  Padding rows
    //    (r >= R) have zero S, C and moments, so Adam keeps them exactly zero.
    float a[RH], pv[RH];
#pragma unroll
    for (int j = 0; j < RH; ++j) {
      a[j] = half_sum_pick(acc[j], acc[RH + j]);
      pv[j] = swap_lo(sv[j], sv[RH + j]);
    }
    if constexpr (ADAM) {
      float m[RH], v[RH];
#pragma unroll
      for (int j = 0; j < RH; ++j) {
        m[j] = c.mv[j];
        v[j] = c.vv[j];
      }
      float nsq = adam_row_fast<RH>(pv, m, v, a, sc.coef, sc.as, ad.project_nonneg != 0);
      st_row_wt<RH>(S + blk, ln.half, pv);
      st_row_wt<RH>(mS + blk, ln.half, m);
      st_row_wt<RH>(vS + blk, ln.half, v);
      nsq = wave_sum_dpp(nsq);
      if (lane == 0) part_nsq[s] = nsq;
    } else {
      // (K-slab, ck > 0: the reduce-scatter layout, one extra slice after every ck slices)
      const int64_t dblk = ck > 0 ? (int64_t)(s + s / ck) * QSC_SLICE * RP : blk;
      st_row_wt<RH>(dS + dblk, ln.half, a);
    }
    const float nll_w = wave_sum_dpp(nll.x + nll.y) * kLn2;
    if (lane == 0) part_nll[s] = nll_w;
    STAMP(w, 4 + 3 * i);
    s = s1;
    ++i;
    return more;
  };
  if (s < nslices) {
    SliceIn<RP, E, ADAM> nxt;
    for (;;) {
      if (!one_slice(cur, nxt)) break;
      if (!one_slice(nxt, cur)) break;
    }
  }
  // the next S-step's scalars (cfinish settles step_s + 1 in between)
  if (ADAM && blockIdx.x == 0 && threadIdx.x == 0) adam_cache_store(acache, ad, st->step_s + 2);
  if constexpr (!ADAM) {
    // K-slab (ck > 0): ||C_slab||^2 of the C this pass read -- the C the next C-step
    // differentiates -- into the extra slice of every rank's chunk of the reduce-scatter buffer,
    // so the reduce-scatter of dS delivers every rank the GLOBAL ||C||^2 with its gradient rows
    // (no all-reduce of its own).  Order of cnorm_sq (thread t < 256 accumulates t, t + 256, ...
    // then the block sum): the same bits as the C-pass's ||C||^2.  (Sc's scratch is free here.)
    if (ck > 0 && blockIdx.x == 0) {
      float s2 = 0.0f;
      if (threadIdx.x < 256)
        for (int i2 = threadIdx.x; i2 < R * K; i2 += 256) {
          const int r = i2 / K, k = i2 - r * K;
          const float c = Cl[k * CP + r];
          s2 = __builtin_fmaf(c, c, s2);
        }
      const float nsq = block_sum(s2, smem);
      if (threadIdx.x == 0)
        for (int c = 0; c < nck; ++c) dS[(int64_t)(c * (ck + 1) + ck) * QSC_SLICE * RP] = nsq;
    }
  }
  STAMP(w, kStampLast);
  RSTAMP(w, 29);
}

// the S-pass launch of qsc_spass and (ck > 0) qsc_spass_kslab
int spass_impl(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
               const int64_t* s_off, const qsc_model* m, int32_t R, float* S, const float* C,
               int32_t mode, float* dS, float* mS, float* vS, const qsc_adam* adam,
               float lambda_s, qsc_state* st, void* ws, size_t ws_bytes, void* stream, int ck,
               int nck) {
  if (!pass_args_ok(d, m, R, ws, ws_bytes) || !S || !C || !s_width || !s_off ||
      (d->s_entries > 0 && !s_entries) || !st)
    return QSC_EINVAL;
  if (mode == 0 && !dS) return QSC_EINVAL;
  if (mode == 1 && (!mS || !vS || !adam)) return QSC_EINVAL;
  if (mode != 0 && mode != 1) return QSC_EINVAL;
  const int RP = rp_of(R);
  const int kind = lik_kind(m);
  const bool sr = d->rowfmt == 1;
  const size_t shm = spass_lds(d, R, sr);
  if (shm > 160 * 1024) return QSC_EINVAL;
  PassWs w = carve(d, R, ws);
  Edges E;
  Lik lk;
  pass_lik(d, m, &E, &lk);
  const int nslices = d->Pp / QSC_SLICE;
  const int bpc = spass_bpc(RP);
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(nslices, kSWaves), (int64_t)cu_count() * bpc));
  qsc_adam ad{};
  if (adam) ad = *adam;
  hipStream_t s = STREAM(stream);
#define SPASS_LAUNCH(RPV, ET, KD, LG)                                                          \
  do {                                                                                         \
    if (mode == 1)                                                                             \
      hipLaunchKernelGGL((spass_kernel<RPV, ET, KD, LG, true>), grid, dim3(kSBlock), shm, s,   \
                         (const ET*)s_entries, s_width, s_off, nslices, lk, E, d->nbins, R,    \
                         d->K, d->Pp, S, C, dS, mS, vS, ad, lambda_s, st, w.snll, w.snsq,       \
                         w.sched, w.acache, 0, 0);                                             \
    else                                                                                       \
      hipLaunchKernelGGL((spass_kernel<RPV, ET, KD, LG, false>), grid, dim3(kSBlock), shm, s,  \
                         (const ET*)s_entries, s_width, s_off, nslices, lk, E, d->nbins, R,    \
                         d->K, d->Pp, S, C, dS, mS, vS, ad, lambda_s, st, w.snll, w.snsq,       \
                         w.sched, w.acache, ck, nck);                                          \
  } while (0)
  QSC_DISPATCH_PASS(SPASS_LAUNCH);
#undef SPASS_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // namespace

#if QSC_DEBUG
int qsc::dbg_line_s(bool clear) { return dbg_line_read(clear); }
#endif

extern "C" {

QSC_API int qsc_spass(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                      const int64_t* s_off, const qsc_model* m, int32_t R, float* S,
                      const float* C, int32_t mode, float* dS, float* mS, float* vS,
                      const qsc_adam* adam, float lambda_s, qsc_state* st, void* ws,
                      size_t ws_bytes, void* stream) {
  return spass_impl(d, s_entries, s_width, s_off, m, R, S, C, mode, dS, mS, vS, adam, lambda_s,
                    st, ws, ws_bytes, stream, 0, 0);
}

QSC_API int qsc_spass_kslab(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                            const int64_t* s_off, const qsc_model* m, int32_t R, float* S,
                            const float* C, float* dS_rs, int32_t chunk_slices, int32_t nranks,
                            qsc_state* st, void* ws, size_t ws_bytes, void* stream) {
  const int nslices = d ? d->Pp / QSC_SLICE : 0;
  if (!d || chunk_slices < 1 || nranks < 1 || (int64_t)chunk_slices * nranks < nslices ||
      !dS_rs)
    return QSC_EINVAL;
  return spass_impl(d, s_entries, s_width, s_off, m, R, S, C, 0, dS_rs, nullptr, nullptr,
                    nullptr, 0.0f, st, ws, ws_bytes, stream, chunk_slices, nranks);
}

#if QSC_DIAG_STAMPS
QSC_API int qsc_diag_stamps_s(unsigned long long* host, int n) {
  return diag_stamps_read(host, n);
}
#endif

}  // extern "C"
