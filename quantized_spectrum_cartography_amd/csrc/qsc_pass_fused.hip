// qsc_pass_fused.hip — the fused launch of the fused passes (qsc_pass.cuh): scfused_kernel, one
// S-step and the next C-pass per pixel tile, and its entry point qsc_scpass.
#include "qsc_pass_host.cuh"

namespace {

// ---------------------------------------------------------------------------------------
// Fused S-step + next C-pass, one workgroup per C-pass pixel tile (16 waves; 8 at rank 16).
// The tile's whole position slices (tile_pos) get their S-step first -- likelihood, dS and
// Adam exactly as spass_kernel, wave w taking the tile's slices w, 2*16-1-w, ... (snake over
// the count-sorted slices) -- and the new S rows are written to HBM (S, mS, vS) AND into the
// LDS tile; after one barrier the same workgroup runs the tile's C-pass units exactly as
// cpass_tile_kernel, at the new S, for the NEXT iteration's C-step.  So one launch replaces
// spass + cpass: no kernel boundary between them and no re-read / staging of the S tile (the
// C-pass of iteration i+1 reads only S_i of its own tile, and C_i, which the S-step also used).
// Kernel sequence semantics are unchanged: spass_i then cpass_{i+1} (same partials, same
// state protocol), so a solver runs cpass+cfinish, then (fused + cfinish) x (n-1), then spass.
// ---------------------------------------------------------------------------------------
// fused launch block: 16 waves (4 per SIMD, 128 VGPRs) up to rank 8; 8 waves at rank 16, whose
// two slice register sets and 16-float rows need up to 256 VGPRs (2 waves per SIMD)
template <int RP>
struct FusedBlock {
  static constexpr int v = RP > 8 ? 512 : 64 * QSC_FUSED_WAVES;
  static constexpr int wpe = RP > 8 ? 2 : (QSC_FUSED_WAVES + 3) / 4;  // waves per SIMD
};

// (device-function form: the 2 KB edge table by reference; kernel form below: by value --
// a kernel argument is never a reference, which would hand the device a host address)
#define QSC_SCF_PARAMS                                                                         \
  const E *__restrict__ s_ent, const int *__restrict__ s_width, const int64_t *__restrict__ s_off, \
      const E *__restrict__ c_ent, const int *__restrict__ c_width,                                \
      const int64_t *__restrict__ c_off, const int *__restrict__ c_kmap, int nks, int NP, int PT,  \
      Lik lk, const Edges &E_, int nbins, int R, int K, float *__restrict__ S,                    \
      const float *__restrict__ C,                                                                \
      float *__restrict__ mS, float *__restrict__ vS, qsc_adam ad, float lambda_s,                \
      qsc_state *__restrict__ st, float *__restrict__ part_nll_s, float *__restrict__ part_nsq_s, \
      float *__restrict__ slab, float *__restrict__ part_nll_c, float *__restrict__ cnsq,         \
      AdamCache *__restrict__ acache
#define QSC_SCF_KPARAMS                                                                        \
  const E *__restrict__ s_ent, const int *__restrict__ s_width, const int64_t *__restrict__ s_off, \
      const E *__restrict__ c_ent, const int *__restrict__ c_width,                                \
      const int64_t *__restrict__ c_off, const int *__restrict__ c_kmap, int nks, int NP, int PT,  \
      Lik lk, Edges E_, int nbins, int R, int K, float *__restrict__ S,                           \
      const float *__restrict__ C,                                                                \
      float *__restrict__ mS, float *__restrict__ vS, qsc_adam ad, float lambda_s,                \
      qsc_state *__restrict__ st, float *__restrict__ part_nll_s, float *__restrict__ part_nsq_s, \
      float *__restrict__ slab, float *__restrict__ part_nll_c, float *__restrict__ cnsq,         \
      AdamCache *__restrict__ acache
#define QSC_SCF_ARGS                                                                            \
  s_ent, s_width, s_off, c_ent, c_width, c_off, c_kmap, nks, NP, PT, lk, E_, nbins, R, K, S, C, mS, \
      vS, ad, lambda_s, st, part_nll_s, part_nsq_s, slab, part_nll_c, cnsq, acache


// One pixel tile t of nt of the fused launch (scfused_kernel: t = the workgroup).  C is
// read-only here.
template <int RP, typename E, int KIND, bool LOG>
__device__ __forceinline__ void scfused_tile(QSC_SCF_PARAMS, const int t, const int nt,
                                             const unsigned tidx) {
  using V4 = typename Ent<E>::V4;
  constexpr int CP = TP<RP, KIND>::v;  // C^T row pitch == S tile row pitch
  constexpr int RH = RP / 2;
  constexpr bool ADAM = true;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Scalars& sc = *reinterpret_cast<Scalars*>(smem);                // 32 B
  float* Cl = smem + 8;                                            // [K][CP] (signed: 2K+1)
  float2* El = reinterpret_cast<float2*>(Cl + (size_t)table_floats<RP, KIND>(K));  // [256]
  float* Sl = reinterpret_cast<float*>(El + 256);                   // [PT][CP] (signed: 2PT+1)
  float* Pl = Sl + (size_t)table_floats<RP, KIND>(PT);              // [U][R][64]  (NP > 1)

  const int NW = blockDim.x >> 6;
  const int U = nks * NP;
  float* Nl = Pl + (NP > 1 ? (size_t)U * R * 64 : 0);               // [max(U,16)]
  const int Kp = nks * 64;
  const int w = __builtin_amdgcn_readfirstlane(tidx >> 6), lane = tidx & 63;
  const int p = lane & (QSC_SLICE - 1), h = lane >> 5;
  const float own_scale = own_scale_of<KIND, LOG>(lk);
  const int nsl = PT / QSC_SLICE;  // slices per tile
  // this wave's n-th slice of the tile (local index) and its global slice
  auto local_of = [&](int n) { return n * NW + ((n & 1) ? (NW - 1 - w) : w); };
  auto global_of = [&](int i) { return i * nt + ((i & 1) ? (nt - 1 - t) : t); };
  [[maybe_unused]] const int wg = t * (FusedBlock<RP>::v / 64) + w;  // (stamps)
  STAMP(wg, 0);
  RSTAMP(wg, 28);
#if QSC_DIAG_STAMPS
  if (lane == 0 && wg < kStampWaves) g_stamps[wg * kStamps + 26] = __builtin_amdgcn_s_getreg(0xF804);
#endif

  // 1. C^T / edge / state reads first (the LDS staging then waits only for them: vmcnt
  //    retires in issue order), then the first slice's reads, then the staging
  const int k0 = tidx;
  // C^T from 16-B reads of the [R][K] C: thread i holds C's flat floats 4i..4i+3 (one row r,
  // four consecutive bins) and writes them transposed; 32x fewer read instructions than a
  // float per (thread, row)
  const int n4 = (R * K) >> 2;
  const bool cvec = (K & 3) == 0 && ((reinterpret_cast<uintptr_t>(C) & 15) == 0);
  float4 cq = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float c0[RP];
  if (cvec) {
    cq = reinterpret_cast<const float4*>(C)[min(k0, n4 - 1)];
  } else {
#pragma unroll
    for (int r = 0; r < RP; ++r) c0[r] = C[(int64_t)min(r, R - 1) * K + min(k0, K - 1)];
  }
  const float2 e0 = stages_edges<KIND>() ? E_.e[min(k0, nbins - 1)] : float2{};
  // the bins of this thread's first two part-sum outputs (step 4), read now: at the tail they
  // would be a dependent global read after the last unit
  const int nps = nks * R * 64;
  int km_pf[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = min(k0 + j * (int)blockDim.x, nps - 1);
    const int ks = i / (R * 64), l = (i - ks * (R * 64)) & 63;
    km_pf[j] = c_kmap[((int64_t)t * nks + ks) * 64 + l];
  }
  float nsq_s = 0.0f;
  int step_s = 0;
  AdamCache ac0{}, ac1{};
  if (tidx == 0) {
    nsq_s = st->normsq_s;
    step_s = st->step_s;
    ac0 = acache[0];  // both slots: no dependent read on step_s
    ac1 = acache[1];
  }
  __builtin_amdgcn_sched_barrier(0);
  STAMP(wg, 13);  // (the C^T, edge, state reads are issued)
  int il = local_of(0);
  SliceIn<RP, E, ADAM> cur;
  const SliceLane ln = slice_lane<RP, E>(p, h);
  // First reads before the staging: waves w < QSC_EARLY_WAVES read their first slice now, the
  // others after the staging barrier.  The C^T reads the staging waits for take 2.5-3 us at a
  // launch's start (profiles/r05/stamps_f.log), long enough to cover every wave's first slice:
  // with all 16 waves early the fused launch is 0.6-0.9 us shorter at C3 than with the oldest
  // wave of each SIMD only (QSC_EARLY_WAVES=4, round 3's choice when the staging was shorter;
  // profiles/r05/ab_early_waves.log).
  const bool early = w < QSC_EARLY_WAVES;
  auto stage = [&]() {
    STAMP(wg, 14);  // (the wave's first-slice reads, if early, are issued)
    if (cvec) {
      const int Ko = sr_off(K);  // the negated half of a signed-row C^T table
      auto put = [&](int i, const float4& v) {
        const int f = 4 * i, r = f / K, k = f - r * K;
        Cl[k * CP + r] = v.x;
        Cl[(k + 1) * CP + r] = v.y;
        Cl[(k + 2) * CP + r] = v.z;
        Cl[(k + 3) * CP + r] = v.w;
        if constexpr (is_sr(KIND)) {
          Cl[(Ko + k) * CP + r] = -v.x;
          Cl[(Ko + k + 1) * CP + r] = -v.y;
          Cl[(Ko + k + 2) * CP + r] = -v.z;
          Cl[(Ko + k + 3) * CP + r] = -v.w;
        }
      };
      if (k0 < n4) put(k0, cq);
      for (int i = k0 + (int)blockDim.x; i < n4; i += blockDim.x)
        put(i, reinterpret_cast<const float4*>(C)[i]);
      for (int i = k0; i < K * (RP - R); i += blockDim.x) {  // rows R..RP-1 are zero
        const int k = i / (RP - R), r = R + (i - k * (RP - R));
        Cl[k * CP + r] = 0.0f;
        if constexpr (is_sr(KIND)) Cl[(Ko + k) * CP + r] = -0.0f;
      }
      if constexpr (is_sr(KIND))
        for (int k = k0; k < K; k += blockDim.x) put_th<RP, KIND>(Cl, K, k, lk.ob_thr);
    } else {
      const int kw = min(k0, K - 1);  // branch-free: threads past K rewrite row K-1
#pragma unroll
      for (int r = 0; r < RP; r += 4)
        put_row4<RP, KIND>(Cl, K, kw, r,
                           make_float4(r < R ? c0[r] : 0.0f, r + 1 < R ? c0[r + 1] : 0.0f,
                                       r + 2 < R ? c0[r + 2] : 0.0f, r + 3 < R ? c0[r + 3] : 0.0f),
                           lk.ob_thr);
      for (int k = k0 + (int)blockDim.x; k < K; k += blockDim.x) {
        float v[RP];
#pragma unroll
        for (int r = 0; r < RP; ++r) v[r] = (r < R) ? C[(int64_t)r * K + k] : 0.0f;
#pragma unroll
        for (int r = 0; r < RP; r += 4)
          put_row4<RP, KIND>(Cl, K, k, r, make_float4(v[r], v[r + 1], v[r + 2], v[r + 3]),
                             lk.ob_thr);
      }
    }
    put_pad_row<RP, KIND>(Cl, K);
    if constexpr (is_sr(KIND)) {
      // the S tile's threshold column and pad row (its S values are written by the S-step)
      for (int q = k0; q < PT; q += blockDim.x) put_th<RP, KIND>(Sl, PT, q, lk.ob_thr);
      put_pad_row<RP, KIND>(Sl, PT);
    }
    if constexpr (stages_edges<KIND>()) {
      El[min(k0, nbins - 1)] = e0;
      for (int b = k0 + (int)blockDim.x; b < nbins; b += blockDim.x) El[b] = E_.e[b];
    }
    STAMP(wg, 10);  // C^T rows written (its reads landed)
    if (tidx == 0) {
      const float nrm = sqrtf(nsq_s);
      sc.coef = nrm > 0.0f ? lambda_s / nrm : 0.0f;
      sc.as = adam_scalars_cached(((step_s + 1) & 1) ? ac1 : ac0, ad, step_s + 1);
      if (t == 0) {
        // book-keeping of spass_kernel (mode 1)
        int pend = st->pending;
        if (pend & QSC_PEND_C) st->step_c += 1;
        pend &= ~QSC_PEND_C;
        st->pending = pend | QSC_PEND_SNLL | QSC_PEND_SUPD;
        st->normsq_s_prev = nsq_s;
        st->iter = st->iter + 1;
      }
    }
    STAMP(wg, 11);  // (wave 0: the scalars are set)
  };
  // (late waves' first reads right after their own staging instead of after the barrier:
  // within noise, round 5, gpurun_out/r05q; not kept)
  if (early) {
    slice_load(cur, s_ent, s_width, s_off, global_of(il < nsl ? il : 0), ln, S, mS, vS);
    stage();
  } else {
    stage();
  }
  __syncthreads();
  if (!early) slice_load(cur, s_ent, s_width, s_off, global_of(il < nsl ? il : 0), ln, S, mS, vS);
  STAMP(wg, 1);
  if (t == 0) {
    // ||C_i||^2 for the next C update's regulariser, from the staged C^T at the start (as a
    // chain of dependent global reads at the end it delayed the last workgroup); the order of
    // cnorm_sq: thread t < 256 accumulates flat indices t, t + 256, ..., then block_sum
    float s2 = 0.0f;
    if (tidx < 256)
      for (int i = tidx; i < R * K; i += 256) {
        const int r = i / K, k = i - r * K;
        const float c = Cl[k * CP + r];
        s2 = __builtin_fmaf(c, c, s2);
      }
    const float nsq = block_sum(s2, Nl);
    if (tidx == 0) *cnsq = nsq;
  }

  // 2. S-step over the wave's slices (next slice's reads in flight; the two register sets
  //    alternate, as in spass_kernel)
  int n = 0;
  auto one_slice = [&](SliceIn<RP, E, ADAM>& c, SliceIn<RP, E, ADAM>& q) -> bool {
    const int il1 = local_of(n + 1);
    const bool more = il1 < nsl;
    const int s = global_of(il);
    prio_level(3 - min(3, n));  // (uniform: the wave's n-th slice)
    // the first slice's reads land before the second slice's are issued: the launch's first
    // burst is then one slice per wave, not two
    if (n == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      STAMP(wg, 12);
    }
    QSC_DCHECK(s < nt * nsl && s_off[s] + (int64_t)s_width[s] * QSC_SLICE <= lk.dbg_ent[0]);
    slice_load(q, s_ent, s_width, s_off, more ? global_of(il1) : s, ln, S, mS, vS);
    float sv[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) sv[r] = c.sv[r];
    f2v own[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) own[j] = f2v{sv[2 * j], sv[2 * j + 1]} * splat2(own_scale);
    f2v accp[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) accp[j] = splat2(0.0f);
    f2v nll = splat2(0.0f);
    walk_halves<RP, E, KIND, LOG>(c.src, ln.ent, 2 * QSC_SLICE, c.j1, c.buf, own, Cl, El, lk,
                                  accp, nll);
    float acc[RP];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) {
      acc[2 * j] = accp[j].x;
      acc[2 * j + 1] = accp[j].y;
    }
    float a[RH], pv[RH], m[RH], v[RH];
#pragma unroll
    for (int j = 0; j < RH; ++j) {
      a[j] = half_sum_pick(acc[j], acc[RH + j]);
      pv[j] = swap_lo(sv[j], sv[RH + j]);
      m[j] = c.mv[j];
      v[j] = c.vv[j];
    }
    float nsq = adam_row_fast<RH>(pv, m, v, a, sc.coef, sc.as, ad.project_nonneg != 0);
    const int64_t blk = (int64_t)s * QSC_SLICE * RP;  // the slice's rows (uniform)
    st_row_wt<RH>(S + blk, ln.half, pv);
    st_row_wt<RH>(mS + blk, ln.half, m);
    st_row_wt<RH>(vS + blk, ln.half, v);
    st_row<RH>(Sl + (il * QSC_SLICE + p) * CP + h * RH, pv);  // the tile row, for the C-pass
    if constexpr (is_sr(KIND)) {
      float nv[RH];
#pragma unroll
      for (int j = 0; j < RH; ++j) nv[j] = -pv[j];
      st_row<RH>(Sl + (sr_off(PT) + il * QSC_SLICE + p) * CP + h * RH, nv);
    }
    nsq = wave_sum_dpp(nsq);
    if (lane == 0) part_nsq_s[s] = nsq;
    const float nll_w = wave_sum_dpp(nll.x + nll.y) * kLn2;
    if (lane == 0) part_nll_s[s] = nll_w;
    STAMP(wg, 5 + min(n, 8));  // end of the wave's n-th slice
    il = il1;
    ++n;
    return more;
  };
  // 3. C-pass units of the tile at the new S (cpass_tile_kernel steps 1, 3, 4).
  int u = w;
  V4 buf[kGroup];
  float cv[RP];
  int wi = 0, jb = 0, je = 0, js = 1, k = 0;
  const V4* src = nullptr;
  const uint32_t lo = (uint32_t)lane * (uint32_t)sizeof(V4);
  // unit uu: its list block and chunk range, the read-ahead of its first chunk group, its bin
  // and C column
  auto unit_begin = [&](int uu) {
    const int ks = uu / NP, part = uu - ks * NP;
    wi = t * nks + ks;
    const int W4 = c_width[wi] >> 2;
    const PartRange pr = part_range(W4, part, NP);
    jb = pr.j0;
    je = pr.j1;
    js = pr.js;
    src = reinterpret_cast<const V4*>(c_ent + c_off[wi]);
    QSC_DCHECK(c_off[wi] + (int64_t)c_width[wi] * 64 <= lk.dbg_ent[1]);
    load_group(src, lo, 64, jb, js, max(pr.j1 - 1, 0), buf);
    k = c_kmap[wi * 64 + lane];  // this lane's bin (count-sorted order)
    QSC_DCHECK(k >= 0 && k < Kp);
#pragma unroll
    for (int r = 0; r < RP; ++r) cv[r] = Cl[min(k, K - 1) * CP + r];  // C_i, as the S-step used
  };
  f2v cnll = splat2(0.0f);
  auto unit_walk = [&](f2v (&accp)[RP / 2]) {
    f2v own[RP / 2];
#pragma unroll
    for (int j = 0; j < RP / 2; ++j)
      own[j] = f2v{(2 * j < R && k < K) ? cv[2 * j] : 0.0f,
                   (2 * j + 1 < R && k < K) ? cv[2 * j + 1] : 0.0f} * splat2(own_scale);
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) accp[j] = splat2(0.0f);
    walk_groups<RP, E, KIND, LOG>(src, lo, 64, jb, je, js, buf, own, Sl, El, lk, accp, cnll);
  };
  auto to_pl = [&](const f2v (&accp)[RP / 2]) {
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) {
      if (2 * j < R) Pl[((size_t)u * R + 2 * j) * 64 + lane] = accp[j].x;
      if (2 * j + 1 < R) Pl[((size_t)u * R + 2 * j + 1) * 64 + lane] = accp[j].y;
    }
  };

  // 2. S-step over the wave's slices (next slice's reads in flight; the two register sets
  //    alternate, as in spass_kernel)
  if (il < nsl) {
    SliceIn<RP, E, ADAM> nxt;
    const bool more = one_slice(cur, nxt);  // round 1 (peeled: its first-slice wait, n == 0)
    if (more)
      for (;;) {
        if (!one_slice(nxt, cur)) break;
        if (!one_slice(cur, nxt)) break;
      }
  }

  // the next launch's S-step scalars, by the oldest wave of block 0 (it has slack: its slices
  // are done long before the tile barrier)
  if (t == 0 && tidx == 0) adam_cache_store(acache, ad, step_s + 2);

  STAMP(wg, 2);
  if (u < U) unit_begin(u);
  __syncthreads();  // the whole S tile is in LDS
  STAMP(wg, 3);
  for (; u < U; u += NW) {
    f2v accp[RP / 2];
    unit_walk(accp);
    const float nll_w = wave_sum_dpp(cnll.x + cnll.y) * kLn2;
    cnll = splat2(0.0f);
    if (NP == 1) {
#pragma unroll
      for (int j = 0; j < RP / 2; ++j) {
        if (2 * j < R) slab[((int64_t)t * R + 2 * j) * Kp + k] = accp[j].x;
        if (2 * j + 1 < R) slab[((int64_t)t * R + 2 * j + 1) * Kp + k] = accp[j].y;
      }
      if (lane == 0) part_nll_c[wi] = nll_w;
    } else {
      to_pl(accp);
      if (lane == 0) Nl[u] = nll_w;
    }
    if (u + NW < U) unit_begin(u + NW);
  }
  STAMP(wg, 4);
  if (NP > 1) {
    __syncthreads();
    for (int i = tidx, j = 0; i < nks * R * 64; i += blockDim.x, ++j) {
      const int ks = i / (R * 64), rl = i - ks * (R * 64);
      const float* pp0 = Pl + (size_t)ks * NP * R * 64 + rl;
      float acc = pp0[0];
      for (int pp = 1; pp < NP; ++pp) acc += pp0[(size_t)pp * R * 64];
      const int r = rl >> 6, l = rl & 63;
      const int kk = j == 0 ? km_pf[0] : j == 1 ? km_pf[1] : c_kmap[((int64_t)t * nks + ks) * 64 + l];
      slab[((int64_t)t * R + r) * Kp + kk] = acc;
    }
    for (int ks = tidx; ks < nks; ks += blockDim.x) {
      float acc = Nl[ks * NP];
      for (int pp = 1; pp < NP; ++pp) acc += Nl[ks * NP + pp];
      part_nll_c[t * nks + ks] = acc;
    }
  }
  STAMP(wg, kStampLast);
  RSTAMP(wg, 29);
}

template <int RP, typename E, int KIND, bool LOG>
__global__ void __launch_bounds__(FusedBlock<RP>::v, FusedBlock<RP>::wpe)
scfused_kernel(QSC_SCF_KPARAMS) {
  scfused_tile<RP, E, KIND, LOG>(QSC_SCF_ARGS, (int)blockIdx.x, (int)gridDim.x, threadIdx.x);
}

}  // namespace

#if QSC_DEBUG
int qsc::dbg_line_fused(bool clear) { return dbg_line_read(clear); }
#endif

extern "C" {

QSC_API int qsc_scpass(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                       const int64_t* s_off, const void* c_entries, const int32_t* c_width,
                       const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                       int32_t R, float* S,
                       const float* C, float* mS, float* vS, const qsc_adam* adam,
                       float lambda_s, qsc_state* st, void* ws, size_t ws_bytes, void* stream) {
  if (!pass_args_ok(d, m, R, ws, ws_bytes) || !qsc_scpass_supported(d, R) || !S || !C || !mS ||
      !vS || !adam || !st || !s_width || !s_off || !c_width || !c_off || !c_kmap ||
      (d->s_entries > 0 && !s_entries) || (d->c_entries > 0 && !c_entries))
    return QSC_EINVAL;
  const int RP = rp_of(R);
  const int kind = lik_kind(m);
  const bool sr = d->rowfmt == 1;
  const int NP = cpass_parts(d, R, sr);
  const size_t shm = scfused_lds(d->PT, R, d->K, d->nks, NP, sr);
  PassWs w = carve(d, R, ws);
  Edges E;
  Lik lk;
  pass_lik(d, m, &E, &lk);
  const qsc_adam ad = *adam;
  const unsigned threads = scpass_threads(d, R);
  hipStream_t s = STREAM(stream);
#define SCPASS_LAUNCH(RPV, ET, KD, LG)                                                         \
  do {                                                                                         \
      hipLaunchKernelGGL((scfused_kernel<RPV, ET, KD, LG>), dim3((unsigned)d->ntiles),         \
                         dim3(threads), shm, s, (const ET*)s_entries, s_width, s_off,         \
                         (const ET*)c_entries, c_width, c_off, c_kmap, d->nks, NP, d->PT, lk, E, \
                         d->nbins, R, d->K, S, C, mS, vS, ad, lambda_s, st, w.snll, w.snsq,    \
                         w.slab, w.cnll, w.cnsq, w.acache);                                    \
  } while (0)
  QSC_DISPATCH_PASS(SCPASS_LAUNCH);
#undef SCPASS_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

#if QSC_DIAG_STAMPS
QSC_API int qsc_diag_stamps_fused(unsigned long long* host, int n) {
  return diag_stamps_read(host, n);
}
#endif

}  // extern "C"
