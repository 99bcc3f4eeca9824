// qsc_pass_finish.hip — what runs between the fused passes (qsc_pass.cuh): the C finish and
// update, the S updates from reduced gradients, the state book-keeping and the small utility
// kernels, with their entry points and the pure host queries about a layout.  Built with the
// passes' flags (f32 denormals flushed), as these kernels always were.
#define QSC_PASS_NO_STAMPS  // no kernel here takes timestamps: no 1 MB table of its own
#include "qsc_pass_host.cuh"

namespace {

// ---------------------------------------------------------------------------------------
// The fixed order of the scalar partials -- the S-passes' per-slice NLL and ||S||^2
// (part_nll_s, part_nsq_s) and the C-passes' per-(tile, k-slice) NLL (part_nll_c) -- which every
// form settles (cfinish's book-keeping block, state_flush: both 1024-thread blocks), so that the
// solver forms agree bit for bit: canonical thread i of kCanon = 1024 sums items i, i + 1024,
// i + 2048, ... in order; then each canonical wave's xor butterfly (wave_sum) and the 16 wave sums
// in wave order; every sum from +0.  A workgroup of 1024 / VF threads stands for the canonical one:
// its thread t is the canonical threads t + f blockDim (f < VF), lane for lane.
//
// The totals are summed whether or not the state says they are pending, and so are never behind
// a load of the state: the loads of a batch (8 items per canonical thread of each array) are all
// issued before the first sum, beside the caller's read of the state words (state_in) -- one
// memory round trip at C3's 8192 slices.  Thread 0 then keeps the totals that were pending
// (settle_store); the workspace arrays always exist (carve), so the loads are in bounds.
// ---------------------------------------------------------------------------------------
constexpr int kCanon = 1024;
struct Canon {
  float nll_s, nsq_s, nll_c;
};

// The totals over nslices S-pass items and (WITH_C) nc C-pass items; sh: LDS [3][16] floats.
// Result valid in thread 0.
template <int VF, bool WITH_C>
__device__ __forceinline__ Canon canon_totals(const float* __restrict__ nll_s,
                                              const float* __restrict__ nsq_s,
                                              const float* __restrict__ nll_c, int nslices, int nc,
                                              float* sh) {
  constexpr int NB = kCanon / VF, NW = kCanon / 64;
  const int tid = threadIdx.x;
  float a[VF], b[VF], c[VF];
#pragma unroll
  for (int f = 0; f < VF; ++f) a[f] = b[f] = c[f] = 0.0f;
  const int n = WITH_C ? max(nslices, nc) : nslices;
  for (int i0 = 0; i0 < n; i0 += 8 * kCanon) {
    float va[VF][8], vb[VF][8], vc[VF][8];
#pragma unroll
    for (int f = 0; f < VF; ++f)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + tid + f * NB + j * kCanon;
        va[f][j] = nll_s[min(i, nslices - 1)];
        vb[f][j] = nsq_s[min(i, nslices - 1)];
        vc[f][j] = WITH_C ? nll_c[min(i, nc - 1)] : 0.0f;
      }
#pragma unroll
    for (int f = 0; f < VF; ++f)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + tid + f * NB + j * kCanon;
        if (i < nslices) {
          a[f] += va[f][j];
          b[f] += vb[f][j];
        }
        if (WITH_C && i < nc) c[f] += vc[f][j];
      }
  }
#pragma unroll
  for (int f = 0; f < VF; ++f) {
    const float wa = wave_sum(a[f]), wb = wave_sum(b[f]), wc = wave_sum(c[f]);
    const int w = (tid >> 6) + f * (NB / 64);  // the canonical wave
    if ((tid & 63) == 0) {
      sh[w] = wa;
      sh[NW + w] = wb;
      sh[2 * NW + w] = wc;
    }
  }
  __syncthreads();
  Canon r{0.0f, 0.0f, 0.0f};
  if (tid == 0)
    for (int w = 0; w < NW; ++w) {
      r.nll_s += sh[w];
      r.nsq_s += sh[NW + w];
      r.nll_c += sh[2 * NW + w];
    }
  return r;
}

// the state words the book-keeping needs, read together ahead of the totals (no load waits for
// another's value)
struct StateIn {
  int step_c, step_s, iter, pending;
  float normsq_s, normsq_c, nll_c, normsq_s_prev;
};
__device__ __forceinline__ StateIn state_in(const qsc_state* __restrict__ st) {
  return StateIn{st->step_c,   st->step_s,   st->iter,  st->pending,
                 st->normsq_s, st->normsq_c, st->nll_c, st->normsq_s_prev};
}

// book-keeping shared by cfinish and state_flush (thread 0): settle a pending S-pass from the
// totals -- totals that are not pending are dropped -- and return the flags left pending (the
// caller stores them); s.normsq_s follows the state
__device__ __forceinline__ int settle_store(qsc_state* __restrict__ st, StateIn& s, const Canon& c,
                                            float* __restrict__ hist, int hist_cap) {
  const int pend = s.pending;
  if (!(pend & (QSC_PEND_SNLL | QSC_PEND_SUPD))) return pend;
  const int it = s.iter - 1;
  st->nll_s = c.nll_s;
  if (hist && it >= 0 && it < hist_cap) {
    hist[4 * it + 0] = s.nll_c;
    hist[4 * it + 1] = c.nll_s;
    hist[4 * it + 2] = s.normsq_c;
    hist[4 * it + 3] = s.normsq_s_prev;
  }
  if (pend & QSC_PEND_SUPD) {
    s.normsq_s = c.nsq_s;
    st->normsq_s = c.nsq_s;
    st->step_s = s.step_s + 1;
  }
  return pend & ~(QSC_PEND_SNLL | QSC_PEND_SUPD);
}

// ---------------------------------------------------------------------------------------
// C finish: fixed-order slab reduction (+ fused regulariser / Adam / projection)
// ---------------------------------------------------------------------------------------
#define QSC_CF_PARAMS                                                                          \
  const float *__restrict__ slab, int ntiles, int nks, int R, int K, float *C, int mode,         \
      float *__restrict__ dC, float *__restrict__ mC, float *__restrict__ vC, qsc_adam ad,       \
      float lambda_c, const float *__restrict__ normsq_ext, const float *__restrict__ cnsq,      \
      qsc_state *__restrict__ st, const float *__restrict__ part_nll_c, int npart_c,             \
      const float *__restrict__ part_nll_s, const float *__restrict__ part_nsq_s, int nslices,   \
      float *__restrict__ hist, int hist_cap, AdamCache *__restrict__ acache
#define QSC_CF_ARGS                                                                           \
  slab, ntiles, nks, R, K, C, mode, dC, mC, vC, ad, lambda_c, normsq_ext, cnsq, st, part_nll_c,  \
      npart_c, part_nll_s, part_nsq_s, nslices, hist, hist_cap, acache
// Bins per column block.  A column's gradient is the sum of kFParts = 16 partials in partial
// order, partial w the sum of tiles w, w + 16, ... in order (the canonical tile groups), every sum
// from +0.  A block of 16 * kFGroup threads takes kFGroup bins of one r: thread t holds bin
// t % kFGroup of partial t / kFGroup with sixteen independent loads in flight.  64: one wave per
// partial, 256-byte rows, C3's 2 MB slab pulled by 32 workgroups of 1024 threads.  Spreading it
// over more CUs lost at C3 -- 32-bin groups (64 workgroups of 512) +1.0 %, 16-bin groups (128 of
// 256, 64-byte rows) -1.1 % against 64's +2.3 % over the parent's headline
// (profiles/cfinish/bench_headline_parent_vs_this.txt); the orders are the same at every size
// (tests/test_gpu_cfinish_order.py passes at 16, 32 and 64).
#ifndef QSC_CFIN_GROUP
#define QSC_CFIN_GROUP 64
#endif
constexpr int kFGroup = QSC_CFIN_GROUP, kFParts = 16;
constexpr int kFinBlock = kFParts * kFGroup;
static_assert(kFGroup == 16 || kFGroup == 32 || kFGroup == 64, "a 64-bin slice in whole groups");

// Workgroup vb of R * Kp / kFGroup + 2: a column block per (r, kFGroup bins); then the
// book-keeping block (canon_totals, settle_store) and the block of the next C-step's Adam
// scalars.  Every block makes one round of loads: none waits for another load's value.
__global__ void __launch_bounds__(kFinBlock) cfinish_kernel(QSC_CF_PARAMS) {
  __shared__ float red[kFParts][kFGroup];
  __shared__ Scalars sc;
  __shared__ float sh[3 * (kCanon / 64)];
  const int Kp = nks * 64, ngk = Kp / kFGroup, ncol = R * ngk;
  const int vb = (int)blockIdx.x, tid = (int)threadIdx.x;

  // ||C||^2 of the C this step differentiates: written by the C-pass (C is read-only there),
  // or the caller's global value (K-slab); never re-read here, where blocks overwrite C
  const float nsq = normsq_ext ? *normsq_ext : *cnsq;

  if (vb == ncol + 1) {
    // the next C-step's Adam scalars (the next S-pass settles step_c + 1 in between)
    if (mode == 1 && tid == 0) adam_cache_store(acache, ad, st->step_c + 2);
    return;
  }
  if (vb == ncol) {
    // book-keeping block: settle the S-pass partials and total the C-pass NLL, in the canonical
    // order
    StateIn s = state_in(st);
    const Canon cs = canon_totals<kCanon / kFinBlock, true>(part_nll_s, part_nsq_s, part_nll_c,
                                                            nslices, npart_c, sh);
    if (tid == 0) {
      int pnd = settle_store(st, s, cs, hist, hist_cap);
      st->nll_c = cs.nll_c;
      if (mode == 1) {
        st->normsq_c = nsq;
        pnd |= QSC_PEND_C;
      }
      if (pnd != s.pending) st->pending = pnd;
      if (mode == 2) dC[(int64_t)R * K] = s.normsq_s;  // this shard's ||S||^2 (IJ-slab)
    }
    return;
  }

  const int r = vb / ngk, k0 = (vb - r * ngk) * kFGroup;
  if (k0 >= K) return;  // padding bins only
  const int w = tid / kFGroup, b = tid % kFGroup, k = k0 + b;
  const int64_t i = (int64_t)r * K + k;
  // the update's inputs ride in the round of the tile loads
  float p0 = 0.0f, m0 = 0.0f, v0 = 0.0f;
  if (mode == 1 && w == 0 && k < K) {
    p0 = C[i];
    m0 = mC[i];
    v0 = vC[i];
  }
  if (tid == 0 && mode == 1) {
    const AdamCache a0 = acache[0], a1 = acache[1];  // both slots: no dependent read on step_c
    const int step = st->step_c + 1;
    const float nrm = sqrtf(nsq);
    sc.coef = nrm > 0.0f ? lambda_c / nrm : 0.0f;
    sc.as = adam_scalars_cached((step & 1) ? a1 : a0, ad, step);
  }
  // tile sum of partial w.  Thirty-two loads in flight per lane made the 1024-thread form slower,
  // 3.26 -> 4.6 us at C3 (profiles/r04/fin_small_wg/ab_c3_grouped_tickets.log)
  const float* col = slab + (int64_t)r * Kp + k;
  const int64_t tstride = (int64_t)R * Kp;
  float a = 0.0f;
  for (int tg = 0; tg < ntiles; tg += 16 * kFParts) {
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      v[j] = col[(int64_t)min(tg + w + j * kFParts, ntiles - 1) * tstride];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (tg + w + j * kFParts < ntiles) a += v[j];
  }
  red[w][b] = a;
  __syncthreads();
  if (w == 0 && k < K) {
    float g = red[0][b];
#pragma unroll
    for (int q = 1; q < kFParts; ++q) g += red[q][b];
    if (mode == 1) {
      float p = p0, m = m0, v = v0;
      g = __fadd_rn(g, __fmul_rn(p, sc.coef));
      adam_elem(p, m, v, g, ad, sc.as);
      C[i] = p;
      mC[i] = m;
      vC[i] = v;
    } else {
      dC[i] = g;  // modes 0 and 2
    }
  }
}

// ---------------------------------------------------------------------------------------
// C update from an externally reduced gradient g [R][K] (IJ-slab sharding, after the RCCL
// all-reduce of the per-shard dC): g + lambda_c C/||C||, Adam, C >= 0; the same state
// protocol as qsc_cfinish mode 1.  normsq_s_ext (nullable): the all-reduced ||S||^2, stored as
// the S-pass's regulariser norm.
__global__ void __launch_bounds__(kFBlock) cupdate_kernel(
    int R, int K, float* __restrict__ C, float* __restrict__ mC, float* __restrict__ vC,
    const float* __restrict__ g, qsc_adam ad, float lambda_c,
    const float* __restrict__ normsq_s_ext, qsc_state* __restrict__ st) {
  constexpr int NW = kFBlock / 64;
  __shared__ float shn[NW];
  __shared__ Scalars sc;
  const int n = R * K;
  const float nsq = cnorm_sq(C, n, shn);
  if (threadIdx.x == 0) {
    const float nrm = sqrtf(nsq);
    sc.coef = nrm > 0.0f ? lambda_c / nrm : 0.0f;
    sc.as = adam_scalars(ad, st->step_c + 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float p = C[i], m = mC[i], v = vC[i];
    const float gg = __fadd_rn(g[i], __fmul_rn(p, sc.coef));
    adam_elem(p, m, v, gg, ad, sc.as);
    C[i] = p;
    mC[i] = m;
    vC[i] = v;
  }
  if (threadIdx.x == 0) {
    st->normsq_c = nsq;
    st->pending |= QSC_PEND_C;
    if (normsq_s_ext) st->normsq_s = *normsq_s_ext;
  }
}

__global__ void __launch_bounds__(1024) flush_kernel(qsc_state* __restrict__ st,
                                                     const float* __restrict__ part_nll_s,
                                                     const float* __restrict__ part_nsq_s,
                                                     int ntiles, int nslices,
                                                     float* __restrict__ hist, int hist_cap) {
  __shared__ float sh[3 * (kCanon / 64)];
  StateIn s = state_in(st);
  const Canon cs =
      canon_totals<1, false>(part_nll_s, part_nsq_s, nullptr, nslices, 0, sh);
  if (threadIdx.x == 0) {
    int pnd = settle_store(st, s, cs, hist, hist_cap);
    if (pnd & QSC_PEND_C) {
      st->step_c = s.step_c + 1;
      pnd &= ~QSC_PEND_C;
    }
    if (pnd != s.pending) st->pending = pnd;
  }
}

// S update from an all-reduced gradient (K-slab): the S-pass's lane mapping (32 positions per
// wave, lane half h owns the row elements [h*RP/2, (h+1)*RP/2)) and its Adam
template <int RP>
__global__ void __launch_bounds__(kSBlock) supdate_kernel(
    int nslices, float* __restrict__ S, float* __restrict__ mS, float* __restrict__ vS,
    const float* __restrict__ gsrc, qsc_adam ad, float lambda_s, qsc_state* __restrict__ st,
    float* __restrict__ part_nsq) {
  constexpr int RH = RP / 2;
  __shared__ Scalars sc;
  if (threadIdx.x == 0) {
    const float nrm = sqrtf(st->normsq_s);
    sc.coef = nrm > 0.0f ? lambda_s / nrm : 0.0f;
    sc.as = adam_scalars(ad, st->step_s + 1);
    if (blockIdx.x == 0) st->pending |= QSC_PEND_SUPD;  // normsq_s / step_s settled later
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * kSWaves + wave;
  if (s >= nslices) return;
  const int64_t o = ((int64_t)s * QSC_SLICE + (lane & (QSC_SLICE - 1))) * RP + (lane >> 5) * RH;
  float p[RH], m[RH], v[RH], g[RH];
  ld_row<RH>(S + o, p);
  ld_row<RH>(mS + o, m);
  ld_row<RH>(vS + o, v);
  ld_row<RH>(gsrc + o, g);
  // the fused S-pass's update (no projection)
  float nsq = adam_row_fast<RH>(p, m, v, g, sc.coef, sc.as, ad.project_nonneg != 0);
  st_row<RH>(S + o, p);
  st_row<RH>(mS + o, m);
  st_row<RH>(vS + o, v);
  nsq = wave_sum(nsq);
  if (lane == 0) part_nsq[s] = nsq;
}

// K-slab S update on this rank's shard of slices [s0, s0 + gridDim slices) with the shard's
// reduce-scattered gradient g_own (rows of slice s0 first): the same lane mapping, Adam and
// per-slice ||S_new||^2 partial as supdate_kernel, for the owned rows only
template <int RP>
__global__ void __launch_bounds__(kSBlock) supdate_slices_kernel(
    int s0, int s1, float* __restrict__ S, float* __restrict__ mS, float* __restrict__ vS,
    const float* __restrict__ g_own, qsc_adam ad, float lambda_s, qsc_state* __restrict__ st,
    float* __restrict__ part_nsq) {
  constexpr int RH = RP / 2;
  __shared__ Scalars sc;
  if (threadIdx.x == 0) {
    const float nrm = sqrtf(st->normsq_s);
    sc.coef = nrm > 0.0f ? lambda_s / nrm : 0.0f;
    sc.as = adam_scalars(ad, st->step_s + 1);
    if (blockIdx.x == 0) st->pending |= QSC_PEND_SUPD;  // normsq_s / step_s settled later
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = s0 + blockIdx.x * kSWaves + wave;
  if (s >= s1) return;
  const int64_t lo = ((int64_t)(lane & (QSC_SLICE - 1))) * RP + (lane >> 5) * RH;
  const int64_t o = (int64_t)s * QSC_SLICE * RP + lo;
  const int64_t og = (int64_t)(s - s0) * QSC_SLICE * RP + lo;
  float p[RH], m[RH], v[RH], g[RH];
  ld_row<RH>(S + o, p);
  ld_row<RH>(mS + o, m);
  ld_row<RH>(vS + o, v);
  ld_row<RH>(g_own + og, g);
  float nsq = adam_row_fast<RH>(p, m, v, g, sc.coef, sc.as, ad.project_nonneg != 0);
  st_row<RH>(S + o, p);
  st_row<RH>(mS + o, m);
  st_row<RH>(vS + o, v);
  nsq = wave_sum(nsq);
  if (lane == 0) part_nsq[s] = nsq;
}

// Per-slice ||S||^2 partials of a replicated S, bit-identical to the ones supdate_kernel /
// supdate_slices_kernel compute from the same rows (same lane mapping, the same fma chain over
// the lane's half row, the same wave sum): after the K-slab all-gather every rank holds every
// slice's partial without exchanging them
template <int RP>
__global__ void __launch_bounds__(kSBlock) slice_nsq_kernel(int nslices,
                                                            const float* __restrict__ S,
                                                            float* __restrict__ part_nsq) {
  constexpr int RH = RP / 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * kSWaves + wave;
  if (s >= nslices) return;
  const int64_t o = ((int64_t)s * QSC_SLICE + (lane & (QSC_SLICE - 1))) * RP + (lane >> 5) * RH;
  float p[RH];
  ld_row<RH>(S + o, p);
  float nsq = 0.0f;
#pragma unroll
  for (int j = 0; j < RH; ++j) nsq = __builtin_fmaf(p[j], p[j], nsq);
  nsq = wave_sum(nsq);
  if (lane == 0) part_nsq[s] = nsq;
}

__global__ void state_init_kernel(qsc_state* st, const double* nsq_part, int nparts) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += nsq_part[i];
    qsc_state z{};
    z.normsq_s = (float)s;
    z.normsq_s_prev = (float)s;
    *st = z;
  }
}

__global__ void __launch_bounds__(kSBlock) nsq_part_kernel(const float* __restrict__ x, int64_t n,
                                                           double* __restrict__ part) {
  __shared__ double sh[kSWaves];
  double s = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    s += v * v;
  }
  const double r = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ void __launch_bounds__(1024) sumsq_small_kernel(const float* __restrict__ x, int n,
                                                           float* __restrict__ out) {
  __shared__ float sh[16];
  const float r = cnorm_sq(x, n, sh);  // the C-pass's order
  if (threadIdx.x == 0) *out = r;
}

// Adam on a flat parameter buffer (the generator / DIP solver's decoder weights or latent Z,
// torch.optim.Adam's update bit for bit: adam_elem) at step = the state's S-pass counter, so one
// captured hipGraph replays every iteration's step (qsc_adam_flat)
__global__ void __launch_bounds__(256) adam_flat_kernel(float* __restrict__ p,
                                                        float* __restrict__ m,
                                                        float* __restrict__ v,
                                                        const float* __restrict__ g, int64_t n,
                                                        qsc_adam ad,
                                                        const qsc_state* __restrict__ st) {
  __shared__ AdamScalars sc;
  if (threadIdx.x == 0) sc = adam_scalars(ad, st->iter);
  __syncthreads();
  const AdamScalars s = sc;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_elem(pp, mm, vv, g[i], ad, s);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

__global__ void selftest_erf_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = erff(x[i]);
  out[n + i] = erf_fast(x[i]);
}

}  // namespace

extern "C" {

QSC_API size_t qsc_pass_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R) return 0;
  return ws_bytes_for(d, R);
}

QSC_API int qsc_state_init(qsc_state* st, const float* S, int32_t R, int32_t Pp, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!st || R < 1 || R > QSC_MAX_R || Pp < 1 || !ws || ws_bytes < 256 * sizeof(double))
    return QSC_EINVAL;
  double* part = (double*)ws;
  const int nb = 256;
  if (S) {
    hipLaunchKernelGGL(nsq_part_kernel, dim3(nb), dim3(kSBlock), 0, STREAM(stream), S,
                       (int64_t)rp_of(R) * Pp, part);  // [Pp][RP], padding rows are zero
    QSC_CHECK_LAUNCH();
  } else {
    QSC_TRY(hipMemsetAsync(part, 0, nb * sizeof(double), STREAM(stream)));
  }
  hipLaunchKernelGGL(state_init_kernel, dim3(1), dim3(64), 0, STREAM(stream), st, part, nb);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int64_t qsc_pass_cnsq_offset(const qsc_obs_desc* d, int32_t R) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R) return -1;
  const uintptr_t base = 4096;  // any aligned address: the carve is base-relative
  return (int64_t)(reinterpret_cast<uintptr_t>(carve(d, R, reinterpret_cast<void*>(base)).cnsq) -
                   base);
}

QSC_API int64_t qsc_pass_part_offset(const qsc_obs_desc* d, int32_t R, int32_t which) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R || which < 0 || which > 3) return -1;
  const uintptr_t base = 4096;
  const PassWs w = carve(d, R, reinterpret_cast<void*>(base));
  const float* part[4] = {w.slab, w.cnll, w.snll, w.snsq};
  return (int64_t)(reinterpret_cast<uintptr_t>(part[which]) - base);
}

QSC_API int qsc_obs_signed_rows_ok(const qsc_obs_desc* d, int32_t R, const qsc_model* m) {
  if (!desc_ok(d) || !m || R < 1 || R > QSC_MAX_R || m->nbounds - 1 != d->nbins) return 0;
  return (is_onebit_cf(lik_kind(m)) && sr_layout_ok(d, R)) ? 1 : 0;
}

QSC_API int qsc_scpass_supported(const qsc_obs_desc* d, int32_t R) {
  if (!desc_ok(d) || R < 1 || R > 16) return 0;
  return scpass_fits(d, R, d->rowfmt == 1) ? 1 : 0;
}

QSC_API int qsc_cfinish(const qsc_obs_desc* d, int32_t R, float* C, int32_t mode, float* dC,
                        float* mC, float* vC, const qsc_adam* adam, float lambda_c,
                        const float* normsq_c_ext, qsc_state* st, float* hist,
                        int32_t hist_cap, void* ws, size_t ws_bytes, void* stream) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R || !C || !st || !ws || ws_bytes < ws_bytes_for(d, R))
    return QSC_EINVAL;
  if ((mode == 0 || mode == 2) && !dC) return QSC_EINVAL;
  if (mode == 1 && (!mC || !vC || !adam)) return QSC_EINVAL;
  if (mode < 0 || mode > 2) return QSC_EINVAL;
  PassWs w = carve(d, R, ws);
  qsc_adam ad{};
  if (adam) ad = *adam;
  hipLaunchKernelGGL(cfinish_kernel, dim3((unsigned)(R * d->nks * (64 / kFGroup) + 2)),
                     dim3(kFinBlock), 0, STREAM(stream), w.slab, d->ntiles, d->nks, R, d->K, C, mode, dC, mC, vC, ad,
                     lambda_c, normsq_c_ext, w.cnsq, st, w.cnll, d->ntiles * d->nks, w.snll,
                     w.snsq, d->Pp / QSC_SLICE, hist, hist_cap, w.acache + 2);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_cupdate(int32_t R, int32_t K, float* C, float* mC, float* vC, const float* g,
                        const qsc_adam* adam, float lambda_c, const float* normsq_s_ext,
                        qsc_state* st, void* stream) {
  if (R < 1 || R > QSC_MAX_R || K < 1 || !C || !mC || !vC || !g || !adam || !st)
    return QSC_EINVAL;
  hipLaunchKernelGGL(cupdate_kernel, dim3(1), dim3(kFBlock), 0, STREAM(stream), R, K, C, mC, vC,
                     g, *adam, lambda_c, normsq_s_ext, st);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_state_flush(const qsc_obs_desc* d, int32_t R, qsc_state* st, float* hist,
                            int32_t hist_cap, void* ws, size_t ws_bytes, void* stream) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R || !st || !ws || ws_bytes < ws_bytes_for(d, R))
    return QSC_EINVAL;
  PassWs w = carve(d, R, ws);
  hipLaunchKernelGGL(flush_kernel, dim3(1), dim3(1024), 0, STREAM(stream), st, w.snll, w.snsq,
                     d->ntiles, d->Pp / QSC_SLICE, hist, hist_cap);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_supdate(const qsc_obs_desc* d, int32_t R, float* S, float* mS, float* vS,
                        const float* g, const qsc_adam* adam, float lambda_s, qsc_state* st,
                        void* ws, size_t ws_bytes, void* stream) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R || !S || !mS || !vS || !g || !adam || !st || !ws ||
      ws_bytes < ws_bytes_for(d, R))
    return QSC_EINVAL;
  PassWs w = carve(d, R, ws);
  const int nslices = d->Pp / QSC_SLICE;
  const dim3 grid((unsigned)ceil_div(nslices, kSWaves)), blk(kSBlock);
  QSC_LAUNCH_RP(supdate_kernel, rp_of(R), grid, blk, 0, STREAM(stream), nslices, S, mS, vS, g,
                *adam, lambda_s, st, w.snsq);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_supdate_slices(const qsc_obs_desc* d, int32_t R, int32_t s0, int32_t s1,
                               float* S, float* mS, float* vS, const float* g_own,
                               const qsc_adam* adam, float lambda_s, qsc_state* st, void* ws,
                               size_t ws_bytes, void* stream) {
  const int nslices = d ? d->Pp / QSC_SLICE : 0;
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R || !S || !mS || !vS || !g_own || !adam || !st ||
      !ws || ws_bytes < ws_bytes_for(d, R) || s0 < 0 || s1 < s0 || s1 > nslices)
    return QSC_EINVAL;
  PassWs w = carve(d, R, ws);
  const int n = s1 - s0;
  const dim3 grid((unsigned)std::max<int64_t>(1, ceil_div(n, kSWaves))), blk(kSBlock);
  // (an empty shard still launches one block: it raises the pending S-update flag like the rest)
  QSC_LAUNCH_RP(supdate_slices_kernel, rp_of(R), grid, blk, 0, STREAM(stream), s0, s1, S, mS, vS,
                g_own, *adam, lambda_s, st, w.snsq);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_slice_nsq(const qsc_obs_desc* d, int32_t R, const float* S, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!desc_ok(d) || R < 1 || R > QSC_MAX_R || !S || !ws || ws_bytes < ws_bytes_for(d, R))
    return QSC_EINVAL;
  PassWs w = carve(d, R, ws);
  const int nslices = d->Pp / QSC_SLICE;
  const dim3 grid((unsigned)ceil_div(nslices, kSWaves)), blk(kSBlock);
  QSC_LAUNCH_RP(slice_nsq_kernel, rp_of(R), grid, blk, 0, STREAM(stream), nslices, S, w.snsq);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_adam_flat(float* p, float* m, float* v, const float* g, int64_t n,
                          const qsc_adam* adam, const qsc_state* st, void* stream) {
  if (n < 0 || !adam || !st || (n > 0 && (!p || !m || !v || !g))) return QSC_EINVAL;
  if (n == 0) return QSC_OK;
  const int64_t blocks = std::min<int64_t>(ceil_div(n, 256), (int64_t)cu_count() * 8);
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, STREAM(stream), p,
                     m, v, g, n, *adam, st);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_sumsq_small(const float* x, int32_t n, float* out, void* stream) {
  if (n < 0 || !x || !out) return QSC_EINVAL;
  hipLaunchKernelGGL(sumsq_small_kernel, dim3(1), dim3(1024), 0, STREAM(stream), x, n, out);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_debug_status(int32_t clear) {
#if QSC_DEBUG
  // every kernel file's flag is read (and cleared); the first one set is reported as
  // file id * 100000 + line (include/qsc.h)
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  const int line[3] = {dbg_line_s(clear != 0), dbg_line_c(clear != 0), dbg_line_fused(clear != 0)};
  for (int f = 0; f < 3; ++f)
    if (line[f] < 0) return -2;
  for (int f = 0; f < 3; ++f)
    if (line[f] > 0) return (f + 1) * 100000 + line[f];
  return 0;
#else
  (void)clear;
  return -1;
#endif
}

QSC_API int qsc_selftest_erf(const float* x, int32_t n, float* out, void* stream) {
  if (n < 0 || !x || !out) return QSC_EINVAL;
  if (n == 0) return QSC_OK;
  hipLaunchKernelGGL(selftest_erf_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                     STREAM(stream), x, n, out);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
