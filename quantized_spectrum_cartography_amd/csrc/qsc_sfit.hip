// qsc_sfit.hip — per-pixel damped Newton / Fisher-scoring fit of the loss fields S for known
// spectra C (include/qsc.h: qsc_sfit, qsc_sfit_workspace_bytes).
//
// Conditional on C the likelihood separates over positions; position q minimises, over
// s = S[q][0..R),
//     f_q(s) = sum_{entries (k, code) of q} -log max(P(code | t = s . c_k), FLT_MIN)
//              + ridge / 2 |s|^2
// with P, the edges, the log-model chain x = log(t + offset) and the saturation rules of
// qsc_info.cuh (qsc_info.hip's header has the formulas).  Per entry, with g_x = -P'/P:
//     f += -log max(P, FLT_MIN)
//     g += g_t c_k,          g_t = g_x (linear) or g_x / (t + offset) (log model)
//     J += h c_k c_k^T,      h = entry_curvature's value: QSC_INFO_OBSERVED (Newton) or
//                            QSC_INFO_EXPECTED (Fisher scoring, J >= 0)
// A pad entry adds exactly 0 to all three; an entry with P == 0 adds 0 to g and J and
// -log FLT_MIN to f; in the log model an entry with t + offset <= 0 makes f = +inf.
//
// The walk is sinfo_kernel's: one wave per slice of QSC_SLICE positions, grid-stride over the
// slices, two lanes per position; lane half h takes entries 2h, 2h + 1 of every 4-entry chunk in
// list order; C^T and the edges sit in LDS at the info_pitch pitch; the next chunk's entries are
// loaded while this one is worked, with clamped reads.  The halves are added once with a lane
// swap (a + b is the same bits on both lanes), so from there on both lanes of a position hold
// the same state and take the same decisions.  No floating-point atomics: the order of every
// sum is fixed by the packing alone, and two calls agree bit for bit.
//
// f is evaluated in fp64 (entry_nll: t, the link and the logarithm from the fp32 s, C and edges);
// g and J stay fp32.  The accept test below compares two values of f that differ, near the
// minimiser, by g . delta ~ |g|^2 / lambda: with fp32 terms (each -log P good to ~2e-7, t = s . c
// rounded to 1e-7) a decrease below ~1e-6 is invisible, true Newton steps are rejected, and the
// iteration stops |g| ~ sqrt(1e-6 lambda) short -- 1e-3 to 1e-2 relative in S at ridge 1e-2,
// measured.  In fp64 the test resolves every step the fp32 g and J can propose.
//
// The iteration runs inside the one launch, with the same structure on every lane:
//     evaluate (f, g, J) at s = S_init[q];  mu = mu0
//     repeat up to max_steps times:
//         Cholesky of J + (ridge + mu) I (rows >= R the identity), delta from (g + ridge s)
//         s' = s - delta;  project: s' = max(s', 0)
//         a pivot that is not positive: the step counts as rejected (s' = s is walked)
//         walk: (f', g', J') at s'
//         accept iff f' <= f and f' is finite: s, (f, g, J) <- s', (f', g', J'),
//             mu <- max(mu / 10, mu0 == 0 ? 0 : kMuMin)
//         else mu <- max(10 mu, kMuMin)
//         converged once an accepted step has |s' - s|_inf <= tol (1 + |s|_inf)
// A converged position stops changing; the wave leaves the loop when every position of its slice
// has converged (ballot).  The state before a trial, (f, g, J), is kept across the trial walk:
// for RP 4 and 8 in a second register set, replaced by a per-lane select on acceptance (no
// private-memory scratch).  For RP 16 two sets of 136 + 16 values and the factor do not fit the
// 512 registers of a lane (the compiler spilled 8 to 24 bytes per lane), so there the accepted
// (g, J) live in a workspace row of the lane's own (RP + NT contiguous floats moved as 16-byte
// vectors, so that every access is the row's address plus an immediate; written on acceptance
// only, read back by the same lane for the factorisation), and the registers hold one set.
//
// Identification.  A pivot p of J + (ridge + mu) I with p <= mu says that J + ridge I itself has
// no positive pivot there (for a positive semidefinite J + ridge I every pivot of the damped
// matrix is mu plus a non-negative Schur complement).  A position whose factorisation had such a
// pivot at every step -- no observations and ridge = 0, say -- is unidentified: it is counted in
// n_unidentified, and what it returns is S_init moved by steps that only the damping defined
// (for the empty position: S_init itself, g = 0).  With mu = 0 this is the plain pivot test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "qsc_common.cuh"
#include "qsc_info.cuh"

namespace {
using namespace qsc;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// the smallest non-zero damping: what a rejected step raises mu to from 0, and the floor of the
// mu / 10 schedule when mu0 > 0
constexpr float kMuMin = 1.0e-6f;

// ranks whose accepted (g, J) are kept in the workspace instead of a second register set
__host__ __device__ constexpr bool sfit_in_ws(int RP) { return RP > 8; }

struct SfitParams {
  float ridge, mu0, tol;
  int max_steps, project;
};

template <int RP, typename E, bool SR, bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) sfit_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    int64_t n_ent, int nslices, Link lk, Edges E_, int R, int K, int P_,
    const int* __restrict__ perm, const float* __restrict__ C, const float* S_init, SfitParams pr,
    float* S_out, float* __restrict__ f_out, int* __restrict__ steps_out,
    int* __restrict__ n_unconverged, int* __restrict__ n_unidentified, float* __restrict__ ws) {
  constexpr int CP = info_pitch(RP);
  constexpr int NT = RP * (RP + 1) / 2;
  constexpr bool WS = sfit_in_ws(RP);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Cl = smem;                                             // [K][CP]
  float2* El = reinterpret_cast<float2*>(Cl + (size_t)K * CP);  // [nbins]
  for (int i = threadIdx.x; i < K * RP; i += kBlock) {
    const int k = i / RP, r = i - k * RP;
    Cl[k * CP + r] = r < R ? C[(int64_t)r * K + k] : 0.0f;
  }
  for (int b = threadIdx.x; b < lk.nbins; b += kBlock) El[b] = E_.e[b];
  __syncthreads();

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int l = lane & (QSC_SLICE - 1), h = lane >> 5;
  const int Ko = sr_off(K);
  const uint32_t pad_value = SR ? 2u * (uint32_t)Ko : (Ent<E>::kPad << Ent<E>::kBits);
  const float mu_floor = pr.mu0 == 0.0f ? 0.0f : kMuMin;
  const double inv_a = 1.0 / (double)lk.a;
  int cnt_unconv = 0, cnt_unident = 0;  // (wave-uniform)
  // WS: the lane's row (g first, then the triangle of J)
  float* wrow = ws + ((size_t)(blockIdx.x * kWaves + wave) * 64 + lane) * (RP + NT);
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    const bool live = p >= 0 && p < P_;
    // the accepted state (sc, fc, gc, Jc) and the trial point st
    float sc[RP], st[RP], gc[WS ? 1 : RP], Jc[WS ? 1 : NT];
    double fc = 0.0;
#pragma unroll
    for (int r = 0; r < RP; r += 4) {
      const float4 x = *reinterpret_cast<const float4*>(S_init + q * RP + r);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[r + e] = (live && r + e < R) ? xs[e] : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < RP; ++r) st[r] = sc[r];
    if (!WS) {
#pragma unroll
      for (int r = 0; r < RP; ++r) gc[r] = 0.0f;
#pragma unroll
      for (int i = 0; i < NT; ++i) Jc[i] = 0.0f;
    }
    float mu = pr.mu0;
    bool done = !live, ident = false, step_ok = true;
    int nwalk = 0;
    const int nch = width[s] >> 2;  // 4-entry chunks of every list of the slice
    const int64_t base = off[s] + l * 4 + 2 * h;
    for (int it = 0;; ++it) {
      // ---- walk: (ft, gt, Jt) at st ----
      double ft = 0.0;
      float gt[RP], Jt[NT];
      bool neg = false;
#pragma unroll
      for (int r = 0; r < RP; ++r) gt[r] = 0.0f;
#pragma unroll
      for (int i = 0; i < NT; ++i) Jt[i] = 0.0f;
      uint32_t n0, n1;
      load_pair<E>(ent, base, n_ent, pad_value, n0, n1);
      for (int ch = 0; ch < nch; ++ch) {
        const uint32_t v[2] = {n0, n1};
        // the next chunk's entries while this one is worked (past the last list: the next slice's
        // entries or the array's pad tail, QSC_ENTRY_TAIL; clamped in load_pair either way)
        load_pair<E>(ent, base + (int64_t)(ch + 1) * (QSC_SLICE * 4), n_ent, pad_value, n0, n1);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          int k, code;
          bool pad;
          decode<E, SR>(v[e], K, Ko, lk.nbins, k, code, pad);
          float cv[RP];
#pragma unroll
          for (int r = 0; r < RP; r += 4) {
            const float4 x = *reinterpret_cast<const float4*>(Cl + k * CP + r);
            cv[r] = x.x;
            cv[r + 1] = x.y;
            cv[r + 2] = x.z;
            cv[r + 3] = x.w;
          }
          float t = 0.0f;
#pragma unroll
          for (int r = 0; r < RP; ++r) t = __builtin_fmaf(st[r], cv[r], t);
          double td = 0.0;
#pragma unroll
          for (int r = 0; r < RP; ++r) td = __builtin_fma((double)st[r], (double)cv[r], td);
          float fe, ge, hh;
          bool use, eneg;
          entry_terms<LOGIT, LOG, KIND>(t, code, El, lk, fe, ge, hh, use, eneg);
          // the fp32 P == 0 (FLT_MIN's term) and t + offset <= 0 (f = +inf below) keep their rule
          const double fd = (fe == -logf(FLT_MIN) || eneg)
                                ? (double)fe
                                : entry_nll<LOGIT, LOG>(td, El[code], lk, inv_a);
          // a pad adds exactly 0 (c_k is finite)
          use = use && !pad;
          ft += pad ? 0.0 : fd;
          neg = neg || (eneg && !pad);
          ge = use ? ge : 0.0f;
          hh = use ? hh : 0.0f;
#pragma unroll
          for (int i = 0; i < RP; ++i) {
            gt[i] = __builtin_fmaf(ge, cv[i], gt[i]);
            const float hi_ = hh * cv[i];
#pragma unroll
            for (int j = i; j < RP; ++j)
              Jt[tri<RP>(i, j)] = __builtin_fmaf(hi_, cv[j], Jt[tri<RP>(i, j)]);
          }
        }
      }
      // the two halves' partial sums: the same bits on both lanes from here on
      ft += __shfl_xor(ft, 32, 64);
      neg = neg || (__shfl_xor((int)neg, 32, 64) != 0);
#pragma unroll
      for (int r = 0; r < RP; ++r) gt[r] += __shfl_xor(gt[r], 32, 64);
#pragma unroll
      for (int i = 0; i < NT; ++i) Jt[i] += __shfl_xor(Jt[i], 32, 64);
      double nsq = 0.0;
#pragma unroll
      for (int r = 0; r < RP; ++r) nsq = __builtin_fma((double)st[r], (double)st[r], nsq);
      ft += 0.5 * (double)pr.ridge * nsq;
      ft = neg ? (double)__builtin_inff() : ft;

      // ---- accept / reject ----
      const bool first = it == 0;
      const bool acc = first || (step_ok && ft <= fc && fabs(ft) < (double)__builtin_inff());
      float dmax = 0.0f, smax = 0.0f;
#pragma unroll
      for (int r = 0; r < RP; ++r) {
        dmax = fmaxf(dmax, fabsf(st[r] - sc[r]));
        smax = fmaxf(smax, fabsf(sc[r]));
      }
      const bool conv = !first && acc && dmax <= pr.tol * (1.0f + smax);
      if (WS && acc && (first || !done)) {
        // (the first evaluation is stored by every lane, so that no row is read unwritten)
#pragma unroll
        for (int r = 0; r < RP; r += 4)
          *reinterpret_cast<float4*>(wrow + r) = make_float4(gt[r], gt[r + 1], gt[r + 2], gt[r + 3]);
#pragma unroll
        for (int i = 0; i < NT; i += 4)
          *reinterpret_cast<float4*>(wrow + RP + i) =
              make_float4(Jt[i], Jt[i + 1], Jt[i + 2], Jt[i + 3]);
      }
      if (!done) {
        nwalk += first ? 0 : 1;
        if (acc) {
          fc = ft;
#pragma unroll
          for (int r = 0; r < RP; ++r) sc[r] = st[r];
          if (!WS) {
#pragma unroll
            for (int r = 0; r < RP; ++r) gc[r] = gt[r];
#pragma unroll
            for (int i = 0; i < NT; ++i) Jc[i] = Jt[i];
          }
          if (!first) mu = fmaxf(mu / 10.0f, mu_floor);
        } else {
          mu = fmaxf(10.0f * mu, kMuMin);
        }
        done = conv;
      }
      if (it == pr.max_steps || __ballot(!done) == 0ull) break;

      // ---- the next trial: Cholesky of Jc + (ridge + mu) I, delta from gc + ridge sc ----
      // lower triangle a[i][j], j <= i, at tri(j, i); rows >= R are the identity (Jc is 0 there)
      float a[NT];
      if (WS) {
#pragma unroll
        for (int i = 0; i < NT; i += 4) {
          const float4 x = *reinterpret_cast<const float4*>(wrow + RP + i);
          a[i] = x.x;
          a[i + 1] = x.y;
          a[i + 2] = x.z;
          a[i + 3] = x.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NT; ++i) a[i] = Jc[i];
      }
      const float lam = pr.ridge + mu;
#pragma unroll
      for (int i = 0; i < RP; ++i) a[tri<RP>(i, i)] = i < R ? a[tri<RP>(i, i)] + lam : 1.0f;
      float dinv[RP], y[RP];
      bool ok = true, idn = true;
#pragma unroll
      for (int j = 0; j < RP; ++j) {
        float piv = a[tri<RP>(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) piv = __builtin_fmaf(-a[tri<RP>(k, j)], a[tri<RP>(k, j)], piv);
        if (j < R) {
          idn = idn && (piv > mu);
          if (!(piv > 0.0f)) {  // (also a NaN block)
            ok = false;
            piv = 1.0f;
          }
        }
        const float d = sqrtf(piv);
        dinv[j] = 1.0f / d;
#pragma unroll
        for (int i = j + 1; i < RP; ++i) {
          float v = a[tri<RP>(j, i)];
#pragma unroll
          for (int k = 0; k < j; ++k) v = __builtin_fmaf(-a[tri<RP>(k, i)], a[tri<RP>(k, j)], v);
          a[tri<RP>(j, i)] = v * dinv[j];
        }
      }
      // L y = g + ridge s, then L^T delta = y (delta in y)
#pragma unroll
      for (int i = 0; i < RP; ++i) {
        float v = __builtin_fmaf(pr.ridge, sc[i], WS ? wrow[i] : gc[i]);
#pragma unroll
        for (int k = 0; k < i; ++k) v = __builtin_fmaf(-a[tri<RP>(k, i)], y[k], v);
        y[i] = v * dinv[i];
      }
#pragma unroll
      for (int i = RP - 1; i >= 0; --i) {
        float v = y[i];
#pragma unroll
        for (int k = i + 1; k < RP; ++k) v = __builtin_fmaf(-a[tri<RP>(i, k)], y[k], v);
        y[i] = v * dinv[i];
      }
      const bool move = ok && !done;
      if (!done) ident = ident || (ok && idn);
      step_ok = ok;
#pragma unroll
      for (int r = 0; r < RP; ++r) {
        float v = sc[r] - y[r];
        v = pr.project ? fmaxf(v, 0.0f) : v;
        st[r] = (move && r < R) ? v : sc[r];
      }
    }
    // ---- results (half 0 writes the position's row) ----
    if (h == 0) {
#pragma unroll
      for (int r = 0; r < RP; r += 4)
        *reinterpret_cast<float4*>(S_out + q * RP + r) =
            make_float4(sc[r], sc[r + 1], sc[r + 2], sc[r + 3]);
      if (f_out != nullptr) f_out[q] = live ? (float)fc : 0.0f;
      if (steps_out != nullptr) steps_out[q] = nwalk;
    }
    cnt_unconv += __popcll(__ballot(h == 0 && live && !done));
    cnt_unident += __popcll(__ballot(h == 0 && live && !ident));
  }
  // one integer atomic per wave and counter (integer addition: any order gives the same count)
  if (lane == 0) {
    if (cnt_unconv != 0) atomicAdd(n_unconverged, cnt_unconv);
    if (cnt_unident != 0) atomicAdd(n_unidentified, cnt_unident);
  }
}

int cu_count_sfit() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
    return 256;
  return n;
}

// the grid of a call: a grid-stride walk over the slices (any grid gives the same bits), as
// qsc_sinfo; with the workspace (one row per lane of the grid) only twice the workgroups that
// are resident at the one wave per SIMD the RP 16 kernels run at
int64_t sfit_grid(int nslices, int RP) {
  const int64_t want = ceil_div(nslices, kWaves);
  return std::min<int64_t>(want, (int64_t)cu_count_sfit() * (sfit_in_ws(RP) ? 2 : 8));
}

}  // namespace

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

QSC_API size_t qsc_sfit_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  if (!d || R < 1 || R > QSC_MAX_R || d->Pp < 1) return 0;
  const int RP = qsc_rank_pad(R);
  if (!sfit_in_ws(RP)) return 0;  // (the state before a trial step stays in registers)
  return (size_t)sfit_grid(d->Pp / QSC_SLICE, RP) * kWaves * 64 * (RP + RP * (RP + 1) / 2) *
         sizeof(float);
}

QSC_API int qsc_sfit(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                     const int64_t* s_off, const int32_t* perm, const qsc_model* m, int32_t R,
                     const float* C, const float* S_init, int32_t kind, float ridge, float mu0,
                     float tol, int32_t max_steps, int32_t project, float* S_out, float* f_out,
                     int32_t* steps, int32_t* n_unconverged, int32_t* n_unidentified, void* ws,
                     size_t ws_bytes, void* stream) {
  if (!d || !s_width || !s_off || !perm || !C || !S_init || !S_out || !n_unconverged ||
      !n_unidentified || !info_model_ok(m))
    return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  if (!(ridge >= 0.0f) || !(mu0 >= 0.0f) || !(tol > 0.0f) || max_steps < 1) return QSC_EINVAL;
  if (!info_layout_ok(d, m, R) || (d->s_entries > 0 && !s_entries)) return QSC_EINVAL;
  const size_t need = qsc_sfit_workspace_bytes(d, R);
  if (need > 0 && (!ws || ws_bytes < need)) return QSC_EINVAL;
  const int RP = qsc_rank_pad(R);
  const size_t shm = sinfo_lds(d->K, RP, d->nbins);
  if (shm > kInfoLdsMax) return QSC_EUNSUPPORTED;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const int nslices = d->Pp / QSC_SLICE;
  const SfitParams pr = {ridge, mu0, tol, max_steps, project != 0};
  const dim3 grid((unsigned)sfit_grid(nslices, RP)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  const bool sr = d->rowfmt == 1;
#define SFIT_LAUNCH_E(RPV, ET, SRV, LGT, LOGV, KD)                                              \
  hipLaunchKernelGGL((sfit_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, shm, hs,            \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, nslices, lk, E, \
                     R, d->K, d->P, perm, C, S_init, pr, S_out, f_out, steps, n_unconverged,    \
                     n_unidentified, (float*)ws)
#define SFIT_LAUNCH_RP(RPV, LGT, LOGV, KD)                                  \
  do {                                                                      \
    if (sr) {                                                               \
      /* (signed rows: linear one-bit only) */                              \
      if (!LOGV) SFIT_LAUNCH_E(RPV, uint16_t, true, LGT, false, KD);        \
    } else if (d->wide) SFIT_LAUNCH_E(RPV, uint32_t, false, LGT, LOGV, KD); \
    else SFIT_LAUNCH_E(RPV, uint16_t, false, LGT, LOGV, KD);                \
  } while (0)
#define SFIT_LAUNCH(LGT, LOGV, KD)                      \
  do {                                                  \
    if (RP == 4) SFIT_LAUNCH_RP(4, LGT, LOGV, KD);      \
    else if (RP == 8) SFIT_LAUNCH_RP(8, LGT, LOGV, KD); \
    else SFIT_LAUNCH_RP(16, LGT, LOGV, KD);             \
  } while (0)
  QSC_INFO_DISPATCH(SFIT_LAUNCH);
#undef SFIT_LAUNCH
#undef SFIT_LAUNCH_RP
#undef SFIT_LAUNCH_E
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
