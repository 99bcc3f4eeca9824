// qsc_sfit_smooth.hip — one red-black visit of the damped Newton fit of the loss fields S under
// the smoothness prior (include/qsc.h: qsc_sfit_smooth, qsc_sfit_smooth_workspace_bytes).
//
// The prior weight * R(S) of qsc_smooth.hip lives on the 4-neighbour grid, which is bipartite in
// the colour (i + j) & 1 of pixel (i, j).  With the rows of the other colour held fixed, an
// own-colour position q minimises, over s = S[q][0..R),
//     phi_q(s) = f_q(s) + weight * sum_{n in N(q)} sum_{r<R} rho(s_r - S[n][r])
// with f_q qsc_sfit's objective (ridge included), N(q) the 2..4 grid neighbours of nbr[q] (all of
// the other colour) and rho qsc_smooth_grad's QUAD or HUBER function.  One launch visits one
// colour in place; it reads neighbour rows only of the other colour and writes rows only of its
// own, so no row that is read as a neighbour is written in the same launch: no race, no second
// buffer, no dependence on grid or wave order.
//
// Per own-colour position the walk is sfit_kernel's (qsc_sfit.hip: one wave per slice, two lanes
// per position, C^T and the edges in LDS, early clamped loads, fp64 f, fp32 g and J); it is
// duplicated here so that qsc_sfit.hip's kernels keep their code and registers.  After the halves
// are summed, each existing neighbour n and each r < R adds, with d = s_r - S[n][r]:
//     f    += weight * rho(d)       in fp64 from the fp32 operands (the accept test compares
//                                   values of phi that differ by |g|^2 / lambda near the minimiser)
//     g_r  += weight * rho'(d)      QUAD: d;  HUBER: clamp(d / delta, -1, 1)
//     J_rr += weight * kappa(d)     QUAD: 1;  HUBER: 1 / max(|d|, delta), the half-quadratic
//                                   majoriser: rho'' inside |d| <= delta, positive outside
// and then qsc_sfit's rules run unchanged: Cholesky of J + (ridge + mu) I, s' = s - delta
// (clipped at 0 with project), accept iff phi' <= phi and finite, the mu schedule, at most
// inner_steps trial evaluations, the early exit on a converged accepted step.  mu restarts at mu0
// every visit; nothing is kept per position between launches.
//
// Neighbour rows are constant during a visit.  They are not staged: the (up to) four rows are
// re-read as 16-byte vectors after every walk, one vector live at a time.  A row is 16 to 64
// bytes that the first read of the visit leaves in the cache, the reads are 4 RP / 4 per position
// against a walk of tens of entries with an LDS row each, and RP 16 has no registers (and the
// walk no LDS to spare at large K) to hold 64 more values across the walk.
//
// The row at the start of the visit is not kept either: it is read again just before the row is
// written (by the lanes that then write it), for the n_moved test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>

#include "qsc_common.cuh"
#include "qsc_info.cuh"

namespace {
using namespace qsc;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// the smallest non-zero damping (qsc_sfit's)
constexpr float kMuMin = 1.0e-6f;
constexpr int64_t kSmoothMaxPp = (int64_t)1 << 28;  // qsc_smooth.hip's position bound

enum { SMOOTH_QUAD = QSC_SMOOTH_QUAD, SMOOTH_HUBER = QSC_SMOOTH_HUBER };

// ranks whose accepted (g, J) are kept in the workspace instead of a second register set
__host__ __device__ constexpr bool sfs_in_ws(int RP) { return RP > 8; }

struct SfsParams {
  float ridge, mu0, tol;
  int inner_steps, project;
  int color, J, Pp;
  int huber;
  float weight, delta, inv_delta;
};

// rho(d) in fp64 from the fp32 operands; inv_dl = 1 / delta, dl = delta (huber only)
__device__ __forceinline__ double rho64(float a, float b, bool huber, double dl, double inv_dl) {
  const double dd = (double)a - (double)b;
  if (!huber) return 0.5 * dd * dd;
  const double zd = dd * inv_dl;
  return fabs(zd) <= 1.0 ? 0.5 * dd * zd : fabs(dd) - 0.5 * dl;
}

template <int RP, typename E, bool SR, bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) sfit_smooth_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    int64_t n_ent, int nslices, Link lk, Edges E_, int R, int K, int P_,
    const int* __restrict__ perm, const int4* __restrict__ nbr, const float* __restrict__ C,
    float* S, SfsParams pr, float* __restrict__ f_out, float* __restrict__ nll_out,
    int* __restrict__ steps_out, int* __restrict__ n_moved, int* __restrict__ n_unconverged,
    int* __restrict__ n_unidentified, float* __restrict__ ws) {
  constexpr int CP = info_pitch(RP);
  constexpr int NT = RP * (RP + 1) / 2;
  constexpr bool WS = sfs_in_ws(RP);
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
  int cnt_moved = 0, cnt_unconv = 0, cnt_unident = 0;  // (wave-uniform)
  // WS: the lane's row (g first, then the triangle of J), reused by every slice of the wave
  float* wrow = ws + ((size_t)(blockIdx.x * kWaves + wave) * 64 + lane) * (RP + NT);
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    // own: a pixel of this visit's colour; every other position is neither changed nor written
    const bool own = p >= 0 && p < P_ && ((((p / pr.J) + (p % pr.J)) & 1) == pr.color);
    if (__ballot(own) == 0ull) continue;  // (wave-uniform)
    // the accepted state (sc, fc, gc, Jc) and the trial point st
    float sc[RP], st[RP], gc[WS ? 1 : RP], Jc[WS ? 1 : NT];
    double fc = 0.0;
#pragma unroll
    for (int r = 0; r < RP; r += 4) {
      const float4 x = *reinterpret_cast<const float4*>(S + q * RP + r);
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) sc[r + e] = (own && r + e < R) ? xs[e] : 0.0f;
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
    bool done = !own, ident = false, step_ok = true;
    int nwalk = 0;
    const int nch = width[s] >> 2;  // 4-entry chunks of every list of the slice
    const int64_t base = off[s] + l * 4 + 2 * h;
    for (int it = 0;; ++it) {
      // ---- walk: (ft, gt, Jt) at st (sfit_kernel's) ----
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
        // the next chunk's entries while this one is worked (clamped in load_pair)
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
      // ---- the prior: every existing neighbour (left, right, up, down), r ascending ----
      int nn[4];
      // (the neighbours' positions are read here, not held across the walk; -1: none, and an
      // entry out of range is read as none)
      // (the fp64 constants are formed here, not held across the walk)
      const double dl = (double)pr.delta, inv_dl = pr.huber ? 1.0 / dl : 1.0;
      double pf = 0.0;
      const int4 n4 = nbr[q];
      const int nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        nn[e] = (own && nv[e] >= 0 && nv[e] < pr.Pp) ? nv[e] : -1;
        if (nn[e] >= 0) {
          const float* nrow = S + (int64_t)nn[e] * RP;
#pragma unroll
          for (int r = 0; r < RP; r += 4) {
            const float4 x = *reinterpret_cast<const float4*>(nrow + r);
            const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float d = st[r + c] - xs[c];
              const double val = rho64(st[r + c], xs[c], pr.huber != 0, dl, inv_dl);
              float der, kap;
              if (pr.huber) {
                const float z = d * pr.inv_delta;
                der = fminf(fmaxf(z, -1.0f), 1.0f);
                kap = 1.0f / fmaxf(fabsf(d), pr.delta);
              } else {
                der = d;
                kap = 1.0f;
              }
              if (r + c < R) {
                pf += val;
                gt[r + c] = __builtin_fmaf(pr.weight, der, gt[r + c]);
                Jt[tri<RP>(r + c, r + c)] =
                    __builtin_fmaf(pr.weight, kap, Jt[tri<RP>(r + c, r + c)]);
              }
            }
          }
        }
      }
      ft = __builtin_fma((double)pr.weight, pf, ft);
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
      if (it == pr.inner_steps || __ballot(!done) == 0ull) break;

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
    // ---- results (half 0 of an own-colour position writes its row; nobody else writes) ----
    const bool wr = own && h == 0;
    bool moved = false;
    if (wr) {
      // the row as the visit found it, read again for the n_moved test, then overwritten
      float dmax = 0.0f, smax = 0.0f;
#pragma unroll
      for (int r = 0; r < RP; r += 4) {
        const float4 x = *reinterpret_cast<const float4*>(S + q * RP + r);
        const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s0 = r + e < R ? xs[e] : 0.0f;
          dmax = fmaxf(dmax, fabsf(sc[r + e] - s0));
          smax = fmaxf(smax, fabsf(s0));
        }
      }
      moved = dmax > pr.tol * (1.0f + smax);
#pragma unroll
      for (int r = 0; r < RP; r += 4)
        *reinterpret_cast<float4*>(S + q * RP + r) =
            make_float4(sc[r], sc[r + 1], sc[r + 2], sc[r + 3]);
      if (f_out != nullptr) f_out[q] = (float)fc;
      if (nll_out != nullptr) {
        // the likelihood part alone: phi minus the ridge and prior terms at the accepted row,
        // formed again here in the walk's order (fp64: the subtraction loses nothing that the
        // fp32 result keeps) so that no second fp64 value is carried across the walks
        double nsq = 0.0, pf = 0.0;
#pragma unroll
        for (int r = 0; r < RP; ++r) nsq = __builtin_fma((double)sc[r], (double)sc[r], nsq);
        const double dl = (double)pr.delta, inv_dl = pr.huber ? 1.0 / dl : 1.0;
        const int4 n4 = nbr[q];
        const int nv[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (nv[e] >= 0 && nv[e] < pr.Pp) {
            const float* nrow = S + (int64_t)nv[e] * RP;
#pragma unroll
            for (int r = 0; r < RP; r += 4) {
              const float4 x = *reinterpret_cast<const float4*>(nrow + r);
              const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
              for (int c = 0; c < 4; ++c)
                pf += r + c < R ? rho64(sc[r + c], xs[c], pr.huber != 0, dl, inv_dl) : 0.0;
            }
          }
        }
        const double nl = fc - (0.5 * (double)pr.ridge * nsq + (double)pr.weight * pf);
        nll_out[q] = (float)(fabs(fc) < (double)__builtin_inff() ? nl : fc);
      }
      if (steps_out != nullptr) steps_out[q] += nwalk;
    }
    cnt_moved += __popcll(__ballot(wr && moved));
    cnt_unconv += __popcll(__ballot(wr && !done));
    cnt_unident += __popcll(__ballot(wr && !ident));
  }
  // one integer atomic per wave and counter (integer addition: any order gives the same count)
  if (lane == 0) {
    if (cnt_moved != 0) atomicAdd(n_moved, cnt_moved);
    if (cnt_unconv != 0) atomicAdd(n_unconverged, cnt_unconv);
    if (cnt_unident != 0) atomicAdd(n_unidentified, cnt_unident);
  }
}

int cu_count_sfs() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
    return 256;
  return n;
}

// qsc_sfit's grid: a grid-stride walk over the slices (any grid gives the same bits); with the
// workspace only twice the workgroups resident at the one wave per SIMD the RP 16 kernels run at
int64_t sfs_grid(int nslices, int RP) {
  const int64_t want = ceil_div(nslices, kWaves);
  return std::min<int64_t>(want, (int64_t)cu_count_sfs() * (sfs_in_ws(RP) ? 2 : 8));
}

}  // namespace

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" {

QSC_API size_t qsc_sfit_smooth_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  if (!d || R < 1 || R > QSC_MAX_R || d->Pp < 1) return 0;
  const int RP = qsc_rank_pad(R);
  if (!sfs_in_ws(RP)) return 0;  // (the state before a trial step stays in registers)
  return (size_t)sfs_grid(d->Pp / QSC_SLICE, RP) * kWaves * 64 * (RP + RP * (RP + 1) / 2) *
         sizeof(float);
}

QSC_API int qsc_sfit_smooth(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                            const int64_t* s_off, const int32_t* perm, const int32_t* nbr,
                            int32_t I, int32_t J, int32_t color, const qsc_model* m, int32_t R,
                            const float* C, float* S, int32_t kind, float ridge, float mu0,
                            float tol, int32_t inner_steps, int32_t project, int32_t smooth_kind,
                            float delta, float weight, float* f_out, float* nll_out,
                            int32_t* steps, int32_t* n_moved, int32_t* n_unconverged,
                            int32_t* n_unidentified, void* ws, size_t ws_bytes, void* stream) {
  if (!d || !s_width || !s_off || !perm || !nbr || !C || !S || !n_moved || !n_unconverged ||
      !n_unidentified || !info_model_ok(m))
    return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  if (!(ridge >= 0.0f) || !(mu0 >= 0.0f) || !(tol > 0.0f) || inner_steps < 1) return QSC_EINVAL;
  if (color != 0 && color != 1) return QSC_EINVAL;
  if (!(weight >= 0.0f)) return QSC_EINVAL;
  if (smooth_kind != SMOOTH_QUAD && smooth_kind != SMOOTH_HUBER) return QSC_EINVAL;
  if (smooth_kind == SMOOTH_HUBER && !(delta > 0.0f)) return QSC_EINVAL;
  if (!info_layout_ok(d, m, R) || (d->s_entries > 0 && !s_entries)) return QSC_EINVAL;
  if (I < 1 || J < 1 || (int64_t)I * J != (int64_t)d->P) return QSC_EINVAL;
  if ((int64_t)d->Pp > kSmoothMaxPp) return QSC_EUNSUPPORTED;
  const size_t need = qsc_sfit_smooth_workspace_bytes(d, R);
  if (need > 0 && (!ws || ws_bytes < need)) return QSC_EINVAL;
  const int RP = qsc_rank_pad(R);
  const size_t shm = sinfo_lds(d->K, RP, d->nbins);
  if (shm > kInfoLdsMax) return QSC_EUNSUPPORTED;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const int nslices = d->Pp / QSC_SLICE;
  const bool huber = smooth_kind == SMOOTH_HUBER;
  const SfsParams pr = {ridge, mu0, tol, inner_steps, project != 0, color, J, d->Pp, huber ? 1 : 0,
                        weight, huber ? delta : 0.0f, huber ? 1.0f / delta : 1.0f};
  const dim3 grid((unsigned)sfs_grid(nslices, RP)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  const bool sr = d->rowfmt == 1;
  const int4* n4 = reinterpret_cast<const int4*>(nbr);
#define SFS_LAUNCH_E(RPV, ET, SRV, LGT, LOGV, KD)                                                 \
  hipLaunchKernelGGL((sfit_smooth_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, shm, hs,       \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, nslices, lk, E, \
                     R, d->K, d->P, perm, n4, C, S, pr, f_out, nll_out, steps, n_moved,           \
                     n_unconverged, n_unidentified, (float*)ws)
#define SFS_LAUNCH_RP(RPV, LGT, LOGV, KD)                                  \
  do {                                                                     \
    if (sr) {                                                              \
      /* (signed rows: linear one-bit only) */                             \
      if (!LOGV) SFS_LAUNCH_E(RPV, uint16_t, true, LGT, false, KD);        \
    } else if (d->wide) SFS_LAUNCH_E(RPV, uint32_t, false, LGT, LOGV, KD); \
    else SFS_LAUNCH_E(RPV, uint16_t, false, LGT, LOGV, KD);                \
  } while (0)
#define SFS_LAUNCH(LGT, LOGV, KD)                      \
  do {                                                 \
    if (RP == 4) SFS_LAUNCH_RP(4, LGT, LOGV, KD);      \
    else if (RP == 8) SFS_LAUNCH_RP(8, LGT, LOGV, KD); \
    else SFS_LAUNCH_RP(16, LGT, LOGV, KD);             \
  } while (0)
  QSC_INFO_DISPATCH(SFS_LAUNCH);
#undef SFS_LAUNCH
#undef SFS_LAUNCH_RP
#undef SFS_LAUNCH_E
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
