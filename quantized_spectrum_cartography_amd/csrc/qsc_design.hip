// qsc_design.hip — expected information gain of a planned batch of readings, per position
// (include/qsc.h: qsc_sgain).
//
// Conditional on C the positions are independent, so the value of a plan w[K] (w_k >= 0 readings
// of bin k) is a per-position figure.  With J_q the information block of the readings already held
// (qsc_sinfo, either kind; passed in), t = S[q] . c_k and h_exp the Fisher information of one
// reading (entry_curvature<..., INFO_EXPECTED>: it does not depend on the code the reading returns)
//     A_q = sum_k w_k h_exp(t_kq) c_k c_k^T,    M0 = J_q + ridge I,    M1 = M0 + A_q
//     D:  1/2 (logdet M1 - logdet M0)           expected entropy reduction, nats
//     A:  tr(M0^-1) - tr(M1^-1)                 reduction of sum_r var(S_r)
//     V:  tr(G M0^-1) - tr(G M1^-1), G = C C^T  reduction of sum_k var(T_hat[k, q])
// Rows and columns >= R are the identity (info_std_kernel's rule) and are left out of every sum.
// A bin with w_k == 0 is not evaluated; in the log model an entry with t + offset <= 0 adds 0
// (entry_terms' neg rule).
//
// Shape (sinfo_kernel's): one wave per slice of QSC_SLICE positions, grid-stride; C^T, the edges
// and w in LDS (a row of C^T is read at one address by the 32 lanes of a half: a broadcast); two
// lanes per position.  Lane half h takes bins h, h + 2, ... of the dense loop over k and keeps the
// upper triangle of its part of A_q in registers; one lane swap adds the parts.  Half 0 then
// factors M0 and half 1 factors M1 (QSC_CHOL_INVERSE, the rule of qsc_info_std: a pivot that is
// not positive marks the matrix), each reduces its own figure -- sum log pivot, sum M[i][j]^2 of
// the inverse factor, or sum_i m_i^T G m_i over its rows -- a second swap forms the difference and
// half 0 stores it.  The difference of two logdets is used as it stands: both are sums of R
// logarithms of pivots good to an ulp, and M1 - M0 is no small perturbation for a plan worth
// asking about.
// M0 not positive definite but M1 is: +inf, a first look (*n_first); M1 not positive definite (or
// a figure that is not finite): 0 (*n_bad).  Padding positions are written as 0 and not counted.
// Integer atomics only, one per wave and counter: two calls agree bit for bit.
#include <hip/hip_runtime.h>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

enum { DESIGN_D = QSC_DESIGN_D, DESIGN_A = QSC_DESIGN_A, DESIGN_V = QSC_DESIGN_V };

template <int RP, bool LOGIT, bool LOG, int CRIT>
__global__ void __launch_bounds__(kBlock) sgain_kernel(
    int nslices, Link lk, Edges E_, int R, int K, int P_, const int* __restrict__ perm,
    const float* __restrict__ S, const float* __restrict__ C, const float* __restrict__ J,
    const float* __restrict__ w, const float* __restrict__ G, float ridge,
    float* __restrict__ gain, int* __restrict__ n_first, int* __restrict__ n_bad) {
  constexpr int CP = info_pitch(RP);
  constexpr int NT = tri_count(RP);
  QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_);
  float* wl = reinterpret_cast<float*>(El + lk.nbins);  // [K], ones without a plan
  for (int k = threadIdx.x; k < K; k += kBlock) wl[k] = w != nullptr ? w[k] : 1.0f;
  __syncthreads();
  QSC_SLANE_GEOMETRY();
  int cnt_first = 0, cnt_bad = 0;  // (wave-uniform)
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    const bool live = p >= 0 && p < P_;
    float sv[RP];
    QSC_ROW_LOAD_MASKED(RP, sv, S + q * RP, live, R)
    // this half's part of A_q: bins h, h + 2, ...
    float acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.0f;
    for (int k = h; k < K; k += 2) {
      const float wk = wl[k];
      if (live && wk != 0.0f) {
        float cv[RP];
        QSC_ROW_LOAD(RP, cv, Cl + k * CP)
        float t = 0.0f;
#pragma unroll
        for (int r = 0; r < RP; ++r) t = __builtin_fmaf(sv[r], cv[r], t);
        float hh = entry_curvature<LOGIT, LOG, INFO_EXPECTED>(t, 0, El, lk);
        if (LOG) hh = (t + lk.offset > 0.0f) ? hh : 0.0f;
        hh *= wk;
        QSC_BLOCK_UPDATE(RP, RP, acc, hh, cv, )
      }
    }
    // the two halves' parts (the same bits on both lanes)
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] += __shfl_xor(acc[i], 32, 64);
    // M0 (half 0) or M1 (half 1): lower triangle a[i][j], j <= i, at tri(j, i)
    float a[NT];
    const float* Jq = J + q * (RP * RP);
#pragma unroll
    for (int i = 0; i < RP; ++i) {
#pragma unroll
      for (int j0 = 0; j0 <= i; j0 += 4) {
        QSC_VEC4(xs, Jq + i * RP + j0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = j0 + e;
          if (j <= i) {
            float v = xs[e];
            if (j == i) v += ridge;
            v += h ? acc[tri<RP>(j, i)] : 0.0f;
            if (i >= R) v = (j == i) ? 1.0f : 0.0f;
            a[tri<RP>(j, i)] = live ? v : ((j == i) ? 1.0f : 0.0f);
          }
        }
      }
    }
    float dinv[RP];
    bool bad = false;
    QSC_CHOL_INVERSE(RP, a, dinv, bad)
    // this half's figure, rows < R only (the identity rows add the same to both and are left out)
    float val = 0.0f;
    if (CRIT == DESIGN_D) {
      // log pivot_j = -2 log(1 / L[j][j])
#pragma unroll
      for (int j = 0; j < RP; ++j) val += j < R ? logf(dinv[j]) : 0.0f;
      val = -val;  // 1/2 logdet
    } else if (CRIT == DESIGN_A) {
      // tr(M^-1) = sum of the squares of L^-1
#pragma unroll
      for (int i = 0; i < RP; ++i) {
        float v = 0.0f;
#pragma unroll
        for (int j = 0; j <= i; ++j) v = __builtin_fmaf(a[tri<RP>(j, i)], a[tri<RP>(j, i)], v);
        val += i < R ? v : 0.0f;
      }
    } else {
      // tr(G M^-1) = sum_i m_i^T G m_i, m_i row i of L^-1 (G[j][jj]: one address on every lane)
#pragma unroll
      for (int i = 0; i < RP; ++i) {
        float v = 0.0f;
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          float y = 0.0f;
#pragma unroll
          for (int jj = 0; jj <= i; ++jj) y = __builtin_fmaf(G[j * RP + jj], a[tri<RP>(jj, i)], y);
          v = __builtin_fmaf(a[tri<RP>(j, i)], y, v);
        }
        val += i < R ? v : 0.0f;
      }
    }
    bad = bad || !(fabsf(val) < __builtin_inff());
    const float other = __shfl_xor(val, 32, 64);
    const bool obad = __shfl_xor((int)bad, 32, 64) != 0;
    // on half 0: (val, bad) of M0, (other, obad) of M1
    const bool bad1 = obad, bad0 = bad;
    const float diff = CRIT == DESIGN_D ? other - val : val - other;
    float g = fmaxf(diff, 0.0f);
    g = bad0 ? __builtin_inff() : g;
    g = bad1 ? 0.0f : g;
    g = live ? g : 0.0f;
    const bool mine = live && h == 0;
    if (h == 0) gain[q] = g;
    cnt_first += __popcll(__ballot(mine && bad0 && !bad1));
    cnt_bad += __popcll(__ballot(mine && bad1));
  }
  // one integer atomic per wave and counter (integer addition: any order gives the same count)
  if (lane == 0) {
    if (cnt_first) atomicAdd(n_first, cnt_first);
    if (cnt_bad) atomicAdd(n_bad, cnt_bad);
  }
}

}  // namespace

extern "C" {

QSC_API int qsc_sgain(const float* S, const float* C, const float* J, const int32_t* perm,
                      const float* w, const float* G, const qsc_model* m, int32_t R, int32_t K,
                      int32_t P, int32_t Pp, int32_t criterion, float ridge, float* gain,
                      int32_t* n_first, int32_t* n_bad, void* stream) {
  if (!S || !C || !J || !perm || !gain || !n_first || !n_bad || !info_model_ok(m))
    return QSC_EINVAL;
  if (R < 1 || R > QSC_MAX_R || K < 1 || P < 1 || Pp < P || (Pp % QSC_SLICE) != 0 ||
      !(ridge >= 0.0f))
    return QSC_EINVAL;
  if (criterion != DESIGN_D && criterion != DESIGN_A && criterion != DESIGN_V) return QSC_EINVAL;
  if (criterion == DESIGN_V && !G) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = walk_launch(K, Pp, m, R, (size_t)K * 4, &wl);  // (w[K] after the edges)
  if (rc != QSC_OK) return rc;
  const int RP = wl.RP;
  const dim3 grid((unsigned)slice_grid(wl.nslices, 8)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  const int kind = INFO_EXPECTED;  // (the planned readings' codes are not known: always expected)
#define SGAIN_LAUNCH_(RPV, LGT, LOGV, CR)                                                  \
  hipLaunchKernelGGL((sgain_kernel<RPV, LGT, LOGV, CR>), grid, blk, wl.shm, hs, wl.nslices, \
                     wl.lk, wl.E, R, K, P, perm, S, C, J, w, G, ridge, gain, n_first, n_bad)
#define SGAIN_CRIT_(RPV, LGT, LOGV)                                       \
  do {                                                                    \
    if (criterion == DESIGN_D) SGAIN_LAUNCH_(RPV, LGT, LOGV, DESIGN_D);   \
    else if (criterion == DESIGN_A) SGAIN_LAUNCH_(RPV, LGT, LOGV, DESIGN_A); \
    else SGAIN_LAUNCH_(RPV, LGT, LOGV, DESIGN_V);                         \
  } while (0)
#define SGAIN_LAUNCH(LGT, LOGV, KD) QSC_RP_DISPATCH(SGAIN_CRIT_, LGT, LOGV)
  QSC_INFO_DISPATCH(SGAIN_LAUNCH);
#undef SGAIN_LAUNCH
#undef SGAIN_CRIT_
#undef SGAIN_LAUNCH_
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
