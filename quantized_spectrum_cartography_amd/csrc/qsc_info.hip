// qsc_info.hip — per-pixel Fisher information of the loss fields and the standard deviations it
// implies (include/qsc.h: qsc_sinfo, qsc_info_std, qsc_entry_info).
//
// Conditional on C, the Hessian of the NLL with respect to S is block diagonal; position q has
//     J_q = sum_{k observed at q} h(k, q) c_k c_k^T,   c_k = C[:, k]                  (R x R)
// with h the curvature of one entry's -log P in t = T_hat[k, q].  In the model domain x (x = t,
// or log(t + offset)), with u = (hi - x) / a, w = (lo - x) / a, phi = F':
//     P   = F(hi - x) - F(lo - x)
//     P'  = -(phi(hi - x) - phi(lo - x))
//     P'' = phi'(hi - x) - phi'(lo - x)
//     g_x = -P' / P
//     observed:  h_x = (P'/P)^2 - P''/P  at the entry's own code
//     expected:  h_x = sum_b (P_b')^2 / P_b  over all bins (bins with P_b == 0 dropped)
//   probit:  phi(y) = exp(-(y/a)^2) / (a sqrt(pi)),  P'' = -(2 u phi(u) - 2 w phi(w)) / a
//   logit:   phi = F (1 - F) / s,                    phi' = phi (1 - 2 F) / s
//   chain:   linear h = h_x;  log model observed h = (h_x - g_x) / (t + offset)^2,
//            expected h = h_x / (t + offset)^2
// The reference has no counterpart (it returns point estimates only).
//
// Numerics.  A bin's pair (u, w) is mirrored into the lower half first ((u, w) -> (-w, -u) when
// u + w > 0: P and P'' are unchanged, P' changes sign), where F is evaluated as a tail
// (0.5 erfc(-z), or E / (1 + E)) at full relative precision, so P never cancels two values near 1.
// A saturated or infinite edge (|z| beyond kSatProbit / kSatLogit, where phi is 0 in fp32)
// contributes exactly 0 to phi and to z phi: no product meets an infinity.  An entry whose P
// underflows to 0 has no representable curvature and contributes 0.
//
// qsc_sinfo walks the S-format lists as qsc_newton.cuh describes; a lane half keeps the upper
// triangle of its partial block in registers; the halves are added once and each half writes
// RP / 2 rows of the full symmetric block.  No atomics: the order of every sum is fixed by the
// packing alone.
// qsc_info_std: one thread per position, Cholesky of J_q + ridge I in registers, the triangular
// inverse in place (QSC_CHOL_INVERSE); std_S from its column norms, std_T[k] = |L^-1 c_k|.
#include <hip/hip_runtime.h>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

template <int RP, typename E, bool SR, bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) sinfo_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    int64_t n_ent, int nslices, Link lk, Edges E_, int R, int K, const float* __restrict__ S,
    const float* __restrict__ C, float* __restrict__ J) {
  constexpr int CP = info_pitch(RP);
  constexpr int NT = tri_count(RP);
  QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_);
  QSC_SLANE(E, SR, K);
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    float sv[RP];
    QSC_ROW_LOAD(RP, sv, S + q * RP)
    float acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.0f;
    QSC_SLICE_LISTS(s);
    QSC_WALK_BEGIN(RP, CP, E, SR, sv)
      float hh = entry_curvature<LOGIT, LOG, KIND>(t, code, El, lk);
      hh = pad ? 0.0f : hh;  // a pad adds exactly 0 (c_k is finite)
      QSC_BLOCK_UPDATE(RP, RP, acc, hh, cv, )
    QSC_WALK_END
    // the two halves' partial blocks (the same bits on both lanes), then each half's rows
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] += __shfl_xor(acc[i], 32, 64);
    float* out = J + q * (RP * RP);
#pragma unroll
    for (int ii = 0; ii < RP / 2; ++ii) {
#pragma unroll
      for (int j = 0; j < RP; j += 4) {
        // row ii (half 0) or row RP / 2 + ii (half 1), columns j .. j + 3
        const int i0 = ii, i1 = RP / 2 + ii;
        const float4 val = make_float4(h ? acc[sym<RP>(i1, j)] : acc[sym<RP>(i0, j)],
                                       h ? acc[sym<RP>(i1, j + 1)] : acc[sym<RP>(i0, j + 1)],
                                       h ? acc[sym<RP>(i1, j + 2)] : acc[sym<RP>(i0, j + 2)],
                                       h ? acc[sym<RP>(i1, j + 3)] : acc[sym<RP>(i0, j + 3)]);
        *reinterpret_cast<float4*>(out + (h * (RP / 2) + ii) * RP + j) = val;
      }
    }
  }
}

// elementwise curvature (qsc_entry_info): the device function of the kernel above
template <bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) entry_info_kernel(const int64_t* __restrict__ Y,
                                                            const float* __restrict__ T, int64_t n,
                                                            Link lk, Edges E_,
                                                            float* __restrict__ H) {
  QSC_ENTRYWISE_STAGE(lk, E_.e[b_]);
  QSC_ENTRYWISE_BEGIN(lk)
    H[i] = entry_curvature<LOGIT, LOG, KIND>(T[i], (int)y, se, lk);
  QSC_ENTRYWISE_END
}

// One thread per position: Cholesky of J_q + ridge I (rows >= R replaced by the identity), the
// inverse of the factor in place, then the standard deviations.
template <int RP>
__global__ void __launch_bounds__(kBlock) info_std_kernel(
    const float* __restrict__ J, const int* __restrict__ perm, int R, int P, int Pp,
    const float* __restrict__ C, int K, float ridge, float* __restrict__ std_S,
    float* __restrict__ std_T, int* __restrict__ nbad) {
  const int64_t q = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  bool bad = false;
  if (q < Pp) {
    const int p = perm[q];
    const bool live = p >= 0 && p < P;
    float out[RP];
#pragma unroll
    for (int i = 0; i < RP; ++i) out[i] = 0.0f;
    if (live) {
      // lower triangle a[i][j], j <= i, at tri(j, i)
      float a[tri_count(RP)];
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
              if (i >= R) v = (j == i) ? 1.0f : 0.0f;
              a[tri<RP>(j, i)] = v;
            }
          }
        }
      }
      float dinv[RP];
      QSC_CHOL_INVERSE(RP, a, dinv, bad)
#pragma unroll
      for (int j = 0; j < RP; ++j) {
        float v = 0.0f;
#pragma unroll
        for (int i = j; i < RP; ++i) v = __builtin_fmaf(a[tri<RP>(j, i)], a[tri<RP>(j, i)], v);
        out[j] = j < R ? (bad ? __builtin_inff() : sqrtf(v)) : 0.0f;
      }
      if (std_T != nullptr) {
        for (int k = 0; k < K; ++k) {  // (C[r][k]: the same address on every lane)
          float ck[RP];
#pragma unroll
          for (int r = 0; r < RP; ++r) ck[r] = r < R ? C[(int64_t)r * K + k] : 0.0f;
          float v = 0.0f;
#pragma unroll
          for (int i = 0; i < RP; ++i) {
            float y = 0.0f;
#pragma unroll
            for (int j = 0; j <= i; ++j) y = __builtin_fmaf(a[tri<RP>(j, i)], ck[j], y);
            v = __builtin_fmaf(y, y, v);
          }
          std_T[(int64_t)k * P + p] = bad ? __builtin_inff() : sqrtf(v);
        }
      }
    }
    QSC_ROW_STORE(RP, std_S + q * RP, out);
  }
  // one integer atomic per wave (integer addition: any order gives the same count)
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && m != 0ull) atomicAdd(nbad, __popcll(m));
}

}  // namespace

extern "C" {

QSC_API int qsc_sinfo(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                      const int64_t* s_off, const qsc_model* m, int32_t R, const float* S,
                      const float* C, int32_t kind, float* J, void* stream) {
  if (!d || !s_width || !s_off || !S || !C || !J || !info_model_ok(m)) return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  if (!info_layout_ok(d, m, R) || (d->s_entries > 0 && !s_entries)) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = walk_launch(d, m, R, &wl);
  if (rc != QSC_OK) return rc;
  const int RP = wl.RP;
  const dim3 grid((unsigned)slice_grid(wl.nslices, 8)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
#define SINFO_LAUNCH(RPV, ET, SRV, LGT, LOGV, KD)                                             \
  hipLaunchKernelGGL((sinfo_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, wl.shm, hs,      \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, wl.nslices, \
                     wl.lk, wl.E, R, d->K, S, C, J)
  QSC_LAYOUT_DISPATCH(SINFO_LAUNCH);
#undef SINFO_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_info_std(const float* J, const int32_t* perm, int32_t R, int32_t P, int32_t Pp,
                         const float* C, int32_t K, float ridge, float* std_S, float* std_T,
                         int32_t* nbad, void* stream) {
  if (!J || !perm || !std_S || !nbad || R < 1 || R > QSC_MAX_R || P < 1 || Pp < P ||
      !(ridge >= 0.0f) || (std_T && (!C || K < 1)))
    return QSC_EINVAL;
  const int RP = qsc_rank_pad(R);
  const dim3 grid((unsigned)ceil_div(Pp, kBlock)), blk(kBlock);
#define STD_LAUNCH(RPV)                                                                          \
  hipLaunchKernelGGL(info_std_kernel<RPV>, grid, blk, 0, STREAM(stream), J, perm, R, P, Pp, C, K, \
                     ridge, std_S, std_T, nbad)
  QSC_RP_DISPATCH(STD_LAUNCH);
#undef STD_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_entry_info(const int64_t* Y, const float* T, int64_t n, const qsc_model* m,
                           int32_t kind, float* H, void* stream) {
  if (!entry_args_ok(m, n, Y, T, H)) return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  if (n == 0) return QSC_OK;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const dim3 grid = entry_grid(n), blk(kBlock);
  hipStream_t hs = STREAM(stream);
#define ENTRY_LAUNCH(LGT, LOGV, KD) \
  hipLaunchKernelGGL((entry_info_kernel<LGT, LOGV, KD>), grid, blk, 0, hs, Y, T, n, lk, E, H)
  QSC_INFO_DISPATCH(ENTRY_LAUNCH);
#undef ENTRY_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
