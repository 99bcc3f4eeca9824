// qsc_check.hip — per-position goodness of fit and level-shift score tests of the readings
// against the fitted model (include/qsc.h: qsc_scheck, qsc_entry_check).
//
// A position is a physical sensor.  Per entry e = (k, y) of position q, with t = s_q . c_k,
// x = t (linear) or log(t + offset), dxdt = 1 or 1 / (t + offset), and P_b, P_b' of every bin from
// bin_terms (bins with P_b == 0 dropped from every sum over b):
//     l   = -log max(P_y, FLT_MIN)
//     H   = -sum_b P_b log P_b                  the model's own expectation of l
//     var = max(sum_b P_b log^2 P_b - H^2, 0)   its variance
//     g_x = -P_y' / P_y                         (0 if P_y == 0)
//     h_x = sum_b P_b'^2 / P_b                  QSC_INFO_EXPECTED
// Per position:
//     D = sum (l - H),  V = sum var,  n = entries used,  u = sum g_x,  Ixx = sum h_x
//     g = sum g_x dxdt c_k + ridge s_q,  v = sum h_x dxdt c_k,  J = sum h_x dxdt^2 c_k c_k^T + ridge I
//     fitted = 0:  u* = u, I* = Ixx
//     fitted = 1:  J = L L^T, a = L^-1 v, b = L^-1 g:  u* = u - a . b,  I* = Ixx - a . a
// (the efficient score of a shift x -> x + delta with s_q the nuisance parameter, and the Schur
// complement of the (R + 1) x (R + 1) expected information of (s_q, delta)).
//
// Shape (sinfo_kernel's): one wave per slice of QSC_SLICE positions, grid-stride; C^T at the
// info_pitch pitch and the edges in LDS; two lanes per position, each takes alternate entry pairs
// in list order; one lane swap adds the halves.  A single loop over the bins per entry gives every
// term, the entry's own code picked inside it.  Per-entry terms are fp32; D and V accumulate in
// fp64 (l - H cancels), the rest in fp32.  With fitted = 1 both lanes of a position then factor J
// column by column (right-looking: a column is dead once it has updated the trailing block and
// the two right-hand sides, so the triangle shrinks as the factor proceeds; the sums run in the
// order of QSC_CHOL_SOLVE, with its pivot rule: a pivot that is not positive is replaced by 1 and
// marks the position).  No workspace, no atomics: two calls agree bit for bit.
#include <hip/hip_runtime.h>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

enum { CHECK_UNTESTABLE = QSC_CHECK_UNTESTABLE, CHECK_INVALID = QSC_CHECK_INVALID,
       CHECK_SATURATED = QSC_CHECK_SATURATED };
// I* <= kGuard Ixx: the shift is confounded with s_q or I* is rounding noise (the fp32 quadratic
// form carries about R 2^-24 Ixx ~ 1e-6 Ixx at R = 16; the guard sits 100 x above that)
constexpr float kGuard = 1.0e-4f;

// One entry's terms at the map value t and the code `code`; neg: t + offset <= 0 in the log model
// (every other output is then meaningless); sat: the fp32 P of the entry's own code is 0.
template <bool LOGIT, bool LOG>
__device__ __forceinline__ void entry_check(float t, int code, const float2* __restrict__ edges,
                                            const Link& c, float& dl, float& var, float& gx,
                                            float& hx, float& dxdt, bool& sat, bool& neg) {
  float x = t;
  dxdt = 1.0f;
  neg = false;
  if (LOG) {
    const float tp = t + c.offset;
    neg = !(tp > 0.0f);
    x = logf(tp);
    dxdt = 1.0f / tp;
  }
  float H = 0.0f, M2 = 0.0f, Py = 0.0f, P1y = 0.0f;
  hx = 0.0f;
  for (int b = 0; b < c.nbins; ++b) {
    const float2 e = edges[b];
    float P, P1, P2;
    bin_terms<LOGIT>(x, e.x, e.y, c, P, P1, P2);
    const bool on = P > 0.0f;
    const float lp = logf(P);
    const float plp = P * lp;
    H -= on ? plp : 0.0f;
    M2 += on ? plp * lp : 0.0f;
    const float term = P1 * P1 / P;
    hx += on ? term : 0.0f;
    Py = b == code ? P : Py;
    P1y = b == code ? P1 : P1y;
  }
  sat = !(Py > 0.0f);
  // (a true division: with a denormal P the reciprocal is +inf)
  gx = sat ? 0.0f : -P1y / Py;
  dl = -logf(fmaxf(Py, FLT_MIN)) - H;
  var = fmaxf(M2 - H * H, 0.0f);
}

template <int RP, typename E, bool SR, bool LOGIT, bool LOG, bool FITTED>
__global__ void __launch_bounds__(kBlock) scheck_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    int64_t n_ent, int nslices, Link lk, Edges E_, int R, int K, int P_,
    const int* __restrict__ perm, const float* __restrict__ S, const float* __restrict__ C,
    float ridge, float4* __restrict__ stat, int* __restrict__ count, int* __restrict__ flags) {
  constexpr int CP = info_pitch(RP);
  constexpr int NT = FITTED ? tri_count(RP) : 1;
  constexpr int NV = FITTED ? RP : 1;
  QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_);
  QSC_SLANE(E, SR, K);
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    const bool live = p >= 0 && p < P_;
    float sv[RP];
    QSC_ROW_LOAD_MASKED(RP, sv, S + q * RP, live, R)
    double D = 0.0, V = 0.0;
    float u = 0.0f, Ixx = 0.0f;
    int n = 0;
    bool inv = false, satf = false;
    float g[NV], v[NV], Jt[NT];
#pragma unroll
    for (int i = 0; i < NV; ++i) g[i] = v[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < NT; ++i) Jt[i] = 0.0f;
    QSC_SLICE_LISTS(s);
    QSC_WALK_BEGIN(RP, CP, E, SR, sv)
      float dl, var, gx, hx, dxdt;
      bool sat, neg;
      entry_check<LOGIT, LOG>(t, code, El, lk, dl, var, gx, hx, dxdt, sat, neg);
      // a pad and an entry with t + offset <= 0 add exactly 0 (selects: their terms may be NaN)
      const bool on = live && !pad && !neg;
      inv = inv || (live && !pad && neg);
      satf = satf || (on && sat);
      n += on ? 1 : 0;
      D += on ? (double)dl : 0.0;
      V += on ? (double)var : 0.0;
      const float gu = (on && !sat) ? gx : 0.0f;
      const float hu = on ? hx : 0.0f;
      u += gu;
      Ixx += hu;
      if (FITTED) {
        const float dx = on ? dxdt : 0.0f;
        const float ge = gu * dx, hv = hu * dx;
        const float hj = hv * dx;
        QSC_BLOCK_UPDATE(RP, NV, Jt, hj, cv, g[i_] = __builtin_fmaf(ge, cv[i_], g[i_]);
                         v[i_] = __builtin_fmaf(hv, cv[i_], v[i_]);)
      }
    QSC_WALK_END
    // the two halves' partial sums: the same bits on both lanes from here on
    D += __shfl_xor(D, 32, 64);
    V += __shfl_xor(V, 32, 64);
    u += __shfl_xor(u, 32, 64);
    Ixx += __shfl_xor(Ixx, 32, 64);
    n += __shfl_xor(n, 32, 64);
    // (the exchange stands outside the ||: a lane whose own bit is set must still take part)
    const int inv_o = __shfl_xor((int)inv, 32, 64), sat_o = __shfl_xor((int)satf, 32, 64);
    inv = inv || inv_o != 0;
    satf = satf || sat_o != 0;
    float us = u, Is = Ixx;
    bool untest = false;
    if (FITTED) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        g[i] += __shfl_xor(g[i], 32, 64);
        v[i] += __shfl_xor(v[i], 32, 64);
      }
#pragma unroll
      for (int i = 0; i < NT; ++i) Jt[i] += __shfl_xor(Jt[i], 32, 64);
      // J + ridge I and g + ridge s; rows and columns >= R the identity (their v and g are 0).
      // Element (i, j), j <= i, of the lower triangle sits at tri(j, i).
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        Jt[tri<RP>(j, j)] += ridge;
        g[j] = __builtin_fmaf(ridge, sv[j], g[j]);
#pragma unroll
        for (int i = j; i < NV; ++i)
          if (i >= R) Jt[tri<RP>(j, i)] = (i == j) ? 1.0f : 0.0f;
      }
      bool bad = false;
      float aa = 0.0f, ab = 0.0f;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        float piv = Jt[tri<RP>(j, j)];
        if (!(piv > 0.0f)) {
          bad = true;
          piv = 1.0f;
        }
        const float di = 1.0f / sqrtf(piv);
        const float ya = v[j] * di, yb = g[j] * di;  // a[j], b[j]
        aa = __builtin_fmaf(ya, ya, aa);
        ab = __builtin_fmaf(ya, yb, ab);
        // column j of L, then its update of the right-hand sides and of the trailing triangle;
        // the column is dead after that
#pragma unroll
        for (int i = j + 1; i < NV; ++i) {
          const float lij = Jt[tri<RP>(j, i)] * di;
          Jt[tri<RP>(j, i)] = lij;
          v[i] = __builtin_fmaf(-lij, ya, v[i]);
          g[i] = __builtin_fmaf(-lij, yb, g[i]);
        }
#pragma unroll
        for (int i = j + 1; i < NV; ++i) {
#pragma unroll
          for (int k = j + 1; k <= i; ++k)
            Jt[tri<RP>(k, i)] =
                __builtin_fmaf(-Jt[tri<RP>(j, i)], Jt[tri<RP>(j, k)], Jt[tri<RP>(k, i)]);
        }
      }
      Is = Ixx - aa;
      us = u - ab;
      untest = bad || !(Is > kGuard * Ixx);
    }
    int fl = 0;
    if (untest && !inv) fl |= CHECK_UNTESTABLE;
    if (inv) fl |= CHECK_INVALID;
    if (satf) fl |= CHECK_SATURATED;
    const bool zero_shift = untest || inv || !live;
    const bool zero_fit = inv || !live;
    const float4 out = make_float4(zero_fit ? 0.0f : (float)D, zero_fit ? 0.0f : (float)V,
                                   zero_shift ? 0.0f : us, zero_shift ? 0.0f : Is);
    if (h == 0) {
      stat[q] = out;
      count[q] = live ? n : 0;
      flags[q] = live ? fl : 0;
    }
  }
}

// elementwise terms (qsc_entry_check): the device function of the kernel above
template <bool LOGIT, bool LOG>
__global__ void __launch_bounds__(kBlock) entry_check_kernel(const int64_t* __restrict__ Y,
                                                             const float* __restrict__ T,
                                                             int64_t n, Link lk, Edges E_,
                                                             float* __restrict__ out) {
  QSC_ENTRYWISE_STAGE(lk, E_.e[b_]);
  QSC_ENTRYWISE_BEGIN(lk)
    float dl, var, gx, hx, dxdt;
    bool sat, neg;
    entry_check<LOGIT, LOG>(T[i], (int)y, se, lk, dl, var, gx, hx, dxdt, sat, neg);
    out[i] = neg ? 0.0f : dl;
    out[n + i] = neg ? 0.0f : var;
    out[2 * n + i] = neg ? 0.0f : gx;
    out[3 * n + i] = neg ? 0.0f : hx;
    out[4 * n + i] = neg ? 0.0f : dxdt;
  QSC_ENTRYWISE_END
}

}  // namespace

extern "C" {

QSC_API int qsc_scheck(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                       const int64_t* s_off, const int32_t* perm, const qsc_model* m, int32_t R,
                       const float* S, const float* C, int32_t fitted, float ridge, float* stat,
                       int32_t* count, int32_t* flags, void* stream) {
  if (!d || !s_width || !s_off || !perm || !S || !C || !stat || !count || !flags ||
      !info_model_ok(m))
    return QSC_EINVAL;
  if ((fitted != 0 && fitted != 1) || !(ridge >= 0.0f)) return QSC_EINVAL;
  if (!info_layout_ok(d, m, R) || (d->s_entries > 0 && !s_entries)) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = walk_launch(d, m, R, &wl);
  if (rc != QSC_OK) return rc;
  const int RP = wl.RP;
  const dim3 grid((unsigned)slice_grid(wl.nslices, 8)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  const int kind = INFO_EXPECTED;  // (h_x is the expected information: the kind is fixed)
#define SCHECK_LAUNCH_(RPV, ET, SRV, LGT, LOGV, FT)                                           \
  hipLaunchKernelGGL((scheck_kernel<RPV, ET, SRV, LGT, LOGV, FT>), grid, blk, wl.shm, hs,     \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, wl.nslices, \
                     wl.lk, wl.E, R, d->K, d->P, perm, S, C, ridge,                           \
                     reinterpret_cast<float4*>(stat), count, flags)
#define SCHECK_LAUNCH(RPV, ET, SRV, LGT, LOGV, KD)                     \
  do {                                                                 \
    if (fitted) SCHECK_LAUNCH_(RPV, ET, SRV, LGT, LOGV, true);         \
    else SCHECK_LAUNCH_(RPV, ET, SRV, LGT, LOGV, false);               \
  } while (0)
  QSC_LAYOUT_DISPATCH(SCHECK_LAUNCH);
#undef SCHECK_LAUNCH
#undef SCHECK_LAUNCH_
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_entry_check(const int64_t* Y, const float* T, int64_t n, const qsc_model* m,
                            float* out, void* stream) {
  if (!entry_args_ok(m, n, Y, T, out)) return QSC_EINVAL;
  if (n == 0) return QSC_OK;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const dim3 grid = entry_grid(n), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  const int kind = INFO_EXPECTED;
#define ENTRY_LAUNCH(LGT, LOGV, KD) \
  hipLaunchKernelGGL((entry_check_kernel<LGT, LOGV>), grid, blk, 0, hs, Y, T, n, lk, E, out)
  QSC_INFO_DISPATCH(ENTRY_LAUNCH);
#undef ENTRY_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
