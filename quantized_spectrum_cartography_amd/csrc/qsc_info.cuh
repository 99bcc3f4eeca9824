// qsc_info.cuh — the link terms (P, P', P''), the per-entry curvature and terms, the S-format list
// decode and the dispatch macros shared by qsc_info.hip (information blocks) and, through
// qsc_newton.cuh, every other kernel over the packed lists (that header names them).
// qsc_info.hip's header has the formulas and the numerics.
//
// Everything lives in an anonymous namespace on purpose: each translation unit gets its own
// (inlined) copy, and the kernels that take a Link by value keep their symbol names.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "qsc_common.cuh"

namespace {
using namespace qsc;

constexpr size_t kInfoLdsMax = 160 * 1024;  // the LDS of one CU, as the passes' bound
constexpr float kSatProbit = 14.0f;   // exp(-z^2) == 0 in fp32 from |z| = 10.2 on
constexpr float kSatLogit = 100.0f;   // exp(-|z|) is denormal from |z| = 87.3 on

enum { INFO_EXPECTED = QSC_INFO_EXPECTED, INFO_OBSERVED = QSC_INFO_OBSERVED };

// per-call constants of the link
struct Link {
  float a, inv_a;  // probit: fp32(sigma * 1.414213); logit: the scale s
  float k1;        // probit: 1 / (a sqrt(pi));  logit: 1 / s
  float offset;
  int nbins;
};

inline Link make_link(const qsc_model* m) {
  Link l;
  if (m->loss == QSC_LOSS_LOGIT) {
    l.a = (float)m->sigma;
    l.k1 = 1.0f / l.a;
  } else {
    l.a = (float)(m->sigma * 1.414213);
    l.k1 = (float)(1.0 / ((double)l.a * 1.7724538509055160273));
  }
  l.inv_a = 1.0f / l.a;
  l.offset = (float)m->offset;
  l.nbins = m->nbounds - 1;
  return l;
}

// y / a, correctly rounded but for rare halfway cases (div_lik's form)
__host__ __device__ __forceinline__ float div_link(float y, const Link& c) {
  const float q = y * c.inv_a;
  const float r = __builtin_fmaf(-q, c.a, y);
  const float f = __builtin_fmaf(r, c.inv_a, q);
  return (fabsf(q) < 3.0e38f) ? f : q;  // (an infinite edge stays infinite, not NaN)
}

// exp(-z^2) with the rounding error of z^2 carried along (z^2 = s + e exactly; the argument's
// error, |z^2| 2^-24, would otherwise be the result's relative error: 1e-6 at |z| = 4)
__host__ __device__ __forceinline__ float exp_neg_sq(float z) {
  const float s = z * z;
  const float e = __builtin_fmaf(z, z, -s);
  const float E = expf(-s);
  return __builtin_fmaf(-e, E, E);
}

// One bin (lo, hi) at x: P, P' and P'' (see the file header).
template <bool LOGIT>
__host__ __device__ __forceinline__ void bin_terms(float x, float lo, float hi, const Link& c,
                                                   float& P, float& P1, float& P2) {
  const float u = div_link(hi - x, c), w = div_link(lo - x, c);
  const bool mir = (u + w) > 0.0f;
  const float uu = mir ? -w : u, ww = mir ? -u : w;  // uu > ww, uu + ww <= 0
  if (LOGIT) {
    const bool su = !(fabsf(uu) < kSatLogit), sw = !(fabsf(ww) < kSatLogit);
    const float Eu = su ? 0.0f : expf(-fabsf(uu)), Ew = sw ? 0.0f : expf(-fabsf(ww));
    const float ru = 1.0f / (1.0f + Eu), rw = 1.0f / (1.0f + Ew);
    const float Fu = uu < 0.0f ? Eu * ru : ru, Fw = ww < 0.0f ? Ew * rw : rw;
    const float fu = Eu * ru * ru, fw = Ew * rw * rw;  // F (1 - F)
    // (1 - 2F) = +-(1 - E) r
    const float mu = (uu < 0.0f ? 1.0f : -1.0f) * (1.0f - Eu) * ru;
    const float mw = (ww < 0.0f ? 1.0f : -1.0f) * (1.0f - Ew) * rw;
    P = Fu - Fw;
    const float p1 = -(fu - fw) * c.k1;
    P1 = mir ? -p1 : p1;
    P2 = (fu * mu - fw * mw) * (c.k1 * c.k1);
  } else {
    const bool su = !(fabsf(uu) < kSatProbit), sw = !(fabsf(ww) < kSatProbit);
    const float eu = su ? 0.0f : exp_neg_sq(uu), ew = sw ? 0.0f : exp_neg_sq(ww);
    // F(z) = 0.5 erfc(-z): the lower edge is a tail, the upper one at most 1
    P = 0.5f * erfcf(-uu) - 0.5f * erfcf(-ww);
    const float pu = eu * c.k1, pw = ew * c.k1;            // phi
    const float zu = su ? 0.0f : uu * pu, zw = sw ? 0.0f : ww * pw;  // z phi
    const float p1 = -(pu - pw);
    P1 = mir ? -p1 : p1;
    P2 = -(2.0f * zu - 2.0f * zw) * c.inv_a;
  }
}

// curvature of one entry's -log P in t (the map value); code in [0, nbins)
template <bool LOGIT, bool LOG, int KIND>
__host__ __device__ __forceinline__ float entry_curvature(float t, int code,
                                                          const float2* __restrict__ edges,
                                                          const Link& c) {
  float x = t, tinv2 = 1.0f;
  if (LOG) {
    const float tp = t + c.offset;
    x = logf(tp);
    const float ti = 1.0f / tp;
    tinv2 = ti * ti;
  }
  float h;
  if (KIND == INFO_OBSERVED) {
    const float2 e = edges[code];
    float P, P1, P2;
    bin_terms<LOGIT>(x, e.x, e.y, c, P, P1, P2);
    const float ip = 1.0f / P;
    const float gx = -P1 * ip;
    h = __builtin_fmaf(gx, gx, -P2 * ip);
    if (LOG) h -= gx;
    h = (P > 0.0f) ? h : 0.0f;
  } else {
    h = 0.0f;
    for (int b = 0; b < c.nbins; ++b) {
      const float2 e = edges[b];
      float P, P1, P2;
      bin_terms<LOGIT>(x, e.x, e.y, c, P, P1, P2);
      const float term = P1 * P1 / P;
      h += (P > 0.0f) ? term : 0.0f;
    }
  }
  return h * tinv2;
}

// ---- the per-entry terms of the Newton fits (qsc_newton.cuh: QSC_ENTRY_ACCUMULATE) ----
// One entry's fp32 f, g_t and h at t (qsc_newton.cuh's header); `use` is false for what adds 0 to
// g and J.
template <bool LOGIT, bool LOG, int KIND>
__device__ __forceinline__ void entry_terms(float t, int code, const float2* __restrict__ edges,
                                            const Link& c, float& fe, float& gt, float& h,
                                            bool& use, bool& neg) {
  float x = t, ti = 1.0f;
  neg = false;
  if (LOG) {
    const float tp = t + c.offset;
    neg = !(tp > 0.0f);
    x = logf(tp);
    ti = 1.0f / tp;
  }
  const float2 e = edges[code];
  float P, P1, P2;
  bin_terms<LOGIT>(x, e.x, e.y, c, P, P1, P2);
  const float ip = 1.0f / P;
  const float gx = -P1 * ip;
  fe = -logf(fmaxf(P, FLT_MIN));
  gt = gx * ti;
  if (KIND == INFO_OBSERVED) {
    // entry_curvature<..., INFO_OBSERVED>'s operations on the terms already at hand
    h = __builtin_fmaf(gx, gx, -P2 * ip);
    if (LOG) h -= gx;
    h *= ti * ti;
  } else {
    h = entry_curvature<LOGIT, LOG, INFO_EXPECTED>(t, code, edges, c);
  }
  use = (P > 0.0f) && !neg;
}

// F(z) - F(y), z >= y, of the link in fp64, both arguments in the lower half (z + y <= 0) so that
// neither value is near 1: probit F(z) = erfc(-z) / 2, logit F(z) = e^z / (1 + e^z).
template <bool LOGIT>
__device__ __forceinline__ double link_diff(double z, double y) {
  if (LOGIT) {
    const double Ez = exp(-fabs(z)), Ey = exp(-fabs(y));
    const double Fz = z < 0.0 ? Ez / (1.0 + Ez) : 1.0 / (1.0 + Ez);
    const double Fy = y < 0.0 ? Ey / (1.0 + Ey) : 1.0 / (1.0 + Ey);
    return Fz - Fy;
  }
  return 0.5 * erfc(-z) - 0.5 * erfc(-y);
}

// One entry's -log max(P, FLT_MIN) in fp64 at t (fp64, from the fp32 s and c_k): bin_terms' P
// (the same mirroring into the lower half; an infinite edge gives F = 0 or 1 by itself).
template <bool LOGIT, bool LOG>
__device__ __forceinline__ double entry_nll(double t, float2 e, const Link& c, double inv_a) {
  const double x = LOG ? log(t + (double)c.offset) : t;
  const double u = ((double)e.y - x) * inv_a, w = ((double)e.x - x) * inv_a;
  const bool mir = (u + w) > 0.0;
  const double P = link_diff<LOGIT>(mir ? -w : u, mir ? -u : w);
  return -log(fmax(P, (double)FLT_MIN));
}

// ---- the model's own parameters (qsc_qfit.hip): theta = (tau, beta), a -> a e^tau, every
// interior edge -> edge + beta ----
// The link at the trial scale: a = fp32(a0 e^tau), a0 the fp64 divisor of the packed model
// (probit sigma0 * 1.414213, logit s0) -- what make_link gives for sigma0 e^tau.
__host__ __device__ __forceinline__ Link calib_link(const Link& base, bool logit, double a0,
                                                    double tau) {
  Link l = base;
  l.a = (float)(a0 * exp(tau));
  l.inv_a = 1.0f / l.a;
  l.k1 = logit ? 1.0f / l.a : (float)(1.0 / ((double)l.a * 1.7724538509055160273));
  return l;
}

// Is the lower / upper edge of bin b shifted by beta?  The two clamp edges of the linear model
// (make_edges' -1e5, +1e5) are not; an infinite edge stays infinite under the addition.
__host__ __device__ __forceinline__ bool calib_lo_shifted(int b, bool log_model) {
  return log_model || b != 0;
}
__host__ __device__ __forceinline__ bool calib_hi_shifted(int b, int nbins, bool log_model) {
  return log_model || b != nbins - 1;
}
// bin b's edges at beta: fp32(edge + beta), the sum in fp64
__host__ __device__ __forceinline__ float2 calib_edges(float2 e, int b, int nbins, bool log_model,
                                                       double beta) {
  float2 r = e;
  if (calib_lo_shifted(b, log_model)) r.x = (float)((double)e.x + beta);
  if (calib_hi_shifted(b, nbins, log_model)) r.y = (float)((double)e.y + beta);
  return r;
}

// One edge at z = (edge - x) / a, in z-units: psi = F', z psi, psi', z psi' and z^2 psi'.  A
// saturated or infinite edge gives exactly 0 for all five (no product meets an infinity).
//   probit: psi = exp(-z^2) / sqrt(pi), psi' = -2 z psi;   logit: psi = F (1 - F), psi' = psi (1 - 2F)
template <bool LOGIT>
__host__ __device__ __forceinline__ void calib_edge_terms(float z, float& A, float& B, float& D,
                                                          float& zD, float& zzD) {
  const bool s = !(fabsf(z) < (LOGIT ? kSatLogit : kSatProbit));
  const float zs = s ? 0.0f : z;
  if (LOGIT) {
    const float E = s ? 0.0f : expf(-fabsf(zs));
    const float r = 1.0f / (1.0f + E);
    A = E * r * r;
    D = A * ((zs < 0.0f ? 1.0f : -1.0f) * (1.0f - E) * r);
  } else {
    A = s ? 0.0f : exp_neg_sq(zs) * 0.56418958354775628695f;
    D = -2.0f * (zs * A);
  }
  B = zs * A;
  zD = zs * D;
  zzD = zs * zD;
}

// One bin (lo, hi), already shifted, at x: P (bin_terms' value, the same operations), its first
// derivatives P1 = (P_tau, P_beta) and second P2 = (P_tt, P_tb, P_bb), from du/dtau = -u,
// du/dbeta = 1/a for a shifted edge and 0 for an unshifted one:
//   P_tau = -(u psi(u) - w psi(w))                 P_beta = (psi(u) - psi(w)) / a
//   P_tt  = (u psi + u^2 psi')(u) - (...)(w)       P_tb   = -((psi + u psi')(u) - (...)(w)) / a
//   P_bb  = (psi'(u) - psi'(w)) / a^2
template <bool LOGIT>
__host__ __device__ __forceinline__ void bin_calib(float x, float lo, float hi, bool slo, bool shi,
                                                   const Link& c, float& P, float (&P1)[2],
                                                   float (&P2)[3]) {
  float Px, Pxx;
  bin_terms<LOGIT>(x, lo, hi, c, P, Px, Pxx);
  const float u = div_link(hi - x, c), w = div_link(lo - x, c);
  float Au, Bu, Du, zDu, zzDu, Aw, Bw, Dw, zDw, zzDw;
  calib_edge_terms<LOGIT>(u, Au, Bu, Du, zDu, zzDu);
  calib_edge_terms<LOGIT>(w, Aw, Bw, Dw, zDw, zzDw);
  const float hu = shi ? 1.0f : 0.0f, hw = slo ? 1.0f : 0.0f;
  P1[0] = -(Bu - Bw);
  P1[1] = (hu * Au - hw * Aw) * c.inv_a;
  P2[0] = (Bu + zzDu) - (Bw + zzDw);
  P2[1] = -(hu * (Au + zDu) - hw * (Aw + zDw)) * c.inv_a;
  P2[2] = (hu * Du - hw * Dw) * (c.inv_a * c.inv_a);
}

// One entry's fp32 f = -log max(P, FLT_MIN), g = (f_tau, f_beta) and H = (f_tt, f_tb, f_bb) at
// the map value t, on the shifted edge table; `use` is false for what adds 0 to g and H.
//   g_i = -P_i / P;  observed H_ij = P_i P_j / P^2 - P_ij / P at the entry's code;
//   expected H_ij = sum_b P_i,b P_j,b / P_b over all bins, bins with P_b == 0 dropped (PSD)
template <bool LOGIT, bool LOG, int KIND>
__host__ __device__ __forceinline__ void entry_calib(float t, int code,
                                                     const float2* __restrict__ edges,
                                                     const Link& c, float& fe, float (&g)[2],
                                                     float (&H)[3], bool& use, bool& neg) {
  float x = t;
  neg = false;
  if (LOG) {
    const float tp = t + c.offset;
    neg = !(tp > 0.0f);
    x = logf(tp);
  }
  const float2 e = edges[code];
  float P, P1[2], P2[3];
  bin_calib<LOGIT>(x, e.x, e.y, calib_lo_shifted(code, LOG), calib_hi_shifted(code, c.nbins, LOG),
                   c, P, P1, P2);
  // (true divisions: with a denormal P the reciprocal is +inf and 0 * inf a NaN, 0 / P is 0)
  fe = -logf(fmaxf(P, FLT_MIN));
  g[0] = -P1[0] / P;
  g[1] = -P1[1] / P;
  if (KIND == INFO_OBSERVED) {
    H[0] = __builtin_fmaf(g[0], g[0], -P2[0] / P);
    H[1] = __builtin_fmaf(g[0], g[1], -P2[1] / P);
    H[2] = __builtin_fmaf(g[1], g[1], -P2[2] / P);
  } else {
    H[0] = H[1] = H[2] = 0.0f;
    for (int b = 0; b < c.nbins; ++b) {
      const float2 eb = edges[b];
      float Pb, Q1[2], Q2[3];
      bin_calib<LOGIT>(x, eb.x, eb.y, calib_lo_shifted(b, LOG), calib_hi_shifted(b, c.nbins, LOG),
                       c, Pb, Q1, Q2);
      const float qt = Q1[0] / Pb, qb = Q1[1] / Pb;
      const bool on = Pb > 0.0f;
      H[0] += on ? Q1[0] * qt : 0.0f;
      H[1] += on ? Q1[1] * qt : 0.0f;
      H[2] += on ? Q1[1] * qb : 0.0f;
    }
  }
  use = (P > 0.0f) && !neg;
}

// ... and its f in fp64 by QSC_ENTRY_ACCUMULATE's rule: entry_nll at the fp64 t, but for the
// fp32 P == 0 (FLT_MIN's term) and t + offset <= 0 (the caller makes the sum +inf)
template <bool LOGIT, bool LOG>
__device__ __forceinline__ double entry_calib_nll(float fe, bool neg, double t, float2 e,
                                                  const Link& c, double inv_a) {
  return (fe == -logf(FLT_MIN) || neg) ? (double)fe : entry_nll<LOGIT, LOG>(t, e, c, inv_a);
}

// upper-triangle index of (i, j), i <= j, of an N x N symmetric block
template <int N>
__host__ __device__ constexpr int tri(int i, int j) {
  return i * N - (i * (i - 1)) / 2 + (j - i);
}
// ... of (i, j) in either order
template <int N>
__host__ __device__ constexpr int sym(int i, int j) {
  return i <= j ? tri<N>(i, j) : tri<N>(j, i);
}

// pitch (floats) of the C^T table in LDS: a row is RP floats read as 16-byte vectors; the 4-float
// pad spreads rows over the banks as the passes' tables do
__host__ __device__ constexpr int info_pitch(int RP) { return RP > 4 ? RP + 4 : 4; }

inline size_t sinfo_lds(int K, int RP, int nbins) {
  return (size_t)K * info_pitch(RP) * 4 + (size_t)nbins * 8;
}

template <typename E>
struct Ent;
template <>
struct Ent<uint16_t> {
  static constexpr int kBits = 12;
  static constexpr uint32_t kPad = 15;
};
template <>
struct Ent<uint32_t> {
  static constexpr int kBits = 24;
  static constexpr uint32_t kPad = 255;
};

// decode one entry value into (k, code, pad); k and code are clamped into range, out-of-range
// values read as pads
template <typename E, bool SR>
__device__ __forceinline__ void decode(uint32_t v, int K, int Ko, int nbins, int& k, int& code,
                                       bool& pad) {
  if (SR) {
    code = (int)v >= Ko ? 1 : 0;
    k = (int)v - (code ? Ko : 0);
    pad = (int)v >= 2 * Ko || k >= K;
  } else {
    k = (int)(v & ((1u << Ent<E>::kBits) - 1u));
    code = (int)(v >> Ent<E>::kBits);
    pad = (uint32_t)code == Ent<E>::kPad || code >= nbins || k >= K;
  }
  k = pad ? 0 : k;
  code = pad ? 0 : code;
}

// the lane's two entries (2h, 2h + 1) of chunk `ch` of a slice; a read past the entry array is
// clamped and returned as pads
template <typename E>
__device__ __forceinline__ void load_pair(const E* __restrict__ ent, int64_t idx, int64_t n_ent,
                                          uint32_t pad_value, uint32_t& v0, uint32_t& v1) {
  const bool in = idx + 1 < n_ent;
  const int64_t i = in ? idx : 0;
  if (sizeof(E) == 2) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(ent + i);  // idx is even: 4-B aligned
    v0 = w & 0xFFFFu;
    v1 = w >> 16;
  } else {
    const uint2 w = *reinterpret_cast<const uint2*>(ent + i);
    v0 = w.x;
    v1 = w.y;
  }
  v0 = in ? v0 : pad_value;
  v1 = in ? v1 : pad_value;
}

inline bool info_model_ok(const qsc_model* m) {
  if (!m || m->nbounds < 2 || m->nbounds > QSC_MAX_BOUNDS || !(m->sigma > 0.0)) return false;
  if (m->loss != QSC_LOSS_PROBIT && m->loss != QSC_LOSS_LOGIT) return false;
  return true;
}

// the layout / model combinations the walk decodes (qsc_sinfo's checks)
inline bool info_layout_ok(const qsc_obs_desc* d, const qsc_model* m, int R) {
  if (R < 1 || R > QSC_MAX_R || d->K < 1 || d->P < 1 || d->Pp < d->P || (d->Pp % 64) != 0 ||
      d->nbins != m->nbounds - 1 || d->s_entries < 0)
    return false;
  if (d->rowfmt != 0 && d->rowfmt != 1) return false;
  // signed rows: the one-bit layout, narrow entries, every row index representable
  if (d->rowfmt == 1 && (d->wide || d->nbins != 2 || (int64_t)sr_rows(d->K) > 0x10000))
    return false;
  if (!d->wide && d->rowfmt == 0 && (d->K > 4096 || d->nbins > 15)) return false;
  if (d->wide && d->K > (1 << 24)) return false;
  if (d->rowfmt == 1 && m->log_model) return false;
  return true;
}

}  // namespace

// dispatch over (link, log model, kind) for APPLY(LAUNCH, LOGIT, LOG, KIND); reads m and kind
#define QSC_INFO_DISPATCH_(APPLY, LAUNCH)                                \
  do {                                                                   \
    const bool lg_ = m->loss == QSC_LOSS_LOGIT, lo_ = m->log_model != 0; \
    if (kind == INFO_OBSERVED) {                                         \
      if (lg_ && lo_) APPLY(LAUNCH, true, true, INFO_OBSERVED);          \
      else if (lg_) APPLY(LAUNCH, true, false, INFO_OBSERVED);           \
      else if (lo_) APPLY(LAUNCH, false, true, INFO_OBSERVED);           \
      else APPLY(LAUNCH, false, false, INFO_OBSERVED);                   \
    } else {                                                             \
      if (lg_ && lo_) APPLY(LAUNCH, true, true, INFO_EXPECTED);          \
      else if (lg_) APPLY(LAUNCH, true, false, INFO_EXPECTED);           \
      else if (lo_) APPLY(LAUNCH, false, true, INFO_EXPECTED);           \
      else APPLY(LAUNCH, false, false, INFO_EXPECTED);                   \
    }                                                                    \
  } while (0)
#define QSC_INFO_APPLY_(LAUNCH, LGT, LOGV, KD) LAUNCH(LGT, LOGV, KD)
// ... for LAUNCH(LOGIT, LOG, KIND)
#define QSC_INFO_DISPATCH(LAUNCH) QSC_INFO_DISPATCH_(QSC_INFO_APPLY_, LAUNCH)

// dispatch over the rank pad 4 / 8 / 16 for LAUNCH(RP, the further arguments); reads RP
#define QSC_RP_DISPATCH(LAUNCH, ...)              \
  do {                                            \
    if (RP == 4) LAUNCH(4, ##__VA_ARGS__);        \
    else if (RP == 8) LAUNCH(8, ##__VA_ARGS__);   \
    else LAUNCH(16, ##__VA_ARGS__);               \
  } while (0)

// ... and over the layout for LAUNCH(RP, E, SR, LOGIT, LOG, KIND): the rank pad, narrow / wide /
// signed-row entries (signed rows: linear one-bit only); reads RP and d as well
#define QSC_LAYOUT_E_(RPV, LAUNCH, LGT, LOGV, KD)                    \
  do {                                                               \
    if (d->rowfmt == 1) {                                            \
      if (!LOGV) LAUNCH(RPV, uint16_t, true, LGT, false, KD);        \
    } else if (d->wide) LAUNCH(RPV, uint32_t, false, LGT, LOGV, KD); \
    else LAUNCH(RPV, uint16_t, false, LGT, LOGV, KD);                \
  } while (0)
#define QSC_LAYOUT_RP_(LAUNCH, LGT, LOGV, KD) QSC_RP_DISPATCH(QSC_LAYOUT_E_, LAUNCH, LGT, LOGV, KD)
#define QSC_LAYOUT_DISPATCH(LAUNCH) QSC_INFO_DISPATCH_(QSC_LAYOUT_RP_, LAUNCH)
