// qsc_newton.cuh — what the kernels over the packed lists share: the Newton fits qsc_sfit.hip
// (per-pixel fit of S), qsc_sfit_smooth.hip (the same under the smoothness prior), qsc_cfit.hip
// (per-bin fit of C) and qsc_qfit.hip (the model's own parameters), and the estimators that walk
// the same lists or factor the same blocks: qsc_info.hip, qsc_check.hip, qsc_design.hip.  Each
// rule below is stated here once; the tests pin every one of them to the bit.
//
// The objective.  One row x (a position's s, or a bin's c) minimises
//     f(x) = sum_{entries} -log max(P(code | t = x . y), FLT_MIN) + ridge / 2 |x|^2
// with y the table row of the entry (c_k, or s_q) and P, the edges, the log-model chain
// x = log(t + offset) and the saturation rules of qsc_info.cuh.  Per entry, with g_x = -P'/P
// (QSC_ENTRY_ACCUMULATE):
//     f += -log max(P, FLT_MIN)     fp64 (entry_nll: t, the link and the logarithm from the fp32
//                                   x, y and edges)
//     g += g_t y,                   g_t = g_x (linear) or g_x / (t + offset) (log model)
//     J += h y y^T,                 h = entry_curvature's value: QSC_INFO_OBSERVED (Newton) or
//                                   QSC_INFO_EXPECTED (Fisher scoring, J >= 0); g and J fp32
// A pad entry adds exactly 0 to all three; an entry whose fp32 P is 0 adds 0 to g and J and the
// fp32 -log FLT_MIN to f; in the log model an entry with t + offset <= 0 makes f = +inf.
// f is fp64 because the accept test compares two values that differ, near the minimiser, by
// g . delta ~ |g|^2 / lambda: with fp32 terms (each -log P good to ~2e-7, t rounded to 1e-7) a
// decrease below ~1e-6 is invisible, true Newton steps are rejected, and the iteration stops
// |g| ~ sqrt(1e-6 lambda) short -- 1e-3 to 1e-2 relative at ridge 1e-2, measured.
//
// The S-format walk (QSC_SLICE_LISTS, QSC_WALK_BEGIN ... QSC_WALK_END: sinfo_kernel,
// scheck_kernel, qfit_walk_kernel and, through QSC_WALK_SLICE, sfit_kernel and
// sfit_smooth_kernel).  One wave per slice of QSC_SLICE positions, grid-stride over the slices,
// two lanes per position; lane half h takes entries 2h, 2h + 1 of every 4-entry chunk in list
// order; C^T and the edges sit in LDS at the info_pitch pitch; the next chunk's entries are loaded
// while this one is worked, with clamped reads.  Three things hold for every user: no read leaves
// the entry array (load_pair); a pad entry adds exactly 0 to every sum (its terms are replaced
// by 0 with a select, and the row it reads, row 0, is finite); the entry order, and with it every sum, is fixed by the packing
// alone.  The halves are added once with a lane swap (a + b is the same bits on both lanes), so
// from there on both lanes of a position hold the same state and take the same decisions.  No
// floating-point atomics.
//
// The block update (QSC_BLOCK_UPDATE: sinfo_kernel, sgain_kernel, scheck_kernel and
// QSC_ENTRY_ACCUMULATE).  J += h y y^T on the packed upper triangle: J[tri(i, j)] += (h y[i]) y[j],
// i <= j, the product h y[i] rounded first, then one fma per element.
//
// The iteration, the same structure for every row:
//     evaluate (f, g, J) at x = x_init;  mu = mu0
//     repeat up to max_steps times:
//         Cholesky of J + (ridge + mu) I (held rows the identity), delta from g + ridge x
//         x' = x - delta;  project: x' = max(x', 0)
//         a pivot that is not positive: the step counts as rejected (x' = x is walked)
//         (f', g', J') at x'
//         accept iff f' <= f and f' is finite (QSC_NEWTON_ACCEPT): x, (f, g, J) <- x', (f', g', J'),
//             mu <- max(mu / 10, mu0 == 0 ? 0 : kMuMin)
//         else mu <- max(10 mu, kMuMin)                                         (QSC_MU_*)   
//         converged once an accepted step has |x' - x|_inf <= tol (1 + |x|_inf)
//
// Identification (QSC_CHOL_SOLVE).  A pivot p of J + (ridge + mu) I with p <= mu says that
// J + ridge I itself has no positive pivot there (for a positive semidefinite J + ridge I every
// pivot of the damped matrix is mu plus a non-negative Schur complement).  A row whose
// factorisation had such a pivot at every step -- no observations and ridge = 0, say -- is
// unidentified: it is counted, and what it returns is x_init moved by steps that only the damping
// defined (for the empty row: x_init itself, g = 0).  With mu = 0 this is the plain pivot test.
//
// The workspace row.  The state before a trial, (f, g, J), is kept across the trial walk: for
// RP 4 and 8 in a second register set, replaced by a per-lane select on acceptance (no
// private-memory scratch).  For RP 16 two sets of 136 + 16 values and the factor do not fit the
// 512 registers of a lane (the compiler spilled 8 to 24 bytes per lane), so there (newton_in_ws)
// the accepted (g, J) live in a workspace row of the lane's own: RP + NT contiguous floats moved as
// 16-byte vectors, so that every access is the row's address plus an immediate; written on
// acceptance only, read back by the same lane for the factorisation; the registers hold one set.
//
// Form.  The host side is ordinary functions.  The device side is statement macros, not
// force-inlined functions: the RP 8 and RP 16 kernels sit at register and occupancy limits, and
// with functions the same arithmetic came out of the compiler with other register counts in 124
// of the 255 kernels of the four files, twice at the cost of a wave of occupancy (DESIGN.md
// section 7o).  A macro expands to the statements the kernels used to carry, so every kernel's
// machine code is what its open-coded body gave (profiles/newton_shared/isa_compare.txt and, for
// the walk, the block update and the element-wise skeleton, profiles/walk_shared/), and a rule
// still has one home.  Each macro's comment lists what it declares in the caller's scope
// and what it reads from it; names ending in an underscore are the macros' own.
#pragma once
#include <algorithm>

#include "qsc_info.cuh"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// the smallest non-zero damping: what a rejected step raises mu to from 0, and the floor of the
// mu / 10 schedule when mu0 > 0
constexpr float kMuMin = 1.0e-6f;

__host__ __device__ constexpr int tri_count(int RP) { return RP * (RP + 1) / 2; }

// ranks whose accepted (g, J) are kept in the workspace instead of a second register set
__host__ __device__ constexpr bool newton_in_ws(int RP) { return RP > 8; }

// the grid of a walk over the slices (grid-stride: any grid gives the same bits): enough
// workgroups to fill the device, few enough that the C^T staging stays a small part of the traffic
inline int64_t slice_grid(int nslices, int per_cu) {
  return std::min<int64_t>(ceil_div(nslices, kWaves), (int64_t)cu_count() * per_cu);
}
// ... of a fit: with the workspace (one row per lane of the grid) only twice the workgroups that
// are resident at the one wave per SIMD the RP 16 kernels run at
inline int64_t newton_grid(int nslices, int RP) {
  return slice_grid(nslices, newton_in_ws(RP) ? 2 : 8);
}
inline size_t newton_ws_bytes(const qsc_obs_desc* d, int R) {
  if (!d || R < 1 || R > QSC_MAX_R || d->Pp < 1) return 0;
  const int RP = qsc_rank_pad(R);
  if (!newton_in_ws(RP)) return 0;  // (the state before a trial step stays in registers)
  return (size_t)newton_grid(d->Pp / QSC_SLICE, RP) * kWaves * 64 * (RP + tri_count(RP)) *
         sizeof(float);
}
inline bool newton_args_ok(int kind, float ridge, float mu0, float tol, int steps) {
  return (kind == INFO_EXPECTED || kind == INFO_OBSERVED) && ridge >= 0.0f && mu0 >= 0.0f &&
         tol > 0.0f && steps >= 1;
}

// what a launch of a walk over the slices takes besides its own arguments
struct WalkLaunch {
  int RP;
  size_t shm;  // C^T, the edges and `extra_lds` bytes of the caller's own
  Link lk;
  Edges E;
  int nslices;
};
// ... filled for K bins and Pp positions; QSC_EUNSUPPORTED when the tables do not fit the LDS.
// The caller's last check: every argument is valid by then (m: info_model_ok).
inline int walk_launch(int K, int Pp, const qsc_model* m, int R, size_t extra_lds, WalkLaunch* wl) {
  wl->RP = qsc_rank_pad(R);
  wl->shm = sinfo_lds(K, wl->RP, m->nbounds - 1) + extra_lds;
  if (wl->shm > kInfoLdsMax) return QSC_EUNSUPPORTED;
  wl->lk = make_link(m);
  make_edges(m, &wl->E);
  wl->nslices = Pp / QSC_SLICE;
  return QSC_OK;
}
// ... for a packed layout (info_layout_ok: d->nbins is the model's)
inline int walk_launch(const qsc_obs_desc* d, const qsc_model* m, int R, WalkLaunch* wl) {
  return walk_launch(d->K, d->Pp, m, R, 0, wl);
}

// the element-wise calls (qsc_entry_*): their argument check and their grid (grid-stride)
inline bool entry_args_ok(const qsc_model* m, int64_t n, const void* Y, const void* T,
                          const void* out) {
  return info_model_ok(m) && n >= 0 && (n == 0 || (Y && T && out));
}
inline dim3 entry_grid(int64_t n) {
  return dim3((unsigned)std::min<int64_t>(ceil_div(n, kBlock), 8192));
}

// QSC_CHOL_SOLVE's rules for a 2 x 2 system in fp64 (qsc_qfit.hip): Cholesky of the damped
// a = (a00, a01, a11) with a held row the identity, then delta from rhs.  ok: every pivot of a free
// row was positive (a failed pivot, also of a NaN block, is replaced by 1); idn: every one
// exceeded mu.
__device__ __forceinline__ void chol2_solve_f64(const double (&a)[3], const bool (&free_)[2],
                                                double mu, const double (&rhs)[2],
                                                double (&delta)[2], bool& ok, bool& idn) {
  ok = true;
  idn = true;
  double p0 = a[0];
  if (free_[0]) {
    idn = idn && (p0 > mu);
    if (!(p0 > 0.0)) {
      ok = false;
      p0 = 1.0;
    }
  }
  const double l10 = a[1] / p0;  // (L[1][0] / L[0][0]: the LDL^T form of the same pivots)
  double p1 = a[2] - l10 * a[1];
  if (free_[1]) {
    idn = idn && (p1 > mu);
    if (!(p1 > 0.0)) {
      ok = false;
      p1 = 1.0;
    }
  }
  const double y1 = rhs[1] - l10 * rhs[0];
  delta[1] = y1 / p1;
  delta[0] = rhs[0] / p0 - l10 * delta[1];
}

}  // namespace

// ---- rows of N floats (N a multiple of 4) as 16-byte vectors ----
// declares `const float xs[4]`: the vector at ptr
#define QSC_VEC4(xs, ptr)                                             \
  const float4 xs##v_ = *reinterpret_cast<const float4*>(ptr);        \
  const float xs[4] = {xs##v_.x, xs##v_.y, xs##v_.z, xs##v_.w}
#define QSC_ROW_LOAD(N, dst, ptr)                                           \
  _Pragma("unroll") for (int r_ = 0; r_ < (N); r_ += 4) {                   \
    const float4 x_ = *reinterpret_cast<const float4*>((ptr) + r_);         \
    (dst)[r_] = x_.x;                                                       \
    (dst)[r_ + 1] = x_.y;                                                   \
    (dst)[r_ + 2] = x_.z;                                                   \
    (dst)[r_ + 3] = x_.w;                                                   \
  }
// dst[r] = row[r] for r < R of a live row, else 0
#define QSC_ROW_LOAD_MASKED(N, dst, ptr, live, R)                           \
  _Pragma("unroll") for (int r_ = 0; r_ < (N); r_ += 4) {                   \
    QSC_VEC4(xs_, (ptr) + r_);                                              \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_)                        \
        (dst)[r_ + e_] = ((live) && r_ + e_ < (R)) ? xs_[e_] : 0.0f;        \
  }
#define QSC_ROW_STORE(N, ptr, src)                                          \
  _Pragma("unroll") for (int r_ = 0; r_ < (N); r_ += 4)                     \
      *reinterpret_cast<float4*>((ptr) + r_) =                              \
          make_float4((src)[r_], (src)[r_ + 1], (src)[r_ + 2], (src)[r_ + 3])

// ---- staging and lane geometry of the S-format walk ----
// declares smem, Cl ([K][CP], rows >= R zero) and El ([nbins]); ends with the workgroup barrier
#define QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_)                                          \
  extern __shared__ __attribute__((aligned(16))) float smem[];                            \
  float* Cl = smem;                                                                       \
  float2* El = reinterpret_cast<float2*>(Cl + (size_t)(K) * (CP));                        \
  for (int i_ = threadIdx.x; i_ < (K) * (RP); i_ += kBlock) {                             \
    const int k_ = i_ / (RP), r_ = i_ - k_ * (RP);                                        \
    Cl[k_ * (CP) + r_] = r_ < (R) ? (C)[(int64_t)r_ * (K) + k_] : 0.0f;                   \
  }                                                                                       \
  for (int b_ = threadIdx.x; b_ < (lk).nbins; b_ += kBlock) El[b_] = (E_).e[b_];          \
  __syncthreads()
// declares wave, lane, l, h (lane l + 32 h: half h of position l of the wave's slice)
#define QSC_SLANE_GEOMETRY()                                                              \
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;                             \
  const int l = lane & (QSC_SLICE - 1), h = lane >> 5
// declares Ko and pad_value: what a clamped read of the lists returns
#define QSC_SLANE_PAD(E, SR, K)                                                           \
  const int Ko = sr_off(K);                                                               \
  const uint32_t pad_value = SR ? 2u * (uint32_t)Ko : (Ent<E>::kPad << Ent<E>::kBits)
// ... both
#define QSC_SLANE(E, SR, K) \
  QSC_SLANE_GEOMETRY();     \
  QSC_SLANE_PAD(E, SR, K)

// ---- the lists of slice s ----
// declares nch (4-entry chunks of every list of the slice) and base (the lane's first pair);
// reads width, off, l, h
#define QSC_SLICE_LISTS(s)         \
  const int nch = width[s] >> 2;   \
  const int64_t base = off[s] + l * 4 + 2 * h

// ---- the walk over the lane's entries of a slice, in list order ----
// Between QSC_WALK_BEGIN and QSC_WALK_END stand the statements for one entry.  Declares for them
// k, code, pad (decode's: clamped into range, a pad reads as k = code = 0), cv[RP] (the C^T row of
// bin k: finite, so a pad's terms can be selected to exactly 0) and t = x . cv in fp32, r
// ascending; reads ent, base, n_ent, nch, pad_value, K, Ko, lk, Cl.
// The next chunk's pair is loaded while this one is worked.  Past the last list that read meets
// the next slice's entries or the array's pad tail (QSC_ENTRY_TAIL) and is never used; load_pair
// clamps it either way, so no read leaves the array.
#define QSC_WALK_BEGIN(RP, CP, E, SR, x)                                                   \
  {                                                                                        \
    uint32_t n0_, n1_;                                                                     \
    load_pair<E>(ent, base, n_ent, pad_value, n0_, n1_);                                   \
    for (int ch_ = 0; ch_ < nch; ++ch_) {                                                  \
      const uint32_t v_[2] = {n0_, n1_};                                                   \
      load_pair<E>(ent, base + (int64_t)(ch_ + 1) * (QSC_SLICE * 4), n_ent, pad_value, n0_, n1_); \
      _Pragma("unroll") for (int e_ = 0; e_ < 2; ++e_) {                                   \
        int k, code;                                                                       \
        bool pad;                                                                          \
        decode<E, SR>(v_[e_], K, Ko, lk.nbins, k, code, pad);                              \
        float cv[RP];                                                                      \
        QSC_ROW_LOAD(RP, cv, Cl + k * (CP))                                                \
        float t = 0.0f;                                                                    \
        _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_) t = __builtin_fmaf((x)[r_], cv[r_], t);
#define QSC_WALK_END \
      }              \
    }                \
  }

// ---- the block update J += hh y y^T on the packed upper triangle of the first N rows ----
// J[tri(i, j)] += (hh y[i]) y[j] for i <= j < N: the product hh y[i] first, then the fma, rows
// and columns ascending.  ROW: statements in i_ that a caller's own row sums run first in row i_
// (may be empty).
#define QSC_BLOCK_UPDATE(RP, N, J, hh, y, ROW)                                             \
  _Pragma("unroll") for (int i_ = 0; i_ < (N); ++i_) {                                     \
    ROW                                                                                    \
    const float hi_ = (hh) * (y)[i_];                                                      \
    _Pragma("unroll") for (int j_ = i_; j_ < (N); ++j_)                                    \
        (J)[tri<RP>(i_, j_)] = __builtin_fmaf(hi_, (y)[j_], (J)[tri<RP>(i_, j_)]);         \
  }

// ---- the element-wise kernels (qsc_entry_*): a walk's device functions on n given (code, t) ----
// declares se[], the edge table in LDS (EDGE: the edges of bin b_, an expression in b_); ends
// with the workgroup barrier
#define QSC_ENTRYWISE_STAGE(lk, EDGE)                                                      \
  __shared__ float2 se[QSC_MAX_BOUNDS - 1];                                                \
  for (int b_ = threadIdx.x; b_ < (lk).nbins; b_ += blockDim.x) se[b_] = (EDGE);           \
  __syncthreads()
// Between QSC_ENTRYWISE_BEGIN and QSC_ENTRYWISE_END stand the statements for element i of the
// grid-stride loop.  Declares i and y (the code Y[i] clamped into [0, nbins)); reads Y, n.
#define QSC_ENTRYWISE_BEGIN(lk)                                                            \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;                  \
       i += (int64_t)gridDim.x * blockDim.x) {                                             \
    int64_t y = Y[i];                                                                      \
    y = y < 0 ? 0 : (y >= (lk).nbins ? (lk).nbins - 1 : y);
#define QSC_ENTRYWISE_END }

// ---- one entry: its terms at t = x . y added to (ft, neg, gt, Jt) ----
#define QSC_ENTRY_ACCUMULATE(RP, LOGIT, LOG, KIND, x, y, code, pad, El, lk, inv_a, ft, neg, gt, Jt) \
  {                                                                                        \
    float t_ = 0.0f;                                                                       \
    _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_) t_ = __builtin_fmaf((x)[r_], (y)[r_], t_); \
    double td_ = 0.0;                                                                      \
    _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_)                                    \
        td_ = __builtin_fma((double)(x)[r_], (double)(y)[r_], td_);                        \
    float fe, ge_, hh_;                                                                    \
    bool use_, eneg_;                                                                      \
    entry_terms<LOGIT, LOG, KIND>(t_, code, El, lk, fe, ge_, hh_, use_, eneg_);            \
    /* the fp32 P == 0 (FLT_MIN's term) and t + offset <= 0 (f = +inf) keep their rule */  \
    const double fd_ = (fe == -logf(FLT_MIN) || eneg_)                                     \
                           ? (double)fe                                                    \
                           : entry_nll<LOGIT, LOG>(td_, (El)[code], lk, inv_a);            \
    /* a pad adds exactly 0 (y is finite) */                                               \
    use_ = use_ && !(pad);                                                                 \
    ft += (pad) ? 0.0 : fd_;                                                               \
    neg = neg || (eneg_ && !(pad));                                                        \
    ge_ = use_ ? ge_ : 0.0f;                                                               \
    hh_ = use_ ? hh_ : 0.0f;                                                               \
    QSC_BLOCK_UPDATE(RP, RP, Jt, hh_, y, (gt)[i_] = __builtin_fmaf(ge_, (y)[i_], (gt)[i_]);) \
  }

// ---- the walk of one slice at st: the halves summed, the ridge term added ----
// declares ft (fp64), gt[RP], Jt[NT] and neg (some entry had t + offset <= 0: the caller makes ft
// +inf once it has added what else belongs to its objective); reads ent, base, n_ent, nch,
// pad_value, K, Ko, lk, Cl, El, inv_a
#define QSC_WALK_SLICE(RP, NT, CP, E, SR, LOGIT, LOG, KIND, st, ridge)                     \
  double ft = 0.0;                                                                         \
  float gt[RP], Jt[NT];                                                                    \
  bool neg = false;                                                                        \
  _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_) gt[r_] = 0.0f;                       \
  _Pragma("unroll") for (int i_ = 0; i_ < (NT); ++i_) Jt[i_] = 0.0f;                       \
  QSC_WALK_BEGIN(RP, CP, E, SR, st)                                                        \
  (void)t; /* (the entry's own t_ is the same sum) */                                      \
  QSC_ENTRY_ACCUMULATE(RP, LOGIT, LOG, KIND, st, cv, code, pad, El, lk, inv_a, ft, neg, gt, Jt) \
  QSC_WALK_END                                                                             \
  /* the two halves' partial sums: the same bits on both lanes from here on */             \
  ft += __shfl_xor(ft, 32, 64);                                                            \
  neg = neg || (__shfl_xor((int)neg, 32, 64) != 0);                                        \
  _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_) gt[r_] += __shfl_xor(gt[r_], 32, 64); \
  _Pragma("unroll") for (int i_ = 0; i_ < (NT); ++i_) Jt[i_] += __shfl_xor(Jt[i_], 32, 64); \
  double nsq_ = 0.0;                                                                       \
  _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_)                                      \
      nsq_ = __builtin_fma((double)(st)[r_], (double)(st)[r_], nsq_);                      \
  ft += 0.5 * (double)(ridge) * nsq_

// ---- accept / reject of the trial xt against the accepted (xc, fc), and the mu schedule ----
// declares acc, conv (and dmax, smax)
#define QSC_NEWTON_ACCEPT(RP, first, step_ok, ft, fc, xt, xc, tol)                         \
  const bool acc = (first) || ((step_ok) && (ft) <= (fc) && fabs(ft) < (double)__builtin_inff()); \
  float dmax = 0.0f, smax = 0.0f;                                                          \
  _Pragma("unroll") for (int r_ = 0; r_ < (RP); ++r_) {                                    \
    dmax = fmaxf(dmax, fabsf((xt)[r_] - (xc)[r_]));                                        \
    smax = fmaxf(smax, fabsf((xc)[r_]));                                                   \
  }                                                                                        \
  const bool conv = !(first) && acc && dmax <= (tol) * (1.0f + smax)
#define QSC_MU_FLOOR(mu0) ((mu0) == 0.0f ? 0.0f : kMuMin)
#define QSC_MU_ACCEPTED(mu, first, mu_floor) \
  if (!(first)) mu = fmaxf(mu / 10.0f, mu_floor)
#define QSC_MU_REJECTED(mu) mu = fmaxf(10.0f * mu, kMuMin)

// ---- Cholesky of the packed upper triangle a (already damped: lower triangle a[i][j], j <= i,
// at tri(j, i); a held row is the identity), then L y = RHS, L^T delta = y (delta in y) ----
// FREE: is row j_ free (an expression in j_); RHS: the right-hand side of row i_ (in i_).
// declares dinv, y, ok (every pivot of a free row was positive; a failed pivot, also of a NaN
// block, is replaced by 1) and idn (every one exceeded mu)
#define QSC_CHOL_SOLVE(RP, a, mu, FREE, RHS)                                               \
  float dinv[RP], y[RP];                                                                   \
  bool ok = true, idn = true;                                                              \
  _Pragma("unroll") for (int j_ = 0; j_ < (RP); ++j_) {                                    \
    float piv = (a)[tri<RP>(j_, j_)];                                                      \
    _Pragma("unroll") for (int k_ = 0; k_ < j_; ++k_)                                      \
        piv = __builtin_fmaf(-(a)[tri<RP>(k_, j_)], (a)[tri<RP>(k_, j_)], piv);            \
    if (FREE) {                                                                            \
      idn = idn && (piv > mu);                                                             \
      if (!(piv > 0.0f)) {                                                                 \
        ok = false;                                                                        \
        piv = 1.0f;                                                                        \
      }                                                                                    \
    }                                                                                      \
    const float d_ = sqrtf(piv);                                                           \
    dinv[j_] = 1.0f / d_;                                                                  \
    _Pragma("unroll") for (int i_ = j_ + 1; i_ < (RP); ++i_) {                             \
      float v_ = (a)[tri<RP>(j_, i_)];                                                     \
      _Pragma("unroll") for (int k_ = 0; k_ < j_; ++k_)                                    \
          v_ = __builtin_fmaf(-(a)[tri<RP>(k_, i_)], (a)[tri<RP>(k_, j_)], v_);            \
      (a)[tri<RP>(j_, i_)] = v_ * dinv[j_];                                                \
    }                                                                                      \
  }                                                                                        \
  _Pragma("unroll") for (int i_ = 0; i_ < (RP); ++i_) {                                    \
    float v_ = RHS;                                                                        \
    _Pragma("unroll") for (int k_ = 0; k_ < i_; ++k_)                                      \
        v_ = __builtin_fmaf(-(a)[tri<RP>(k_, i_)], y[k_], v_);                             \
    y[i_] = v_ * dinv[i_];                                                                 \
  }                                                                                        \
  _Pragma("unroll") for (int i_ = (RP)-1; i_ >= 0; --i_) {                                 \
    float v_ = y[i_];                                                                      \
    _Pragma("unroll") for (int k_ = i_ + 1; k_ < (RP); ++k_)                               \
        v_ = __builtin_fmaf(-(a)[tri<RP>(i_, k_)], y[k_], v_);                             \
    y[i_] = v_ * dinv[i_];                                                                 \
  }

// ---- Cholesky of a (as above, rows already set), then M = L^-1 in place: M[j][j] = 1 / L[j][j],
// M[i][j] = -(sum_{k = j}^{i-1} L[i][k] M[k][j]) / L[i][i] (columns > j still hold L) ----
// fills dinv (1 / L[i][i]); sets bad on a pivot that is not positive (also a NaN block).
// diag(A^-1)[j] is then sum_{i >= j} M[i][j]^2.
#define QSC_CHOL_INVERSE(RP, a, dinv, bad)                                                 \
  _Pragma("unroll") for (int j_ = 0; j_ < (RP); ++j_) {                                    \
    float piv_ = (a)[tri<RP>(j_, j_)];                                                     \
    _Pragma("unroll") for (int k_ = 0; k_ < j_; ++k_)                                      \
        piv_ = __builtin_fmaf(-(a)[tri<RP>(k_, j_)], (a)[tri<RP>(k_, j_)], piv_);          \
    if (!(piv_ > 0.0f)) {                                                                  \
      bad = true;                                                                          \
      piv_ = 1.0f;                                                                         \
    }                                                                                      \
    const float d_ = sqrtf(piv_);                                                          \
    (dinv)[j_] = 1.0f / d_;                                                                \
    (a)[tri<RP>(j_, j_)] = d_;                                                             \
    _Pragma("unroll") for (int i_ = j_ + 1; i_ < (RP); ++i_) {                             \
      float v_ = (a)[tri<RP>(j_, i_)];                                                     \
      _Pragma("unroll") for (int k_ = 0; k_ < j_; ++k_)                                    \
          v_ = __builtin_fmaf(-(a)[tri<RP>(k_, i_)], (a)[tri<RP>(k_, j_)], v_);            \
      (a)[tri<RP>(j_, i_)] = v_ * (dinv)[j_];                                              \
    }                                                                                      \
  }                                                                                        \
  _Pragma("unroll") for (int j_ = 0; j_ < (RP); ++j_) {                                    \
    (a)[tri<RP>(j_, j_)] = (dinv)[j_];                                                     \
    _Pragma("unroll") for (int i_ = j_ + 1; i_ < (RP); ++i_) {                             \
      float v_ = 0.0f;                                                                     \
      _Pragma("unroll") for (int k_ = j_; k_ < i_; ++k_)                                   \
          v_ = __builtin_fmaf((a)[tri<RP>(k_, i_)], (a)[tri<RP>(j_, k_)], v_);             \
      (a)[tri<RP>(j_, i_)] = -v_ * (dinv)[i_];                                             \
    }                                                                                      \
  }

// ---- the workspace row of the calling lane: g first, then the triangle of J ----
#define QSC_WS_ROW(ws, wave, lane, RP, NT) \
  ((ws) + ((size_t)(blockIdx.x * kWaves + (wave)) * 64 + (lane)) * ((RP) + (NT)))
#define QSC_WS_PUT(RP, NT, wrow, g, J) \
  QSC_ROW_STORE(RP, wrow, g);          \
  QSC_ROW_STORE(NT, (wrow) + (RP), J)
