// qsc_qfit.hip — Newton / Fisher-scoring fit of the observation model's own parameters for known
// S and C: the noise scale and a common shift of the quantiser's levels (include/qsc.h:
// qsc_qfit_workspace_bytes, qsc_qfit_begin, qsc_qfit_iterate, qsc_qfit_finish, qsc_entry_calib).
//
// theta = (tau, beta): sigma = sigma0 e^tau (through the link's divisor a = fp32(a0 e^tau)) and
// every interior, finite edge b_i + beta (qsc_info.cuh: calib_link, calib_edges; the two clamp
// edges of the linear model stay).  Given S and C,
//     F(theta) = sum_{entries} -log max(P(code | x; a, edges), FLT_MIN)
//                + prior_scale / 2 tau^2 + prior_shift / 2 beta^2
// with x = t or log(t + offset), t = S[q] . c_k, and P bin_terms' value.  Per entry (entry_calib,
// bin_calib in qsc_info.cuh), with u = (hi - x) / a, w = (lo - x) / a on the shifted edges and psi
// the link's density in z-units, du/dtau = -u, du/dbeta = 1 / a:
//     P_tau = -(u psi(u) - w psi(w)),   P_beta = (psi(u) - psi(w)) / a,   g_i = -P_i / P
//     observed H_ij = P_i P_j / P^2 - P_ij / P;   expected H_ij = sum_b P_i,b P_j,b / P_b  (PSD)
// A saturated or infinite edge contributes exactly 0; an unshifted edge has no beta derivative;
// an entry with fp32 P == 0 adds 0 to g and H and -log FLT_MIN to f; t + offset <= 0 in the log
// model makes F = +inf; a pad adds exactly 0.
//
// qfit_walk_kernel: qsc_sinfo's walk (qsc_newton.cuh: one wave per slice, grid-stride, two lanes
// per position, C^T and the edges in LDS).  The trial theta is read from the device-resident
// state at kernel start; the kernel forms its Link and its shifted edge table from it, so a whole
// fit is stream-ordered.  Per entry f is fp64 (entry_nll's way, from the fp32 operands), g[2] and
// H[3] fp32; every lane adds them in fp64 in list order; the two halves of a position are added
// with the lane swap (xor 32), then the 32 positions of the slice with the butterfly xor 16, 8, 4,
// 2, 1 (a + b is the same bits on both lanes, so every lane ends with the same six sums); lane 0
// writes the slice's partial of 6 doubles.  One partial per slice, whatever the grid.
//
// qfit_step_kernel: one workgroup.  Thread i adds the partials of slices i, i + 256, i + 512, ...
// in ascending order; the 256 thread sums are then folded in LDS, thread i += thread i + w for
// w = 128, 64, ..., 1: an order that depends on the number of slices only.  Thread 0 adds the
// prior, accepts or rejects the walked trial (QSC_NEWTON_ACCEPT, QSC_MU_*), solves the damped
//     (H + diag(prior) + mu I) delta = g + prior * theta
// in fp64 with the parameters outside fit_mask as identity rows (qsc_cfit's held set; a pivot
// <= mu counts as unidentified by QSC_CHOL_SOLVE's rule: chol2_solve_f64) and writes the next
// trial.  No floating-point atomics anywhere: two runs agree bit for bit on any grid.
//
//     begin:    state <- (tau0, beta0), mu0;  walk at the start
//     iterate:  step (accept / reject the walked trial, next trial);  walk at the trial
//     finish:   accept / reject the last walked trial;  theta, F, covariance, steps, flags
#include <hip/hip_runtime.h>

#include <cstddef>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

enum { FLAG_FIRST = 1, FLAG_DONE = 2, FLAG_IDENT = 4, FLAG_STEP_OK = 8 };
enum { FIT_SCALE = QSC_QFIT_SCALE, FIT_SHIFT = QSC_QFIT_SHIFT };
constexpr int kTerms = 6;  // f, g_tau, g_beta, H_tt, H_tb, H_bb

// the device-resident state, at the head of the workspace
struct QfitState {
  double prior[2];
  double theta_t[2], theta_a[2];  // trial, accepted
  double fc, f_start;             // accepted F (prior included), F at the start
  double g[2], H[3];              // accepted gradient and curvature (without the prior)
  float mu0, tol, mu;
  int max_steps, fit_mask, nwalk, flags, n_active;
};

constexpr size_t kStateBytes = (sizeof(QfitState) + 15) & ~(size_t)15;

inline size_t qfit_ws_bytes(const qsc_obs_desc* d) {
  return kStateBytes + (size_t)(d->Pp / QSC_SLICE) * kTerms * sizeof(double);
}
inline double* qfit_partials(void* ws) {
  return reinterpret_cast<double*>(static_cast<char*>(ws) + kStateBytes);
}

// the fp64 divisor of the packed model: calib_link's a0
inline double qfit_a0(const qsc_model* m) {
  return m->loss == QSC_LOSS_LOGIT ? m->sigma : m->sigma * 1.414213;
}

// ---------------------------------------------------------------------------------------
// the walk: one partial (f, g, H) per slice at the trial theta
// ---------------------------------------------------------------------------------------
template <int RP, typename E, bool SR, bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) qfit_walk_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    int64_t n_ent, int nslices, Link lk0, Edges E_, double a0, int R, int K,
    const float* __restrict__ S, const float* __restrict__ C, const QfitState* st,
    double* __restrict__ part) {
  constexpr int CP = info_pitch(RP);
  const double tau = st->theta_t[0], beta = st->theta_t[1];
  const Link lk = calib_link(lk0, LOGIT, a0, tau);
  QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_);
  // the edge table at beta (each thread shifts the entries it staged), then the barrier again
  for (int b = threadIdx.x; b < lk.nbins; b += kBlock)
    El[b] = calib_edges(E_.e[b], b, lk.nbins, LOG, beta);
  __syncthreads();
  QSC_SLANE(E, SR, K);
  const double inv_a = 1.0 / (double)lk.a;
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    float sv[RP];
    QSC_ROW_LOAD(RP, sv, S + q * RP)
    double acc[kTerms];
#pragma unroll
    for (int i = 0; i < kTerms; ++i) acc[i] = 0.0;
    bool neg = false;
    QSC_SLICE_LISTS(s);
    QSC_WALK_BEGIN(RP, CP, E, SR, sv)
      double td = 0.0;
#pragma unroll
      for (int r = 0; r < RP; ++r) td = __builtin_fma((double)sv[r], (double)cv[r], td);
      float fe, ge[2], he[3];
      bool use, eneg;
      entry_calib<LOGIT, LOG, KIND>(t, code, El, lk, fe, ge, he, use, eneg);
      const double fd = entry_calib_nll<LOGIT, LOG>(fe, eneg, td, El[code], lk, inv_a);
      // a pad adds exactly 0
      use = use && !pad;
      acc[0] += pad ? 0.0 : fd;
      neg = neg || (eneg && !pad);
      acc[1] += use ? (double)ge[0] : 0.0;
      acc[2] += use ? (double)ge[1] : 0.0;
      acc[3] += use ? (double)he[0] : 0.0;
      acc[4] += use ? (double)he[1] : 0.0;
      acc[5] += use ? (double)he[2] : 0.0;
    QSC_WALK_END
    // the two halves of every position, then the 32 positions: the same bits on every lane
    int negi = neg ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int i = 0; i < kTerms; ++i) acc[i] += __shfl_xor(acc[i], m, 64);
      negi |= __shfl_xor(negi, m, 64);
    }
    if (lane == 0) {
      double* out = part + (size_t)s * kTerms;
      out[0] = negi ? (double)__builtin_inff() : acc[0];
#pragma unroll
      for (int i = 1; i < kTerms; ++i) out[i] = acc[i];
    }
  }
}

// elementwise terms (qsc_entry_calib): the device functions of the walk above
template <bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) entry_calib_kernel(
    const int64_t* __restrict__ Y, const float* __restrict__ T, int64_t n, Link lk0, Edges E_,
    double a0, double tau, double beta, double* __restrict__ out) {
  const Link lk = calib_link(lk0, LOGIT, a0, tau);
  QSC_ENTRYWISE_STAGE(lk, calib_edges(E_.e[b_], b_, lk.nbins, LOG, beta));
  const double inv_a = 1.0 / (double)lk.a;
  QSC_ENTRYWISE_BEGIN(lk)
    const float t = T[i];
    float fe, ge[2], he[3];
    bool use, neg;
    entry_calib<LOGIT, LOG, KIND>(t, (int)y, se, lk, fe, ge, he, use, neg);
    const double fd = entry_calib_nll<LOGIT, LOG>(fe, neg, (double)t, se[y], lk, inv_a);
    out[i] = neg ? (double)__builtin_inff() : fd;
    out[n + i] = use ? (double)ge[0] : 0.0;
    out[2 * n + i] = use ? (double)ge[1] : 0.0;
    out[3 * n + i] = use ? (double)he[0] : 0.0;
    out[4 * n + i] = use ? (double)he[1] : 0.0;
    out[5 * n + i] = use ? (double)he[2] : 0.0;
  QSC_ENTRYWISE_END
}

// ---------------------------------------------------------------------------------------
// state initialisation (begin)
// ---------------------------------------------------------------------------------------
__global__ void qfit_init_kernel(QfitState* st, QfitState init) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *st = init;
}

// ---------------------------------------------------------------------------------------
// the step: reduce, accept / reject, solve, next trial (final: results instead)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) qfit_step_kernel(
    QfitState* st, const double* __restrict__ part, int nslices, int final_,
    double* __restrict__ theta_out, double* __restrict__ f_out, double* __restrict__ cov_out,
    double* __restrict__ gh_out, int* __restrict__ steps_out, int* __restrict__ flags_out) {
  __shared__ double red[kTerms][kBlock];
  const int tid = threadIdx.x;
  // thread i: slices i, i + 256, ... in ascending order; then the fold over the threads
  double a[kTerms];
#pragma unroll
  for (int i = 0; i < kTerms; ++i) a[i] = 0.0;
  for (int s = tid; s < nslices; s += kBlock) {
#pragma unroll
    for (int i = 0; i < kTerms; ++i) a[i] += part[(size_t)s * kTerms + i];
  }
#pragma unroll
  for (int i = 0; i < kTerms; ++i) red[i][tid] = a[i];
  __syncthreads();
  for (int w = kBlock / 2; w >= 1; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int i = 0; i < kTerms; ++i) red[i][tid] += red[i][tid + w];
    }
    __syncthreads();
  }
  if (tid != 0) return;

  const float mu_floor = QSC_MU_FLOOR(st->mu0);
  const double prior[2] = {st->prior[0], st->prior[1]};
  int fl = st->flags;
  int nwalk = st->nwalk;
  const bool first = (fl & FLAG_FIRST) != 0;
  bool done = (fl & FLAG_DONE) != 0;
  const bool frozen = done || (!first && nwalk >= st->max_steps);
  double ta[2] = {st->theta_a[0], st->theta_a[1]};
  float mu = st->mu;
  if (!frozen) {
    const double tt[2] = {st->theta_t[0], st->theta_t[1]};
    // F of the trial: the likelihood sum, then the prior
    const double ft =
        red[0][0] + 0.5 * prior[0] * tt[0] * tt[0] + 0.5 * prior[1] * tt[1] * tt[1];
    const double fc = st->fc;
    const bool step_ok = (fl & FLAG_STEP_OK) != 0;
    QSC_NEWTON_ACCEPT(2, first, step_ok, ft, fc, tt, ta, st->tol);
    nwalk += first ? 0 : 1;
    if (acc) {
      st->g[0] = red[1][0];
      st->g[1] = red[2][0];
      st->H[0] = red[3][0];
      st->H[1] = red[4][0];
      st->H[2] = red[5][0];
      ta[0] = tt[0];
      ta[1] = tt[1];
      st->theta_a[0] = tt[0];
      st->theta_a[1] = tt[1];
      st->fc = ft;
      if (first) st->f_start = ft;
      QSC_MU_ACCEPTED(mu, first, mu_floor);
    } else {
      QSC_MU_REJECTED(mu);
    }
    done = conv;
    fl &= ~(FLAG_FIRST | FLAG_DONE);
    fl |= done ? FLAG_DONE : 0;
  }
  const bool free_[2] = {(st->fit_mask & FIT_SCALE) != 0, (st->fit_mask & FIT_SHIFT) != 0};
  const bool live = !frozen && !done && nwalk < st->max_steps;
  if (live && !final_) {
    // ---- the next trial: (H + diag(prior) + mu I) delta = g + prior * theta on the fitted set ----
    const double m = (double)mu;
    const double A[3] = {free_[0] ? st->H[0] + prior[0] + m : 1.0,
                         (free_[0] && free_[1]) ? st->H[1] : 0.0,
                         free_[1] ? st->H[2] + prior[1] + m : 1.0};
    const double rhs[2] = {free_[0] ? st->g[0] + prior[0] * ta[0] : 0.0,
                           free_[1] ? st->g[1] + prior[1] * ta[1] : 0.0};
    double delta[2];
    bool ok, idn;
    chol2_solve_f64(A, free_, m, rhs, delta, ok, idn);
    fl = (ok && idn) ? (fl | FLAG_IDENT) : fl;
    fl = ok ? (fl | FLAG_STEP_OK) : (fl & ~FLAG_STEP_OK);
    // a failed pivot: the step counts as rejected (the accepted point is walked again)
    st->theta_t[0] = (ok && free_[0]) ? ta[0] - delta[0] : ta[0];
    st->theta_t[1] = (ok && free_[1]) ? ta[1] - delta[1] : ta[1];
  } else if (!frozen) {
    // converged or exhausted: the trial is the accepted point from here on
    st->theta_t[0] = ta[0];
    st->theta_t[1] = ta[1];
  }
  if (!frozen) {
    st->mu = mu;
    st->nwalk = nwalk;
    st->flags = fl;
  }
  st->n_active = live ? 1 : 0;
  if (!final_) return;
  theta_out[0] = ta[0];
  theta_out[1] = ta[1];
  f_out[0] = st->fc;
  f_out[1] = st->f_start;
  if (steps_out != nullptr) *steps_out = nwalk;
  *flags_out = ((fl & FLAG_DONE) == 0 ? QSC_QFIT_UNCONVERGED : 0) |
               ((fl & FLAG_IDENT) == 0 ? QSC_QFIT_UNIDENTIFIED : 0);
  if (gh_out != nullptr) {
    gh_out[0] = st->g[0];
    gh_out[1] = st->g[1];
    gh_out[2] = st->H[0];
    gh_out[3] = st->H[1];
    gh_out[4] = st->H[2];
  }
  if (cov_out != nullptr) {
    // the inverse of H + diag(prior) over the fitted parameters, from the pivots of its
    // factorisation; a pivot that is not positive (also of a NaN block): +inf, never NaN
    const double inf = (double)__builtin_inff();
    const double a00 = st->H[0] + prior[0], a01 = st->H[1], a11 = st->H[2] + prior[1];
    double c00 = 0.0, c01 = 0.0, c11 = 0.0;
    if (free_[0] && free_[1]) {
      const double l10 = a01 / a00, p1 = a11 - l10 * a01;
      if (a00 > 0.0 && p1 > 0.0) {
        c11 = 1.0 / p1;
        c01 = -l10 * c11;
        c00 = 1.0 / a00 - l10 * c01;
      } else {
        c00 = c01 = c11 = inf;
      }
    } else if (free_[0]) {
      c00 = a00 > 0.0 ? 1.0 / a00 : inf;
    } else {
      c11 = a11 > 0.0 ? 1.0 / a11 : inf;
    }
    cov_out[0] = c00;
    cov_out[1] = c01;
    cov_out[2] = c11;
  }
}

int qfit_walk(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
              const int64_t* s_off, const qsc_model* m, int R, const float* S, const float* C,
              int kind, const WalkLaunch& wl, void* ws, hipStream_t hs) {
  const int RP = wl.RP;
  const double a0 = qfit_a0(m);
  const dim3 grid((unsigned)slice_grid(wl.nslices, 8)), blk(kBlock);
  const QfitState* st = static_cast<const QfitState*>(ws);
  double* part = qfit_partials(ws);
#define QFIT_LAUNCH(RPV, ET, SRV, LGT, LOGV, KD)                                              \
  hipLaunchKernelGGL((qfit_walk_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, wl.shm, hs,  \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, wl.nslices, \
                     wl.lk, wl.E, a0, R, d->K, S, C, st, part)
  QSC_LAYOUT_DISPATCH(QFIT_LAUNCH);
#undef QFIT_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

int qfit_step(const qsc_obs_desc* d, void* ws, int final_, double* theta_out, double* f_out,
              double* cov_out, double* gh_out, int* steps, int* flags, hipStream_t hs) {
  hipLaunchKernelGGL(qfit_step_kernel, dim3(1), dim3(kBlock), 0, hs, static_cast<QfitState*>(ws),
                     qfit_partials(ws), d->Pp / QSC_SLICE, final_, theta_out, f_out, cov_out,
                     gh_out, steps, flags);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

// the argument checks the three calls share, then the walk's launch record; QSC_OK, or the code
// to return
int qfit_check(const qsc_obs_desc* d, const qsc_model* m, int R, const void* ws, size_t ws_bytes,
               WalkLaunch* wl) {
  if (!d || !info_model_ok(m) || !info_layout_ok(d, m, R)) return QSC_EINVAL;
  if (!ws || ws_bytes < qfit_ws_bytes(d)) return QSC_EINVAL;
  return walk_launch(d, m, R, wl);
}

}  // namespace

extern "C" {

QSC_API size_t qsc_qfit_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  if (!d || R < 1 || R > QSC_MAX_R || d->Pp < QSC_SLICE || (d->Pp % 64) != 0) return 0;
  return qfit_ws_bytes(d);
}

QSC_API int64_t qsc_qfit_active_offset(void) { return (int64_t)offsetof(QfitState, n_active); }

QSC_API int qsc_qfit_begin(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                           const int64_t* s_off, const qsc_model* m, int32_t R, const float* S,
                           const float* C, int32_t kind, int32_t fit_mask, double prior_scale,
                           double prior_shift, double tau0, double beta0, float mu0, float tol,
                           int32_t max_steps, void* ws, size_t ws_bytes, void* stream) {
  if (!s_width || !s_off || !S || !C) return QSC_EINVAL;
  if (!newton_args_ok(kind, 0.0f, mu0, tol, max_steps)) return QSC_EINVAL;
  if (fit_mask < 1 || fit_mask > (FIT_SCALE | FIT_SHIFT)) return QSC_EINVAL;
  if (!(prior_scale >= 0.0) || !(prior_shift >= 0.0) || !(tau0 == tau0) || !(beta0 == beta0))
    return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = qfit_check(d, m, R, ws, ws_bytes, &wl);
  if (rc != QSC_OK) return rc;
  if (d->s_entries > 0 && !s_entries) return QSC_EINVAL;
  QfitState init = {};
  init.prior[0] = prior_scale;
  init.prior[1] = prior_shift;
  init.theta_t[0] = init.theta_a[0] = tau0;
  init.theta_t[1] = init.theta_a[1] = beta0;
  init.mu0 = init.mu = mu0;
  init.tol = tol;
  init.max_steps = max_steps;
  init.fit_mask = fit_mask;
  init.flags = FLAG_FIRST | FLAG_STEP_OK;
  hipStream_t hs = STREAM(stream);
  hipLaunchKernelGGL(qfit_init_kernel, dim3(1), dim3(64), 0, hs, static_cast<QfitState*>(ws), init);
  QSC_CHECK_LAUNCH();
  return qfit_walk(d, s_entries, s_width, s_off, m, R, S, C, kind, wl, ws, hs);
}

QSC_API int qsc_qfit_iterate(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                             const int64_t* s_off, const qsc_model* m, int32_t R, const float* S,
                             const float* C, int32_t kind, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!s_width || !s_off || !S || !C) return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = qfit_check(d, m, R, ws, ws_bytes, &wl);
  if (rc != QSC_OK) return rc;
  if (d->s_entries > 0 && !s_entries) return QSC_EINVAL;
  hipStream_t hs = STREAM(stream);
  const int rs = qfit_step(d, ws, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hs);
  if (rs != QSC_OK) return rs;
  return qfit_walk(d, s_entries, s_width, s_off, m, R, S, C, kind, wl, ws, hs);
}

QSC_API int qsc_qfit_finish(const qsc_obs_desc* d, const qsc_model* m, int32_t R,
                            double* theta_out, double* f_out, double* cov_out, double* gh_out,
                            int32_t* steps, int32_t* flags, void* ws, size_t ws_bytes,
                            void* stream) {
  if (!theta_out || !f_out || !flags) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = qfit_check(d, m, R, ws, ws_bytes, &wl);
  if (rc != QSC_OK) return rc;
  return qfit_step(d, ws, 1, theta_out, f_out, cov_out, gh_out, steps, flags, STREAM(stream));
}

QSC_API int qsc_entry_calib(const int64_t* Y, const float* T, int64_t n, const qsc_model* m,
                            double tau, double beta, int32_t kind, double* out, void* stream) {
  if (!entry_args_ok(m, n, Y, T, out)) return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  if (!(tau == tau) || !(beta == beta)) return QSC_EINVAL;
  if (n == 0) return QSC_OK;
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const double a0 = qfit_a0(m);
  const dim3 grid = entry_grid(n), blk(kBlock);
  hipStream_t hs = STREAM(stream);
#define CALIB_LAUNCH(LGT, LOGV, KD)                                                            \
  hipLaunchKernelGGL((entry_calib_kernel<LGT, LOGV, KD>), grid, blk, 0, hs, Y, T, n, lk, E, a0, \
                     tau, beta, out)
  QSC_INFO_DISPATCH(CALIB_LAUNCH);
#undef CALIB_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
