// qsc_sfit.hip — per-pixel damped Newton / Fisher-scoring fit of the loss fields S for known
// spectra C (include/qsc.h: qsc_sfit, qsc_sfit_workspace_bytes).
//
// Conditional on C the likelihood separates over positions; position q minimises, over
// s = S[q][0..R), qsc_newton.cuh's objective with the table rows c_k = C[:, k].  That header has
// the per-entry terms, the walk, the iteration, the identification rule and the workspace row
// (as statement macros); this file is the kernel that runs them for every position, and the C
// entry point.
//
// The iteration runs inside the one launch, with the same structure on every lane.  A converged
// position stops changing; the wave leaves the loop when every position of its slice has
// converged (ballot).  Two calls agree bit for bit.
#include <hip/hip_runtime.h>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

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
  constexpr int NT = tri_count(RP);
  constexpr bool WS = newton_in_ws(RP);
  QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_);
  QSC_SLANE(E, SR, K);
  const float mu_floor = QSC_MU_FLOOR(pr.mu0);
  const double inv_a = 1.0 / (double)lk.a;
  int cnt_unconv = 0, cnt_unident = 0;  // (wave-uniform)
  float* wrow = QSC_WS_ROW(ws, wave, lane, RP, NT);
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    const bool live = p >= 0 && p < P_;
    // the accepted state (sc, fc, gc, Jc) and the trial point st
    float sc[RP], st[RP], gc[WS ? 1 : RP], Jc[WS ? 1 : NT];
    double fc = 0.0;
    QSC_ROW_LOAD_MASKED(RP, sc, S_init + q * RP, live, R)
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
    QSC_SLICE_LISTS(s);
    for (int it = 0;; ++it) {
      // ---- walk: (ft, gt, Jt) at st ----
      QSC_WALK_SLICE(RP, NT, CP, E, SR, LOGIT, LOG, KIND, st, pr.ridge);
      ft = neg ? (double)__builtin_inff() : ft;

      // ---- accept / reject ----
      const bool first = it == 0;
      QSC_NEWTON_ACCEPT(RP, first, step_ok, ft, fc, st, sc, pr.tol);
      if (WS && acc && (first || !done)) {
        // (the first evaluation is stored by every lane, so that no row is read unwritten)
        QSC_WS_PUT(RP, NT, wrow, gt, Jt);
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
          QSC_MU_ACCEPTED(mu, first, mu_floor);
        } else {
          QSC_MU_REJECTED(mu);
        }
        done = conv;
      }
      if (it == pr.max_steps || __ballot(!done) == 0ull) break;

      // ---- the next trial: Cholesky of Jc + (ridge + mu) I, delta from gc + ridge sc ----
      // rows >= R are the identity (Jc is 0 there)
      float a[NT];
      if (WS) {
        QSC_ROW_LOAD(NT, a, wrow + RP)
      } else {
#pragma unroll
        for (int i = 0; i < NT; ++i) a[i] = Jc[i];
      }
      const float lam = pr.ridge + mu;
#pragma unroll
      for (int i = 0; i < RP; ++i) a[tri<RP>(i, i)] = i < R ? a[tri<RP>(i, i)] + lam : 1.0f;
      QSC_CHOL_SOLVE(RP, a, mu, j_ < R, __builtin_fmaf(pr.ridge, sc[i_], WS ? wrow[i_] : gc[i_]))
      // a failed pivot: the step counts as rejected (st = sc is walked)
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
      QSC_ROW_STORE(RP, S_out + q * RP, sc);
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

}  // namespace

extern "C" {

QSC_API size_t qsc_sfit_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  return newton_ws_bytes(d, R);
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
  if (!newton_args_ok(kind, ridge, mu0, tol, max_steps)) return QSC_EINVAL;
  if (!info_layout_ok(d, m, R) || (d->s_entries > 0 && !s_entries)) return QSC_EINVAL;
  const size_t need = newton_ws_bytes(d, R);
  if (need > 0 && (!ws || ws_bytes < need)) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = walk_launch(d, m, R, &wl);
  if (rc != QSC_OK) return rc;
  const int RP = wl.RP;
  const SfitParams pr = {ridge, mu0, tol, max_steps, project != 0};
  const dim3 grid((unsigned)newton_grid(wl.nslices, RP)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
#define SFIT_LAUNCH(RPV, ET, SRV, LGT, LOGV, KD)                                              \
  hipLaunchKernelGGL((sfit_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, wl.shm, hs,       \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, wl.nslices, \
                     wl.lk, wl.E, R, d->K, d->P, perm, C, S_init, pr, S_out, f_out, steps,    \
                     n_unconverged, n_unidentified, (float*)ws)
  QSC_LAYOUT_DISPATCH(SFIT_LAUNCH);
#undef SFIT_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
