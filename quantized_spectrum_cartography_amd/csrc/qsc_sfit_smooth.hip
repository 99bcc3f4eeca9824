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
// Per own-colour position the walk, the per-entry terms and the iteration are qsc_newton.cuh's,
// as in sfit_kernel.  After the halves are summed, each existing neighbour n and each r < R adds,
// with d = s_r - S[n][r]:
//     f    += weight * rho(d)       in fp64 from the fp32 operands (the accept test compares
//                                   values of phi that differ by |g|^2 / lambda near the minimiser)
//     g_r  += weight * rho'(d)      QUAD: d;  HUBER: clamp(d / delta, -1, 1)
//     J_rr += weight * kappa(d)     QUAD: 1;  HUBER: 1 / max(|d|, delta), the half-quadratic
//                                   majoriser: rho'' inside |d| <= delta, positive outside
// and only then is phi made +inf for a trial outside the log model's domain.  At most inner_steps
// trial evaluations per visit; mu restarts at mu0 every visit; nothing is kept per position
// between launches.
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

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

constexpr int64_t kSmoothMaxPp = (int64_t)1 << 28;  // qsc_smooth.hip's position bound

enum { SMOOTH_QUAD = QSC_SMOOTH_QUAD, SMOOTH_HUBER = QSC_SMOOTH_HUBER };

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
  constexpr int NT = tri_count(RP);
  constexpr bool WS = newton_in_ws(RP);
  QSC_STAGE_TABLE(RP, CP, K, R, C, lk, E_);
  QSC_SLANE(E, SR, K);
  const float mu_floor = QSC_MU_FLOOR(pr.mu0);
  const double inv_a = 1.0 / (double)lk.a;
  int cnt_moved = 0, cnt_unconv = 0, cnt_unident = 0;  // (wave-uniform)
  // (reused by every slice of the wave)
  float* wrow = QSC_WS_ROW(ws, wave, lane, RP, NT);
  for (int s = blockIdx.x * kWaves + wave; s < nslices; s += gridDim.x * kWaves) {
    const int64_t q = (int64_t)s * QSC_SLICE + l;
    const int p = perm[q];
    // own: a pixel of this visit's colour; every other position is neither changed nor written
    const bool own = p >= 0 && p < P_ && ((((p / pr.J) + (p % pr.J)) & 1) == pr.color);
    if (__ballot(own) == 0ull) continue;  // (wave-uniform)
    // the accepted state (sc, fc, gc, Jc) and the trial point st
    float sc[RP], st[RP], gc[WS ? 1 : RP], Jc[WS ? 1 : NT];
    double fc = 0.0;
    QSC_ROW_LOAD_MASKED(RP, sc, S + q * RP, own, R)
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
    QSC_SLICE_LISTS(s);
    for (int it = 0;; ++it) {
      // ---- walk: (ft, gt, Jt) at st (sfit_kernel's) ----
      QSC_WALK_SLICE(RP, NT, CP, E, SR, LOGIT, LOG, KIND, st, pr.ridge);
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
            QSC_VEC4(xs, nrow + r);
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
      if (it == pr.inner_steps || __ballot(!done) == 0ull) break;

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
    // ---- results (half 0 of an own-colour position writes its row; nobody else writes) ----
    const bool wr = own && h == 0;
    bool moved = false;
    if (wr) {
      // the row as the visit found it, read again for the n_moved test, then overwritten
      float dmax = 0.0f, smax = 0.0f;
#pragma unroll
      for (int r = 0; r < RP; r += 4) {
        QSC_VEC4(xs, S + q * RP + r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s0 = r + e < R ? xs[e] : 0.0f;
          dmax = fmaxf(dmax, fabsf(sc[r + e] - s0));
          smax = fmaxf(smax, fabsf(s0));
        }
      }
      moved = dmax > pr.tol * (1.0f + smax);
      QSC_ROW_STORE(RP, S + q * RP, sc);
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
              QSC_VEC4(xs, nrow + r);
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

}  // namespace

extern "C" {

QSC_API size_t qsc_sfit_smooth_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  return newton_ws_bytes(d, R);
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
  if (!newton_args_ok(kind, ridge, mu0, tol, inner_steps)) return QSC_EINVAL;
  if (color != 0 && color != 1) return QSC_EINVAL;
  if (!(weight >= 0.0f)) return QSC_EINVAL;
  if (smooth_kind != SMOOTH_QUAD && smooth_kind != SMOOTH_HUBER) return QSC_EINVAL;
  if (smooth_kind == SMOOTH_HUBER && !(delta > 0.0f)) return QSC_EINVAL;
  if (!info_layout_ok(d, m, R) || (d->s_entries > 0 && !s_entries)) return QSC_EINVAL;
  if (I < 1 || J < 1 || (int64_t)I * J != (int64_t)d->P) return QSC_EINVAL;
  if ((int64_t)d->Pp > kSmoothMaxPp) return QSC_EUNSUPPORTED;
  const size_t need = newton_ws_bytes(d, R);
  if (need > 0 && (!ws || ws_bytes < need)) return QSC_EINVAL;
  WalkLaunch wl;
  const int rc = walk_launch(d, m, R, &wl);
  if (rc != QSC_OK) return rc;
  const int RP = wl.RP;
  const bool huber = smooth_kind == SMOOTH_HUBER;
  const SfsParams pr = {ridge, mu0, tol, inner_steps, project != 0, color, J, d->Pp, huber ? 1 : 0,
                        weight, huber ? delta : 0.0f, huber ? 1.0f / delta : 1.0f};
  const dim3 grid((unsigned)newton_grid(wl.nslices, RP)), blk(kBlock);
  hipStream_t hs = STREAM(stream);
  const int4* n4 = reinterpret_cast<const int4*>(nbr);
#define SFS_LAUNCH(RPV, ET, SRV, LGT, LOGV, KD)                                                \
  hipLaunchKernelGGL((sfit_smooth_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, wl.shm, hs, \
                     (const ET*)s_entries, s_width, s_off, (int64_t)d->s_entries, wl.nslices,  \
                     wl.lk, wl.E, R, d->K, d->P, perm, n4, C, S, pr, f_out, nll_out, steps,    \
                     n_moved, n_unconverged, n_unidentified, (float*)ws)
  QSC_LAYOUT_DISPATCH(SFS_LAUNCH);
#undef SFS_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
