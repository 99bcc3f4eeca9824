// qsc_cfit.hip — per-bin projected Newton / Fisher-scoring fit of the spectra C for known loss
// fields S (include/qsc.h: qsc_cfit_workspace_bytes, qsc_cfit_begin, qsc_cfit_iterate,
// qsc_cfit_finish).
//
// Conditional on S the likelihood separates over frequency bins; bin k minimises, over
// c = C[0..R)[k], qsc_newton.cuh's objective with the table rows s_q = S[q] of the positions
// observed in the bin: qsc_sfit's problem with the roles of S and C exchanged, with the same
// per-entry terms, accept rule, mu schedule and factorisation (that header).  But a bin's entries
// are spread over every pixel tile of the C-format lists, so the evaluation and the R x R solve
// are two kernels with a fixed-order reduction between them.
//
// cfit_eval_kernel: the walk.  The work unit is the C-pass's: (pixel tile, 64-bin k-slice),
// lane = bin c_kmap[(t nks + ks) 64 + lane].  One workgroup owns a fixed, contiguous group of
// tiles and walks them in sequence; per tile it stages the tile's S rows (snake tile-row ->
// position map, tile_pos) in LDS once, then its waves take the tile's k-slices.  A lane keeps f
// (fp64), g[RP] and the RP (RP + 1) / 2 upper-triangle accumulators of J in registers over its
// list, loading the next 4-entry chunk before the arithmetic of this one.  c_kmap orders the bins
// of EVERY TILE by their count in that tile, so the bin a lane walks changes from tile to tile: at
// the end of a unit the lane folds its registers into the row of its bin in the group's partial
// (the first tile of the group stores, the later ones add).  The partial of a group is written by
// its one workgroup only, each (tile, bin) by exactly one lane, tiles in ascending order with a
// workgroup barrier between them: no atomics, and the order of every sum is fixed by the layout.
// The number of groups G comes from the layout alone (cfit_groups): one per tile while the
// partials stay below kPartialCap, fewer and longer groups beyond.
//
// cfit_step_kernel: one wave per bin.  Adds the G partials in ascending group order (f, g and J
// in fp64, g and J then rounded to fp32; the accumulators of g and J one per lane, each summed in
// that order by its lane), and lane 0 applies the accept / reject rule against the bin's
// device-resident state, factors J + (ridge + mu) I with the held rows replaced by the identity
// (two-metric projected Newton: the held set is A = {r : c_r <= 0 and gamma_r > 0},
// gamma = g + ridge c), solves, and writes the next trial column.  The gradient and block of a
// trial are only reduced when the trial is accepted (f decides), straight into the state.
//
//     begin:    state <- C_init, mu0;  walk at C_init
//     iterate:  step (accept / reject the walked trial, next trial);  walk at the trial
//     finish:   accept / reject the last walked trial;  C_out, f, steps, counters, std_C
#include <hip/hip_runtime.h>

#include <algorithm>

#include "qsc_common.cuh"
#include "qsc_newton.cuh"

namespace {
using namespace qsc;

constexpr int kStepBlock = 64;
// the most partial bytes one call may ask for; beyond it tiles share a group
constexpr size_t kPartialCap = (size_t)64 << 20;
constexpr int kMaxGroups = 1024;

enum { FLAG_FIRST = 1, FLAG_DONE = 2, FLAG_IDENT = 4, FLAG_STEP_OK = 8 };

struct CfitParams {
  float ridge, mu0, tol;
  int max_steps, project, n_active, pad0_, pad1_;
};

// the workspace, carved (host and device agree through this one function)
struct CfitWs {
  CfitParams* prm;
  double* pf;   // [G][K]            partial f
  double* fc;   // [K]               accepted f (ridge term included)
  float* pgj;   // [G][K][NA]        partial rows: g, then the triangle of J (NA = row_floats)
  float* gj;    // [K][NA]           accepted g, J
  float* Ct;    // [R][K]            trial C
  float* Ca;    // [R][K]            accepted C
  float* mu;    // [K]
  int* nwalk;   // [K]
  int* flags;   // [K]
};

// floats of one (g, J) row: g[RP], the triangle of J, padded to whole 16-byte vectors
__host__ __device__ constexpr int row_floats(int RP) { return (RP + tri_count(RP) + 3) & ~3; }

inline int cfit_groups(const qsc_obs_desc* d, int RP) {
  const size_t row = (size_t)d->K * (row_floats(RP) * sizeof(float) + sizeof(double));
  const int64_t fit = std::max<int64_t>(1, (int64_t)(kPartialCap / row));
  return (int)std::min<int64_t>(std::min<int64_t>(d->ntiles, kMaxGroups), fit);
}

inline size_t cfit_carve(const qsc_obs_desc* d, int R, int RP, int G, void* ws, CfitWs* w) {
  const size_t K = (size_t)d->K, NA = (size_t)row_floats(RP);
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* r = p ? p + o : nullptr;
    o += (bytes + 15) & ~(size_t)15;
    return r;
  };
  w->prm = reinterpret_cast<CfitParams*>(take(sizeof(CfitParams)));
  w->pf = reinterpret_cast<double*>(take((size_t)G * K * sizeof(double)));
  w->fc = reinterpret_cast<double*>(take(K * sizeof(double)));
  w->pgj = reinterpret_cast<float*>(take((size_t)G * NA * K * sizeof(float)));
  w->gj = reinterpret_cast<float*>(take(NA * K * sizeof(float)));
  w->Ct = reinterpret_cast<float*>(take((size_t)R * K * sizeof(float)));
  w->Ca = reinterpret_cast<float*>(take((size_t)R * K * sizeof(float)));
  w->mu = reinterpret_cast<float*>(take(K * sizeof(float)));
  w->nwalk = reinterpret_cast<int*>(take(K * sizeof(int)));
  w->flags = reinterpret_cast<int*>(take(K * sizeof(int)));
  return o;
}

// LDS of the walk: the S tile at the info_pitch pitch and the edges
inline size_t cfit_lds(int PT, int RP, int nbins) {
  return (size_t)PT * info_pitch(RP) * 4 + (size_t)nbins * 8;
}

// the lane's 4 entries of one chunk; a read past the entry array is clamped and returned as pads
template <typename E>
__device__ __forceinline__ void load_quad(const E* __restrict__ ent, int64_t idx, int64_t n_ent,
                                          uint32_t pad_value, uint32_t (&v)[4]) {
  const bool in = idx >= 0 && idx + 3 < n_ent;
  const int64_t i = in ? idx : 0;
  if (sizeof(E) == 2) {
    const uint2 w = *reinterpret_cast<const uint2*>(ent + i);  // idx is a multiple of 4
    v[0] = w.x & 0xFFFFu;
    v[1] = w.x >> 16;
    v[2] = w.y & 0xFFFFu;
    v[3] = w.y >> 16;
  } else {
    const uint4 w = *reinterpret_cast<const uint4*>(ent + i);
    v[0] = w.x;
    v[1] = w.y;
    v[2] = w.z;
    v[3] = w.w;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = in ? v[e] : pad_value;
}

// ---------------------------------------------------------------------------------------
// the walk: (f, g, J) of every bin at the trial C, one partial per (tile group, bin)
// ---------------------------------------------------------------------------------------
template <int RP, typename E, bool SR, bool LOGIT, bool LOG, int KIND>
__global__ void __launch_bounds__(kBlock) cfit_eval_kernel(
    const E* __restrict__ ent, const int* __restrict__ width, const int64_t* __restrict__ off,
    const int* __restrict__ kmap, int64_t n_ent, int nks, int PT, int ntiles, int G, Link lk,
    Edges E_, int R, int K, const float* __restrict__ S, const float* Ct, double* pf, float* pgj) {
  constexpr int SP = info_pitch(RP);
  constexpr int NT = tri_count(RP);
  constexpr int V = RP / 4;  // float4 per row
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Sl = smem;                                              // [PT][SP]
  float2* El = reinterpret_cast<float2*>(Sl + (size_t)PT * SP);  // [nbins]
  for (int b = threadIdx.x; b < lk.nbins; b += blockDim.x) El[b] = E_.e[b];

  const int NW = blockDim.x >> 6;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int Qo = sr_off(PT);
  const uint32_t pad_value = SR ? 2u * (uint32_t)Qo : (Ent<E>::kPad << Ent<E>::kBits);
  const double inv_a = 1.0 / (double)lk.a;
  const int g = blockIdx.x;
  // the group's tiles: a contiguous range, the same split for every call on this layout
  const int t0 = (int)(((int64_t)g * ntiles) / G), t1 = (int)(((int64_t)(g + 1) * ntiles) / G);
  double* pfg = pf + (size_t)g * K;
  constexpr int NA = row_floats(RP);
  float* pg = pgj + (size_t)g * K * NA;
  const float4* __restrict__ src4 = reinterpret_cast<const float4*>(S);

  for (int t = t0; t < t1; ++t) {
    // (the barrier also orders the previous tile's partial rows before this tile's adds to them:
    // another wave of this workgroup may hold the bin now)
    __syncthreads();
    for (int i = threadIdx.x; i < PT * V; i += blockDim.x) {
      const int ql = i / V, c = i - ql * V;
      *reinterpret_cast<float4*>(Sl + (size_t)ql * SP + 4 * c) = src4[tile_pos(t, ql, ntiles) * V + c];
    }
    __syncthreads();
    for (int ks = wave; ks < nks; ks += NW) {
      const int64_t wi = (int64_t)t * nks + ks;
      const int nch = width[wi] >> 2;
      const int64_t base = off[wi] + lane * 4;
      const int k = kmap[wi * 64 + lane];
      const bool live = k >= 0 && k < K;  // (k >= K: an empty padding bin)
      float cv[RP];
#pragma unroll
      for (int r = 0; r < RP; ++r) cv[r] = (live && r < R) ? Ct[(int64_t)r * K + k] : 0.0f;
      double ft = 0.0;
      float gt[RP], Jt[NT];
      bool neg = false;
#pragma unroll
      for (int r = 0; r < RP; ++r) gt[r] = 0.0f;
#pragma unroll
      for (int i = 0; i < NT; ++i) Jt[i] = 0.0f;
      uint32_t nx[4];
      load_quad<E>(ent, base, n_ent, pad_value, nx);
      for (int ch = 0; ch < nch; ++ch) {
        const uint32_t v[4] = {nx[0], nx[1], nx[2], nx[3]};
        // the next chunk's entries while this one is worked (past the last chunk: the next block's
        // entries or the array's pad tail, QSC_ENTRY_TAIL; clamped in load_quad either way)
        load_quad<E>(ent, base + (int64_t)(ch + 1) * 256, n_ent, pad_value, nx);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int q, code;
          bool pad;
          decode<E, SR>(v[e], PT, Qo, lk.nbins, q, code, pad);
          float sv[RP];
          QSC_ROW_LOAD(RP, sv, Sl + (size_t)q * SP)
          QSC_ENTRY_ACCUMULATE(RP, LOGIT, LOG, KIND, cv, sv, code, pad, El, lk, inv_a, ft, neg, gt,
                               Jt)
        }
      }
      ft = neg ? (double)__builtin_inff() : ft;
      // fold into the group's partial row of this lane's bin (first tile: store), 16 bytes at a time
      if (live) {
        // element i of the row: g, then the triangle of J, then the padding
        auto val = [&](int i) { return i < RP ? gt[i] : (i < RP + NT ? Jt[i - RP] : 0.0f); };
        float4* row = reinterpret_cast<float4*>(pg + (size_t)k * NA);
        if (t == t0) {
          pfg[k] = ft;
#pragma unroll
          for (int i = 0; i < NA; i += 4)
            row[i >> 2] = make_float4(val(i), val(i + 1), val(i + 2), val(i + 3));
        } else {
          pfg[k] += ft;
#pragma unroll
          for (int i = 0; i < NA; i += 4) {
            const float4 o = row[i >> 2];
            row[i >> 2] =
                make_float4(o.x + val(i), o.y + val(i + 1), o.z + val(i + 2), o.w + val(i + 3));
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// state initialisation (begin)
// ---------------------------------------------------------------------------------------
__global__ void cfit_init_kernel(CfitWs w, CfitParams pr, int R, int K, const float* C_init) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) *w.prm = pr;
  if (k >= K) return;
  for (int r = 0; r < R; ++r) {
    const float c = C_init[(int64_t)r * K + k];
    w.Ct[(int64_t)r * K + k] = c;
    w.Ca[(int64_t)r * K + k] = c;
  }
  w.mu[k] = pr.mu0;
  w.fc[k] = 0.0;
  w.nwalk[k] = 0;
  w.flags[k] = FLAG_FIRST | FLAG_STEP_OK;
}

// ---------------------------------------------------------------------------------------
// the step: reduce, accept / reject, factor, solve, next trial (final: results instead)
// ---------------------------------------------------------------------------------------
// One wave per bin.  Every sum over the G partials runs in ascending group order in fp64, eight
// loads in flight at a time: f on every lane (the same addresses, so the same bits: the accept
// decision is lane-uniform), the accumulators a = lane, lane + 64, ... of g and J one per lane.
// The bin's state logic -- factor, solve, next trial, results -- is lane 0's alone.
template <typename T>
__device__ __forceinline__ double sum_groups(const T* __restrict__ p, size_t stride, int G) {
  double s = 0.0;
  for (int g0 = 0; g0 < G; g0 += 8) {
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (g0 + j < G) ? (double)p[(size_t)(g0 + j) * stride] : 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];  // (s + 0.0 == s: the tail changes nothing)
  }
  return s;
}

template <int RP>
__global__ void __launch_bounds__(kStepBlock) cfit_step_kernel(
    CfitWs w, int R, int K, int G, int final_, float* C_out, double* __restrict__ f_out,
    int* __restrict__ steps_out, float* __restrict__ std_C, int* __restrict__ n_unconverged,
    int* __restrict__ n_unidentified) {
  constexpr int NT = tri_count(RP);
  constexpr int NA = row_floats(RP);
  const int k = blockIdx.x, lane = threadIdx.x;
  const CfitParams pr = *w.prm;
  const float mu_floor = QSC_MU_FLOOR(pr.mu0);
  int fl = w.flags[k];
  int nwalk = w.nwalk[k];
  const bool first = (fl & FLAG_FIRST) != 0;
  bool done = (fl & FLAG_DONE) != 0;
  const bool frozen = done || (!first && nwalk >= pr.max_steps);
  float ca[RP];
#pragma unroll
  for (int r = 0; r < RP; ++r) ca[r] = r < R ? w.Ca[(int64_t)r * K + k] : 0.0f;
  float mu = w.mu[k];
  float* gjk = w.gj + (size_t)k * NA;
  if (!frozen) {
    float ct[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) ct[r] = r < R ? w.Ct[(int64_t)r * K + k] : 0.0f;
    // ---- f of the trial: the G partials in ascending group order, then the ridge term ----
    double ft = sum_groups(w.pf + k, (size_t)K, G);
    double nsq = 0.0;
#pragma unroll
    for (int r = 0; r < RP; ++r) nsq = __builtin_fma((double)ct[r], (double)ct[r], nsq);
    ft += 0.5 * (double)pr.ridge * nsq;
    const double fc = w.fc[k];
    const bool step_ok = (fl & FLAG_STEP_OK) != 0;
    QSC_NEWTON_ACCEPT(RP, first, step_ok, ft, fc, ct, ca, pr.tol);
    nwalk += first ? 0 : 1;
    if (acc) {
      // the accepted gradient and block: fp64 sums in group order, rounded to fp32 once
      for (int a = lane; a < RP + NT; a += kStepBlock)
        gjk[a] = (float)sum_groups(w.pgj + (size_t)k * NA + a, (size_t)K * NA, G);
#pragma unroll
      for (int r = 0; r < RP; ++r) ca[r] = ct[r];
      if (lane == 0) {
        w.fc[k] = ft;
#pragma unroll
        for (int r = 0; r < RP; ++r)
          if (r < R) w.Ca[(int64_t)r * K + k] = ct[r];
      }
      QSC_MU_ACCEPTED(mu, first, mu_floor);
    } else {
      QSC_MU_REJECTED(mu);
    }
    done = conv;
    fl &= ~(FLAG_FIRST | FLAG_DONE);
    fl |= done ? FLAG_DONE : 0;
  }
  // (the rows of g and J the lanes wrote, before lane 0 reads them)
  __syncthreads();
  if (lane != 0) return;
  const bool live = !frozen && !done && nwalk < pr.max_steps;
  if (live && !final_) {
    // ---- the next trial: Cholesky of J + (ridge + mu) I on the free set ----
    float a[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) a[i] = gjk[RP + i];
    float gam[RP];
    bool held[RP];
#pragma unroll
    for (int r = 0; r < RP; ++r) {
      const float gr = r < R ? gjk[r] : 0.0f;
      gam[r] = __builtin_fmaf(pr.ridge, ca[r], gr);
      held[r] = r >= R || (pr.project && ca[r] <= 0.0f && gam[r] > 0.0f);
      gam[r] = held[r] ? 0.0f : gam[r];
    }
    const float lam = pr.ridge + mu;
#pragma unroll
    for (int i = 0; i < RP; ++i) {
#pragma unroll
      for (int j = i; j < RP; ++j) {
        float v = a[tri<RP>(i, j)];
        if (i == j) v = held[i] ? 1.0f : v + lam;
        else if (held[i] || held[j]) v = 0.0f;
        a[tri<RP>(i, j)] = v;
      }
    }
    QSC_CHOL_SOLVE(RP, a, mu, !held[j_], gam[i_])
    fl = (ok && idn) ? (fl | FLAG_IDENT) : fl;
    fl = ok ? (fl | FLAG_STEP_OK) : (fl & ~FLAG_STEP_OK);
#pragma unroll
    for (int r = 0; r < RP; ++r) {
      float v = ca[r] - y[r];
      v = pr.project ? fmaxf(v, 0.0f) : v;
      v = (ok && !held[r]) ? v : ca[r];
      if (r < R) w.Ct[(int64_t)r * K + k] = v;
    }
  } else if (!frozen) {
    // converged or exhausted: the trial column is the accepted column from here on
#pragma unroll
    for (int r = 0; r < RP; ++r)
      if (r < R) w.Ct[(int64_t)r * K + k] = ca[r];
  }
  if (!frozen) {
    w.mu[k] = mu;
    w.nwalk[k] = nwalk;
    w.flags[k] = fl;
  }
  // integer atomics only (integer addition: any order gives the same count)
  if (live) atomicAdd(&w.prm->n_active, 1);
  if (!final_) return;
  if ((fl & FLAG_DONE) == 0) atomicAdd(n_unconverged, 1);
  if ((fl & FLAG_IDENT) == 0) atomicAdd(n_unidentified, 1);
#pragma unroll
  for (int r = 0; r < RP; ++r)
    if (r < R) C_out[(int64_t)r * K + k] = ca[r];
  if (f_out != nullptr) f_out[k] = w.fc[k];
  if (steps_out != nullptr) steps_out[k] = nwalk;
  if (std_C != nullptr) {
    // sqrt(diag((J + ridge I)^-1)) at the accepted point (qsc_info_std's steps); the bound is not
    // applied here
    float a[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) a[i] = gjk[RP + i];
#pragma unroll
    for (int i = 0; i < RP; ++i) {
#pragma unroll
      for (int j = i; j < RP; ++j) {
        float v = a[tri<RP>(i, j)];
        if (i == j) v = i < R ? v + pr.ridge : 1.0f;
        else if (j >= R) v = 0.0f;
        a[tri<RP>(i, j)] = v;
      }
    }
    float dinv[RP];
    bool bad = false;
    QSC_CHOL_INVERSE(RP, a, dinv, bad)
#pragma unroll
    for (int j = 0; j < RP; ++j) {
      float v = 0.0f;
#pragma unroll
      for (int i = j; i < RP; ++i) v = __builtin_fmaf(a[tri<RP>(j, i)], a[tri<RP>(j, i)], v);
      if (j < R) std_C[(int64_t)j * K + k] = bad ? __builtin_inff() : sqrtf(v);
    }
  }
}

// the C-format checks of the walk (info_layout_ok's, for the tile rows instead of the bins)
inline bool cfit_layout_ok(const qsc_obs_desc* d, const qsc_model* m, int R) {
  if (R < 1 || R > QSC_MAX_R || d->K < 1 || d->P < 1 || d->Pp < d->P || d->PT < 64 ||
      (d->PT % 64) != 0 || d->ntiles < 1 || (int64_t)d->ntiles * d->PT != d->Pp ||
      d->nks != (d->K + 63) / 64 || d->nbins != m->nbounds - 1 || d->c_entries < QSC_ENTRY_TAIL)
    return false;
  if (d->rowfmt != 0 && d->rowfmt != 1) return false;
  if (d->rowfmt == 1 && (d->wide || d->nbins != 2 || (int64_t)sr_rows(d->PT) > 0x10000))
    return false;
  if (!d->wide && d->rowfmt == 0 && (d->PT > 4096 || d->nbins > 15)) return false;
  if (d->wide && d->PT > (1 << 24)) return false;
  if (d->rowfmt == 1 && m->log_model) return false;
  return true;
}

int cfit_walk(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
              const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m, int R, int RP, int G,
              const float* S, int kind, const CfitWs& w, hipStream_t hs) {
  const size_t shm = cfit_lds(d->PT, RP, d->nbins);
  const Link lk = make_link(m);
  Edges E;
  make_edges(m, &E);
  const dim3 grid((unsigned)G), blk((unsigned)(64 * std::min(d->nks, kWaves)));
#define CFIT_LAUNCH(RPV, ET, SRV, LGT, LOGV, KD)                                                \
  hipLaunchKernelGGL((cfit_eval_kernel<RPV, ET, SRV, LGT, LOGV, KD>), grid, blk, shm, hs,       \
                     (const ET*)c_entries, c_width, c_off, c_kmap, (int64_t)d->c_entries, d->nks, \
                     d->PT, d->ntiles, G, lk, E, R, d->K, S, w.Ct, w.pf, w.pgj)
  QSC_LAYOUT_DISPATCH(CFIT_LAUNCH);
#undef CFIT_LAUNCH
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

int cfit_step(int R, int RP, int K, int G, const CfitWs& w, int final_, float* C_out,
              double* f_out, int* steps, float* std_C, int* n_unconverged, int* n_unidentified,
              hipStream_t hs) {
  // the active-bin counter of this step (a memset node when captured)
  QSC_TRY(hipMemsetAsync(&w.prm->n_active, 0, sizeof(int), hs));
  const dim3 grid((unsigned)K), blk(kStepBlock);  // one wave per bin
#define CFIT_STEP(RPV)                                                                          \
  hipLaunchKernelGGL(cfit_step_kernel<RPV>, grid, blk, 0, hs, w, R, K, G, final_, C_out, f_out, \
                     steps, std_C, n_unconverged, n_unidentified)
  if (RP == 4) CFIT_STEP(4);
  else if (RP == 8) CFIT_STEP(8);
  else CFIT_STEP(16);
#undef CFIT_STEP
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

// the argument checks the three calls share; QSC_OK, or the code to return
int cfit_check(const qsc_obs_desc* d, const qsc_model* m, int R, const void* ws, size_t ws_bytes) {
  if (!d || !info_model_ok(m) || !cfit_layout_ok(d, m, R)) return QSC_EINVAL;
  const size_t need = qsc_cfit_workspace_bytes(d, R);
  if (need == 0 || !ws || ws_bytes < need) return QSC_EINVAL;
  if (cfit_lds(d->PT, qsc_rank_pad(R), d->nbins) > kInfoLdsMax) return QSC_EUNSUPPORTED;
  return QSC_OK;
}

}  // namespace

extern "C" {

QSC_API size_t qsc_cfit_workspace_bytes(const qsc_obs_desc* d, int32_t R) {
  if (!d || R < 1 || R > QSC_MAX_R || d->K < 1 || d->ntiles < 1) return 0;
  const int RP = qsc_rank_pad(R);
  CfitWs w;
  return cfit_carve(d, R, RP, cfit_groups(d, RP), nullptr, &w);
}

QSC_API int32_t qsc_cfit_groups(const qsc_obs_desc* d, int32_t R) {
  if (!d || R < 1 || R > QSC_MAX_R || d->K < 1 || d->ntiles < 1) return 0;
  return cfit_groups(d, qsc_rank_pad(R));
}

QSC_API int64_t qsc_cfit_active_offset(void) { return (int64_t)offsetof(CfitParams, n_active); }

QSC_API int qsc_cfit_begin(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                           const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                           int32_t R, const float* S, const float* C_init, int32_t kind,
                           float ridge, float mu0, float tol, int32_t max_steps, int32_t project,
                           void* ws, size_t ws_bytes, void* stream) {
  // (the entry array always holds its QSC_ENTRY_TAIL pads, which the walk's read-ahead may touch)
  if (!c_entries || !c_width || !c_off || !c_kmap || !S || !C_init) return QSC_EINVAL;
  if (!newton_args_ok(kind, ridge, mu0, tol, max_steps)) return QSC_EINVAL;
  const int rc = cfit_check(d, m, R, ws, ws_bytes);
  if (rc != QSC_OK) return rc;
  const int RP = qsc_rank_pad(R), G = cfit_groups(d, RP);
  CfitWs w;
  cfit_carve(d, R, RP, G, ws, &w);
  const CfitParams pr = {ridge, mu0, tol, max_steps, project != 0, 0, 0, 0};
  hipStream_t hs = STREAM(stream);
  hipLaunchKernelGGL(cfit_init_kernel, dim3((unsigned)ceil_div(d->K, 256)), dim3(256), 0, hs, w, pr,
                     R, d->K, C_init);
  QSC_CHECK_LAUNCH();
  return cfit_walk(d, c_entries, c_width, c_off, c_kmap, m, R, RP, G, S, kind, w, hs);
}

QSC_API int qsc_cfit_iterate(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                             const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                             int32_t R, const float* S, int32_t kind, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!c_entries || !c_width || !c_off || !c_kmap || !S) return QSC_EINVAL;
  if (kind != INFO_EXPECTED && kind != INFO_OBSERVED) return QSC_EINVAL;
  const int rc = cfit_check(d, m, R, ws, ws_bytes);
  if (rc != QSC_OK) return rc;
  const int RP = qsc_rank_pad(R), G = cfit_groups(d, RP);
  CfitWs w;
  cfit_carve(d, R, RP, G, ws, &w);
  hipStream_t hs = STREAM(stream);
  const int rs = cfit_step(R, RP, d->K, G, w, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, hs);
  if (rs != QSC_OK) return rs;
  return cfit_walk(d, c_entries, c_width, c_off, c_kmap, m, R, RP, G, S, kind, w, hs);
}

QSC_API int qsc_cfit_finish(const qsc_obs_desc* d, const qsc_model* m, int32_t R, float* C_out,
                            double* f_out, int32_t* steps, float* std_C, int32_t* n_unconverged,
                            int32_t* n_unidentified, void* ws, size_t ws_bytes, void* stream) {
  if (!C_out || !n_unconverged || !n_unidentified) return QSC_EINVAL;
  const int rc = cfit_check(d, m, R, ws, ws_bytes);
  if (rc != QSC_OK) return rc;
  const int RP = qsc_rank_pad(R), G = cfit_groups(d, RP);
  CfitWs w;
  cfit_carve(d, R, RP, G, ws, &w);
  return cfit_step(R, RP, d->K, G, w, 1, C_out, f_out, steps, std_C, n_unconverged,
                   n_unidentified, STREAM(stream));
}

}  // extern "C"
