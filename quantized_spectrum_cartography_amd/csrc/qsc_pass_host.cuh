// qsc_pass_host.cuh — host side of the fused passes (qsc_pass.cuh): the workspace layout, every
// LDS-size and C-pass partition rule (they call one another across the kernel families, so they
// live together), the argument checks and launch preamble common to the pass launchers, and the
// dispatch macros over (rank, entry type, likelihood kind, log model).
#pragma once
#include "qsc_pass.cuh"

namespace {

// pitch (floats) and row count of a gather table (sr: signed rows)
inline int tpitch(int R, bool sr) {
  const int RP = R <= 4 ? 4 : (R <= 8 ? 8 : 16);
  return (sr || RP > 4) ? RP + 4 : 4;
}
inline size_t trows(int rows, bool sr) { return sr ? (size_t)sr_rows(rows) : (size_t)rows; }
// floats of a gather table
inline size_t tfloats(int rows, int R, bool sr) { return trows(rows, sr) * tpitch(R, sr); }

// LDS bytes of cpass_tile_kernel
size_t cpass_tile_lds(int PT, int R, int nks, int NP, bool sr) {
  const size_t U = (size_t)nks * NP;
  return tfloats(PT, R, sr) * 4 + 2 * 256 * 4 + (NP > 1 ? U * R * 64 * 4 : 0) +
         std::max<size_t>(U, 16) * 4;
}

// LDS bytes of scfused_kernel
size_t scfused_lds(int PT, int R, int K, int nks, int NP, bool sr) {
  const size_t U = (size_t)nks * NP;
  return 32 + tfloats(K, R, sr) * 4 + 256 * 8 + tfloats(PT, R, sr) * 4 +
         (NP > 1 ? U * R * 64 * 4 : 0) + std::max<size_t>(U, 16) * 4;
}

// The C-pass tile partition of a layout: NP parts per bin list, up to 16 waves per tile, while
// a part keeps >= QSC_CPART_MIN_CHUNKS 4-entry chunks and, at the signed-row size (the same NP
// for both row formats), the tile form's LDS fits and so does the fused launch's where it can
// fit at all; true when the tile form applies (>= 4 units, LDS fits at the layout's own row
// format `sr`)
// rank 16: units (k-slices x parts) per tile at most -- 8, one per wave of the 8-wave
// workgroups: c4k K-slab C-pass 24.8 us at 16 units (two per wave), 22.6 us at 8, 22.7 us with
// 12 units on 12-wave workgroups (profiles/r06/r16/ab_r16_units_waves.log)
#ifndef QSC_R16_UNITS
#define QSC_R16_UNITS 8
#endif
bool tile_parts(const qsc_obs_desc* d, int R, bool sr, int* np) {
  const int nks = d->nks;
  const int maxu = R > 8 ? QSC_R16_UNITS : QSC_CTILE_MAXW;
  int NP = nks >= maxu ? 1 : maxu / nks;
  const double chunks = (double)d->nnz / ((double)d->ntiles * d->K) / 4.0;
  const bool fused = scfused_lds(d->PT, R, d->K, nks, 1, true) <= 160 * 1024;
  while (NP > 1 && (chunks / NP < QSC_CPART_MIN_CHUNKS ||
                    cpass_tile_lds(d->PT, R, nks, NP, true) > 160 * 1024 ||
                    (fused && scfused_lds(d->PT, R, d->K, nks, NP, true) > 160 * 1024)))
    --NP;
  *np = NP;
  return QSC_CPASS_TILE && nks * NP >= 4 && cpass_tile_lds(d->PT, R, nks, NP, sr) <= 160 * 1024;
}

// ---- workspace layout ----
struct PassWs {
  float* slab;      // ntiles * R * Kp
  float* cnll;      // ntiles * nks
  float* snll;      // nslices
  float* snsq;      // nslices
  double* init;     // 256
  int* sched;       // S-pass queue counters [kSchedQ] + finished-wave counter (zero between launches)
  float* cnsq;      // ||C||^2 of the C the last C-pass read (written by the C-pass)
  AdamCache* acache;  // [0..1] S-side, [2..3] C-side step scalars (adam_scalars_cached)
};

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

PassWs carve(const qsc_obs_desc* d, int R, void* ws) {
  char* w = (char*)ws;
  PassWs p;
  const int64_t Kp = (int64_t)d->nks * 64;
  p.slab = (float*)w;
  w += al((size_t)d->ntiles * R * Kp * 4);
  p.cnll = (float*)w;
  w += al((size_t)d->ntiles * d->nks * 4);
  p.snll = (float*)w;
  w += al((size_t)(d->Pp / QSC_SLICE) * 4);
  p.snsq = (float*)w;
  w += al((size_t)(d->Pp / QSC_SLICE) * 4);
  p.init = (double*)w;
  w += al(256 * 8);
  p.sched = (int*)w;
  w += al((kSchedQ + 1) * 4);
  p.cnsq = (float*)w;
  w += al(4);
  p.acache = (AdamCache*)w;
  w += al(4 * sizeof(AdamCache));
  return p;
}

size_t ws_bytes_for(const qsc_obs_desc* d, int R) {
  const int64_t Kp = (int64_t)d->nks * 64;
  return al((size_t)d->ntiles * R * Kp * 4) + al((size_t)d->ntiles * d->nks * 4) +
         2 * al((size_t)(d->Pp / QSC_SLICE) * 4) + al(256 * 8) + al((kSchedQ + 1) * 4) + al(4) +
         al(4 * sizeof(AdamCache));
}

bool desc_ok(const qsc_obs_desc* d) {
  return d && d->K >= 1 && d->P >= 1 && d->Pp >= d->P && (d->Pp % 64) == 0 && d->PT >= 64 &&
         (d->PT % 64) == 0 && d->ntiles * d->PT == d->Pp && d->nks * 64 >= d->K &&
         d->nbins >= 1;
}

int rp_of(int R) { return R <= 4 ? 4 : (R <= 8 ? 8 : 16); }

// linear model edges pre-divided by a for the scaled entry form (lik_grad2)
void scale_edges(Edges* E, int nbins, float a) {
  for (int c = 0; c < nbins; ++c)
    E->e[c] = make_float2((float)((double)E->e[c].x / a), (float)((double)E->e[c].y / a));
}

// the QSC_DEBUG bounds of a launch (Lik::dbg_*): gather-table rows and entry counts
void set_dbg(Lik& lk, const qsc_obs_desc* d, bool sr) {
  lk.dbg_rows[0] = sr ? sr_rows(d->K) : d->K;
  lk.dbg_rows[1] = sr ? sr_rows(d->PT) : d->PT;
  lk.dbg_ent[0] = d->s_entries;
  lk.dbg_ent[1] = d->c_entries;
}

// resident S-pass workgroups per CU (persistent grid); RP=16 needs twice the registers
#ifndef QSC_SPASS_BPC
#define QSC_SPASS_BPC 2
#endif

size_t cpass_lds(const qsc_obs_desc* d, int R, bool sr) {
  return tfloats(d->PT, R, sr) * 4 + 2 * 256 * 4 + (size_t)kCParts * R * 64 * 4 + kCParts * 4;
}
size_t spass_lds(const qsc_obs_desc* d, int R, bool sr) {
  return 32 + tfloats(d->K, R, sr) * 4 + (size_t)d->nbins * 8;
}
int spass_bpc(int RP) { return RP > 8 ? 2 : RP == 8 ? QSC_SPASS_BPC8 : QSC_SPASS_BPC; }

// fused S-step + next C-pass: the partition (parts per bin list) of the C-pass form qsc_cpass
// uses for this layout -- the tile form's NP, or kCParts where qsc_cpass falls back to the
// per-(tile, k-slice) form -- so that the fused launch sums every dC in the same order
int cpass_parts(const qsc_obs_desc* d, int R, bool sr) {
  int NP = 1;
  return tile_parts(d, R, sr, &NP) ? NP : kCParts;
}

// the fused launch applies (its C-pass partition and LDS fit), with or without signed rows
bool scpass_fits(const qsc_obs_desc* d, int R, bool sr) {
  const int NP = cpass_parts(d, R, sr);
  const int U = d->nks * NP;
  // any unit count: small problems (C2: one 64-bin slice, ~13 entries per bin and tile, so one
  // unit per tile) run their C-pass units on the first waves while the rest wait at the end
  return U >= 1 && U <= QSC_CTILE_MAXW && d->PT <= 4096 &&
         scfused_lds(d->PT, R, d->K, d->nks, NP, sr) <= 160 * 1024;
}

// Signed-row layouts (include/qsc.h rowfmt 1): the one-bit kind, narrow entries whose values
// reach row 2K / 2PT, and every pass form the code-field layout would use still fitting its
// LDS (the S-pass at its resident-block count; the C-pass tile form or, where that does not
// apply, the per-slice form; the fused launch where it applies)
bool sr_layout_ok(const qsc_obs_desc* d, int R) {
  if (d->wide || d->nbins != 2 || (int64_t)sr_rows(d->K) > 0x10000 ||
      (int64_t)sr_rows(d->PT) > 0x10000)
    return false;
  const int RP = rp_of(R);
  if (spass_lds(d, R, true) * spass_bpc(RP) > 160 * 1024) return false;
  int np0 = 1, np1 = 1;
  const bool tile = tile_parts(d, R, false, &np0);
  if (tile ? !tile_parts(d, R, true, &np1) : cpass_lds(d, R, true) > 160 * 1024) return false;
  if (scpass_fits(d, R, false) && !scpass_fits(d, R, true)) return false;
  return true;
}

// a launch's layout / likelihood-kind pairing: signed rows need a one-bit kind (either link)
bool rowfmt_ok(const qsc_obs_desc* d, int R, int kind) {
  if (d->rowfmt == 0) return true;
  return d->rowfmt == 1 && is_onebit_cf(kind) && sr_layout_ok(d, R);
}

// threads of the fused launch at rank R (waves: two S-step slices each, 4..16; 4..8 at rank 16;
// one slice each on tiles of at most QSC_FUSED_ONE_SLICE slices)
#ifndef QSC_FUSED_ONE_SLICE
#define QSC_FUSED_ONE_SLICE 16  // C2 (8-slice tiles, 8 waves): 133 k -> 145 k grad-steps/s
#endif
unsigned scpass_threads(const qsc_obs_desc* d, int R) {
  const int nsl = d->PT / QSC_SLICE;
  const int per = nsl <= QSC_FUSED_ONE_SLICE ? nsl : nsl / 2;
  return 64u * (unsigned)std::min(rp_of(R) > 8 ? 8 : QSC_FUSED_WAVES, std::max(4, per));
}

// the argument checks every pass launcher (qsc_spass*, qsc_cpass*, qsc_scpass) starts with; each
// adds only the checks of its own pointers
bool pass_args_ok(const qsc_obs_desc* d, const qsc_model* m, int R, const void* ws,
                  size_t ws_bytes) {
  return desc_ok(d) && m && m->nbounds - 1 == d->nbins && R >= 1 && R <= QSC_MAX_R && ws &&
         ws_bytes >= ws_bytes_for(d, R) && rowfmt_ok(d, R, lik_kind(m));
}

// what every pass launch needs from (d, m): the bin edges -- the squared loss's targets, or for
// the linear models pre-divided by a -- and the likelihood constants with the debug bounds
void pass_lik(const qsc_obs_desc* d, const qsc_model* m, Edges* E, Lik* lk) {
  make_edges(m, E);
  *lk = make_lik(m);
  set_dbg(*lk, d, d->rowfmt == 1);
  if (lik_kind(m) == LIK_SQUARED)
    make_sq_targets(m, E);
  else if (!m->log_model)
    scale_edges(E, m->nbounds - 1, lk->a);
}

}  // namespace

#if QSC_DEBUG
// the QSC_DCHECK flag of each pass kernel file (0: none failed, -2: the read failed), defined in
// that file over dbg_line_read; qsc_debug_status asks them in this order (file id 1, 2, 3)
namespace qsc {
int dbg_line_s(bool clear);
int dbg_line_c(bool clear);
int dbg_line_fused(bool clear);
}  // namespace qsc
#endif

// launch KERNEL<RP> of the rank-templated update kernels for the padded rank RP
#define QSC_LAUNCH_RP(KERNEL, RP, ...)                                  \
  do {                                                                  \
    if ((RP) == 4) hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__);          \
    else if ((RP) == 8) hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__);     \
    else hipLaunchKernelGGL(KERNEL<16>, __VA_ARGS__);                   \
  } while (0)

// dispatch over (RP, entry type, likelihood kind, log) for a kernel template K<RP,E,KIND,LOG,...>
#define QSC_DISPATCH_RP(LAUNCH, KD, LG)                                                  \
  do {                                                                                   \
    if (d->wide) {                                                                       \
      if (RP == 4) LAUNCH(4, uint32_t, KD, LG);                                          \
      else if (RP == 8) LAUNCH(8, uint32_t, KD, LG);                                     \
      else LAUNCH(16, uint32_t, KD, LG);                                                 \
    } else {                                                                             \
      if (RP == 4) LAUNCH(4, uint16_t, KD, LG);                                          \
      else if (RP == 8) LAUNCH(8, uint16_t, KD, LG);                                     \
      else LAUNCH(16, uint16_t, KD, LG);                                                 \
    }                                                                                    \
  } while (0)
// signed-row layouts (rowfmt 1) are narrow and one-bit only
#define QSC_DISPATCH_RP_NARROW(LAUNCH, KD, LG)                                           \
  do {                                                                                   \
    if (RP == 4) LAUNCH(4, uint16_t, KD, LG);                                            \
    else if (RP == 8) LAUNCH(8, uint16_t, KD, LG);                                       \
    else LAUNCH(16, uint16_t, KD, LG);                                                   \
  } while (0)
#ifdef QSC_DEV_ONE_VARIANT  // (ISA work: only the signed-row instantiation of rank QSC_DEV_ONE_VARIANT)
#define QSC_DISPATCH_PASS(LAUNCH)                   \
  do {                                              \
    (void)kind;                                     \
    if (sr && RP == QSC_DEV_ONE_VARIANT) LAUNCH(QSC_DEV_ONE_VARIANT, uint16_t, LIK_ONEBIT_SR, false); \
    else return QSC_EUNSUPPORTED;                   \
  } while (0)
#else
#define QSC_DISPATCH_PASS(LAUNCH)                                                        \
  do {                                                                                   \
    if (sr && kind == LIK_LOGIT_ONEBIT)                                                  \
      QSC_DISPATCH_RP_NARROW(LAUNCH, LIK_LOGIT_ONEBIT_SR, false);                        \
    else if (sr) QSC_DISPATCH_RP_NARROW(LAUNCH, LIK_ONEBIT_SR, false);                   \
    else if (kind == LIK_ONEBIT) QSC_DISPATCH_RP(LAUNCH, LIK_ONEBIT, false);             \
    else if (kind == LIK_LOGIT_ONEBIT) QSC_DISPATCH_RP(LAUNCH, LIK_LOGIT_ONEBIT, false); \
    else if (kind == LIK_LOGIT_GENERAL && m->log_model)                                  \
      QSC_DISPATCH_RP(LAUNCH, LIK_LOGIT_GENERAL, true);                                  \
    else if (kind == LIK_LOGIT_GENERAL) QSC_DISPATCH_RP(LAUNCH, LIK_LOGIT_GENERAL, false); \
    else if (kind == LIK_SQUARED && m->log_model) QSC_DISPATCH_RP(LAUNCH, LIK_SQUARED, true); \
    else if (kind == LIK_SQUARED) QSC_DISPATCH_RP(LAUNCH, LIK_SQUARED, false);           \
    else if (m->log_model) QSC_DISPATCH_RP(LAUNCH, LIK_GENERAL, true);                   \
    else QSC_DISPATCH_RP(LAUNCH, LIK_GENERAL, false);                                    \
  } while (0)
#endif
