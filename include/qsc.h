/*
 * qsc.h — C ABI of libqsc_hip.so, the MI355X (gfx950) hot path of the one-bit / quantized
 * maximum-likelihood tensor factorisation of shresthasagar/quantized_spectrum_cartography.
 *
 * The reference has no native boundary: its hot path is module-level Python on torch CPU
 * tensors (qmc/quantization_model.py, qmc/quantization_model_log.py) driven by the alternating
 * solver in qmc/qmc.ipynb cell 1 (raw-JSON lines :559-645).  Each entry point below names the
 * reference function it replaces (file:line).  The Python package
 * quantized_spectrum_cartography_amd binds these symbols with ctypes.
 *
 * Conventions
 *   - every pointer argument is DEVICE memory owned by the caller (contiguous, naturally
 *     aligned), except arguments documented as host pointers (qsc_model*, qsc_obs_desc*);
 *   - the library never allocates device memory: callers size workspaces with the
 *     *_workspace_bytes() queries;
 *   - every call is asynchronous on the given hipStream_t (passed as void*), except the two
 *     calls documented as synchronous (qsc_obs_layout, qsc_device_check);
 *   - return value: 0 on success, QSC_EINVAL on a bad argument, otherwise a hipError_t.
 *
 * Tensor layouts (fp32 unless stated; "pixel" p = i*J + j, P = I*J):
 *   S   [R][P]        emitter spatial loss fields   (reference S: (R,1,I,J))
 *   C   [R][K]        emitter power spectra         (reference C: (R,K))
 *   T   [K][P]        radio map T = sum_r S_r (x) c_r (reference get_tensor output (K,I,J))
 *   Y   [K][P] int64  bin indices                   (reference quantize output)
 *   codes [K][P] u8   Y with the sampling mask folded in: 0xFF = unobserved
 */
#ifndef QSC_H_
#define QSC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSC_API __attribute__((visibility("default")))

#define QSC_OK 0
#define QSC_EINVAL 100000
#define QSC_EUNSUPPORTED 100001 /* configuration this library build does not run */
#define QSC_MAX_BOUNDS 256 /* nbins <= 255: code 0xFF is the "unobserved" sentinel */
#define QSC_MAX_R 16       /* rank bound of the fused passes */
#define QSC_UNOBSERVED 0xFF

/* Probit observation model, host struct passed by pointer.
 *   reference: F_probit qmc/quantization_model.py:57-61 (constant 1.414213, kept verbatim);
 *              prob_probit qmc/quantization_model.py:22-39 (linear: b[0]=-1e5, b[-1]=1e5 clamp)
 *              and qmc/quantization_model_log.py:23-41 (log model: no clamp);
 *              quantize qmc/quantization_model.py:8-20 / _log.py:9-21 (b[-1]=inf).
 * sigma and offset are doubles because the reference passes Python floats: the library forms
 * fp32(sigma*1.414213) and fp32(offset) exactly as torch does for a tensor-scalar op. */
typedef struct qsc_model {
  int32_t nbounds;   /* number of bin boundaries = nbins + 1, 2..QSC_MAX_BOUNDS */
  int32_t log_model; /* 0: linear model, 1: log-domain model x = log(t + offset) */
  double sigma;      /* probit noise standard deviation */
  double offset;     /* log-model offset (ignored when log_model == 0) */
  float bounds[QSC_MAX_BOUNDS]; /* bin boundaries as the caller gives them (unclamped) */
  int32_t loss;      /* QSC_LOSS_PROBIT (0), QSC_LOSS_SQUARED (1) or QSC_LOSS_LOGIT (2), see below */
  int32_t reserved_;
} qsc_model;
/* loss of the fused passes (qsc_spass / qsc_cpass):
 *   QSC_LOSS_PROBIT:  -sum_obs log P(y | x)                        qmc/qmc.ipynb :572, :631
 *   QSC_LOSS_SQUARED:  sum_obs (x - Obs)^2, Obs = (b[y] + b[y+1]) / 2 on the raw edges
 *                      (get_quantized_obs_from_ordinal, qmc/quantization_model_log.py:43-51):
 *                      the Euclidean "DowJons" criterion ||Wx (T_hat - Obs)||_F^2 of
 *                      qmc/qmc_dowjons.ipynb :142, :160 (sigma is unused).
 *   QSC_LOSS_LOGIT:   -sum_obs log P(y | x) under the logistic (ordered-logit) link
 *                      F(y) = 1 / (1 + exp(-y / s)), s = sigma  (F_sigmoid,
 *                      qmc/quantization_model.py:43-47, at s = 1):
 *                      P = F(b[y+1] - x) - F(b[y] - x) with prob_probit's edge handling (linear
 *                      model: b[0] = -1e5, b[-1] = 1e5; log model: raw edges).  sigma is the
 *                      logistic SCALE; the noise standard deviation is s pi / sqrt(3).
 * with x = t (linear) or log(t + offset) (log model); the state's nll_* fields then hold the
 * squared-loss sums (QSC_LOSS_SQUARED) or the logistic NLL (QSC_LOSS_LOGIT). */
#define QSC_LOSS_PROBIT 0
#define QSC_LOSS_SQUARED 1
#define QSC_LOSS_LOGIT 2

/* Adam hyper-parameters (torch.optim.Adam defaults: betas (0.9, 0.999), eps 1e-8).  The
 * per-step bias corrections are computed on the device from the step counters held in the
 * solver state, so one captured hipGraph can be replayed for every iteration. */
typedef struct qsc_adam {
  double lr; /* doubles: torch forms 1 - beta^step and lr / bc1 in Python floats */
  double beta1;
  double beta2;
  double eps;
  int32_t project_nonneg; /* apply x[x<0] = 0 after the step (qmc/qmc.ipynb :579) */
  int32_t pad_;
} qsc_adam;

/* Device-resident solver scalars (one struct per solve, caller-allocated device memory,
 * initialised by qsc_state_init).  Kernels read and write it; the host reads it back only
 * when it wants the cost history.  Book-keeping protocol (no extra launches per iteration):
 * every block of a kernel reads the counters it needs at its start; the one-thread updates
 * are deferred to the NEXT kernel of the other block type through `pending`:
 *   cfinish (mode 1) sets QSC_PEND_C; the next qsc_spass applies step_c += 1;
 *   qsc_spass sets QSC_PEND_SNLL (and qsc_spass mode 1 / qsc_supdate set QSC_PEND_SUPD);
 *   the next qsc_cfinish (or qsc_state_flush) reduces the S-side partials into nll_s /
 *   normsq_s, applies step_s += 1 and appends the history row of that iteration. */
#define QSC_PEND_C 1
#define QSC_PEND_SNLL 2
#define QSC_PEND_SUPD 4
typedef struct qsc_state {
  int32_t step_c;   /* Adam steps taken on C */
  int32_t step_s;   /* Adam steps taken on S */
  int32_t iter;     /* S-passes issued (outer iterations) */
  int32_t pending;  /* QSC_PEND_* flags, see above */
  float normsq_s;   /* ||S||_F^2 of the current S */
  float normsq_c;   /* ||C||_F^2 of C before the last C update */
  float nll_c;      /* NLL of the last C-pass   (-sum Wx log P, qmc/qmc.ipynb :572) */
  float nll_s;      /* NLL of the last S-pass */
  float normsq_s_prev; /* ||S||^2 the last S-pass was evaluated with */
  int32_t fused_fault; /* reserved, 0 (the fault word of round 4-5's one-launch forms, which
                          were measured slower than the launch pairs and removed) */
  uint64_t fin_ticket; /* reserved, 0 */
  float reserved[4];
} qsc_state;

/* Packed observation layout, produced by qsc_obs_layout (host struct).
 * Positions q in 0..Pp-1 are pixels re-ordered by observation count (perm[q] = pixel).
 *  S-format ("pixel slices"): for slice s (QSC_SLICE = 32 positions), position l in the slice,
 *     entry j < s_width[s]:
 *     idx = s_off[s] + (j/4)*128 + l*4 + (j%4);  value = k | code << KBITS  (code PAD = pad)
 *     (the S-pass gives each pixel two lanes, which take alternate 4-entry chunks) */
#define QSC_SLICE 32
/* Both entry arrays end with QSC_ENTRY_TAIL pad entries (counted in s_entries / c_entries) so
 * that the passes may issue their read-ahead loads without bounds branches. */
#define QSC_ENTRY_TAIL 256
/*
 *  C-format ("frequency slices" per pixel tile): tile t (PT positions), k-slice ks (64 lanes),
 *     lane l walks bin k = c_kmap[(t*nks+ks)*64 + l], entry j < c_width[t*nks+ks]:
 *     idx = c_off[t*nks+ks] + (j/4)*256 + l*4 + (j%4);  value = qlocal | code << QBITS
 *     c_kmap: per tile, the bins 0..64*nks-1 (those >= K are empty padding bins) ordered by
 *     their observation count in the tile, descending (ties: lower k first).  A wave walks its
 *     64 lists in lockstep, padded to the longest; count-sorted slices keep that padding small
 *     (C3: 24 % of the entries with k = 64*ks + l, a few % sorted).
 *     Tile rows are whole S-format slices dealt in snake order, so that every tile holds the
 *     same mix of dense and sparse positions (positions are count-sorted): row qlocal of tile t
 *     is position  g*QSC_SLICE + qlocal%QSC_SLICE,  g = i*ntiles + (i odd ? ntiles-1-t : t),
 *     i = qlocal/QSC_SLICE.
 *  narrow (wide == 0): uint16 entries, KBITS = QBITS = 12, code PAD = 15 (K, PT <= 4096, nbins <= 15)
 *  wide   (wide == 1): uint32 entries, KBITS = QBITS = 24, code PAD = 255
 *  Signed-row entries (rowfmt == 1; one-bit linear model, narrow only, set by the caller between
 *  qsc_obs_layout and qsc_obs_fill when qsc_obs_signed_rows_ok): the value is the row of the
 *  pass's LDS table directly -- with  Ko = round_up(K, 16), Qo = round_up(PT, 16):
 *  S-format  k + (code == 1 ? Ko : 0),  pads 2Ko + r;  C-format  qlocal + (code == 1 ? Qo : 0),
 *  pads 2Qo + r  (r in 0..15).  The passes stage each factor row twice, as [+row, +thr'] and
 *  [-row, -thr'] (thr' the scaled threshold), plus 16 neutral pad rows, so an entry's code is
 *  applied by the gather itself (z of code 1 is -z of code 0, exactly).
 *  List order: qsc_obs_fill writes each list in ascending k / qlocal order with its pads last;
 *  qsc_obs_schedule may then permute every list (and choose its pads' rows r) so that the lanes
 *  of each 16-lane ds_read_b128 group read rows of distinct residues mod 16 at every slot --
 *  bank-conflict-free gathers.  The passes accept either order (a list's order only changes the
 *  order its gradient terms are summed in). */
typedef struct qsc_obs_desc {
  int32_t K;      /* frequency bins in this (local) slab */
  int32_t P;      /* pixels I*J */
  int32_t Pp;     /* P rounded up to PT */
  int32_t PT;     /* C-pass pixel tile (positions), multiple of 64, <= 4096 when narrow */
  int32_t ntiles; /* Pp / PT */
  int32_t nks;    /* ceil(K / 64) */
  int32_t wide;   /* entry width selector, see above */
  int32_t nbins;  /* number of bins (codes 0..nbins-1) */
  int64_t nnz;    /* observed entries */
  int64_t s_entries; /* S-format entries incl. padding */
  int64_t c_entries; /* C-format entries incl. padding */
  int32_t rowfmt; /* 0: code-field entries; 1: signed-row entries (see above) */
  int32_t reserved_;
} qsc_obs_desc;

/* ---------------------------------------------------------------------------------------
 * library / device
 * ------------------------------------------------------------------------------------- */
QSC_API int qsc_version(void);
/* rank padding of the position-order factor layout: 4, 8 or 16 (R <= QSC_MAX_R), else 0 */
QSC_API int qsc_rank_pad(int32_t R);
QSC_API const char* qsc_error_string(int code);
/* synchronous: returns 0 if device `dev` is a gfx950 the code objects can run on */
QSC_API int qsc_device_check(int dev);

/* ---------------------------------------------------------------------------------------
 * elementwise model ops
 * ------------------------------------------------------------------------------------- */
/* quantize: qmc/quantization_model.py:8-20 (linear), qmc/quantization_model_log.py:9-21 (log).
 * noise = torch.randn(X.shape) drawn by the caller (host RNG, as in the reference);
 * x = X + noise*fp32(sigma) (linear) or log(X + offset) + noise*fp32(sigma) (log);
 * Y = i for b[i] < x <= b[i+1] (i >= 1, b[-1] = +inf), else 0.                             */
QSC_API int qsc_quantize(const float* X, const float* noise, int64_t n, const qsc_model* m,
                         int64_t* Y, void* stream);
/* bin step of quantize alone: Y = i for b[i] < x <= b[i+1] (i >= 1, b[-1] = +inf), else 0, for
 * observations x already formed by the caller.  The log model's x = log(X + offset) +
 * randn*std (qmc/quantization_model_log.py:14) is formed on the host with torch's own CPU log,
 * so that Y is bit-identical to the reference's (ocml logf and ATen's vectorised log differ by
 * an ulp on some inputs); the binning loop (qml:15-20) runs here.                            */
QSC_API int qsc_bin_codes(const float* x, int64_t n, const qsc_model* m, int64_t* Y,
                          void* stream);
/* prob_probit: qmc/quantization_model.py:22-39, qmc/quantization_model_log.py:23-41.
 * P = F(b[Y+1] - Xhat) - F(b[Y] - Xhat), F(y) = 0.5*(1 + erf(y / fp32(sigma*1.414213))). */
QSC_API int qsc_prob_probit(const int64_t* Y, const float* Xhat, int64_t n, const qsc_model* m,
                            float* P, void* stream);
/* vector-Jacobian product of prob_probit w.r.t. Xhat: gX = gP * dP/dXhat */
QSC_API int qsc_prob_probit_bwd(const int64_t* Y, const float* Xhat, const float* gP, int64_t n,
                                const qsc_model* m, float* gX, void* stream);
/* F_probit: qmc/quantization_model.py:57-61 */
QSC_API int qsc_f_probit(const float* y, int64_t n, double sigma, float* out, void* stream);
/* Logistic link (QSC_LOSS_LOGIT) counterparts of the three calls above; m->sigma / scale is the
 * logistic scale s, m->loss is not read.
 * F_logit: F(y) = 1 / (1 + exp(-y / s)); F_sigmoid, qmc/quantization_model.py:43-47, is s = 1.
 * Evaluated as exp(-|y|/s) / (1 + exp(-|y|/s)) or its complement, so neither tail overflows. */
QSC_API int qsc_f_logit(const float* y, int64_t n, double scale, float* out, void* stream);
/* prob_logit: prob_probit (qmc/quantization_model.py:22-39, qmc/quantization_model_log.py:23-41)
 * with F_logit in place of F_probit: P = F(b[Y+1] - Xhat) - F(b[Y] - Xhat), same edge clamps. */
QSC_API int qsc_prob_logit(const int64_t* Y, const float* Xhat, int64_t n, const qsc_model* m,
                           float* P, void* stream);
/* vector-Jacobian product of prob_logit w.r.t. Xhat: gX = gP * (f(w) - f(u)) / s, f = F (1 - F),
 * u = (b[Y+1] - Xhat) / s, w = (b[Y] - Xhat) / s  (the autograd backward of the lines above) */
QSC_API int qsc_prob_logit_bwd(const int64_t* Y, const float* Xhat, const float* gP, int64_t n,
                               const qsc_model* m, float* gX, void* stream);
/* mid-bin values: get_quantized_obs_from_ordinal, qmc/quantization_model_log.py:43-51 */
QSC_API int qsc_obs_from_ordinal(const int64_t* Y, int64_t n, const qsc_model* m, float* out,
                                 void* stream);
/* fold the Bernoulli sampling mask Wx (qmc/qmc.ipynb :493) into uint8 codes:
 * codes = (Wx == 0) ? 0xFF : Y.  Wx may be NULL (all observed).  Entries with Y outside
 * [0, nbins) are counted into *bad (device int32, caller zeroes it). */
QSC_API int qsc_pack_codes(const int64_t* Y, const float* Wx, int64_t n, int32_t nbins,
                           uint8_t* codes, int32_t* bad, void* stream);

/* ---------------------------------------------------------------------------------------
 * reconstruction T = sum_r S_r (x) c_r
 *   reference: outer qmc/quantization_model.py:70-77, get_tensor :79-86
 *   (qmc/quantization_model_log.py:80-96).  The r-sum is accumulated in the reference's
 *   order with separate fp32 multiply and add, so T is bit-identical to get_tensor.
 * ------------------------------------------------------------------------------------- */
QSC_API int qsc_reconstruct(const float* S, const float* C, int32_t R, int32_t P, int32_t K,
                            float* T, void* stream);
/* backward of get_tensor: dS[r][p] = sum_k gT[k][p] C[r][k], dC[r][k] = sum_p gT[k][p] S[r][p].
 * Either output may be NULL.  Deterministic (fixed-order partial sums in ws). */
QSC_API size_t qsc_reconstruct_bwd_workspace_bytes(int32_t R, int32_t P, int32_t K);
QSC_API int qsc_reconstruct_bwd(const float* gT, const float* S, const float* C, int32_t R,
                                int32_t P, int32_t K, float* dS, float* dC, void* ws,
                                size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * reductions: NMSE qmc/quantization_model.py:88-92, NMSE_LOG qmc/quantization_model_log.py:104-111
 * out2[0] = sum (f(a) - f(b))^2, out2[1] = sum f(b)^2 (fp64, device), f = identity or
 * log(. + fp32(offset)) when use_log.  a == NULL means a = reconstruct(S, C) computed on the fly
 * (fused: the map is never materialised).
 * ------------------------------------------------------------------------------------- */
QSC_API size_t qsc_reduce_workspace_bytes(int64_t n);
QSC_API int qsc_diff_sumsq(const float* a, const float* b, int64_t n, int32_t use_log,
                           double offset, double* out2, void* ws, size_t ws_bytes, void* stream);
QSC_API int qsc_map_diff_sumsq(const float* S, const float* C, const float* Ttrue, int32_t R,
                               int32_t P, int32_t K, int32_t use_log, double offset,
                               double* out2, void* ws, size_t ws_bytes, void* stream);
/* the solver's NMSE history inside the iteration sequence (NMSE(get_tensor(S, C), T_true) after
 * every S-step, qmc/qmc.ipynb :582, :637): with the state's iteration counter it = st->iter,
 * when it % every == 0 writes hist[2*(it/every - 1) + {0, 1}] = {sum (T_hat - T)^2, sum T^2}
 * (slots < cap), otherwise does nothing -- so it can be captured into every iteration of a
 * replayed hipGraph.  S_pos is the passes' position-order S [Pp][RP]; iperm[p] = the position
 * of pixel p (the inverse of qsc_obs_order's perm). */
QSC_API int qsc_map_nmse_track(const float* S_pos, const int32_t* iperm, int32_t RP,
                               const float* C, const float* Ttrue, int32_t R, int32_t P,
                               int32_t K, int32_t use_log, double offset, const qsc_state* st,
                               int32_t every, double* hist, int32_t cap, void* ws,
                               size_t ws_bytes, void* stream);
/* out[0] = sum x^2 (fp32 result, fixed order) */
QSC_API int qsc_sumsq(const float* x, int64_t n, float* out, void* ws, size_t ws_bytes,
                      void* stream);

/* ---------------------------------------------------------------------------------------
 * observation packing (one-time setup of a solve): dense codes -> sliced sparse formats.
 * The reference evaluates every (k,p) entry and multiplies unobserved ones by Wx = 0
 * (qmc/qmc.ipynb :572); the build reads only observed entries.
 * ------------------------------------------------------------------------------------- */
/* cnt[p] = number of observed k for pixel p (async) */
QSC_API int qsc_obs_count(const uint8_t* codes, int32_t K, int32_t P, int32_t* cnt, void* stream);
/* perm[q] = pixels sorted by cnt descending, stable; positions P <= q < Pp are padding (-1).
 * Pp = P rounded up to the C-pass tile PT (a multiple of 64). */
QSC_API size_t qsc_obs_order_workspace_bytes(int32_t P);
QSC_API int qsc_obs_order(const int32_t* cnt, int32_t P, int32_t Pp, int32_t* perm, void* ws,
                          size_t ws_bytes, void* stream);
/* SYNCHRONOUS: computes slice widths/offsets of both formats and the C-format bin order, and
 * fills *desc.  s_width[Pp/QSC_SLICE], s_off[Pp/QSC_SLICE + 1], c_width[ntiles*nks],
 * c_off[ntiles*nks + 1], c_kmap[ntiles*nks*64]. */
QSC_API size_t qsc_obs_layout_workspace_bytes(int32_t K, int32_t P, int32_t PT);
QSC_API int qsc_obs_layout(const uint8_t* codes, int32_t K, int32_t P, int32_t PT, int32_t nbins,
                           const int32_t* perm, const int32_t* cnt, int32_t* s_width,
                           int64_t* s_off, int32_t* c_width, int64_t* c_off, int32_t* c_kmap,
                           void* ws, size_t ws_bytes, qsc_obs_desc* desc, void* stream);
/* 1 if the signed-row entry format (rowfmt = 1) applies to this layout at rank R under model m:
 * the one-bit linear model (saturated outer edges, probit or logistic loss), narrow entries, and the doubled
 * LDS tables of every pass fit.  Passes given a rowfmt = 1 layout they cannot run return
 * QSC_EINVAL. */
QSC_API int qsc_obs_signed_rows_ok(const qsc_obs_desc* desc, int32_t R, const qsc_model* m);
QSC_API int qsc_obs_fill(const uint8_t* codes, const qsc_obs_desc* desc, const int32_t* perm,
                         const int32_t* s_width, const int64_t* s_off, const int32_t* c_width,
                         const int64_t* c_off, const int32_t* c_kmap, void* s_entries,
                         void* c_entries, void* stream);
/* Bank-conflict-free list order (qsc_sched.cuh): re-orders the filled entries of both formats in
 * place, per 16-lane group of a slice / (tile, k-slice) block, as an edge colouring of lanes x
 * row residues (each slot holds each residue ceil(count / W) times at most, once whenever the
 * group has <= W entries of that residue).  Blocks with lists longer than 256 keep their order.
 * SYNCHRONOUS (reads the longest list width); run once per packing, after qsc_obs_fill. */
QSC_API size_t qsc_obs_schedule_workspace_bytes(const qsc_obs_desc* desc);
QSC_API int qsc_obs_schedule(const qsc_obs_desc* desc, const int32_t* s_width,
                             const int64_t* s_off, const int32_t* c_width, const int64_t* c_off,
                             void* s_entries, void* c_entries, void* ws, size_t ws_bytes,
                             void* stream);
/* Host (CPU) form of one group's schedule, the same code as the device pass (tests / tools):
 * in/out are 16 lists of W uint32 entry values, lane-major; rowfmt/rows/wide describe the
 * entry values as in qsc_obs_desc (rows = K for S-format lists, PT for C-format lists).
 * Returns 0, or 1 when the group was copied unchanged (W > 256). */
QSC_API int qsc_sched_lists_host(const uint32_t* in, uint32_t* out, int32_t W, int32_t rowfmt,
                                 int32_t rows, int32_t wide);
/* gather/scatter between natural pixel order [R][P] and position order [Pp][RP]
 * (RP = qsc_rank_pad(R); rows R..RP-1 and positions of no pixel are zero-filled / ignored) */
QSC_API int qsc_perm_gather(const float* nat, const int32_t* perm, int32_t R, int32_t P,
                            int32_t Pp, float* pos, void* stream);
QSC_API int qsc_perm_scatter(const float* pos, const int32_t* perm, int32_t R, int32_t P,
                             int32_t Pp, float* nat, void* stream);

/* ---------------------------------------------------------------------------------------
 * fused likelihood + gradient passes (the hot path)
 *   per observed entry e=(k,p):  t = sum_r S[r,p] C[r,k]  (reference order),
 *   x = t (linear) or log(t + offset), P = prob_probit, nll -= log P,
 *   g = (exp(-u^2) - exp(-w^2)) / (a sqrt(pi) P) * (log ? 1/(t+offset) : 1)
 *   (QSC_LOSS_LOGIT: P = prob_logit, g = (f(u) - f(w)) / (s P) * (log ? 1/(t+offset) : 1))
 *   dS[r,p] = sum_k g C[r,k], dC[r,k] = sum_p g S[r,p]
 *   (replaces get_tensor -> log -> prob_probit -> -sum(Wx log P) -> autograd backward,
 *    qmc/qmc.ipynb :566-575 and :626-633)
 * S, mS, vS, dS are in position order [Pp][RP] (pixel-major: a position's RP = qsc_rank_pad(R)
 * values are one 16/32/64-byte row, rows r >= R zero); C, mC, vC in [R][K].
 * ------------------------------------------------------------------------------------- */
/* Pass workspace: zero it once before its first use (the S-pass keeps a slice scheduler in it
 * and leaves it zero on exit); one workspace serves one stream at a time. */
QSC_API size_t qsc_pass_workspace_bytes(const qsc_obs_desc* d, int32_t R);
/* zero the state; normsq_s = ||S||^2 of the initial S ([Pp][RP] position order; nullable: 0) */
QSC_API int qsc_state_init(qsc_state* st, const float* S, int32_t R, int32_t Pp, void* ws,
                           size_t ws_bytes, void* stream);
/* S-pass.  mode 0: write dS (NLL gradient only, no regulariser) — used by the generator/DIP
 * solvers and K-slab sharding; mode 1: fused S-step — dS + lambda_s*S/||S|| then Adam on S
 * (S, mS, vS updated in place).  Writes per-slice partials into ws (see qsc_state). */
QSC_API int qsc_spass(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                      const int64_t* s_off, const qsc_model* m, int32_t R, float* S,
                      const float* C, int32_t mode, float* dS, float* mS, float* vS,
                      const qsc_adam* adam, float lambda_s, qsc_state* st, void* ws,
                      size_t ws_bytes, void* stream);
/* K-slab S-pass (north-star sharding; the gradient half of the S-step, qmc/qmc.ipynb :626-633,
 * over this rank's bins): qsc_spass mode 0 with dS written in the reduce-scatter layout of
 * nranks chunks of chunk_slices position slices, each followed by ONE extra slice
 * (dS_rs[nranks][chunk_slices + 1][QSC_SLICE][RP]), and ||C_slab||^2 of the C it read stored in
 * element 0 of every chunk's extra slice -- so the reduce-scatter of dS_rs hands every rank the
 * summed gradient of its rows AND the global ||C||^2 the next C-step's non-squared regulariser
 * needs (no separate all-reduce).  Other extra-slice elements are left untouched (keep them 0).
 * Needs chunk_slices * nranks >= Pp / QSC_SLICE. */
QSC_API int qsc_spass_kslab(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                            const int64_t* s_off, const qsc_model* m, int32_t R, float* S,
                            const float* C, float* dS_rs, int32_t chunk_slices, int32_t nranks,
                            qsc_state* st, void* ws, size_t ws_bytes, void* stream);
/* C-pass: per-tile partial dC slab + NLL partials into ws. */
QSC_API int qsc_cpass(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                      const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m, int32_t R,
                      const float* S, const float* C, void* ws, size_t ws_bytes, void* stream);
/* Fused S-step + next C-pass (free-S solver, Adam on S): one launch equal to qsc_spass(mode 1)
 * followed by qsc_cpass at the updated S -- same partials, same state protocol -- so a solver
 * runs  cpass, cfinish, (scpass, cfinish) x (n-1), spass  for n outer iterations
 * (qmc/qmc.ipynb :562-634).  One workgroup per C-pass pixel tile: the tile's S-step results
 * feed its C-pass through LDS.  Available when qsc_scpass_supported(d, R). */
QSC_API int qsc_scpass_supported(const qsc_obs_desc* d, int32_t R);
QSC_API int qsc_scpass(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                       const int64_t* s_off, const void* c_entries, const int32_t* c_width,
                       const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                       int32_t R, float* S,
                       const float* C, float* mS, float* vS, const qsc_adam* adam,
                       float lambda_s, qsc_state* st, void* ws, size_t ws_bytes, void* stream);
/* reduce the C-pass slab (fixed order).  mode 0: write dC (NLL gradient only); mode 1: fused
 * C-step: dC + lambda_c*C/||C||, Adam on C, projection; mode 2 (IJ-slab sharding): as mode 0 and
 * dC[R*K] (dC holds R*K + 1 floats) receives this shard's ||S||^2 after the S-pass partials are
 * settled, so one all-reduce carries both.  Block 0 also records nll_c / normsq_c and settles a
 * pending S-pass (see qsc_state), appending history row [nll_c, nll_s, normsq_c, normsq_s] of
 * each completed iteration to hist (nullable).
 * normsq_c_ext (device, nullable): global ||C||^2 supplied by the caller (K-slab sharding). */
QSC_API int qsc_cfinish(const qsc_obs_desc* d, int32_t R, float* C, int32_t mode, float* dC,
                        float* mC, float* vC, const qsc_adam* adam, float lambda_c,
                        const float* normsq_c_ext, qsc_state* st, float* hist,
                        int32_t hist_cap, void* ws, size_t ws_bytes, void* stream);
/* C update from an externally reduced gradient g [R][K] (IJ-slab sharding, after the RCCL
 * all-reduce of the shards' dC): g + lambda_c*C/||C||, Adam on C, projection, with the state
 * protocol of qsc_cfinish mode 1.  normsq_s_ext (device, nullable): the all-reduced ||S||^2,
 * stored as the regulariser norm the next qsc_spass uses.  One workgroup (R*K is small). */
QSC_API int qsc_cupdate(int32_t R, int32_t K, float* C, float* mC, float* vC, const float* g,
                        const qsc_adam* adam, float lambda_c, const float* normsq_s_ext,
                        qsc_state* st, void* stream);
/* settle everything pending in st (S-pass partials, counters, history) — one block; used at
 * the end of a solve and between passes that are not followed by a qsc_cfinish. */
QSC_API int qsc_state_flush(const qsc_obs_desc* d, int32_t R, qsc_state* st, float* hist,
                            int32_t hist_cap, void* ws, size_t ws_bytes, void* stream);
/* S update from an externally reduced gradient g [Pp][RP] (K-slab sharding, after the RCCL
 * all-reduce of the partial dS): g + lambda_s*S/||S||, Adam on S, ||S_new||^2 partials, with
 * the same state protocol as the fused qsc_spass mode 1. */
QSC_API int qsc_supdate(const qsc_obs_desc* d, int32_t R, float* S, float* mS, float* vS,
                        const float* g, const qsc_adam* adam, float lambda_s, qsc_state* st,
                        void* ws, size_t ws_bytes, void* stream);
/* K-slab S update of this rank's shard (reduce-scatter of the partial dS ->
 * Adam on the owned 1/N of S -> all-gather): the slices [s0, s1) of S, mS, vS are updated from
 * g_own, the shard's reduce-scattered gradient ((s1-s0)*QSC_SLICE rows of RP floats, slice s0
 * first), exactly as qsc_supdate updates them; other slices are untouched.  Same state
 * protocol (the per-slice ||S_new||^2 partials of the shard; see qsc_slice_nsq). */
QSC_API int qsc_supdate_slices(const qsc_obs_desc* d, int32_t R, int32_t s0, int32_t s1,
                               float* S, float* mS, float* vS, const float* g_own,
                               const qsc_adam* adam, float lambda_s, qsc_state* st, void* ws,
                               size_t ws_bytes, void* stream);
/* per-slice ||S||^2 partials of every slice of S (into the pass workspace), bit-identical to
 * those qsc_supdate / qsc_supdate_slices write for the same rows: run after the all-gather of
 * the updated shards so the pending S-update settles the global ||S_new||^2 on every rank. */
QSC_API int qsc_slice_nsq(const qsc_obs_desc* d, int32_t R, const float* S, void* ws,
                          size_t ws_bytes, void* stream);
/* qsc_cpass that also writes every position slice's ||S||^2 partial (the values qsc_slice_nsq
 * writes, bit for bit) from the S tile it stages anyway: the K-slab solver's C-pass after the
 * all-gather of S, which then needs no separate qsc_slice_nsq launch. */
QSC_API int qsc_cpass_nsq(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                          const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                          int32_t R, const float* S, const float* C, void* ws, size_t ws_bytes,
                          void* stream);
/* byte offset, in the pass workspace, of the float where qsc_cpass / qsc_cpass_nsq leave ||C||^2
 * of the C they read (the fixed order of qsc_sumsq_small): a K-slab solver all-reduces it in
 * place and hands it to qsc_cfinish as normsq_c_ext.  -1 on an invalid descriptor. */
QSC_API int64_t qsc_pass_cnsq_offset(const qsc_obs_desc* d, int32_t R);
/* byte offset, in the pass workspace, of the partials qsc_cfinish / qsc_state_flush sum (for
 * tests that re-sum them).  which 0: the C-pass dC slab [ntiles][R][64 nks]; 1: the C-pass NLL
 * partials [ntiles * nks]; 2, 3: the S-pass NLL and ||S||^2 partials [Pp / QSC_SLICE].  -1 on an
 * invalid descriptor or `which`. */
QSC_API int64_t qsc_pass_part_offset(const qsc_obs_desc* d, int32_t R, int32_t which);
/* ||x||^2 into *out (fp32, fixed order), e.g. the local ||C_slab||^2 before an all-reduce */
QSC_API int qsc_sumsq_small(const float* x, int32_t n, float* out, void* stream);
/* Adam (torch.optim.Adam's update, bit for bit with torch 2.x's single-tensor CPU path) on a flat
 * buffer of n parameters p with moments m, v and gradient g, at step = st->iter: the S-pass
 * counter, i.e. the S-step this update belongs to -- the generator / DIP solver's step on Z or
 * the decoder weights (qmc/qmc.ipynb :634), which a captured hipGraph then replays for every
 * iteration. */
QSC_API int qsc_adam_flat(float* p, float* m, float* v, const float* g, int64_t n,
                          const qsc_adam* adam, const qsc_state* st, void* stream);
/* ---------------------------------------------------------------------------------------
 * Spatial smoothness prior on the loss fields (free-S solver, qsc_smooth.hip).
 *   R(S) = sum_{r<R} sum_{edges {p,p'}} rho(S_r(p) - S_r(p')) over the 4-neighbour graph of the
 *   I x J pixel grid, each edge once, no edges across the border:
 *     QSC_SMOOTH_QUAD:   rho(d) = d^2 / 2;  gradient at p: sum_n (S_r(p) - S_r(n))
 *     QSC_SMOOTH_HUBER:  rho(d) = d^2 / (2 delta) for |d| <= delta, else |d| - delta / 2
 *                        (smoothed anisotropic TV);  gradient: sum_n clamp((S_r(p) - S_r(n)) / delta, -1, 1)
 *   Replaces nothing in the reference: its only S-side regulariser is lambda_s ||Z||_F
 *   (qmc/qmc.ipynb :573, :631) and its spatial prior is the generator / decoder itself.  The
 *   free-S solver adds smooth * R(S) to the cost of both steps and runs its S-step as
 *   qsc_spass (mode 0) -> qsc_smooth_grad -> qsc_supdate.
 * Workspace: qsc_smooth_workspace_bytes(Pp) bytes (0 when Pp is out of range) serve either call.
 * Its first int32 is the history step counter of qsc_smooth_grad and belongs to the caller: zero
 * it when a solve starts; the calls never touch the rest of its first 16 bytes.
 * ------------------------------------------------------------------------------------- */
#define QSC_SMOOTH_QUAD 0
#define QSC_SMOOTH_HUBER 1
QSC_API size_t qsc_smooth_workspace_bytes(int32_t Pp);
/* Neighbour table of the position order, once per observation set: nbr[Pp][4] int32 = the
 * positions of the left, right, upper and lower grid neighbours of position q's pixel
 * p = perm[q] = i*J + j (the inverse permutation of p-1, p+1, p-J, p+J; it is built in ws on the
 * device), -1 outside the grid; padding positions (perm[q] == -1) get four -1.  P = I*J <= Pp. */
QSC_API int qsc_smooth_neighbors(const int32_t* perm, int32_t P, int32_t Pp, int32_t I, int32_t J,
                                 int32_t* nbr, void* ws, size_t ws_bytes, void* stream);
/* dS[q][r] += weight * dR/dS[q][r] for r < R (dS as qsc_spass mode 0 wrote it; rows r >= R and
 * positions without neighbours, the padding ones among them, are not written; dS nullable:
 * penalty only) and *pen = R(S), unweighted (pen nullable when pen_hist is given).  S, dS in
 * position order [Pp][RP]; every row and neighbour row is read as whole 16-byte vectors.
 * Deterministic: wave sums, one partial per block in ws, then a fixed-order sum -- no
 * floating-point atomics.  pen_hist (nullable): a [hist_cap] float history; the row written is
 * the workspace's step counter (rows >= hist_cap are dropped, as qsc_cfinish drops its own),
 * which the call then increments on the device -- so the call can be captured into every
 * iteration of a replayed hipGraph.  (The counter is not qsc_state.iter: that one is settled
 * through the deferred `pending` protocol.)  delta is read for QSC_SMOOTH_HUBER only (> 0).
 * QSC_EUNSUPPORTED when Pp exceeds the supported 2^28 positions. */
QSC_API int qsc_smooth_grad(const float* S, const int32_t* nbr, int32_t R, int32_t Pp,
                            int32_t kind, float delta, float weight, float* dS, float* pen,
                            float* pen_hist, int32_t hist_cap, void* ws, size_t ws_bytes,
                            void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-pixel confidence from Fisher information (qsc_info.hip).
 *   Conditional on C, the Hessian of the NLL with respect to S is block diagonal: position q has
 *     J_q = sum_{k observed at q} h(k, q) c_k c_k^T,  c_k = C[:, k]                   (R x R)
 *   with h the curvature of one entry's -log P in t = T_hat[k, q].  In the model domain x
 *   (x = t, or log(t + offset)), with phi = F' the link's density:
 *     P   = F(hi - x) - F(lo - x)           (the edge handling of prob_probit / prob_logit)
 *     P'  = -(phi(hi - x) - phi(lo - x)),  P'' = phi'(hi - x) - phi'(lo - x),  g_x = -P'/P
 *     QSC_INFO_OBSERVED:  h_x = (P'/P)^2 - P''/P at the entry's own code (what a double backward
 *                         of the NLL gives)
 *     QSC_INFO_EXPECTED:  h_x = sum_b (P_b')^2 / P_b over all nbins bins, bins with P_b == 0
 *                         dropped: independent of the code and >= 0, the Fisher information of
 *                         the Cramer-Rao bound
 *     probit: a = fp32(sigma * 1.414213), phi(y) = exp(-(y/a)^2) / (a sqrt(pi)),
 *             P'' = -(2 u phi(u) - 2 w phi(w)) / a,  u = (hi - x)/a, w = (lo - x)/a
 *     logit:  phi = F (1 - F) / s,  phi' = phi (1 - 2F) / s
 *     A saturated or infinite edge contributes exactly 0 to phi and to z phi; an entry whose P
 *     underflows to 0 contributes 0.
 *     linear model: h = h_x;  log model: observed h = (h_x - g_x) / (t + offset)^2 (it may be
 *     negative, so J_q may be indefinite: that is the Hessian, not an error), expected
 *     h = h_x / (t + offset)^2.
 *   C is treated as known (its R K parameters are informed by millions of entries); the C-side
 *   information and a joint covariance are not computed.  Replaces nothing in the reference,
 *   which returns point estimates only.
 * ------------------------------------------------------------------------------------- */
#define QSC_INFO_EXPECTED 0
#define QSC_INFO_OBSERVED 1
/* Information blocks J[Pp][RP][RP] (fp32, full symmetric blocks in position order,
 * RP = qsc_rank_pad(R), rows and columns >= R zero) from one walk over the S-format lists of any
 * layout qsc_obs_fill produces (narrow / wide, rowfmt 0 / 1); S in position order [Pp][RP],
 * C [R][K].  Pad entries add exactly 0; positions without observations and padding positions get
 * an all-zero block (written, not skipped).  Each block is summed by its position's two lanes in
 * list order -- no floating-point atomics, two calls agree bit for bit.  No workspace.
 * QSC_EINVAL for m->loss == QSC_LOSS_SQUARED (not a likelihood) and for a layout / model
 * mismatch; QSC_EUNSUPPORTED when C^T (K rows of RP (+4) floats) and the bin edges exceed the
 * 160 KiB of LDS. */
QSC_API int qsc_sinfo(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                      const int64_t* s_off, const qsc_model* m, int32_t R, const float* S,
                      const float* C, int32_t kind, float* J, void* stream);
/* Standard deviations from the blocks, one Cholesky of J_q + ridge I (R x R) per position:
 *   std_S[Pp][RP] = sqrt(diag((J_q + ridge I)^-1)), position order, rows >= R zero;
 *   std_T[K][P] (nullable; pixel order through perm, p = perm[q]) =
 *     sqrt(c_k^T (J_p + ridge I)^-1 c_k), the delta-method standard deviation of the map entry
 *     T_hat[k, p], observed or not.
 * A non-positive pivot marks the whole position unidentified: its std_S (rows < R) and std_T are
 * +inf, never NaN, and it is counted into *nbad (device int32, the caller zeroes it; integer
 * atomics only, so the call is deterministic).  Padding positions (perm[q] < 0) are not
 * factored and not counted; their std_S rows are written as 0.  ridge >= 0.  No workspace. */
QSC_API int qsc_info_std(const float* J, const int32_t* perm, int32_t R, int32_t P, int32_t Pp,
                         const float* C, int32_t K, float ridge, float* std_S, float* std_T,
                         int32_t* nbad, void* stream);
/* Elementwise curvature h of -log P(Y | t) in the map value t = T[i] (the device function of
 * qsc_sinfo: same formulas, same chain through log(t + offset) in the log model), kind as above;
 * Y outside [0, nbins) is clamped as qsc_prob_probit clamps it. */
QSC_API int qsc_entry_info(const int64_t* Y, const float* T, int64_t n, const qsc_model* m,
                           int32_t kind, float* H, void* stream);

/* ---------------------------------------------------------------------------------------
 * Expected information gain of planned readings, per position (qsc_design.hip): where to
 * measure next.
 *   A plan is w[K], w_k >= 0: the number of readings planned in bin k (NULL: one of every bin).
 *   Conditional on C the positions are independent, so the value of the plan at position q is
 *   a figure of that position alone, and the best n distinct sites are the top n.  With J_q the
 *   block of the readings already held (qsc_sinfo, either kind), t_kq = S[q] . c_k and h_exp the
 *   QSC_INFO_EXPECTED curvature above (it does not depend on the code a reading will return):
 *     A_q = sum_k w_k h_exp(t_kq) c_k c_k^T,   M0 = J_q + ridge I,   M1 = M0 + A_q
 *     QSC_DESIGN_D:  1/2 (logdet M1 - logdet M0)            expected entropy reduction, nats
 *     QSC_DESIGN_A:  tr(M0^-1) - tr(M1^-1)                  reduction of sum_r var(S_r)
 *     QSC_DESIGN_V:  tr(G M0^-1) - tr(G M1^-1), G = C C^T   reduction of sum_k var(T_hat[k, q])
 *   Rows and columns >= R are replaced by the identity (qsc_info_std's rule) and contribute 0.
 *   A bin with w_k == 0 adds exactly 0 and is not evaluated; in the log model an entry with
 *   t + offset <= 0 adds 0.  The factorisations are qsc_info_std's Cholesky with its pivot rule:
 *     M0 not positive definite, M1 positive definite (an unobserved position with ridge = 0):
 *       gain = +inf, a first look, counted into *n_first;
 *     M1 not positive definite (or a figure that is not finite): gain = 0, counted into *n_bad;
 *   never NaN, and never negative (a difference that rounds below 0 is written as 0).  Padding
 *   positions (perm[q] < 0) are written as 0 and not counted.
 * ------------------------------------------------------------------------------------- */
#define QSC_DESIGN_D 0
#define QSC_DESIGN_A 1
#define QSC_DESIGN_V 2
/* gain[Pp] (fp32, position order) from S [Pp][RP] (position order, RP = qsc_rank_pad(R)),
 * C [R][K], the blocks J[Pp][RP][RP] of qsc_sinfo and perm[Pp] as qsc_info_std; w[K] nullable;
 * G[RP][RP] (C C^T, rows and columns >= R zero) is read for QSC_DESIGN_V only.  The walk is dense
 * over k: no observation lists are needed.  Two lanes per position, each sums alternate bins in
 * order of k; *n_first and *n_bad are device int32 the caller zeroes (integer atomics only): two
 * calls agree bit for bit.  No workspace, no allocation, stream-ordered, capturable.
 * QSC_EINVAL for m->loss == QSC_LOSS_SQUARED or a bad model, R outside [1, QSC_MAX_R], K or P < 1,
 * Pp < P or no multiple of QSC_SLICE, ridge < 0 or NaN, an unknown criterion, or G == NULL with
 * QSC_DESIGN_V; QSC_EUNSUPPORTED when C^T, the bin edges and w exceed the 160 KiB of LDS
 * (qsc_sinfo's rule with K floats more). */
QSC_API int qsc_sgain(const float* S, const float* C, const float* J, const int32_t* perm,
                      const float* w, const float* G, const qsc_model* m, int32_t R, int32_t K,
                      int32_t P, int32_t Pp, int32_t criterion, float ridge, float* gain,
                      int32_t* n_first, int32_t* n_bad, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-position goodness of fit and level-shift score tests (qsc_check.hip): are the readings of
 * a position -- a physical sensor -- consistent with the fitted model?
 *   Take position q with entries e = (k, y); pad entries are skipped.  Let t = s_q . c_k, x = t
 *   (linear model) or log(t + offset), dxdt = 1 or 1 / (t + offset).  P_b, P_b' of bin
 *   b = 0 .. nbins - 1 are qsc_sinfo's (the same device function, mirroring and saturation rules);
 *   bins with P_b == 0 are dropped from every sum over b.  Per entry:
 *     l   = -log max(P_y, FLT_MIN)
 *     H   = -sum_b P_b log P_b                   the model's own expectation of l
 *     var = max(sum_b P_b log^2 P_b - H^2, 0)    its variance
 *     g_x = -P_y' / P_y                          the score in x at the observed code; 0 if P_y == 0
 *     h_x = sum_b P_b'^2 / P_b                   QSC_INFO_EXPECTED, as qsc_sinfo
 *   Per position, with `fitted` 0 or 1:
 *     D   = sum_e (l - H)        V = sum_e var        n = entries used
 *     u   = sum_e g_x            Ixx = sum_e h_x
 *     g   = sum_e g_x dxdt c_k + ridge s_q            (R; the S-gradient of qsc_sfit's objective)
 *     v   = sum_e h_x dxdt c_k                        (R; expected cross information of shift and s)
 *     J   = sum_e h_x dxdt^2 c_k c_k^T + ridge I      (R x R; qsc_sinfo's expected block)
 *     fitted = 0:  u* = u,                I* = Ixx
 *     fitted = 1:  u* = u - v^T J^-1 g,   I* = Ixx - v^T J^-1 v   (efficient score, Schur complement)
 *   With J = L L^T one forward substitution per right-hand side is enough: a = L^-1 v, b = L^-1 g,
 *   I* = Ixx - a . a, u* = u - a . b.
 *   Under the model at the true (S, C) and with fitted = 0, D has mean 0 and variance V exactly,
 *   for any n, and u has mean 0 and variance Ixx exactly (the Fisher identity).  With fitted = 1,
 *   u* / sqrt(I*) is Neyman's C(alpha) statistic for a shift delta of the position's received level
 *   (x -> x + delta) with s_q the nuisance parameter; it is valid to first order where s_q is not
 *   exactly the conditional MLE, because g is carried.  D is not corrected for the fit: after a fit
 *   of s_q to the same readings it is biased low by about R / 2; on held-out readings with
 *   fitted = 0 it is exact.  C is treated as known, as in qsc_sinfo.
 *   The flag word of a position:
 *     QSC_CHECK_UNTESTABLE  fitted = 1 and J has a pivot that is not positive (qsc_info_std's
 *                           rule) or I* <= 1e-4 Ixx: the shift is confounded with s_q, or I* is
 *                           rounding noise (the fp32 quadratic form carries about
 *                           R 2^-24 Ixx ~ 1e-6 Ixx at R = 16; the guard is 100 x that).  u* and I*
 *                           are written as 0.  A position without entries is untestable.
 *     QSC_CHECK_INVALID     log model: an entry has t + offset <= 0.  All four statistics are
 *                           written as 0, n counts the remaining entries, and the untestable bit
 *                           is left clear (the shift test was not evaluated).
 *     QSC_CHECK_SATURATED   an entry's fp32 P_y is 0: its l is -log FLT_MIN and it adds 0 to g_x,
 *                           g and u (its H, var and h_x are added as usual).
 *   Padding positions (perm[q] < 0) get all zeros and flag 0.  Nothing is ever NaN.
 * ------------------------------------------------------------------------------------- */
#define QSC_CHECK_UNTESTABLE 1
#define QSC_CHECK_INVALID 2
#define QSC_CHECK_SATURATED 4
/* stat[Pp][4] = (D, V, u*, I*) (fp32, one 16-byte store per position), count[Pp] = n and
 * flags[Pp], all in position order, from one walk over the S-format lists of any layout
 * qsc_obs_fill produces (qsc_sinfo's walk: two lanes per position, alternate entry pairs in list
 * order, one lane exchange); S in position order [Pp][RP], C [R][K], perm[Pp] as qsc_info_std.
 * Per-entry terms are fp32; D and V are summed in fp64 (l - H cancels), the rest in fp32.  No
 * workspace, no allocation, no atomics: two calls agree bit for bit; stream-ordered, capturable.
 * QSC_EINVAL for m->loss == QSC_LOSS_SQUARED or a bad model, a layout / model mismatch
 * (qsc_sinfo's checks), ridge < 0 or NaN, or fitted outside {0, 1}; QSC_EUNSUPPORTED by
 * qsc_sinfo's LDS rule. */
QSC_API int qsc_scheck(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                       const int64_t* s_off, const int32_t* perm, const qsc_model* m, int32_t R,
                       const float* S, const float* C, int32_t fitted, float ridge, float* stat,
                       int32_t* count, int32_t* flags, void* stream);
/* Elementwise terms of the walk above at the map value t = T[i] and the code Y[i] (the same device
 * function): out[5][n] (fp32) = l - H, var, g_x, h_x, dxdt.  Y outside [0, nbins) is clamped as
 * qsc_entry_info clamps it; in the log model an element with t + offset <= 0 gets five zeros. */
QSC_API int qsc_entry_check(const int64_t* Y, const float* T, int64_t n, const qsc_model* m,
                            float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-pixel damped Newton / Fisher-scoring fit of the loss fields for known spectra (qsc_sfit.hip).
 *   Conditional on C the likelihood separates over positions.  Position q minimises over
 *   s = S[q][0..R)
 *     f_q(s) = sum_{entries (k, code) of q} -log max(P(code | t = s . c_k), FLT_MIN)
 *              + ridge / 2 |s|^2
 *   with P, the edges, the log-model chain and the saturation rules of qsc_sinfo above (convex in
 *   the linear model: both links are log-concave).  Per entry f += -log max(P, FLT_MIN),
 *   g += g_t c_k with g_t = -P'/P dx/dt, J += h c_k c_k^T with h the entry curvature of `kind`
 *   (QSC_INFO_OBSERVED: Newton; QSC_INFO_EXPECTED: Fisher scoring, J >= 0).  A pad entry adds
 *   exactly 0; an entry with P == 0 adds 0 to g, J and -log FLT_MIN to f; in the log model an
 *   entry with t + offset <= 0 makes f_q = +inf (such a trial point is rejected).
 *   One launch runs, per position (two lanes; the walk of qsc_sinfo):
 *     evaluate (f, g, J) at s = S_init[q];  mu = mu0
 *     repeat up to max_steps times:
 *       solve (J + (ridge + mu) I) delta = g + ridge s   (Cholesky in registers)
 *       s' = s - delta;  project != 0: s' = max(s', 0)
 *       a pivot that is not positive: the step counts as rejected
 *       evaluate (f', g', J') at s'
 *       accept iff f' <= f and f' is finite: s <- s', mu <- max(mu / 10, mu0 == 0 ? 0 : mu_min)
 *       else mu <- max(10 mu, mu_min)                                      mu_min = 1e-6
 *       converged once an accepted step has |s' - s|_inf <= tol (1 + |s|_inf)
 *   A converged position stops changing; a wave ends when all its positions have converged.
 *   f is evaluated in fp64 (from the fp32 s, C and edges) so that the accept test resolves the
 *   decreases |g|^2 / lambda of the last steps; g and J are fp32.
 * ------------------------------------------------------------------------------------- */
/* Bytes of workspace qsc_sfit needs for this layout and rank: 0 for R <= 8 (the state before a
 * trial step stays in registers); for R > 8 one row of the accepted (g, J) per lane of the grid
 * (at most a few tens of MB, independent of P beyond that). */
QSC_API size_t qsc_sfit_workspace_bytes(const qsc_obs_desc* d, int32_t R);
/* S_out[Pp][RP] (position order, RP = qsc_rank_pad(R); rows >= R and padding positions zero;
 * S_out may alias S_init) = the iteration above from S_init[Pp][RP], over the S-format lists of
 * any layout qsc_obs_fill produces; perm[Pp] as qsc_info_std (perm[q] < 0: a padding position);
 * C [R][K].  f_out[Pp] (nullable): the final f_q, ridge term included (0 for padding);
 * steps[Pp] (nullable, int32): the trial evaluations the position used (<= max_steps; the
 * evaluation at S_init is not counted).  *n_unconverged, *n_unidentified: device int32 counters
 * the caller zeroes, each incremented by one integer atomic per wave:
 *   n_unconverged   positions that had not converged after max_steps;
 *   n_unidentified  positions where, at every step, a pivot p of J + (ridge + mu) I had p <= mu,
 *                   i.e. J + ridge I itself had no positive pivot there (for mu = 0: the pivot
 *                   was not positive at every step) -- no observations and ridge = 0, say; such
 *                   a position returns S_init unchanged (its g is 0).
 * Padding positions are never counted.  Every sum is in list order -- no floating-point atomics;
 * two calls agree bit for bit.  Stream-ordered, never allocates, capturable into a hipGraph.
 * QSC_EINVAL for m->loss == QSC_LOSS_SQUARED, ridge < 0, mu0 < 0, tol <= 0, max_steps < 1, an
 * unknown kind, a layout / model mismatch or a workspace smaller than
 * qsc_sfit_workspace_bytes; QSC_EUNSUPPORTED when C^T and the edges exceed the 160 KiB of LDS
 * (qsc_sinfo's rule). */
QSC_API int qsc_sfit(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                     const int64_t* s_off, const int32_t* perm, const qsc_model* m, int32_t R,
                     const float* C, const float* S_init, int32_t kind, float ridge, float mu0,
                     float tol, int32_t max_steps, int32_t project, float* S_out, float* f_out,
                     int32_t* steps, int32_t* n_unconverged, int32_t* n_unidentified, void* ws,
                     size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Newton fit of the loss fields under the smoothness prior: red-black visits (qsc_sfit_smooth.hip).
 *   The prior weight * R(S) (qsc_smooth_grad above) couples each pixel to its 4 grid neighbours.
 *   That graph is bipartite in the colour (i + j) & 1 of pixel p = i*J + j: with the rows of the
 *   other colour held fixed, the own-colour positions are independent again.  Position q of
 *   colour c minimises over s = S[q][0..R)
 *     phi_q(s) = f_q(s) + weight * sum_{n in N(q)} sum_{r<R} rho(s_r - S[n][r])
 *   with f_q qsc_sfit's objective (ridge included), N(q) the 2..4 existing entries of nbr[q] (all
 *   of colour 1 - c) and rho of QSC_SMOOTH_QUAD / _HUBER.  Every edge joins the two colours, so
 *     sum_{q of colour c} phi_q + sum_{q of colour 1 - c} f_q
 *       = F(S) = NLL + ridge / 2 |S|^2 + weight * R(S),   each edge once:
 *   a visit in which every position accepts a step only when its own phi_q does not increase
 *   leaves F non-increasing, and alternating the colours is block coordinate descent on F
 *   (convex under the linear model).
 *   One launch is one visit of one colour, in place on S[Pp][RP] (position order).  Position q
 *   takes part iff p = perm[q] >= 0 and ((p / J) + (p % J)) & 1 == color; positions of the other
 *   colour and padding positions are neither changed nor written.  The neighbour rows a visit
 *   reads are of the other colour, so no row read as a neighbour is written in the same launch:
 *   no race, no second buffer, no dependence on grid or wave order.
 *   Per own-colour position: qsc_sfit's walk gives (f, g, J) of f_q at the trial point; then each
 *   existing neighbour n (in the order left, right, up, down) and each r < R adds, with
 *   d = s_r - S[n][r]:
 *     f    += weight * rho(d)     in fp64 from the fp32 operands
 *     g_r  += weight * rho'(d)    QUAD: d;   HUBER: clamp(d / delta, -1, 1)
 *     J_rr += weight * kappa(d)   QUAD: 1;   HUBER: 1 / max(|d|, delta), the half-quadratic
 *                                 majoriser (rho'' for |d| <= delta, positive outside, so that a
 *                                 step is defined where rho'' = 0)
 *   and qsc_sfit's iteration runs on (phi, g, J) unchanged:
 *     evaluate at s = S[q];  mu = mu0   (mu restarts every visit; no per-position state is kept
 *                                        between launches)
 *     repeat up to inner_steps times:
 *       solve (J + (ridge + mu) I) delta = g + ridge s;  s' = s - delta;  project: s' = max(s', 0)
 *       a pivot that is not positive: the step counts as rejected
 *       evaluate (phi', g', J') at s'
 *       accept iff phi' <= phi and phi' is finite: s <- s', mu <- max(mu / 10, mu0 == 0 ? 0 : mu_min)
 *       else mu <- max(10 mu, mu_min)                                       mu_min = 1e-6
 *       converged once an accepted step has |s' - s|_inf <= tol (1 + |s|_inf)
 *   The neighbour rows are re-read (16-byte vectors, from the cache) after every walk; nothing of
 *   them is staged in LDS or registers.
 * ------------------------------------------------------------------------------------- */
/* Bytes of workspace qsc_sfit_smooth needs: qsc_sfit_workspace_bytes' rule (0 for R <= 8; for
 * R > 8 one row of the accepted (g, J) per lane of the grid, reused across slices). */
QSC_API size_t qsc_sfit_smooth_workspace_bytes(const qsc_obs_desc* d, int32_t R);
/* One visit of colour `color` (0 or 1), in place on S.  nbr[Pp][4]: qsc_smooth_neighbors' table
 * of the same perm (-1: no neighbour; an entry outside [0, Pp) is read as none); I * J == d->P.
 * Lists, perm, m, R, C, kind, ridge, mu0, tol, project as qsc_sfit; smooth_kind, delta, weight as
 * qsc_smooth_grad (delta is read for QSC_SMOOTH_HUBER only; weight = 0 makes a visit qsc_sfit's
 * iteration on the colour's positions).  Outputs, written for own-colour positions only:
 *   f_out[Pp]   (nullable) the final phi_q;
 *   nll_out[Pp] (nullable) its likelihood part alone, without the ridge and the prior: it depends
 *               on the position's own row only, so it stays valid after visits of the other colour;
 *   steps[Pp]   (nullable, int32) += the trial evaluations of this visit (the caller zeroes it);
 * and device int32 counters the caller zeroes, each incremented by one integer atomic per wave:
 *   n_moved        own-colour positions whose row changed over the visit by more than
 *                  tol (1 + |s_start|_inf) in the infinity norm;
 *   n_unconverged  those that had not converged after inner_steps;
 *   n_unidentified qsc_sfit's pivot rule on the matrix with the prior's diagonal: a position
 *                  without observations at ridge 0 is identified through its neighbours.
 * No floating-point atomics; two calls from the same S agree bit for bit.  Stream-ordered, never
 * allocates, capturable into a hipGraph.  QSC_EINVAL for everything qsc_sfit rejects and for
 * color outside {0, 1}, weight < 0, an unknown smooth_kind, HUBER with delta <= 0,
 * inner_steps < 1, I * J != d->P or a workspace smaller than qsc_sfit_smooth_workspace_bytes;
 * QSC_EUNSUPPORTED by qsc_sfit's LDS rule (the neighbour rows take no LDS) and beyond
 * qsc_smooth_grad's 2^28 positions. */
QSC_API int qsc_sfit_smooth(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                            const int64_t* s_off, const int32_t* perm, const int32_t* nbr,
                            int32_t I, int32_t J, int32_t color, const qsc_model* m, int32_t R,
                            const float* C, float* S, int32_t kind, float ridge, float mu0,
                            float tol, int32_t inner_steps, int32_t project, int32_t smooth_kind,
                            float delta, float weight, float* f_out, float* nll_out,
                            int32_t* steps, int32_t* n_moved, int32_t* n_unconverged,
                            int32_t* n_unidentified, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-bin projected Newton / Fisher-scoring fit of the spectra for known loss fields (qsc_cfit.hip).
 *   Conditional on S the likelihood separates over frequency bins.  Bin k minimises over
 *   c = C[0..R)[k]
 *     f_k(c) = sum_{positions q observed in bin k} -log max(P(code | t = S[q] . c), FLT_MIN)
 *              + ridge / 2 |c|^2
 *   with P, the edges, the log-model chain, the saturation rules and the entry curvature h of
 *   `kind` exactly as qsc_sinfo / qsc_sfit above (the same device functions).  Per entry
 *   f += -log max(P, FLT_MIN), g += g_t s_q, J += h s_q s_q^T; a pad entry adds exactly 0;
 *   P == 0 adds 0 to g and J and -log FLT_MIN to f; in the log model t + offset <= 0 makes
 *   f = +inf.  The iteration starts at c = C_init[:, k], mu = mu0 and repeats up to max_steps times:
 *     gamma = g + ridge c;  held set A = {r : c_r <= 0 and gamma_r > 0} with project, else empty
 *     solve (J + (ridge + mu) I) delta = gamma with the rows and columns of A replaced by the
 *       identity and gamma_A = 0, so delta_A = 0   (a two-metric projected Newton step)
 *     c' = c - delta;  project != 0: c' = max(c', 0)
 *     a pivot (of the free rows) that is not positive: the step counts as rejected
 *     evaluate (f', g', J') at c'
 *     accept iff f' <= f and f' is finite: c <- c', mu <- max(mu / 10, mu0 == 0 ? 0 : mu_min)
 *     else mu <- max(10 mu, mu_min)                                         mu_min = 1e-6
 *     converged once an accepted step has |c' - c|_inf <= tol (1 + |c|_inf)
 *   A converged bin stops changing.  With project = 0 this is qsc_sfit's iteration with the roles
 *   of S and C exchanged.  f is evaluated and summed in fp64 (from the fp32 S, c and edges: the
 *   accept test compares sums of tens of thousands of terms); g and J are fp32 per partial.
 *   A bin's entries are spread over all pixel tiles of the C-format lists, so an evaluation is a
 *   walk (one workgroup per group of tiles, one partial (f, g, triangle of J) per (group, bin),
 *   the number of groups G fixed by the layout) and a step (one wave per bin: the G partials
 *   are added in ascending group order in fp64, g and J then rounded to fp32; one lane then
 *   accepts or rejects against the bin's device-resident state, factors, solves and writes the
 *   next trial column).  The calls:
 *     qsc_cfit_begin     state <- C_init, mu0 and the parameters;  walk at C_init
 *     qsc_cfit_iterate   one step, then the walk at the new trial  (call it up to max_steps times;
 *                        bins that converged or used max_steps trials no longer change, so
 *                        further calls are harmless and stopping early once no bin is active
 *                        gives the same bits)
 *     qsc_cfit_finish    accepts or rejects the last walked trial and writes the results
 *   Every call is stream-ordered, never allocates and is capturable into a hipGraph.  There are
 *   no floating-point atomics: the order of every sum is fixed by the layout, two runs agree
 *   bit for bit.  S is in position order [Pp][RP] (RP = qsc_rank_pad(R)), C_init / C_out [R][K].
 * ------------------------------------------------------------------------------------- */
/* Bytes of the workspace the three calls share (the partials of the G tile groups, at most
 * 64 MiB: one group per tile while that fits, and the per-bin state: trial and accepted column,
 * f, g, J, mu, steps, flags); 0 on an invalid descriptor.  Its contents carry the fit from
 * qsc_cfit_begin to qsc_cfit_finish; one workspace serves one fit at a time. */
QSC_API size_t qsc_cfit_workspace_bytes(const qsc_obs_desc* d, int32_t R);
/* G, the number of tile groups (partials per bin) of this layout and rank: min(ntiles, 1024,
 * 64 MiB / bytes of one group's partials); group g walks tiles [g ntiles / G, (g + 1) ntiles / G).
 * 0 on an invalid descriptor. */
QSC_API int32_t qsc_cfit_groups(const qsc_obs_desc* d, int32_t R);
/* byte offset, in that workspace, of the int32 counter of bins still active (neither converged
 * nor out of steps) after the last qsc_cfit_iterate: a caller may read it back now and then and
 * stop iterating at 0 */
QSC_API int64_t qsc_cfit_active_offset(void);
/* QSC_EINVAL for m->loss == QSC_LOSS_SQUARED, ridge < 0, mu0 < 0, tol <= 0, max_steps < 1, an
 * unknown kind, a layout / model mismatch or a workspace smaller than qsc_cfit_workspace_bytes
 * (qsc_sfit's rules); QSC_EUNSUPPORTED when the S tile (PT rows of RP (+4) floats) and the edges
 * exceed the 160 KiB of LDS; QSC_EINVAL also for c_entries == NULL (the array always holds its
 * QSC_ENTRY_TAIL pads).  C_init is copied: it may be the later C_out. */
QSC_API int qsc_cfit_begin(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                           const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                           int32_t R, const float* S, const float* C_init, int32_t kind,
                           float ridge, float mu0, float tol, int32_t max_steps, int32_t project,
                           void* ws, size_t ws_bytes, void* stream);
/* (the same lists, model, R, S and kind as the qsc_cfit_begin of this workspace) */
QSC_API int qsc_cfit_iterate(const qsc_obs_desc* d, const void* c_entries, const int32_t* c_width,
                             const int64_t* c_off, const int32_t* c_kmap, const qsc_model* m,
                             int32_t R, const float* S, int32_t kind, void* ws, size_t ws_bytes,
                             void* stream);
/* C_out[R][K] = the accepted columns;  f_out[K] (nullable, fp64): the final f_k, ridge term
 * included;  steps[K] (nullable, int32): the trial evaluations the bin used (<= max_steps; the
 * evaluation at C_init is not counted);  std_C[R][K] (nullable) =
 * sqrt(diag((J + ridge I)^-1)) of the accepted block (qsc_info_std's Cholesky inverse; the
 * bound c >= 0 is ignored here: the figure is that of the unconstrained problem, also for
 * entries held at 0); a non-positive pivot gives +inf for the whole bin, never NaN.
 * *n_unconverged, *n_unidentified: device int32 counters the caller zeroes, incremented by one
 * integer atomic per bin concerned:
 *   n_unconverged   bins that had not converged;
 *   n_unidentified  bins where, at every step, a pivot p of the free rows of J + (ridge + mu) I
 *                   had p <= mu (qsc_sfit's rule) -- no observations and ridge = 0, say; such a
 *                   bin returns C_init unchanged (its g is 0). */
QSC_API int qsc_cfit_finish(const qsc_obs_desc* d, const qsc_model* m, int32_t R, float* C_out,
                            double* f_out, int32_t* steps, float* std_C, int32_t* n_unconverged,
                            int32_t* n_unidentified, void* ws, size_t ws_bytes, void* stream);

/* debug builds (QSC_DEBUG=1, _build.py --debug): the last failed bounds check in the pass
 * kernels (entry offsets, gather-table rows, lane bins; a failed check is recorded and its index
 * clamped, never trapped) as file id * 100000 + source line, 0 if none, -1 in release builds,
 * -2 if the device could not be read.  Every pass kernel file keeps a flag of its own; they are
 * asked in the order of their ids -- 1: qsc_pass_s.hip, 2: qsc_pass_c.hip, 3: qsc_pass_fused.hip
 * -- and the first flag set is returned (the line is that file's, or one of qsc_pass.cuh, which
 * holds the walks they share).  SYNCHRONOUS (device synchronise); clear != 0 resets all flags. */
QSC_API int qsc_debug_status(int32_t clear);
/* diagnostics: out[0..n) = ocml erff(x), out[n..2n) = the erf of the fused passes (erf_fast) */
QSC_API int qsc_selftest_erf(const float* x, int32_t n, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * R x R normal equations (MFMA): backup/algorithms/NMF_SPA.m:18-19 pseudo-inverse and
 * backup/algorithms/joint_opt_ae.m:404-416 regularised least squares.
 *   G[R][R] = sum_p w[p] S[r,p] S[r',p]      (w = pixel mask or NULL)     -- v_mfma_f32_16x16x4_f32
 *   B[R][K] = sum_p w[p] S[r,p] T[k,p]
 *   C = (G + lambda I)^-1 B                   (Cholesky, one workgroup)
 * ------------------------------------------------------------------------------------- */
QSC_API size_t qsc_gram_workspace_bytes(int32_t R, int32_t P, int32_t K);
QSC_API int qsc_gram(const float* S, const float* w, int32_t R, int32_t P, float* G, void* ws,
                     size_t ws_bytes, void* stream);
QSC_API int qsc_gram_rhs(const float* S, const float* T, const float* w, int32_t R, int32_t P,
                         int32_t K, float* B, void* ws, size_t ws_bytes, void* stream);
QSC_API int qsc_chol_solve(const float* G, const float* B, int32_t R, int32_t K, float lambda,
                           float* X, void* stream);

/* ---------------------------------------------------------------------------------------
 * SPA warm start and non-negative C-update.
 *   qsc_syrk:  G[K][K] = sum_p w[p] T[a,p] T[b,p]   (T row-major [K][P]; K x K Gram of the
 *              data on the f32 MFMA; deterministic)
 *   qsc_spa:   backup/algorithms/NMF_SPA.m:1-29 on Tm = T' restricted to the pixel mask w
 *              (w[p] != 0 marks an observed pixel, NULL = all): SPA (NMF_SPA.m:31-56) picks up
 *              to R frequency bins into sel[R] (-1 padded; *count = how many), then
 *              C[R][K] = rows of (inv(Sm'Sm) Sm' Tm)' after ColumnPositive, C >= 0 and
 *              unit-norm (ColumnNormalization), S[R][P] = mask * T[sel] * d (Sm' of the
 *              reference, d = the column norms removed from C).  Optional G_out[K][K] copy.
 *              K <= 4096.  Stream-ordered: *count is device memory.
 *   qsc_nnls:  backup/algorithms/joint_opt_ae.m:409-417 lsqnonneg([Q'; lambda I], [y; 0]) per
 *              bin in normal-equation form: X[:,k] = argmin_{x >= 0} ||A x - b_k||, given
 *              G = Q Q^T (R x R) and B = Q Y^T (R x K); `lambda` is added to the diagonal of G
 *              (pass the reference's lambda squared).  Lawson-Hanson active set, one thread per
 *              bin; NaN column if a passive sub-system is not positive definite.
 * ------------------------------------------------------------------------------------- */
QSC_API size_t qsc_syrk_workspace_bytes(int32_t K, int32_t P);
QSC_API int qsc_syrk(const float* T, const float* w, int32_t K, int32_t P, float* G, void* ws,
                     size_t ws_bytes, void* stream);
QSC_API size_t qsc_spa_workspace_bytes(int32_t K, int32_t P, int32_t R);
QSC_API int qsc_spa(const float* T, const float* w, int32_t K, int32_t P, int32_t R,
                    int32_t* sel, int32_t* count, float* C, float* S, float* G_out, void* ws,
                    size_t ws_bytes, void* stream);
QSC_API int qsc_nnls(const float* G, const float* B, int32_t R, int32_t K, float lambda,
                     float* X, void* stream);

/* ---------------------------------------------------------------------------------------
 * Synthetic radio maps: qmc/generate_map.m:80-113.
 *   S[r][i*J+j] = min(1, (d/d0)^-alpha[r]) * 10^(shadow[r][i*J+j]/10), d = |(j res, i res) -
 *   (loc[2r], loc[2r+1])|, then S[r] /= ||S[r]||_F (f64, fixed order; norms[r] = the norm if
 *   non-NULL) and, if db, S = 10 log10(S).  shadow: the correlated shadowing field in dB
 *   (Shadowing_data.m; drawn by circulant embedding in maps.py).  The map is then
 *   qsc_reconstruct(S, C).
 * ------------------------------------------------------------------------------------- */
QSC_API size_t qsc_map_compose_workspace_bytes(int32_t R, int32_t I, int32_t J);
QSC_API int qsc_map_compose(const float* shadow, const float* loc, const float* alpha, int32_t R,
                            int32_t I, int32_t J, float res, float d0, int32_t db, float* S,
                            float* norms, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Observation packing from a LIST of readings (csrc/qsc_obs_readings.hip): device arrays k[n],
 * p[n] (int32, pixel p = i*J + j) and code[n] (uint8 when code_bytes = 1, int32 when 4),
 * 1 <= n < 2^31, in any order; a cell (k, p) may be read any number of times, and every reading
 * is one independent observation.  The result is the packing of qsc_obs_desc above, filled from
 * the list instead of a dense codes[K][P]:
 *   - without repeated cells every output (cnt, s_width, s_off, c_width, c_off, c_kmap, *desc,
 *     s_entries, c_entries) is bit-identical to qsc_obs_count / _layout / _fill on the equivalent
 *     codes, whatever the order of the list;
 *   - with repeats, a position's S-format list holds its readings in ascending k and a (tile,
 *     bin) C-format list in ascending qlocal, equal keys in the order of the list (stable); bin
 *     order and widths follow from the counts of READINGS by the rules above; desc->nnz counts
 *     readings;
 *   - integer atomics are used for counts only: the packed bytes are a function of the list.
 * Sequence: qsc_obs_readings_count -> (qsc_obs_order, or a caller's perm) ->
 * qsc_obs_readings_layout -> qsc_obs_readings_fill -> (qsc_obs_schedule, unchanged).
 * ------------------------------------------------------------------------------------- */
/* cnt[p] = number of in-range readings of pixel p (zeroed here), and *bad (device int32, the
 * caller zeroes it) += the number of readings with k outside [0,K), p outside [0,P) or code
 * outside [0,nbins).  Nothing is ever packed from such a reading; callers raise on *bad != 0. */
QSC_API int qsc_obs_readings_count(const int32_t* k, const int32_t* p, const void* code,
                                   int32_t code_bytes, int64_t n, int32_t K, int32_t P,
                                   int32_t nbins, int32_t* cnt, int32_t* bad, void* stream);
/* bytes of `packed`, the sorted readings the caller keeps for qsc_obs_readings_fill (8 n plus
 * the segment tables: 4 (Pp + 1) + 8 ntiles 64 nks), and of the layout call's workspace (32 n
 * for the sort keys and values, the radix sort's own buffers, and the count tables); 0 for
 * arguments out of range */
QSC_API size_t qsc_obs_readings_packed_bytes(int64_t n, int32_t K, int32_t P, int32_t PT);
QSC_API size_t qsc_obs_readings_workspace_bytes(int64_t n, int32_t K, int32_t P, int32_t PT);
/* SYNCHRONOUS (as qsc_obs_layout: reads the totals): sorts the readings into both formats'
 * orders (-> packed), computes widths, offsets and the C-format bin order, and fills *desc
 * (rowfmt 0; nnz = the in-range readings).  perm must be a permutation of the pixels over the
 * Pp positions (-1 = padding), cnt the output of qsc_obs_readings_count.  *max_repeat (HOST
 * pointer, may be NULL) receives the largest number of readings of one cell.  K and PT must be
 * below 2^24 and ntiles * 64 nks below 2^31. */
QSC_API int qsc_obs_readings_layout(const int32_t* k, const int32_t* p, const void* code,
                                    int32_t code_bytes, int64_t n, int32_t K, int32_t P,
                                    int32_t PT, int32_t nbins, const int32_t* perm,
                                    const int32_t* cnt, int32_t* s_width, int64_t* s_off,
                                    int32_t* c_width, int64_t* c_off, int32_t* c_kmap,
                                    void* packed, size_t packed_bytes, void* ws, size_t ws_bytes,
                                    qsc_obs_desc* desc, int32_t* max_repeat, void* stream);
/* qsc_obs_fill's counterpart: writes s_entries / c_entries in the format desc->rowfmt from
 * `packed` (asynchronous; may be called again with another rowfmt and other entry arrays). */
QSC_API int qsc_obs_readings_fill(const void* packed, size_t packed_bytes, int64_t n,
                                  const qsc_obs_desc* desc, const int32_t* s_width,
                                  const int64_t* s_off, const int32_t* c_width,
                                  const int64_t* c_off, const int32_t* c_kmap, void* s_entries,
                                  void* c_entries, void* stream);

/* ---------------------------------------------------------------------------------------
 * Calibration of the quantiser: Newton / Fisher-scoring fit of the noise scale and of a common
 * shift of the levels, for known S and C (qsc_qfit.hip).  Not in the reference, which hard-codes
 * sigma.
 *   Two parameters theta = (tau, beta):
 *     scale  sigma = sigma0 e^tau, sigma0 = m->sigma (for QSC_LOSS_LOGIT the logistic scale); it
 *            acts through the link's divisor a = fp32(a0 e^tau), a0 = sigma0 * 1.414213 (probit)
 *            or sigma0 (logit): what a model packed with sigma0 e^tau gives;
 *     shift  every interior, finite edge becomes fp32(b_i + beta).  In the linear model the two
 *            clamp edges (-1e5, +1e5) are not shifted; in the log model every finite raw edge is
 *            and infinite ones stay (there the shift is a common gain).
 *   Given S and C the fit minimises
 *     F(theta) = sum_{packed entries} -log max(P(code | x; a, edges), FLT_MIN)
 *                + prior_scale / 2 tau^2 + prior_shift / 2 beta^2
 *   with x = t or log(t + offset), t = S[q] . c_k, and P exactly qsc_sinfo's (the same mirroring
 *   and saturation rules).  Per entry, with u = (hi - x) / a, w = (lo - x) / a on the shifted edges,
 *   psi the link's density in z-units (probit exp(-z^2) / sqrt(pi), logit F (1 - F)),
 *   du/dtau = -u and du/dbeta = 1 / a (0 for an unshifted edge):
 *     P_tau  = -(u psi(u) - w psi(w))               P_beta = (psi(u) - psi(w)) / a
 *     P_tt   = (z psi + z^2 psi')(u) - (...)(w)     P_tb   = -((psi + z psi')(u) - (...)(w)) / a
 *     P_bb   = (psi'(u) - psi'(w)) / a^2
 *     g_i = -P_i / P
 *     QSC_INFO_OBSERVED:  H_ij = P_i P_j / P^2 - P_ij / P at the entry's own code
 *     QSC_INFO_EXPECTED:  H_ij = sum_b P_i,b P_j,b / P_b over all bins, bins with P_b == 0
 *                         dropped: positive semidefinite (the default of qmc.fit_noise)
 *   A saturated or infinite edge contributes exactly 0 to psi, z psi and z^2 psi'; an entry whose
 *   fp32 P is 0 adds 0 to g and H and -log FLT_MIN to F; in the log model t + offset <= 0 makes
 *   F = +inf; a pad entry adds exactly 0.  f is fp64 per entry (from the fp32 S, C and edges, as
 *   qsc_sfit forms it), g and H fp32 per entry; all sums are fp64.
 *   An evaluation is a walk (qsc_sinfo's, over the S-format lists of any layout qsc_obs_fill /
 *   qsc_obs_readings_fill produces; it reads the trial theta from the device-resident state and
 *   forms its link and shifted edges itself) that leaves one partial of 6 doubles per slice of
 *   QSC_SLICE positions -- each lane adds its entries in list order, the two halves of a position
 *   are added, then the 32 positions with the butterfly xor 16, 8, 4, 2, 1 -- and a step of one
 *   workgroup: thread i of 256 adds the partials of slices i, i + 256, ... in ascending order, the
 *   thread sums are folded i += i + w for w = 128, 64, ..., 1 (an order fixed by the number of
 *   slices alone); then, in fp64,
 *     accept iff F' <= F and F' is finite: theta <- theta', mu <- max(mu / 10, mu0 == 0 ? 0 : mu_min)
 *     else mu <- max(10 mu, mu_min)                                          mu_min = 1e-6
 *     converged once an accepted step has |theta' - theta|_inf <= tol (1 + |theta|_inf)
 *     solve (H + diag(prior) + mu I) delta = g + prior * theta, a parameter outside fit_mask an
 *       identity row (delta = 0);  theta' = theta - delta
 *     a pivot that is not positive: the step counts as rejected; a pivot <= mu at every step:
 *       unidentified (qsc_sfit's rule)
 *   The calls (qsc_cfit's sequence):
 *     qsc_qfit_begin     state <- (tau0, beta0), mu0 and the parameters;  walk at the start
 *     qsc_qfit_iterate   one step, then the walk at the new trial (call it up to max_steps times;
 *                        a converged or exhausted fit no longer changes)
 *     qsc_qfit_finish    accepts or rejects the last walked trial and writes the results
 *   Every call is stream-ordered, never allocates and is capturable into a hipGraph.  No
 *   floating-point atomics: two runs agree bit for bit, on any grid.
 * ------------------------------------------------------------------------------------- */
#define QSC_QFIT_SCALE 1 /* fit_mask bits */
#define QSC_QFIT_SHIFT 2
#define QSC_QFIT_UNCONVERGED 1 /* flags bits of qsc_qfit_finish */
#define QSC_QFIT_UNIDENTIFIED 2
/* Bytes of the workspace the three calls share (the state and one partial of 6 doubles per
 * slice: 48 Pp / QSC_SLICE bytes); 0 on an invalid descriptor or rank.  Its contents carry the
 * fit from qsc_qfit_begin to qsc_qfit_finish; one workspace serves one fit at a time. */
QSC_API size_t qsc_qfit_workspace_bytes(const qsc_obs_desc* d, int32_t R);
/* byte offset, in that workspace, of the int32 that is 1 while the fit is active (neither
 * converged nor out of steps) after the last qsc_qfit_iterate: a caller may read it back now and
 * then and stop iterating at 0 */
QSC_API int64_t qsc_qfit_active_offset(void);
/* S in position order [Pp][RP] (RP = qsc_rank_pad(R)), C [R][K]; kind as qsc_sinfo; fit_mask a
 * non-empty union of QSC_QFIT_SCALE and QSC_QFIT_SHIFT.  QSC_EINVAL for m->loss ==
 * QSC_LOSS_SQUARED, an empty or unknown fit_mask, a negative prior or mu0, tol <= 0,
 * max_steps < 1, an unknown kind, a layout / model mismatch (qsc_sinfo's checks) or a workspace
 * smaller than qsc_qfit_workspace_bytes; QSC_EUNSUPPORTED by qsc_sinfo's LDS rule. */
QSC_API int qsc_qfit_begin(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                           const int64_t* s_off, const qsc_model* m, int32_t R, const float* S,
                           const float* C, int32_t kind, int32_t fit_mask, double prior_scale,
                           double prior_shift, double tau0, double beta0, float mu0, float tol,
                           int32_t max_steps, void* ws, size_t ws_bytes, void* stream);
/* (the same lists, model, R, S, C and kind as the qsc_qfit_begin of this workspace) */
QSC_API int qsc_qfit_iterate(const qsc_obs_desc* d, const void* s_entries, const int32_t* s_width,
                             const int64_t* s_off, const qsc_model* m, int32_t R, const float* S,
                             const float* C, int32_t kind, void* ws, size_t ws_bytes,
                             void* stream);
/* All outputs are device memory.  theta_out[2] = the accepted (tau, beta);  f_out[2] = F there
 * and F at the start, the prior terms included;  cov_out[3] (nullable) = (tt, tb, bb) of the
 * inverse of the accepted H + diag(prior) over the fitted parameters (0 in the row and column of
 * one that is not fitted), +inf on a pivot that is not positive, never NaN;  gh_out[5] (nullable)
 * = the accepted g (2) and H (3: tt, tb, bb), without the prior;  *steps (nullable) = the trial
 * evaluations used (<= max_steps; the evaluation at the start is not counted);  *flags =
 * QSC_QFIT_UNCONVERGED | QSC_QFIT_UNIDENTIFIED as they apply (unidentified: at every step a
 * pivot p of the fitted rows of H + diag(prior) + mu I had p <= mu -- all terms saturated and
 * no prior, say; such a fit returns the start). */
QSC_API int qsc_qfit_finish(const qsc_obs_desc* d, const qsc_model* m, int32_t R,
                            double* theta_out, double* f_out, double* cov_out, double* gh_out,
                            int32_t* steps, int32_t* flags, void* ws, size_t ws_bytes,
                            void* stream);
/* Elementwise terms of one entry at the map value t = T[i] and code Y[i] (the device functions of
 * the walk, as qsc_entry_info exposes qsc_sinfo's): out[6][n] (fp64) = f, g_tau, g_beta, H_tt,
 * H_tb, H_bb at (tau, beta); f in fp64 from the fp32 t (+inf for t + offset <= 0 in the log
 * model), g and H the fp32 values.  Y outside [0, nbins) is clamped as qsc_prob_probit clamps it. */
QSC_API int qsc_entry_calib(const int64_t* Y, const float* T, int64_t n, const qsc_model* m,
                            double tau, double beta, int32_t kind, double* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Draw readings from the model at (S, C), at the observed cells only, into the packed layout
 * that already exists (qsc_draw.hip): the primitive of the parametric bootstrap and of
 * simulation from a truth.  Not in the reference.  qsc_quantize adds noise to a dense map and
 * bins it; a draw here uses the very P_b the likelihood evaluates.
 *   One reading at bin k, pixel p (natural index i J + j), occurrence j_occ (0 for the first
 *   reading of the cell (k, p), 1 for the second, ...; always 0 for dense codes), replicate rep:
 *     t    = s_p . c_k                fp32, r ascending, by fma
 *     x    = t  (linear model)  or  log(t + offset)
 *     P_b  = qsc_sinfo's P of bin b = 0 .. nbins - 1 at x (the same device function: the edges as
 *            the likelihood forms them, the truncated 1.414213, the mirroring and saturation rules)
 *     Z    = sum_b P_b                fp32, b ascending
 *     n    = x0 >> 8,  (x0, x1, x2, x3) = Philox4x32-10(counter, key)      24 bits
 *     u    = (n + 1/2) 2^-24          0 < u < 1; as an fp32 NUMBER u would round to 1 for
 *                                     n = 2^24 - 1 (n + 1/2 has 25 bits), so u itself is never
 *                                     formed in fp32:
 *     thr  = RN_fp32((n + 1/2) 2^-24 Z)        = fma(n, Zs, Zs / 2), Zs = Z 2^-24: one rounding
 *     code = the smallest b with thr < sum_{b' <= b} P_b' (running fp32 sum, b ascending);
 *            if no bin passes (thr rounded up to the last sum), the last b with P_b > 0
 *   A bin whose fp32 P_b is 0 is never drawn (thr < cum_b and thr >= cum_{b-1} need P_b > 0), so
 *   the NLL of drawn data never meets -log FLT_MIN.  Two bins: the same rule, one comparison.
 *   Log model with t + offset <= 0: the reading keeps the code it has and *invalid (device
 *   int32; the caller zeroes it; an integer atomic) is incremented, once per reading.  A reading
 *   whose every P_b is 0 or NaN (a NaN t) keeps its code as well.  Nothing is NaN.
 *   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
 *   SC'11), all arithmetic on uint32:
 *     counter (c0, c1, c2, c3) = (k, p, j_occ, rep);  key (k0, k1) = (seed & 0xFFFFFFFF, seed >> 32)
 *     ten times:  (hi0, lo0) = 0xD2511F53 * c0   (the 64-bit product's halves)
 *                 (hi1, lo1) = 0xCD9E8D57 * c2
 *                 (c0, c1, c2, c3) = (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
 *                 (k0, k1) = (k0 + 0x9E3779B9, k1 + 0xBB67AE85)      (unused after the tenth)
 *     x0 = c0.  Known answer: the all-zero counter and key give 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 *   A reading's draw is a function of (seed, rep, k, p, j_occ) and the model at its cell alone:
 *   not of the tile, pixel order, list schedule, entry format, grid, or dense / readings input.
 * Both calls: asynchronous on `stream`, no allocation, no workspace, no floating-point atomics,
 * capturable.  QSC_EINVAL for m->loss == QSC_LOSS_SQUARED (not a likelihood) or a bad model, a
 * null pointer, R outside [1, QSC_MAX_R], replicate < 0, shapes out of range or a model / layout
 * mismatch; QSC_EUNSUPPORTED, before any launch, where a kernel's tables do not fit the LDS.
 * ------------------------------------------------------------------------------------- */
/* Dense: codes[K][P] (0xFF = unobserved) -> codes_out[K][P] (another array).  Unobserved cells
 * stay 0xFF; an observed cell gets its draw with j_occ = 0 (a code outside [0, nbins) is copied).
 * S is read as natural planes [R][P], C as [R][K]: a workgroup works on consecutive pixels of one
 * bin, so that plane reads are coalesced and c_k is uniform; position rows would need the inverse
 * pixel order and scatter.  The observed cells of a tile are compacted in LDS before the bin loop
 * (about one cell in ten is observed: a thread per cell would idle nine lanes in ten there). */
QSC_API int qsc_draw_codes(const uint8_t* codes, int32_t K, int32_t P, const qsc_model* m,
                           int32_t R, const float* S, const float* C, int64_t seed,
                           int32_t replicate, uint8_t* codes_out, int32_t* invalid, void* stream);
/* Readings: `packed` (qsc_obs_readings_layout's sorted readings, packed_bytes of them, n = d->nnz
 * readings) -> packed_out (another array of packed_bytes): the segment tables are copied, and the
 * code of every sorted reading is replaced in BOTH sorted arrays.  j_occ is a reading's place in
 * its run of equal keys (found by looking back along the run, at most max_repeat long); both
 * arrays are stable sorts of one list, so reading j_occ of a cell is the same reading in both and
 * receives the same code.  (k, p) of an S-format reading: k from the reading, the position from
 * the segment table, p = perm[position]; of a C-format reading: the bin from the tile's segment
 * table, the position from qlocal by the tile rule, p = perm[position].  S in position order
 * [Pp][RP] (the order of both arrays' keys), C [R][K], perm[Pp] as qsc_obs_readings_layout took it.
 * Follow with qsc_obs_readings_fill (and qsc_obs_schedule) on packed_out for the entry arrays. */
QSC_API int qsc_draw_readings(const void* packed, size_t packed_bytes, int64_t n,
                              const qsc_obs_desc* d, const int32_t* perm, const qsc_model* m,
                              int32_t R, const float* S, const float* C, int64_t seed,
                              int32_t replicate, void* packed_out, int32_t* invalid,
                              void* stream);
/* Listed cells: code[e] = the draw at bin k[e], pixel p[e] (natural index), occurrence occ[e]
 * (occ NULL: 0), e = 0 .. n - 1, whether the cell is observed or not -- the rule above word for
 * word, by the same device functions, so that a draw at (k, p, j_occ) is the code qsc_draw_codes /
 * qsc_draw_readings give the reading (k, p, j_occ).  There is no present code to keep: a reading
 * nothing is drawn for (log model with t + offset <= 0, counted in *invalid; every P_b zero or
 * NaN; k or p out of range) gets QSC_UNOBSERVED.  k, p, occ: device int32 lists; S natural planes
 * [R][P], C [R][K] (qsc_draw_codes' sum).  One thread per query. */
QSC_API int qsc_draw_list(const int32_t* k, const int32_t* p, const int32_t* occ, int64_t n,
                          int32_t K, int32_t P, const qsc_model* m, int32_t R, const float* S,
                          const float* C, int64_t seed, int32_t replicate, uint8_t* code,
                          int32_t* invalid, void* stream);

/* ---------------------------------------------------------------------------------------
 * Subsets of packed observations (qsc_obs_select.hip): narrow, split and read back what is
 * already packed, on the device.  Not in the reference.  Behind Observations.select / split /
 * folds / readings.
 *   THE KEEP RULE.  Reading (k, p, j_occ) of the parent (bin k, pixel p = i J + j in natural
 *   order, j_occ its occurrence number in its cell as the draws count it: 0 for dense codes) is
 *   kept iff
 *       keep_pixel[p] != 0  and  keep_bin[k] != 0  and  ((lo <= u24 < hi) != invert)
 *     keep_pixel  uint8[P], natural pixel order; NULL = all ones
 *     keep_bin    uint8[K]; NULL = all ones
 *     u24         = x0 >> 8, (x0, ..) = Philox4x32-10(counter (k, p, j_occ, 0x80000000),
 *                   key (seed & 0xFFFFFFFF, seed >> 32)): the generator of the draws above, on
 *                   a stream they never use (their word 3 is a replicate < 2^31)
 *     0 <= lo <= hi <= 2^24, invert 0 or 1;  lo = 0, hi = 2^24, invert = 0 switches the range
 *                   rule off (u24 < 2^24 always; no Philox is then evaluated)
 *   All arithmetic is on integers: there is no rounding, and a host reference is exact.  The rule
 *   reads nothing of the packing: a reading is kept or not whatever the tile, pixel order, list
 *   schedule, entry format and dense / readings input.  Complementary ranges (invert) partition
 *   the parent exactly; the ranges [(f << 24) / n, ((f + 1) << 24) / n) of f = 0 .. n - 1 tile
 *   [0, 2^24) and partition it into n folds.
 * All calls: asynchronous on `stream`, no allocation, integer atomics for *kept only (positions
 * of exported readings are decided by scans: the output bytes are a function of the input).
 * QSC_EINVAL for a null pointer, a shape out of range, a range outside 0 <= lo <= hi <= 2^24, an
 * invert other than 0 / 1, a workspace too small or a layout mismatch.
 * ------------------------------------------------------------------------------------- */
#define QSC_EXPORT_CHUNK_CODES 4096    /* cells of codes[K][P] (flat) per workgroup */
#define QSC_EXPORT_CHUNK_READINGS 1024 /* sorted readings per workgroup */
/* Dense: out[k][p] = codes[k][p] where the cell is observed and kept, 0xFF elsewhere (out is
 * another array).  *kept (device int64, zeroed by the caller) += the number of kept cells.
 * 16-byte loads when P % 16 == 0 and both arrays are 16-byte aligned, byte loads otherwise; the
 * observed cells of a chunk are compacted in LDS first, so an unobserved cell costs no Philox. */
QSC_API int qsc_select_codes(const uint8_t* codes, int32_t K, int32_t P, const uint8_t* keep_pixel,
                             const uint8_t* keep_bin, int64_t seed, int32_t lo, int32_t hi,
                             int32_t invert, uint8_t* out, int64_t* kept, void* stream);
/* Workspace of either export below over `entries` entries (K P cells, or n readings); 0 when out
 * of range.  Sized for chunks of QSC_EXPORT_CHUNK_READINGS: exact for the readings form, an upper
 * bound (about four times what it uses) for the codes form, whose chunks are four times as large. */
QSC_API size_t qsc_export_workspace_bytes(int64_t entries);
/* The kept cells of a dense codes[K][P] as three lists (int32 k, int32 p, uint8 code), ascending
 * (k, p); *n_out (device int64) = their number.  The lists need room for every observed cell
 * (the parent's nnz).  A stable stream compaction: kept count per chunk, one exclusive scan of the
 * chunk counts, the rule again with an in-chunk ballot / popcount scan and the scatter. */
QSC_API int qsc_export_codes(const uint8_t* codes, int32_t K, int32_t P, const uint8_t* keep_pixel,
                             const uint8_t* keep_bin, int64_t seed, int32_t lo, int32_t hi,
                             int32_t invert, int32_t* k_out, int32_t* p_out, uint8_t* code_out,
                             int64_t* n_out, void* ws, size_t ws_bytes, void* stream);
/* The kept readings of a list packing (`packed`, n = d->nnz readings, perm[Pp] as
 * qsc_obs_readings_layout took them), read from the S-format sorted array: the position from the
 * segment table, p = perm[position], k and the code from the reading, j_occ by looking back along
 * the run of equal k inside the position's own segment (a run may cross a chunk boundary).  Order:
 * (position, k, occurrence).  The lists need room for n readings.  The same three steps. */
QSC_API int qsc_export_readings(const void* packed, size_t packed_bytes, int64_t n,
                                const qsc_obs_desc* d, const int32_t* perm,
                                const uint8_t* keep_pixel, const uint8_t* keep_bin, int64_t seed,
                                int32_t lo, int32_t hi, int32_t invert, int32_t* k_out,
                                int32_t* p_out, uint8_t* code_out, int64_t* n_out, void* ws,
                                size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Growing a list packing (qsc_obs_append.hip): how often a cell has been read, and the append of a
 * batch of readings without re-sorting the parent.  Not in the reference.  Behind
 * Observations.occurrences / draw / append.
 *   Both sort keys of the list packing -- (position, k) and (tile, bin in k order, qlocal) --
 *   depend on the pixel order alone.  With the parent's perm kept, the batch is sorted on its own
 *   (the layout's key kernel and stable radix sort) and each sorted array of the result is the
 *   stable merge of the parent's with the batch's, parent readings first on equal keys: bit for
 *   bit what qsc_obs_readings_layout gives for the parent's readings (in qsc_export_readings'
 *   order) followed by the batch, under the same perm.  ins[i] = the number of parent readings
 *   with a key <= batch reading i's (an upper bound inside one parent segment); batch reading i
 *   goes to i + ins[i], parent reading e to e + #{i : ins[i] <= e} -- the parent's readings need
 *   neither position nor key, a chunk of QSC_MERGE_CHUNK of them bounds its search range once and
 *   stages it in LDS, and a chunk the batch does not touch is a shifted copy.  Widths, offsets, bin
 *   order and *desc come from the new counts by qsc_obs_readings_layout's own stages.  Integer
 *   arithmetic only; integer atomics for counts and max_repeat; the output bytes are a function of
 *   the inputs.
 * Sequence: qsc_obs_readings_count on the batch (*bad) -> cnt = the parent's cnt + the batch's ->
 * qsc_obs_readings_merge -> qsc_obs_readings_fill -> (qsc_obs_schedule).
 * ------------------------------------------------------------------------------------- */
#define QSC_MERGE_CHUNK 1024 /* parent readings per workgroup of the merge */
/* cnt[e] = the number of readings of cell (k[e], p[e]) the parent holds, e = 0 .. m - 1 (0 for k or
 * p out of range).  Dense parent (codes != NULL; packed, iperm unused): codes[k][p] != 0xFF.  List
 * parent (codes NULL): in the S-format segment of position iperm[p] (iperm[P]: the inverse of
 * perm, -1 = no position), the upper minus the lower bound of k.  One thread per query; integer
 * only, no atomics, no allocation, asynchronous, capturable. */
QSC_API int qsc_obs_cell_counts(const uint8_t* codes, const void* packed, size_t packed_bytes,
                                int64_t n, const qsc_obs_desc* d, const int32_t* iperm,
                                const int32_t* k, const int32_t* p, int64_t m, int32_t* cnt,
                                void* stream);
/* bytes of packed_out (n + m readings) and of the merge's workspace (32 m for the batch's sort,
 * 8 m for its sorted values and ins, the radix sort's buffers, and the count tables: it follows m,
 * not n); 0 for arguments out of range (n + m >= 2^31 among them) */
QSC_API size_t qsc_obs_readings_merge_packed_bytes(int64_t n, int64_t m, int32_t K, int32_t P,
                                                   int32_t PT);
QSC_API size_t qsc_obs_readings_merge_workspace_bytes(int64_t n, int64_t m, int32_t K, int32_t P,
                                                      int32_t PT);
/* SYNCHRONOUS (as qsc_obs_readings_layout: reads the totals).  packed / n / d / perm: the parent
 * (d->nnz = n, left untouched); k, p, code (code_bytes 1 or 4): the batch, m >= 1 readings in any
 * order, repeats allowed, checked by qsc_obs_readings_count; cnt[P]: the per-pixel counts of parent
 * plus batch.  Outputs as qsc_obs_readings_layout's, for n + m readings.  *max_repeat (HOST
 * pointer): on entry the parent's, on return the result's (only cells the batch touches can have
 * grown).  QSC_EINVAL for n + m >= 2^31, a null pointer, a layout mismatch or buffers too small. */
QSC_API int qsc_obs_readings_merge(const void* packed, size_t packed_bytes, int64_t n,
                                   const qsc_obs_desc* d, const int32_t* perm, const int32_t* k,
                                   const int32_t* p, const void* code, int32_t code_bytes,
                                   int64_t m, const int32_t* cnt, int32_t* s_width, int64_t* s_off,
                                   int32_t* c_width, int64_t* c_off, int32_t* c_kmap,
                                   void* packed_out, size_t packed_out_bytes, void* ws,
                                   size_t ws_bytes, qsc_obs_desc* desc, int32_t* max_repeat,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QSC_H_ */
