// qsc_pass.cuh — device machinery shared by the fused one-bit / quantized probit likelihood +
// gradient passes (gfx950): the tunables, the gather tables, the per-entry walks and the
// per-slice register sets.  The kernel families that include it, one translation unit each (all
// built with f32 denormals flushed, _build.py PASS_SOURCES):
//   qsc_pass_s.hip       spass_kernel                       (qsc_spass, qsc_spass_kslab)
//   qsc_pass_c.hip       cpass_kernel, cpass_tile_kernel    (qsc_cpass, qsc_cpass_nsq)
//   qsc_pass_fused.hip   scfused_kernel                     (qsc_scpass)
//   qsc_pass_finish.hip  finish / update / book-keeping kernels and the host queries
// Host-side sizing and dispatch rules: qsc_pass_host.cuh.
//
// The passes replace, per alternating-solver iteration (qmc/qmc.ipynb cell 1, :559-634):
//   T_hat = get_tensor(S, C); T_hat = log(T_hat + offset);               (:568-571, :626-629)
//   nll = -sum(Wx * log(prob_probit(Y, T_hat, b, std)))                   (:572, :631)
//   cost = nll + lambda_c*||C|| + lambda_s*||S or Z||; cost.backward()     (:573-575, :632-633)
//   optimizer.step(); C[C<0] = 0                                          (:576, :579, :634)
// with explicit gradients (include/qsc.h) over observed entries only.
//
// Work mapping (wave64):
//   S-pass: persistent grid; a wave takes 32-pixel slices (two lanes per pixel, each walking
//           half of the pixel's observed (k, code) list, S-format); S[p,:] and dS stay in
//           registers, C[:,k] is gathered from an LDS copy of C^T; the Adam update of S is
//           fused into the epilogue (no dS round trip through HBM).
//   C-pass: a 4-wave workgroup per (pixel tile, 64-bin slice); lane = bin k walking a quarter
//           of the tile's observed (pixel, code) list for k (C-format) against the tile's S rows
//           in LDS; C[:,k] and dC[:,k] stay in registers.  Per-tile dC partials go to a slab
//           that qsc_cfinish reduces in a fixed order (bitwise deterministic; no atomics).
// The per-entry math (lik_grad2, qsc_common.cuh) is branch-free and evaluates two entries per
// packed instruction where the math allows.
#pragma once
#include <algorithm>

#include "qsc_common.cuh"

using namespace qsc;

namespace {

#if QSC_DEBUG
// this file's QSC_DCHECK flag (qsc_common.cuh): without relocatable device code a __device__
// global cannot be shared, so every kernel file has its own and qsc_debug_status asks each
__device__ int g_qsc_dbg_line = 0;
// host: the flag's value (0: no check failed; -2: the read failed), cleared on request
inline int dbg_line_read(bool clear) {
  int line = 0;
  if (hipMemcpyFromSymbol(&line, HIP_SYMBOL(g_qsc_dbg_line), sizeof(int)) != hipSuccess) return -2;
  if (clear && line) {
    const int zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_qsc_dbg_line), &zero, sizeof(int)) != hipSuccess) return -2;
  }
  return line;
}
#endif

constexpr int kSBlock = 256;   // S-pass / S-update: 4 waves = 4 slices of QSC_SLICE pixels
constexpr int kSWaves = kSBlock / 64;
#ifndef QSC_CPASS_BLOCK
#define QSC_CPASS_BLOCK 512
#endif
constexpr int kCBlock = QSC_CPASS_BLOCK;  // C-pass: kCBlock/64 waves = parts of one (tile, 64-bin slice)
constexpr int kCParts = kCBlock / 64;
// C-pass tile form: a bin list is split into parts while each part keeps at least this many
// 4-entry chunks and the tile form's LDS (at the signed-row size, so that both row formats of a
// layout get the same partition) fits (tile_parts; every C-pass form and the fused launches
// share the partition).  C2: 1.5 against 3.0, 145 k -> 148 k grad-steps/s
#ifndef QSC_CPART_MIN_CHUNKS
#define QSC_CPART_MIN_CHUNKS 1.5
#endif
constexpr int kFBlock = 1024;  // qsc_cupdate's one workgroup (the C finish sizes its own)

// occupancy targets (waves per SIMD) that bound the register allocation of the passes; the
// rank-16 instances need twice the registers for the S/C row vectors
#ifndef QSC_SPASS_WAVES
#define QSC_SPASS_WAVES 4
#endif
// fused launch: waves that read their first slice before the staging barrier (see scfused)
#ifndef QSC_EARLY_WAVES
#define QSC_EARLY_WAVES 16
#endif
// fair wave priorities: a wave lowers its s_setprio level as it progresses (S-step: per slice;
// C-pass walks: per quarter of the unit's chunk range), so the SIMD
// arbiter, oldest-first among equal levels, keeps the waves of a SIMD abreast instead of
// finishing them one after another (the last wave of a phase otherwise runs alone,
// latency-bound: profiles/r05/stamps_simd.log).  A/B at C3: fused launch -0.5 us
// (profiles/r05/ab_fair_prio.log; a per-half-slice variant was within noise and is removed)
__device__ __forceinline__ void prio_level(int lvl) {  // 3 = most urgent
  if (lvl >= 3)
    __builtin_amdgcn_s_setprio(3);
  else if (lvl == 2)
    __builtin_amdgcn_s_setprio(2);
  else if (lvl == 1)
    __builtin_amdgcn_s_setprio(1);
  else
    __builtin_amdgcn_s_setprio(0);
}
// fused launch at rank <= 8: waves per workgroup (16: 128 VGPRs each; 12: 168, 3 per SIMD --
// slower, profiles/r05/ab_twelve_waves.log, with or without a software-pipelined S-step gather,
// which is removed: at 16 waves it spills)
#ifndef QSC_FUSED_WAVES
#define QSC_FUSED_WAVES 16
#endif
// C-pass parts: part p of np walks a contiguous block of its list's chunks; every C-pass form
// uses the one partition, so their sums agree bit for bit.  (Round 3's phase split of the fused
// launch -- C-pass chunks of the first S-step round's rows walked between the S-step rounds,
// which needed strided parts -- spilled at 128 VGPRs and ran slower; removed in round 6.)
#ifndef QSC_CPASS_WAVES
#define QSC_CPASS_WAVES 4
#endif
// (The stride js is always 1 since the phase split went; it stays because taking it out changes
// the code of 25 cpass_tile_kernel instantiations: profiles/split/isa_identical.txt.)
struct PartRange {
  int j0, j1, js;  // chunks j0, j0 + js, ... < j1
};
__device__ inline PartRange part_range(int W4, int p, int np) {
  return PartRange{(W4 * p) / np, (W4 * (p + 1)) / np, 1};
}
// C-pass tile form (cpass_tile_kernel): on by default; up to QSC_CTILE_MAXW waves per tile, at
// rank 16 QSC_CTILE_W16: 8 (2 per SIMD, 256 VGPRs).  At 16 waves (128 VGPRs) the rank-16 walk's
// 16-float C column, accumulators and pipelined gather rows spill 14-62 VGPRs
// (tools/isa_stats.py), which made the c4k C-pass 2.3x slower per entry than rank 8
#ifndef QSC_CPASS_TILE
#define QSC_CPASS_TILE 1
#endif
#ifndef QSC_CTILE_MAXW
#define QSC_CTILE_MAXW 16
#endif
#ifndef QSC_CTILE_W16
#define QSC_CTILE_W16 8
#endif
#ifndef QSC_CTILE_SREG
#define QSC_CTILE_SREG 4
#endif
#ifndef QSC_CTILE_CT
#define QSC_CTILE_CT 1
#endif
template <int RP, int W>
struct Occ {
  static constexpr int v = (RP > 8) ? (W > 4 ? 4 : W) : W;
};
// the persistent S-pass holds two slices' inputs in registers: rank 16 gets 256 VGPRs (2 waves
// per SIMD), rank 8 fits 128 (QSC_SPASS_BPC8 = 3 resident blocks: measured fastest of 2, 3, 4)
#ifndef QSC_SPASS_BPC8
#define QSC_SPASS_BPC8 3  // resident S-pass blocks per CU at rank 8 (3 waves per SIMD)
#endif
template <int RP, int EB, int W>
struct OccS {
  static constexpr int v = (RP > 8) ? (W > 2 ? 2 : W) : (RP == 8) ? QSC_SPASS_BPC8 : W;
};

// LDS row pitch (floats) of an RP-float gathered row: 16-B aligned for ds_read_b128 and, for
// RP >= 8, not a multiple of 32 B so that random rows spread over all 64 banks
template <int RP>
struct Pitch {
  static constexpr int v = (RP == 4) ? 4 : RP + 4;
};
// Signed-row tables keep each row's signed threshold (the dot product's seed) in the row
// itself: floats RP, RP+1 = {thr~, +0}, one 8-B LDS read per entry.  (A dense column of thr~/2
// after the rows, one 4-B read with the rows' banks spread 64 ways instead of 16, measured
// slower: 31.75 vs 30.97 us for the fused launch, the extra address VALU outweighing it.)
// table pitch of a likelihood kind
template <int RP, int KIND>
struct TP {
  static constexpr int v = is_sr(KIND) ? RP + 4 : Pitch<RP>::v;
};
// signed-row kinds (one-bit) never read the LDS edge table: the S-pass and fused launch skip
// its read and staging, so their staging waits for the C^T reads only
template <int KIND>
__device__ constexpr bool stages_edges() {
  return !is_sr(KIND);
}
// rows of a table: K (C^T) or PT (S tile), or sr_rows(rows) with signed rows (qsc_common.cuh)
template <int KIND>
__device__ __host__ __forceinline__ int table_rows(int rows) {
  return is_sr(KIND) ? sr_rows(rows) : rows;
}
// floats of a gather table of `rows` rows
template <int RP, int KIND>
__device__ __host__ __forceinline__ int table_floats(int rows) {
  return table_rows<KIND>(rows) * TP<RP, KIND>::v;
}
// the signed thresholds of rows i (+thr~) and sr_off(rows) + i (-thr~) of a signed-row table
template <int RP, int KIND>
__device__ __forceinline__ void put_th(float* tab, int rows, int i, float th) {
  constexpr int P = TP<RP, KIND>::v;
  *reinterpret_cast<float2*>(tab + i * P + RP) = make_float2(th, 0.0f);
  *reinterpret_cast<float2*>(tab + (sr_off(rows) + i) * P + RP) = make_float2(-th, 0.0f);
}
// row i of a gather table from 4-float groups v[0..RP): signed-row tables also get the threshold
// in float RP and the negated copy at row sr_off(rows) + i
template <int RP, int KIND>
__device__ __forceinline__ void put_row4(float* tab, int rows, int i, int r, const float4& v,
                                         float th) {
  constexpr int P = TP<RP, KIND>::v;
  *reinterpret_cast<float4*>(tab + i * P + r) = v;
  if constexpr (is_sr(KIND)) {
    *reinterpret_cast<float4*>(tab + (sr_off(rows) + i) * P + r) =
        make_float4(-v.x, -v.y, -v.z, -v.w);
    if (r == 0) put_th<RP, KIND>(tab, rows, i, th);
  }
}
// the kSrPadRows neutral pad rows 2 sr_off(rows) + r of a signed-row table ([0, kPadZ]: P == 1,
// g == 0 exactly), one per bank residue r (the scheduled pads of qsc_sched.cuh)
template <int RP, int KIND>
__device__ __forceinline__ void put_pad_row(float* tab, int rows) {
  if constexpr (is_sr(KIND)) {
    constexpr int P = TP<RP, KIND>::v;
    if (threadIdx.x < kSrPadRows) {
      float* row = tab + (2 * sr_off(rows) + (int)threadIdx.x) * P;
#pragma unroll
      for (int r = 0; r < RP; ++r) row[r] = 0.0f;
      *reinterpret_cast<float2*>(row + RP) = make_float2(kPadZ, 0.0f);
    }
  }
}

template <typename E>
struct Ent;
template <>
struct Ent<uint16_t> {
  static constexpr int kBits = 12;
  static constexpr uint32_t kMask = 0xFFF;
  static constexpr int kPad = 15;
  using V4 = uint2;     // 4 entries = 8 bytes
  using V2 = uint32_t;  // 2 entries (half a chunk: the S-pass lane's share)
  __device__ static __forceinline__ void unpack(const V4& v, uint32_t (&e)[4]) {
    e[0] = v.x & 0xFFFF;
    e[1] = v.x >> 16;
    e[2] = v.y & 0xFFFF;
    e[3] = v.y >> 16;
  }
  __device__ static __forceinline__ void unpack2(const V2& v, uint32_t (&e)[2]) {
    e[0] = v & 0xFFFF;
    e[1] = v >> 16;
  }
};
template <>
struct Ent<uint32_t> {
  static constexpr int kBits = 24;
  static constexpr uint32_t kMask = 0xFFFFFF;
  static constexpr int kPad = 255;
  using V4 = uint4;  // 4 entries = 16 bytes
  using V2 = uint2;  // 2 entries
  __device__ static __forceinline__ void unpack(const V4& v, uint32_t (&e)[4]) {
    e[0] = v.x;
    e[1] = v.y;
    e[2] = v.z;
    e[3] = v.w;
  }
  __device__ static __forceinline__ void unpack2(const V2& v, uint32_t (&e)[2]) {
    e[0] = v.x;
    e[1] = v.y;
  }
};

// Per-lane global access at byte offset `lo` (32 bits) from a wave-uniform base: the address is
// SGPR base + zero-extended VGPR offset (the global_load/store saddr form), so the per-access
// 64-bit address arithmetic stays on the scalar unit instead of costing VALU per load.
template <typename T>
__device__ __forceinline__ T ld_lane(const T* base, uint32_t lo) {
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + lo);
}
template <typename T>
__device__ __forceinline__ void st_lane(T* base, uint32_t lo, const T& v) {
  *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + lo) = v;
}

// LDS row of RP floats as RP/2 packed pairs (16-B reads)
template <int RP>
__device__ __forceinline__ void lds_row2(const float* base, f2v (&v)[RP / 2]) {
#pragma unroll
  for (int r = 0; r < RP; r += 4) {
    const float4 x = *reinterpret_cast<const float4*>(base + r);
    v[r / 2] = f2v{x.x, x.y};
    v[r / 2 + 1] = f2v{x.z, x.w};
  }
}

// t = sum_r own[r] * o[r], accumulated pairwise in r (RP/2 packed FMAs + one add)
template <int RP>
__device__ __forceinline__ float dot2(const f2v (&own)[RP / 2], const f2v (&o)[RP / 2]) {
  f2v d = own[0] * o[0];
#pragma unroll
  for (int j = 1; j < RP / 2; ++j) d = fma2(own[j], o[j], d);
  return d.x + d.y;
}

// z0 + sum_r own[r] * o[r]: the one-bit kind's z' with its offset seeded into the first FMA
template <int RP>
__device__ __forceinline__ float dot2z(const f2v (&own)[RP / 2], const f2v (&o)[RP / 2], float z0) {
  f2v d = fma2(own[0], o[0], f2v{z0, 0.0f});
#pragma unroll
  for (int j = 1; j < RP / 2; ++j) d = fma2(own[j], o[j], d);
  // an opaque (empty) asm on the sum keeps it one v_add_f32: without it the backend turns the
  // two entries' horizontal adds into three v_mov + a v_pk_add_f32
  float r = d.x + d.y;
  asm("" : "+v"(r));
  return r;
}

// the same with the seed pair read from a signed-row table ({thr~, +0}: no register move)
template <int RP>
__device__ __forceinline__ float dot2s(const f2v (&own)[RP / 2], const f2v (&o)[RP / 2], f2v seed) {
  f2v d = fma2(own[0], o[0], seed);
#pragma unroll
  for (int j = 1; j < RP / 2; ++j) d = fma2(own[j], o[j], d);
  float r = d.x + d.y;
  asm("" : "+v"(r));
  return r;
}

// factor the register row is pre-multiplied by: linear kinds evaluate in a scaled form
// (lik_grad2): -1/a (general), -sqrt(log2 e)/a (one-bit); the log model / squared loss use t
template <int KIND, bool LOG>
__device__ __forceinline__ float own_scale_of(const Lik& lk) {
  if (LOG || KIND == LIK_SQUARED) return 1.0f;
  return (is_onebit_cf(KIND) || is_sr(KIND)) ? -lk.ob_scale : -lk.inv_a;
}

struct Scalars {
  float coef;  // lambda / ||x||  (0 when ||x|| == 0, as torch's norm backward)
  AdamScalars as;
};

// A 4-entry chunk is processed as two packed pairs, each in two halves, the gather (pair_rows)
// and the arithmetic (pair_math): `own` is the lane's register vector (S of the pixel or C of the
// frequency bin, r-pairs), `tab` the LDS table of the other factor indexed by the entry's low
// bits.  Pad entries carry index 0 (a valid row) and code kPad; the one-bit kind moves them to
// z' = kPadZ where they contribute exactly 0, the other kinds mask them.  The NLL is accumulated
// as a pair (summed by the caller).
// (signed-row kind: the entry IS the row, whose float RP is the signed threshold -> tha/thb)
#ifndef QSC_DIAG_NOCONF_C
#define QSC_DIAG_NOCONF_C 0
#endif
#ifndef QSC_DIAG_NOCONF_S
#define QSC_DIAG_NOCONF_S 0
#endif
// Row addresses of signed-row entries (16-bit entries: the entry IS the row index).  The walks
// unpack an entry straight to its row's LDS address with one v_mad_u32_u16 (op_sel picks the
// dword's high entry): idx * pitch + the table's address, instead of a mask / shift and a
// multiply-add per entry.  (Index form in the debug and diagnostic builds, which check or
// rewrite the indices.)
#ifndef QSC_SR_ADDR
#define QSC_SR_ADDR 1
#endif
#if QSC_SR_ADDR && !QSC_DEBUG && !QSC_DIAG_NOLDS && !QSC_DIAG_NOCONF_C && !QSC_DIAG_NOCONF_S
#define QSC_SR_ADDR_ON 1
#else
#define QSC_SR_ADDR_ON 0
#endif
typedef __attribute__((address_space(3))) const char lds_char;
typedef float f4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const f4v lds_f4v;
typedef __attribute__((address_space(3))) const f2v lds_f2v;
template <typename E, int KIND>
__device__ constexpr bool sr_addr() {
  return QSC_SR_ADDR_ON && is_sr(KIND) && sizeof(E) == 2;
}
__device__ __forceinline__ uint32_t mad_u16_lo(uint32_t v, uint32_t pb, uint32_t off) {
  uint32_t r;
  asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(pb), "s"(off));
  return r;
}
__device__ __forceinline__ uint32_t mad_u16_hi(uint32_t v, uint32_t pb, uint32_t off) {
  uint32_t r;
  asm("v_mad_u32_u16 %0, %1, %2, %3 op_sel:[1,0,0,0]" : "=v"(r) : "v"(v), "v"(pb), "s"(off));
  return r;
}
// a gather table's LDS address (wave-uniform)
__device__ __forceinline__ uint32_t lds_off(const float* tab) {
  return __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(lds_char*)reinterpret_cast<const char*>(tab));
}
// RP floats at LDS address a as RP/2 packed pairs (lds_row2 on an LDS address)
template <int RP>
__device__ __forceinline__ void lds_row2_at(uint32_t a, f2v (&v)[RP / 2]) {
#pragma unroll
  for (int r = 0; r < RP; r += 4) {
    const f4v x = *(lds_f4v*)(uintptr_t)(a + 4 * r);
    v[r / 2] = f2v{x.x, x.y};
    v[r / 2 + 1] = f2v{x.z, x.w};
  }
}
// unpack 4 / 2 entries: indices, or (sr_addr) their rows' LDS byte addresses
template <int RP, typename E, int KIND>
__device__ __forceinline__ void ent_rows4(const typename Ent<E>::V4& v, uint32_t off,
                                          uint32_t (&e)[4]) {
  if constexpr (sr_addr<E, KIND>()) {
    constexpr uint32_t PB = TP<RP, KIND>::v * 4;
    e[0] = mad_u16_lo(v.x, PB, off);
    e[1] = mad_u16_hi(v.x, PB, off);
    e[2] = mad_u16_lo(v.y, PB, off);
    e[3] = mad_u16_hi(v.y, PB, off);
  } else {
    (void)off;
    Ent<E>::unpack(v, e);
  }
}
template <int RP, typename E, int KIND>
__device__ __forceinline__ void ent_rows2(const typename Ent<E>::V2& v, uint32_t off,
                                          uint32_t (&e)[2]) {
  if constexpr (sr_addr<E, KIND>()) {
    constexpr uint32_t PB = TP<RP, KIND>::v * 4;
    e[0] = mad_u16_lo(v, PB, off);
    e[1] = mad_u16_hi(v, PB, off);
  } else {
    (void)off;
    Ent<E>::unpack2(v, e);
  }
}

// TBL: the table gathered from, 0 = C^T (S-step), 1 = the S tile (C-pass)
template <int RP, typename E, int KIND, int TBL = 0>
__device__ __forceinline__ void pair_rows(uint32_t ea, uint32_t eb, const f2v (&own)[RP / 2],
                                          const float* __restrict__ tab, f2v (&oa)[RP / 2],
                                          f2v (&ob)[RP / 2], f2v& tha, f2v& thb, const Lik& lk) {
  using T = Ent<E>;
  constexpr int P = TP<RP, KIND>::v;
  constexpr int DG = TBL == 1 ? QSC_DIAG_NOCONF_C : QSC_DIAG_NOCONF_S;
  uint32_t ia = is_sr(KIND) ? ea : (ea & T::kMask), ib = is_sr(KIND) ? eb : (eb & T::kMask);
#if QSC_DEBUG
  {
    const uint32_t lim = (uint32_t)lk.dbg_rows[TBL];
    QSC_DCHECK(ia < lim && ib < lim);
    ia = ia < lim ? ia : 0u;
    ib = ib < lim ? ib : 0u;
  }
#endif
  if constexpr (DG != 0) {
    // diagnostic builds only (wrong values): every 16-lane group of a ds_read_b128 reads rows of
    // 16 distinct residues mod 16, i.e. conflict-free gathers (bounds the bank-conflict cost)
    ia = (ia & ~15u) | (threadIdx.x & 15u);
    ib = (ib & ~15u) | (threadIdx.x & 15u);
  }
#if QSC_DIAG_NOLDS  // diagnostic build: no gather (bounds the LDS share of the pass)
#pragma unroll
  for (int j = 0; j < RP / 2; ++j) {
    oa[j] = own[j] + splat2((float)ia);
    ob[j] = own[j] + splat2((float)ib);
  }
  tha = splat2((float)ia);
  thb = splat2((float)ib);
#else
  (void)own;
  if constexpr (sr_addr<E, KIND>()) {
    // ia, ib: the rows' LDS addresses (ent_rows4 / ent_rows2)
    (void)tab;
    (void)lk;
    lds_row2_at<RP>(ia, oa);
    lds_row2_at<RP>(ib, ob);
    tha = *(lds_f2v*)(uintptr_t)(ia + RP * 4);
    thb = *(lds_f2v*)(uintptr_t)(ib + RP * 4);
    return;
  }
  lds_row2<RP>(tab + ia * P, oa);
  lds_row2<RP>(tab + ib * P, ob);
  if constexpr (is_sr(KIND)) {
#if QSC_DIAG_SR_NOTH  // diagnostic build: no threshold read (wrong values; bounds its LDS cost)
    tha = thb = f2v{0.5f, 0.0f};
#else
    tha = *reinterpret_cast<const f2v*>(tab + ia * P + RP);
    thb = *reinterpret_cast<const f2v*>(tab + ib * P + RP);
#endif
    (void)lk;  // (the table's layout is static)
  } else {
    tha = thb = splat2(0.0f);
  }
#endif
}

// the arithmetic of an entry pair on its gathered rows oa, ob
template <int RP, typename E, int KIND, bool LOG>
__device__ __forceinline__ void pair_math(uint32_t ea, uint32_t eb, const f2v (&own)[RP / 2],
                                          const f2v (&oa)[RP / 2], const f2v (&ob)[RP / 2],
                                          f2v tha, f2v thb,
                                          const float2* __restrict__ edges, const Lik& lk,
                                          f2v (&acc)[RP / 2], f2v& nll, f2v& pq) {
  using T = Ent<E>;
  if constexpr (is_sr(KIND)) {
    // signed rows: z~ = thr~ + own . row~ (both carry the entry's sign), no code / pad handling
    const f2v t = f2v{dot2s<RP>(own, oa, tha), dot2s<RP>(own, ob, thb)};
    // P goes to the caller (pq), which takes log2 of two pairs' product: the NLL costs one
    // v_log per four entries (P >= 2^-25 or exactly 0, so four factors stay normal in fp32)
    f2v g;
#if QSC_DIAG_NOMATH
    g = t * splat2(1e-3f);
    pq = splat2(1.0f) + t * splat2(1e-30f);
#else
    if constexpr (KIND == LIK_LOGIT_ONEBIT_SR) {
      // logistic: pq = r = 1 / (1 + E) in [1/2, 1] goes to the caller's product (log2 P =
      // log2 r + min(z~, 0)); the linear tail part is summed here
      f2v lin;
      logit_onebit_rg(t, lk, pq, lin, g);
      nll -= lin;
    } else {
      onebit_sr_pg(t, lk, pq, g);
    }
#endif
    (void)edges;
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) acc[j] = fma2(splat2(g.x), oa[j], acc[j]);
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) acc[j] = fma2(splat2(g.y), ob[j], acc[j]);
    (void)ea;
    (void)eb;
    return;
  } else {
    const int ca = (int)(ea >> T::kBits), cb = (int)(eb >> T::kBits);
    const bool pa = ca == T::kPad, pb = cb == T::kPad;
    f2v t;
    if constexpr (is_onebit_cf(KIND))
      t = f2v{dot2z<RP>(own, oa, lk.ob_thr), dot2z<RP>(own, ob, lk.ob_thr)};
    else
      t = f2v{dot2<RP>(own, oa), dot2<RP>(own, ob)};
    f2v log2P, g;
#if QSC_DIAG_NOMATH  // diagnostic build: no likelihood arithmetic (bounds the VALU share)
    g = t * splat2(1e-3f);
    log2P = t;
#else
    if constexpr (is_onebit_cf(KIND))
      lik_grad2<KIND, LOG>(t, ca, cb, pa, pb, edges, lk, log2P, g);
    else
      lik_grad2<KIND, LOG>(t, pa ? 0 : ca, pb ? 0 : cb, pa, pb, edges, lk, log2P, g);
#endif
    float ga = g.x, gb = g.y;
    if constexpr (is_onebit_cf(KIND)) {
      nll -= log2P;  // log2 units: scaled by ln 2 later
    } else {
      ga = pa ? 0.0f : ga;
      gb = pb ? 0.0f : gb;
      nll -= f2v{pa ? 0.0f : log2P.x, pb ? 0.0f : log2P.y};
    }
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) acc[j] = fma2(splat2(ga), oa[j], acc[j]);
#pragma unroll
    for (int j = 0; j < RP / 2; ++j) acc[j] = fma2(splat2(gb), ob[j], acc[j]);
  }
}

// half a chunk (the S-pass lane's unit: the pixel's two lanes split every chunk) of a
// code-field kind: gather + arithmetic of its entry pair
template <int RP, typename E, int KIND, bool LOG>
__device__ __forceinline__ void half_chunk(const typename Ent<E>::V2& v, const f2v (&own)[RP / 2],
                                           const float* __restrict__ tab,
                                           const float2* __restrict__ edges, const Lik& lk,
                                           f2v (&acc)[RP / 2], f2v& nll) {
  uint32_t e[2];
  Ent<E>::unpack2(v, e);
  f2v oa[RP / 2], ob[RP / 2];
  f2v tha, thb, pq;
  pair_rows<RP, E, KIND, 0>(e[0], e[1], own, tab, oa, ob, tha, thb, lk);
  pair_math<RP, E, KIND, LOG>(e[0], e[1], own, oa, ob, tha, thb, edges, lk, acc, nll, pq);
}

// Read-ahead of a lane list in groups of NB chunks (chunk j at src[j * row], row in V4 units).
// Loads are unconditional with the index clamped to the lane's last chunk (the entry arrays end
// with a QSC_ENTRY_TAIL pad, so even an empty list's chunk 0 is addressable): the number of
// loads in flight is static, so the compiler waits for exactly the group it consumes
// (vmcnt(NB)) instead of draining every prefetch at a branch merge.
constexpr int kGroup = 4;
constexpr int kSchedQ = 16;  // S-pass slice queues (scheduler counters), QSC_PASS workspace

template <typename V4>
__device__ __forceinline__ void load_group(const V4* __restrict__ src, uint32_t lo, int row, int jb,
                                           int js, int jlast, V4 (&b)[kGroup]) {
#pragma unroll
  for (int i = 0; i < kGroup; ++i) {
    const int j = min(jb + i * js, jlast);
    b[i] = ld_lane(src + (int64_t)j * row, lo);
  }
}

// Consume group b (chunks jb, jb+js, ..., < j1), then walk the rest of the list with the next
// group's loads issued ahead of the current group's arithmetic.
// Software-pipelined gather: the LDS rows of the next entry pair are read before the current
// pair's arithmetic, so the LDS latency runs under it (the group's chunks are loaded, clamped,
// so a prefetch past the list end reads valid rows that are never used).  (The same in the
// S-pass walk spills at the 128-VGPR budget of the fused launch and was slower: DESIGN.md 7b.)
template <int RP, typename E, int KIND, bool LOG>
__device__ __forceinline__ void walk_groups(const typename Ent<E>::V4* __restrict__ src,
                                            uint32_t lo, int row, int jb, int j1, int js,
                                            typename Ent<E>::V4 (&b)[kGroup],
                                            const f2v (&own)[RP / 2],
                                            const float* __restrict__ tab,
                                            const float2* __restrict__ edges, const Lik& lk,
                                            f2v (&acc)[RP / 2], f2v& nll) {
  using V4 = typename Ent<E>::V4;
  const int jlast = max(j1 - 1, 0);
  const int jfirst = jb, jspan = max(j1 - jb, 1);
  auto fair = [&]() { prio_level(3 - min(3, (4 * (jb - jfirst)) / jspan)); };
  const uint32_t off = sr_addr<E, KIND>() ? lds_off(tab) : 0u;
  f2v ra[RP / 2], rb[RP / 2];
  f2v tra, trb;
  {
    uint32_t e[4];
    ent_rows4<RP, E, KIND>(b[0], off, e);
    pair_rows<RP, E, KIND, 1>(e[0], e[1], own, tab, ra, rb, tra, trb, lk);
  }
  for (;;) {
    fair();
    const int jn = jb + kGroup * js;
    const bool more = jn < j1;
    V4 nb[kGroup];
    load_group(src, lo, row, jn, js, jlast, nb);  // unconditional: static vmcnt accounting
#pragma unroll
    for (int i = 0; i < kGroup; ++i)
      if (jb + i * js < j1) {
        uint32_t e[4];
        ent_rows4<RP, E, KIND>(b[i], off, e);
        f2v xa[RP / 2], xb[RP / 2];
        f2v txa, txb, pqa, pqb;
        pair_rows<RP, E, KIND, 1>(e[2], e[3], own, tab, xa, xb, txa, txb, lk);
        pair_math<RP, E, KIND, LOG>(e[0], e[1], own, ra, rb, tra, trb, edges, lk, acc, nll, pqa);
        if (i + 1 < kGroup) {
          uint32_t f[4];
          ent_rows4<RP, E, KIND>(b[i + 1], off, f);
          pair_rows<RP, E, KIND, 1>(f[0], f[1], own, tab, ra, rb, tra, trb, lk);
        }
        pair_math<RP, E, KIND, LOG>(e[2], e[3], own, xa, xb, txa, txb, edges, lk, acc, nll, pqb);
        if constexpr (is_sr(KIND)) {
          const f2v pp = pqa * pqb;
          nll.x -= __builtin_amdgcn_logf(pp.x * pp.y);
        }
      }
    if (!more) break;
#pragma unroll
    for (int i = 0; i < kGroup; ++i) b[i] = nb[i];
    {
      uint32_t e[4];
      ent_rows4<RP, E, KIND>(b[0], off, e);
      pair_rows<RP, E, KIND, 1>(e[0], e[1], own, tab, ra, rb, tra, trb, lk);
    }
    jb = jn;
  }
}

// S-pass form: the pixel's two lanes split every 4-entry chunk (lane half h takes entries 2h,
// 2h+1 of each chunk row), so both walk the same, wave-uniform chunk range [0, j1) with one
// entry pair per chunk row -- no lane idles on an odd chunk count (C3: 12 % -> 6 % padded
// evaluations).  Group b holds chunk rows jb .. jb+kGroupS-1 (src[j * row]); the next group is
// read ahead unconditionally (clamped to the last row: static vmcnt accounting).
constexpr int kGroupS = 8;

template <int RP, typename E, int KIND, bool LOG>
__device__ __forceinline__ void walk_halves(const typename Ent<E>::V2* __restrict__ src,
                                            uint32_t lo, int row, int j1,
                                            typename Ent<E>::V2 (&b)[kGroupS],
                                            const f2v (&own)[RP / 2],
                                            const float* __restrict__ tab,
                                            const float2* __restrict__ edges, const Lik& lk,
                                            f2v (&acc)[RP / 2], f2v& nll) {
  using V2 = typename Ent<E>::V2;
  j1 = __builtin_amdgcn_readfirstlane(j1);
  const int jlast = max(j1 - 1, 0);
  int jb = 0;
  const uint32_t off = sr_addr<E, KIND>() ? lds_off(tab) : 0u;
  for (;;) {
    const int jn = jb + kGroupS;
    const bool more = jn < j1;
    V2 nb[kGroupS];
#pragma unroll
    for (int i = 0; i < kGroupS; ++i) nb[i] = ld_lane(src + (int64_t)min(jn + i, jlast) * row, lo);
    if constexpr (is_sr(KIND)) {
      // half chunks in pairs: one v_log of the four entries' product P
#pragma unroll
      for (int i = 0; i < kGroupS; i += 2)
        if (jb + i < j1) {
          f2v pa, pb = splat2(1.0f);
          {
            uint32_t e[2];
            ent_rows2<RP, E, KIND>(b[i], off, e);
            f2v oa[RP / 2], ob[RP / 2], tha, thb;
            pair_rows<RP, E, KIND, 0>(e[0], e[1], own, tab, oa, ob, tha, thb, lk);
            pair_math<RP, E, KIND, LOG>(e[0], e[1], own, oa, ob, tha, thb, edges, lk, acc, nll,
                                        pa);
          }
          if (jb + i + 1 < j1) {
            uint32_t e[2];
            ent_rows2<RP, E, KIND>(b[i + 1], off, e);
            f2v oa[RP / 2], ob[RP / 2], tha, thb;
            pair_rows<RP, E, KIND, 0>(e[0], e[1], own, tab, oa, ob, tha, thb, lk);
            pair_math<RP, E, KIND, LOG>(e[0], e[1], own, oa, ob, tha, thb, edges, lk, acc, nll,
                                        pb);
          }
          const f2v pp = pa * pb;
          nll.x -= __builtin_amdgcn_logf(pp.x * pp.y);
        }
    } else {
#pragma unroll
      for (int i = 0; i < kGroupS; ++i)
        if (jb + i < j1) half_chunk<RP, E, KIND, LOG>(b[i], own, tab, edges, lk, acc, nll);
    }
    if (!more) break;
#pragma unroll
    for (int i = 0; i < kGroupS; ++i) b[i] = nb[i];
    jb = jn;
  }
}

[[maybe_unused]] constexpr int kStampLast = 31;
#if QSC_DIAG_STAMPS && !defined(QSC_PASS_NO_STAMPS)
// diagnostic builds only: per-wave timestamps of a pass's phases (s_memtime, shader clock).
// File-local like the debug flag: each kernel file has its own table and exports its reader
// (qsc_diag_stamps_s / _c / _fused); qsc_pass_finish.hip, which stamps nothing, opts out
// (QSC_PASS_NO_STAMPS)
constexpr int kStampWaves = 4096, kStamps = 32;
__device__ unsigned long long g_stamps[kStampWaves * kStamps];
inline int diag_stamps_read(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps),
                                  sizeof(unsigned long long) * (size_t)std::min(n, kStampWaves * kStamps));
}
#define STAMP(w, i)                                                                 \
  do {                                                                               \
    if ((threadIdx.x & 63) == 0 && (w) < kStampWaves && (i) < kStamps)               \
      g_stamps[(w) * kStamps + (i)] = __builtin_amdgcn_s_memtime();                  \
  } while (0)
#define RSTAMP(w, i)                                                                 \
  do {                                                                               \
    if ((threadIdx.x & 63) == 0 && (w) < kStampWaves && (i) < kStamps)               \
      g_stamps[(w) * kStamps + (i)] = __builtin_amdgcn_s_memrealtime();              \
  } while (0)
#else
#define STAMP(w, i) \
  do {              \
  } while (0)
#define RSTAMP(w, i) \
  do {               \
  } while (0)
#endif

// Sum over the 64 lanes in a fixed order without LDS traffic: xor-1/xor-2 quad permutes and
// the row half-mirror / mirror DPP moves leave every lane of a 16-lane row holding the row sum;
// the four row sums are read into scalars and added in row order.  Result uniform.
__device__ __forceinline__ float dpp_f(float x, int ctrl) {
  switch (ctrl) {  // the DPP control must be an immediate
    case 0xB1: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, false));
    case 0x4E: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, false));
    case 0x141: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x141, 0xF, 0xF, false));
    default: return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x140, 0xF, 0xF, false));
  }
}
__device__ __forceinline__ float wave_sum_dpp(float x) {
  x += dpp_f(x, 0xB1);   // quad_perm [1,0,3,2]
  x += dpp_f(x, 0x4E);   // quad_perm [2,3,0,1]
  x += dpp_f(x, 0x141);  // row_half_mirror
  x += dpp_f(x, 0x140);  // row_mirror
  const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 0));
  const float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 16));
  const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 32));
  const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 48));
  return ((a + b) + c) + d;
}

// The S-step epilogue's lane-pair combine: a pixel's two lanes (l, l + 32) hold partial dS rows
// x = elements 0..RH-1 and y = RH..RP-1 of the same pixel; one v_permlane32_swap exchanges x's
// upper 32 lanes with y's lower ones, so lane l < 32 gets x[l] + x[l + 32] (its half's sums) and
// lane l >= 32 y[l - 32] + y[l]: half_sum + pick of both in 2 VALU, the same sums in the same
// order.  swap_lo: the value of x (lane < 32) or of y taken from the partner lane (lane >= 32):
// the half-row selection of a row both lanes hold.
__device__ __forceinline__ float half_sum_pick(float x, float y) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false,
                                                  false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap_lo(float x, float y) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false,
                                                  false);
  return __uint_as_float(r[0]);
}

// ||C||^2 in one fixed order (threads 0..255 stride 256, then the block sum): shared by the
// C-pass (256-thread blocks) and qsc_cupdate (1024), so both give the same bits
__device__ __forceinline__ float cnorm_sq(const float* __restrict__ C, int n, float* sh) {
  float s2 = 0.0f;
  if (threadIdx.x < 256)
    for (int i0 = threadIdx.x; i0 < n; i0 += 8 * 256) {  // 8 reads in flight, summed in order
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = C[min(i0 + 256 * j, n - 1)];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i0 + 256 * j < n) s2 = __builtin_fmaf(v[j], v[j], s2);
    }
  return block_sum(s2, sh);
}

// N consecutive floats (N = 2, 4, 8) of a position-order row: 8/16-byte vector accesses
template <int N>
__device__ __forceinline__ void ld_row(const float* __restrict__ src, float (&v)[N]) {
  if constexpr (N == 2) {
    const float2 x = *reinterpret_cast<const float2*>(src);
    v[0] = x.x;
    v[1] = x.y;
  } else {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const float4 x = *reinterpret_cast<const float4*>(src + i);
      v[i] = x.x;
      v[i + 1] = x.y;
      v[i + 2] = x.z;
      v[i + 3] = x.w;
    }
  }
}
template <int N>
__device__ __forceinline__ void st_row(float* __restrict__ dst, const float (&v)[N]) {
  if constexpr (N == 2) {
    *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int i = 0; i < N; i += 4)
      *reinterpret_cast<float4*>(dst + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  }
}

// The same at byte offset `lo` from a wave-uniform base (ld_lane / st_lane: saddr form)
template <int N>
__device__ __forceinline__ void ld_row(const float* __restrict__ base, uint32_t lo, float (&v)[N]) {
  if constexpr (N == 2) {
    const float2 x = ld_lane(reinterpret_cast<const float2*>(base), lo);
    v[0] = x.x;
    v[1] = x.y;
  } else {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const float4 x = ld_lane(reinterpret_cast<const float4*>(base), lo + 4 * i);
      v[i] = x.x;
      v[i + 1] = x.y;
      v[i + 2] = x.z;
      v[i + 3] = x.w;
    }
  }
}
template <int N>
__device__ __forceinline__ void st_row(float* __restrict__ base, uint32_t lo, const float (&v)[N]) {
  if constexpr (N == 2) {
    st_lane(reinterpret_cast<float2*>(base), lo, make_float2(v[0], v[1]));
  } else {
#pragma unroll
    for (int i = 0; i < N; i += 4)
      st_lane(reinterpret_cast<float4*>(base), lo + 4 * i,
              make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]));
  }
}

// The same store written through this XCD's L2 (agent-scope sc1 buffer stores): the line is not
// left dirty in L2, so the end-of-launch write-back has less to drain (the S-step's S, mS, vS
// rows are 25 MB per launch at C3; MI355X_MICROARCH.md prices a boundary at +B / 6 TB/s for B
// dirty bytes).  Byte offsets from `base` below 2^31.
template <int N>
__device__ __forceinline__ void st_row_wt(float* base, uint32_t lo, const float (&v)[N]) {
  typedef unsigned u4v __attribute__((ext_vector_type(4)));
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, 0x7fffffff,
                                                                     0x00020000);
  if constexpr (N == 2) {
    const u2v w = {__float_as_uint(v[0]), __float_as_uint(v[1])};
    __builtin_amdgcn_raw_buffer_store_b64(w, r, lo, 0, 16);  // aux 16: sc1
  } else {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
      const u4v w = {__float_as_uint(v[i]), __float_as_uint(v[i + 1]), __float_as_uint(v[i + 2]),
                     __float_as_uint(v[i + 3])};
      __builtin_amdgcn_raw_buffer_store_b128(w, r, lo + 16 * (i / 4), 0, 16);
    }
  }
}

// Per-slice registers read from HBM: the first group of entry chunks, S[:, q] and (fused Adam)
// the moments of the lane's rows.  Two sets live at once (current + prefetched next slice).
template <int RP, typename E, bool ADAM>
struct SliceIn {
  typename Ent<E>::V2 buf[kGroupS];
  float sv[RP];
  float mv[RP / 2], vv[RP / 2];
  int j1;
  const typename Ent<E>::V2* src;  // the slice's entries (wave-uniform; lanes add SliceLane::ent)

  __device__ __forceinline__ void assign(const SliceIn& o) {
#pragma unroll
    for (int i = 0; i < kGroupS; ++i) buf[i] = o.buf[i];
#pragma unroll
    for (int r = 0; r < RP; ++r) sv[r] = o.sv[r];
    if constexpr (ADAM) {
#pragma unroll
      for (int i = 0; i < RP / 2; ++i) {
        mv[i] = o.mv[i];
        vv[i] = o.vv[i];
      }
    }
    j1 = o.j1;
    src = o.src;
  }
};

// Issue every global read of slice s for this lane (unconditional loads: static vmcnt).
// Entries: the lane's half (entries 2h, 2h+1) of its position's chunk in each chunk row of
// QSC_SLICE positions (2 * QSC_SLICE halves per row), the first kGroupS rows.
// Position-order rows are [Pp][RP]: the lane reads its pixel's whole S row and the half
// [h*RP/2, (h+1)*RP/2) of the Adam moments it will update.
// Per-lane byte offsets of the S-pass accesses (constant for a lane): its entry half within a
// chunk row, its pixel's S row and its half of that row within a slice's block of rows.
struct SliceLane {
  uint32_t ent, row, half;
};
template <int RP, typename E>
__device__ __forceinline__ SliceLane slice_lane(int p, int h) {
  SliceLane l;
  l.ent = (uint32_t)(2 * p + h) * (uint32_t)sizeof(typename Ent<E>::V2);
  l.row = (uint32_t)(p * RP) * 4u;
  l.half = l.row + (uint32_t)(h * (RP / 2)) * 4u;
  return l;
}

template <int RP, typename E, bool ADAM>
__device__ __forceinline__ void slice_load(SliceIn<RP, E, ADAM>& in, const E* __restrict__ ent,
                                           const int* __restrict__ width,
                                           const int64_t* __restrict__ off, int s,
                                           const SliceLane& ln, const float* __restrict__ S,
                                           const float* __restrict__ mS,
                                           const float* __restrict__ vS) {
  using V2 = typename Ent<E>::V2;
  // both slice words read before either is used: one scalar-cache round trip, not two in a
  // chain (the entry reads below depend on both; at the start of a launch this chain is the
  // critical path to the first slice's data)
  const int64_t o = off[s];
  const int wd = width[s];
  in.j1 = wd >> 2;
  in.src = reinterpret_cast<const V2*>(ent + o);
  const int jlast = max(in.j1 - 1, 0);
#pragma unroll
  for (int i = 0; i < kGroupS; ++i)
    in.buf[i] = ld_lane(in.src + (int64_t)min(i, jlast) * (2 * QSC_SLICE), ln.ent);
  const int64_t blk = (int64_t)s * QSC_SLICE * RP;  // the slice's rows (uniform)
  ld_row<RP>(S + blk, ln.row, in.sv);
  if constexpr (ADAM) {
    ld_row<RP / 2>(mS + blk, ln.half, in.mv);
    ld_row<RP / 2>(vS + blk, ln.half, in.vv);
  }
}

}  // namespace
