// qsc_obs_readings.cuh — the caller-kept sorted readings (`packed`) of the list packing: their
// shapes, their carving and the search of a segment table.  Shared by qsc_obs_readings.hip (which
// writes them and fills the entry formats from them), qsc_draw.hip (which redraws their codes),
// qsc_obs_select.hip (which exports the kept ones as lists) and qsc_obs_append.hip (which merges a
// sorted batch into them, between the layout's own stages: declared at the end of this file).
// Written here once for all of them: the occurrence number of a sorted reading (occurrence), the
// walks of the two arrays (walk_s_slice, walk_c_tile), the check of a caller's `packed` (packed_of).
//
// A sorted reading is  idx | code << 24  (idx = k or qlocal < 2^24, the wide format's own bound).
#pragma once
#include "qsc_common.cuh"

namespace {
using namespace qsc;

constexpr int kIdxBits = 24;
constexpr uint32_t kIdxMask = (1u << kIdxBits) - 1;

// the list l of `nl` contiguous segments that holds sorted reading e: seg[l] <= e < seg[l + 1]
// (seg[0] <= e < seg[nl] on entry; empty segments are stepped over)
__device__ __forceinline__ int seg_find(const int* seg, int nl, int e) {
  int lo = 0, hi = nl;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// The occurrence number j of sorted reading e (index idx, its list starting at seg_lo): the
// readings of the same cell in front of it, counted by looking back along the run of equal indices
// (at most max_repeat long).  Both arrays are stable sorts of one list, so reading j of a cell is
// the same reading in both; the Philox counter of every draw and of every keep decision hangs on
// this j.  A run may begin before the caller's chunk: the reads are global.
__device__ __forceinline__ uint32_t occurrence(const uint32_t* __restrict__ rd, int64_t e,
                                               int seg_lo, uint32_t idx) {
  uint32_t j = 0;
  for (int64_t b = e - 1; b >= seg_lo && (rd[b] & kIdxMask) == idx; --b) ++j;
  return j;
}

// The walk of slice s of the S-format sorted array by one wave: the slice's 32 lists are one
// contiguous run of rd, read coalesced; `seg` (this wave's QSC_SLICE + 1 ints of LDS) gets their
// bounds.  body(e, l, rd[e], seg[l]) for every reading e of the slice, l its list.  Every wave of
// the workgroup calls it (one barrier); -> false for a wave past the last slice, which ends there.
template <typename Body>
__device__ __forceinline__ bool walk_s_slice(const uint32_t* __restrict__ rd,
                                             const int* __restrict__ seg_all, int64_t n, int ns,
                                             int s, int* seg, Body&& body) {
  const int lane = threadIdx.x & 63;
  const bool live = s < ns;
  if (live && lane <= QSC_SLICE) seg[lane] = seg_all[(int64_t)s * QSC_SLICE + lane];
  __syncthreads();
  if (!live) return false;
  const int lo = seg[0], hi = seg[QSC_SLICE];
  for (int64_t e = (int64_t)lo + lane; e < hi && e < n; e += 64) {
    const int l = seg_find(seg, QSC_SLICE, (int)e);
    body(e, l, rd[e], seg[l]);
  }
  return true;
}

// The walk of tile t of the C-format sorted array by one workgroup: the tile's Kp bin lists (bins
// in k order) are one contiguous run of rd; `seg` (Kp + 1 ints of LDS) receives their bounds.
// body(e, k, rd[e], seg[k]) for every reading e of the tile, k its bin.  One barrier.
template <typename Body>
__device__ __forceinline__ void walk_c_tile(const uint32_t* __restrict__ rd,
                                            const int* __restrict__ seg_all, int64_t n, int t,
                                            int Kp, int* seg, Body&& body) {
  for (int i = threadIdx.x; i <= Kp; i += blockDim.x) seg[i] = seg_all[(int64_t)t * Kp + i];
  __syncthreads();
  const int lo = seg[0], hi = seg[Kp];
  for (int64_t e = (int64_t)lo + threadIdx.x; e < hi && e < n; e += blockDim.x) {
    const int k = seg_find(seg, Kp, (int)e);
    body(e, k, rd[e], seg[k]);
  }
}

// shapes both calls derive from (K, P, PT)
struct Dims {
  int64_t Pp, ns, nt, nks, Kp, nc, nb;  // nb = nt * Kp bins, nc = nt * nks blocks
};
inline bool dims_of(int32_t K, int32_t P, int32_t PT, Dims* d) {
  if (K < 1 || P < 1 || PT < 64 || (PT & 63)) return false;
  d->Pp = round_up(P, PT);
  d->ns = d->Pp / QSC_SLICE;
  d->nt = d->Pp / PT;
  d->nks = ceil_div(K, 64);
  d->Kp = d->nks * 64;
  d->nc = d->nt * d->nks;
  d->nb = d->nt * d->Kp;
  // every table is indexed and scanned with int
  return d->Pp < (int64_t)1 << 31 && d->nb < ((int64_t)1 << 31) - 1;
}

// the caller-kept sorted readings
struct Packed {
  uint32_t* s_rd;  // [n]  k | code << 24, by (position, k)
  uint32_t* c_rd;  // [n]  qlocal | code << 24, by (tile, bin, qlocal)
  int* s_seg;      // [Pp + 1]  first sorted reading of every position's list
  int* c_seg;      // [nt * Kp + 1]  ... of every (tile, bin) list, bins in k order
  int* c_kinv;     // [nt * Kp]  place of bin k in the tile's c_kmap
};
inline size_t packed_carve(char* b, int64_t n, const Dims& d, Packed* pk) {
  char* w = b;
  pk->s_rd = (uint32_t*)w;
  w += align_up((size_t)n * 4);
  pk->c_rd = (uint32_t*)w;
  w += align_up((size_t)n * 4);
  pk->s_seg = (int*)w;
  w += align_up((size_t)(d.Pp + 1) * 4);
  pk->c_seg = (int*)w;
  w += align_up((size_t)(d.nb + 1) * 4);
  pk->c_kinv = (int*)w;
  w += align_up((size_t)d.nb * 4);
  return (size_t)(w - b);
}

inline bool n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }

// a caller's descriptor against the shapes its (K, P, PT) give -> *dm
inline bool desc_dims(const qsc_obs_desc* d, Dims* dm) {
  return d && dims_of(d->K, d->P, d->PT, dm) && dm->Pp == d->Pp && dm->nt == d->ntiles &&
         dm->nks == d->nks;
}
// ... and a caller's `packed` of n readings against it -> *pk.  counted: n is d->nnz, i.e. every
// reading has a position (the fill alone also takes a layout where some have none)
inline bool packed_of(const void* packed, size_t packed_bytes, int64_t n, const qsc_obs_desc* d,
                      Dims* dm, Packed* pk, bool counted = true) {
  return packed && n_ok(n) && desc_dims(d, dm) && (!counted || d->nnz == n) &&
         packed_bytes >= packed_carve((char*)packed, n, *dm, pk);
}

}  // namespace

// The stages of the list layout (qsc_obs_readings.hip defines them), in the order
// qsc_obs_readings_layout runs them; qsc_obs_append.hip runs the same ones around its merges, so
// that widths, offsets, bin order and the descriptor of an appended packing come from the very
// code that lays out a re-sorted one.  Host functions; every stage is stream-ordered except
// rd_layout_finish, which reads the totals back.
namespace qsc {

// the layout's workspace for a list of n readings
struct RdWs {
  int* iperm;        // [P]
  int* poscnt;       // [Pp + 1]
  int* ccount;       // [nt * Kp + 1]
  int64_t* s_sizes;  // [ns + 1]
  int64_t* c_sizes;  // [nc + 1]
  int64_t* totals;   // [4]: s_off, c_off totals; then two ints, nnz and max_repeat
  uint64_t* s_key;   // [n] x 3: S keys, C keys, sorted keys
  uint64_t* c_key;
  uint64_t* key_out;
  uint32_t* s_val;   // [n] x 2
  uint32_t* c_val;
  void* cub;
  size_t cub_bytes;
};
// carves b (may be null: sizing only) -> bytes, 0 for shapes out of range
size_t rd_ws_carve(char* b, int64_t n, int32_t K, int32_t P, int32_t PT, RdWs* ws);
// the kernels' LDS tables fit the device and K, PT fit a sorted reading's 24-bit index
bool rd_layout_fits(int32_t K, int32_t P, int32_t PT);
// inverse pixel order and per-position counts from cnt[P] -> w.iperm, w.poscnt; S-format slice
// widths, offsets and list segments -> s_width, s_off, s_seg[Pp + 1]
int rd_layout_positions(const RdWs& w, int32_t K, int32_t P, int32_t PT, const int32_t* perm,
                        const int32_t* cnt, int32_t* s_width, int64_t* s_off, int* s_seg,
                        hipStream_t s);
// sort keys and values of both orders -> w.s_key, w.s_val, w.c_key, w.c_val; w.ccount[bin] += 1
// per placed reading (the caller initialises w.ccount)
int rd_layout_keys(const RdWs& w, const int32_t* k, const int32_t* p, const void* code,
                   int32_t code_bytes, int64_t n, int32_t K, int32_t P, int32_t PT, int32_t nbins,
                   hipStream_t s);
// the stable radix sort of n (key, value) pairs with keys <= max_key
int rd_sort_pairs(const RdWs& w, const uint64_t* key_in, uint64_t* key_out, const uint32_t* val_in,
                  uint32_t* val_out, int64_t n, uint64_t max_key, hipStream_t s);
// after the sorts: bin order, C-format widths, offsets and list segments from w.ccount -> c_width,
// c_off, c_kmap, c_seg, c_kinv; the totals (SYNCHRONOUS) -> *desc, *max_repeat (the int the
// caller's kernels left at ((int*)(w.totals + 2))[1])
int rd_layout_finish(const RdWs& w, int32_t K, int32_t P, int32_t PT, int32_t nbins,
                     const int* s_seg, const int64_t* s_off, int32_t* c_width, int64_t* c_off,
                     int32_t* c_kmap, int* c_seg, int* c_kinv, qsc_obs_desc* desc,
                     int32_t* max_repeat, hipStream_t s);

}  // namespace qsc
