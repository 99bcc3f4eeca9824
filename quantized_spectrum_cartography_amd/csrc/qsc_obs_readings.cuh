// qsc_obs_readings.cuh — the caller-kept sorted readings (`packed`) of the list packing: their
// shapes, their carving and the search of a segment table.  Shared by qsc_obs_readings.hip (which
// writes them and fills the entry formats from them), qsc_draw.hip (which redraws their codes) and
// qsc_obs_select.hip (which exports the kept ones as lists).
//
// A sorted reading is  idx | code << 24  (idx = k or qlocal < 2^24, the wide format's own bound).
#pragma once
#include "qsc_common.cuh"

namespace {
using namespace qsc;

constexpr int kIdxBits = 24;
constexpr uint32_t kIdxMask = (1u << kIdxBits) - 1;

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

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

}  // namespace
