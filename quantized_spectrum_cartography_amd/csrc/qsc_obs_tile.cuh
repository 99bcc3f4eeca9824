// qsc_obs_tile.cuh — the dense 4096-cell tile of the kernels that work on codes[K][P] cell by cell
// (qsc_draw.hip: draw_codes_kernel; qsc_obs_select.hip: select_codes_kernel, export_codes_kernel).
// About one cell in ten is observed, so a workgroup of kTileBlock threads loads kTile consecutive
// cells into LDS (one 16-byte load per thread where tile_vec_ok, byte loads otherwise), lists the
// offsets of the observed ones in ascending order (stage_observed) so that the costly per-cell work
// runs on full waves, and writes the tile back in the layout it was read in.
// The list is made by a ballot / popcount scan (block_scan, scan_pos; the readings export uses them
// too): element i * kTileBlock + tid of a chunk is bit i of thread tid's mask; the popcounts of the
// ROUNDS x 4 (round, wave) ballots are scanned by one wave64 with shuffles, and an element's place
// is its (round, wave) prefix plus the popcount of its ballot below its lane.  No atomics decide it.
#pragma once
#include "qsc_common.cuh"

namespace {

constexpr int kTileBlock = 256;              // threads of a workgroup of these kernels
constexpr int kTileWaves = kTileBlock / 64;
constexpr int kCells = 16;                   // cells per thread
constexpr int kTile = kTileBlock * kCells;   // cells per workgroup
static_assert(kTile == QSC_EXPORT_CHUNK_CODES, "qsc.h");
static_assert(kCells * kTileWaves <= 64, "one wave64 scans the (round, wave) counts");

// every thread's 16 cells are one aligned 16-byte word of the array(s) the kernel reads / writes
inline bool tile_vec_ok(int P, const void* a, const void* b = nullptr) {
  return (P % kCells) == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0;
}

// the nc <= kTile cells from codes + base on into `tile` (no barrier)
template <bool VEC>
__device__ __forceinline__ void tile_load(const uint8_t* __restrict__ codes, int64_t base, int nc,
                                          uint8_t* tile) {
  if (VEC) {
    const int o = threadIdx.x * kCells;
    // (the cell count is a multiple of 16: a thread's 16 cells are all inside or all outside)
    if (o < nc) *reinterpret_cast<uint4*>(tile + o) = *reinterpret_cast<const uint4*>(codes + base + o);
  } else {
#pragma unroll
    for (int i = 0; i < kCells; ++i) {
      const int o = i * kTileBlock + threadIdx.x;
      if (o < nc) tile[o] = codes[base + o];
    }
  }
}
// ... and back, to out + base on (after the caller's barrier)
template <bool VEC>
__device__ __forceinline__ void tile_store(uint8_t* __restrict__ out, int64_t base, int nc,
                                           const uint8_t* tile) {
  if (VEC) {
    const int o = threadIdx.x * kCells;
    if (o < nc) *reinterpret_cast<uint4*>(out + base + o) = *reinterpret_cast<const uint4*>(tile + o);
  } else {
#pragma unroll
    for (int i = 0; i < kCells; ++i) {
      const int o = i * kTileBlock + threadIdx.x;
      if (o < nc) out[base + o] = tile[o];
    }
  }
}

// Exclusive scan of the selected elements of a chunk: bit i of `mask` selects element
// i * kTileBlock + tid.  Leaves the (round, wave) prefixes in wcnt[0 .. 63] and the total in
// wcnt[64] (which is returned).  Every thread of the workgroup calls it.
template <int ROUNDS>
__device__ __forceinline__ int block_scan(uint32_t mask, int* wcnt) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < ROUNDS; ++i) {
    const unsigned long long b = __ballot((mask >> i) & 1u);
    if (lane == 0) wcnt[i * kTileWaves + wave] = __popcll(b);
  }
  __syncthreads();
  if (wave == 0) {
    const int v = lane < ROUNDS * kTileWaves ? wcnt[lane] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(inc, d);
      if (lane >= d) inc += u;
    }
    wcnt[lane] = inc - v;
    if (lane == 63) wcnt[64] = inc;
  }
  __syncthreads();
  return wcnt[64];
}
// the place of element (round i, this thread) among the selected ones; all threads call it
__device__ __forceinline__ int scan_pos(uint32_t mask, int i, const int* wcnt) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned long long b = __ballot((mask >> i) & 1u);
  return wcnt[i * kTileWaves + wave] + __popcll(b & ((1ull << lane) - 1ull));
}

// The chunk [c0, c0 + nc) of the flat codes into `tile`, the offsets of its observed cells into
// `list`, ascending.  -> their number.  Ends with a barrier.
template <bool VEC>
__device__ __forceinline__ int stage_observed(const uint8_t* __restrict__ codes, int64_t c0, int nc,
                                              uint8_t* tile, uint16_t* list, int* wcnt) {
  tile_load<VEC>(codes, c0, nc, tile);
  __syncthreads();
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < kCells; ++i) {
    const int o = i * kTileBlock + threadIdx.x;
    if (o < nc && tile[o] != 0xFFu) mask |= 1u << i;
  }
  const int nl = block_scan<kCells>(mask, wcnt);
#pragma unroll
  for (int i = 0; i < kCells; ++i) {
    const int pos = scan_pos(mask, i, wcnt);
    if ((mask >> i) & 1u) list[pos] = (uint16_t)(i * kTileBlock + threadIdx.x);
  }
  __syncthreads();
  return nl;
}

}  // namespace
