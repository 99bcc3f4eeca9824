// qsc_obs_fmt.cuh — the packed entry formats of include/qsc.h (qsc_obs_desc) as code: entry and
// pad values, the chunked slot of an entry, and the read-ahead tail.  Shared by the two packers,
// qsc_obs.hip (from dense codes) and qsc_obs_readings.hip (from a list of readings), so that both
// write one format.
#pragma once

#include "qsc_common.cuh"

namespace {

template <typename E>
struct EntryTraits;
template <>
struct EntryTraits<uint16_t> {
  static constexpr int kBits = 12;
  static constexpr uint32_t kPad = 15;
};
template <>
struct EntryTraits<uint32_t> {
  static constexpr int kBits = 24;
  static constexpr uint32_t kPad = 255;
};

// chunked column-major slot of entry j of lane `lane` in a list group of `lanes` lanes
__device__ __forceinline__ int64_t slot(int64_t base, int lanes, int lane, int j) {
  return base + (int64_t)(j >> 2) * (lanes * 4) + lane * 4 + (j & 3);
}

// Entry values (include/qsc.h): code-field form  idx | code << KBITS  (pad: code PAD), or the
// signed-row form (rowfmt 1)  idx + (code == 1 ? sr_off(rows) : 0)  (pad: row 2 sr_off(rows)),
// where `rows` is the table's row count, K for the S-format and PT for the C-format
template <typename E>
__device__ __forceinline__ E entry_of(uint32_t idx, uint32_t code, int sr, int rows) {
  using Tr = EntryTraits<E>;
  return sr ? (E)(idx + (code == 1 ? (uint32_t)qsc::sr_off(rows) : 0u))
            : (E)(idx | (code << Tr::kBits));
}
template <typename E>
__host__ __device__ __forceinline__ E pad_of(int sr, int rows) {
  using Tr = EntryTraits<E>;
  return sr ? (E)(2u * (uint32_t)qsc::sr_off(rows)) : (E)(Tr::kPad << Tr::kBits);
}

// pad entries after the last list (read-ahead tail, QSC_ENTRY_TAIL)
template <typename E>
__global__ void tail_fill_kernel(E* __restrict__ ent, int64_t start, int n, int sr, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ent[start + i] = pad_of<E>(sr, rows);
}

}  // namespace
