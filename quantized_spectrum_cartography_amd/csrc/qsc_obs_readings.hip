// qsc_obs_readings.hip — packing of the two sliced sparse formats (include/qsc.h, qsc_obs_desc)
// from a LIST of readings (k, p, code), in any order, a cell read any number of times.
//
// Why: qsc_obs.hip finds the observed cells by scanning a dense codes[K][P], which holds one
// reading per cell at most and costs K P reads whatever the density.  Here the work follows the
// list: two stable radix sorts put the readings into the order of each format -- (position, k)
// for the S-format, (tile, bin, qlocal) for the C-format -- so that every packed list is one
// contiguous segment of a sorted array, found from scans of the integer count tables.  The fill
// kernels read those segments coalesced and scatter the 2- or 4-byte entries into the chunked
// layout.  Integer atomics are used for counts only; the packed bytes depend on the input order
// alone (equal keys keep it: the sort is stable), never on grid or wave order.
//
// The sorted readings are kept by the caller (`packed`, qsc_obs_readings_packed_bytes; their layout
// is qsc_obs_readings.cuh's): a sorted reading is  idx | code << 24  (idx = k or qlocal < 2^24, the
// wide format's own bound), from which qsc_obs_readings_fill writes either entry format again
// without a dense codes array.
#include <hipcub/hipcub.hpp>

#include "qsc_common.cuh"
#include "qsc_obs_fmt.cuh"
#include "qsc_obs_readings.cuh"

using namespace qsc;

namespace {

constexpr int kBlock = 256;
__device__ __forceinline__ int code_at(const void* code, int code_bytes, int64_t i) {
  return code_bytes == 1 ? (int)((const uint8_t*)code)[i] : ((const int32_t*)code)[i];
}

__device__ __forceinline__ bool reading_ok(int k, int p, int c, int K, int P, int nbins) {
  return k >= 0 && k < K && p >= 0 && p < P && c >= 0 && c < nbins;
}

// cnt[p] += 1 per valid reading of pixel p; *bad += 1 per reading outside the ranges
__global__ void __launch_bounds__(kBlock) rd_count_kernel(const int* __restrict__ k,
                                                          const int* __restrict__ p,
                                                          const void* __restrict__ code,
                                                          int code_bytes, int64_t n, int K, int P,
                                                          int nbins, int* __restrict__ cnt,
                                                          int* __restrict__ bad) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int kk = k[i], pp = p[i];
  if (reading_ok(kk, pp, code_at(code, code_bytes, i), K, P, nbins))
    atomicAdd(&cnt[pp], 1);
  else
    atomicAdd(bad, 1);
}

// iperm[perm[q]] = q; poscnt[q] = readings of position q (0 for padding positions)
__global__ void __launch_bounds__(kBlock) rd_positions_kernel(const int* __restrict__ perm,
                                                              const int* __restrict__ cnt, int P,
                                                              int Pp, int* __restrict__ iperm,
                                                              int* __restrict__ poscnt) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > Pp) return;
  int c = 0;
  if (q < Pp) {
    const int p = perm[q];
    if (p >= 0 && p < P) {
      iperm[p] = q;
      c = cnt[p];
    }
  }
  poscnt[q] = c;  // poscnt[Pp] = 0: the scan's total slot
}

// S-format slice widths: QSC_SLICE * round4(longest list of the slice)
__global__ void __launch_bounds__(kBlock) rd_s_width_kernel(const int* __restrict__ poscnt,
                                                            int nslices, int* __restrict__ width,
                                                            int64_t* __restrict__ sizes) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nslices) return;
  if (s == nslices) {
    sizes[s] = 0;
    return;
  }
  int m = 0;
  for (int l = 0; l < QSC_SLICE; ++l) m = max(m, poscnt[s * QSC_SLICE + l]);
  m = (m + 3) & ~3;
  width[s] = m;
  sizes[s] = (int64_t)m * QSC_SLICE;
}

// tile and row of a position: the inverse of tile_pos (qsc_common.cuh)
__device__ __forceinline__ void tile_of(int pos, int nt, int* t, int* ql) {
  const int g = pos / QSC_SLICE, l = pos % QSC_SLICE;
  const int i = g / nt, r = g - i * nt;
  *t = (i & 1) ? (nt - 1 - r) : r;
  *ql = i * QSC_SLICE + l;
}

// Sort keys and sorted values of both formats.  A reading that is out of range, or whose pixel
// has no position, gets the key past every valid one: it sorts behind the segments (which are
// sized from the counts of valid readings) and is never packed.
__global__ void __launch_bounds__(kBlock) rd_keys_kernel(
    const int* __restrict__ k, const int* __restrict__ p, const void* __restrict__ code,
    int code_bytes, int64_t n, int K, int P, int Pp, int PT, int nt, int Kp, int nbins,
    const int* __restrict__ iperm, uint64_t* __restrict__ s_key, uint32_t* __restrict__ s_val,
    uint64_t* __restrict__ c_key, uint32_t* __restrict__ c_val, int* __restrict__ ccount) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int kk = k[i], pp = p[i], c = code_at(code, code_bytes, i);
  int pos = -1;
  if (reading_ok(kk, pp, c, K, P, nbins)) pos = iperm[pp];
  if (pos < 0 || pos >= Pp) {
    s_key[i] = (uint64_t)Pp * (uint64_t)K;
    c_key[i] = (uint64_t)nt * (uint64_t)Kp * (uint64_t)PT;
    s_val[i] = 0;
    c_val[i] = 0;
    return;
  }
  int t, ql;
  tile_of(pos, nt, &t, &ql);
  s_key[i] = (uint64_t)pos * (uint64_t)K + (uint64_t)kk;
  s_val[i] = (uint32_t)kk | ((uint32_t)c << kIdxBits);
  const int64_t bin = (int64_t)t * Kp + kk;
  c_key[i] = (uint64_t)bin * (uint64_t)PT + (uint64_t)ql;
  c_val[i] = (uint32_t)ql | ((uint32_t)c << kIdxBits);
  atomicAdd(&ccount[bin], 1);
}

// largest number of readings of one cell: the longest run of equal keys among the first `valid`
// sorted S-format keys (every run is walked once, from its first element)
__global__ void __launch_bounds__(kBlock) rd_max_repeat_kernel(const uint64_t* __restrict__ key,
                                                               const int* __restrict__ valid,
                                                               int64_t n, int* __restrict__ out) {
  const int64_t nv = min((int64_t)*valid, n);
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nv) return;
  const uint64_t v = key[i];
  if (i > 0 && key[i - 1] == v) return;
  int64_t e = i + 1;
  while (e < nv && key[e] == v) ++e;
  atomicMax(out, (int)(e - i));
}

// C-format layout of one pixel tile (one block per tile) from the tile's per-bin reading counts:
// the bins ordered by count, descending, ties to the lower k (padding bins K..Kp-1 count -1, so
// they come last) -> c_kmap and its inverse, and the slice widths (the slice's first, i.e.
// longest, list rounded up to chunks of 4): the rules of qsc_obs.hip's c_layout_kernel
__global__ void __launch_bounds__(kBlock) rd_c_order_kernel(const int* __restrict__ ccount, int K,
                                                            int nks, int* __restrict__ width,
                                                            int64_t* __restrict__ sizes,
                                                            int* __restrict__ kmap,
                                                            int* __restrict__ kinv) {
  extern __shared__ int lcnt[];  // [Kp] counts, then [Kp] bin order
  const int Kp = nks * 64;
  int* lord = lcnt + Kp;
  const int t = blockIdx.x;
  for (int i = threadIdx.x; i < Kp; i += blockDim.x)
    lcnt[i] = i < K ? ccount[(int64_t)t * Kp + i] : -1;
  __syncthreads();
  for (int k = threadIdx.x; k < Kp; k += blockDim.x) {
    const int c = lcnt[k];
    int rank = 0;
    for (int k2 = 0; k2 < Kp; ++k2) {
      const int c2 = lcnt[k2];
      rank += (c2 > c) || (c2 == c && k2 < k);
    }
    lord[rank] = k;
    kmap[(int64_t)t * Kp + rank] = k;
    kinv[(int64_t)t * Kp + k] = rank;
  }
  __syncthreads();
  for (int ks = threadIdx.x; ks < nks; ks += blockDim.x) {
    int m = max(lcnt[lord[ks * 64]], 0);
    m = (m + 3) & ~3;
    width[(int64_t)t * nks + ks] = m;
    sizes[(int64_t)t * nks + ks] = (int64_t)m * 64;
  }
  if (t == 0 && threadIdx.x == 0) sizes[(int64_t)gridDim.x * nks] = 0;  // the scan's total slot
}

// S-format fill, one wave per slice (walk_s_slice, qsc_obs_readings.cuh): each reading is stored
// at its chunked slot.  Then the slice's slots are swept in address order for the pads.
template <typename E>
__global__ void __launch_bounds__(kBlock) rd_s_fill_kernel(const uint32_t* __restrict__ rd,
                                                           const int* __restrict__ seg_all,
                                                           int64_t n, int ns, int K,
                                                           const int* __restrict__ width,
                                                           const int64_t* __restrict__ off,
                                                           E* __restrict__ ent, int sr) {
  __shared__ int seg_sh[kBlock / 64][QSC_SLICE + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s = blockIdx.x * (kBlock / 64) + wave;
  int* seg = seg_sh[wave];
  const int W = s < ns ? width[s] : 0;
  const int64_t base = s < ns ? off[s] : 0;
  auto store = [&](int64_t e, int l, uint32_t v, int e0) {
    const int j = (int)e - e0;
    // (j >= W cannot happen for consistent tables; the test keeps the store in the slice)
    if (j < W) ent[slot(base, QSC_SLICE, l, j)] = entry_of<E>(v & kIdxMask, v >> kIdxBits, sr, K);
  };
  if (!walk_s_slice(rd, seg_all, n, ns, s, seg, store)) return;
  const E pad = pad_of<E>(sr, K);
  for (int64_t o = lane; o < (int64_t)W * QSC_SLICE; o += 64) {  // W * 32 may pass 2^31
    const int l = (int)(o >> 2) & (QSC_SLICE - 1), j = (int)(o / (QSC_SLICE * 4)) * 4 + (int)(o & 3);
    if (j >= seg[l + 1] - seg[l]) ent[base + o] = pad;
  }
}

// C-format fill, one block per tile (walk_c_tile, qsc_obs_readings.cuh): each reading finds its
// bin's place in the count-sorted order in kinv and is stored at its chunked slot.  Then every
// (tile, k-slice) block is swept in address order for the pads.
template <typename E>
__global__ void __launch_bounds__(kBlock) rd_c_fill_kernel(
    const uint32_t* __restrict__ rd, const int* __restrict__ seg_all, int64_t n, int K, int PT,
    int nks, const int* __restrict__ width, const int64_t* __restrict__ off,
    const int* __restrict__ kmap, const int* __restrict__ kinv, E* __restrict__ ent, int sr) {
  extern __shared__ int seg[];  // [Kp + 1]
  const int Kp = nks * 64;
  const int t = blockIdx.x;
  walk_c_tile(rd, seg_all, n, t, Kp, seg, [&](int64_t e, int k, uint32_t v, int e0) {
    const int j = (int)e - e0;
    const int rank = kinv[(int64_t)t * Kp + k];
    if (rank < 0 || rank >= Kp) return;
    const int64_t wi = (int64_t)t * nks + (rank >> 6);
    if (j >= width[wi]) return;  // (cannot happen for consistent tables)
    ent[slot(off[wi], 64, rank & 63, j)] = entry_of<E>(v & kIdxMask, v >> kIdxBits, sr, PT);
  });
  const E pad = pad_of<E>(sr, PT);
  for (int ks = 0; ks < nks; ++ks) {
    const int64_t wi = (int64_t)t * nks + ks;
    const int W = width[wi];
    const int64_t base = off[wi];
    for (int64_t o = threadIdx.x; o < (int64_t)W * 64; o += blockDim.x) {  // W * 64 may pass 2^31
      const int l = (int)(o >> 2) & 63, j = (int)(o >> 8) * 4 + (int)(o & 3);
      const int k = kmap[wi * 64 + l];
      const int c = (k >= 0 && k < K) ? seg[k + 1] - seg[k] : 0;
      if (j >= c) ent[base + o] = pad;
    }
  }
}

int key_bits(uint64_t max_key) {
  int b = 1;
  while (b < 64 && (max_key >> b)) ++b;
  return b;
}

size_t cub_sort_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                           (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
  return b;
}
size_t cub_scan32_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int*)nullptr, (int*)nullptr, (int)n);
  return b;
}
size_t cub_scan64_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t*)nullptr, (int64_t*)nullptr, (int)n);
  return b;
}

size_t ws_carve(char* b, int64_t n, int32_t P, const Dims& d, RdWs* ws) {
  char* w = b;
  ws->iperm = (int*)w;
  w += align_up((size_t)P * 4);
  ws->poscnt = (int*)w;
  w += align_up((size_t)(d.Pp + 1) * 4);
  ws->ccount = (int*)w;
  w += align_up((size_t)(d.nb + 1) * 4);
  ws->s_sizes = (int64_t*)w;
  w += align_up((size_t)(d.ns + 1) * 8);
  ws->c_sizes = (int64_t*)w;
  w += align_up((size_t)(d.nc + 1) * 8);
  ws->totals = (int64_t*)w;
  w += align_up(4 * 8);
  ws->s_key = (uint64_t*)w;
  w += align_up((size_t)n * 8);
  ws->c_key = (uint64_t*)w;
  w += align_up((size_t)n * 8);
  ws->key_out = (uint64_t*)w;
  w += align_up((size_t)n * 8);
  ws->s_val = (uint32_t*)w;
  w += align_up((size_t)n * 4);
  ws->c_val = (uint32_t*)w;
  w += align_up((size_t)n * 4);
  ws->cub = w;
  size_t cb = cub_sort_bytes(n);
  cb = std::max(cb, cub_scan32_bytes(d.Pp + 1));
  cb = std::max(cb, cub_scan32_bytes(d.nb + 1));
  cb = std::max(cb, cub_scan64_bytes(d.ns + 1));
  cb = std::max(cb, cub_scan64_bytes(d.nc + 1));
  ws->cub_bytes = align_up(cb);
  w += ws->cub_bytes;
  return (size_t)(w - b);
}

}  // namespace

// ---- the stages of the layout (qsc_obs_readings.cuh declares them; qsc_obs_append.hip runs them
// around its merges) ----
namespace qsc {

size_t rd_ws_carve(char* b, int64_t n, int32_t K, int32_t P, int32_t PT, RdWs* ws) {
  Dims d;
  if (!n_ok(n) || !dims_of(K, P, PT, &d)) return 0;
  return ws_carve(b, n, P, d, ws);
}

bool rd_layout_fits(int32_t K, int32_t P, int32_t PT) {
  Dims d;
  if (!dims_of(K, P, PT, &d)) return false;
  // rd_c_order_kernel's LDS (counts + order, 2 ints per bin) and rd_c_fill_kernel's (Kp + 1
  // segment bounds) against the device's own limit: qsc_obs_layout's rule
  int dev = 0, lds_max = 64 * 1024;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
        v > 0)
      lds_max = v;
  }
  if (d.Kp * 2 * (int64_t)sizeof(int) > lds_max) return false;
  // a sorted reading keeps its index in 24 bits (the wide entry's own field)
  return (int64_t)K < (1 << kIdxBits) && (int64_t)PT < (1 << kIdxBits);
}

int rd_layout_positions(const RdWs& w, int32_t K, int32_t P, int32_t PT, const int32_t* perm,
                        const int32_t* cnt, int32_t* s_width, int64_t* s_off, int* s_seg,
                        hipStream_t s) {
  Dims d;
  if (!dims_of(K, P, PT, &d)) return QSC_EINVAL;
  const int Pp = (int)d.Pp, ns = (int)d.ns;
  QSC_TRY(hipMemsetAsync(w.iperm, 0xFF, (size_t)P * sizeof(int), s));  // -1: no position
  hipLaunchKernelGGL(rd_positions_kernel, dim3((unsigned)ceil_div(Pp + 1, kBlock)), dim3(kBlock),
                     0, s, perm, cnt, P, Pp, w.iperm, w.poscnt);
  QSC_CHECK_LAUNCH();
  hipLaunchKernelGGL(rd_s_width_kernel, dim3((unsigned)ceil_div(ns + 1, kBlock)), dim3(kBlock), 0,
                     s, w.poscnt, ns, s_width, w.s_sizes);
  QSC_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  QSC_TRY(hipcub::DeviceScan::ExclusiveSum(w.cub, cb, w.poscnt, s_seg, Pp + 1, s));
  cb = w.cub_bytes;
  QSC_TRY(hipcub::DeviceScan::ExclusiveSum(w.cub, cb, w.s_sizes, s_off, ns + 1, s));
  return QSC_OK;
}

int rd_layout_keys(const RdWs& w, const int32_t* k, const int32_t* p, const void* code,
                   int32_t code_bytes, int64_t n, int32_t K, int32_t P, int32_t PT, int32_t nbins,
                   hipStream_t s) {
  Dims d;
  if (!dims_of(K, P, PT, &d)) return QSC_EINVAL;
  hipLaunchKernelGGL(rd_keys_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, k, p,
                     code, code_bytes, n, K, P, (int)d.Pp, PT, (int)d.nt, (int)d.Kp, nbins, w.iperm,
                     w.s_key, w.s_val, w.c_key, w.c_val, w.ccount);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

int rd_sort_pairs(const RdWs& w, const uint64_t* key_in, uint64_t* key_out, const uint32_t* val_in,
                  uint32_t* val_out, int64_t n, uint64_t max_key, hipStream_t s) {
  size_t cb = w.cub_bytes;
  QSC_TRY(hipcub::DeviceRadixSort::SortPairs(w.cub, cb, key_in, key_out, val_in, val_out, (int)n,
                                             0, key_bits(max_key), s));
  return QSC_OK;
}

int rd_layout_finish(const RdWs& w, int32_t K, int32_t P, int32_t PT, int32_t nbins,
                     const int* s_seg, const int64_t* s_off, int32_t* c_width, int64_t* c_off,
                     int32_t* c_kmap, int* c_seg, int* c_kinv, qsc_obs_desc* desc,
                     int32_t* max_repeat, hipStream_t s) {
  Dims d;
  if (!dims_of(K, P, PT, &d)) return QSC_EINVAL;
  const int Pp = (int)d.Pp, ns = (int)d.ns, nt = (int)d.nt, nks = (int)d.nks, Kp = (int)d.Kp;
  const int nc = (int)d.nc, nb = (int)d.nb;
  const int wide = (K > 4096 || PT > 4096 || nbins > 15) ? 1 : 0;
  // C-format: bin order and widths per tile, list segments
  hipLaunchKernelGGL(rd_c_order_kernel, dim3((unsigned)nt), dim3(kBlock), Kp * 2 * sizeof(int), s,
                     w.ccount, K, nks, c_width, w.c_sizes, c_kmap, c_kinv);
  QSC_CHECK_LAUNCH();
  size_t cb = w.cub_bytes;
  QSC_TRY(hipcub::DeviceScan::ExclusiveSum(w.cub, cb, w.ccount, c_seg, nb + 1, s));
  cb = w.cub_bytes;
  QSC_TRY(hipcub::DeviceScan::ExclusiveSum(w.cub, cb, w.c_sizes, c_off, nc + 1, s));

  int* scal = (int*)(w.totals + 2);  // [0] nnz, [1] max_repeat
  QSC_TRY(hipMemcpyAsync(w.totals, s_off + ns, 8, hipMemcpyDeviceToDevice, s));
  QSC_TRY(hipMemcpyAsync(w.totals + 1, c_off + nc, 8, hipMemcpyDeviceToDevice, s));
  QSC_TRY(hipMemcpyAsync(scal, s_seg + Pp, sizeof(int), hipMemcpyDeviceToDevice, s));
  int64_t host_tot[3];
  QSC_TRY(hipMemcpyAsync(host_tot, w.totals, sizeof(host_tot), hipMemcpyDeviceToHost, s));
  QSC_TRY(hipStreamSynchronize(s));
  const int32_t nnz = (int32_t)(host_tot[2] & 0xFFFFFFFF);
  const int32_t rep = (int32_t)(host_tot[2] >> 32);
  desc->K = K;
  desc->P = P;
  desc->Pp = Pp;
  desc->PT = PT;
  desc->ntiles = nt;
  desc->nks = nks;
  desc->wide = wide;
  desc->nbins = nbins;
  desc->s_entries = host_tot[0] + QSC_ENTRY_TAIL;
  desc->c_entries = host_tot[1] + QSC_ENTRY_TAIL;
  desc->nnz = nnz;
  desc->rowfmt = 0;
  desc->reserved_ = 0;
  if (max_repeat) *max_repeat = rep;
  return QSC_OK;
}

}  // namespace qsc

extern "C" {

QSC_API int qsc_obs_readings_count(const int32_t* k, const int32_t* p, const void* code,
                                   int32_t code_bytes, int64_t n, int32_t K, int32_t P,
                                   int32_t nbins, int32_t* cnt, int32_t* bad, void* stream) {
  if (!k || !p || !code || !cnt || !bad || !n_ok(n) || K < 1 || P < 1 || nbins < 1 ||
      nbins > QSC_MAX_BOUNDS - 1 || (code_bytes != 1 && code_bytes != 4))
    return QSC_EINVAL;
  hipStream_t s = STREAM(stream);
  QSC_TRY(hipMemsetAsync(cnt, 0, (size_t)P * sizeof(int), s));
  hipLaunchKernelGGL(rd_count_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, k,
                     p, code, code_bytes, n, K, P, nbins, cnt, bad);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API size_t qsc_obs_readings_packed_bytes(int64_t n, int32_t K, int32_t P, int32_t PT) {
  Dims d;
  Packed pk;
  if (!n_ok(n) || !dims_of(K, P, PT, &d)) return 0;
  return packed_carve(nullptr, n, d, &pk);
}

QSC_API size_t qsc_obs_readings_workspace_bytes(int64_t n, int32_t K, int32_t P, int32_t PT) {
  Dims d;
  RdWs ws;
  if (!n_ok(n) || !dims_of(K, P, PT, &d)) return 0;
  return ws_carve(nullptr, n, P, d, &ws);
}

QSC_API int qsc_obs_readings_layout(const int32_t* k, const int32_t* p, const void* code,
                                    int32_t code_bytes, int64_t n, int32_t K, int32_t P,
                                    int32_t PT, int32_t nbins, const int32_t* perm,
                                    const int32_t* cnt, int32_t* s_width, int64_t* s_off,
                                    int32_t* c_width, int64_t* c_off, int32_t* c_kmap,
                                    void* packed, size_t packed_bytes, void* ws, size_t ws_bytes,
                                    qsc_obs_desc* desc, int32_t* max_repeat, void* stream) {
  Dims d;
  if (!k || !p || !code || !perm || !cnt || !s_width || !s_off || !c_width || !c_off || !c_kmap ||
      !packed || !ws || !desc || !n_ok(n) || nbins < 1 || nbins > QSC_MAX_BOUNDS - 1 ||
      (code_bytes != 1 && code_bytes != 4) || !dims_of(K, P, PT, &d))
    return QSC_EINVAL;
  Packed pk;
  RdWs w;
  if (packed_bytes < packed_carve((char*)packed, n, d, &pk) ||
      ws_bytes < ws_carve((char*)ws, n, P, d, &w))
    return QSC_EINVAL;
  if (!rd_layout_fits(K, P, PT)) return QSC_EINVAL;
  const int Pp = (int)d.Pp;
  hipStream_t s = STREAM(stream);

  // positions: inverse pixel order, per-position counts, slice widths, list segments
  int rc = rd_layout_positions(w, K, P, PT, perm, cnt, s_width, s_off, pk.s_seg, s);
  if (rc != QSC_OK) return rc;

  // keys of both orders and the (tile, bin) counts, then the two stable sorts
  QSC_TRY(hipMemsetAsync(w.ccount, 0, (size_t)(d.nb + 1) * sizeof(int), s));
  rc = rd_layout_keys(w, k, p, code, code_bytes, n, K, P, PT, nbins, s);
  if (rc != QSC_OK) return rc;
  rc = rd_sort_pairs(w, w.s_key, w.key_out, w.s_val, pk.s_rd, n, (uint64_t)Pp * (uint64_t)K, s);
  if (rc != QSC_OK) return rc;
  int* scal = (int*)(w.totals + 2);  // [0] nnz, [1] max_repeat
  QSC_TRY(hipMemsetAsync(scal, 0, 2 * sizeof(int64_t), s));
  hipLaunchKernelGGL(rd_max_repeat_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s,
                     w.key_out, pk.s_seg + Pp, n, scal + 1);
  QSC_CHECK_LAUNCH();
  rc = rd_sort_pairs(w, w.c_key, w.key_out, w.c_val, pk.c_rd, n,
                     (uint64_t)d.nt * (uint64_t)d.Kp * (uint64_t)PT, s);
  if (rc != QSC_OK) return rc;

  // C-format bin order, widths, offsets and list segments; the totals; the descriptor
  return rd_layout_finish(w, K, P, PT, nbins, pk.s_seg, s_off, c_width, c_off, c_kmap, pk.c_seg,
                          pk.c_kinv, desc, max_repeat, s);
}

QSC_API int qsc_obs_readings_fill(const void* packed, size_t packed_bytes, int64_t n,
                                  const qsc_obs_desc* d, const int32_t* s_width,
                                  const int64_t* s_off, const int32_t* c_width,
                                  const int64_t* c_off, const int32_t* c_kmap, void* s_entries,
                                  void* c_entries, void* stream) {
  Dims dm;
  Packed pk;
  if (!s_width || !s_off || !c_width || !c_off || !c_kmap || !s_entries || !c_entries ||
      !packed_of(packed, packed_bytes, n, d, &dm, &pk, /*counted=*/false) ||
      d->s_entries < QSC_ENTRY_TAIL || d->c_entries < QSC_ENTRY_TAIL)
    return QSC_EINVAL;
  // signed rows: narrow entries, every row index (up to the last pad row) representable
  const int sr = d->rowfmt == 1 ? 1 : 0;
  if (d->rowfmt != 0 && (d->rowfmt != 1 || d->wide || (int64_t)sr_rows(d->K) > 0x10000 ||
                         (int64_t)sr_rows(d->PT) > 0x10000 || d->nbins != 2))
    return QSC_EINVAL;
  if (!d->wide && (d->K > 4096 || d->PT > 4096 || d->nbins > 15)) return QSC_EINVAL;
  hipStream_t s = STREAM(stream);
  const dim3 tg((QSC_ENTRY_TAIL + kBlock - 1) / kBlock), tb(kBlock);
  const dim3 sg((unsigned)ceil_div(dm.ns, kBlock / 64)), cg((unsigned)dm.nt);
  const size_t cshm = (size_t)(dm.Kp + 1) * sizeof(int);
  const int ns = (int)dm.ns;
  if (d->wide) {
    hipLaunchKernelGGL(tail_fill_kernel<uint32_t>, tg, tb, 0, s, (uint32_t*)s_entries,
                       d->s_entries - QSC_ENTRY_TAIL, QSC_ENTRY_TAIL, 0, d->K);
    hipLaunchKernelGGL(tail_fill_kernel<uint32_t>, tg, tb, 0, s, (uint32_t*)c_entries,
                       d->c_entries - QSC_ENTRY_TAIL, QSC_ENTRY_TAIL, 0, d->PT);
    hipLaunchKernelGGL(rd_s_fill_kernel<uint32_t>, sg, dim3(kBlock), 0, s, pk.s_rd, pk.s_seg, n,
                       ns, d->K, s_width, s_off, (uint32_t*)s_entries, 0);
    QSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(rd_c_fill_kernel<uint32_t>, cg, dim3(kBlock), cshm, s, pk.c_rd, pk.c_seg, n,
                       d->K, d->PT, d->nks, c_width, c_off, c_kmap, pk.c_kinv,
                       (uint32_t*)c_entries, 0);
  } else {
    hipLaunchKernelGGL(tail_fill_kernel<uint16_t>, tg, tb, 0, s, (uint16_t*)s_entries,
                       d->s_entries - QSC_ENTRY_TAIL, QSC_ENTRY_TAIL, sr, d->K);
    hipLaunchKernelGGL(tail_fill_kernel<uint16_t>, tg, tb, 0, s, (uint16_t*)c_entries,
                       d->c_entries - QSC_ENTRY_TAIL, QSC_ENTRY_TAIL, sr, d->PT);
    hipLaunchKernelGGL(rd_s_fill_kernel<uint16_t>, sg, dim3(kBlock), 0, s, pk.s_rd, pk.s_seg, n,
                       ns, d->K, s_width, s_off, (uint16_t*)s_entries, sr);
    QSC_CHECK_LAUNCH();
    hipLaunchKernelGGL(rd_c_fill_kernel<uint16_t>, cg, dim3(kBlock), cshm, s, pk.c_rd, pk.c_seg, n,
                       d->K, d->PT, d->nks, c_width, c_off, c_kmap, pk.c_kinv,
                       (uint16_t*)c_entries, sr);
  }
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
