// qsc_smooth.hip — spatial smoothness prior on the loss fields S_r(i,j), evaluated in the
// solver's position-ordered layout (include/qsc.h: S [Pp][RP], one 16/32/64-byte row per position).
//
//   R(S) = sum_r sum_{edges {p,p'}} rho(S_r(p) - S_r(p'))      4-neighbour grid graph, each edge once
//   quad:   rho(d) = d^2 / 2                         rho'(d) = d
//   huber:  rho(d) = d^2 / (2 delta)  (|d| <= delta) rho'(d) = clamp(d / delta, -1, 1)
//           rho(d) = |d| - delta / 2  (otherwise)
//
// The reference has no spatial prior on S (its S-side regulariser is lambda_s ||Z||_F,
// qmc/qmc.ipynb :573, :631, and the prior is the generator itself); this is the build's own
// Tikhonov / anisotropic-TV term for the free-S solver.
//
// Neighbour table: positions are pixels sorted by observation count, so the four grid neighbours
// of a position sit anywhere in S.  qsc_smooth_neighbors resolves perm -> pixel -> neighbour
// pixel -> position once per observation set into nbr[Pp][4] (left, right, up, down; -1 = none),
// and the per-iteration kernel gathers through that one table.
//
// Lane mapping of smooth_grad_kernel: one thread per float4 chunk of a position row (RP / 4
// threads per position), so a row and its four neighbour rows are read as whole dwordx4 loads
// and consecutive lanes cover consecutive bytes of S and dS.  The penalty is reduced in a fixed
// order: lanes of a wave (butterfly), waves of a block, one partial per block in the workspace,
// then one block sums the partials (smooth_finish_kernel) -- no floating-point atomics, so two
// runs agree bit for bit.
#include <hip/hip_runtime.h>

#include "qsc_common.cuh"

namespace {
using namespace qsc;

constexpr int kBlock = 256;
// position bound: the neighbour table is 16 bytes per position and one penalty partial is kept
// per block; beyond this the index arithmetic of the launches (grid sizes as 32-bit) is not
// exercised by any test, so such calls are refused
constexpr int64_t kSmoothMaxPp = (int64_t)1 << 28;
// workspace: a 16-byte header (word 0: the history step counter, owned by the caller between
// calls) followed by max(Pp, partials) 4-byte words (the inverse permutation of
// qsc_smooth_neighbors / the per-block penalty partials of qsc_smooth_grad)
constexpr size_t kHeader = 16;

enum { SMOOTH_QUAD = 0, SMOOTH_HUBER = 1 };

__global__ void __launch_bounds__(kBlock) iperm_clear_kernel(int* __restrict__ iperm, int P) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p < P) iperm[p] = -1;
}

__global__ void __launch_bounds__(kBlock) iperm_fill_kernel(const int* __restrict__ perm, int P,
                                                            int Pp, int* __restrict__ iperm) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= Pp) return;
  const int p = perm[q];
  if (p >= 0 && p < P) iperm[p] = (int)q;
}

__global__ void __launch_bounds__(kBlock) neighbors_kernel(const int* __restrict__ perm,
                                                           const int* __restrict__ iperm, int P,
                                                           int Pp, int I, int J,
                                                           int4* __restrict__ nbr) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= Pp) return;
  const int p = perm[q];
  int4 n = make_int4(-1, -1, -1, -1);
  if (p >= 0 && p < P) {
    const int i = p / J, j = p - i * J;
    if (j > 0) n.x = iperm[p - 1];
    if (j + 1 < J) n.y = iperm[p + 1];
    if (i > 0) n.z = iperm[p - J];
    if (i + 1 < I) n.w = iperm[p + J];
    // (a pixel that perm does not list has no position: -1, as outside the grid)
    if (n.x >= Pp) n.x = -1;
    if (n.y >= Pp) n.y = -1;
    if (n.z >= Pp) n.z = -1;
    if (n.w >= Pp) n.w = -1;
  }
  nbr[q] = n;
}

// rho(d) and rho'(d) of one difference; ka = 1 (quad) or 1 / delta (huber), hd = delta / 2
template <int KIND>
__device__ __forceinline__ void rho(float d, float ka, float hd, float& val, float& der) {
  if (KIND == SMOOTH_QUAD) {
    val = 0.5f * d * d;
    der = d;
  } else {
    const float z = d * ka;  // d / delta
    const float ad = fabsf(d);
    const bool in = fabsf(z) <= 1.0f;
    val = in ? 0.5f * d * z : ad - hd;
    der = fminf(fmaxf(z, -1.0f), 1.0f);
  }
}

template <int RP, int KIND>
__global__ void __launch_bounds__(kBlock) smooth_grad_kernel(
    const float4* __restrict__ S, const int4* __restrict__ nbr, int R, int Pp, float ka, float hd,
    float weight, float4* __restrict__ dS, float* __restrict__ part) {
  constexpr int CH = RP / 4;  // float4 chunks (threads) per position
  __shared__ float sh[kBlock / 64];
  const int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  const int64_t q = t / CH;
  const int c = (int)(t - q * CH);
  float pen = 0.0f;
  if (q < Pp) {
    const int4 n = nbr[q];
    const int nn[4] = {n.x, n.y, n.z, n.w};
    bool any = false;
    float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 s4 = S[q * CH + c];
    float v[4][4];  // [neighbour][row element], in registers (every loop below is unrolled)
    bool has[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      has[e] = nn[e] >= 0 && nn[e] < Pp;  // (a table entry out of range is read as "none")
      any = any || has[e];
      const float4 x = has[e] ? S[(int64_t)nn[e] * CH + c] : zero;
      v[e][0] = x.x;
      v[e][1] = x.y;
      v[e][2] = x.z;
      v[e][3] = x.w;
    }
    if (any) {
      const float s[4] = {s4.x, s4.y, s4.z, s4.w};
      float g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        g[j] = 0.0f;
        const bool live = c * 4 + j < R;  // rows r >= R carry no field
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float val, der;
          rho<KIND>(s[j] - v[e][j], ka, hd, val, der);
          if (has[e] && live) {
            g[j] += der;
            // each edge once, from its left (e == 1: right neighbour) or upper (e == 3: down
            // neighbour) end
            if (e == 1 || e == 3) pen += val;
          }
        }
      }
      if (dS != nullptr && c * 4 < R) {
        float4 d = dS[q * CH + c];
        d.x = c * 4 + 0 < R ? __builtin_fmaf(weight, g[0], d.x) : d.x;
        d.y = c * 4 + 1 < R ? __builtin_fmaf(weight, g[1], d.y) : d.y;
        d.z = c * 4 + 2 < R ? __builtin_fmaf(weight, g[2], d.z) : d.z;
        d.w = c * 4 + 3 < R ? __builtin_fmaf(weight, g[3], d.w) : d.w;
        dS[q * CH + c] = d;
      }
    }
  }
  const float r = block_sum(pen, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// One block: the fixed-order sum of the per-block partials -> *pen, and the history row chosen
// by the caller-owned step counter (rows beyond cap are dropped, as qsc_cfinish drops its own)
__global__ void __launch_bounds__(kBlock) smooth_finish_kernel(const float* __restrict__ part,
                                                               int nparts, float* __restrict__ pen,
                                                               float* __restrict__ hist, int cap,
                                                               int* __restrict__ step) {
  __shared__ float sh[kBlock / 64];
  float s = 0.0f;
  for (int i = threadIdx.x; i < nparts; i += kBlock) s += part[i];
  const float r = block_sum(s, sh);
  if (threadIdx.x == 0) {
    if (pen != nullptr) pen[0] = r;
    if (hist != nullptr) {
      const int it = step[0];
      if (it >= 0 && it < cap) hist[it] = r;
      step[0] = it + 1;
    }
  }
}

inline int64_t grad_blocks(int64_t Pp, int RP) { return ceil_div(Pp * (RP / 4), kBlock); }

inline size_t smooth_ws_bytes(int64_t Pp) {
  // the inverse permutation (<= Pp words) or the partials at the widest rank (Pp * 4 / 256)
  return kHeader + (size_t)Pp * sizeof(int32_t);
}

}  // namespace

extern "C" {

QSC_API size_t qsc_smooth_workspace_bytes(int32_t Pp) {
  if (Pp < 1 || (int64_t)Pp > kSmoothMaxPp) return 0;
  return smooth_ws_bytes(Pp);
}

QSC_API int qsc_smooth_neighbors(const int32_t* perm, int32_t P, int32_t Pp, int32_t I, int32_t J,
                                 int32_t* nbr, void* ws, size_t ws_bytes, void* stream) {
  if (!perm || !nbr || !ws || I < 1 || J < 1 || P < 1 || Pp < P || (int64_t)I * J != (int64_t)P)
    return QSC_EINVAL;
  if ((int64_t)Pp > kSmoothMaxPp) return QSC_EUNSUPPORTED;
  if (ws_bytes < smooth_ws_bytes(Pp)) return QSC_EINVAL;
  int* iperm = reinterpret_cast<int*>(static_cast<char*>(ws) + kHeader);
  hipStream_t hs = STREAM(stream);
  const dim3 blk(kBlock);
  hipLaunchKernelGGL(iperm_clear_kernel, dim3((unsigned)ceil_div(P, kBlock)), blk, 0, hs, iperm, P);
  QSC_CHECK_LAUNCH();
  hipLaunchKernelGGL(iperm_fill_kernel, dim3((unsigned)ceil_div(Pp, kBlock)), blk, 0, hs, perm, P,
                     Pp, iperm);
  QSC_CHECK_LAUNCH();
  hipLaunchKernelGGL(neighbors_kernel, dim3((unsigned)ceil_div(Pp, kBlock)), blk, 0, hs, perm,
                     iperm, P, Pp, I, J, reinterpret_cast<int4*>(nbr));
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

QSC_API int qsc_smooth_grad(const float* S, const int32_t* nbr, int32_t R, int32_t Pp,
                            int32_t kind, float delta, float weight, float* dS, float* pen,
                            float* pen_hist, int32_t hist_cap, void* ws, size_t ws_bytes,
                            void* stream) {
  if (!S || !nbr || !ws || R < 1 || R > QSC_MAX_R || Pp < 1 || (!pen && !pen_hist) ||
      (pen_hist && hist_cap < 1))
    return QSC_EINVAL;
  if (kind != SMOOTH_QUAD && kind != SMOOTH_HUBER) return QSC_EINVAL;
  if (kind == SMOOTH_HUBER && !(delta > 0.0f)) return QSC_EINVAL;
  if ((int64_t)Pp > kSmoothMaxPp) return QSC_EUNSUPPORTED;
  if (ws_bytes < smooth_ws_bytes(Pp)) return QSC_EINVAL;
  const int RP = qsc_rank_pad(R);
  int* step = static_cast<int*>(ws);
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + kHeader);
  const int64_t nblk = grad_blocks(Pp, RP);  // <= Pp / 16 + 1 words: inside the workspace
  const float ka = kind == SMOOTH_HUBER ? 1.0f / delta : 1.0f;
  const float hd = kind == SMOOTH_HUBER ? 0.5f * delta : 0.0f;
  hipStream_t hs = STREAM(stream);
  const dim3 grid((unsigned)nblk), blk(kBlock);
  const float4* S4 = reinterpret_cast<const float4*>(S);
  const int4* n4 = reinterpret_cast<const int4*>(nbr);
  float4* d4 = reinterpret_cast<float4*>(dS);
#define QSC_SMOOTH_LAUNCH(RPV)                                                                 \
  do {                                                                                         \
    if (kind == SMOOTH_QUAD)                                                                   \
      hipLaunchKernelGGL((smooth_grad_kernel<RPV, SMOOTH_QUAD>), grid, blk, 0, hs, S4, n4, R,  \
                         Pp, ka, hd, weight, d4, part);                                        \
    else                                                                                       \
      hipLaunchKernelGGL((smooth_grad_kernel<RPV, SMOOTH_HUBER>), grid, blk, 0, hs, S4, n4, R, \
                         Pp, ka, hd, weight, d4, part);                                        \
  } while (0)
  if (RP == 4)
    QSC_SMOOTH_LAUNCH(4);
  else if (RP == 8)
    QSC_SMOOTH_LAUNCH(8);
  else
    QSC_SMOOTH_LAUNCH(16);
#undef QSC_SMOOTH_LAUNCH
  QSC_CHECK_LAUNCH();
  hipLaunchKernelGGL(smooth_finish_kernel, dim3(1), blk, 0, hs, part, (int)nblk, pen, pen_hist,
                     hist_cap, step);
  QSC_CHECK_LAUNCH();
  return QSC_OK;
}

}  // extern "C"
