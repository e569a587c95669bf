// Row walk, lane-group reductions and launch grids shared by the krca_graph_* translation units
// (graph_struct.hip, graph_reach.hip).  Everything here has internal linkage.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "krca_common.h"

namespace {

constexpr int TPB = 256;
constexpr int kBatchMax = 32;   // rounds between two read-backs, at most


__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// reductions over an aligned group of W lanes (W = 64: the wave); every lane gets the result
template <int W>
__device__ __forceinline__ int32_t grp_max(int32_t x) {
  for (int m = W / 2; m; m >>= 1) x = max(x, __shfl_xor(x, m, 64));
  return x;
}
template <int W>
__device__ __forceinline__ int32_t grp_min(int32_t x) {
  for (int m = W / 2; m; m >>= 1) x = min(x, __shfl_xor(x, m, 64));
  return x;
}
template <int W>
__device__ __forceinline__ int32_t grp_sum(int32_t x) {
  for (int m = W / 2; m; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
template <int W>
__device__ __forceinline__ uint64_t grp_min_u64(uint64_t x) {
  for (int m = W / 2; m; m >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), m, 64);
    const uint64_t y = ((uint64_t)hi << 32) | lo;
    x = y < x ? y : x;
  }
  return x;
}
template <int W>
__device__ __forceinline__ uint64_t grp_or_u64(uint64_t x) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  for (int m = W / 2; m; m >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, m, 64);
    hi |= (uint32_t)__shfl_xor((int)hi, m, 64);
  }
  return ((uint64_t)hi << 32) | lo;
}
template <int W>
__device__ __forceinline__ bool grp_any(bool p) {
  return grp_max<W>(p ? 1 : 0) != 0;
}
__device__ __forceinline__ bool wave_any(bool p) { return __ballot(p) != 0; }

__device__ __forceinline__ bool in_range(int32_t c, int64_t N) { return (uint64_t)(int64_t)c < (uint64_t)N; }

template <int W>
struct Width {
  static constexpr int value = W;
};

// Row walk: f(Width<w>, r) runs once per row r of [0, N) on an aligned group of w lanes, all of them
// with the same r.  W = 64: a wave per row.  W = 16: four rows per wave and step, for graphs of short
// rows; a row above kLongRow entries is left to the whole wave (f(Width<64>, r)) once the wave's short
// rows are done, so a hub row is never walked 16 entries at a time.  Waves stride over the rows.
constexpr int kLongRow = 512;
template <int W, class F>
__device__ __forceinline__ void for_rows(const int64_t* __restrict__ row_ptr, int64_t N, F f) {
  constexpr int G = 64 / W;
  const int64_t wave = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * TPB) >> 6;
  for (int64_t base = wave * G; base < N; base += nw * G) {  // wave-uniform
    if (W == 64) {
      f(Width<64>{}, base);
      continue;
    }
    const int64_t r = base + lane_id() / W;
    bool lng = false;
    if (r < N) {
      lng = row_ptr[r + 1] - row_ptr[r] > kLongRow;
      if (!lng) f(Width<W>{}, r);
    }
    uint64_t todo = __ballot(lng && (lane_id() & (W - 1)) == 0);
    while (todo) {  // wave-uniform
      const int l = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      f(Width<64>{}, base + l / W);
    }
  }
}
// the entries of row r, w per step; e is this lane's entry
#define GS_ENTRIES(e, r, w) \
  for (int64_t e = row_ptr[r] + (threadIdx.x & ((w)-1)), gs_e1 = row_ptr[(r) + 1]; e < gs_e1; e += (w))
#define GS_LEADER(w) ((threadIdx.x & ((w)-1)) == 0)
#define GS_NODES(v) \
  for (int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x, gs_nt = (int64_t)gridDim.x * TPB; v < N; v += gs_nt)

// ---- host side ----------------------------------------------------------------------------------

inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

struct Grid {
  unsigned rows, nodes;
  bool wide;  // a wave per row (else 16 lanes per row)
};
// E = row_ptr[N] is read back (the one thing the host needs to know of the graph): rows of 32 entries
// or more on average get a wave each
int grid_of(const int64_t* row_ptr, int64_t N, hipStream_t st, Grid* g) {
  int64_t E = 0;
  KRCA_HIP(hipMemcpyAsync(&E, row_ptr + N, sizeof(E), hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  const int cap_knob = krca::tuning().graph_grid;
  const int64_t cap = cap_knob > 0 ? cap_knob : (1 << 20);
  g->wide = E >= 32 * N;
  const int64_t rows_per_wg = (TPB / 64) * (g->wide ? 1 : 4);
  g->rows = (unsigned)std::max<int64_t>(1, std::min(cap, krca::ceil_div(N, rows_per_wg)));
  g->nodes = (unsigned)std::max<int64_t>(1, std::min(cap, krca::ceil_div(N, TPB)));
  return KRCA_OK;
}
// launch a row kernel K<..., W> at the grid's row width
#define GS_ROWS_LAUNCH(g, st, K, ...)                                                                      \
  do {                                                                                                     \
    if ((g).wide) hipLaunchKernelGGL(HIP_KERNEL_NAME(K<64>), dim3((g).rows), dim3(TPB), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(K<16>), dim3((g).rows), dim3(TPB), 0, st, __VA_ARGS__);        \
  } while (0)
#define GS_ROWS_LAUNCH_PULL(g, st, pull, K, ...)                                                              \
  do {                                                                                                        \
    if (pull) {                                                                                               \
      if ((g).wide) hipLaunchKernelGGL(HIP_KERNEL_NAME(K<1, 64>), dim3((g).rows), dim3(TPB), 0, st, __VA_ARGS__); \
      else hipLaunchKernelGGL(HIP_KERNEL_NAME(K<1, 16>), dim3((g).rows), dim3(TPB), 0, st, __VA_ARGS__);      \
    } else {                                                                                                  \
      if ((g).wide) hipLaunchKernelGGL(HIP_KERNEL_NAME(K<0, 64>), dim3((g).rows), dim3(TPB), 0, st, __VA_ARGS__); \
      else hipLaunchKernelGGL(HIP_KERNEL_NAME(K<0, 16>), dim3((g).rows), dim3(TPB), 0, st, __VA_ARGS__);      \
    }                                                                                                         \
  } while (0)

int batch_max(int64_t N) { return N < 16384 ? kBatchMax : (N < 262144 ? 4 : 1); }

}  // namespace
