// Onset precedence pass (krca_rca_precede / krca_rca_first_mover_key).
//
// What explain.hip does for scores, for episode onsets (krca_rolling_timeline): over the pull-CSR
// (row k = the callers j of k, edges j -> k) and the per-pod onset step (onset < 0: no sustained
// episode), every edge j -> k with j != k between two pods that have an onset is classified
//   k earlier than j   onset_k + slack < onset_j   (the dependency went first: j is a follower)
//   k later than j     onset_j + slack < onset_k
//   concurrent         otherwise.
// Per caller j (over the rows j appears in): dep_earlier, dep_concurrent (int32 atomic adds) and
// dep_first = min ((int64)onset_k << 32 | k) over its earlier dependencies (64-bit atomic min;
// INT64_MAX: none).  Per callee k: caller_later, caller_concurrent, caller_earlier, reduced inside
// the wave that walks row k (no atomics).  Integer counts and an integer min: the result does not
// depend on the schedule.
//
// Only the rows of pods with an onset are walked -- the same shape as explain.hip: compact their
// ids (wave ballot, one atomic per wave), then a wave per listed pod with lanes striding the row.
// A first mover is a pod with an onset and no earlier dependency; its key orders first movers by
// the callers that follow it, then by the episode's peak.
#include <algorithm>

#include "krca_common.h"

namespace {

constexpr int TPB = 256;
constexpr int64_t kListGrid = 1024;  // workgroups (4 waves each) walking the listed pods' rows

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(TPB) void precede_list(const int32_t* __restrict__ onset, int64_t N,
                                                    int32_t* __restrict__ list, uint32_t* __restrict__ n_list) {
  const int lane = threadIdx.x & 63;
  // block-uniform trip count: every lane of a wave runs the same iterations (the ballot needs them)
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < N; base += (int64_t)gridDim.x * TPB) {
    const int64_t i = base + threadIdx.x;
    const bool a = i < N && onset[i] >= 0;
    const unsigned long long m = __ballot(a);
    if (m == 0ull) continue;  // wave-uniform
    const int leader = __ffsll(m) - 1;
    uint32_t off = 0;
    if (lane == leader) off = atomicAdd(n_list, (uint32_t)__popcll(m));
    off = __shfl(off, leader, 64);
    if (a) {
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      list[off + below] = (int32_t)i;  // off + below < number of pods with an onset <= N
    }
  }
}

__global__ __launch_bounds__(TPB) void precede_rows(const int32_t* __restrict__ list,
                                                    const uint32_t* __restrict__ n_list,
                                                    const int32_t* __restrict__ onset, int64_t slack,
                                                    const int64_t* __restrict__ row_ptr,
                                                    const int32_t* __restrict__ col,
                                                    int32_t* __restrict__ dep_earlier,
                                                    int32_t* __restrict__ dep_concurrent,
                                                    unsigned long long* __restrict__ dep_first,
                                                    int32_t* __restrict__ caller_later,
                                                    int32_t* __restrict__ caller_concurrent,
                                                    int32_t* __restrict__ caller_earlier) {
  const int lane = threadIdx.x & 63;
  const int64_t n = *n_list;
  for (int64_t w = ((int64_t)blockIdx.x * TPB + threadIdx.x) >> 6; w < n; w += ((int64_t)gridDim.x * TPB) >> 6) {
    const int32_t k = list[w];
    const int64_t ok = onset[k];  // >= 0: k is listed
    const unsigned long long first = ((unsigned long long)ok << 32) | (uint32_t)k;
    const int64_t e1 = row_ptr[k + 1];
    int later = 0, conc = 0, earlier = 0;
    for (int64_t e = row_ptr[k] + lane; e < e1; e += 64) {
      const int32_t j = col[e];
      if (j == k) continue;
      const int64_t oj = onset[j];
      if (oj < 0) continue;
      if (ok + slack < oj) {  // k went first: j follows it
        ++later;
        atomicAdd(dep_earlier + j, 1);
        atomicMin(dep_first + j, first);
      } else if (oj + slack < ok) {
        ++earlier;
      } else {
        ++conc;
        atomicAdd(dep_concurrent + j, 1);
      }
    }
    later = wave_sum(later);
    conc = wave_sum(conc);
    earlier = wave_sum(earlier);
    if (lane == 0) {
      caller_later[k] = later;
      caller_concurrent[k] = conc;
      caller_earlier[k] = earlier;
    }
  }
}

__global__ __launch_bounds__(TPB) void first_mover_key(const int32_t* __restrict__ onset,
                                                       const float* __restrict__ peak,
                                                       const int32_t* __restrict__ dep_earlier,
                                                       const int32_t* __restrict__ caller_later,
                                                       const int32_t* __restrict__ caller_concurrent, int64_t N,
                                                       int64_t* __restrict__ key) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    int64_t kv = 0;
    if (onset[i] >= 0 && dep_earlier[i] == 0) {
      const int64_t f = std::min<int64_t>((int64_t)caller_later[i] + (int64_t)caller_concurrent[i], (1 << 20) - 1);
      kv = (f << 32) | (int64_t)__float_as_uint(peak[i]);  // peak >= 0: its bits order as the float does
    }
    key[i] = kv;
  }
}

}  // namespace

extern "C" {

// workspace: list int32[N] | counter (256 B)
int64_t krca_rca_precede_ws_size(int64_t N) { return 4 * std::max<int64_t>(N, 1) + 256; }

int krca_rca_precede(const int32_t* onset, int64_t N, int32_t slack, const int64_t* row_ptr, const int32_t* col,
                     int32_t* dep_earlier, int32_t* dep_concurrent, int64_t* dep_first, int32_t* caller_later,
                     int32_t* caller_concurrent, int32_t* caller_earlier, void* ws, void* stream) {
  KRCA_CHECK_ARG(N > 0 && N < INT32_MAX && slack >= 0, "krca_rca_precede: bad sizes N=%lld slack=%d", (long long)N,
                 slack);
  KRCA_CHECK_ARG(onset && row_ptr && col && dep_earlier && dep_concurrent && dep_first && caller_later &&
                     caller_concurrent && caller_earlier && ws,
                 "krca_rca_precede: null pointer");
  KRCA_CHECK_ARG(((uintptr_t)ws & 3) == 0, "krca_rca_precede: workspace must be 4-byte aligned");
  hipStream_t st = krca::as_stream(stream);
  int32_t* list = reinterpret_cast<int32_t*>(ws);
  uint32_t* n_list = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + 4 * N);
  KRCA_HIP(hipMemsetAsync(n_list, 0, sizeof(uint32_t), st));
  for (int32_t* p : {dep_earlier, dep_concurrent, caller_later, caller_concurrent, caller_earlier})
    KRCA_HIP(hipMemsetAsync(p, 0, N * sizeof(int32_t), st));
  const int rc = krca_fill_i64(dep_first, N, INT64_MAX, stream);
  if (rc != KRCA_OK) return rc;
  const unsigned g0 = (unsigned)std::min<int64_t>(krca::ceil_div(N, TPB), 2048);
  hipLaunchKernelGGL(precede_list, dim3(g0), dim3(TPB), 0, st, onset, N, list, n_list);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(precede_rows, dim3((unsigned)kListGrid), dim3(TPB), 0, st, list, n_list, onset, (int64_t)slack,
                     row_ptr, col, dep_earlier, dep_concurrent, reinterpret_cast<unsigned long long*>(dep_first),
                     caller_later, caller_concurrent, caller_earlier);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

int krca_rca_first_mover_key(const int32_t* onset, const float* peak, const int32_t* dep_earlier,
                             const int32_t* caller_later, const int32_t* caller_concurrent, int64_t N, int64_t* key,
                             void* stream) {
  KRCA_CHECK_ARG(N > 0, "krca_rca_first_mover_key: bad size");
  KRCA_CHECK_ARG(onset && peak && dep_earlier && caller_later && caller_concurrent && key,
                 "krca_rca_first_mover_key: null pointer");
  const unsigned g = (unsigned)std::min<int64_t>(krca::ceil_div(N, TPB), 2048);
  hipLaunchKernelGGL(first_mover_key, dim3(g), dim3(TPB), 0, krca::as_stream(stream), onset, peak, dep_earlier,
                     caller_later, caller_concurrent, N, key);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

}  // extern "C"
