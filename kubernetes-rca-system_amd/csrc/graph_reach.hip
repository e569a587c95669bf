// Blast radius of up to 64 sources on the device: bit-parallel multi-source BFS over
// the dependency CSR and the greedy cover of the marked nodes by the sources' radii.
//
// One 64-bit word per node carries all sources: bit k of reach[v] = source k reaches v.  A level is one
// round over the CSR in either layout, without a transpose (as graph_struct.hip): the end of an edge
// the bits flow TO is the receiver.  When the row is the receiver (pull == dir) it GATHERS: a row whose
// word already holds all K bits is skipped, any other ORs front[c] over its
// entries and commits new = acc & ~seen in place (the frontier is double-buffered, so one kernel is a
// level).  When the row is the sender (pull != dir: the PageRank pull-CSR asked for dependents) it
// SCATTERS: a row with an empty frontier word costs that one read, any other reads seen[c] per entry
// and issues a non-returning 64-bit atomicOr into nxt[c] only where it adds a bit; a per-node kernel
// then commits new = nxt & ~seen, seen |= new, front = new, nxt = 0.  `seen` is the caller's reach array.
//
// Tallies: the nodes a bit gained in a level are counted per wave (one ballot per bit that is set in
// any lane's new word, once more under `mark`), summed per workgroup in LDS and flushed with one 64-bit
// atomic per non-zero counter into the level's histogram bin; no per-node histogram traffic.  A level
// that flushed nothing changed nothing: the host stops there.  Every output is an integer function of
// the edge set, so both layouts and every schedule give the same bytes.
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "graph_rows.h"

namespace {

constexpr int kTab = 65;  // counters per channel of the LDS table: 64 bits + one total (cover only)
// workspace: int32 changed[32] | int32 depth[64] at 512 | u64 counts[2][kTab] (cover) | u64 tally[64][2][64] |
// two u64 [N] arrays
constexpr int64_t kDepthOff = 512, kCountsOff = 768, kTallyOff = 2048, kArraysOff = kTallyOff + 64 * 128 * 8;
static_assert(kCountsOff + 2 * kTab * 8 <= kTallyOff && kArraysOff % 256 == 0, "workspace layout");

typedef unsigned long long u64;

struct Sources {
  int32_t v[KRCA_REACH_MAX_SRC];
};

__device__ __forceinline__ void tab_clear(u64* tab) {
  for (int i = threadIdx.x; i < 2 * kTab; i += TPB) tab[i] = 0;
  __syncthreads();
}

// For every bit k set in some active lane's `bits`: tab[k] += the lanes that have it, tab[kTab + k] +=
// those of them with `flag`.  May be called by a part of the wave: only active lanes vote and are read.
__device__ __forceinline__ void tally_bits(uint64_t bits, bool flag, u64* tab) {
  uint64_t todo = bits;
  for (;;) {
    const uint64_t any = __ballot(todo != 0);
    if (!any) break;  // uniform over the active lanes
    const int from = __ffsll((u64)any) - 1;
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)todo, from, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(todo >> 32), from, 64);
    const int k = __ffsll((u64)(((uint64_t)hi << 32) | lo)) - 1;
    const bool has = (bits >> k) & 1;
    const int n = __popcll(__ballot(has)), nf = __popcll(__ballot(has && flag));
    todo &= ~(1ull << k);
    if (lane_id() == from) {
      atomicAdd(&tab[k], (u64)n);
      if (nf) atomicAdd(&tab[kTab + k], (u64)nf);
    }
  }
}

// the workgroup's counters into the level's bin ([2][64]); a bit that gained a node: depth, changed
__device__ __forceinline__ void level_flush(const u64* tab, u64* __restrict__ bin, int32_t* __restrict__ depth,
                                            int32_t level, int32_t* __restrict__ changed) {
  __syncthreads();
  for (int i = threadIdx.x; i < 128; i += TPB) {
    const u64 c = tab[(i >> 6) * kTab + (i & 63)];
    if (!c) continue;
    atomicAdd(&bin[i], c);
    if (i < 64) {
      atomicMax(&depth[i], level);
      *changed = 1;
    }
  }
}

__global__ __launch_bounds__(TPB) void gr_init(int64_t N, uint64_t* __restrict__ seen, uint64_t* __restrict__ a,
                                               uint64_t* __restrict__ b) {
  GS_NODES(v) {
    seen[v] = 0;
    a[v] = 0;
    b[v] = 0;
  }
}

// level 0: source k is at distance 0 from itself (duplicate sources share a node: atomicOr)
__global__ void gr_seed(Sources src, int32_t K, uint64_t* __restrict__ seen, uint64_t* __restrict__ front,
                        const uint8_t* __restrict__ mark, u64* __restrict__ tally, int32_t* __restrict__ depth) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const int32_t s = src.v[k];
  atomicOr(reinterpret_cast<u64*>(&seen[s]), 1ull << k);
  atomicOr(reinterpret_cast<u64*>(&front[s]), 1ull << k);
  tally[k] = 1;
  tally[64 + k] = mark ? (mark[s] != 0 ? 1 : 0) : 1;
  depth[k] = 0;
}

// the row is the receiver
template <int W>
__global__ __launch_bounds__(TPB) void gr_gather(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                 int64_t N, const uint64_t* __restrict__ front,
                                                 uint64_t* __restrict__ front_out, uint64_t* __restrict__ seen,
                                                 const uint8_t* __restrict__ mark, uint64_t full, int32_t level,
                                                 u64* __restrict__ bin, int32_t* __restrict__ depth,
                                                 int32_t* __restrict__ changed) {
  __shared__ u64 tab[2 * kTab];
  tab_clear(tab);
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    const uint64_t s = seen[r];
    uint64_t nw = 0;
    if (s != full) {  // the same for the row's w lanes
      uint64_t acc = 0;
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (in_range(c, N)) acc |= front[c];
      }
      nw = grp_or_u64<w>(acc) & ~s;
    }
    const bool lead = GS_LEADER(w);
    if (lead) {
      front_out[r] = nw;
      if (nw) seen[r] = s | nw;
    }
    const bool hit = lead && nw != 0;
    tally_bits(hit ? nw : 0, hit && (mark ? mark[r] != 0 : true), tab);
  });
  level_flush(tab, bin, depth, level, changed);
}

// the row is the sender
template <int W>
__global__ __launch_bounds__(TPB) void gr_scatter(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                  int64_t N, const uint64_t* __restrict__ front,
                                                  const uint64_t* __restrict__ seen, uint64_t* __restrict__ nxt) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    const uint64_t f = front[r];
    if (!f) return;
    GS_ENTRIES(e, r, w) {
      const int32_t c = col[e];
      if (!in_range(c, N)) continue;
      const uint64_t add = f & ~seen[c];
      if (add) atomicOr(reinterpret_cast<u64*>(&nxt[c]), (u64)add);
    }
  });
}

__global__ __launch_bounds__(TPB) void gr_commit(int64_t N, uint64_t* __restrict__ seen, uint64_t* __restrict__ front,
                                                 uint64_t* __restrict__ nxt, const uint8_t* __restrict__ mark,
                                                 int32_t level, u64* __restrict__ bin, int32_t* __restrict__ depth,
                                                 int32_t* __restrict__ changed) {
  __shared__ u64 tab[2 * kTab];
  tab_clear(tab);
  GS_NODES(v) {
    const uint64_t n = nxt[v];
    uint64_t nw = 0;
    if (n) {
      nxt[v] = 0;
      const uint64_t s = seen[v];
      nw = n & ~s;
      if (nw) seen[v] = s | nw;
    }
    if (front[v] != nw) front[v] = nw;
    tally_bits(nw, nw != 0 && (mark ? mark[v] != 0 : true), tab);
  }
  level_flush(tab, bin, depth, level, changed);
}

// One step of the greedy cover.  counts[k] = marked nodes that have bit k and no chosen bit;
// counts[kTab + k] = those of them whose word is 1 << k alone (the exclusive count while nothing is
// chosen); counts[64] = marked nodes, counts[kTab + 64] = marked nodes with a non-empty word.
__global__ __launch_bounds__(TPB) void gr_cover(const uint64_t* __restrict__ reach, const uint8_t* __restrict__ mark,
                                                int64_t N, uint64_t full, uint64_t chosen, u64* __restrict__ counts) {
  __shared__ u64 tab[2 * kTab];
  tab_clear(tab);
  int32_t nm = 0, nc = 0;
  GS_NODES(v) {
    const bool marked = mark ? mark[v] != 0 : true;
    const uint64_t r = reach[v] & full;
    nm += marked;
    nc += marked && r != 0;
    tally_bits(marked && !(r & chosen) ? r : 0, __popcll((u64)r) == 1, tab);
  }
  nm = grp_sum<64>(nm);
  nc = grp_sum<64>(nc);
  if (lane_id() == 0) {
    if (nm) atomicAdd(&tab[64], (u64)nm);
    if (nc) atomicAdd(&tab[kTab + 64], (u64)nc);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kTab; i += TPB)
    if (tab[i]) atomicAdd(&counts[i], tab[i]);
}

int64_t arrays_bytes(int64_t N) { return align256(N * 8); }

}  // namespace

extern "C" {

int64_t krca_graph_reach_ws_size(int64_t N) {
  if (N < 0) return 0;
  return kArraysOff + 2 * arrays_bytes(N);
}

int krca_graph_reach(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, const int32_t* src_host,
                     int32_t K, int32_t dir, int32_t max_hops, const uint8_t* mark, int32_t H, void* ws, uint64_t* reach,
                     int64_t* hist_host, int32_t* depth_host, int32_t* rounds_host, void* stream) {
  KRCA_CHECK_ARG(N >= 1 && N <= (int64_t)INT32_MAX - 1, "krca_graph_reach: N = %lld outside [1, 2^31 - 2]", (long long)N);
  KRCA_CHECK_ARG(pull == 0 || pull == 1, "krca_graph_reach: pull must be 0 or 1");
  KRCA_CHECK_ARG(dir == KRCA_REACH_DEPENDENTS || dir == KRCA_REACH_DEPENDENCIES, "krca_graph_reach: dir must be 0 or 1");
  KRCA_CHECK_ARG(K >= 1 && K <= KRCA_REACH_MAX_SRC, "krca_graph_reach: K = %d outside [1, 64]", K);
  KRCA_CHECK_ARG(H >= 2 && H <= 64, "krca_graph_reach: H = %d outside [2, 64]", H);
  KRCA_CHECK_ARG(row_ptr && col && src_host && ws && reach && hist_host && depth_host, "krca_graph_reach: null pointer");
  Sources src = {};
  for (int k = 0; k < K; ++k) {
    KRCA_CHECK_ARG(src_host[k] >= 0 && src_host[k] < N, "krca_graph_reach: source %d = %d outside [0, N)", k, src_host[k]);
    src.v[k] = src_host[k];
  }
  if (rounds_host) rounds_host[0] = 0;
  hipStream_t st = krca::as_stream(stream);
  char* base = reinterpret_cast<char*>(ws);
  int32_t* words = reinterpret_cast<int32_t*>(base);
  int32_t* depth = reinterpret_cast<int32_t*>(base + kDepthOff);
  u64* tally = reinterpret_cast<u64*>(base + kTallyOff);
  uint64_t* buf[2] = {reinterpret_cast<uint64_t*>(base + kArraysOff),
                      reinterpret_cast<uint64_t*>(base + kArraysOff + arrays_bytes(N))};
  const uint64_t full = K == 64 ? ~0ull : (1ull << K) - 1;
  const bool gather = pull == dir;  // bits flow along the edges when dir = 1: to the row when it lists predecessors
  Grid g;
  if (int rc = grid_of(row_ptr, N, st, &g)) return rc;
  KRCA_HIP(hipMemsetAsync(tally, 0, (size_t)H * 128 * 8, st));
  hipLaunchKernelGGL(gr_init, dim3(g.nodes), dim3(TPB), 0, st, N, reach, buf[0], buf[1]);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gr_seed, dim3(1), dim3(64), 0, st, src, K, reach, buf[0], mark, tally, depth);
  KRCA_LAUNCH_CHECK();

  // levels 1, 2, ...: a batch of rounds, each with its own "changed" word, then one read-back
  int32_t host[kBatchMax];
  const int64_t limit = N + 2, cut = max_hops > 0 ? max_hops : INT64_MAX;
  const int bmax = batch_max(N);
  int64_t done = 0;
  bool fixed = false;
  for (int B = std::min(2, bmax); !fixed && done < cut; B = std::min(2 * B, bmax)) {
    const int b = (int)std::min<int64_t>(B, std::min(limit, cut) - done);
    if (b <= 0) {
      krca::set_error("krca_graph_reach: no fixed point within N + 2 = %lld rounds", (long long)limit);
      return KRCA_ENOTCONV;
    }
    KRCA_HIP(hipMemsetAsync(words, 0, sizeof(host), st));
    for (int k = 0; k < b; ++k) {
      const int64_t level = done + k + 1;
      u64* bin = tally + std::min<int64_t>(level, H - 1) * 128;
      const int32_t lv = (int32_t)std::min<int64_t>(level, INT32_MAX);
      if (gather) {
        GS_ROWS_LAUNCH(g, st, gr_gather, row_ptr, col, N, buf[(level - 1) & 1], buf[level & 1], reach, mark, full, lv, bin,
                       depth, words + k);
      } else {
        GS_ROWS_LAUNCH(g, st, gr_scatter, row_ptr, col, N, buf[0], reach, buf[1]);
        KRCA_LAUNCH_CHECK();
        hipLaunchKernelGGL(gr_commit, dim3(g.nodes), dim3(TPB), 0, st, N, reach, buf[0], buf[1], mark, lv, bin, depth,
                           words + k);
      }
      KRCA_LAUNCH_CHECK();
    }
    KRCA_HIP(hipMemcpyAsync(host, words, sizeof(host), hipMemcpyDeviceToHost, st));
    KRCA_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < b && !fixed; ++k)
      if (!host[k]) {
        fixed = true;
        done += k + 1;
      }
    if (!fixed) done += b;
  }
  static_assert(sizeof(u64) == sizeof(int64_t), "tally words");
  std::vector<int64_t> bins((size_t)H * 128);
  int32_t dep[64];
  KRCA_HIP(hipMemcpyAsync(bins.data(), tally, (size_t)H * 128 * 8, hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipMemcpyAsync(dep, depth, sizeof(dep), hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  for (int m = 0; m < 2; ++m)
    for (int k = 0; k < K; ++k)
      for (int h = 0; h < H; ++h) hist_host[((int64_t)m * K + k) * H + h] = bins[(h * 2 + m) * 64 + k];
  for (int k = 0; k < K; ++k) depth_host[k] = dep[k];
  if (rounds_host) rounds_host[0] = (int32_t)std::min<int64_t>(done, INT32_MAX);
  return KRCA_OK;
}

int krca_graph_reach_cover(const uint64_t* reach, const uint8_t* mark, int64_t N, int32_t K, void* ws,
                           int32_t* order_host, int64_t* gain_host, int64_t* exclusive_host, int64_t* totals_host,
                           void* stream) {
  KRCA_CHECK_ARG(N >= 1 && N <= (int64_t)INT32_MAX - 1, "krca_graph_reach_cover: N = %lld outside [1, 2^31 - 2]",
                 (long long)N);
  KRCA_CHECK_ARG(K >= 1 && K <= KRCA_REACH_MAX_SRC, "krca_graph_reach_cover: K = %d outside [1, 64]", K);
  KRCA_CHECK_ARG(reach && ws && order_host && gain_host && exclusive_host && totals_host,
                 "krca_graph_reach_cover: null pointer");
  for (int k = 0; k < K; ++k) {
    order_host[k] = -1;
    gain_host[k] = 0;
    exclusive_host[k] = 0;
  }
  totals_host[0] = totals_host[1] = 0;
  hipStream_t st = krca::as_stream(stream);
  u64* counts = reinterpret_cast<u64*>(reinterpret_cast<char*>(ws) + kCountsOff);
  const uint64_t full = K == 64 ? ~0ull : (1ull << K) - 1;
  const int cap_knob = krca::tuning().graph_grid;
  const int64_t cap = cap_knob > 0 ? cap_knob : (1 << 20);
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min(cap, krca::ceil_div(N, TPB)));
  uint64_t chosen = 0;
  int64_t host[2 * kTab];
  for (int j = 0; j < K; ++j) {
    KRCA_HIP(hipMemsetAsync(counts, 0, sizeof(host), st));
    hipLaunchKernelGGL(gr_cover, dim3(grid), dim3(TPB), 0, st, reach, mark, N, full, chosen, counts);
    KRCA_LAUNCH_CHECK();
    KRCA_HIP(hipMemcpyAsync(host, counts, j == 0 ? sizeof(host) : 64 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    KRCA_HIP(hipStreamSynchronize(st));
    if (j == 0) {
      for (int k = 0; k < K; ++k) exclusive_host[k] = host[kTab + k];
      totals_host[0] = host[64];
      totals_host[1] = host[kTab + 64];
    }
    int best = 0;
    for (int k = 1; k < K; ++k)
      if (host[k] > host[best]) best = k;  // ties: the lowest k
    if (host[best] <= 0) break;
    order_host[j] = best;
    gain_host[j] = host[best];
    chosen |= 1ull << best;
  }
  return KRCA_OK;
}

}  // extern "C"
