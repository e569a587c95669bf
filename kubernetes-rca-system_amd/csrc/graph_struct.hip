// Dependency-graph structure on the device: strongly connected components, the
// longest chain of the condensation and one shortest witness cycle.  Replaces the two exponential host
// searches of TopologyAgent._analyze_service_dependencies (ref:agents/topology_agent.py:262-320:
// nx.simple_cycles, nx.all_simple_paths over every ordered pair) and tracecols.first_cycle.
//
// The graph is one CSR in either layout (pull = 0: row u lists the successors of u; pull = 1: row v
// lists the predecessors of v).  No transpose is built: every phase is a monotone fixed point over the
// edges {u -> v}, and a row can serve either end of its edges -- the end that is the row GATHERS (reads
// its entries' values, one write per row), the other end SCATTERS (a non-returning 32-bit atomicMin /
// atomicMax / atomicOr per entry that still improves, after a plain read that skips the rest).  A
// monotone fixed point is unique, so both layouts and every schedule give the same bytes.
//
// Rows run from 0 to N entries (the hub of a service mesh is a row of tens of thousands).  At 32 entries
// per row or more a wave walks one row, 64 entries per step; below, 16 lanes walk a row (four rows per
// wave) and leave a row of more than 512 entries to the whole wave (for_rows).  Waves stride over the
// rows, the grid is capped (KRCA_GRAPH_GRID).
// A column outside [0, N) is skipped before anything is indexed by it and counted once, by the first
// pass of krca_graph_scc.  A removed node costs its row one 4-byte read per round.
//
// Rounds are plain launches driven from the host: a batch of rounds, each writing its own "changed"
// word, then one read-back; the first round that changed nothing ends the loop.  No grid barrier, no
// workgroup waits on another, and every loop gives up after N + 2 rounds (KRCA_ENOTCONV).
//
// SCC: trim (a node with no live predecessor or no live successor other than itself is a component on
// its own), forward colouring (colour[v] = the largest id that reaches v among the live nodes, with one
// pointer jump colour[v] <- colour[colour[v]] per round), backward reachability from every colour's
// root (colour[r] == r) inside its colour, removal of what was reached, repeat on what is left; then
// the labels are replaced by the smallest member id, so the method does not show in the output.
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "graph_rows.h"

namespace {

constexpr int kCtlBytes = 512;  // int32 changed[32] | int32 live[32] | int64 acc[32]
constexpr int kAcc = 32;        // first accumulator, in int64 words of ctl
constexpr int32_t kInf = INT32_MAX;

// accumulators (int64 words from kAcc)
enum { A_BAD = 0, A_NCOMP, A_NCYC, A_NCYCN, A_LARGEST, A_FIRST, A_BADLAB, A_KEY };

__device__ __forceinline__ void acc_add(int64_t* ctl, int which, int64_t x) {
  atomicAdd(reinterpret_cast<unsigned long long*>(ctl + kAcc + which), (unsigned long long)x);
}
__device__ __forceinline__ int32_t* acc_i32(int64_t* ctl, int which) {
  return reinterpret_cast<int32_t*>(ctl + kAcc + which);
}

// ---- SCC ----------------------------------------------------------------------------------------

// first pass: bad columns counted, self-loops found; every node live (colour = own id), marks clear
template <int W>
__global__ __launch_bounds__(TPB) void gs_scan(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                               int64_t N, int32_t* __restrict__ colour, int32_t* __restrict__ mk,
                                               int32_t* __restrict__ comp, uint8_t* __restrict__ flags,
                                               int64_t* __restrict__ ctl) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    int bad = 0;
    bool self = false;
    GS_ENTRIES(e, r, w) {
      const int32_t c = col[e];
      if (!in_range(c, N)) ++bad;
      else if (c == r) self = true;
    }
    bad = grp_sum<w>(bad);
    self = grp_any<w>(self);
    if (GS_LEADER(w)) {
      if (bad) acc_add(ctl, A_BAD, bad);
      colour[r] = (int32_t)r;
      mk[r] = 0;
      comp[r] = -1;
      flags[r] = self ? 2 : 0;
    }
  });
}

// trim, first half: bit 0 of mk[x] = x is the row end of an edge between two live nodes, bit 1 = the
// column end (self-loops do not count)
template <int W>
__global__ __launch_bounds__(TPB) void gs_trim_mark(const int64_t* __restrict__ row_ptr,
                                                    const int32_t* __restrict__ col, int64_t N,
                                                    const int32_t* __restrict__ colour, int32_t* __restrict__ mk) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    if (colour[r] < 0) return;
    bool has = false;
    GS_ENTRIES(e, r, w) {
      const int32_t c = col[e];
      if (!in_range(c, N) || c == r || colour[c] < 0) continue;
      has = true;
      if (!(mk[c] & 2)) atomicOr(&mk[c], 2);
    }
    if (grp_any<w>(has) && GS_LEADER(w)) atomicOr(&mk[r], 1);
  });
}

// trim, second half: a live node that is not both ends becomes its own component
__global__ __launch_bounds__(TPB) void gs_trim_apply(int64_t N, int32_t* __restrict__ colour, int32_t* __restrict__ mk,
                                                     int32_t* __restrict__ comp, int32_t* __restrict__ changed,
                                                     int32_t* __restrict__ live) {
  bool ch = false, lv = false;
  GS_NODES(v) {
    if (colour[v] < 0) continue;
    const int32_t m = mk[v];
    mk[v] = 0;
    if (m != 3) {
      comp[v] = (int32_t)v;
      colour[v] = -1;
      ch = true;
    } else {
      lv = true;
    }
  }
  if (wave_any(ch) && lane_id() == 0) *changed = 1;
  if (wave_any(lv) && lane_id() == 0) *live = 1;
}

__global__ __launch_bounds__(TPB) void gs_colour_init(int64_t N, int32_t* __restrict__ colour,
                                                      int32_t* __restrict__ mk) {
  GS_NODES(v) {
    if (colour[v] < 0) continue;
    colour[v] = (int32_t)v;
    mk[v] = 0;
  }
}

// colour[v] = max(colour[v], colour[u]) over the live edges u -> v; a removed node holds -1
template <int PULL, int W>
__global__ __launch_bounds__(TPB) void gs_colour_round(const int64_t* __restrict__ row_ptr,
                                                       const int32_t* __restrict__ col, int64_t N,
                                                       int32_t* __restrict__ colour, int32_t* __restrict__ changed) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    const int32_t c0 = colour[r];
    if (c0 < 0) return;
    int32_t cr = max(c0, colour[c0]);  // colour[c0] reaches c0, which reaches r
    bool ch = false;
    if (PULL) {
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (in_range(c, N)) cr = max(cr, colour[c]);
      }
      cr = grp_max<w>(cr);
    } else {
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (!in_range(c, N)) continue;
        const int32_t cc = colour[c];
        if (cc >= 0 && cc < cr) {
          atomicMax(&colour[c], cr);
          ch = true;
        }
      }
      ch = grp_any<w>(ch);
    }
    if (GS_LEADER(w)) {
      if (cr > c0) {
        atomicMax(&colour[r], cr);
        ch = true;
      }
      if (ch) *changed = 1;
    }
  });
}

__global__ __launch_bounds__(TPB) void gs_reach_init(int64_t N, const int32_t* __restrict__ colour,
                                                     int32_t* __restrict__ mk) {
  GS_NODES(v) {
    if (colour[v] >= 0) mk[v] = colour[v] == v ? 1 : 0;
  }
}

// backward reachability inside a colour: u is reached when an edge u -> v leads to a reached v of its
// colour.  mk: 0 not reached, 1 reached, 2 reached and its row already scattered (pull = 1)
template <int PULL, int W>
__global__ __launch_bounds__(TPB) void gs_reach_round(const int64_t* __restrict__ row_ptr,
                                                      const int32_t* __restrict__ col, int64_t N,
                                                      const int32_t* __restrict__ colour, int32_t* __restrict__ mk,
                                                      int32_t* __restrict__ changed) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    const int32_t cr = colour[r];
    if (cr < 0) return;
    const int32_t mr = mk[r];
    bool hit = false;
    if (PULL) {
      if (mr != 1) return;
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (!in_range(c, N) || colour[c] != cr || mk[c] != 0) continue;
        mk[c] = 1;
        hit = true;
      }
      hit = grp_any<w>(hit);
      if (GS_LEADER(w)) {
        mk[r] = 2;
        if (hit) *changed = 1;
      }
    } else {
      if (mr != 0) return;
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (in_range(c, N) && colour[c] == cr && mk[c] != 0) hit = true;
      }
      if (grp_any<w>(hit) && GS_LEADER(w)) {
        mk[r] = 1;
        *changed = 1;
      }
    }
  });
}

__global__ __launch_bounds__(TPB) void gs_assign(int64_t N, int32_t* __restrict__ colour, int32_t* __restrict__ mk,
                                                 int32_t* __restrict__ comp) {
  GS_NODES(v) {
    const int32_t c = colour[v];
    if (c < 0) continue;
    if (mk[v] != 0) {
      comp[v] = c;
      colour[v] = -1;
    }
    mk[v] = 0;
  }
}

__global__ __launch_bounds__(TPB) void gs_label_init(int64_t N, int32_t* __restrict__ minid,
                                                     int32_t* __restrict__ size) {
  GS_NODES(v) {
    minid[v] = kInf;
    size[v] = 0;
  }
}

__global__ __launch_bounds__(TPB) void gs_label_reduce(int64_t N, const int32_t* __restrict__ comp,
                                                       int32_t* __restrict__ minid, int32_t* __restrict__ size) {
  GS_NODES(v) {
    const int32_t l = comp[v];
    if (!in_range(l, N)) continue;  // only after a failed run; keeps the index in range
    if (minid[l] > v) atomicMin(&minid[l], (int32_t)v);
    atomicAdd(&size[l], 1);
  }
}

__global__ __launch_bounds__(TPB) void gs_label_apply(int64_t N, int32_t* __restrict__ comp,
                                                      const int32_t* __restrict__ minid,
                                                      const int32_t* __restrict__ size, uint8_t* __restrict__ flags,
                                                      int64_t* __restrict__ ctl) {
  int ncomp = 0, ncyc = 0, ncycn = 0;
  int32_t largest = 0, first = kInf;
  GS_NODES(v) {
    const int32_t l = comp[v];
    if (!in_range(l, N)) continue;
    const int32_t m = minid[l], s = size[l];
    const uint8_t self = flags[v] & 2;
    const bool cyc = s >= 2 || self;
    const bool rep = m == v;
    comp[v] = m;
    flags[v] = (uint8_t)(self | (cyc ? 1 : 0) | (rep ? 4 : 0));
    ncomp += rep;
    ncyc += rep && cyc;
    ncycn += cyc;
    largest = max(largest, s);
    if (rep && cyc) first = min(first, m);
  }
  ncomp = grp_sum<64>(ncomp);
  ncyc = grp_sum<64>(ncyc);
  ncycn = grp_sum<64>(ncycn);
  largest = grp_max<64>(largest);
  first = grp_min<64>(first);
  if (lane_id() == 0) {
    if (ncomp) acc_add(ctl, A_NCOMP, ncomp);
    if (ncyc) acc_add(ctl, A_NCYC, ncyc);
    if (ncycn) acc_add(ctl, A_NCYCN, ncycn);
    if (largest) atomicMax(acc_i32(ctl, A_LARGEST), largest);
    if (first != kInf) atomicMin(acc_i32(ctl, A_FIRST), first);
  }
}

__global__ void gs_acc_init(int64_t* __restrict__ ctl) {
  if (threadIdx.x < 16) ctl[kAcc + threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) *acc_i32(ctl, A_FIRST) = kInf;
}

// ---- chain over the condensation ----------------------------------------------------------------

__global__ __launch_bounds__(TPB) void gs_chain_init(int64_t N, const int32_t* __restrict__ comp,
                                                     int32_t* __restrict__ ddn, int32_t* __restrict__ dup,
                                                     int32_t* __restrict__ nx, int64_t* __restrict__ ctl) {
  bool bad = false;
  GS_NODES(v) {
    ddn[v] = 1;
    dup[v] = 1;
    nx[v] = kInf;
    if (!in_range(comp[v], N)) bad = true;
  }
  if (wave_any(bad) && lane_id() == 0) *acc_i32(ctl, A_BADLAB) = 1;
}

// depth over the edges between different components, kept at the component's label.  G is the depth
// the row end gathers (pull = 0: depth_dn of the caller row; pull = 1: depth_up of the callee row),
// S the one it scatters to its entries' components.  A depth above N means comp is no component
// labelling (the condensation has a cycle): flagged, never stored.
template <int W>
__global__ __launch_bounds__(TPB) void gs_chain_round(const int64_t* __restrict__ row_ptr,
                                                      const int32_t* __restrict__ col, int64_t N,
                                                      const int32_t* __restrict__ comp, int32_t* __restrict__ G,
                                                      int32_t* __restrict__ S, int32_t* __restrict__ changed,
                                                      int64_t* __restrict__ ctl) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    const int32_t lr = comp[r];
    if (!in_range(lr, N)) return;
    const int32_t g0 = G[lr], s1 = S[lr] + 1;
    int32_t g = g0;
    bool ch = false, over = false;
    GS_ENTRIES(e, r, w) {
      const int32_t c = col[e];
      if (!in_range(c, N)) continue;
      const int32_t lc = comp[c];
      if (!in_range(lc, N) || lc == lr) continue;
      g = max(g, G[lc] + 1);
      if (S[lc] < s1) {
        if (s1 > N) over = true;
        else {
          atomicMax(&S[lc], s1);
          ch = true;
        }
      }
    }
    g = grp_max<w>(g);
    ch = grp_any<w>(ch);
    over = grp_any<w>(over);
    if (GS_LEADER(w)) {
      if (g > g0) {
        if (g > N) over = true;
        else {
          atomicMax(&G[lr], g);
          ch = true;
        }
      }
      if (ch) *changed = 1;
      if (over) *acc_i32(ctl, A_BADLAB) = 1;
    }
  });
}

// nx[label of u] = the smallest label of a forward neighbour component one level shallower
template <int PULL, int W>
__global__ __launch_bounds__(TPB) void gs_chain_next(const int64_t* __restrict__ row_ptr,
                                                     const int32_t* __restrict__ col, int64_t N,
                                                     const int32_t* __restrict__ comp, const int32_t* __restrict__ ddn,
                                                     int32_t* __restrict__ nx) {
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    const int32_t lr = comp[r];
    if (!in_range(lr, N)) return;
    const int32_t dr = ddn[lr];
    int32_t best = kInf;
    GS_ENTRIES(e, r, w) {
      const int32_t c = col[e];
      if (!in_range(c, N)) continue;
      const int32_t lc = comp[c];
      if (!in_range(lc, N) || lc == lr) continue;
      if (PULL) {  // edge c -> r
        if (dr == ddn[lc] - 1 && nx[lc] > lr) atomicMin(&nx[lc], lr);
      } else if (ddn[lc] == dr - 1) {
        best = min(best, lc);
      }
    }
    if (!PULL) {
      best = grp_min<w>(best);
      if (GS_LEADER(w) && best != kInf && nx[lr] > best) atomicMin(&nx[lr], best);
    }
  });
}

__global__ __launch_bounds__(TPB) void gs_chain_out(int64_t N, const int32_t* __restrict__ comp,
                                                    const int32_t* __restrict__ ddn, const int32_t* __restrict__ dup,
                                                    const int32_t* __restrict__ nx, int32_t* __restrict__ depth_dn,
                                                    int32_t* __restrict__ depth_up, int32_t* __restrict__ next,
                                                    int64_t* __restrict__ ctl) {
  uint64_t key = 0;
  GS_NODES(v) {
    const int32_t l = comp[v];
    if (!in_range(l, N)) {
      depth_dn[v] = 0;
      depth_up[v] = 0;
      next[v] = -1;
      continue;
    }
    const int32_t d = ddn[l], n = nx[l];
    depth_dn[v] = d;
    depth_up[v] = dup[l];
    next[v] = n == kInf ? -1 : n;
    const uint64_t k = ((uint64_t)(uint32_t)d << 32) | (uint32_t)(INT32_MAX - l);
    key = k > key ? k : key;
  }
  key = ~grp_min_u64<64>(~key);
  if (lane_id() == 0 && key) atomicMax(reinterpret_cast<unsigned long long*>(ctl + kAcc + A_KEY), (unsigned long long)key);
}

// ---- witness cycle ---------------------------------------------------------------------------------

__global__ __launch_bounds__(TPB) void gs_cycle_init(int64_t N, int64_t root, int32_t* __restrict__ dist,
                                                     uint64_t* __restrict__ key) {
  GS_NODES(v) {
    dist[v] = v == root ? 0 : kInf;
    key[v] = ~0ull;
  }
}

// dist[u] = min(dist[u], dist[v] + 1) over the edges u -> v inside root's component: at the fixed
// point, the BFS distance from u to root
template <int PULL, int W>
__global__ __launch_bounds__(TPB) void gs_cycle_round(const int64_t* __restrict__ row_ptr,
                                                      const int32_t* __restrict__ col, int64_t N,
                                                      const int32_t* __restrict__ comp, int64_t root,
                                                      int32_t* __restrict__ dist, int32_t* __restrict__ changed) {
  const int32_t C = comp[root];
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    if (comp[r] != C) return;
    const int32_t d0 = dist[r];
    bool ch = false;
    if (PULL) {  // edges c -> r
      if (d0 == kInf) return;
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (!in_range(c, N) || comp[c] != C) continue;
        if (dist[c] > d0 + 1) {
          atomicMin(&dist[c], d0 + 1);
          ch = true;
        }
      }
      if (grp_any<w>(ch) && GS_LEADER(w)) *changed = 1;
    } else {  // edges r -> c
      int32_t m = kInf;
      GS_ENTRIES(e, r, w) {
        const int32_t c = col[e];
        if (in_range(c, N) && comp[c] == C) m = min(m, dist[c]);
      }
      m = grp_min<w>(m);
      if (GS_LEADER(w) && m != kInf && m + 1 < d0) {
        atomicMin(&dist[r], m + 1);
        *changed = 1;
      }
    }
  });
}

// key[u] = min over the edges u -> w inside the component of (dist[w] << 32) | w
template <int PULL, int W>
__global__ __launch_bounds__(TPB) void gs_cycle_key(const int64_t* __restrict__ row_ptr,
                                                    const int32_t* __restrict__ col, int64_t N,
                                                    const int32_t* __restrict__ comp, int64_t root,
                                                    const int32_t* __restrict__ dist, uint64_t* __restrict__ key) {
  const int32_t C = comp[root];
  for_rows<W>(row_ptr, N, [&](auto width, int64_t r) {
    constexpr int w = decltype(width)::value;
    if (comp[r] != C) return;
    const int32_t dr = dist[r];
    uint64_t best = ~0ull;
    GS_ENTRIES(e, r, w) {
      const int32_t c = col[e];
      if (!in_range(c, N) || comp[c] != C) continue;
      if (PULL) {  // edge c -> r: r is a successor of c
        if (dr == kInf) continue;
        const uint64_t k = ((uint64_t)(uint32_t)dr << 32) | (uint32_t)r;
        if (key[c] > k) atomicMin(reinterpret_cast<unsigned long long*>(&key[c]), (unsigned long long)k);
      } else {
        const int32_t dc = dist[c];
        if (dc == kInf) continue;
        const uint64_t k = ((uint64_t)(uint32_t)dc << 32) | (uint32_t)c;
        best = k < best ? k : best;
      }
    }
    if (!PULL) {
      best = grp_min_u64<w>(best);
      if (GS_LEADER(w)) key[r] = best;
    }
  });
}

__global__ __launch_bounds__(TPB) void gs_cycle_out(int64_t N, const int32_t* __restrict__ comp, int64_t root,
                                                    const uint64_t* __restrict__ key, int32_t* __restrict__ hop) {
  const int32_t C = comp[root];
  GS_NODES(v) {
    const uint64_t k = key[v];
    hop[v] = (comp[v] == C && k != ~0ull) ? (int32_t)(uint32_t)k : -1;
  }
}

// ---- host side ----------------------------------------------------------------------------------

// Runs launch(changed + k, live + k), k = 0, 1, ..., in batches until a round leaves its changed word 0; at most
// N + 2 rounds.  *rounds += the rounds up to and including that one; *live_out = its live word.
template <class Launch>
int run_rounds(hipStream_t st, int64_t* ctl, int64_t N, const char* what, int64_t* rounds, int32_t* live_out,
               Launch launch) {
  int32_t* words = reinterpret_cast<int32_t*>(ctl);
  int32_t host[2 * kBatchMax];
  const int64_t limit = N + 2;
  const int bmax = batch_max(N);
  int64_t done = 0;
  for (int B = std::min(2, bmax);; B = std::min(2 * B, bmax)) {
    const int b = (int)std::min<int64_t>(B, limit - done);
    if (b <= 0) {
      krca::set_error("%s: no fixed point within N + 2 = %lld rounds", what, (long long)limit);
      return KRCA_ENOTCONV;
    }
    KRCA_HIP(hipMemsetAsync(words, 0, sizeof(host), st));
    for (int k = 0; k < b; ++k) {
      launch(words + k, words + kBatchMax + k);
      KRCA_LAUNCH_CHECK();
    }
    KRCA_HIP(hipMemcpyAsync(host, words, sizeof(host), hipMemcpyDeviceToHost, st));
    KRCA_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < b; ++k)
      if (!host[k]) {
        *rounds += done + k + 1;
        if (live_out) *live_out = host[kBatchMax + k];
        return KRCA_OK;
      }
    done += b;
  }
}

int check_graph_args(const char* what, int64_t N, int32_t pull) {
  KRCA_CHECK_ARG(N >= 0 && N <= (int64_t)INT32_MAX - 1, "%s: N = %lld outside [0, 2^31 - 2]", what, (long long)N);
  KRCA_CHECK_ARG(pull == 0 || pull == 1, "%s: pull must be 0 or 1", what);
  return KRCA_OK;
}

}  // namespace

extern "C" {

int64_t krca_graph_scc_ws_size(int64_t N) {
  if (N < 0) return 0;
  return kCtlBytes + 2 * align256(N * 4);
}
int64_t krca_graph_chain_ws_size(int64_t N) {
  if (N < 0) return 0;
  return kCtlBytes + 3 * align256(N * 4);
}
int64_t krca_graph_cycle_ws_size(int64_t N) {
  if (N < 0) return 0;
  return kCtlBytes + align256(N * 8) + align256(N * 4);
}

int krca_graph_scc(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, void* ws, int32_t* comp,
                   uint8_t* flags, int64_t* stats_host, int32_t* rounds_host, void* stream) {
  if (int rc = check_graph_args("krca_graph_scc", N, pull)) return rc;
  KRCA_CHECK_ARG(stats_host, "krca_graph_scc: null stats_host");
  for (int i = 0; i < 6; ++i) stats_host[i] = i == 4 ? -1 : 0;
  if (rounds_host)
    for (int i = 0; i < 4; ++i) rounds_host[i] = 0;
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(row_ptr && col && ws && comp && flags, "krca_graph_scc: null pointer");
  hipStream_t st = krca::as_stream(stream);
  int64_t* ctl = reinterpret_cast<int64_t*>(ws);
  int32_t* colour = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + kCtlBytes);
  int32_t* mk = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(colour) + align256(N * 4));
  Grid g;
  if (int rc = grid_of(row_ptr, N, st, &g)) return rc;
  hipLaunchKernelGGL(gs_acc_init, dim3(1), dim3(64), 0, st, ctl);
  KRCA_LAUNCH_CHECK();
  GS_ROWS_LAUNCH(g, st, gs_scan, row_ptr, col, N, colour, mk, comp, flags, ctl);
  KRCA_LAUNCH_CHECK();
  int64_t passes = 0, r_trim = 0, r_colour = 0, r_reach = 0;
  for (;; ++passes) {
    if (passes > N + 2) {
      krca::set_error("krca_graph_scc: nodes left after N + 2 passes");
      return KRCA_ENOTCONV;
    }
    int32_t live = 0;
    if (int rc = run_rounds(st, ctl, N, "krca_graph_scc (trim)", &r_trim, &live, [&](int32_t* ch, int32_t* lv) {
          GS_ROWS_LAUNCH(g, st, gs_trim_mark, row_ptr, col, N, colour, mk);
          hipLaunchKernelGGL(gs_trim_apply, dim3(g.nodes), dim3(TPB), 0, st, N, colour, mk, comp, ch, lv);
        }))
      return rc;
    if (!live) break;
    hipLaunchKernelGGL(gs_colour_init, dim3(g.nodes), dim3(TPB), 0, st, N, colour, mk);
    KRCA_LAUNCH_CHECK();
    if (int rc = run_rounds(st, ctl, N, "krca_graph_scc (colour)", &r_colour, nullptr, [&](int32_t* ch, int32_t*) {
          GS_ROWS_LAUNCH_PULL(g, st, pull, gs_colour_round, row_ptr, col, N, colour, ch);
        }))
      return rc;
    hipLaunchKernelGGL(gs_reach_init, dim3(g.nodes), dim3(TPB), 0, st, N, colour, mk);
    KRCA_LAUNCH_CHECK();
    if (int rc = run_rounds(st, ctl, N, "krca_graph_scc (reach)", &r_reach, nullptr, [&](int32_t* ch, int32_t*) {
          GS_ROWS_LAUNCH_PULL(g, st, pull, gs_reach_round, row_ptr, col, N, colour, mk, ch);
        }))
      return rc;
    hipLaunchKernelGGL(gs_assign, dim3(g.nodes), dim3(TPB), 0, st, N, colour, mk, comp);
    KRCA_LAUNCH_CHECK();
  }
  // canonical labels: the smallest member id (colour / mk are free now)
  hipLaunchKernelGGL(gs_label_init, dim3(g.nodes), dim3(TPB), 0, st, N, colour, mk);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gs_label_reduce, dim3(g.nodes), dim3(TPB), 0, st, N, comp, colour, mk);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gs_label_apply, dim3(g.nodes), dim3(TPB), 0, st, N, comp, colour, mk, flags, ctl);
  KRCA_LAUNCH_CHECK();
  int64_t acc[8];
  KRCA_HIP(hipMemcpyAsync(acc, ctl + kAcc, sizeof(acc), hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  const int32_t first = (int32_t)(uint32_t)(uint64_t)acc[A_FIRST];
  stats_host[0] = acc[A_NCOMP];
  stats_host[1] = acc[A_NCYC];
  stats_host[2] = acc[A_NCYCN];
  stats_host[3] = (int32_t)(uint32_t)(uint64_t)acc[A_LARGEST];
  stats_host[4] = first == kInf ? -1 : first;
  stats_host[5] = acc[A_BAD];
  if (rounds_host) {
    const int64_t r[4] = {passes, r_trim, r_colour, r_reach};
    for (int i = 0; i < 4; ++i) rounds_host[i] = (int32_t)std::min<int64_t>(r[i], INT32_MAX);
  }
  return KRCA_OK;
}

int krca_graph_chain(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, const int32_t* comp, void* ws,
                     int32_t* depth_dn, int32_t* depth_up, int32_t* next, int64_t* stats_host, int32_t* rounds_host,
                     void* stream) {
  if (int rc = check_graph_args("krca_graph_chain", N, pull)) return rc;
  KRCA_CHECK_ARG(stats_host, "krca_graph_chain: null stats_host");
  stats_host[0] = 0;
  stats_host[1] = -1;
  if (rounds_host) rounds_host[0] = 0;
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(row_ptr && col && comp && ws && depth_dn && depth_up && next, "krca_graph_chain: null pointer");
  hipStream_t st = krca::as_stream(stream);
  int64_t* ctl = reinterpret_cast<int64_t*>(ws);
  int32_t* ddn = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + kCtlBytes);
  int32_t* dup = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ddn) + align256(N * 4));
  int32_t* nx = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(dup) + align256(N * 4));
  Grid g;
  if (int rc = grid_of(row_ptr, N, st, &g)) return rc;
  hipLaunchKernelGGL(gs_acc_init, dim3(1), dim3(64), 0, st, ctl);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gs_chain_init, dim3(g.nodes), dim3(TPB), 0, st, N, comp, ddn, dup, nx, ctl);
  KRCA_LAUNCH_CHECK();
  int64_t rounds = 0;
  int32_t* G = pull ? dup : ddn;
  int32_t* S = pull ? ddn : dup;
  if (int rc = run_rounds(st, ctl, N, "krca_graph_chain", &rounds, nullptr, [&](int32_t* ch, int32_t*) {
        GS_ROWS_LAUNCH(g, st, gs_chain_round, row_ptr, col, N, comp, G, S, ch, ctl);
      }))
    return rc;
  GS_ROWS_LAUNCH_PULL(g, st, pull, gs_chain_next, row_ptr, col, N, comp, ddn, nx);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gs_chain_out, dim3(g.nodes), dim3(TPB), 0, st, N, comp, ddn, dup, nx, depth_dn, depth_up, next, ctl);
  KRCA_LAUNCH_CHECK();
  int64_t acc[8];
  KRCA_HIP(hipMemcpyAsync(acc, ctl + kAcc, sizeof(acc), hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  if (rounds_host) rounds_host[0] = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
  KRCA_CHECK_ARG((int32_t)acc[A_BADLAB] == 0,
                 "krca_graph_chain: comp is not a component labelling (a label outside [0, N) or a cycle between labels)");
  const uint64_t key = (uint64_t)acc[A_KEY];
  stats_host[0] = (int64_t)(key >> 32);
  stats_host[1] = (int64_t)INT32_MAX - (int64_t)(uint32_t)key;
  return KRCA_OK;
}

int krca_graph_cycle(const int64_t* row_ptr, const int32_t* col, int64_t N, int32_t pull, const int32_t* comp,
                     int64_t root, void* ws, int32_t* hop, int32_t* rounds_host, void* stream) {
  if (int rc = check_graph_args("krca_graph_cycle", N, pull)) return rc;
  if (rounds_host) rounds_host[0] = 0;
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(root >= 0 && root < N, "krca_graph_cycle: root %lld outside [0, N)", (long long)root);
  KRCA_CHECK_ARG(row_ptr && col && comp && ws && hop, "krca_graph_cycle: null pointer");
  hipStream_t st = krca::as_stream(stream);
  int64_t* ctl = reinterpret_cast<int64_t*>(ws);
  uint64_t* key = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(ws) + kCtlBytes);
  int32_t* dist = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(key) + align256(N * 8));
  Grid g;
  if (int rc = grid_of(row_ptr, N, st, &g)) return rc;
  hipLaunchKernelGGL(gs_cycle_init, dim3(g.nodes), dim3(TPB), 0, st, N, root, dist, key);
  KRCA_LAUNCH_CHECK();
  int64_t rounds = 0;
  if (int rc = run_rounds(st, ctl, N, "krca_graph_cycle", &rounds, nullptr, [&](int32_t* ch, int32_t*) {
        GS_ROWS_LAUNCH_PULL(g, st, pull, gs_cycle_round, row_ptr, col, N, comp, root, dist, ch);
      }))
    return rc;
  GS_ROWS_LAUNCH_PULL(g, st, pull, gs_cycle_key, row_ptr, col, N, comp, root, dist, key);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(gs_cycle_out, dim3(g.nodes), dim3(TPB), 0, st, N, comp, root, key, hop);
  KRCA_LAUNCH_CHECK();
  KRCA_HIP(hipStreamSynchronize(st));
  if (rounds_host) rounds_host[0] = (int32_t)std::min<int64_t>(rounds, INT32_MAX);
  return KRCA_OK;
}

}  // extern "C"
