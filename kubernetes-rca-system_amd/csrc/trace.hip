// krca_trace_* — span analytics behind TracesAgent: parent links, call edges, keyed latency histograms.
//
// The reference's TracesAgent emits canned findings ("In a real implementation, you would actually
// fetch and analyze real trace data", ref:agents/traces_agent.py:209-381); its data-access layer fixes
// the schemas a trace backend serves (ref:utils/mock_k8s_client.py:1146-1311: latency percentiles per
// service, error rate per service, the call graph, slow operations).  Here they are computed from
// columnar spans (krca/tracecols.py), one entry per span: svc, parent (index in the table), dur_us, err.
//
//   link       child -> parent scatter (64-bit duration sums, error bits), then per span: caller service,
//              self time, origin / propagated error flags.
//   edges      the distinct (caller, callee) keys through a device hash table (open addressing, 64-bit
//              CAS); the E keys are ordered on the host inside the call (E << N), every per-span step
//              stays on the device.
//   stats      keyed log-linear histogram (32 sub-buckets per octave, 896 buckets) + a 64-byte record
//              per slot.  Small S: LDS-private tables per workgroup, flushed once.  Large S: global
//              integer atomics for the histogram; a wave first folds lanes that share a slot (and,
//              inside such a group, a bucket), a bounded number of rounds, and the records go through
//              a per-workgroup LDS cache claimed first come, so a popular slot's record (two adds on
//              one address per span otherwise) reaches memory once per workgroup.
//   quantiles  nearest rank over the histogram, one wave per slot.
// Every reduction is an integer add / max / or: results do not depend on arrival order.
#include "krca_common.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace {

constexpr int TPB = 256;
constexpr int NB = 896;                            // 64 + 26 octaves x 32
constexpr int REC = 8;                             // int64 words per slot record
constexpr int SLOT_BYTES = NB * 4 + REC * 8;       // LDS bytes per slot of the small-S path
constexpr int LDS_BUDGET = 64 * 1024;              // per workgroup: two workgroups share a CU's 160 KiB
constexpr int LDS_MAX_SLOTS = LDS_BUDGET / SLOT_BYTES;  // 17
constexpr int TPB_LDS = 512;
constexpr int PEEL_ROUNDS = 6;                     // slot groups (and buckets per group) folded per wave
constexpr int MAXQ = 16;
constexpr int PER_LANE = NB / 64;                  // 14 buckets per lane in the quantile scan
constexpr int64_t HASH_MIN = 1024;

__host__ __device__ inline int bucket_of(uint32_t d) {
  if (d < 64) return (int)d;
  const int e = 31 - __builtin_clz(d);
  return 64 + (e - 6) * 32 + (int)(d >> (e - 5)) - 32;
}
__host__ __device__ inline uint32_t bucket_lo(int b) {
  if (b < 64) return (uint32_t)b;
  const int e = 6 + ((b - 64) >> 5), m = 32 + ((b - 64) & 31);
  return (uint32_t)m << (e - 5);
}
__host__ __device__ inline uint32_t bucket_hi(int b) {
  if (b < 64) return (uint32_t)b;
  const int e = 6 + ((b - 64) >> 5), m = 32 + ((b - 64) & 31);
  return (uint32_t)(((uint64_t)(m + 1) << (e - 5)) - 1);
}

unsigned grid_for(int64_t n, int tpb = TPB, int64_t cap = 8192) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(krca::ceil_div(n, tpb), cap));
}

__global__ __launch_bounds__(TPB) void fill_u64(uint64_t* __restrict__ p, int64_t n, uint64_t v) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x; w < n; w += stride) p[w] = v;
}
__global__ __launch_bounds__(TPB) void fill_i32(int32_t* __restrict__ p, int64_t n, int32_t v) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x; w < n; w += stride) p[w] = v;
}

// ---- link -------------------------------------------------------------------------------------
// ws: 8 x u64 counters (word 0 = bad spans) | child_sum u64[N] | child_err u32[N]
constexpr int64_t LINK_HDR = 8;
inline int64_t link_ws_words(int64_t N) { return LINK_HDR + N + (N + 1) / 2; }

__device__ inline bool svc_ok(int32_t s, int32_t S) { return (uint32_t)s < (uint32_t)S; }

__global__ __launch_bounds__(TPB) void link_scatter(const int32_t* __restrict__ svc, const int32_t* __restrict__ parent,
                                                    const uint32_t* __restrict__ dur, const uint8_t* __restrict__ err,
                                                    int64_t N, int32_t S, unsigned long long* __restrict__ counters,
                                                    unsigned long long* __restrict__ child_sum,
                                                    uint32_t* __restrict__ child_err) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  unsigned long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    if (!svc_ok(svc[i], S)) {
      ++bad;
      continue;
    }
    const int64_t p = parent[i];
    if (p < 0 || p >= N || p == i) continue;
    if (!svc_ok(svc[p], S)) continue;
    atomicAdd(child_sum + p, (unsigned long long)dur[i]);
    if (err[i]) atomicOr(child_err + p, 1u);
  }
  if (bad) atomicAdd(counters, bad);
}

__global__ __launch_bounds__(TPB) void link_final(const int32_t* __restrict__ svc, const int32_t* __restrict__ parent,
                                                  const uint32_t* __restrict__ dur, const uint8_t* __restrict__ err,
                                                  int64_t N, int32_t S, const unsigned long long* __restrict__ child_sum,
                                                  const uint32_t* __restrict__ child_err, int32_t* __restrict__ caller_svc,
                                                  uint32_t* __restrict__ self_us, uint8_t* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    const int32_t s = svc[i];
    if (!svc_ok(s, S)) {
      caller_svc[i] = -1;
      self_us[i] = 0;
      flags[i] = 0;
      continue;
    }
    const int64_t p = parent[i];
    int32_t caller = -1;
    bool parent_err = false;
    if (p >= 0 && p < N && p != i) {
      const int32_t ps = svc[p];
      if (svc_ok(ps, S)) {
        if (ps != s) caller = ps;
        parent_err = err[p] != 0;
      }
    }
    const unsigned long long cs = child_sum[i];
    const uint32_t d = dur[i];
    const bool e = err[i] != 0;
    uint8_t f = e ? 1 : 0;
    if (e && child_err[i] == 0) f |= 2;
    if (e && parent_err && caller >= 0) f |= 4;
    caller_svc[i] = caller;
    self_us[i] = (unsigned long long)d > cs ? (uint32_t)(d - cs) : 0u;
    flags[i] = f;
  }
}

// ---- edges ------------------------------------------------------------------------------------
// ws: 8 x u64 counters (0 = distinct keys inserted, 1 = compaction cursor) | key int64[T] | rank int32[T]
inline int64_t hash_slots(int64_t cap) {
  int64_t t = HASH_MIN;
  while (t < 2 * cap) t <<= 1;
  return t;
}
__device__ inline int64_t hash_of(int64_t key, int64_t mask) {
  return (int64_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> 20) & mask;
}
__device__ inline int64_t edge_key_of(const int32_t* caller_svc, const int32_t* svc, int64_t i, int32_t S) {
  const int32_t c = caller_svc[i], s = svc[i];
  return (svc_ok(c, S) && svc_ok(s, S)) ? (int64_t)c * S + s : -1;
}

__global__ __launch_bounds__(TPB) void edge_insert(const int32_t* __restrict__ caller_svc, const int32_t* __restrict__ svc,
                                                   int64_t N, int32_t S, int64_t cap, int64_t T,
                                                   unsigned long long* counters, long long* table) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  const int64_t mask = T - 1;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    const int64_t key = edge_key_of(caller_svc, svc, i, S);
    if (key < 0) continue;
    // past cap the caller retries with a larger table: stop filling this one
    if ((int64_t)__hip_atomic_load(counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap) continue;
    int64_t h = hash_of(key, mask);
    for (int64_t probe = 0; probe < T; ++probe) {  // bounded: a full table ends the walk
      long long cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == -1) cur = atomicCAS((unsigned long long*)(table + h), (unsigned long long)-1LL, (unsigned long long)key);
      if (cur == -1) {  // this thread claimed the slot
        atomicAdd(counters, 1ull);
        break;
      }
      if (cur == key) break;
      h = (h + 1) & mask;
    }
  }
}

__global__ __launch_bounds__(TPB) void edge_compact(const long long* __restrict__ table, int64_t T, int64_t cap,
                                                    unsigned long long* counters, int64_t* __restrict__ edge_key) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < T; j += stride) {
    const long long k = table[j];
    if (k == -1) continue;
    const unsigned long long pos = atomicAdd(counters + 1, 1ull);
    if ((int64_t)pos < cap) edge_key[pos] = k;
  }
}

__global__ __launch_bounds__(TPB) void edge_rank(const long long* __restrict__ table, int64_t T,
                                                 const int64_t* __restrict__ edge_key, int64_t E,
                                                 int32_t* __restrict__ rank) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x; j < T; j += stride) {
    const long long k = table[j];
    if (k == -1) continue;
    int64_t lo = 0, hi = E;  // first position with edge_key >= k
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (edge_key[mid] < k) lo = mid + 1; else hi = mid;
    }
    rank[j] = (lo < E && edge_key[lo] == k) ? (int32_t)lo : -1;
  }
}

__global__ __launch_bounds__(TPB) void edge_lookup(const int32_t* __restrict__ caller_svc, const int32_t* __restrict__ svc,
                                                   int64_t N, int32_t S, int64_t T, const long long* __restrict__ table,
                                                   const int32_t* __restrict__ rank, int32_t* __restrict__ edge_slot) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  const int64_t mask = T - 1;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    const int64_t key = edge_key_of(caller_svc, svc, i, S);
    int32_t out = -1;
    if (key >= 0) {
      int64_t h = hash_of(key, mask);
      for (int64_t probe = 0; probe < T; ++probe) {
        const long long cur = table[h];
        if (cur == key) {
          out = rank[h];
          break;
        }
        if (cur == -1) break;
        h = (h + 1) & mask;
      }
    }
    edge_slot[i] = out;
  }
}

// ---- stats ------------------------------------------------------------------------------------
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
  return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

__device__ inline void rec_add(int64_t* rp, unsigned long long n, unsigned long long sum, uint32_t mx,
                               unsigned long long n0, unsigned long long n1, unsigned long long n2) {
  atomicAdd((unsigned long long*)rp, n);
  atomicAdd((unsigned long long*)(rp + 1), sum);
  // the maximum only grows: a stale read is a smaller one, so skipping on it is safe
  if (rp[2] < (int64_t)mx) atomicMax((long long*)(rp + 2), (long long)mx);
  if (n0) atomicAdd((unsigned long long*)(rp + 3), n0);
  if (n1) atomicAdd((unsigned long long*)(rp + 4), n1);
  if (n2) atomicAdd((unsigned long long*)(rp + 5), n2);
}

// Record cache of the large-S path: RC_SLOTS entries per workgroup in LDS, claimed first come (two
// probes), so the records of the slots a workgroup meets early -- the popular ones -- are summed on
// chip and reach memory once per workgroup; a slot that finds no entry goes to memory directly.
constexpr int RC_SLOTS = 512;
constexpr int RC_WORDS = 6;

__device__ inline void rec_put(int32_t* ltag, unsigned long long* lrec, int64_t* rec, int32_t s, unsigned long long n,
                               unsigned long long sum, uint32_t mx, unsigned long long n0, unsigned long long n1,
                               unsigned long long n2) {
  const int idx = (int)(((uint32_t)s * 2654435761u) >> 23);  // 9 bits
  int hit = -1;
  for (int p = 0; p < 2 && hit < 0; ++p) {
    const int j = (idx + p) & (RC_SLOTS - 1);
    int32_t t = __hip_atomic_load(ltag + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t == -1) {
      t = atomicCAS(ltag + j, -1, s);
      if (t == -1) t = s;  // claimed
    }
    if (t == s) hit = j;
  }
  if (hit < 0) {
    rec_add(rec + (int64_t)s * REC, n, sum, mx, n0, n1, n2);
    return;
  }
  unsigned long long* r = lrec + hit * RC_WORDS;
  atomicAdd(r, n);
  atomicAdd(r + 1, sum);
  atomicMax(r + 2, (unsigned long long)mx);
  if (n0) atomicAdd(r + 3, n0);
  if (n1) atomicAdd(r + 4, n1);
  if (n2) atomicAdd(r + 5, n2);
}

// small S: the whole [S][NB] histogram and the records live in LDS, flushed once per workgroup
__global__ __launch_bounds__(TPB_LDS) void stats_lds(const int32_t* __restrict__ slot, const uint32_t* __restrict__ val,
                                                     const uint8_t* __restrict__ flags, int64_t N, int32_t S,
                                                     int64_t* rec, uint32_t* hist) {
  extern __shared__ unsigned long long lds[];
  unsigned long long* lrec = lds;                 // [S][REC]
  uint32_t* lh = (uint32_t*)(lds + (int64_t)S * REC);  // [S][NB]
  const int nrec = S * REC, nh = S * NB;
  for (int w = threadIdx.x; w < nrec; w += TPB_LDS) lrec[w] = 0;
  for (int w = threadIdx.x; w < nh; w += TPB_LDS) lh[w] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * TPB_LDS;
  for (int64_t i = (int64_t)blockIdx.x * TPB_LDS + threadIdx.x; i < N; i += stride) {
    const int32_t s = __builtin_nontemporal_load(slot + i);
    if (!svc_ok(s, S)) continue;
    const uint32_t v = __builtin_nontemporal_load(val + i);
    const uint8_t f = __builtin_nontemporal_load(flags + i);
    atomicAdd(lh + s * NB + bucket_of(v), 1u);
    unsigned long long* rp = lrec + s * REC;
    atomicAdd(rp, 1ull);
    atomicAdd(rp + 1, (unsigned long long)v);
    atomicMax(rp + 2, (unsigned long long)v);
    if (f & 1) atomicAdd(rp + 3, 1ull);
    if (f & 2) atomicAdd(rp + 4, 1ull);
    if (f & 4) atomicAdd(rp + 5, 1ull);
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nh; w += TPB_LDS) {
    const uint32_t c = lh[w];
    if (c) atomicAdd(hist + w, c);
  }
  for (int w = threadIdx.x; w < nrec; w += TPB_LDS) {
    const unsigned long long x = lrec[w];
    if (!x) continue;
    if ((w & (REC - 1)) == 2)
      atomicMax((long long*)(rec + w), (long long)x);
    else
      atomicAdd((unsigned long long*)(rec + w), x);
  }
}

// large S: global atomics.  PEEL: up to PEEL_ROUNDS slot groups of two or more lanes are folded (one
// lane issues the record's update for the group; inside the group up to PEEL_ROUNDS buckets shared by
// two or more lanes are folded too); every other lane issues its own; record updates go through the
// workgroup's LDS record cache (rec_put).  Each lane's contribution is issued exactly once either way.
template <bool PEEL>
__global__ __launch_bounds__(TPB) void stats_global(const int32_t* __restrict__ slot, const uint32_t* __restrict__ val,
                                                    const uint8_t* __restrict__ flags, int64_t N, int32_t S,
                                                    int64_t* rec, uint32_t* hist) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * TPB;
  __shared__ int32_t ltag[PEEL ? RC_SLOTS : 1];
  __shared__ unsigned long long lrec[PEEL ? RC_SLOTS * RC_WORDS : 1];
  if (PEEL) {
    for (int w = threadIdx.x; w < RC_SLOTS; w += TPB) ltag[w] = -1;
    for (int w = threadIdx.x; w < RC_SLOTS * RC_WORDS; w += TPB) lrec[w] = 0;
    __syncthreads();
  }
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < N; base += stride) {  // block-uniform trip count
    const int64_t i = base + threadIdx.x;
    int32_t s = -1;
    uint32_t v = 0;
    uint8_t f = 0;
    if (i < N) {
      s = __builtin_nontemporal_load(slot + i);
      v = __builtin_nontemporal_load(val + i);
      f = __builtin_nontemporal_load(flags + i);
      if (!svc_ok(s, S)) s = -1;
    }
    const int b = bucket_of(v);
    bool rec_todo = s >= 0, hist_todo = s >= 0;
    if (PEEL) {
      // leaders come from the lanes that see their own slot in a lane 1, 2, 4 ... 32 further on (rotating):
      // the lanes of a hot slot almost surely see one another, and a wave without repeats runs no round
      bool dup = false;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) dup |= (__shfl(s, (lane + o) & 63, 64) == s);
      uint64_t cand = __ballot(dup && s >= 0);
      for (int r = 0; r < PEEL_ROUNDS && cand; ++r) {  // wave-uniform: cand is a ballot
        const int leader = __ffsll((unsigned long long)cand) - 1;
        const int32_t ls = __shfl(s, leader, 64);
        const bool mine = (s == ls);
        const uint64_t m = __ballot(mine);
        cand &= ~m;
        if (__popcll(m) < 2) continue;
        const unsigned long long sum = wave_sum_u64(mine ? (unsigned long long)v : 0ull);
        const uint32_t mx = wave_max_u32(mine ? v : 0u);
        const unsigned long long n0 = __popcll(__ballot(mine && (f & 1)));
        const unsigned long long n1 = __popcll(__ballot(mine && (f & 2)));
        const unsigned long long n2 = __popcll(__ballot(mine && (f & 4)));
        if (lane == leader) rec_put(ltag, lrec, rec, ls, (unsigned long long)__popcll(m), sum, mx, n0, n1, n2);
        if (mine) rec_todo = false;
        uint64_t hc = m;
        for (int q = 0; q < PEEL_ROUNDS && hc; ++q) {
          const int l2 = __ffsll((unsigned long long)hc) - 1;
          const int lb = __shfl(b, l2, 64);
          const bool same = mine && b == lb;
          const uint64_t m2 = __ballot(same);
          hc &= ~m2;
          if (__popcll(m2) < 2) continue;
          if (lane == l2) atomicAdd(hist + (int64_t)ls * NB + lb, (uint32_t)__popcll(m2));
          if (same) hist_todo = false;
        }
      }
    }
    if (rec_todo) {
      if (PEEL)
        rec_put(ltag, lrec, rec, s, 1ull, v, v, f & 1, (f >> 1) & 1, (f >> 2) & 1);
      else
        rec_add(rec + (int64_t)s * REC, 1ull, v, v, f & 1, (f >> 1) & 1, (f >> 2) & 1);
    }
    if (hist_todo) atomicAdd(hist + (int64_t)s * NB + b, 1u);
  }
  if (PEEL) {
    __syncthreads();
    for (int j = threadIdx.x; j < RC_SLOTS; j += TPB) {
      const int32_t t = ltag[j];
      const unsigned long long* r = lrec + j * RC_WORDS;
      if (t >= 0 && r[0]) rec_add(rec + (int64_t)t * REC, r[0], r[1], (uint32_t)r[2], r[3], r[4], r[5]);
    }
  }
}

// ---- quantiles --------------------------------------------------------------------------------
struct QArgs {
  int32_t q[MAXQ];
};

__global__ __launch_bounds__(TPB) void quantiles(const int64_t* __restrict__ rec, const uint32_t* __restrict__ hist,
                                                 int32_t S, QArgs qa, int32_t Q, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wpb = TPB / 64;
  for (int64_t s = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); s < S; s += (int64_t)gridDim.x * wpb) {  // per wave
    const int64_t n = rec[s * REC];
    const int64_t mxw = rec[s * REC + 2];
    const uint32_t mx = mxw < 0 ? 0u : (mxw > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)mxw);
    uint32_t c[PER_LANE];
    unsigned long long local = 0;
    const uint32_t* row = hist + s * NB + lane * PER_LANE;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
      c[j] = row[j];
      local += c[j];
    }
    unsigned long long incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long w = (unsigned long long)__shfl_up((long long)incl, o, 64);
      if (lane >= o) incl += w;
    }
    const unsigned long long excl = incl - local;
    for (int qi = 0; qi < Q; ++qi) {
      unsigned long long k = 0;
      if (n > 0) k = ((unsigned long long)qa.q[qi] * (unsigned long long)n + 999ull) / 1000ull;
      const bool hit = k > excl && k <= incl;  // k >= 1: at most one lane
      if (hit) {
        unsigned long long run = excl;
        int bsel = lane * PER_LANE + PER_LANE - 1;
        bool found = false;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
          run += c[j];
          if (!found && run >= k) {
            bsel = lane * PER_LANE + j;
            found = true;
          }
        }
        const uint32_t h = bucket_hi(bsel);
        out[s * Q + qi] = h < mx ? h : mx;
      }
      if (__ballot(hit) == 0 && lane == 0) out[s * Q + qi] = 0;  // empty slot (or a record that disagrees with its histogram)
    }
  }
}

}  // namespace

extern "C" {

int32_t krca_trace_nbuckets(void) { return NB; }
int32_t krca_trace_bucket(uint32_t d) { return bucket_of(d); }
int krca_trace_bucket_bounds(int32_t b, uint32_t* lo_host, uint32_t* hi_host) {
  KRCA_CHECK_ARG(b >= 0 && b < NB && lo_host && hi_host, "krca_trace_bucket_bounds: b=%d not in [0, %d) or null out", b, NB);
  *lo_host = bucket_lo(b);
  *hi_host = bucket_hi(b);
  return KRCA_OK;
}
int32_t krca_trace_lds_max_slots(void) { return LDS_MAX_SLOTS; }

int64_t krca_trace_link_ws_size(int64_t N) { return 8 * link_ws_words(std::max<int64_t>(N, 0)); }

int krca_trace_link(const int32_t* svc, const int32_t* parent, const uint32_t* dur_us, const uint8_t* err, int64_t N,
                    int32_t S, int32_t* caller_svc, uint32_t* self_us, uint8_t* flags, void* ws, void* stream) {
  KRCA_CHECK_ARG(N >= 0 && N < INT_MAX, "krca_trace_link: N=%lld out of [0, 2^31-1)", (long long)N);
  KRCA_CHECK_ARG(S >= 0, "krca_trace_link: S < 0");
  KRCA_CHECK_ARG(ws, "krca_trace_link: null workspace");
  hipStream_t st = krca::as_stream(stream);
  unsigned long long* w = static_cast<unsigned long long*>(ws);
  const int64_t words = link_ws_words(N);
  hipLaunchKernelGGL(fill_u64, dim3(grid_for(words)), dim3(TPB), 0, st, (uint64_t*)w, words, (uint64_t)0);
  KRCA_LAUNCH_CHECK();
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(svc && parent && dur_us && err && caller_svc && self_us && flags, "krca_trace_link: null array");
  unsigned long long* child_sum = w + LINK_HDR;
  uint32_t* child_err = reinterpret_cast<uint32_t*>(w + LINK_HDR + N);
  hipLaunchKernelGGL(link_scatter, dim3(grid_for(N)), dim3(TPB), 0, st, svc, parent, dur_us, err, N, S, w, child_sum,
                     child_err);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(link_final, dim3(grid_for(N)), dim3(TPB), 0, st, svc, parent, dur_us, err, N, S, child_sum,
                     child_err, caller_svc, self_us, flags);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

int64_t krca_trace_edge_ws_size(int64_t cap) { return 8 * 8 + 12 * hash_slots(std::max<int64_t>(cap, 0)); }

int krca_trace_edges(const int32_t* caller_svc, const int32_t* svc, int64_t N, int32_t S, int64_t cap, void* ws,
                     int64_t* edge_key, int32_t* edge_slot, int64_t* n_edges_host, void* stream) {
  KRCA_CHECK_ARG(N >= 0 && N < INT_MAX, "krca_trace_edges: N=%lld out of [0, 2^31-1)", (long long)N);
  KRCA_CHECK_ARG(S >= 0 && cap >= 0 && cap < (1ll << 40), "krca_trace_edges: S=%d or cap=%lld out of range", S,
                 (long long)cap);
  KRCA_CHECK_ARG(ws && n_edges_host, "krca_trace_edges: null workspace or count");
  *n_edges_host = 0;
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(caller_svc && svc && edge_slot && (edge_key || cap == 0), "krca_trace_edges: null array");
  hipStream_t st = krca::as_stream(stream);
  const int64_t T = hash_slots(cap);
  unsigned long long* counters = static_cast<unsigned long long*>(ws);
  long long* table = reinterpret_cast<long long*>(counters + 8);
  int32_t* rank = reinterpret_cast<int32_t*>(table + T);
  hipLaunchKernelGGL(fill_u64, dim3(grid_for(8)), dim3(TPB), 0, st, (uint64_t*)counters, (int64_t)8, (uint64_t)0);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(fill_u64, dim3(grid_for(T)), dim3(TPB), 0, st, (uint64_t*)table, T, ~(uint64_t)0);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_insert, dim3(grid_for(N)), dim3(TPB), 0, st, caller_svc, svc, N, S, cap, T, counters, table);
  KRCA_LAUNCH_CHECK();
  unsigned long long count = 0;
  KRCA_HIP(hipMemcpyAsync(&count, counters, sizeof(count), hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  *n_edges_host = (int64_t)count;
  if ((int64_t)count > cap) return KRCA_OK;  // a lower bound: the caller grows cap and calls again
  const int64_t E = (int64_t)count;
  if (E == 0) {
    hipLaunchKernelGGL(fill_i32, dim3(grid_for(N)), dim3(TPB), 0, st, edge_slot, N, (int32_t)-1);
    KRCA_LAUNCH_CHECK();
    KRCA_HIP(hipStreamSynchronize(st));
    return KRCA_OK;
  }
  hipLaunchKernelGGL(edge_compact, dim3(grid_for(T)), dim3(TPB), 0, st, table, T, cap, counters, edge_key);
  KRCA_LAUNCH_CHECK();
  std::vector<int64_t> keys((size_t)E);  // E distinct edges, far fewer than spans: ordered on the host
  KRCA_HIP(hipMemcpyAsync(keys.data(), edge_key, sizeof(int64_t) * E, hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  std::sort(keys.begin(), keys.end());
  KRCA_HIP(hipMemcpyAsync(edge_key, keys.data(), sizeof(int64_t) * E, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(edge_rank, dim3(grid_for(T)), dim3(TPB), 0, st, table, T, edge_key, E, rank);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_lookup, dim3(grid_for(N)), dim3(TPB), 0, st, caller_svc, svc, N, S, T, table, rank, edge_slot);
  KRCA_LAUNCH_CHECK();
  KRCA_HIP(hipStreamSynchronize(st));
  return KRCA_OK;
}

int krca_trace_stats(const int32_t* slot, const uint32_t* val, const uint8_t* flags, int64_t N, int32_t S,
                     int32_t accumulate, int64_t* rec, uint32_t* hist, void* stream) {
  KRCA_CHECK_ARG(N >= 0 && N < INT_MAX, "krca_trace_stats: N=%lld out of [0, 2^31-1)", (long long)N);
  KRCA_CHECK_ARG(S >= 0, "krca_trace_stats: S < 0");
  if (S == 0) return KRCA_OK;
  KRCA_CHECK_ARG(rec && hist && ((uintptr_t)hist & 7) == 0, "krca_trace_stats: null or misaligned output");
  const int impl = krca::tuning().trace_impl;
  KRCA_CHECK_ARG(impl >= 0 && impl <= 3, "krca_trace_stats: KRCA_TRACE_IMPL=%d not in [0, 3]", impl);
  KRCA_CHECK_ARG(impl != 1 || S <= LDS_MAX_SLOTS, "krca_trace_stats: KRCA_TRACE_IMPL=1 (LDS) holds at most %d slots, S=%d",
                 LDS_MAX_SLOTS, S);
  hipStream_t st = krca::as_stream(stream);
  if (!accumulate) {
    hipLaunchKernelGGL(fill_u64, dim3(grid_for((int64_t)S * REC)), dim3(TPB), 0, st, (uint64_t*)rec, (int64_t)S * REC,
                       (uint64_t)0);
    KRCA_LAUNCH_CHECK();
    hipLaunchKernelGGL(fill_u64, dim3(grid_for((int64_t)S * NB / 2)), dim3(TPB), 0, st, (uint64_t*)hist,
                       (int64_t)S * NB / 2, (uint64_t)0);  // NB is even, hist 8-byte aligned
    KRCA_LAUNCH_CHECK();
  }
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(slot && val && flags, "krca_trace_stats: null input");
  const bool lds = impl == 1 || (impl == 0 && S <= LDS_MAX_SLOTS);
  if (lds) {
    // each thread takes 16 or more records before another workgroup (and its flush) is added
    const unsigned grid = grid_for(N, TPB_LDS * 16, 512);
    hipLaunchKernelGGL(stats_lds, dim3(grid), dim3(TPB_LDS), (size_t)S * SLOT_BYTES, st, slot, val, flags, N, S, rec, hist);
  } else if (impl == 3) {
    hipLaunchKernelGGL((stats_global<false>), dim3(grid_for(N)), dim3(TPB), 0, st, slot, val, flags, N, S, rec, hist);
  } else {
    // 32 or more records per thread before another workgroup (and its record-cache flush) is added
    hipLaunchKernelGGL((stats_global<true>), dim3(grid_for(N, TPB * 32, 2048)), dim3(TPB), 0, st, slot, val, flags, N, S,
                       rec, hist);
  }
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

int krca_trace_quantiles(const int64_t* rec, const uint32_t* hist, int32_t S, const int32_t* permille_host, int32_t Q,
                         uint32_t* out, void* stream) {
  KRCA_CHECK_ARG(S >= 0, "krca_trace_quantiles: S < 0");
  KRCA_CHECK_ARG(Q >= 1 && Q <= MAXQ && permille_host, "krca_trace_quantiles: Q=%d not in [1, %d] or null permille", Q, MAXQ);
  QArgs qa = {};
  for (int i = 0; i < Q; ++i) {
    KRCA_CHECK_ARG(permille_host[i] >= 1 && permille_host[i] <= 1000, "krca_trace_quantiles: permille[%d]=%d not in [1, 1000]",
                   i, permille_host[i]);
    qa.q[i] = permille_host[i];
  }
  if (S == 0) return KRCA_OK;
  KRCA_CHECK_ARG(rec && hist && out, "krca_trace_quantiles: null array");
  hipStream_t st = krca::as_stream(stream);
  hipLaunchKernelGGL(quantiles, dim3(grid_for(S, TPB / 64)), dim3(TPB), 0, st, rec, hist, S, qa, Q, out);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

}  // extern "C"
