// Log-template novelty across stream windows: a device-resident open-addressing table
// keyed by the exact pair (group, template hash) and the kernels that fold one window's
// krca_template_hist output into it.
//
// Key claim without a lock or a spin: CAS the hash word EMPTY -> h and go on if the previous value was
// EMPTY or h; CAS the group word EMPTY_G -> g; the slot is this key's if the previous value was EMPTY_G
// or g, else the probe moves to the next slot.  Every thread that sets a hash word goes on to the group
// word, so no slot is left with a hash and no group when the kernel ends; keys are never removed (expiry
// restarts a record in place, the rehash reclaims), so every probe for a key sees the same chain and a
// key sits in exactly one slot.  The key words are read with plain (agent-scope) loads first: in
// steady state almost every key exists and costs no CAS.
//
// nov_insert   walks the containers (a lane per container of <= kShort templates, the wave for a longer
//              one): per entry one 64-bit add (cur_docs and cur_lines packed) and one atomicMin
//              (first_doc), folded per workgroup in LDS first and flushed once per distinct key; the
//              first toucher of a global slot appends it to the touched list.
// nov_finish   over the touched list: expiry, NOVEL / SURGE, report append, commit, per-window fields
//              cleared; or, when the insert pass could not place a key, the rollback of those fields.
// nov_docs     second walk: the committed flags of every container's templates -> doc_novel, doc_surge.
// nov_init / nov_rehash  initialise a table; reinsert the records young enough into a new one.
// One read-back per update (the header's counters), after the last kernel.
#include <limits.h>
#include <stdint.h>

#include <algorithm>

#include "graph_rows.h"
#include "tmpl_novelty_layout.h"

namespace {

using krca::NovHeader;
using krca::NovReport;
using krca::NovSlot;
typedef unsigned long long u64;

constexpr int kInsertRounds = 4;  // containers per thread of the insert pass (its LDS fold wants many entries)
constexpr int64_t kProbeBlock = 1024;  // probes between two looks at the overflow flag
constexpr int kShort = 8;  // templates a single lane walks; a longer container is left to the wave
constexpr uint64_t kLinesMask = (1ull << krca::kNovLinesBits) - 1;

template <class T>
__device__ __forceinline__ T load_relaxed(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the table behind a header: capacity 0 when the header is not one nov_init wrote (the kernels then do nothing)
struct Table {
  NovSlot* slots;
  int32_t* touched;
  int64_t capacity;
};
__device__ __forceinline__ Table table_of(NovHeader* hdr) {
  char* b = reinterpret_cast<char*>(hdr) + krca::kNovHeaderBytes;
  const int64_t c = hdr->magic == krca::kNovMagic ? hdr->capacity : 0;
  const bool ok = c >= krca::kNovMinCapacity && c <= krca::kNovMaxCapacity && (c & (c - 1)) == 0;
  return {reinterpret_cast<NovSlot*>(b), reinterpret_cast<int32_t*>(b + (ok ? c : 0) * krca::kNovSlotBytes), ok ? c : 0};
}

// the slot of key (g, h), claimed if `claim` and absent; -1: not there / no slot left (or the overflow
// flag is up: the window is rolled back anyway)
__device__ __forceinline__ int64_t nov_find(NovSlot* __restrict__ slots, int64_t capacity, uint64_t h, int32_t g,
                                            bool claim, NovHeader* __restrict__ hdr) {
  const int64_t mask = capacity - 1;
  int64_t s = krca::nov_home(h, g, capacity);
  for (int64_t n0 = 0; n0 < capacity; n0 += kProbeBlock) {
    // the call already fails (some key found no slot): stop walking a full table.  Looked at once per
    // kProbeBlock slots only: looked at every 32 slots, the 512 k-key window of the bench took a third longer
    if (n0 && load_relaxed(&hdr->overflow)) return -1;
    const int64_t n1 = n0 + kProbeBlock < capacity ? n0 + kProbeBlock : capacity;
    for (int64_t n = n0; n < n1; ++n, s = (s + 1) & mask) {
      uint64_t kh = load_relaxed(&slots[s].hash);
      if (kh == krca::kNovEmptyHash) {
        if (!claim) return -1;
        kh = atomicCAS(reinterpret_cast<u64*>(&slots[s].hash), (u64)krca::kNovEmptyHash, (u64)h);
        if (kh == krca::kNovEmptyHash) kh = h;
      }
      if (kh != h) continue;
      int32_t kg = load_relaxed(&slots[s].group);
      if (kg == krca::kNovEmptyGroup) {
        if (!claim) return -1;
        kg = atomicCAS(&slots[s].group, krca::kNovEmptyGroup, g);
        if (kg == krca::kNovEmptyGroup) {
          kg = g;
          atomicAdd(reinterpret_cast<u64*>(&hdr->n_claimed), 1ull);
        }
      }
      if (kg == g) return s;
    }
  }
  return -1;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x) {
  for (int m = 32; m; m >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), m, 64);
    x += ((uint64_t)hi << 32) | lo;
  }
  return x;
}
__device__ __forceinline__ int64_t shfl_i64(int64_t x, int l) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, l, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)x >> 32), l, 64);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Entry walk: f(d, g, idx) -> uint64 for every entry slot idx = doc_line0[d] + j, j < n_templates[d],
// inside [0, n_lines); fin(d, sum of f) once per container d of [0, ndocs), by one lane.  A container
// with a negative group or template count has no entries.  Waves stride over the containers.
template <class F, class E>
__device__ __forceinline__ void for_entries(const int32_t* __restrict__ n_templates, const int64_t* __restrict__ doc_line0,
                                            const int32_t* __restrict__ group, int64_t ndocs, int64_t n_lines, F f, E fin) {
  const int64_t first = (int64_t)blockIdx.x * TPB + (threadIdx.x & ~63), nthr = (int64_t)gridDim.x * TPB;
  for (int64_t base = first; base < ndocs; base += nthr) {  // wave-uniform
    const int64_t d = base + lane_id();
    int32_t n = 0, g = 0;
    uint64_t o = 0;
    if (d < ndocs) {
      n = n_templates[d];
      o = (uint64_t)doc_line0[d];
      g = group ? group[d] : 0;
      if (g < 0 || n < 0) n = 0;
    }
    const bool lng = n > kShort;
    if (d < ndocs && !lng) {
      uint64_t acc = 0;
      for (int32_t j = 0; j < n; ++j) {
        const uint64_t idx = o + (uint64_t)j;
        if (idx < (uint64_t)n_lines) acc += f(d, g, (int64_t)idx);
      }
      fin(d, acc);
    }
    uint64_t todo = __ballot(lng);
    while (todo) {  // wave-uniform
      const int l = __ffsll((u64)todo) - 1;
      todo &= todo - 1;
      const int32_t nn = __shfl(n, l, 64), gg = __shfl(g, l, 64);
      const uint64_t oo = (uint64_t)shfl_i64((int64_t)o, l);
      uint64_t acc = 0;
      for (int32_t j = lane_id(); j < nn; j += 64) {
        const uint64_t idx = oo + (uint64_t)j;
        if (idx < (uint64_t)n_lines) acc += f(base + l, gg, (int64_t)idx);
      }
      acc = wave_sum_u64(acc);
      if (lane_id() == 0) fin(base + l, acc);
    }
  }
}

// Per-workgroup pre-aggregation of the insert pass: the window's hot templates show in most containers,
// and one global atomic per entry on their few slots serialises in L2.  Each workgroup first folds its
// entries into an LDS table of kLds keys (the same claim protocol, LDS atomics, at most kLdsProbes
// probes; an entry that finds no LDS slot goes to the global table directly) and then flushes one
// global add per distinct key it holds.
constexpr int kLds = 1024, kLdsProbes = 8;
struct LdsTable {
  u64 hash[kLds];
  u64 cur[kLds];
  int32_t group[kLds];
  int32_t first_doc[kLds];
};

__device__ __forceinline__ bool lds_add(LdsTable& t, uint64_t h, int32_t g, u64 add, int32_t d) {
  int s = (int)krca::nov_home(h, g, kLds);
  for (int n = 0; n < kLdsProbes; ++n, s = (s + 1) & (kLds - 1)) {
    u64 kh = __hip_atomic_load(&t.hash[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (kh == krca::kNovEmptyHash) {
      kh = atomicCAS(&t.hash[s], (u64)krca::kNovEmptyHash, (u64)h);
      if (kh == krca::kNovEmptyHash) kh = h;
    }
    if (kh != h) continue;
    int32_t kg = __hip_atomic_load(&t.group[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (kg == krca::kNovEmptyGroup) {
      kg = atomicCAS(&t.group[s], krca::kNovEmptyGroup, g);
      if (kg == krca::kNovEmptyGroup) kg = g;
    }
    if (kg != g) continue;
    atomicAdd(&t.cur[s], add);
    atomicMin(&t.first_doc[s], d);
    return true;
  }
  return false;
}

// one key's window contribution into the global table; false: no slot left
__device__ __forceinline__ bool nov_add(NovHeader* __restrict__ hdr, NovSlot* __restrict__ slots,
                                        int32_t* __restrict__ touched, int64_t capacity, uint64_t h, int32_t g, u64 add,
                                        int32_t d) {
  const int64_t s = nov_find(slots, capacity, h, g, true, hdr);
  if (s < 0) {
    hdr->overflow = 1;
    return false;
  }
  const u64 old = atomicAdd(reinterpret_cast<u64*>(&slots[s].cur), add);
  if (old == 0) touched[atomicAdd(&hdr->n_touched, 1)] = (int32_t)s;  // distinct slots: below capacity
  atomicMin(&slots[s].first_doc, d);
  return true;
}

__global__ __launch_bounds__(TPB) void nov_insert(NovHeader* __restrict__ hdr, const uint64_t* __restrict__ tmpl_hash,
                                                  const int32_t* __restrict__ tmpl_count,
                                                  const int32_t* __restrict__ n_templates,
                                                  const int64_t* __restrict__ doc_line0,
                                                  const int32_t* __restrict__ group, int64_t ndocs, int64_t n_lines) {
  __shared__ LdsTable lds;
  const Table t = table_of(hdr);
  if (!t.capacity) return;  // the same for the whole grid
  NovSlot* __restrict__ slots = t.slots;
  int32_t* __restrict__ touched = t.touched;
  const int64_t capacity = t.capacity;
  for (int i = threadIdx.x; i < kLds; i += TPB) {
    lds.hash[i] = krca::kNovEmptyHash;
    lds.cur[i] = 0;
    lds.group[i] = krca::kNovEmptyGroup;
    lds.first_doc[i] = krca::kNovNoDoc;
  }
  __syncthreads();
  uint64_t mine = 0;
  for_entries(
      n_templates, doc_line0, group, ndocs, n_lines,
      [&](int64_t d, int32_t g, int64_t idx) -> uint64_t {
        const int32_t c = tmpl_count[idx];
        if (c <= 0) return 0;
        const uint64_t h = krca::nov_remap(tmpl_hash[idx]);
        const u64 add = (1ull << krca::kNovLinesBits) | (u64)c;
        if (!lds_add(lds, h, g, add, (int32_t)d)) nov_add(hdr, slots, touched, capacity, h, g, add, (int32_t)d);
        return 1;
      },
      [&](int64_t, uint64_t acc) { mine += acc; });
  __syncthreads();
  for (int i = threadIdx.x; i < kLds; i += TPB)
    if (lds.group[i] != krca::kNovEmptyGroup)  // a claimed hash word always has its group by now
      nov_add(hdr, slots, touched, capacity, lds.hash[i], lds.group[i], lds.cur[i], lds.first_doc[i]);
  mine = wave_sum_u64(mine);
  if (lane_id() == 0 && mine) atomicAdd(reinterpret_cast<u64*>(&hdr->n_entries), (u64)mine);
}

// a * b >= c * d over the non-negative 64-bit values, exactly (128-bit products)
__device__ __forceinline__ bool mul_ge(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  const uint64_t lh = __umul64hi(a, b), ll = a * b, rh = __umul64hi(c, d), rl = c * d;
  return lh != rh ? lh > rh : ll >= rl;
}

__global__ __launch_bounds__(TPB) void nov_finish(NovHeader* __restrict__ hdr, int32_t window, int32_t ttl,
                                                  int32_t surge_ratio, int32_t surge_min, int32_t report,
                                                  NovReport* __restrict__ rep, int32_t cap) {
  const Table t = table_of(hdr);
  if (!t.capacity) return;
  NovSlot* __restrict__ slots = t.slots;
  const int32_t* __restrict__ touched = t.touched;
  const int32_t n = hdr->n_touched;
  const bool rollback = hdr->overflow != 0;
  const int64_t first = (int64_t)blockIdx.x * TPB + (threadIdx.x & ~63), nthr = (int64_t)gridDim.x * TPB;
  for (int64_t base = first; base < n; base += nthr) {  // wave-uniform
    const int64_t i = base + lane_id();
    const bool on = i < n;
    NovSlot* sl = on ? &slots[touched[i]] : nullptr;
    if (rollback) {
      if (on) {
        sl->cur = 0;
        sl->first_doc = krca::kNovNoDoc;
      }
      continue;
    }
    int32_t flags = 0;
    bool born = false;
    if (on) {
      const uint64_t cur = sl->cur;
      const int64_t lines = (int64_t)(cur & kLinesMask);
      const int32_t docs = (int32_t)(cur >> krca::kNovLinesBits);
      const int32_t n_win = sl->n_win;
      const bool absent = n_win == 0 || (ttl > 0 && (int64_t)sl->last_win < (int64_t)window - ttl);
      const int64_t total = absent ? 0 : sl->total;
      const int32_t first_win = absent ? window : sl->first_win;
      if (report) {
        if (absent) flags = krca::kNovNovel;
        else if (lines >= surge_min && mul_ge((uint64_t)lines, (uint64_t)std::max(window - first_win, 0), (uint64_t)surge_ratio,
                                               (uint64_t)total))
          flags = krca::kNovSurge;
      }
      born = n_win == 0;
      // commit
      sl->first_win = first_win;
      sl->last_win = window;
      sl->n_win = absent ? 1 : n_win + 1;
      sl->total = total + lines;
      sl->flags = flags;
      sl->cur = 0;
      const int32_t first_doc = sl->first_doc;
      sl->first_doc = krca::kNovNoDoc;
      // the report record
      const uint64_t m = __ballot(flags != 0);
      if (flags) {
        const int leader = __ffsll((u64)m) - 1;
        int32_t at = 0;
        if (lane_id() == leader) at = atomicAdd(&hdr->n_reported, __popcll((u64)m));
        at = __shfl(at, leader, 64) + __popcll((u64)(m & ((1ull << lane_id()) - 1)));
        if (at < cap) {
          NovReport r;
          r.hash = sl->hash;
          r.total_before = total;
          r.cur_lines = lines;
          r.group = sl->group;
          r.flags = flags;
          r.cur_docs = docs;
          r.first_doc = first_doc;
          r.first_win = first_win;
          r.pad = 0;
          rep[at] = r;
        }
      }
    }
    const uint64_t mn = __ballot(flags == krca::kNovNovel), ms = __ballot(flags == krca::kNovSurge), mb = __ballot(born);
    if (lane_id() == 0) {
      if (mn) atomicAdd(&hdr->n_novel, __popcll((u64)mn));
      if (ms) atomicAdd(&hdr->n_surge, __popcll((u64)ms));
      if (mb) atomicAdd(reinterpret_cast<u64*>(&hdr->n_live), (u64)__popcll((u64)mb));
    }
  }
}

__global__ __launch_bounds__(TPB) void nov_docs(NovHeader* __restrict__ hdr, const uint64_t* __restrict__ tmpl_hash,
                                                const int32_t* __restrict__ tmpl_count,
                                                const int32_t* __restrict__ n_templates,
                                                const int64_t* __restrict__ doc_line0,
                                                const int32_t* __restrict__ group, int64_t ndocs, int64_t n_lines,
                                                int32_t report, int32_t* __restrict__ doc_novel,
                                                int32_t* __restrict__ doc_surge) {
  const Table t = table_of(hdr);
  if (!t.capacity || hdr->overflow) return;  // the call fails: outputs unspecified
  NovSlot* __restrict__ slots = t.slots;
  const int64_t capacity = t.capacity;
  for_entries(
      n_templates, doc_line0, group, ndocs, n_lines,
      [&](int64_t, int32_t g, int64_t idx) -> uint64_t {
        if (!report || tmpl_count[idx] <= 0) return 0;
        const int64_t s = nov_find(slots, capacity, krca::nov_remap(tmpl_hash[idx]), g, false, hdr);
        if (s < 0) return 0;
        const int32_t fl = slots[s].flags;
        return (uint64_t)(fl & krca::kNovNovel) | ((uint64_t)((fl & krca::kNovSurge) != 0) << 32);
      },
      [&](int64_t d, uint64_t acc) {
        if (doc_novel) doc_novel[d] = (int32_t)(uint32_t)acc;
        if (doc_surge) doc_surge[d] = (int32_t)(acc >> 32);
      });
}

__global__ __launch_bounds__(TPB) void nov_init(NovHeader* __restrict__ hdr, NovSlot* __restrict__ slots, int64_t capacity) {
  const int64_t N = capacity;
  GS_NODES(s) {
    NovSlot e = {};
    e.hash = krca::kNovEmptyHash;
    e.group = krca::kNovEmptyGroup;
    e.first_doc = krca::kNovNoDoc;
    slots[s] = e;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    NovHeader h = {};
    h.magic = krca::kNovMagic;
    h.capacity = capacity;
    *hdr = h;
  }
}

__global__ void nov_window_begin(NovHeader* __restrict__ hdr) {
  hdr->n_entries = 0;
  hdr->n_touched = hdr->overflow = hdr->n_novel = hdr->n_surge = hdr->n_reported = 0;
}

__global__ __launch_bounds__(TPB) void nov_rehash(const NovSlot* __restrict__ old, int64_t N, NovHeader* __restrict__ hdr,
                                                  NovSlot* __restrict__ slots, int64_t capacity, int32_t min_last_window) {
  GS_NODES(i) {
    const NovSlot o = old[i];
    if (o.hash == krca::kNovEmptyHash || o.group == krca::kNovEmptyGroup || o.n_win <= 0 || o.last_win < min_last_window)
      continue;
    const int64_t s = nov_find(slots, capacity, o.hash, o.group, true, hdr);
    if (s < 0) {
      hdr->overflow = 1;
      continue;
    }
    slots[s].first_win = o.first_win;  // one old slot per key: no other thread writes this record
    slots[s].last_win = o.last_win;
    slots[s].n_win = o.n_win;
    slots[s].total = o.total;
    slots[s].flags = o.flags;
    atomicAdd(reinterpret_cast<u64*>(&hdr->n_live), 1ull);
  }
}

struct State {
  NovHeader* hdr;
  NovSlot* slots;
  int32_t* touched;
};
State state_of(void* state, int64_t capacity) {
  char* b = reinterpret_cast<char*>(state);
  return {reinterpret_cast<NovHeader*>(b), reinterpret_cast<NovSlot*>(b + krca::kNovHeaderBytes),
          reinterpret_cast<int32_t*>(b + krca::kNovHeaderBytes + capacity * krca::kNovSlotBytes)};
}
unsigned grid_for(int64_t n, int64_t most) { return (unsigned)std::max<int64_t>(1, std::min(most, krca::ceil_div(n, TPB))); }

int read_header(const void* state, NovHeader* h, hipStream_t st, const char* who) {
  KRCA_HIP(hipMemcpyAsync(h, state, sizeof(*h), hipMemcpyDeviceToHost, st));
  KRCA_HIP(hipStreamSynchronize(st));
  if (h->magic != krca::kNovMagic || !krca::nov_capacity_ok(h->capacity)) {
    krca::set_error("%s: the state was not initialised by krca_template_novelty_init", who);
    return KRCA_EINVAL;
  }
  return KRCA_OK;
}

}  // namespace

extern "C" {

int64_t krca_template_novelty_layout(int32_t which) {
  switch (which) {
    case 0: return krca::kNovHeaderBytes;
    case 1: return krca::kNovSlotBytes;
    case 2: return krca::kNovReportBytes;
    case 3: return krca::kNovLinesBits;
    case 4: return krca::kNovMaxDocs;
    default: return -1;
  }
}

int64_t krca_template_novelty_home_slot(uint64_t hash, int32_t group, int64_t capacity) {
  if (!krca::nov_capacity_ok(capacity) || group < 0) return -1;
  return krca::nov_home(krca::nov_remap(hash), group, capacity);
}

int64_t krca_template_novelty_state_size(int64_t capacity) {
  return krca::nov_capacity_ok(capacity) ? krca::nov_state_bytes(capacity) : 0;
}

int krca_template_novelty_init(void* state, int64_t capacity, void* stream) {
  KRCA_CHECK_ARG(krca::nov_capacity_ok(capacity), "krca_template_novelty_init: capacity %lld is no power of two in [64, 2^30]",
                 (long long)capacity);
  KRCA_CHECK_ARG(state != nullptr, "krca_template_novelty_init: null state");
  hipStream_t st = krca::as_stream(stream);
  State s = state_of(state, capacity);
  hipLaunchKernelGGL(nov_init, dim3(grid_for(capacity, 1 << 16)), dim3(TPB), 0, st, s.hdr, s.slots, capacity);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

int krca_template_novelty_update(void* state, const uint64_t* tmpl_hash, const int32_t* tmpl_count,
                                 int64_t n_lines, const int32_t* n_templates, const int64_t* doc_line0,
                                 const int32_t* group, int64_t ndocs, int32_t window, int32_t ttl, int32_t surge_ratio,
                                 int32_t surge_min, int32_t report, void* report_out, int32_t cap, int32_t* doc_novel,
                                 int32_t* doc_surge, int64_t* counts_host, void* stream) {
  KRCA_CHECK_ARG(ndocs >= 0 && ndocs <= krca::kNovMaxDocs, "krca_template_novelty_update: ndocs = %lld outside [0, 2^24 - 1]",
                 (long long)ndocs);
  KRCA_CHECK_ARG(n_lines >= 0 && window >= 0 && ttl >= 0 && cap >= 0,
                 "krca_template_novelty_update: negative n_lines, window, ttl or cap");
  KRCA_CHECK_ARG(surge_ratio >= 1 && surge_min >= 1, "krca_template_novelty_update: surge_ratio and surge_min must be >= 1");
  KRCA_CHECK_ARG(!(report != 0 && cap > 0 && report_out == nullptr),
                 "krca_template_novelty_update: report asked for with cap > 0 and a null report buffer");
  KRCA_CHECK_ARG(state && counts_host, "krca_template_novelty_update: null state or counts");
  KRCA_CHECK_ARG(ndocs == 0 || (n_templates && doc_line0 && (n_lines == 0 || (tmpl_hash && tmpl_count))),
                 "krca_template_novelty_update: null template array");
  for (int i = 0; i < 6; ++i) counts_host[i] = 0;
  hipStream_t st = krca::as_stream(stream);
  NovHeader* hdr = reinterpret_cast<NovHeader*>(state);
  hipLaunchKernelGGL(nov_window_begin, dim3(1), dim3(1), 0, st, hdr);
  KRCA_LAUNCH_CHECK();
  const unsigned walk_grid = grid_for(ndocs, 1 << 16);
  if (ndocs > 0 && n_lines > 0) {
    hipLaunchKernelGGL(nov_insert, dim3(grid_for(krca::ceil_div(ndocs, kInsertRounds), 1 << 16)), dim3(TPB), 0, st, hdr, tmpl_hash, tmpl_count, n_templates, doc_line0, group, ndocs, n_lines);
    KRCA_LAUNCH_CHECK();
    // the touched count stays on the device: a grid that strides over the list
    hipLaunchKernelGGL(nov_finish, dim3(grid_for(n_lines, 2048)), dim3(TPB), 0, st, hdr, window, ttl, surge_ratio, surge_min, report ? 1 : 0,
                       reinterpret_cast<NovReport*>(report_out), report ? cap : 0);
    KRCA_LAUNCH_CHECK();
  }
  if (ndocs > 0 && (doc_novel || doc_surge)) {
    hipLaunchKernelGGL(nov_docs, dim3(walk_grid), dim3(TPB), 0, st, hdr, tmpl_hash, tmpl_count, n_templates, doc_line0, group, ndocs, n_lines, report ? 1 : 0, doc_novel, doc_surge);
    KRCA_LAUNCH_CHECK();
  }
  NovHeader h;
  if (int rc = read_header(state, &h, st, "krca_template_novelty_update")) return rc;
  counts_host[0] = h.n_entries;
  counts_host[1] = h.n_touched;
  counts_host[5] = h.n_live;
  if (h.overflow) {
    krca::set_error("krca_template_novelty_update: the table of %lld slots is full (%lld hold a key); rehash into a larger one",
                    (long long)h.capacity, (long long)h.n_claimed);
    return KRCA_ENOMEM;
  }
  counts_host[2] = h.n_novel;
  counts_host[3] = h.n_surge;
  counts_host[4] = h.n_reported;
  return KRCA_OK;
}

int krca_template_novelty_rehash(const void* old_state, void* new_state, int64_t new_capacity, int32_t min_last_window,
                                 void* stream) {
  KRCA_CHECK_ARG(krca::nov_capacity_ok(new_capacity),
                 "krca_template_novelty_rehash: capacity %lld is no power of two in [64, 2^30]", (long long)new_capacity);
  KRCA_CHECK_ARG(old_state && new_state && old_state != new_state, "krca_template_novelty_rehash: null or aliased state");
  hipStream_t st = krca::as_stream(stream);
  NovHeader h;
  if (int rc = read_header(old_state, &h, st, "krca_template_novelty_rehash")) return rc;
  State o = state_of(const_cast<void*>(old_state), h.capacity), s = state_of(new_state, new_capacity);
  hipLaunchKernelGGL(nov_init, dim3(grid_for(new_capacity, 1 << 16)), dim3(TPB), 0, st, s.hdr, s.slots, new_capacity);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(nov_rehash, dim3(grid_for(h.capacity, 1 << 16)), dim3(TPB), 0, st, o.slots, h.capacity, s.hdr, s.slots,
                     new_capacity, min_last_window);
  KRCA_LAUNCH_CHECK();
  if (int rc = read_header(new_state, &h, st, "krca_template_novelty_rehash")) return rc;
  if (h.overflow) {
    krca::set_error("krca_template_novelty_rehash: %lld slots do not hold the surviving records", (long long)new_capacity);
    return KRCA_ENOMEM;
  }
  return KRCA_OK;
}

}  // extern "C"
