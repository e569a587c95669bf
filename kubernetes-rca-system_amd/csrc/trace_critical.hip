// krca_trace_critical — the critical path of every trace of a window (include/krca.h t1).
//
// Which of a span's microseconds was the request waiting for?  Each span is swept from its end
// towards its start over its children: the child that ended last before the cursor is SELECTED, the
// cursor moves to that child's start, a child still running at the cursor was hidden behind the one
// chosen.  A span is on the path when every link from it up to a root was selected; its critical
// time is its duration minus the selected children's clipped pieces.
//
// csrc has no sort: the children of a parent are gathered into one contiguous list and the sweep is a
// repeated arg-max over it.
//   mark      per span: bad / root / valid parent (vp[i], so no later pass gathers svc / start of a
//             parent again), children counted per parent with integer atomics.
//   scan      exclusive scan of the counts (tile sums, one workgroup over the sums, tiles again); the
//             last pass also appends the parents with more than SMALL_MAX children to a list.
//   scatter   each child claims a position in its parent's list and writes there its index and its
//             interval CLIPPED to the parent and RELATIVE to the parent's start: both ends lie in
//             [0, dur_p], two uint32.  Arrival order is arbitrary; the total tie order of the sweep
//             makes the result independent of it.
//   sweep     parents with 1 .. SMALL_MAX children: one lane each, O(c^2) over c * 8 contiguous bytes.
//             A workgroup first orders its 256 parents by child count (counting sort in LDS), so the
//             lanes of a wave carry similar counts.  Heavier parents: one workgroup each, a parallel
//             arg-max per selection.  The sweep writes crit_us[p] = dur_p - selected pieces.
//   final     per span: walk up the valid parents while the links are selected (at most D_MAX steps);
//             path bits; crit_us kept on the path, 0 off it.
// Everything is integer; no result depends on arrival order.
#include "krca_common.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int TPB = 256;
constexpr int D_MAX = 4096;
constexpr int SMALL_MAX = 16;          // 16 children = 128 contiguous bytes of (cs, ce) per lane: one cache line
constexpr int SCAN_PER = 8;
constexpr int SCAN_TILE = TPB * SCAN_PER;  // counts per scan tile
constexpr int SCAN2_TPB = 1024;
constexpr int HEAVY_GRID = 256;
constexpr int64_t HDR = 8;             // u64 words: 0 = bad spans, 1 = heavy parents
constexpr int64_t START_LIM = 1ll << 62;
constexpr int32_t VP_ROOT = -1, VP_BAD = -2;

// ws: header | rel uint2[N] | vp i32[N] | cnt u32[N] | off u32[N] | child u32[N] | heavy u32[N/(SMALL_MAX+1)+1]
//     | tile sums u32[tiles] | sel u8[N]; every part starts 8-byte aligned
struct Layout {
  int64_t rel, vp, cnt, off, child, heavy, bsum, sel, total, tiles;
};
inline int64_t up8(int64_t x) { return (x + 7) & ~(int64_t)7; }
inline Layout layout(int64_t N) {
  Layout L;
  L.tiles = krca::ceil_div(N, SCAN_TILE);
  int64_t o = HDR * 8;
  L.rel = o, o += 8 * N;
  L.vp = o, o += up8(4 * N);
  L.cnt = o, o += up8(4 * N);
  L.off = o, o += up8(4 * N);
  L.child = o, o += up8(4 * N);
  L.heavy = o, o += up8(4 * (N / (SMALL_MAX + 1) + 1));
  L.bsum = o, o += up8(4 * L.tiles);
  L.sel = o, o += up8(N);
  L.total = o;
  return L;
}

unsigned grid_for(int64_t n, int tpb = TPB, int64_t cap = 8192) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(krca::ceil_div(n, tpb), cap));
}

__device__ inline bool svc_ok(int32_t s, int32_t S) { return (uint32_t)s < (uint32_t)S; }
__device__ inline bool start_ok(int64_t s) { return s >= -START_LIM && s < START_LIM; }

// header and counts zeroed: hdr u64[HDR], cnt u32[N] (two separate parts of ws)
__global__ __launch_bounds__(TPB) void crit_zero(unsigned long long* __restrict__ hdr, uint32_t* __restrict__ cnt, int64_t N) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t < HDR) hdr[t] = 0;
  for (int64_t i = t; i < N; i += stride) cnt[i] = 0;
}

__global__ __launch_bounds__(TPB) void crit_mark(const int32_t* __restrict__ svc, const int32_t* __restrict__ parent,
                                                 const int64_t* __restrict__ start, int64_t N, int32_t S,
                                                 unsigned long long* __restrict__ hdr, int32_t* __restrict__ vp,
                                                 uint32_t* __restrict__ cnt) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  unsigned long long bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    if (!svc_ok(svc[i], S) || !start_ok(start[i])) {
      vp[i] = VP_BAD;
      ++bad;
      continue;
    }
    const int64_t p = parent[i];
    int32_t v = VP_ROOT;
    if (p >= 0 && p < N && p != i && svc_ok(svc[p], S) && start_ok(start[p])) {
      v = (int32_t)p;
      atomicAdd(cnt + p, 1u);
    }
    vp[i] = v;
  }
  if (bad) atomicAdd(hdr, bad);
}

// ---- scan -------------------------------------------------------------------------------------
__device__ inline uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t w = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v += w;
  }
  return v;
}

// exclusive prefix of v over the workgroup's NT threads (NT / 64 <= 16 waves); *total = the workgroup's sum.
// wsum: NT / 64 LDS words; two barriers, so back-to-back calls may reuse wsum.
template <int NT>
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan(v, lane);
  __syncthreads();  // the previous call's readers are done with wsum
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint32_t x = wsum[w];
    if (w < wave) before += x;
    all += x;
  }
  *total = all;
  return before + incl - v;
}

__global__ __launch_bounds__(TPB) void scan_tile_sums(const uint32_t* __restrict__ cnt, int64_t N, int64_t tiles,
                                                      uint32_t* __restrict__ bsum) {
  __shared__ uint32_t wsum[TPB / 64];
  for (int64_t b = blockIdx.x; b < tiles; b += gridDim.x) {  // block-uniform
    const int64_t i0 = b * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j)
      if (i0 + j < N) s += cnt[i0 + j];
    uint32_t total;
    block_excl_scan<TPB>(s, wsum, &total);
    if (threadIdx.x == 0) bsum[b] = total;
  }
}

__global__ __launch_bounds__(SCAN2_TPB) void scan_sums(uint32_t* __restrict__ bsum, int64_t tiles) {
  __shared__ uint32_t wsum[SCAN2_TPB / 64];
  uint32_t carry = 0;
  for (int64_t base = 0; base < tiles; base += SCAN2_TPB) {  // block-uniform
    const int64_t j = base + threadIdx.x;
    const uint32_t v = j < tiles ? bsum[j] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan<SCAN2_TPB>(v, wsum, &total);
    if (j < tiles) bsum[j] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(TPB) void scan_tiles(const uint32_t* __restrict__ cnt, int64_t N, int64_t tiles,
                                                  const uint32_t* __restrict__ bsum, uint32_t* __restrict__ off,
                                                  unsigned long long* __restrict__ hdr, uint32_t* __restrict__ heavy) {
  __shared__ uint32_t wsum[TPB / 64];
  for (int64_t b = blockIdx.x; b < tiles; b += gridDim.x) {  // block-uniform
    const int64_t i0 = b * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    uint32_t c[SCAN_PER], s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) {
      c[j] = i0 + j < N ? cnt[i0 + j] : 0u;
      s += c[j];
    }
    uint32_t total;
    uint32_t run = bsum[b] + block_excl_scan<TPB>(s, wsum, &total);
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) {
      if (i0 + j < N) {
        off[i0 + j] = run;
        // at most N / (SMALL_MAX + 1) parents hold more than SMALL_MAX of the at most N children
        if (c[j] > SMALL_MAX) heavy[atomicAdd(hdr + 1, 1ull)] = (uint32_t)(i0 + j);
      }
      run += c[j];
    }
  }
}

// ---- scatter ----------------------------------------------------------------------------------
// off[p] is the cursor of p's list: after this pass it is the list's END, its start is off[p] - cnt[p]
__global__ __launch_bounds__(TPB) void crit_scatter(const int64_t* __restrict__ start, const uint32_t* __restrict__ dur,
                                                    int64_t N, const int32_t* __restrict__ vp, uint32_t* __restrict__ off,
                                                    uint32_t* __restrict__ child, uint2* __restrict__ rel,
                                                    uint8_t* __restrict__ sel) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    sel[i] = 0;
    const int32_t p = vp[i];
    if (p < 0) continue;
    const int64_t s = start[i], e = s + (int64_t)dur[i];  // |start| <= 2^62: no overflow
    const int64_t ps = start[p], pe = ps + (int64_t)dur[p];
    const int64_t cs = s > ps ? s : ps, ce = e < pe ? e : pe;
    uint2 r = make_uint2(0u, 0u);  // an empty piece (ce <= cs) is never selected
    if (ce > cs) r = make_uint2((uint32_t)(cs - ps), (uint32_t)(ce - ps));
    const uint32_t pos = atomicAdd(off + p, 1u);  // < the number of valid children <= N
    child[pos] = (uint32_t)i;
    rel[pos] = r;
  }
}

// ---- sweep ------------------------------------------------------------------------------------
// the order of the sweep: larger end, then smaller start, then lower span index
__device__ inline bool better(uint32_t ce, uint32_t cs, uint32_t idx, uint32_t bce, uint32_t bcs, uint32_t bidx) {
  if (ce != bce) return ce > bce;
  if (cs != bcs) return cs < bcs;
  return idx < bidx;
}

__global__ __launch_bounds__(TPB) void sweep_small(const uint32_t* __restrict__ dur, int64_t N,
                                                   const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ off,
                                                   const uint32_t* __restrict__ child, const uint2* __restrict__ rel,
                                                   uint8_t* __restrict__ sel, uint32_t* __restrict__ crit_us) {
  __shared__ uint32_t bin[SMALL_MAX + 1];
  __shared__ uint16_t order[TPB];
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < N; base += stride) {  // block-uniform
    // counting sort of the workgroup's 256 parents by child count: thread t then takes the t-th
    if (threadIdx.x <= SMALL_MAX) bin[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c = 0;
    if (base + threadIdx.x < N) c = cnt[base + threadIdx.x];
    if (c > SMALL_MAX) c = 0;  // the heavy kernel's
    const uint32_t rank = atomicAdd(bin + c, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t run = 0;
      for (int k = SMALL_MAX; k >= 0; --k) {  // largest counts first
        const uint32_t n = bin[k];
        bin[k] = run;
        run += n;
      }
    }
    __syncthreads();
    order[bin[c] + rank] = (uint16_t)threadIdx.x;
    __syncthreads();
    const int64_t p = base + order[threadIdx.x];
    c = p < N ? cnt[p] : 0u;
    if (c == 0 || c > SMALL_MAX) continue;  // no barrier below
    const uint32_t beg = off[p] - c;
    const uint32_t d = dur[p];
    uint32_t cursor = d, sum = 0;
    for (;;) {  // every selection lowers the cursor: at most c rounds
      int best = -1;
      uint32_t bce = 0, bcs = 0, bidx = 0;
      for (uint32_t k = 0; k < c; ++k) {
        const uint2 r = rel[beg + k];
        if (r.y <= r.x || r.y > cursor) continue;
        if (best >= 0 && (r.y < bce || (r.y == bce && r.x > bcs))) continue;
        const uint32_t idx = child[beg + k];
        if (best < 0 || better(r.y, r.x, idx, bce, bcs, bidx)) best = (int)k, bce = r.y, bcs = r.x, bidx = idx;
      }
      if (best < 0) break;
      sel[bidx] = 1;
      sum += bce - bcs;
      cursor = bcs;
    }
    crit_us[p] = d - sum;  // the pieces are disjoint and inside [0, d]
  }
}

__global__ __launch_bounds__(TPB) void sweep_heavy(const uint32_t* __restrict__ dur, const uint32_t* __restrict__ cnt,
                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ child,
                                                   const uint2* __restrict__ rel, const unsigned long long* __restrict__ hdr,
                                                   const uint32_t* __restrict__ heavy, uint8_t* __restrict__ sel,
                                                   uint32_t* __restrict__ crit_us) {
  __shared__ uint32_t wce[TPB / 64], wcs[TPB / 64], widx[TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_heavy = (int64_t)hdr[1];
  for (int64_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {  // block-uniform
    const uint32_t p = heavy[h];
    const uint32_t c = cnt[p], beg = off[p] - c, d = dur[p];
    uint32_t cursor = d, sum = 0;
    for (;;) {  // block-uniform: every thread sees the same winner
      // ce = 0 marks "none": a selectable piece has ce > cs >= 0
      uint32_t bce = 0, bcs = 0, bidx = 0;
      for (uint32_t k = threadIdx.x; k < c; k += TPB) {
        const uint2 r = rel[beg + k];
        if (r.y <= r.x || r.y > cursor) continue;
        const uint32_t idx = child[beg + k];
        if (bce == 0 || better(r.y, r.x, idx, bce, bcs, bidx)) bce = r.y, bcs = r.x, bidx = idx;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oce = (uint32_t)__shfl_xor((int)bce, o, 64), ocs = (uint32_t)__shfl_xor((int)bcs, o, 64),
                       oidx = (uint32_t)__shfl_xor((int)bidx, o, 64);
        if (oce != 0 && (bce == 0 || better(oce, ocs, oidx, bce, bcs, bidx))) bce = oce, bcs = ocs, bidx = oidx;
      }
      __syncthreads();  // the previous round's readers are done
      if (lane == 0) wce[wave] = bce, wcs[wave] = bcs, widx[wave] = bidx;
      __syncthreads();
      bce = 0, bcs = 0, bidx = 0;
#pragma unroll
      for (int w = 0; w < TPB / 64; ++w) {
        const uint32_t oce = wce[w], ocs = wcs[w], oidx = widx[w];
        if (oce != 0 && (bce == 0 || better(oce, ocs, oidx, bce, bcs, bidx))) bce = oce, bcs = ocs, bidx = oidx;
      }
      if (bce == 0) break;
      if (threadIdx.x == 0) sel[bidx] = 1;
      sum += bce - bcs;
      cursor = bcs;
    }
    if (threadIdx.x == 0) crit_us[p] = d - sum;
  }
}

// ---- final ------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void crit_final(const uint32_t* __restrict__ dur, int64_t N, const int32_t* __restrict__ vp,
                                                  const uint32_t* __restrict__ cnt, const uint8_t* __restrict__ sel,
                                                  uint32_t* __restrict__ crit_us, uint8_t* __restrict__ path) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    const int32_t v = vp[i];
    if (v == VP_BAD) {
      crit_us[i] = 0;
      path[i] = 0;
      continue;
    }
    uint8_t bits;
    bool on = false;
    if (v == VP_ROOT) {
      bits = 4 | 2;
      on = true;
    } else {
      bits = sel[i];
      if (bits) {
        int32_t a = v;  // the k-th valid ancestor, k = 1: the link below it is selected
        for (int k = 1; k <= D_MAX; ++k) {
          const int32_t up = vp[a];  // never VP_BAD: a valid parent is not bad
          if (up == VP_ROOT) {
            on = true;
            break;
          }
          if (!sel[a]) break;
          a = up;
        }
      }
      if (on) bits |= 2;
    }
    // a span with children had dur - selected pieces written by its sweep; a leaf keeps its duration
    crit_us[i] = on ? (cnt[i] ? crit_us[i] : dur[i]) : 0u;
    path[i] = bits;
  }
}

}  // namespace

extern "C" {

int32_t krca_trace_critical_max_depth(void) { return D_MAX; }
int32_t krca_trace_critical_small_max(void) { return SMALL_MAX; }
int64_t krca_trace_critical_ws_size(int64_t N) { return layout(std::max<int64_t>(N, 0)).total; }

int krca_trace_critical(const int32_t* svc, const int32_t* parent, const int64_t* start_us, const uint32_t* dur_us,
                        int64_t N, int32_t S, uint32_t* crit_us, uint8_t* path, void* ws, void* stream) {
  KRCA_CHECK_ARG(N >= 0 && N < INT_MAX, "krca_trace_critical: N=%lld out of [0, 2^31-1)", (long long)N);
  KRCA_CHECK_ARG(S >= 0, "krca_trace_critical: S < 0");
  KRCA_CHECK_ARG(ws && ((uintptr_t)ws & 7) == 0, "krca_trace_critical: null or misaligned workspace");
  hipStream_t st = krca::as_stream(stream);
  const Layout L = layout(N);
  char* w = static_cast<char*>(ws);
  unsigned long long* hdr = reinterpret_cast<unsigned long long*>(w);
  uint2* rel = reinterpret_cast<uint2*>(w + L.rel);
  int32_t* vp = reinterpret_cast<int32_t*>(w + L.vp);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(w + L.cnt);
  uint32_t* off = reinterpret_cast<uint32_t*>(w + L.off);
  uint32_t* child = reinterpret_cast<uint32_t*>(w + L.child);
  uint32_t* heavy = reinterpret_cast<uint32_t*>(w + L.heavy);
  uint32_t* bsum = reinterpret_cast<uint32_t*>(w + L.bsum);
  uint8_t* sel = reinterpret_cast<uint8_t*>(w + L.sel);
  hipLaunchKernelGGL(crit_zero, dim3(grid_for(N)), dim3(TPB), 0, st, hdr, cnt, N);
  KRCA_LAUNCH_CHECK();
  if (N == 0) return KRCA_OK;
  KRCA_CHECK_ARG(svc && parent && start_us && dur_us && crit_us && path, "krca_trace_critical: null array");
  const unsigned g = grid_for(N), gt = grid_for(L.tiles, 1, 4096);
  hipLaunchKernelGGL(crit_mark, dim3(g), dim3(TPB), 0, st, svc, parent, start_us, N, S, hdr, vp, cnt);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_tile_sums, dim3(gt), dim3(TPB), 0, st, cnt, N, L.tiles, bsum);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_sums, dim3(1), dim3(SCAN2_TPB), 0, st, bsum, L.tiles);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_tiles, dim3(gt), dim3(TPB), 0, st, cnt, N, L.tiles, bsum, off, hdr, heavy);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(crit_scatter, dim3(g), dim3(TPB), 0, st, start_us, dur_us, N, vp, off, child, rel, sel);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(sweep_small, dim3(g), dim3(TPB), 0, st, dur_us, N, cnt, off, child, rel, sel, crit_us);
  KRCA_LAUNCH_CHECK();
  // the number of heavy parents stays on the device: a fixed grid walks the list
  hipLaunchKernelGGL(sweep_heavy, dim3(HEAVY_GRID), dim3(TPB), 0, st, dur_us, cnt, off, child, rel, hdr, heavy, sel,
                     crit_us);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(crit_final, dim3(g), dim3(TPB), 0, st, dur_us, N, vp, cnt, sel, crit_us, path);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

}  // extern "C"
