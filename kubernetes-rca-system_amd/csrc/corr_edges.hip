// Lead/lag correlation along dependency edges (krca_corr_edges / krca_corr_lead_key).
//
// Inputs: z float32 [N][T], pod-major, in krca_corr_prepare's z32 layout (nothing is standardised
// here; for c_0 = Pearson r the rows have unit variance, which is z32 times sqrt(T)); the pull-CSR as krca_rca_precede takes it (row k = the callers j of k, edges j -> k);
// L = max_lag in [0, KRCA_CORR_MAX_LAG]; tau >= 0; slack in [0, L]; an optional mask uint8 [N].
// For the edge at CSR position e, in row k with j = col[e], and each l in [-L, L]:
//   S_l = sum over t in [max(0,-l), min(T, T-l))  of  z[j][t+l] * z[k][t],     c_l = S_l / T
// (an empty overlap gives 0; for standardised rows c_0 is Pearson r and |c_l| <= 1: the biased
// cross-correlation estimator; l > 0: the caller's series follows the dependency's by l steps).
// S_l is accumulated in float32 with fused multiply-adds in a fixed order per edge (each of 16 lanes its
// steps in ascending order, then rotations by 8, 4, 2, 1 lanes; no float atomics), so two launches
// give the same bits; c_l = (float)((double)S_l / (double)T), one correctly rounded division.
// Per edge [E], fully written:  r0 = c_0;  lag (int8) = the l of the largest |S_l| (the same order as
// |c_l|), visiting 0, +1, -1, +2, -2, ... and replacing only on strictly greater (ties: the smaller
// |l|, then the positive l);  r_lag = c_lag.  A self loop, an edge with mask[j] == 0 or mask[k] == 0
// (or a column outside [0, N)) gets r0 = r_lag = 0, lag = 0 and is not classified.
// An edge is correlated when fabsf(r_lag) > tau (float32 compare of the stored value); a correlated
// edge is DEP_LEADS when lag > slack, CALLER_LEADS when lag < -slack, SYNC otherwise.
// Per caller j [N], over the rows j appears in: dep_lead, dep_sync (int32 atomic adds) and
// dep_best = max over its DEP_LEADS edges of ((int64)bits(|r_lag|) << 32) | (uint32)(0x7FFFFFFF - k)
// (64-bit atomic max; the strongest leading dependency, ties to the lower id; 0: none).
// Per callee k [N]: caller_follow (the DEP_LEADS edges of row k), caller_sync, caller_lead.
// Integer counts and an integer max: independent of the schedule.
//
// Shape: a wave takes one row k, or one 512-caller chunk of a long row.  It keeps z[k] with a zero
// halo of LT >= L steps on both sides in LDS (LT = 0, 4, 8 or 16).  Each group of 16 lanes streams the
// rows of R = 2 callers with 16-byte loads (T % 4 == 0; 4-byte loads otherwise), so a wave has 8 edges
// in flight and the next 64 steps of each are loaded under the current steps' FMAs.  A lane holding
// z[j][u .. u+3] reads the 4 + 2 LT steps of z[k] around u once for its R rows and updates its
// R x (2 LT + 1) accumulators; four DPP row rotations per accumulator sum them over the 16 lanes, and
// lane 0 of the group picks the lag, stores the edge and does the per-caller atomics.  The first
// launch walks chunk 0 of every row, stores the per-callee counts plainly and appends the further
// chunks of long rows to a list (one atomic per row); the second launch walks that list and adds its
// per-callee counts atomically.
#include <algorithm>

#include "krca_common.h"

namespace {

constexpr int TPB = 256;
constexpr int kChunk = 512;        // callers per work item (a row, or a chunk of a long row)
constexpr int kMaxLdsBytes = 65536;  // static + dynamic LDS a workgroup gets without an opt-in

struct Args {
  const float* z;
  int64_t N;
  int32_t T;
  const int64_t* row_ptr;
  const int32_t* col;
  int32_t L;
  float tau;
  int32_t slack;
  const uint8_t* mask;
  float* r0;
  int8_t* lag;
  float* r_lag;
  int32_t* dep_lead;
  int32_t* dep_sync;
  unsigned long long* dep_best;
  int32_t* caller_follow;
  int32_t* caller_sync;
  int32_t* caller_lead;
  int2* items;        // {row, chunk} of the chunks >= 1 of long rows
  uint32_t* n_items;
  int32_t lds_stride;  // floats per wave: T + 2 LT rounded up to 4
};

__device__ __forceinline__ int wave_sum(int v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// v rotated right by N lanes inside each row of 16 lanes (DPP row_ror: one VALU operand modifier)
template <int N>
__device__ __forceinline__ float row_ror(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + N, 0xF, 0xF, true));
}

// the sum over a row of 16 lanes, in a fixed order per lane (callers use lane 0 of the row)
__device__ __forceinline__ float row_sum(float v) {
  v += row_ror<8>(v);
  v += row_ror<4>(v);
  v += row_ror<2>(v);
  v += row_ror<1>(v);
  return v;
}

// x[r] = z[j[r]][c .. c + V) for the rows that are on and c < T, zeros otherwise
template <int V, int R>
__device__ __forceinline__ void load_steps(const float* __restrict__ z, int T, const int32_t (&j)[R], const bool (&on)[R],
                                           int c, float (&x)[R][V]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int v = 0; v < V; ++v) x[r][v] = 0.f;
    if (on[r] && c < T) {
      const float* zj = z + (size_t)j[r] * T + c;
      if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(zj);
        x[r][0] = q.x;
        x[r][1] = q.y;
        x[r][2] = q.z;
        x[r][3] = q.w;
      } else {
        x[r][0] = zj[0];
      }
    }
  }
}

// orders this wave's LDS writes before its later LDS reads (and the reverse) across lanes
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LT: lags held per side (>= L; the halo width), V: steps per lane and load (4: 16-byte loads, needs
// T % 4 == 0), R: caller rows in flight, LIST: walk the chunk list instead of the rows
template <int LT, int V, int R, bool LIST>
__global__ __launch_bounds__(TPB) void corr_edges_rows(const Args a) {
  extern __shared__ float4 lds_all[];
  constexpr int NL = 2 * LT + 1;
  const int lane = threadIdx.x & 63, grp = lane >> 4, sub = lane & 15;
  const int T = a.T;
  float* lds = reinterpret_cast<float*>(lds_all) + (size_t)(threadIdx.x >> 6) * a.lds_stride;  // lds[i] = z[k][i - LT]
  for (int i = lane; i < LT; i += 64) {
    lds[i] = 0.f;
    lds[LT + T + i] = 0.f;
  }
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t n_work = LIST ? (int64_t)*a.n_items : a.N;
  for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < n_work; w += n_waves) {
    int32_t k = (int32_t)w;
    int64_t chunk = 0;
    if (LIST) {
      const int2 it = a.items[w];
      k = it.x;
      chunk = it.y;
    }
    const int64_t rb = a.row_ptr[k], re = a.row_ptr[k + 1];
    const int64_t e0 = rb + chunk * kChunk, e1 = std::min<int64_t>(re, e0 + kChunk);
    if (!LIST) {
      const int64_t n_chunks = (re - rb + kChunk - 1) / kChunk;
      if (n_chunks > 1) {  // wave-uniform; the list holds at most E / kChunk items
        uint32_t off = 0;
        if (lane == 0) off = atomicAdd(a.n_items, (uint32_t)(n_chunks - 1));
        off = __shfl(off, 0, 64);
        for (int64_t c = 1 + lane; c < n_chunks; c += 64) a.items[off + c - 1] = make_int2(k, (int)c);
      }
    }
    int follow = 0, sync = 0, lead = 0;  // per lane; summed over the wave after the row
    if (e0 < e1 && a.mask && a.mask[k] == 0) {
      for (int64_t e = e0 + lane; e < e1; e += 64) {
        a.r0[e] = 0.f;
        a.r_lag[e] = 0.f;
        a.lag[e] = 0;
      }
    } else if (e0 < e1) {
      wave_sync();  // the previous row's reads are done
      const float* zk = a.z + (size_t)k * T;
      for (int t = lane * V; t < T; t += 64 * V) {
        if constexpr (V == 4)
          *reinterpret_cast<float4*>(lds + LT + t) = *reinterpret_cast<const float4*>(zk + t);
        else
          lds[LT + t] = zk[t];
      }
      wave_sync();
      for (int64_t e = e0; e < e1; e += 4 * R) {  // 16 lanes per edge: R edges per group, 4 R per wave
        int32_t j[R];
        bool on[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t ee = e + 4 * r + grp;
          j[r] = ee < e1 ? a.col[ee] : k;
          on[r] = j[r] != k && (uint32_t)j[r] < (uint64_t)a.N;
          if (on[r] && a.mask) on[r] = a.mask[j[r]] != 0;
        }
        float acc[R][NL];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int i = 0; i < NL; ++i) acc[r][i] = 0.f;
        float x[R][V], xn[R][V];
        load_steps<V, R>(a.z, T, j, on, sub * V, x);
        for (int c = sub * V; c < T; c += 16 * V) {
          load_steps<V, R>(a.z, T, j, on, c + 16 * V, xn);  // the next steps, in flight under this step's FMAs
          // win[m] = z[k][c + m - LT]; step u = c + v at lag l pairs with z[k][u - l] = win[v + LT - l]
          float win[V + 2 * LT];
          if constexpr (V == 4) {
#pragma unroll
            for (int m = 0; m < V + 2 * LT; m += 4) {
              const float4 q = *reinterpret_cast<const float4*>(lds + c + m);
              win[m] = q.x;
              win[m + 1] = q.y;
              win[m + 2] = q.z;
              win[m + 3] = q.w;
            }
          } else {
#pragma unroll
            for (int m = 0; m < V + 2 * LT; ++m) win[m] = lds[c + m];
          }
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < V; ++v) {
#pragma unroll
              for (int i = 0; i < NL; ++i)  // i = l + LT
                acc[r][i] = __builtin_fmaf(x[r][v], win[v + 2 * LT - i], acc[r][i]);
              x[r][v] = xn[r][v];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int i = 0; i < NL; ++i) acc[r][i] = row_sum(acc[r][i]);  // lane 0 of each group is used
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int64_t ee = e + 4 * r + grp;
          if (sub != 0 || ee >= e1) continue;
          // a skipped edge (self loop, masked, column out of range) kept zeros: lag 0, c = 0, never > tau
          float bs = acc[r][LT], best = fabsf(bs);
          int bl = 0;
#pragma unroll
          for (int m = 1; m <= LT; ++m) {
            if (m <= a.L) {
              const float p = acc[r][LT + m], q = acc[r][LT - m];
              if (fabsf(p) > best) {
                best = fabsf(p);
                bs = p;
                bl = m;
              }
              if (fabsf(q) > best) {
                best = fabsf(q);
                bs = q;
                bl = -m;
              }
            }
          }
          const float c0 = (float)((double)acc[r][LT] / (double)T);
          const float cl = (float)((double)bs / (double)T);
          a.r0[ee] = c0;
          a.r_lag[ee] = cl;
          a.lag[ee] = (int8_t)bl;
          if (fabsf(cl) > a.tau) {
            if (bl > a.slack) {
              ++follow;
              atomicAdd(a.dep_lead + j[r], 1);
              atomicMax(a.dep_best + j[r],
                        ((unsigned long long)__float_as_uint(fabsf(cl)) << 32) | (uint32_t)(0x7FFFFFFF - k));
            } else if (bl < -a.slack) {
              ++lead;
            } else {
              ++sync;
              atomicAdd(a.dep_sync + j[r], 1);
            }
          }
        }
      }
    }
    follow = wave_sum(follow);
    sync = wave_sum(sync);
    lead = wave_sum(lead);
    if (lane == 0) {
      if (LIST) {
        if (follow) atomicAdd(a.caller_follow + k, follow);
        if (sync) atomicAdd(a.caller_sync + k, sync);
        if (lead) atomicAdd(a.caller_lead + k, lead);
      } else {
        a.caller_follow[k] = follow;
        a.caller_sync[k] = sync;
        a.caller_lead[k] = lead;
      }
    }
  }
}

__global__ __launch_bounds__(TPB) void corr_lead_key(const int32_t* __restrict__ dep_lead,
                                                     const int32_t* __restrict__ caller_follow,
                                                     const float* __restrict__ score, int64_t N,
                                                     int64_t* __restrict__ key) {
  const int64_t stride = (int64_t)gridDim.x * TPB;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < N; i += stride) {
    int64_t kv = 0;
    const float s = score[i];
    const int32_t f = caller_follow[i];
    if (dep_lead[i] == 0 && f > 0 && s > 0.f)  // a NaN score compares false
      kv = (std::min<int64_t>(f, (1 << 20) - 1) << 32) | (int64_t)__float_as_uint(s);  // s > 0: bits order as floats
    key[i] = kv;
  }
}

template <int LT, int V, int R>
int launch(const Args& a, int wpb, hipStream_t st) {
  const size_t lds = (size_t)wpb * a.lds_stride * sizeof(float);
  const unsigned g0 = (unsigned)std::min<int64_t>(krca::ceil_div(a.N, wpb), 2048);
  hipLaunchKernelGGL((corr_edges_rows<LT, V, R, false>), dim3(g0), dim3(64 * wpb), lds, st, a);
  KRCA_LAUNCH_CHECK();
  hipLaunchKernelGGL((corr_edges_rows<LT, V, R, true>), dim3(1024), dim3(64 * wpb), lds, st, a);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

// R = 2 rows per lane group at every LT: at C4 / T = 1440, L = 8 took 26.2 ms with R = 2, 36.5 with R = 4
// (219 VGPRs) and 30.8 with R = 1; L = 0 took 19.0 ms with R = 2 and 21.4 with R = 4
template <int V>
int launch_lt(const Args& a, int lt, int wpb, hipStream_t st) {
  switch (lt) {
    case 0: return launch<0, V, 2>(a, wpb, st);
    case 4: return launch<4, V, 2>(a, wpb, st);
    case 8: return launch<8, V, 2>(a, wpb, st);
    default: return launch<16, V, 2>(a, wpb, st);
  }
}

int pick_lt(int L) { return L == 0 ? 0 : L <= 4 ? 4 : L <= 8 ? 8 : 16; }

}  // namespace

extern "C" {

// workspace: counter (256 B) | chunk list int2[E / 512 + 1]
int64_t krca_corr_edges_ws_size(int64_t N, int64_t E) {
  (void)N;
  return 8 * (std::max<int64_t>(E, 0) / kChunk + 1) + 256;
}

int krca_corr_edges(const float* z, int64_t N, int32_t T, const int64_t* row_ptr, const int32_t* col, int32_t max_lag,
                    float tau, int32_t slack, const uint8_t* mask, float* r0, int8_t* lag, float* r_lag,
                    int32_t* dep_lead, int32_t* dep_sync, int64_t* dep_best, int32_t* caller_follow,
                    int32_t* caller_sync, int32_t* caller_lead, void* ws, void* stream) {
  KRCA_CHECK_ARG(N > 0 && N < INT32_MAX && T >= 1, "krca_corr_edges: bad sizes N=%lld T=%d", (long long)N, T);
  KRCA_CHECK_ARG(max_lag >= 0 && max_lag <= KRCA_CORR_MAX_LAG && slack >= 0 && slack <= max_lag && tau >= 0.f,
                 "krca_corr_edges: need 0 <= slack <= max_lag <= %d and tau >= 0 (max_lag=%d slack=%d tau=%g)",
                 KRCA_CORR_MAX_LAG, max_lag, slack, (double)tau);
  KRCA_CHECK_ARG(z && row_ptr && col && r0 && lag && r_lag && dep_lead && dep_sync && dep_best && caller_follow &&
                     caller_sync && caller_lead && ws,
                 "krca_corr_edges: null pointer");
  KRCA_CHECK_ARG(((uintptr_t)ws & 7) == 0, "krca_corr_edges: workspace must be 8-byte aligned");
  const int lt = pick_lt(max_lag);
  const bool vec = T % 4 == 0 && ((uintptr_t)z & 15) == 0;
  const int64_t stride = ((int64_t)T + 2 * lt + 3) & ~int64_t(3);
  KRCA_CHECK_ARG(stride * 4 <= kMaxLdsBytes, "krca_corr_edges: T=%d does not fit a wave's LDS row (T + 2 L <= %d)", T,
                 kMaxLdsBytes / 4);
  const int wpb = 4 * stride * 4 <= kMaxLdsBytes ? 4 : 1;
  hipStream_t st = krca::as_stream(stream);
  Args a{z, N, T, row_ptr, col, max_lag, tau, slack, mask, r0, lag, r_lag, dep_lead, dep_sync,
         reinterpret_cast<unsigned long long*>(dep_best), caller_follow, caller_sync, caller_lead,
         reinterpret_cast<int2*>(reinterpret_cast<char*>(ws) + 256), reinterpret_cast<uint32_t*>(ws), (int32_t)stride};
  KRCA_HIP(hipMemsetAsync(a.n_items, 0, sizeof(uint32_t), st));
  KRCA_HIP(hipMemsetAsync(dep_lead, 0, N * sizeof(int32_t), st));
  KRCA_HIP(hipMemsetAsync(dep_sync, 0, N * sizeof(int32_t), st));
  KRCA_HIP(hipMemsetAsync(dep_best, 0, N * sizeof(int64_t), st));
  return vec ? launch_lt<4>(a, lt, wpb, st) : launch_lt<1>(a, lt, wpb, st);
}

int krca_corr_lead_key(const int32_t* dep_lead, const int32_t* caller_follow, const float* score, int64_t N,
                       int64_t* key, void* stream) {
  KRCA_CHECK_ARG(N > 0, "krca_corr_lead_key: bad size");
  KRCA_CHECK_ARG(dep_lead && caller_follow && score && key, "krca_corr_lead_key: null pointer");
  const unsigned g = (unsigned)std::min<int64_t>(krca::ceil_div(N, TPB), 2048);
  hipLaunchKernelGGL(corr_lead_key, dim3(g), dim3(TPB), 0, krca::as_stream(stream), dep_lead, caller_follow, score, N,
                     key);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

}  // extern "C"
