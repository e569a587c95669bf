// Peer deviation score (include/krca.h krca_peer_score): per group of pods (CSR grp_ptr / member) and
// metric, the lower median and MAD of a per-pod statistic v[P][M] over the group's valid members, and
// each member's robust deviation from them; per pod the largest deviation and its metric.
//
// Design (MI355X).  Group sizes are heavily skewed (replica sets of 3 .. a DaemonSet or an "all nodes"
// group of tens of thousands), so the selection has three homes for its keys, one bisection:
//   n <= 64        peer_small: one wave per group, one lane per member, the key in a register; the count
//                  of a bisection step is one ballot + popcount (scalar unit), no LDS, no per-thread array.
//                  The lane then holds its pod's whole row and writes peer / score / lead itself.
//   64 < n <= cap  peer_stat<true>: the valid members' keys of one (group, metric) in an LDS tile
//   n > cap        peer_stat<false>: the same keys compacted into the workspace, [metric][member] inside
//                  the span M * grp_ptr[g] .. M * grp_ptr[g + 1] (spans of different groups are disjoint,
//                  so nothing is allocated on the device); every pass is a coalesced sweep.
// peer_small visits every group and appends those above 64 to one of two lists in the workspace (order
// free: no output depends on it).  peer_stat drains a list with a fixed grid that strides over
// (entry, metric) items -- the list length is read from the workspace, never by the host -- and writes
// grp_med / grp_mad only.  One workgroup per (group, metric), not per group, for both lists: the M
// selections of a group are independent, the groups above 64 are few (a handful of DaemonSets), and M
// workgroups per group keep more CUs busy; the price is M strided gathers of rows that stay in L2.
// peer_apply then takes one workgroup per listed group, one thread per member at a time, and writes what
// peer_small writes for its groups.  Kernel boundaries order the phases; no flag, fence or spin.
// Pods in no group: peer_init stores lead = -2 for every pod (P bytes), every member's lead is
// overwritten with a value in [-1, 63], and peer_finish writes the defaults where -2 is still there --
// a defaults pass over peer[P][M] in front would cost 4*P*M more bytes.
// cap = 4096 keys = 16 KB of LDS per 256-thread workgroup: eight workgroups per CU fit the 160 KB, so
// the wave limit (32 per CU), not the tile, bounds the occupancy.
// The > cap path is correct at any size and not tuned: 64 sweeps of n keys by one workgroup.
#include <cmath>

#include "krca_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPeerSmall = 64;
constexpr int kPeerCap = 4096;
constexpr int kTpb = 256;
constexpr int kWaves = kTpb / 64;
constexpr int kStatGridLds = 1024, kStatGridWs = 256, kApplyGrid = 1024;
constexpr int64_t kHdrBytes = 256;

__host__ __device__ inline int64_t list_bytes(int64_t G) { return (G * 8 + 255) / 256 * 256; }

// total order of include/krca.h (krca_shift_score's): -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN
__device__ __forceinline__ uint32_t to_key(float x) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, x);
  return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}
__device__ __forceinline__ float from_key(uint32_t key) {
  return __builtin_bit_cast(float, (key & 0x80000000u) ? key & 0x7fffffffu : ~key);
}

__device__ __forceinline__ float peer_value(float x, float med, float mad, float min_scale) {
  double den = 1.4826 * (double)mad;
  if (!(den > (double)min_scale)) den = (double)min_scale;
  return den > 0.0 ? (float)(((double)x - (double)med) / den) : 0.0f;
}

// group g's member span, clamped into [0, n_member] so a malformed grp_ptr reads nothing out of bounds
__device__ __forceinline__ void group_span(const int64_t* __restrict__ grp_ptr, int64_t g, int64_t n_member, int64_t& lo,
                                           int64_t& n) {
  int64_t a = grp_ptr[g], b = grp_ptr[g + 1];
  a = a < 0 ? 0 : (a > n_member ? n_member : a);
  b = b < a ? a : (b > n_member ? n_member : b);
  lo = a;
  n = b - a;
}

template <int CH>
__device__ __forceinline__ void load_chunk(float (&x)[CH], const float* p, bool vec) {
  if constexpr (CH >= 4) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < CH; j += 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + j);
        x[j] = q.x, x[j + 1] = q.y, x[j + 2] = q.z, x[j + 3] = q.w;
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < CH; ++j) x[j] = p[j];
}

template <int CH>
__device__ __forceinline__ void store_chunk(float* p, const float (&x)[CH], bool vec) {
  if constexpr (CH >= 4) {
    if (vec) {
#pragma unroll
      for (int j = 0; j < CH; j += 4) *reinterpret_cast<float4*>(p + j) = make_float4(x[j], x[j + 1], x[j + 2], x[j + 3]);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < CH; ++j) p[j] = x[j];
}

__global__ __launch_bounds__(kTpb) void peer_init_kernel(int64_t P, int8_t* __restrict__ lead,
                                                         unsigned long long* __restrict__ hdr) {
  const int64_t p = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (p < 2) hdr[p] = 0;  // the two list lengths
  if (p < P) lead[p] = (int8_t)-2;
}

__global__ __launch_bounds__(kTpb) void peer_finish_kernel(int64_t P, int M, float* __restrict__ peer,
                                                           float* __restrict__ score, int8_t* __restrict__ lead) {
  const int64_t p = (int64_t)blockIdx.x * kTpb + threadIdx.x;
  if (p >= P || lead[p] != (int8_t)-2) return;
  for (int m = 0; m < M; ++m) peer[p * M + m] = 0.0f;
  score[p] = 0.0f;
  lead[p] = (int8_t)-1;
}

// the key of 0-based rank r among the valid lanes' keys: the largest c with count(key < c) <= r
__device__ __forceinline__ uint32_t wave_select(uint32_t key, bool valid, int r) {
  uint32_t c = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = c | (1u << bit);
    if (__popcll(__ballot(valid && key < cand)) <= r) c = cand;
  }
  return c;
}

template <int CH>  // CH = min(M, 8): metrics per register chunk
__global__ __launch_bounds__(kTpb) void peer_small_kernel(
    const float* __restrict__ v, int64_t P, int M, const int64_t* __restrict__ grp_ptr,
    const int32_t* __restrict__ member, int64_t G, int64_t n_member, int min_members, float min_scale, float out_thr,
    float* __restrict__ peer, float* __restrict__ score, int8_t* __restrict__ lead, float* __restrict__ grp_med,
    float* __restrict__ grp_mad, int32_t* __restrict__ grp_out, unsigned long long* __restrict__ hdr,
    int64_t* __restrict__ list_lds, int64_t* __restrict__ list_ws, int vec) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (g >= G) return;  // wave-uniform
  int64_t lo, n_g;
  group_span(grp_ptr, g, n_member, lo, n_g);
  if (n_g > kPeerSmall) {
    if (lane == 0) {
      if (n_g <= kPeerCap)
        list_lds[atomicAdd(&hdr[0], 1ull)] = g;
      else
        list_ws[atomicAdd(&hdr[1], 1ull)] = g;
    }
    return;
  }
  int64_t id = -1;
  if (lane < n_g) id = member[lo + lane];
  const bool valid = id >= 0 && id < P;
  const int n = __popcll(__ballot(valid));
  const bool enough = n >= min_members;
  const int r = (n - 1) >> 1;
  const int64_t row = (valid ? id : 0) * M;
  float best = 0.0f;
  int bm = 0;
  for (int m0 = 0; m0 < M; m0 += CH) {
    float x[CH], o[CH];
    load_chunk<CH>(x, v + row + m0, vec);
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      float med = 0.0f, mad = 0.0f;
      if (n > 0) {
        med = from_key(wave_select(to_key(x[j]), valid, r));
        mad = from_key(wave_select(to_key(fabsf(x[j] - med)), valid, r));
      }
      const float pr = enough ? peer_value(x[j], med, mad, min_scale) : 0.0f;
      const float a = pr != pr ? 0.0f : fabsf(pr);
      if (a > best) best = a, bm = m0 + j;
      const int cnt = __popcll(__ballot(valid && fabsf(pr) > out_thr));
      if (lane == 0) {
        grp_med[g * M + m0 + j] = med;
        grp_mad[g * M + m0 + j] = mad;
        grp_out[g * M + m0 + j] = cnt;
      }
      o[j] = pr;
    }
    if (valid) store_chunk<CH>(peer + row + m0, o, vec);
  }
  if (valid) {
    score[id] = best;
    lead[id] = best > 0.0f ? (int8_t)bm : (int8_t)-1;
  }
}

// the key of rank r among keys[0 .. n), all waves of the workgroup; one barrier per bit (the partial
// sums alternate between two slots, so a wave that runs ahead writes the slot nobody reads)
__device__ __forceinline__ uint32_t block_select(const uint32_t* keys, int64_t n, int64_t r, long long (*part)[kWaves]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t c = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = c | (1u << bit);
    long long cnt = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kTpb) {
      const int64_t i = i0 + tid;
      cnt += __popcll(__ballot(i < n && keys[i] < cand));
    }
    if (lane == 0) part[bit & 1][wave] = cnt;
    __syncthreads();
    long long tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) tot += part[bit & 1][w];
    if (tot <= r) c = cand;
  }
  return c;
}

// median and MAD of metric m over the valid members mem[0 .. n_g); keys: room for n_g words
__device__ __forceinline__ void stat_item(uint32_t* keys, const float* __restrict__ v, int64_t P, int M, int m,
                                          const int32_t* __restrict__ mem, int64_t n_g, unsigned long long* s_cnt,
                                          long long (*part)[kWaves], float* out_med, float* out_mad) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) *s_cnt = 0;
  __syncthreads();
  for (int64_t i0 = 0; i0 < n_g; i0 += kTpb) {  // gather + compact (the order of a multiset is free)
    const int64_t i = i0 + tid;
    int64_t id = -1;
    if (i < n_g) id = mem[i];
    const bool valid = id >= 0 && id < P;
    const uint32_t key = valid ? to_key(v[id * M + m]) : 0u;
    const unsigned long long mask = __ballot(valid);
    unsigned long long base = 0;
    if (lane == 0 && mask) base = atomicAdd(s_cnt, (unsigned long long)__popcll(mask));
    base = __shfl(base, 0, 64);
    if (valid) keys[base + __popcll(mask & ((1ull << lane) - 1ull))] = key;
  }
  __syncthreads();
  const int64_t n = (int64_t)*s_cnt;
  float med = 0.0f, mad = 0.0f;
  if (n > 0) {  // workgroup-uniform
    med = from_key(block_select(keys, n, (n - 1) >> 1, part));
    for (int64_t i = tid; i < n; i += kTpb) keys[i] = to_key(fabsf(from_key(keys[i]) - med));
    __syncthreads();
    mad = from_key(block_select(keys, n, (n - 1) >> 1, part));
  }
  if (tid == 0) {
    *out_med = med;
    *out_mad = mad;
  }
  __syncthreads();  // the next item reuses s_cnt, part and the tile
}

template <bool kLds>
__global__ __launch_bounds__(kTpb) void peer_stat_kernel(const float* __restrict__ v, int64_t P, int M, int log_m,
                                                         const int64_t* __restrict__ grp_ptr,
                                                         const int32_t* __restrict__ member, int64_t n_member,
                                                         const unsigned long long* __restrict__ hdr,
                                                         const int64_t* __restrict__ list, uint32_t* __restrict__ ws_keys,
                                                         float* __restrict__ grp_med, float* __restrict__ grp_mad) {
  __shared__ uint32_t tile[kLds ? kPeerCap : 1];
  __shared__ unsigned long long s_cnt;
  __shared__ long long part[2][kWaves];
  const int64_t items = (int64_t)hdr[kLds ? 0 : 1] << log_m;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t g = list[w >> log_m];
    const int m = (int)(w & (M - 1));
    int64_t lo, n_g;
    group_span(grp_ptr, g, n_member, lo, n_g);
    if constexpr (kLds)
      stat_item(tile, v, P, M, m, member + lo, n_g, &s_cnt, part, grp_med + g * M + m, grp_mad + g * M + m);
    else
      stat_item(ws_keys + lo * M + (int64_t)m * n_g, v, P, M, m, member + lo, n_g, &s_cnt, part, grp_med + g * M + m,
                grp_mad + g * M + m);
  }
}

// peer / score / lead of the listed groups' members and grp_out, from the grp_med / grp_mad peer_stat wrote
template <int CH>
__global__ __launch_bounds__(kTpb) void peer_apply_kernel(
    const float* __restrict__ v, int64_t P, int M, const int64_t* __restrict__ grp_ptr,
    const int32_t* __restrict__ member, int64_t n_member, int min_members, float min_scale, float out_thr,
    float* __restrict__ peer, float* __restrict__ score, int8_t* __restrict__ lead, const float* __restrict__ grp_med,
    const float* __restrict__ grp_mad, int32_t* __restrict__ grp_out, const unsigned long long* __restrict__ hdr,
    const int64_t* __restrict__ list_lds, const int64_t* __restrict__ list_ws, int vec) {
  __shared__ float s_med[64], s_mad[64];
  __shared__ int s_out[64];
  __shared__ unsigned long long s_n;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t n_lds = (int64_t)hdr[0], n_all = n_lds + (int64_t)hdr[1];
  for (int64_t e = blockIdx.x; e < n_all; e += gridDim.x) {
    const int64_t g = e < n_lds ? list_lds[e] : list_ws[e - n_lds];
    int64_t lo, n_g;
    group_span(grp_ptr, g, n_member, lo, n_g);
    const int32_t* mem = member + lo;
    if (tid < M) {
      s_med[tid] = grp_med[g * M + tid];
      s_mad[tid] = grp_mad[g * M + tid];
      s_out[tid] = 0;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    long long c = 0;
    for (int64_t i0 = 0; i0 < n_g; i0 += kTpb) {
      const int64_t i = i0 + tid;
      int64_t id = -1;
      if (i < n_g) id = mem[i];
      c += __popcll(__ballot(id >= 0 && id < P));
    }
    if (lane == 0 && c) atomicAdd(&s_n, (unsigned long long)c);
    __syncthreads();
    const bool enough = (int64_t)s_n >= (int64_t)min_members;
    for (int64_t i0 = 0; i0 < n_g; i0 += kTpb) {
      const int64_t i = i0 + tid;
      int64_t id = -1;
      if (i < n_g) id = mem[i];
      const bool valid = id >= 0 && id < P;
      const int64_t row = (valid ? id : 0) * M;
      float best = 0.0f;
      int bm = 0;
      for (int m0 = 0; m0 < M; m0 += CH) {
        float x[CH], o[CH];
        load_chunk<CH>(x, v + row + m0, vec);
#pragma unroll
        for (int j = 0; j < CH; ++j) {
          const float pr = enough ? peer_value(x[j], s_med[m0 + j], s_mad[m0 + j], min_scale) : 0.0f;
          const float a = pr != pr ? 0.0f : fabsf(pr);
          if (a > best) best = a, bm = m0 + j;
          const int cnt = __popcll(__ballot(valid && fabsf(pr) > out_thr));
          if (lane == 0 && cnt) atomicAdd(&s_out[m0 + j], cnt);
          o[j] = pr;
        }
        if (valid) store_chunk<CH>(peer + row + m0, o, vec);
      }
      if (valid) {
        score[id] = best;
        lead[id] = best > 0.0f ? (int8_t)bm : (int8_t)-1;
      }
    }
    __syncthreads();
    if (tid < M) grp_out[g * M + tid] = s_out[tid];
    __syncthreads();  // the next group rewrites the shared words
  }
}

template <int CH>
void launch_groups(hipStream_t st, const float* v, int64_t P, int M, const int64_t* grp_ptr, const int32_t* member,
                   int64_t G, int64_t n_member, int min_members, float min_scale, float out_thr, float* peer,
                   float* score, int8_t* lead, float* grp_med, float* grp_mad, int32_t* grp_out, unsigned long long* hdr,
                   int64_t* list_lds, int64_t* list_ws, uint32_t* ws_keys, int vec) {
  int log_m = 0;
  while ((1 << log_m) < M) ++log_m;
  hipLaunchKernelGGL(peer_small_kernel<CH>, dim3((unsigned)krca::ceil_div(G, kWaves)), dim3(kTpb), 0, st, v, P, M,
                     grp_ptr, member, G, n_member, min_members, min_scale, out_thr, peer, score, lead, grp_med, grp_mad,
                     grp_out, hdr, list_lds, list_ws, vec);
  hipLaunchKernelGGL(peer_stat_kernel<true>, dim3(kStatGridLds), dim3(kTpb), 0, st, v, P, M, log_m, grp_ptr, member,
                     n_member, hdr, list_lds, ws_keys, grp_med, grp_mad);
  hipLaunchKernelGGL(peer_stat_kernel<false>, dim3(kStatGridWs), dim3(kTpb), 0, st, v, P, M, log_m, grp_ptr, member,
                     n_member, hdr, list_ws, ws_keys, grp_med, grp_mad);
  hipLaunchKernelGGL(peer_apply_kernel<CH>, dim3(kApplyGrid), dim3(kTpb), 0, st, v, P, M, grp_ptr, member, n_member,
                     min_members, min_scale, out_thr, peer, score, lead, grp_med, grp_mad, grp_out, hdr, list_lds,
                     list_ws, vec);
}

}  // namespace

extern "C" {

int32_t krca_peer_small_max(void) { return kPeerSmall; }
int32_t krca_peer_lds_cap(void) { return kPeerCap; }

int64_t krca_peer_ws_size(int64_t P, int32_t M, int64_t G, int64_t n_member) {
  (void)P;
  if (G < 0) G = 0;
  if (n_member < 0) n_member = 0;
  if (M < 1) M = 1;
  return kHdrBytes + 2 * list_bytes(G) + n_member * (int64_t)M * 4;
}

int krca_peer_score(const float* v, int64_t P, int32_t M, const int64_t* grp_ptr, const int32_t* member, int64_t G,
                    int64_t n_member, int32_t min_members, float min_scale, float out_thr, float* peer, float* score,
                    int8_t* lead, float* grp_med, float* grp_mad, int32_t* grp_out, void* ws, void* stream) {
  KRCA_CHECK_ARG(P >= 0 && G >= 0 && n_member >= 0, "krca_peer_score: bad sizes P=%lld G=%lld n_member=%lld",
                 (long long)P, (long long)G, (long long)n_member);
  KRCA_CHECK_ARG(M >= 1 && M <= 64 && (M & (M - 1)) == 0, "krca_peer_score: M=%d must be a power of two <= 64", M);
  KRCA_CHECK_ARG(min_members >= 1, "krca_peer_score: min_members=%d must be >= 1", min_members);
  KRCA_CHECK_ARG(std::isfinite(min_scale) && min_scale >= 0.f, "krca_peer_score: min_scale must be finite and >= 0");
  KRCA_CHECK_ARG(std::isfinite(out_thr) && out_thr >= 0.f, "krca_peer_score: out_thr must be finite and >= 0");
  KRCA_CHECK_ARG(P * (int64_t)M < (int64_t(1) << 32), "krca_peer_score: P*M must be < 2^32");
  KRCA_CHECK_ARG(G < (int64_t(1) << 32), "krca_peer_score: G must be < 2^32");
  if (P == 0) return KRCA_OK;
  KRCA_CHECK_ARG(v && peer && score && lead && ws, "krca_peer_score: null pointer");
  KRCA_CHECK_ARG(G == 0 || (grp_ptr && grp_med && grp_mad && grp_out), "krca_peer_score: null group pointer");
  KRCA_CHECK_ARG(n_member == 0 || member, "krca_peer_score: null member pointer");
  hipStream_t st = krca::as_stream(stream);
  char* w = static_cast<char*>(ws);
  unsigned long long* hdr = reinterpret_cast<unsigned long long*>(w);
  int64_t* list_lds = reinterpret_cast<int64_t*>(w + kHdrBytes);
  int64_t* list_ws = reinterpret_cast<int64_t*>(w + kHdrBytes + list_bytes(G));
  uint32_t* ws_keys = reinterpret_cast<uint32_t*>(w + kHdrBytes + 2 * list_bytes(G));
  const dim3 pods((unsigned)krca::ceil_div(P, kTpb));
  hipLaunchKernelGGL(peer_init_kernel, pods, dim3(kTpb), 0, st, P, lead, hdr);
  if (G > 0) {
    // rows as float4 when both row arrays are 16-byte aligned (M >= 4: every row then is)
    const int vec = M >= 4 && ((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(peer)) & 15) == 0;
#define KRCA_PEER_LAUNCH(CH)                                                                                          \
  launch_groups<CH>(st, v, P, M, grp_ptr, member, G, n_member, min_members, min_scale, out_thr, peer, score, lead,   \
                    grp_med, grp_mad, grp_out, hdr, list_lds, list_ws, ws_keys, vec)
    if (M >= 8)
      KRCA_PEER_LAUNCH(8);
    else if (M == 4)
      KRCA_PEER_LAUNCH(4);
    else if (M == 2)
      KRCA_PEER_LAUNCH(2);
    else
      KRCA_PEER_LAUNCH(1);
#undef KRCA_PEER_LAUNCH
  }
  hipLaunchKernelGGL(peer_finish_kernel, pods, dim3(kTpb), 0, st, P, M, peer, score, lead);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

}  // extern "C"
