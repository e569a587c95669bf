// Level-shift score (include/krca.h krca_shift_score): per series, the lower median of the last R
// samples against the lower median and MAD of a baseline window of B samples that ends R + G steps
// before the end of the time-major [T][P][M] tensor the scorer reads.
//
// Design (MI355X): one lane per series s = p*M + m, one wave per workgroup.  A row of a window is
// 64 consecutive floats per wave (256 B, coalesced, non-temporal: read once) and all rows of a
// window are independent loads.  The samples go, as order-preserving unsigned keys, into a per-wave
// LDS column tile [max(B, R)][64]: lane l owns word t*64 + l, so every tile access of a wave is 64
// consecutive words (conflict-free) and no lane reads another lane's words (no barrier anywhere).
// Selection is a 32-step bitwise bisection over the key space -- at each bit, count the keys below
// the candidate -- which needs no per-thread array (runtime-indexed arrays would go to scratch) and
// serves any n <= 256 with the same code.  It runs three times over the tile: the baseline's
// median, then the distances |x - median| written over the baseline in place, then the recent
// rows.  Cost per series: 32 * (2B + R) key reads and compares; the call is bound by that (the LDS
// round trip at the few waves per CU the tile leaves: DESIGN.md §3.19), not by the (B + R) * 4
// bytes it reads from HBM.
// The pod reduction (max |shift| and its lowest metric) is wave shuffles inside the pod's aligned M lanes.
#include <cmath>

#include "krca_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kShiftMaxBaseline = 256;
constexpr int kShiftMaxRecent = 64;

// total order of include/krca.h: -NaN < -Inf < ... < -0 < +0 < ... < +Inf < +NaN, as unsigned keys
__device__ __forceinline__ uint32_t to_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ uint32_t from_key(uint32_t key) { return (key & 0x80000000u) ? key & 0x7fffffffu : ~key; }

// rows [t0, t0 + n) of the lane's series -> keys in the lane's tile column, kLoadBatch independent
// loads in flight per lane.  Every load is unconditional: a lane past the last series reads series 0
// (xs) and the tail of the last batch re-reads row n - 1, so no branch sits between the loads.
constexpr int kLoadBatch = 16;
__device__ __forceinline__ void load_keys(uint32_t* col, const float* __restrict__ xs, int64_t S, int t0, int n) {
  const float* p = xs + (int64_t)t0 * S;
  for (int t = 0; t < n; t += kLoadBatch) {
    uint32_t b[kLoadBatch];
#pragma unroll
    for (int j = 0; j < kLoadBatch; ++j) {
      const int tt = t + j < n ? t + j : n - 1;
      b[j] = __builtin_bit_cast(uint32_t, __builtin_nontemporal_load(p + (int64_t)tt * S));
    }
#pragma unroll
    for (int j = 0; j < kLoadBatch; ++j)
      if (t + j < n) col[(t + j) * 64] = to_key(b[j]);
  }
}

// the key of 0-based rank r among the n keys of the lane's column: the largest v with
// count(key < v) <= r, built bit by bit from the top
__device__ __forceinline__ uint32_t select_key(const uint32_t* col, int n, int r) {
  uint32_t v = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = v | (1u << bit);
    int c0 = 0, c1 = 0;
    int t = 0;
#pragma unroll 8
    for (; t + 1 < n; t += 2) {
      c0 += col[t * 64] < cand ? 1 : 0;
      c1 += col[(t + 1) * 64] < cand ? 1 : 0;
    }
    if (t < n) c0 += col[t * 64] < cand ? 1 : 0;
    if (c0 + c1 <= r) v = cand;
  }
  return v;
}

__global__ __launch_bounds__(64) void shift_score_kernel(const float* __restrict__ x, int64_t S, int M, int T, int B,
                                                         int R, int G, float min_scale, float* __restrict__ shift,
                                                         float* __restrict__ base_med, float* __restrict__ base_mad,
                                                         float* __restrict__ recent_med, float* __restrict__ score,
                                                         int8_t* __restrict__ lead) {
  extern __shared__ uint32_t tile[];  // [max(B, R)][64]
  const int lane = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * 64 + lane;
  const bool active = s < S;
  const float* xs = x + (active ? s : 0);
  uint32_t* col = tile + lane;

  load_keys(col, xs, S, T - R - G - B, B);
  const uint32_t med_bits = from_key(select_key(col, B, (B - 1) >> 1));
  const float med = __builtin_bit_cast(float, med_bits);
#pragma unroll 8
  for (int t = 0; t < B; ++t) {  // the distances replace the samples (the same multiset in any order)
    const float v = __builtin_bit_cast(float, from_key(col[t * 64]));
    col[t * 64] = to_key(__builtin_bit_cast(uint32_t, fabsf(v - med)));
  }
  const float mad = __builtin_bit_cast(float, from_key(select_key(col, B, (B - 1) >> 1)));
  load_keys(col, xs, S, T - R, R);
  const float rmed = __builtin_bit_cast(float, from_key(select_key(col, R, (R - 1) >> 1)));

  double den = 1.4826 * (double)mad;
  if (!(den > (double)min_scale)) den = (double)min_scale;
  const float sh = den > 0.0 ? (float)(((double)rmed - (double)med) / den) : 0.0f;

  // pod combine over the pod's M wave-aligned lanes: max |shift| skipping NaN, lowest m on ties
  const int m = lane & (M - 1);
  float a = sh != sh ? 0.f : fabsf(sh);
  int am = m;
  for (int off = 1; off < M; off <<= 1) {
    const float oa = __shfl_xor(a, off, 64);
    const int om = __shfl_xor(am, off, 64);
    if (oa > a || (oa == a && om < am)) {
      a = oa;
      am = om;
    }
  }
  if (!active) return;
  shift[s] = sh;
  base_med[s] = med;
  base_mad[s] = mad;
  recent_med[s] = rmed;
  if (m == 0) {
    const int64_t p = s / M;
    score[p] = a;
    lead[p] = a > 0.f ? (int8_t)am : (int8_t)-1;
  }
}

}  // namespace

extern "C" {

int32_t krca_shift_max_baseline(void) { return kShiftMaxBaseline; }
int32_t krca_shift_max_recent(void) { return kShiftMaxRecent; }

int krca_shift_score(const float* x, int64_t P, int32_t M, int32_t T, int32_t B, int32_t R, int32_t G, float min_scale,
                     float* shift, float* base_med, float* base_mad, float* recent_med, float* score, int8_t* lead,
                     void* stream) {
  KRCA_CHECK_ARG(P >= 0 && T >= 0, "krca_shift_score: bad sizes P=%lld T=%d", (long long)P, T);
  KRCA_CHECK_ARG(M >= 1 && M <= 64 && (M & (M - 1)) == 0, "krca_shift_score: M=%d must be a power of two <= 64", M);
  KRCA_CHECK_ARG(B >= 2 && B <= kShiftMaxBaseline, "krca_shift_score: baseline B=%d must be in [2, %d]", B,
                 kShiftMaxBaseline);
  KRCA_CHECK_ARG(R >= 1 && R <= kShiftMaxRecent, "krca_shift_score: recent R=%d must be in [1, %d]", R,
                 kShiftMaxRecent);
  KRCA_CHECK_ARG(G >= 0, "krca_shift_score: guard G=%d must be >= 0", G);
  KRCA_CHECK_ARG((int64_t)B + G + R <= (int64_t)T, "krca_shift_score: B + G + R = %lld exceeds T=%d",
                 (long long)B + G + R, T);
  KRCA_CHECK_ARG(std::isfinite(min_scale) && min_scale >= 0.f, "krca_shift_score: min_scale must be finite and >= 0");
  if (P == 0) return KRCA_OK;
  KRCA_CHECK_ARG(x && shift && base_med && base_mad && recent_med && score && lead, "krca_shift_score: null pointer");
  const int64_t S = P * (int64_t)M;
  KRCA_CHECK_ARG(S < (int64_t(1) << 32), "krca_shift_score: P*M must be < 2^32");
  const int rows = B > R ? B : R;
  hipLaunchKernelGGL(shift_score_kernel, dim3((unsigned)krca::ceil_div(S, 64)), dim3(64), (size_t)rows * 64 * 4,
                     krca::as_stream(stream), x, S, M, T, B, R, G, min_scale, shift, base_med, base_mad, recent_med,
                     score, lead);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

}  // extern "C"
