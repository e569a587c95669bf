// Per-pod scoring kernels.
//
//  krca_usage_flags    — the instantaneous CPU / memory thresholds of
//                        ref:agents/metrics_agent.py:88-114 and :135-161 (x > 80 strict, high if > 90).
//  krca_rolling_score  — rolling-window z-scores over a time-major [T][P][M] float32 tensor.
//  krca_rolling_timeline — the same pass, also keeping WHEN each series exceeded: episodes of
//                        exceedances in the exceed branch, combined per pod in the epilogue.
//  krca_stream_score / krca_stream_timeline — the two carried forward over a stream, the state in HBM.
//
// Design (MI355X): HBM-streaming, one lane per series s = p*M + m.  At every time step a wave
// reads 64 consecutive floats (256 B, fully coalesced) and the trailing window of W samples
// lives in registers (a ring indexed by the compile-time position inside an unrolled block: W
// entries, or W + D with D rows of prefetch in the pipelined kernel, score_walk.h), so each input
// byte crosses HBM exactly once: 4*P*M*T bytes per call.  The
// window statistics are float64 sliding sums updated in a FIXED order, so the integer outputs
// (n_exceed, flags) are bit-identical to the C restatement in oracle/krca_oracle.c; the
// threshold test is |z| > thr  <=>  A^2 > thr^2*B (A = W*x - s1, B = W*s2 - s1^2), with no
// division or square root; all products that feed a decision are explicit fma()s.
// Pod-level reductions (max |z|, sum of exceedances, flag OR) are wave shuffles inside the
// aligned M-lane group of the pod.
#include "krca_common.h"
#include "score_walk.h"

#pragma clang fp contract(off)

namespace {

// the step arithmetic and the pipelined kernel's per-series walk (host and device code)
using krca_walk::kVarEps;
using krca_walk::prefetch_rows;
using krca_walk::score_walk;
using krca_walk::step;
using krca_walk::StepState;

__global__ __launch_bounds__(256) void usage_flags_kernel(const float2* __restrict__ usage, int64_t P,
                                                          uint8_t* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    const float2 u = usage[p];
    flags[p] = (u.x > 80.f ? KRCA_F_CPU80 : 0u) | (u.x > 90.f ? KRCA_F_CPU90 : 0u) |
               (u.y > 80.f ? KRCA_F_MEM80 : 0u) | (u.y > 90.f ? KRCA_F_MEM90 : 0u);
  }
}

// Episode policies of krca_walk::step().  NoEpisodes: the scorer, nothing tracked.
struct NoEpisodes {
  static constexpr bool kTrack = false;
  struct Args {};
  __device__ __forceinline__ explicit NoEpisodes(Args) {}
};

struct TimelineOut {
  int32_t* onset;
  int32_t* last;
  int32_t* count;
  float* peak;
  int8_t* lead;
  uint8_t* n_metrics;
};

// Episode state of one series (krca_rolling_timeline; semantics in include/krca.h): the open
// episode (c_*) and the kept one (k_*) = the sustained episode (cnt >= min_count) of the largest
// peak so far, the later one on equal peaks.  c_cnt == 0: none open; k_cnt == 0: none kept.
struct Episodes {
  static constexpr bool kTrack = true;
  struct Args {
    int gap, min_count;
    TimelineOut out;
  };
  int gap, min_count;
  int c_on, c_last, c_cnt;
  float c_peak;
  int k_on, k_last, k_cnt;
  float k_peak;
  __device__ __forceinline__ explicit Episodes(const Args& a)
      : gap(a.gap), min_count(a.min_count), c_on(-1), c_last(-1), c_cnt(0), c_peak(0.f), k_on(-1), k_last(-1),
        k_cnt(0), k_peak(-1.f) {}
  // the open episode ended: keep it if it is sustained and at least as strong as the kept one
  __device__ __forceinline__ void close() {
    if (c_cnt >= min_count && c_peak >= k_peak) {
      k_on = c_on;
      k_last = c_last;
      k_cnt = c_cnt;
      k_peak = c_peak;
    }
  }
  __device__ __forceinline__ void hit(int t, double A, double B) {
    const float z = (float)(fabs(A) / sqrt(B));  // pod_epilogue's expression for z_last
    if (c_cnt > 0 && t - c_last <= gap) {
      c_last = t;
      ++c_cnt;
      c_peak = fmaxf(c_peak, z);
    } else {
      close();
      c_on = c_last = t;
      c_cnt = 1;
      c_peak = z;
    }
  }
};

// The streaming form (krca_stream_timeline; semantics in include/krca.h): the same two episodes,
// loaded from and stored to the episode state [8][S] (planes c_on, c_last, c_cnt, c_peak, k_on,
// k_last, k_cnt, k_peak: a wave's accesses are 256 consecutive bytes per plane), plus the horizon H
// after which an episode stops being reported.  A separate type: the batch kernels instantiate
// Episodes alone and carry none of this (rolling_score_pipe<60, 20> takes 124 VGPRs as the scorer, 4
// under the 128 of four waves per SIMD, and 140 with Episodes: DESIGN.md §3.13, Registers).
struct StreamEpisodes : Episodes {
  struct Args {
    int gap, min_count, H;
    int32_t* state;
    TimelineOut out;
  };
  int H;
  bool c_dirty, k_dirty;  // the open / the kept episode changed in this call: only then it is stored
  __device__ __forceinline__ explicit StreamEpisodes(const Args& a)
      : Episodes(Episodes::Args{a.gap, a.min_count, a.out}), H(a.H), c_dirty(false), k_dirty(false) {}
  __device__ __forceinline__ void load(const int32_t* p, int64_t S, int64_t sl) {
    c_on = p[sl];
    c_last = p[S + sl];
    c_cnt = p[2 * S + sl];
    c_peak = __builtin_bit_cast(float, p[3 * S + sl]);
    k_on = p[4 * S + sl];
    k_last = p[5 * S + sl];
    k_cnt = p[6 * S + sl];
    k_peak = __builtin_bit_cast(float, p[7 * S + sl]);
  }
  __device__ __forceinline__ void store(int32_t* p, int64_t S, int64_t sl) const {
    if (c_dirty) {
      p[sl] = c_on;
      p[S + sl] = c_last;
      p[2 * S + sl] = c_cnt;
      p[3 * S + sl] = __builtin_bit_cast(int32_t, c_peak);
    }
    if (k_dirty) {
      p[4 * S + sl] = k_on;
      p[5 * S + sl] = k_last;
      p[6 * S + sl] = k_cnt;
      p[7 * S + sl] = __builtin_bit_cast(int32_t, k_peak);
    }
  }
  // the open episode ended at step `now`: it replaces the kept one if it is sustained and the kept
  // one is absent, expired or no stronger
  __device__ __forceinline__ void close(int now) {
    if (c_cnt >= min_count && (k_cnt == 0 || now - k_last >= H || c_peak >= k_peak)) {
      k_on = c_on;
      k_last = c_last;
      k_cnt = c_cnt;
      k_peak = c_peak;
      k_dirty = true;
    }
  }
  __device__ __forceinline__ void hit(int t, double A, double B) {
    const float z = (float)(fabs(A) / sqrt(B));
    c_dirty = true;
    if (c_cnt > 0 && t - c_last <= gap) {
      c_last = t;
      ++c_cnt;
      c_peak = fmaxf(c_peak, z);
    } else {
      close(t);
      c_on = c_last = t;
      c_cnt = 1;
      c_peak = z;
    }
  }
};

// Pod combine of one episode per series (`has`: the lane has one), over the pod's M wave-aligned
// lanes (every lane of the wave takes part in the shuffles; a lane past S contributes "no
// episode").  Anchor = the episode of the largest peak (ties: lowest m); members = the episodes
// within `gap` of overlapping the anchor's [onset, last].
__device__ __forceinline__ void timeline_combine(bool has, int e_on, int e_last, int e_cnt, float e_peak, int gap,
                                                 int64_t s, bool active, int M, const TimelineOut& o) {
  const int lane = threadIdx.x & 63;
  const int m = lane & (M - 1);  // == s & (M - 1): workgroups start at a multiple of 256 series
  float ap = has ? e_peak : -1.f;
  int am = m;
  for (int off = 1; off < M; off <<= 1) {
    const float op = __shfl_xor(ap, off, 64);
    const int om = __shfl_xor(am, off, 64);
    if (op > ap || (op == ap && om < am)) {
      ap = op;
      am = om;
    }
  }
  const int src = (lane & ~(M - 1)) + am;
  const int64_t a_on = __shfl(e_on, src, 64), a_last = __shfl(e_last, src, 64);
  const bool mem = has && (int64_t)e_on <= a_last + gap && a_on <= (int64_t)e_last + gap;
  long long first = mem ? (((long long)e_on << 8) | m) : INT64_MAX;  // min: earliest onset, then lowest m
  int lastv = mem ? e_last : -1;
  int cnt = mem ? e_cnt : 0;
  int nm = mem ? 1 : 0;
  for (int off = 1; off < M; off <<= 1) {
    const long long of = __shfl_xor(first, off, 64);
    first = of < first ? of : first;
    const int ol = __shfl_xor(lastv, off, 64);
    lastv = ol > lastv ? ol : lastv;
    cnt += __shfl_xor(cnt, off, 64);
    nm += __shfl_xor(nm, off, 64);
  }
  if (!active || m != 0) return;
  const int64_t p = s / M;
  o.onset[p] = nm ? (int32_t)(first >> 8) : -1;
  o.last[p] = lastv;
  o.count[p] = cnt;
  o.peak[p] = nm ? ap : 0.f;
  o.lead[p] = nm ? (int8_t)(first & 0xff) : (int8_t)-1;
  o.n_metrics[p] = (uint8_t)nm;
}

// krca_rolling_timeline: the series is over, so its open episode closes; the kept ones combine
__device__ __forceinline__ void timeline_epilogue(Episodes& ep, int64_t s, bool active, int M,
                                                  const TimelineOut& o) {
  ep.close();
  timeline_combine(active && ep.k_cnt > 0, ep.k_on, ep.k_last, ep.k_cnt, ep.k_peak, ep.gap, s, active, M, o);
}

// krca_stream_timeline: the view of the series at step `now` (the call's last step), formed on
// copies -- the open episode stays open for the next call.  An episode is reported while
// now - last < H; the open one must be sustained, and wins over a valid kept one on c_peak >= k_peak
// (what close() would decide).
__device__ __forceinline__ void stream_timeline_epilogue(const StreamEpisodes& ep, int now, int64_t s, bool active,
                                                         int M, const TimelineOut& o) {
  const bool k_ok = ep.k_cnt > 0 && now - ep.k_last < ep.H;
  const bool c_ok = ep.c_cnt >= ep.min_count && now - ep.c_last < ep.H;
  const bool use_c = c_ok && (!k_ok || ep.c_peak >= ep.k_peak);
  timeline_combine(active && (use_c || k_ok), use_c ? ep.c_on : ep.k_on, use_c ? ep.c_last : ep.k_last,
                   use_c ? ep.c_cnt : ep.k_cnt, use_c ? ep.c_peak : ep.k_peak, ep.gap, s, active, M, o);
}

// Pod epilogue shared by both kernels: z_last per series, pod max|z|, exceedance sum, flags.
__device__ __forceinline__ void pod_epilogue(const StepState& st, double epsB, int64_t s, bool active, int M, int T,
                                             const float* __restrict__ xs, int64_t S,
                                             float* __restrict__ z_last, float* __restrict__ score,
                                             int32_t* __restrict__ n_exceed, uint8_t* __restrict__ flags) {
  const bool has_z = st.bl > epsB;
  const float z = has_z ? (float)(st.al / sqrt(st.bl)) : 0.f;
  const int m = (int)(s & (M - 1));
  float vlast = (active && T > 0) ? xs[(int64_t)(T - 1) * S] : 0.f;
  unsigned f = 0;
  if (m == 0) f = (vlast > 80.f ? KRCA_F_CPU80 : 0u) | (vlast > 90.f ? KRCA_F_CPU90 : 0u);
  if (m == 1) f = (vlast > 80.f ? KRCA_F_MEM80 : 0u) | (vlast > 90.f ? KRCA_F_MEM90 : 0u);
  float az = fabsf(z);
  int cnt = st.cnt;
  for (int off = 1; off < M; off <<= 1) {  // the M lanes of a pod are aligned inside the wave
    az = fmaxf(az, __shfl_xor(az, off, 64));
    cnt += __shfl_xor(cnt, off, 64);
    f |= __shfl_xor(f, off, 64);
  }
  if (!active) return;
  z_last[s] = z;
  if (m == 0) {
    const int64_t p = s / M;
    score[p] = az;
    n_exceed[p] = cnt;
    flags[p] = (uint8_t)f;
  }
}

template <int W>
__global__ __launch_bounds__(256) void rolling_score_ring(const float* __restrict__ x, int64_t S, int T, int M,
                                                          double thr2, float* __restrict__ z_last,
                                                          float* __restrict__ score, int32_t* __restrict__ n_exceed,
                                                          uint8_t* __restrict__ flags) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = s < S;
  const float* xs = x + (active ? s : 0);
  const double Wd = (double)W, epsB = kVarEps * Wd * Wd;
  StepState st{0.0, 0.0, 0, 0.0, 0.0};
  float ring[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const float v = (j < T && active) ? xs[(int64_t)j * S] : 0.f;
    ring[j] = v;
    const double vd = (double)v;
    st.s1 = st.s1 + vd;
    st.s2 = fma(vd, vd, st.s2);
  }
  int t0 = W;
  for (; t0 + W <= T; t0 += W) {  // full W-step blocks: every ring slot index is static
    float nx[W];
#pragma unroll
    for (int j = 0; j < W; ++j) nx[j] = active ? xs[(int64_t)(t0 + j) * S] : 0.f;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      step(st, nx[j], ring[j], Wd, epsB, thr2, t0 + j == T - 1);
      ring[j] = nx[j];
    }
  }
  if (t0 < T) {  // tail block
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if (t0 + j < T) {
        const float v = active ? xs[(int64_t)(t0 + j) * S] : 0.f;
        step(st, v, ring[j], Wd, epsB, thr2, t0 + j == T - 1);
        ring[j] = v;
      }
    }
  }
  pod_epilogue(st, epsB, s, active, M, T, xs, S, z_last, score, n_exceed, flags);
}

// gfx950 buffer loads: a wave-uniform buffer descriptor on a block of rows, the lane's 32-bit byte
// offset in voffset and the row offset j*S*4 in soffset, so a load costs no per-lane address
// arithmetic (`buffer_load_dword v, v_off, s[rsrc], s_off offen`).
template <int AUX = 0>  // cache policy bits: 0 default, 2 = nt (streamed once)
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, AUX));
}

// Software-pipelined form of rolling_score_ring over buffer loads (same arithmetic, same bits): the
// walk of score_walk.h, a rotating ring of W + D sample registers whose loads leave one per step,
// D rows ahead of their use, so each wave keeps about D rows (D*256 B) in flight through its whole
// compute phase and no sample is copied between registers.  Buffer descriptors cover exactly the
// rows < T of a group: loads past the end return 0 and touch no memory, which lets the prefetch run
// ahead unconditionally.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const float* x, int64_t S, uint32_t rowb, int t, int n,
                                                            int T) {
  int m = T - t;
  m = m < 0 ? 0 : (m > n ? n : m);
  m = __builtin_amdgcn_readfirstlane(m);  // wave-uniform: keeps the descriptor in SGPRs (no v_med3 waterfall)
  return __builtin_amdgcn_make_buffer_rsrc((void*)(x + (int64_t)(m ? t : 0) * S), 0, (int)(rowb * (uint32_t)m),
                                           0x00020000);
}

// Row sources of the pipelined kernel (the interface is score_walk()'s).  SpanRows: one descriptor
// per group spanning its n <= D rows (needs 4*S*D < 2^31: up to ~3.3M pods x 8 metrics at D = 20),
// rebuilt by scalar code.  BlockRows: one descriptor per row covering only the workgroup's 256
// series (base = x + t*S + s0), so any S < 2^32 works; it costs a few scalar instructions per row,
// off the vector path.
struct SpanRows {
  struct Group {
    __amdgpu_buffer_rsrc_t rs;
  };
  const float* x;
  int64_t S;
  uint32_t rowb, voff;
  int T;
  __device__ __forceinline__ SpanRows(const float* x_, int64_t S_, int T_, int64_t s, bool active)
      : x(x_), S(S_), rowb((uint32_t)(S_ * 4)), voff(active ? (uint32_t)s * 4u : 0u), T(T_) {}
  __device__ __forceinline__ Group group(int t, int n) const { return Group{span_rsrc(x, S, rowb, t, n, T)}; }
  template <int AUX>
  __device__ __forceinline__ float load(const Group& g, int j) const {
    return bload<AUX>(g.rs, voff, rowb * (uint32_t)j);
  }
};

struct BlockRows {
  struct Group {
    int t;
  };
  const float* xb;  // x + s0, s0 = the workgroup's first series
  int64_t S;
  uint32_t voff;
  int nrec;  // bytes of the workgroup's series inside [0, S)
  int T;
  __device__ __forceinline__ BlockRows(const float* x_, int64_t S_, int T_, int64_t, bool)
      : S(S_), voff(threadIdx.x * 4u), T(T_) {
    const int64_t s0 = (int64_t)blockIdx.x * blockDim.x;
    xb = x_ + s0;
    const int64_t n = S_ - s0;
    nrec = __builtin_amdgcn_readfirstlane((int)(4 * (n < (int64_t)blockDim.x ? n : (int64_t)blockDim.x)));
  }
  __device__ __forceinline__ Group group(int t, int) const { return Group{t}; }
  template <int AUX>
  __device__ __forceinline__ float load(const Group& g, int j) const {
    const int tt = g.t + j;
    const bool in = tt < T;
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (int64_t)(in ? tt : 0) * S), 0, in ? nrec : 0, 0x00020000);
    return bload<AUX>(rs, voff, 0);
  }
};

// Ep = Episodes: krca_rolling_timeline's form of the same pass (the episode state in the exceed
// branch, the pod combine of the kept episodes behind the scorer's epilogue).
template <int W, int D, int AUX = 0, class Rows = SpanRows, class Ep = NoEpisodes>
__global__ __launch_bounds__(256) void rolling_score_pipe(const float* __restrict__ x, int64_t S, int T, int M,
                                                          double thr2, float* __restrict__ z_last,
                                                          float* __restrict__ score, int32_t* __restrict__ n_exceed,
                                                          uint8_t* __restrict__ flags, typename Ep::Args targs) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = s < S;
  const Rows rows(x, S, T, s, active);
  StepState st{0.0, 0.0, 0, 0.0, 0.0};
  Ep ep(targs);
  score_walk<W, D, AUX>(rows, T, thr2, st, ep);  // requires T > W, checked by the launcher
  const double Wd = (double)W, epsB = kVarEps * Wd * Wd;
  pod_epilogue(st, epsB, s, active, M, T, x + (active ? s : 0), S, z_last, score, n_exceed, flags);
  if constexpr (Ep::kTrack) timeline_epilogue(ep, s, active, M, targs.out);
}

// Any W: the outgoing sample x[t-W] is re-read (same values, same arithmetic -> same bits).
template <class Ep = NoEpisodes>
__global__ __launch_bounds__(256) void rolling_score_reread(const float* __restrict__ x, int64_t S, int T, int W,
                                                            int M, double thr2, float* __restrict__ z_last,
                                                            float* __restrict__ score,
                                                            int32_t* __restrict__ n_exceed,
                                                            uint8_t* __restrict__ flags, typename Ep::Args targs) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = s < S;
  const float* xs = x + (active ? s : 0);
  const double Wd = (double)W, epsB = kVarEps * Wd * Wd;
  StepState st{0.0, 0.0, 0, 0.0, 0.0};
  Ep ep(targs);
  for (int j = 0; j < W && j < T; ++j) {
    const double vd = active ? (double)xs[(int64_t)j * S] : 0.0;
    st.s1 = st.s1 + vd;
    st.s2 = fma(vd, vd, st.s2);
  }
  for (int t = W; t < T; ++t) {
    const float v = active ? xs[(int64_t)t * S] : 0.f;
    const float o = active ? xs[(int64_t)(t - W) * S] : 0.f;
    step(st, v, o, Wd, epsB, thr2, t == T - 1, ep, t);
  }
  pod_epilogue(st, epsB, s, active, M, T, xs, S, z_last, score, n_exceed, flags);
  if constexpr (Ep::kTrack) timeline_epilogue(ep, s, active, M, targs.out);
}

// ---- streaming rescoring (BASELINE configs[4]) ----------------------------
// The batch scorer applied to an unbounded stream, carried forward window by window: state per
// series = the float64 window sums (s1, s2), the last W samples (ring [W][S]) and the exceedance
// bits of the last H evaluated steps (bits [ceil(H/32)][S]) with their count.  A window of delta
// new steps t0 .. t0+delta-1 runs exactly the batch kernel's operations for those steps (the
// prologue sums while t < W, step() after), so after any sequence of windows z_last / score /
// flags equal krca_rolling_score over the whole series so far, and n_exceed counts its
// exceedances over the last H evaluated steps (all of them while there are fewer than H).
// Per series and window: 20 B of state read + written, 12*delta B of samples (new, old, ring
// write) and 8*delta B of exceedance bits.
struct StreamState {
  double* s1;
  double* s2;
  int32_t* cnt;
  float* ring;
  uint32_t* bits;
};

//
// Ep = StreamEpisodes: krca_stream_timeline's form.  The lane's 8 words of episode state are loaded
// with the sums (the latency overlaps the first sample loads), updated in the exceed branch and
// stored only by the lanes whose episodes changed (the t0 == 0 call stores every lane's initial
// state); the pod combine of the views runs behind the scorer's epilogue.  Per series and window it
// adds 32 B of state read, and 18 B of outputs per pod.
template <class Ep = NoEpisodes>
__global__ __launch_bounds__(256) void stream_score(const float* __restrict__ xn, int64_t S, int delta, int64_t t0,
                                                    int W, int H, int M, double thr2, StreamState stt,
                                                    float* __restrict__ z_last, float* __restrict__ score,
                                                    int32_t* __restrict__ n_exceed, uint8_t* __restrict__ flags,
                                                    typename Ep::Args targs) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = s < S;
  const int64_t sl = active ? s : 0;
  const double Wd = (double)W, epsB = kVarEps * Wd * Wd;
  StepState st{0.0, 0.0, 0, 0.0, 0.0};
  Ep ep(targs);
  int cnt = 0;
  if (t0 > 0) {
    st.s1 = stt.s1[sl];
    st.s2 = stt.s2[sl];
    cnt = stt.cnt[sl];
    if constexpr (Ep::kTrack) ep.load(targs.state, S, sl);
  } else if constexpr (Ep::kTrack) {
    ep.c_dirty = ep.k_dirty = true;  // the stream starts: whatever the state held is replaced
  }
  for (int j = 0; j < delta; ++j) {
    const int64_t t = t0 + j;
    const float v = xn[(int64_t)j * S + sl];
    float* rp = stt.ring + (t % W) * S + sl;
    if (t < W) {  // the batch prologue: window fill
      const double vd = (double)v;
      st.s1 = st.s1 + vd;
      st.s2 = fma(vd, vd, st.s2);
    } else {
      const float o = *rp;
      st.cnt = 0;
      step(st, v, o, Wd, epsB, thr2, j == delta - 1, ep, (int)t);
      const int64_t e = t - W;  // index among the evaluated steps
      uint32_t* wp = stt.bits + ((e % H) >> 5) * S + sl;
      const uint32_t bit = 1u << ((e % H) & 31);
      const uint32_t word = *wp;  // zeroed when the stream starts (t0 == 0)
      cnt += st.cnt - ((word & bit) ? 1 : 0);
      if (active) *wp = st.cnt ? (word | bit) : (word & ~bit);
    }
    if (active) *rp = v;
  }
  if (active) {
    stt.s1[sl] = st.s1;
    stt.s2[sl] = st.s2;
    stt.cnt[sl] = cnt;
    if constexpr (Ep::kTrack) ep.store(targs.state, S, sl);
  }
  st.cnt = cnt;
  if (t0 + delta - 1 < W) st.bl = 0.0;  // no evaluated step yet: z = 0
  pod_epilogue(st, epsB, s, active, M, delta, xn + sl, S, z_last, score, n_exceed, flags);
  if constexpr (Ep::kTrack) stream_timeline_epilogue(ep, (int)(t0 + delta - 1), s, active, M, targs.out);
}

bool pipe_window(int W) { return W == 60 || W == 30 || W == 20 || W == 15 || W == 10; }

// the metric stream is read once: non-temporal loads (cache policy nt), 6.17 -> 6.61 TB/s at C4
// (tools/score_ab.py)
constexpr int kNt = 2;

struct ScoreCall {
  const float* x;
  int64_t S;
  int T, W, M;
  double thr2;
  float* z_last;
  float* score;
  int32_t* n_exceed;
  uint8_t* flags;
  dim3 grid;
  hipStream_t st;
};

template <class Ep>
void launch_reread(const ScoreCall& c, const typename Ep::Args& ea) {
  hipLaunchKernelGGL(rolling_score_reread<Ep>, c.grid, dim3(256), 0, c.st, c.x, c.S, c.T, c.W, c.M, c.thr2, c.z_last,
                     c.score, c.n_exceed, c.flags, ea);
}

// a window with a compiled-in size.  The ring kernel has no timeline form: the timeline re-reads
// wherever the scorer runs it (T <= W, or forced).
template <int W, class Ep>
void launch_window(int variant, const ScoreCall& c, const typename Ep::Args& ea) {
  constexpr int D = prefetch_rows(W);
  if (variant == KRCA_SCORE_PIPE)
    hipLaunchKernelGGL((rolling_score_pipe<W, D, kNt, SpanRows, Ep>), c.grid, dim3(256), 0, c.st, c.x, c.S, c.T, c.M,
                       c.thr2, c.z_last, c.score, c.n_exceed, c.flags, ea);
  else if (variant == KRCA_SCORE_PIPE_ROWS)
    hipLaunchKernelGGL((rolling_score_pipe<W, D, kNt, BlockRows, Ep>), c.grid, dim3(256), 0, c.st, c.x, c.S, c.T, c.M,
                       c.thr2, c.z_last, c.score, c.n_exceed, c.flags, ea);
  else if constexpr (Ep::kTrack)
    launch_reread<Ep>(c, ea);
  else
    hipLaunchKernelGGL(rolling_score_ring<W>, c.grid, dim3(256), 0, c.st, c.x, c.S, c.T, c.M, c.thr2, c.z_last, c.score,
                       c.n_exceed, c.flags);
}

// krca_rolling_score (Ep = NoEpisodes) and krca_rolling_timeline (Episodes): the kernel that
// krca_rolling_score_variant names for these sizes
template <class Ep>
int launch_score(const char* fn, const float* x, int64_t P, int32_t M, int32_t T, int32_t W, float z_thr, float* z_last,
                 float* score, int32_t* n_exceed, uint8_t* flags, const typename Ep::Args& ea, void* stream) {
  KRCA_CHECK_ARG(P >= 0 && T >= 0 && W >= 1, "%s: bad sizes P=%lld T=%d W=%d", fn, (long long)P, T, W);
  KRCA_CHECK_ARG(M >= 1 && M <= 64 && (M & (M - 1)) == 0, "%s: M=%d must be a power of two <= 64", fn, M);
  bool outs = x && z_last && score && n_exceed && flags;
  if constexpr (Ep::kTrack) {
    KRCA_CHECK_ARG(ea.gap >= 0 && ea.min_count >= 1, "%s: gap=%d must be >= 0, min_count=%d >= 1", fn, ea.gap,
                   ea.min_count);
    const TimelineOut& o = ea.out;
    outs = outs && o.onset && o.last && o.count && o.peak && o.lead && o.n_metrics;
  }
  if (P == 0) return KRCA_OK;
  KRCA_CHECK_ARG(outs, "%s: null pointer", fn);
  const int64_t S = P * (int64_t)M;
  KRCA_CHECK_ARG(S < (int64_t(1) << 32), "%s: P*M must be < 2^32", fn);
  const double thr2 = (double)z_thr * (double)z_thr;
  const dim3 grid((unsigned)krca::ceil_div(S, 256));
  const ScoreCall c{x, S, T, W, M, thr2, z_last, score, n_exceed, flags, grid, krca::as_stream(stream)};
  const int variant = krca_rolling_score_variant(P, M, T, W);
  switch (W) {  // the cases are pipe_window()'s
    case 60: launch_window<60, Ep>(variant, c, ea); break;
    case 30: launch_window<30, Ep>(variant, c, ea); break;
    case 20: launch_window<20, Ep>(variant, c, ea); break;
    case 15: launch_window<15, Ep>(variant, c, ea); break;
    case 10: launch_window<10, Ep>(variant, c, ea); break;
    default: launch_reread<Ep>(c, ea);
  }
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}
}  // namespace

extern "C" {

// state: s1, s2 f64 [S] | cnt i32 [S] | ring f32 [W][S] | bits u32 [ceil(H/32)][S]  (S = P*M)
int64_t krca_stream_state_size(int64_t P, int32_t M, int32_t W, int32_t H) {
  const int64_t S = P * M;
  return S * (8 + 8 + 4) + (int64_t)W * S * 4 + krca::ceil_div(H, 32) * S * 4 + 64;
}

// episode state of krca_stream_timeline: int32 / float32 planes [8][S]
int64_t krca_stream_episode_state_size(int64_t P, int32_t M) { return P * (int64_t)M * 8 * 4; }

}  // extern "C"

namespace {
// krca_stream_score (Ep = NoEpisodes) and krca_stream_timeline (StreamEpisodes)
template <class Ep>
int launch_stream(const char* fn, const float* x_new, int64_t P, int32_t M, int32_t delta, int64_t t0, int32_t W,
                  int32_t H, float z_thr, void* state, float* z_last, float* score, int32_t* n_exceed, uint8_t* flags,
                  const typename Ep::Args& ea, void* stream) {
  KRCA_CHECK_ARG(P >= 0 && delta >= 1 && t0 >= 0 && W >= 1 && H >= 1, "%s: bad sizes", fn);
  KRCA_CHECK_ARG(M >= 1 && M <= 64 && (M & (M - 1)) == 0, "%s: M=%d must be a power of two <= 64", fn, M);
  bool ptrs = x_new && state && z_last && score && n_exceed && flags;
  if constexpr (Ep::kTrack) {
    KRCA_CHECK_ARG(ea.gap >= 0 && ea.min_count >= 1, "%s: gap=%d must be >= 0, min_count=%d >= 1", fn, ea.gap,
                   ea.min_count);
    KRCA_CHECK_ARG(t0 + delta <= (int64_t)INT32_MAX, "%s: t0 + delta = %lld is past INT32_MAX (onsets are int32)", fn,
                   (long long)(t0 + delta));
    const TimelineOut& o = ea.out;
    ptrs = ptrs && ea.state && o.onset && o.last && o.count && o.peak && o.lead && o.n_metrics;
  }
  if (P == 0) return KRCA_OK;
  KRCA_CHECK_ARG(ptrs, "%s: null pointer", fn);
  if constexpr (Ep::kTrack)
    KRCA_CHECK_ARG(((uintptr_t)ea.state & 3) == 0, "%s: the episode state must be 4-byte aligned", fn);
  const int64_t S = P * (int64_t)M;
  char* b = reinterpret_cast<char*>(state);
  StreamState stt;
  stt.s1 = reinterpret_cast<double*>(b);
  stt.s2 = stt.s1 + S;
  stt.cnt = reinterpret_cast<int32_t*>(stt.s2 + S);
  stt.ring = reinterpret_cast<float*>(stt.cnt + S);
  stt.bits = reinterpret_cast<uint32_t*>(stt.ring + (int64_t)W * S);
  hipStream_t st = krca::as_stream(stream);
  if (t0 == 0) KRCA_HIP(hipMemsetAsync(stt.bits, 0, krca::ceil_div(H, 32) * S * 4, st));
  hipLaunchKernelGGL(stream_score<Ep>, dim3((unsigned)krca::ceil_div(S, 256)), dim3(256), 0, st, x_new, S, delta, t0, W,
                     H, M, (double)z_thr * (double)z_thr, stt, z_last, score, n_exceed, flags, ea);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}
}  // namespace

extern "C" {

int krca_stream_score(const float* x_new, int64_t P, int32_t M, int32_t delta, int64_t t0, int32_t W, int32_t H,
                      float z_thr, void* state, float* z_last, float* score, int32_t* n_exceed, uint8_t* flags,
                      void* stream) {
  return launch_stream<NoEpisodes>("krca_stream_score", x_new, P, M, delta, t0, W, H, z_thr, state, z_last, score,
                                   n_exceed, flags, NoEpisodes::Args{}, stream);
}

int krca_stream_timeline(const float* x_new, int64_t P, int32_t M, int32_t delta, int64_t t0, int32_t W, int32_t H,
                         float z_thr, int32_t gap, int32_t min_count, void* state, void* ep_state, float* z_last,
                         float* score, int32_t* n_exceed, uint8_t* flags, int32_t* onset, int32_t* last, int32_t* count,
                         float* peak, int8_t* lead, uint8_t* n_metrics, void* stream) {
  const StreamEpisodes::Args ea{gap, min_count, H, reinterpret_cast<int32_t*>(ep_state),
                                TimelineOut{onset, last, count, peak, lead, n_metrics}};
  return launch_stream<StreamEpisodes>("krca_stream_timeline", x_new, P, M, delta, t0, W, H, z_thr, state, z_last,
                                       score, n_exceed, flags, ea, stream);
}

int krca_usage_flags(const float* usage, int64_t P, uint8_t* flags, void* stream) {
  KRCA_CHECK_ARG(P >= 0, "krca_usage_flags: P < 0");
  if (P == 0) return KRCA_OK;
  KRCA_CHECK_ARG(usage && flags, "krca_usage_flags: null pointer");
  const int64_t blocks = std::min<int64_t>(krca::ceil_div(P, 256), 4096);
  hipLaunchKernelGGL(usage_flags_kernel, dim3((unsigned)blocks), dim3(256), 0, krca::as_stream(stream),
                     reinterpret_cast<const float2*>(usage), P, flags);
  KRCA_LAUNCH_CHECK();
  return KRCA_OK;
}

int krca_rolling_score_variant(int64_t P, int32_t M, int32_t T, int32_t W) {
  const int impl = krca::tuning().score_impl;  // tests force KRCA_SCORE_RING / KRCA_SCORE_PIPE_ROWS at small shapes
  if (!pipe_window(W)) return KRCA_SCORE_REREAD;
  if (T <= W || impl == KRCA_SCORE_RING) return KRCA_SCORE_RING;
  if (impl == KRCA_SCORE_PIPE_ROWS) return KRCA_SCORE_PIPE_ROWS;
  return P * (int64_t)M * 4 * prefetch_rows(W) < (int64_t(1) << 31) ? KRCA_SCORE_PIPE : KRCA_SCORE_PIPE_ROWS;
}

int krca_rolling_score(const float* x, int64_t P, int32_t M, int32_t T, int32_t W, float z_thr, float* z_last,
                       float* score, int32_t* n_exceed, uint8_t* flags, void* stream) {
  return launch_score<NoEpisodes>("krca_rolling_score", x, P, M, T, W, z_thr, z_last, score, n_exceed, flags,
                                  NoEpisodes::Args{}, stream);
}

int krca_rolling_timeline(const float* x, int64_t P, int32_t M, int32_t T, int32_t W, float z_thr, int32_t gap,
                          int32_t min_count, float* z_last, float* score, int32_t* n_exceed, uint8_t* flags,
                          int32_t* onset, int32_t* last, int32_t* count, float* peak, int8_t* lead,
                          uint8_t* n_metrics, void* stream) {
  const Episodes::Args tl{gap, min_count, TimelineOut{onset, last, count, peak, lead, n_metrics}};
  return launch_score<Episodes>("krca_rolling_timeline", x, P, M, T, W, z_thr, z_last, score, n_exceed, flags, tl,
                                stream);
}

}  // extern "C"
