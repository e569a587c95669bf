// The per-series walk of the pipelined rolling scorer (rolling_score_pipe in score.hip): the
// arithmetic of one step and the schedule of sample registers and row requests around it.  Host
// and device code: tests/host/score_walk_host.cpp instantiates the same walk over a plain array and
// checks its indexing on the CPU; score.hip supplies the buffer-load row sources and the shuffle
// epilogues, which stay device-only.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KRCA_WALK_FN __host__ __device__ __forceinline__
#else
#define KRCA_WALK_FN inline
#endif

#pragma clang fp contract(off)

namespace krca_walk {

constexpr double kVarEps = 1e-12;

struct StepState {
  double s1, s2;  // window sum and sum of squares (float64, fixed order)
  int cnt;        // exceedances of this series
  double al, bl;  // A and B (below) at t = T-1
};

// One time step of the rolling statistics; `old` is x[t-W].  With A = W*x_t - s1 and
// B = W*s2 - s1^2 (= W^2 * var, ddof 0):  z = A / sqrt(B),  |z| > thr  <=>  A^2 > thr^2 * B,
// var > 1e-12  <=>  B > 1e-12 * W^2 — 13 float64 operations per sample, no division or sqrt.
// The fma()s are explicit (and mirrored in oracle/krca_oracle.c): one rounding each.
KRCA_WALK_FN void step(StepState& st, float v, float old, double Wd, double epsB, double thr2, bool last) {
  const double vd = (double)v;
  const double od = (double)old;
  const double A = fma(Wd, vd, -st.s1);
  const double B = fma(Wd, st.s2, -(st.s1 * st.s1));
  st.cnt += (B > epsB) && (fma(A, A, -(thr2 * B)) > 0.0);
  if (last) {
    st.al = A;
    st.bl = B;
  }
  st.s1 = (st.s1 + vd) - od;
  st.s2 = fma(-od, od, fma(vd, vd, st.s2));
}

// The same step for the kernels that exist in a scoring and a timeline form.  `ep` is an episode
// policy (score.hip) and sees the exceedances only: with Ep::kTrack false (NoEpisodes,
// krca_rolling_score) this is plain step() and the code of the scorer's kernels is what it was
// without the parameter; with kTrack true (Episodes, krca_rolling_timeline) ep.hit(t, A, B) gets
// every exceeding step t of the series.
template <class Ep>
KRCA_WALK_FN void step(StepState& st, float v, float old, double Wd, double epsB, double thr2, bool last, Ep& ep,
                       int t) {
  if constexpr (!Ep::kTrack) {
    step(st, v, old, Wd, epsB, thr2, last);
  } else {
    const double vd = (double)v;
    const double od = (double)old;
    const double A = fma(Wd, vd, -st.s1);
    const double B = fma(Wd, st.s2, -(st.s1 * st.s1));
    const bool exceed = (B > epsB) && (fma(A, A, -(thr2 * B)) > 0.0);
    st.cnt += exceed;
    if (exceed) ep.hit(t, A, B);  // rare and divergent; the only place episode state is touched
    if (last) {
      st.al = A;
      st.bl = B;
    }
    st.s1 = (st.s1 + vd) - od;
    st.s2 = fma(-od, od, fma(vd, vd, st.s2));
  }
}

// Prefetch distance D of the walk, in rows, per pipelined window: a wave keeps about D rows
// (D * 256 B) in flight through the whole loop.  W = 60 is the measured choice; the
// A/B libraries of that measurement set KRCA_SCORE_D60, the shipped library never does.
#ifndef KRCA_SCORE_D60
#define KRCA_SCORE_D60 20
#endif
constexpr int prefetch_rows(int W) { return W == 60 ? KRCA_SCORE_D60 : (W == 30 || W == 15 ? 15 : 10); }

// The walk of one series over rows [0, T), T > W: window sums over rows [0, W), then step() for
// t = W .. T-1, in that order.
//
// Samples live in one rotating ring of R = W + D registers: x[t] in slot[t % R].  Every loop below
// is unrolled and walks whole rounds of R steps that start at tb = W (mod R), so every slot index
// is static: at position u of a round (t = tb + u) the step reads new = slot[(W + u) % R] and
// old = slot[u], which holds x[t - W]; that register is dead after the step, so the request for row
// t + D lands in it.  Requests leave one per step, D rows ahead of their use, and no sample is ever
// copied from one register to another.
//
// Rows come from `rows` in groups of up to D consecutive rows: g = rows.group(t, n) announces rows
// [t, t + n), rows.load<AUX>(g, j) returns row t + j of the series, or 0 (touching no memory) when
// t + j >= T.  Every row < T is requested exactly once; the requests run up to R - 1 rows past T
// and the guarded final round never reads what they returned.  Only that round, the one holding
// t = T-1, keeps the last-step A and B, so the steady loop has no per-sample select.
template <int W, int D, int AUX, class Rows, class Ep>
KRCA_WALK_FN void score_walk(const Rows& rows, int T, double thr2, StepState& st, Ep& ep) {
  constexpr int R = W + D;
  const double Wd = (double)W, epsB = kVarEps * Wd * Wd;
  float slot[R];
  // prologue: rows [0, R) fill the window and the first D rows of prefetch
#pragma unroll
  for (int u0 = 0; u0 < R; u0 += D) {
    const int n = R - u0 < D ? R - u0 : D;
    const typename Rows::Group g = rows.group(u0, n);
#pragma unroll
    for (int j = 0; j < n; ++j) slot[u0 + j] = rows.template load<AUX>(g, j);
  }
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const double vd = (double)slot[j];
    st.s1 = st.s1 + vd;
    st.s2 = fma(vd, vd, st.s2);
  }
  int tb = W;
  for (; tb + R < T; tb += R) {  // full rounds that do not contain t = T-1
#pragma unroll
    for (int u0 = 0; u0 < R; u0 += D) {
      const int n = R - u0 < D ? R - u0 : D;
      const typename Rows::Group g = rows.group(tb + u0 + D, n);
#pragma unroll
      for (int j = 0; j < n; ++j) {
        const int u = u0 + j;
        step(st, slot[(W + u) % R], slot[u], Wd, epsB, thr2, false, ep, tb + u);
        slot[u] = rows.template load<AUX>(g, j);  // row tb + u + D
      }
    }
  }
  // final round: steps [tb, T), 1..R of them.  Rows [tb, tb + D) are in their slots; the requests
  // of positions [0, W) bring rows [tb + D, tb + R), the last a step here can read.
#pragma unroll
  for (int u0 = 0; u0 < R; u0 += D) {
    const int n = R - u0 < D ? R - u0 : D;
    const int nl = W - u0 < 0 ? 0 : (W - u0 < n ? W - u0 : n);  // requests of this group
    const typename Rows::Group g = rows.group(tb + u0 + D, nl);
#pragma unroll
    for (int j = 0; j < n; ++j) {
      const int u = u0 + j, t = tb + u;
      if (t < T) step(st, slot[(W + u) % R], slot[u], Wd, epsB, thr2, t == T - 1, ep, t);
      if (j < nl) slot[u] = rows.template load<AUX>(g, j);
    }
  }
}

}  // namespace krca_walk
