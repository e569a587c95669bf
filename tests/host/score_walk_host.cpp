// Host instantiation of the pipelined scorer's per-series walk (csrc/score_walk.h) for
// tests/test_score_walk_cpu.py: the same template the kernel runs, over a row source that reads a
// plain time-major array, logs every row it is asked for and returns 0 -- or, to show that such a
// value is never used, a poison -- for rows at or past T.  swalk_ref is the plain restatement of
// oracle/krca_oracle.c's loop that the walk must match bit for bit.
#include <cmath>
#include <cstdint>

#include "score_walk.h"

#pragma clang fp contract(off)

namespace {

struct ArrayRows {
  struct Group {
    int t;
  };
  const float* xs;  // the series' first sample; rows are `stride` floats apart
  int64_t stride;
  int T;
  float past;  // what a row >= T returns
  int32_t* log;
  int cap;
  mutable int n;
  Group group(int t, int) const { return Group{t}; }
  template <int AUX>
  float load(const Group& g, int j) const {
    const int t = g.t + j;
    if (n < cap) log[n] = t;
    ++n;
    return t < T ? xs[(int64_t)t * stride] : past;
  }
};

struct NoEpisodes {  // the scorer's episode policy: nothing tracked
  static constexpr bool kTrack = false;
};

template <int W, int D>
int run(ArrayRows& rows, double thr2, double* out, int32_t* cnt) {
  krca_walk::StepState st{0.0, 0.0, 0, 0.0, 0.0};
  NoEpisodes ep;
  krca_walk::score_walk<W, D, 0>(rows, rows.T, thr2, st, ep);
  out[0] = st.s1;
  out[1] = st.s2;
  out[2] = st.al;
  out[3] = st.bl;
  *cnt = st.cnt;
  return rows.n;
}

}  // namespace

extern "C" {

// the library's prefetch distance for a pipelined window
int swalk_prefetch_rows(int W) { return krca_walk::prefetch_rows(W); }

// Walk series xs[t * stride], t < T, with the (W, D) instantiation: out = {s1, s2, A_last, B_last},
// *cnt = exceedances.  Returns the number of row requests (the first `cap` are in log), -1 for a
// pair that is not instantiated here.
int swalk_run(int W, int D, const float* xs, int64_t stride, int T, double thr2, int poison, double* out,
              int32_t* cnt, int32_t* log, int cap) {
  ArrayRows rows{xs, stride, T, poison ? std::nanf("") : 0.f, log, cap, 0};
#define KRCA_WALK_CASE(w, d) \
  if (W == w && D == d) return run<w, d>(rows, thr2, out, cnt);
  KRCA_WALK_CASE(60, 16)
  KRCA_WALK_CASE(60, 20)
  KRCA_WALK_CASE(60, 24)
  KRCA_WALK_CASE(30, 15)
  KRCA_WALK_CASE(20, 10)
  KRCA_WALK_CASE(15, 15)
  KRCA_WALK_CASE(10, 10)
#undef KRCA_WALK_CASE
  return -1;
}

// oracle/krca_oracle.c's loop for one series, T > W
void swalk_ref(int W, const float* xs, int64_t stride, int T, double thr2, double* out, int32_t* cnt) {
  const double Wd = (double)W, epsB = 1e-12 * Wd * Wd;
  double s1 = 0.0, s2 = 0.0, al = 0.0, bl = 0.0;
  int32_t c = 0;
  for (int j = 0; j < W && j < T; ++j) {
    const double vd = (double)xs[(int64_t)j * stride];
    s1 = s1 + vd;
    s2 = fma(vd, vd, s2);
  }
  for (int t = W; t < T; ++t) {
    const double vd = (double)xs[(int64_t)t * stride];
    const double od = (double)xs[(int64_t)(t - W) * stride];
    const double A = fma(Wd, vd, -s1);
    const double B = fma(Wd, s2, -(s1 * s1));
    c += (B > epsB) && (fma(A, A, -(thr2 * B)) > 0.0);
    if (t == T - 1) {
      al = A;
      bl = B;
    }
    s1 = (s1 + vd) - od;
    s2 = fma(-od, od, fma(vd, vd, s2));
  }
  out[0] = s1;
  out[1] = s2;
  out[2] = al;
  out[3] = bl;
  *cnt = c;
}

}  // extern "C"
