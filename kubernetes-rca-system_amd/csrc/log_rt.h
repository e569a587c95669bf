// The two pattern-table policies of the log scan's walk kernels.  Included by logscan.hip inside its
// namespace, ahead of log_dfa<Tab> and log_dfa_long<Tab, CARRY>: a policy supplies the table fill,
// the symbol lookups, the transition steps and the category masks; the walks themselves exist once.
//
//   TabBuiltin  the 13 compiled-in patterns (log_dfa_tables.h, constant memory; 31 symbols, 512
//               states at most) in static LDS: DfaLds4's 32-bit entries carrying the target's
//               category mask for the lockstep walk, DfaLds' 16-bit entries for the long-line walk.
//   TabRt<RSL>  a set compiled at RUN TIME (include/krca.h; krca/logdfa.py builds the tables) in
//               dynamic LDS, rows of 1 << RSL columns.
//
// TabRt's table is a straight copy of the device form (log_rt_layout.h): 16-bit entries {target state
// | kRtAcc}.  A 32-bit entry carrying the mask fits 160 KiB of LDS only up to 640 states of 64
// columns, and its 16-bit row offsets stop at 64 KiB; one 16-bit form covers every set inside the
// limits (1024 x 64 x 2 B = 128 KiB) and halves the 13 shipped patterns' table (25 KB for 49 KB).  The
// price: the row offset is rebuilt per step (an AND and a shift-add on the dependent chain where
// TabBuiltin has one SDWA add) and the category masks come from out[] -- read only for the entries
// flagged kRtAcc, tested once per 16-byte block.
//
// Memory safety: what rt_fill copies is sanitised (targets clamped to nstate - 1, symbols to the row
// width, masks to ncat bits), so whatever the device form holds, every table index stays below
// nstate << RSL and every out[] index below nstate.
#pragma once

using krca::kRtAcc;
using krca::kRtState;

struct TabBuiltin {
  static __device__ __forceinline__ DfaLds4& d4() {
    __shared__ DfaLds4 d;
    return d;
  }
  static __device__ __forceinline__ uint32_t* rng() {
    __shared__ uint32_t r[3 * KRCA_DFA_NRANGE];
    return r;
  }
  static __device__ __forceinline__ DfaLds& dl() {
    __shared__ DfaLds d;
    return d;
  }
  // -- the lockstep walk: st is the last entry read (mask << 16 | row offset), acc the OR of the entries
  __device__ __forceinline__ void fill_walk() const {
    load_ranges(rng());
    dfa4_load(d4());  // (its barrier covers the ranges)
  }
  __device__ __forceinline__ uint32_t byte_off(uint32_t b) const { return d4().sym[b]; }
  __device__ __forceinline__ uint32_t cp_off(uint32_t cp) const {
    return range_sym(rng(), KRCA_DFA_NRANGE, KRCA_DFA_OTHER, cp) * 4;
  }
  __device__ __forceinline__ void steps(const uint32_t (&so)[16], uint32_t& st, uint32_t& acc) const {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t t = dfa4_step(d4(), st, so[k]);
      st = t;
      acc |= t;
    }
  }
  __device__ __forceinline__ uint32_t line_mask(uint32_t acc) const { return acc >> 16; }
  // -- the long-line walk: a state is its row's offset in DfaLds::trans
  __device__ __forceinline__ void fill_long() const { dfa_load(dl()); }
  __device__ __forceinline__ uint32_t step(uint32_t st, uint32_t cp) const { return dl().trans[st + cp_symbol(dl(), cp)]; }
  __device__ __forceinline__ uint32_t state(uint32_t t) const { return t & (kAcc - 1); }
  __device__ __forceinline__ bool accepts(uint32_t t) const { return (t & kAcc) != 0; }
  __device__ __forceinline__ uint32_t mask(uint32_t st) const { return dl().out[st / KRCA_DFA_NSYM]; }
  __device__ __forceinline__ int warm() const { return WARM; }
};

struct RtDims {  // krca_log_dims as the kernels take it (re-checked against the limits by the host)
  int32_t ncat, nsym, nstate, nrange, warm, other;
  uint32_t out_off, sym_off, rng_off, bytes;
};

extern __shared__ __attribute__((aligned(16))) uint8_t rt_lds[];

template <int RSL>
__device__ __forceinline__ void rt_fill(const uint8_t* __restrict__ tab, const RtDims dm) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tab);
  uint32_t* dst = reinterpret_cast<uint32_t*>(rt_lds);
  const uint32_t last = (uint32_t)dm.nstate - 1u, nop = (1u << RSL) - 1u, cat = (1u << dm.ncat) - 1u;
  const int w_out = (int)(dm.out_off / 4), w_sym = (int)(dm.sym_off / 4), w_rng = (int)(dm.rng_off / 4),
            w_end = (int)(dm.bytes / 4);
  const int n_trans = (dm.nstate << RSL) / 2;  // words holding entries; the padding up to out_off is never read
  for (int i0 = threadIdx.x; i0 < w_end; i0 += 8 * (int)blockDim.x) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * (int)blockDim.x;
      v[u] = i < w_end ? src[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * (int)blockDim.x;
      if (i >= w_end) continue;
      uint32_t x = v[u];
      if (i < n_trans) {
        const uint32_t a = min(x & kRtState, last), b = min((x >> 16) & kRtState, last);
        x = (x & (kRtAcc | (kRtAcc << 16))) | a | (b << 16);
      } else if (i < w_out) {
        x = 0u;
      } else if (i < w_sym) {
        x &= cat | (cat << 16);
      } else if (i < w_rng) {
        x = min(x & 0xFFu, nop) | (min((x >> 8) & 0xFFu, nop) << 8) | (min((x >> 16) & 0xFFu, nop) << 16) |
            (min(x >> 24, nop) << 24);
        x <<= 1;  // LDS holds the symbols' entry offsets in bytes (<= 126 each: no carry between the bytes)
      } else if ((i - w_rng) % 3 == 2) {
        x = min(x, nop);
      }
      dst[i] = x;
    }
  }
  __syncthreads();
}

template <int RSL>
struct TabRt {  // (a kernel argument: the device form and its dimensions)
  const uint8_t* tab;
  RtDims dm;
  // byte-addressed: entry (state, symbol) at ((state << RSL) + symbol) * 2
  __device__ __forceinline__ const uint8_t* trans() const { return rt_lds; }
  __device__ __forceinline__ const uint16_t* out() const { return reinterpret_cast<const uint16_t*>(rt_lds + dm.out_off); }
  __device__ __forceinline__ const uint8_t* sym() const { return rt_lds + dm.sym_off; }  // byte -> symbol * 2
  __device__ __forceinline__ const uint32_t* rng() const { return reinterpret_cast<const uint32_t*>(rt_lds + dm.rng_off); }
  __device__ __forceinline__ uint32_t cp_sym(uint32_t cp) const {  // (nrange <= 1024 triples, whatever they hold)
    return range_sym(rng(), dm.nrange, (uint32_t)dm.other, cp);
  }
  // -- the lockstep walk: st is the last entry read (state | flag), acc the line's mask
  __device__ __forceinline__ void fill_walk() const { rt_fill<RSL>(tab, dm); }
  __device__ __forceinline__ uint32_t byte_off(uint32_t b) const { return sym()[b]; }
  __device__ __forceinline__ uint32_t cp_off(uint32_t cp) const { return cp_sym(cp) * 2; }
  __device__ __forceinline__ void steps(const uint32_t (&so)[16], uint32_t& st, uint32_t& acc) const {
    uint32_t t[16], any = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      st = *reinterpret_cast<const uint16_t*>(trans() + (((st & kRtState) << (RSL + 1)) + so[k]));
      t[k] = st;
      any |= st;
    }
    if (any & kRtAcc) {  // (rare) a category was reported in this block: its mask from out[]
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (t[k] & kRtAcc) acc |= out()[t[k] & kRtState];
    }
  }
  __device__ __forceinline__ uint32_t line_mask(uint32_t acc) const { return acc; }
  // -- the long-line walk: a state is its number
  __device__ __forceinline__ void fill_long() const { rt_fill<RSL>(tab, dm); }
  __device__ __forceinline__ uint32_t step(uint32_t st, uint32_t cp) const {
    const uint32_t sy = cp < 128 ? (uint32_t)sym()[cp] >> 1 : cp_sym(cp);
    return *reinterpret_cast<const uint16_t*>(trans() + (((st << RSL) + sy) << 1));
  }
  __device__ __forceinline__ uint32_t state(uint32_t t) const { return t & kRtState; }
  __device__ __forceinline__ bool accepts(uint32_t t) const { return (t & kRtAcc) != 0; }
  __device__ __forceinline__ uint32_t mask(uint32_t st) const { return out()[st]; }
  __device__ __forceinline__ int warm() const { return dm.warm; }  // the set's longest alternative minus one
};
