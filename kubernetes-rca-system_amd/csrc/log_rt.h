// Walk, long-line and histogram kernels over pattern tables compiled at RUN TIME (include/krca.h;
// krca/logdfa.py builds the tables).  Included by logscan.hip inside its namespace: siblings of
// log_dfa / log_dfa_long / log_hist, which keep the 13 compiled-in patterns in constant memory and
// whose layout stops at 31 symbols and 512 states.
//
// The table lives in dynamic LDS, a straight copy of the device form (log_rt_layout.h): 16-bit
// entries {target state | kRtAcc} in rows of 32 or 64 columns.  A 32-bit entry carrying the target's
// category mask (log_dfa's form: no accept test at all) fits 160 KiB of LDS only up to 640 states of
// 64 columns, and its 16-bit row offsets stop at 64 KiB; one 16-bit form covers every set inside the
// limits (1024 x 64 x 2 B = 128 KiB) and halves the 13 shipped patterns' table (25 KB for 49 KB).  The
// price: the row offset is rebuilt per step (an AND and a shift-add on the dependent chain where
// log_dfa has one SDWA add) and the category masks come from out[] -- read only for the entries
// flagged kRtAcc, tested once per 16-byte block.
//
// Memory safety: what the fill copies is sanitised (targets clamped to nstate - 1, symbols to the row
// width, masks to ncat bits), so whatever the device form holds, every table index stays below
// nstate << RSL and every out[] index below nstate.
#pragma once

using krca::kRtAcc;
using krca::kRtState;

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

struct RtTab {
  const uint8_t* trans;   // byte-addressed: entry (state, symbol) at ((state << RSL) + symbol) * 2
  const uint16_t* out;
  const uint8_t* sym;    // byte -> symbol * 2
  const uint32_t* rng;
  __device__ __forceinline__ RtTab(const RtDims& dm)
      : trans(rt_lds), out(reinterpret_cast<const uint16_t*>(rt_lds + dm.out_off)), sym(rt_lds + dm.sym_off),
        rng(reinterpret_cast<const uint32_t*>(rt_lds + dm.rng_off)) {}
};

// the symbol of code point cp >= 0x80: binary search of the range table in LDS (nrange <= 1024: the
// probes stay inside the nrange triples whatever they hold)
__device__ __forceinline__ uint32_t rt_cp_sym(const uint32_t* rng, int nrange, uint32_t other, uint32_t cp) {
  uint32_t sy = other;
  int a = 0, z = nrange - 1;
  while (a <= z) {
    const int mid = (a + z) >> 1;
    if (cp < rng[3 * mid]) z = mid - 1;
    else if (cp > rng[3 * mid + 1]) a = mid + 1;
    else {
      sy = rng[3 * mid + 2];
      break;
    }
  }
  return sy;
}

// ---- log_dfa_rt: log_dfa's lockstep walk (16-byte blocks, a ring of three buffer loads, the byte ->
// symbol table with NOP for bytes outside the line and continuation bytes, lead bytes decoded and
// looked up in the range table) over the run-time table
template <int RSL>
__global__ __launch_bounds__(DFA_TPB) void log_dfa_rt(const uint8_t* __restrict__ text, int64_t nbytes, int64_t L,
                                                      const int64_t* __restrict__ Ld, int64_t cap,
                                                      const int64_t* __restrict__ line_start,
                                                      const int64_t* __restrict__ line_end,
                                                      uint32_t* __restrict__ line_mask, int32_t* __restrict__ long_q,
                                                      int32_t* __restrict__ n_long, const uint8_t* __restrict__ tab,
                                                      const RtDims dm) {
  rt_fill<RSL>(tab, dm);
  const RtTab T(dm);
  L = lines_of(L, Ld, cap);
  for (int64_t l0 = (int64_t)blockIdx.x * DFA_TPB; l0 < L; l0 += (int64_t)gridDim.x * DFA_TPB) {
    const int64_t base = line_start[l0] & ~(int64_t)15;
    const int64_t rem = nbytes - base;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(text + base), 0, (int)(rem < (int64_t)INT32_MAX ? rem : (int64_t)INT32_MAX), 0x00020000);
    const int64_t l = l0 + threadIdx.x;
    if (l >= L) continue;
    const int64_t s = line_start[l], e = line_end[l];
    if (e - s > LONG_LINE) {
      long_q[atomicAdd(n_long, 1)] = (int32_t)l;  // a wave per long line (log_dfa_long_rt)
      continue;
    }
    uint32_t st = 0, acc = 0;                     // st: the last entry read (state | flag)
    int off = (int)((s & ~(int64_t)3) - base);
    int rs_ = (int)(s & 3);
    int re_ = (int)(e - (s & ~(int64_t)3));
    const int end_off = (int)min(rem, (int64_t)INT32_MAX);
    auto load = [&](int q) -> uint4 {
      return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, q, 0, 0));
    };
    auto block = [&](uint4& cur, uint4& far) -> bool {
      far = load(off + 32);
      uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
      if (off + 16 > end_off) {  // the text's last bytes (a buffer load straddling the end reads 0)
#pragma unroll 1
        for (int k = 0; k < 16; ++k) {
          const uint32_t b = off + k < end_off ? (uint32_t)text[base + off + k] : 0u;
          w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | (b << (8 * (k & 3)));
        }
      }
      const int lo = max(rs_, 0), hi = min(re_, 16);
      const uint32_t lo4 = (uint32_t)lo * 0x01010101u, hi4x = line_hi4x(hi);
      uint32_t so[16], hib = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t in = word_in_line(j, lo4, hi4x);
        hib |= w[j] & in;
        const uint32_t x = w[j] | (in ^ 0x80808080u);  // outside the line: >= 0x80, NOP
#pragma unroll
        for (int k = 0; k < 4; ++k) so[4 * j + k] = T.sym[(x >> (8 * k)) & 0xFFu];
      }
      if (hib) {  // in-line bytes >= 0x80 (rare): the lead bytes' code points
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
          if (b >= 0xC0 && k >= lo && k < hi) {
            const uint32_t cp = utf8_cp(b, [&](int r) -> uint32_t {
              const int q = k + r;
              if (q < 16) return (w[q >> 2] >> (8 * (q & 3))) & 0xFFu;
              return off + q < end_off ? (uint32_t)text[base + off + q] : 0u;
            });
            so[k] = rt_cp_sym(T.rng, dm.nrange, (uint32_t)dm.other, cp) * 2;
          }
        }
      }
      uint32_t t[16], any = 0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        st = *reinterpret_cast<const uint16_t*>(T.trans + (((st & kRtState) << (RSL + 1)) + so[k]));
        t[k] = st;
        any |= st;
      }
      if (any & kRtAcc) {  // (rare) a category was reported in this block: its mask from out[]
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (t[k] & kRtAcc) acc |= T.out[t[k] & kRtState];
      }
      const bool more = re_ > 16;
      off += 16;
      rs_ -= 16;
      re_ -= 16;
      return more;
    };
    if (s < e) {
      uint4 R0 = load(off), R1 = load(off + 16), R2;
      while (block(R0, R2) && block(R1, R0) && block(R2, R1)) {
      }
    }
    line_mask[l] = acc;
  }
}

// ---- log_dfa_long_rt: a wave per line over 1 KiB, 64 segments, each warmed up over the dm.warm code
// points before it (the set's longest alternative minus one; log_dfa_long's constant is 23)
template <int RSL>
__global__ __launch_bounds__(TPB) void log_dfa_long_rt(const uint8_t* __restrict__ text, int64_t nbytes,
                                                       const int64_t* __restrict__ line_start,
                                                       const int64_t* __restrict__ line_end,
                                                       uint32_t* __restrict__ line_mask,
                                                       const int32_t* __restrict__ long_q,
                                                       const int32_t* __restrict__ n_long,
                                                       const uint8_t* __restrict__ tab, const RtDims dm) {
  const int nq = *n_long;
  if ((int64_t)blockIdx.x * (TPB / 64) >= nq) return;  // no long line for this block: skip the table fill
  rt_fill<RSL>(tab, dm);
  const RtTab T(dm);
  const int lane = threadIdx.x & 63;
  Bytes B;
  B.init(text, nbytes);
  auto symbol = [&](uint32_t cp) -> uint32_t {
    return cp < 128 ? (uint32_t)T.sym[cp] >> 1 : rt_cp_sym(T.rng, dm.nrange, (uint32_t)dm.other, cp);
  };
  auto entry = [&](uint32_t st, uint32_t sy) -> uint32_t {
    return *reinterpret_cast<const uint16_t*>(T.trans + ((((st & kRtState) << RSL) + sy) << 1));
  };
  for (int j = (int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)); j < nq; j += (int)(gridDim.x * (TPB / 64))) {
    const int64_t l = long_q[j];
    const int64_t s = line_start[l], e = line_end[l];
    const int64_t seg = (e - s + 63) / 64;
    const int64_t a = min(e, s + lane * seg), b = min(e, a + seg);
    uint32_t st = 0, mask = 0;
    const int64_t p0 = a > s ? cp_align(B, a, e) : s;  // first code point starting in [a, b)
    if (p0 > s && p0 < b) {  // warm-up over the <= warm code points of the line before p0
      int64_t k = p0;
      int seen = 0;
      while (k > s && seen < dm.warm) {
        const uint32_t c = B.at(k - 1);
        --k;
        if ((c & 0xC0) != 0x80) ++seen;
      }
      while (k < p0) {
        uint32_t cp;
        const int len = decode(B, k, cp);
        st = entry(st, symbol(cp));
        k += len;
      }
    }
    for (int64_t p = p0; p < b;) {
      uint32_t cp;
      const int len = decode(B, p, cp);
      st = entry(st, symbol(cp));
      if (__builtin_expect((st & kRtAcc) != 0, 0)) mask |= T.out[st & kRtState];
      p += len;
    }
    for (int off = 32; off > 0; off >>= 1) mask |= __shfl_xor(mask, off, 64);
    if (lane == 0) line_mask[l] = mask;
  }
}

// ---- log_dfa_long_carry_rt: log_dfa_long_rt for tables with KRCA_LOG_FLAG_CARRY (loop items: a match has
// no longest length, so no warm-up makes a segment's start state right).  Same segments, same warm-up
// and first walk; then the state is carried along the wave.  Per round: prev = the predecessor lane's
// exit state (the start state for lane 0); a wave-wide vote -- executed by all 64 lanes, those with an
// empty segment included -- ends the line when no lane has prev != entry; else the lanes that differ
// take prev as their entry and walk their segment again.  After round r lanes 0..r hold the true
// states, so the loop ends within 63 rounds for every table (the bound is also its trip count).
// Masks of superseded walks stay ORed in: every walk starts from the state that some suffix of the
// text before its segment leads to from the start state, so what it reports is a match inside the
// line, and the last walk of every lane is the true one.  An empty segment hands its entry on.
// Worst case: a state that survives every boundary (".*" armed in segment 0) makes lane r walk in round
// r alone -- one serial walk of the line.  No workspace, no atomics; reads the bytes the first walk reads.
template <int RSL>
__global__ __launch_bounds__(TPB) void log_dfa_long_carry_rt(const uint8_t* __restrict__ text, int64_t nbytes,
                                                             const int64_t* __restrict__ line_start,
                                                             const int64_t* __restrict__ line_end,
                                                             uint32_t* __restrict__ line_mask,
                                                             const int32_t* __restrict__ long_q,
                                                             const int32_t* __restrict__ n_long,
                                                             const uint8_t* __restrict__ tab, const RtDims dm) {
  const int nq = *n_long;
  if ((int64_t)blockIdx.x * (TPB / 64) >= nq) return;  // no long line for this block: skip the table fill
  rt_fill<RSL>(tab, dm);
  const RtTab T(dm);
  const int lane = threadIdx.x & 63;
  Bytes B;
  B.init(text, nbytes);
  auto symbol = [&](uint32_t cp) -> uint32_t {
    return cp < 128 ? (uint32_t)T.sym[cp] >> 1 : rt_cp_sym(T.rng, dm.nrange, (uint32_t)dm.other, cp);
  };
  auto entry = [&](uint32_t st, uint32_t sy) -> uint32_t {
    return *reinterpret_cast<const uint16_t*>(T.trans + ((((st & kRtState) << RSL) + sy) << 1));
  };
  // (j is the same for the 64 lanes of a wave: the shuffles and the vote below run with every lane active)
  for (int j = (int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)); j < nq; j += (int)(gridDim.x * (TPB / 64))) {
    const int64_t l = long_q[j];
    const int64_t s = line_start[l], e = line_end[l];
    const int64_t seg = (e - s + 63) / 64;
    const int64_t a = min(e, s + lane * seg), b = min(e, a + seg);
    uint32_t mask = 0;
    const int64_t p0 = a > s ? cp_align(B, a, e) : s;  // first code point starting in [a, b)
    uint32_t st_in = 0;
    if (p0 > s && p0 < b) {  // warm-up over the <= warm code points of the line before p0 (speculation only)
      int64_t k = p0;
      int seen = 0;
      while (k > s && seen < dm.warm) {
        const uint32_t c = B.at(k - 1);
        --k;
        if ((c & 0xC0) != 0x80) ++seen;
      }
      while (k < p0) {
        uint32_t cp;
        const int len = decode(B, k, cp);
        st_in = entry(st_in, symbol(cp));
        k += len;
      }
      st_in &= kRtState;
    }
    uint32_t st_out = 0;
    bool redo = true;  // round 0: every lane's first walk
    for (int round = 0;; ++round) {
      if (redo) {  // [p0, b) from st_in (an empty segment hands it on)
        uint32_t st = st_in;
        for (int64_t p = p0; p < b;) {
          uint32_t cp;
          const int len = decode(B, p, cp);
          st = entry(st, symbol(cp));
          if (__builtin_expect((st & kRtAcc) != 0, 0)) mask |= T.out[st & kRtState];
          p += len;
        }
        st_out = st & kRtState;
      }
      if (round == 63) break;
      uint32_t prev = __shfl_up(st_out, 1, 64);
      if (lane == 0) prev = 0;
      redo = prev != st_in;
      if (!__any(redo)) break;
      if (redo) st_in = prev;
    }
    for (int off = 32; off > 0; off >>= 1) mask |= __shfl_xor(mask, off, 64);
    if (lane == 0) line_mask[l] = mask;
  }
}

// ---- log_hist_rt: log_hist with the category count as an argument (output stride and loop bounds);
// the per-lane arrays stay sized for KRCA_LOG_MAX_NCAT
constexpr int RT_NC = KRCA_LOG_MAX_NCAT;

template <bool DENSE>
__global__ __launch_bounds__(TPB) void log_hist_rt(const int64_t* __restrict__ doc_off, int64_t D,
                                                   const int64_t* __restrict__ chunk_line0, int64_t nchunks,
                                                   const int64_t* __restrict__ line_start,
                                                   uint32_t* __restrict__ line_mask, int64_t L,
                                                   const int64_t* __restrict__ Ld, int64_t cap,
                                                   int32_t* __restrict__ doc_lines, int32_t* __restrict__ hist,
                                                   int32_t* __restrict__ examples, int64_t* __restrict__ doc_line0,
                                                   const int ncat) {
  __shared__ int32_t s_ex[TPB * RT_NC * (DENSE ? 3 : 1)];
  const uint32_t cat_bits = (1u << ncat) - 1u;
  L = lines_of(L, Ld, cap);
  int32_t mycnt[RT_NC];
#pragma unroll
  for (int c = 0; c < RT_NC; ++c) mycnt[c] = 0;
  const int64_t d0 = (int64_t)blockIdx.x * TPB;
  const int64_t d = d0 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = d < D;
  const int64_t lo = valid ? first_line_at(line_start, L, chunk_line0, nchunks, doc_off[d]) : L;
  int64_t hi = __shfl_down(lo, 1, 64);
  if (valid && (lane == 63 || d + 1 == D)) hi = first_line_at(line_start, L, chunk_line0, nchunks, doc_off[d + 1]);
  const bool small = valid && hi - lo <= HIST_SMALL;
  if (small) {
    int32_t cnt[RT_NC], ex[RT_NC][3];
#pragma unroll
    for (int c = 0; c < RT_NC; ++c) {
      cnt[c] = 0;
      ex[c][0] = ex[c][1] = ex[c][2] = -1;
    }
    uint32_t full = 0;  // bins holding three examples already
    for (int64_t l = lo; l < hi; ++l) {
      const uint32_t m = line_mask[l] & cat_bits;
      const uint32_t exb = m & ~full;
      if (exb) line_mask[l] = m | (exb << EX_SHIFT);
#pragma unroll
      for (int c = 0; c < RT_NC; ++c) {
        if ((m >> c) & 1u) {
          const int f = cnt[c];
          if (DENSE) {
            if (f == 0) ex[c][0] = (int32_t)l;
            if (f == 1) ex[c][1] = (int32_t)l;
            if (f == 2) ex[c][2] = (int32_t)l;
          }
          if (f == 2) full |= 1u << c;
          cnt[c] = f + 1;
        }
      }
    }
    doc_lines[d] = (int32_t)(hi - lo);
    if (doc_line0) doc_line0[d] = lo;
#pragma unroll
    for (int c = 0; c < RT_NC; ++c) mycnt[c] = cnt[c];
    if (DENSE) {
      int32_t* ed = s_ex + threadIdx.x * RT_NC * 3;
#pragma unroll
      for (int c = 0; c < RT_NC; ++c) {
        ed[c * 3] = ex[c][0];
        ed[c * 3 + 1] = ex[c][1];
        ed[c * 3 + 2] = ex[c][2];
      }
    }
  }
  uint64_t big = __ballot(valid && !small);
  const uint64_t below = (1ull << lane) - 1ull;  // lanes before this one
  while (big) {  // wave-uniform: the wave takes the large containers one at a time
    const int j = __ffsll((unsigned long long)big) - 1;
    big &= big - 1;
    const int64_t dj = d - lane + j;
    const int64_t blo = __shfl(lo, j, 64), bhi = __shfl(hi, j, 64);
    int32_t cnt[RT_NC];
#pragma unroll
    for (int c = 0; c < RT_NC; ++c) cnt[c] = 0;
    int32_t* ex = s_ex + (threadIdx.x - lane + j) * RT_NC * 3;
    for (int64_t b = blo; b < bhi; b += 64) {
      const bool in = b + lane < bhi;
      const uint32_t m = in ? (line_mask[b + lane] & cat_bits) : 0u;
      uint32_t exb = 0;
#pragma unroll
      for (int c = 0; c < RT_NC; ++c) {
        const uint64_t bal = __ballot((m >> c) & 1u);
        const int f = cnt[c];  // wave-uniform
        if (((m >> c) & 1u) && f + __popcll(bal & below) < 3) exb |= 1u << c;
        if (DENSE && f < 3) {
          uint64_t bb = bal;
          for (int k = f; k < 3 && bb; ++k) {
            const int q = __ffsll((unsigned long long)bb) - 1;
            if (lane == 0) ex[c * 3 + k] = (int32_t)(b + q);
            bb &= bb - 1;
          }
        }
        cnt[c] = f + __popcll(bal);
      }
      if (exb) line_mask[b + lane] = m | (exb << EX_SHIFT);
    }
    if (lane == j) {
#pragma unroll
      for (int c = 0; c < RT_NC; ++c) mycnt[c] = cnt[c];
    }
    if (lane == 0) {
      doc_lines[dj] = (int32_t)(bhi - blo);
      if (doc_line0) doc_line0[dj] = blo;
      if (DENSE) {
#pragma unroll
        for (int c = 0; c < RT_NC; ++c)
          for (int k = cnt[c] < 3 ? cnt[c] : 3; k < 3; ++k) ex[c * 3 + k] = -1;
      }
    }
  }
  // LDS rows are RT_NC wide, the outputs ncat wide: element i of the block's output is (i / ncat, i % ncat)
  const int nv = (int)(D - d0 < TPB ? D - d0 : TPB);
  if (DENSE) {
    __syncthreads();
    const int row = ncat * 3;
    for (int i = threadIdx.x; i < nv * row; i += TPB) examples[d0 * row + i] = s_ex[(i / row) * RT_NC * 3 + i % row];
  }
  __syncthreads();  // the buffer now takes the histograms
#pragma unroll
  for (int c = 0; c < RT_NC; ++c) s_ex[threadIdx.x * RT_NC + c] = mycnt[c];
  __syncthreads();
  for (int i = threadIdx.x; i < nv * ncat; i += TPB) hist[d0 * ncat + i] = s_ex[(i / ncat) * RT_NC + i % ncat];
}

// ---- launch: LDS the runtime grants, occupancy, the walk, one of the two long-line kernels, the histogram ----
inline RtDims rt_dims(const krca_log_dims& d, const krca::LogRtLayout& l) {
  RtDims r;
  r.ncat = d.ncat, r.nsym = d.nsym, r.nstate = d.nstate, r.nrange = d.nrange, r.warm = d.warm, r.other = d.other;
  r.out_off = l.out_off, r.sym_off = l.sym_off, r.rng_off = l.rng_off, r.bytes = l.bytes;
  return r;
}

// workgroups per CU x CUs for `kernel` with `lds` bytes of dynamic LDS, after opting in above the default
// per-workgroup limit; KRCA_EINVAL (before any launch) when the runtime cannot launch it
inline int rt_prepare(const void* kernel, const char* name, int tpb, uint32_t lds, hipStream_t st, int64_t* resident,
                      std::atomic<uint32_t>& asked) {
  int dev = 0;
  KRCA_HIP(st ? hipStreamGetDevice(st, &dev) : hipGetDevice(&dev));
  int base = 0, cus = 0;
  KRCA_HIP(hipDeviceGetAttribute(&base, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  KRCA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  hipFuncAttributes fa;
  KRCA_HIP(hipFuncGetAttributes(&fa, kernel));
  if ((int64_t)fa.sharedSizeBytes + lds > (int64_t)base) {  // above the default: opt in (the runtime refuses what the CU lacks)
    // never below what an earlier call opted in to (another thread may be launching with it)
    uint32_t want = asked.load();
    while (want < lds && !asked.compare_exchange_weak(want, lds)) {
    }
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(want, lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      krca::set_error("%s: a pattern table of %u bytes of LDS cannot launch on this device (default limit %d bytes, opt-in "
                      "refused: %s)", name, lds, base, hipGetErrorString(e));
      return KRCA_EINVAL;
    }
  }
  int per_cu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, tpb, lds);
  if (e != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    krca::set_error("%s: no workgroup with a pattern table of %u bytes of LDS fits a compute unit of this device", name, lds);
    return KRCA_EINVAL;
  }
  *resident = (int64_t)per_cu * std::max(cus, 1);
  return KRCA_OK;
}

struct RtPlan {  // what krca_log_scan_tables / krca_log_match_tables launch, decided before the first kernel
  RtDims dm;
  int rsl;
  bool carry;  // KRCA_LOG_FLAG_CARRY: long lines go to log_dfa_long_carry_rt
  int64_t walk_resident, long_resident;
};

template <int RSL>
int rt_plan_t(RtPlan& p, hipStream_t st) {
  // the runtime's answers for the last (device, table size) of this thread: a scan per window asks once, not
  // five host queries in front of every scan's first launch
  static thread_local struct { int dev; uint32_t bytes; bool carry; int64_t walk, lng; } last = {-1, 0, false, 0, 0};
  int dev = 0;
  KRCA_HIP(st ? hipStreamGetDevice(st, &dev) : hipGetDevice(&dev));
  if (last.dev == dev && last.bytes == p.dm.bytes && last.carry == p.carry) {
    p.walk_resident = last.walk, p.long_resident = last.lng;
    return KRCA_OK;
  }
  static std::atomic<uint32_t> asked_walk{0}, asked_long{0}, asked_carry{0};  // largest opt-in requested per kernel
  int rc = rt_prepare(reinterpret_cast<const void*>(&log_dfa_rt<RSL>), "log_dfa_rt", DFA_TPB, p.dm.bytes, st, &p.walk_resident,
                      asked_walk);
  if (!rc && !p.carry)
    rc = rt_prepare(reinterpret_cast<const void*>(&log_dfa_long_rt<RSL>), "log_dfa_long_rt", TPB, p.dm.bytes, st,
                    &p.long_resident, asked_long);
  if (!rc && p.carry)
    rc = rt_prepare(reinterpret_cast<const void*>(&log_dfa_long_carry_rt<RSL>), "log_dfa_long_carry_rt", TPB, p.dm.bytes, st,
                    &p.long_resident, asked_carry);
  if (!rc) last = {dev, p.dm.bytes, p.carry, p.walk_resident, p.long_resident};
  return rc;
}

inline int rt_plan(const char* who, const void* tables_dev, int64_t tables_dev_bytes, const krca_log_dims* dims, hipStream_t st,
                   RtPlan& p) {
  KRCA_CHECK_ARG(tables_dev && dims, "%s: null pattern tables", who);
  KRCA_CHECK_ARG(krca::log_dims_ok(*dims), "%s: table dimensions outside the limits of include/krca.h", who);
  const krca::LogRtLayout l = krca::log_rt_layout(*dims);
  KRCA_CHECK_ARG(tables_dev_bytes >= (int64_t)l.bytes, "%s: device tables of %lld bytes, these dimensions need %u", who,
                 (long long)tables_dev_bytes, l.bytes);
  KRCA_CHECK_ARG(((uintptr_t)tables_dev & 3) == 0, "%s: device tables must be 4-byte aligned", who);
  p.dm = rt_dims(*dims, l);
  p.rsl = l.rsl;
  p.carry = (dims->flags & KRCA_LOG_FLAG_CARRY) != 0;
  return l.rsl == 5 ? rt_plan_t<5>(p, st) : rt_plan_t<6>(p, st);
}

template <int RSL>
void rt_launch_walk(const RtPlan& p, hipStream_t st, const uint8_t* text, int64_t nbytes, int64_t L, const int64_t* Ld,
                    int64_t cap, const int64_t* line_start, const int64_t* line_end, uint32_t* line_mask, int32_t* long_q,
                    int32_t* n_long, const uint8_t* tab) {
  const int64_t lines = Ld ? cap : L;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(krca::ceil_div(lines, DFA_TPB), p.walk_resident));
  hipLaunchKernelGGL(log_dfa_rt<RSL>, dim3((unsigned)grid), dim3(DFA_TPB), p.dm.bytes, st, text, nbytes, L, Ld, cap,
                     line_start, line_end, line_mask, long_q, n_long, tab, p.dm);
  const int64_t grid_long = std::max<int64_t>(1, std::min<int64_t>(256, p.long_resident));
  hipLaunchKernelGGL(p.carry ? log_dfa_long_carry_rt<RSL> : log_dfa_long_rt<RSL>, dim3((unsigned)grid_long), dim3(TPB),
                     p.dm.bytes, st, text, nbytes, line_start, line_end, line_mask, (const int32_t*)long_q,
                     (const int32_t*)n_long, tab, p.dm);
}
