// Device form of run-time log pattern tables (include/krca.h, "pattern tables compiled at run
// time"): the LDS layout of log_dfa / log_dfa_long over TabRt, shared by the host packer
// (log_tables.cpp) and the table policy (log_rt.h).  All offsets in bytes, multiples of 16.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/krca.h"

namespace krca {

constexpr uint32_t kRtAcc = 0x8000u;     // entry flag: the target state reports a category
constexpr uint32_t kRtState = 0x3FFu;    // entry bits of the target state (KRCA_LOG_MAX_NSTATE = 1024)

struct LogRtLayout {
  int rsl;            // log2 of the columns per state row: 5 (nsym <= 31) or 6
  uint32_t out_off;   // uint16 out[nstate]           (trans uint16[nstate << rsl] sits at 0)
  uint32_t sym_off;   // uint8  sym[256]: byte -> symbol (bytes >= 0x80 and separators -> the identity column)
  uint32_t rng_off;   // uint32 rng[nrange][3]
  uint32_t bytes;     // the whole form
};

inline bool log_dims_ok(const krca_log_dims& d) {
  return d.ncat >= 1 && d.ncat <= KRCA_LOG_MAX_NCAT && d.nsym >= 1 && d.nsym <= KRCA_LOG_MAX_NSYM && d.nstate >= 1 &&
         d.nstate <= KRCA_LOG_MAX_NSTATE && d.nrange >= 0 && d.nrange <= KRCA_LOG_MAX_NRANGE && d.warm >= 0 &&
         d.warm <= KRCA_LOG_MAX_WARM && d.other >= 0 && d.other < d.nsym && (d.flags & ~KRCA_LOG_FLAG_CARRY) == 0;
}

inline LogRtLayout log_rt_layout(const krca_log_dims& d) {
  auto up16 = [](uint32_t x) { return (x + 15u) & ~15u; };
  LogRtLayout l;
  l.rsl = d.nsym <= 31 ? 5 : 6;
  l.out_off = up16(((uint32_t)d.nstate << l.rsl) * 2u);
  l.sym_off = up16(l.out_off + (uint32_t)d.nstate * 2u);
  l.rng_off = l.sym_off + 256u;
  l.bytes = up16(l.rng_off + (uint32_t)d.nrange * 12u);
  return l;
}

// writes the device form of a VALIDATED image (krca_log_tables_check) to out[log_rt_layout(d).bytes]
void log_tables_pack(const void* image, const krca_log_dims& d, uint8_t* out);

}  // namespace krca
