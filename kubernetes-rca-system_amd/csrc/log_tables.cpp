// Run-time log pattern tables, host side (include/krca.h): validation of a table image and its
// packing into the device form the walk kernels copy into LDS.  Host only: callable without a GPU.
#include <string.h>

#include <vector>

#include "krca_common.h"
#include "log_rt_layout.h"

namespace {

constexpr int64_t kHeader = 48, kAscii = 128;

uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

struct ImageView {
  const uint8_t *ascii, *ranges, *trans, *out;
};

ImageView view(const uint8_t* im, const krca_log_dims& d) {
  ImageView v;
  v.ascii = im + kHeader;
  v.ranges = v.ascii + kAscii;
  v.trans = v.ranges + (int64_t)d.nrange * 12;
  v.out = v.trans + (int64_t)d.nstate * d.nsym * 2;
  return v;
}

}  // namespace

namespace krca {

void log_tables_pack(const void* image, const krca_log_dims& d, uint8_t* out) {
  const uint8_t* im = static_cast<const uint8_t*>(image);
  const ImageView v = view(im, d);
  const LogRtLayout l = log_rt_layout(d);
  memset(out, 0, l.bytes);
  const int rs = 1 << l.rsl, nop = rs - 1;
  uint16_t* trans = reinterpret_cast<uint16_t*>(out);
  for (int s = 0; s < d.nstate; ++s)
    for (int c = 0; c < rs; ++c) {  // the symbols, then identity columns up to the row width
      const uint32_t t = c < d.nsym ? rd16(v.trans + ((int64_t)s * d.nsym + c) * 2) : (uint32_t)s;
      trans[(s << l.rsl) + c] = (uint16_t)(t | (rd16(v.out + 2 * t) ? kRtAcc : 0u));
    }
  for (int s = 0; s < d.nstate; ++s) {
    const uint16_t m = (uint16_t)rd16(v.out + 2 * s);
    memcpy(out + l.out_off + 2 * s, &m, 2);
  }
  for (int b = 0; b < 256; ++b) {  // no separator inside a line; bytes >= 0x80: lead bytes are decoded by the walk
    const uint32_t sy = b < 128 ? v.ascii[b] : (uint32_t)nop;
    out[l.sym_off + b] = (uint8_t)(sy == KRCA_LOG_SYM_SEP ? (uint32_t)nop : sy);
  }
  for (int i = 0; i < 3 * d.nrange; ++i) {
    uint32_t x = rd32(v.ranges + 4 * i);
    if (i % 3 == 2 && x == KRCA_LOG_SYM_SEP) x = (uint32_t)nop;  // (never met inside a line)
    memcpy(out + l.rng_off + 4 * i, &x, 4);
  }
}

}  // namespace krca

extern "C" {

int krca_log_tables_check(const void* image_host, int64_t image_bytes, krca_log_dims* dims_host) {
  KRCA_CHECK_ARG(image_host && image_bytes >= kHeader, "krca_log_tables_check: image of %lld bytes is shorter than its header",
                 (long long)image_bytes);
  const uint8_t* im = static_cast<const uint8_t*>(image_host);
  KRCA_CHECK_ARG(rd32(im) == KRCA_LOG_IMAGE_MAGIC, "krca_log_tables_check: bad magic 0x%08X", rd32(im));
  KRCA_CHECK_ARG(rd32(im + 4) == KRCA_LOG_IMAGE_VERSION, "krca_log_tables_check: image version %u, this library reads %u",
                 rd32(im + 4), KRCA_LOG_IMAGE_VERSION);
  uint32_t h[6];
  for (int i = 0; i < 6; ++i) h[i] = rd32(im + 8 + 4 * i);
  KRCA_CHECK_ARG(h[0] >= 1 && h[0] <= KRCA_LOG_MAX_NCAT, "krca_log_tables_check: ncat %u outside 1..%d", h[0], KRCA_LOG_MAX_NCAT);
  KRCA_CHECK_ARG(h[1] >= 1 && h[1] <= KRCA_LOG_MAX_NSYM, "krca_log_tables_check: nsym %u outside 1..%d", h[1], KRCA_LOG_MAX_NSYM);
  KRCA_CHECK_ARG(h[2] >= 1 && h[2] <= KRCA_LOG_MAX_NSTATE, "krca_log_tables_check: nstate %u outside 1..%d", h[2],
                 KRCA_LOG_MAX_NSTATE);
  KRCA_CHECK_ARG(h[3] <= KRCA_LOG_MAX_NRANGE, "krca_log_tables_check: nrange %u above %d", h[3], KRCA_LOG_MAX_NRANGE);
  KRCA_CHECK_ARG(h[4] <= KRCA_LOG_MAX_WARM, "krca_log_tables_check: warm %u above %d", h[4], KRCA_LOG_MAX_WARM);
  KRCA_CHECK_ARG(h[5] < h[1], "krca_log_tables_check: symbol %u of unlisted code points is not below nsym %u", h[5], h[1]);
  krca_log_dims d;
  d.ncat = (int32_t)h[0], d.nsym = (int32_t)h[1], d.nstate = (int32_t)h[2], d.nrange = (int32_t)h[3];
  d.warm = (int32_t)h[4], d.other = (int32_t)h[5];
  d.digest = (uint64_t)rd32(im + 32) | (uint64_t)rd32(im + 36) << 32;
  int64_t need = kHeader + kAscii + (int64_t)d.nrange * 12 + (int64_t)d.nstate * d.nsym * 2 + (int64_t)d.nstate * 2;
  need = (need + 7) & ~(int64_t)7;
  KRCA_CHECK_ARG(rd32(im + 40) == need, "krca_log_tables_check: header says %u bytes, its dimensions need %lld",
                 rd32(im + 40), (long long)need);
  d.flags = rd32(im + 44);
  KRCA_CHECK_ARG((d.flags & ~KRCA_LOG_FLAG_CARRY) == 0, "krca_log_tables_check: flags 0x%X has a bit this library does not know",
                 d.flags);
  KRCA_CHECK_ARG(image_bytes >= need, "krca_log_tables_check: truncated image: %lld bytes of %lld", (long long)image_bytes,
                 (long long)need);
  const ImageView v = view(im, d);
  for (int c = 0; c < 128; ++c)
    KRCA_CHECK_ARG(v.ascii[c] < d.nsym || v.ascii[c] == KRCA_LOG_SYM_SEP, "krca_log_tables_check: ascii_sym[%d] = %u is no symbol",
                   c, v.ascii[c]);
  uint32_t prev = 0x7F;
  for (int r = 0; r < d.nrange; ++r) {
    const uint32_t lo = rd32(v.ranges + 12 * r), hi = rd32(v.ranges + 12 * r + 4), sy = rd32(v.ranges + 12 * r + 8);
    KRCA_CHECK_ARG(lo > prev && hi >= lo && hi < 0x110000u,
                   "krca_log_tables_check: range %d [0x%X, 0x%X] is not sorted, disjoint and inside 0x80..0x10FFFF", r, lo, hi);
    KRCA_CHECK_ARG(sy < (uint32_t)d.nsym || sy == KRCA_LOG_SYM_SEP, "krca_log_tables_check: range %d has symbol %u", r, sy);
    prev = hi;
  }
  const int64_t nt = (int64_t)d.nstate * d.nsym;
  for (int64_t i = 0; i < nt; ++i)
    KRCA_CHECK_ARG(rd16(v.trans + 2 * i) < (uint32_t)d.nstate, "krca_log_tables_check: transition %lld goes to state %u of %d",
                   (long long)i, rd16(v.trans + 2 * i), d.nstate);
  for (int s = 0; s < d.nstate; ++s)
    KRCA_CHECK_ARG(rd16(v.out + 2 * s) < (1u << d.ncat), "krca_log_tables_check: out[%d] = 0x%X has a bit at or above ncat %d", s,
                   rd16(v.out + 2 * s), d.ncat);
  if (dims_host) *dims_host = d;
  return KRCA_OK;
}

int64_t krca_log_tables_dev_size(const krca_log_dims* dims_host) {
  if (!dims_host || !krca::log_dims_ok(*dims_host)) return 0;
  return krca::log_rt_layout(*dims_host).bytes;
}

}  // extern "C"
