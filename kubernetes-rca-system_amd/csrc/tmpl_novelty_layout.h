// State of the log-template novelty table (include/krca.h "template novelty"): the
// header, the slot and the report record as the kernels (template_novelty.hip) read and write them,
// the empty markers and the home-slot function.  krca/novelty.py mirrors this file (numpy dtypes and
// home_slot()) for the tests, the snapshots and the export of the live records.
//
// state = NovHeader (256 bytes) | NovSlot[capacity] | int32 touched[capacity]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace krca {

constexpr uint64_t kNovEmptyHash = ~0ull;  // hash word of a slot no key has claimed
constexpr int32_t kNovEmptyGroup = -1;     // group word of such a slot (groups are >= 0)
constexpr uint64_t kNovMagic = 0x314C504D54564F4Eull;  // "NOVTMPL1"
constexpr int kNovHeaderBytes = 256, kNovSlotBytes = 64, kNovReportBytes = 48;
constexpr int kNovLinesBits = 40;  // cur = cur_docs << 40 | cur_lines: one 64-bit add per entry
constexpr int64_t kNovMinCapacity = 64, kNovMaxCapacity = 1ll << 30;
constexpr int64_t kNovMaxDocs = (1ll << (64 - kNovLinesBits)) - 1;
constexpr int32_t kNovNoDoc = INT32_MAX;
constexpr int32_t kNovNovel = 1, kNovSurge = 2;

// a template hash equal to the empty marker is counted under the marker - 1 (the two then share a
// record; tests/template_novelty_ref.py applies the same remap)
__host__ __device__ inline uint64_t nov_remap(uint64_t h) { return h == kNovEmptyHash ? kNovEmptyHash - 1 : h; }

// home slot of key (group, remapped hash) in a table of `capacity` (a power of two) slots; probing is
// linear from there, wrapping.  The mix only spreads the keys: the key itself is compared exactly.
__host__ __device__ inline int64_t nov_home(uint64_t h, int32_t g, int64_t capacity) {
  uint64_t x = h ^ ((uint64_t)(uint32_t)g * 0x9E3779B97F4A7C15ull);
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (int64_t)(x & (uint64_t)(capacity - 1));
}

struct NovSlot {
  uint64_t hash;      // kNovEmptyHash until claimed, then immutable
  int32_t group;      // kNovEmptyGroup until claimed, then immutable
  int32_t first_win;  // the record: window of first sight since the last expiry,
  int32_t last_win;   //   last window with a line,
  int32_t n_win;      //   windows with a line (0 = absent),
  int64_t total;      //   lines
  uint64_t cur;       // this window, zero between calls: cur_docs << kNovLinesBits | cur_lines
  int32_t first_doc;  // this window, kNovNoDoc between calls: the lowest container showing the key
  int32_t flags;      // kNovNovel | kNovSurge of the last window that touched the slot
  uint64_t pad[2];
};
static_assert(sizeof(NovSlot) == kNovSlotBytes, "slot layout");

struct NovHeader {
  uint64_t magic;
  int64_t capacity;
  int64_t n_claimed;  // slots holding a key (records and absent ones)
  int64_t n_live;     // slots with n_win > 0
  // the window's counters, zeroed by every update
  int64_t n_entries;
  int32_t n_touched, overflow, n_novel, n_surge, n_reported, pad0;
  uint64_t pad[24];
};
static_assert(sizeof(NovHeader) == kNovHeaderBytes, "header layout");

struct NovReport {
  uint64_t hash;  // remapped
  int64_t total_before;
  int64_t cur_lines;
  int32_t group, flags, cur_docs, first_doc, first_win, pad;
};
static_assert(sizeof(NovReport) == kNovReportBytes, "report layout");

inline bool nov_capacity_ok(int64_t c) { return c >= kNovMinCapacity && c <= kNovMaxCapacity && (c & (c - 1)) == 0; }
inline int64_t nov_state_bytes(int64_t c) { return (kNovHeaderBytes + c * (kNovSlotBytes + 4) + 255) / 256 * 256; }

}  // namespace krca
