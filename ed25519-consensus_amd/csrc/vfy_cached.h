// Host-side bookkeeping of the cached incremental verifier (edc_vfy_set_cached, include/edc.h):
// how many items the queue calls were offered, how many of them the table vouched for, and which
// retained items are already records (the insert watermark). Plain C++ with no HIP in it, so it
// can be compiled into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace edc {

struct CachedState {
  bool on = false;        // configuration: survives edc_verifier_reset
  uint64_t offered = 0;   // items given to queue calls since the last reset
  uint64_t hits = 0;      // of those, skipped as records of the table
  size_t inserted = 0;    // retained items [0, inserted) are records (or were refused by a fallback)
};

// origin is 32 bits per retained item: a queue call of m more items must keep offered below 2^32
inline bool cached_room(const CachedState& c, size_t m) {
  return m <= 0xFFFFFFFFull && c.offered + m <= 0xFFFFFFFFull;
}

// The mode may change only while nothing was offered since create / reset and nothing is retained.
inline bool cached_can_switch(const CachedState& c, size_t retained) { return retained == 0 && c.offered == 0; }

// A queue call offered m items of which `miss` were appended. False (and no change) if miss > m.
inline bool cached_offer(CachedState& c, size_t m, size_t miss) {
  if (miss > m) return false;
  c.offered += m;
  c.hits += m - miss;
  return true;
}

// After a verdict over n retained items: the range [*a, *b) still to insert (false: none).
inline bool cached_insert_due(const CachedState& c, size_t n, size_t* a, size_t* b) {
  if (!c.on || n <= c.inserted) return false;
  *a = c.inserted;
  *b = n;
  return true;
}

inline void cached_insert_done(CachedState& c, size_t b) { c.inserted = b; }

// edc_verifier_reset: the counts and the watermark start over, the mode stays.
inline void cached_reset(CachedState& c) {
  c.offered = c.hits = 0;
  c.inserted = 0;
}

}  // namespace edc
