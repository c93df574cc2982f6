// Templated messages (edc_tmpl_*, include/edc.h): message i = head[tpl[i]] || var_i || tail[tpl[i]].
// The host-side checks of a template set and of a call's items, and the bound that sizes the
// expansion's arena without a read-back. Plain C++ with no HIP in it, so it can be compiled into a
// stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace edc {

constexpr uint32_t TMPL_MAX_COUNT = 65535;        // tpl[i] is 16 bits
constexpr size_t TMPL_MAX_BLOB = 1u << 20;        // head blob + tail blob, bytes
constexpr size_t TMPL_PAD = 16;                   // k_challenge stages whole aligned 16-byte chunks

// What a checked set is worth to the rest of a call.
struct TmplShape {
  uint32_t head_bytes = 0, tail_bytes = 0;        // blob sizes
  uint32_t max_head = 0, max_tail = 0;            // longest head / tail
};

// count + 1 offsets into one blob: monotone; *bytes = the blob's size (its last offset),
// *longest = the longest piece. False when an offset decreases.
inline bool tmpl_check_offsets(uint32_t count, const uint32_t* off, uint32_t* bytes, uint32_t* longest) {
  uint32_t mx = 0;
  for (uint32_t t = 0; t < count; ++t) {
    if (off[t + 1] < off[t]) return false;
    const uint32_t len = off[t + 1] - off[t];
    mx = len > mx ? len : mx;
  }
  *bytes = off[count];
  *longest = mx;
  return true;
}

// A template set: count in 1..65535, both offset arrays present and monotone, the two blobs at
// most 1 MiB together, and a blob pointer wherever there are bytes.
inline bool tmpl_check_set(uint32_t count, const uint8_t* head, const uint32_t* head_off, const uint8_t* tail,
                           const uint32_t* tail_off, TmplShape* shape) {
  if (count < 1 || count > TMPL_MAX_COUNT || !head_off || !tail_off) return false;
  TmplShape s;
  if (!tmpl_check_offsets(count, head_off, &s.head_bytes, &s.max_head)) return false;
  if (!tmpl_check_offsets(count, tail_off, &s.tail_bytes, &s.max_tail)) return false;
  if ((size_t)s.head_bytes + (size_t)s.tail_bytes > TMPL_MAX_BLOB) return false;
  if ((s.head_bytes && !head) || (s.tail_bytes && !tail)) return false;
  *shape = s;
  return true;
}

// The items of a host call: tpl[i] < count, var_off[0] == 0, var_off monotone.
inline bool tmpl_check_items(uint32_t count, size_t n, const uint16_t* tpl, const uint32_t* var_off) {
  if (!n) return true;
  if (!tpl || !var_off || var_off[0] != 0) return false;
  for (size_t i = 0; i < n; ++i)
    if (tpl[i] >= count || var_off[i + 1] < var_off[i]) return false;
  return true;
}

// Bytes of the arena that holds any n items of a set with this shape and var_bytes of holes:
// every item at its longest, plus the padding behind the last message.
inline size_t tmpl_arena_bound(size_t n, const TmplShape& s, size_t var_bytes) {
  return n * ((size_t)s.max_head + (size_t)s.max_tail) + var_bytes + TMPL_PAD;
}

}  // namespace edc
