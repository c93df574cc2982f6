// Commit sets (edc_commits_*, include/edc.h): n items in queue order cut into nc commits by nc + 1
// offsets, each commit its own batch::Verifier (reference src/batch.rs:110-217). The host-side
// checks of the offsets and of a templated set's per-commit templates and holes, and the reduction
// from per-item codes to per-commit verdicts. Plain C++ with no HIP in it, so it can be compiled
// into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace edc {

constexpr uint64_t COMMITS_MAX_ITEMS = 1ull << 28;   // one launch holds fewer items than this

// nc + 1 offsets (nc >= 1): commit_off[0] == 0, monotone, commit_off[nc] < 2^28. *n = the item
// count (the last offset). Empty commits (repeated offsets) are allowed.
inline bool commits_check_offsets(size_t nc, const uint32_t* commit_off, size_t* n) {
  if (nc < 1 || !commit_off || commit_off[0] != 0) return false;
  for (size_t c = 0; c < nc; ++c)
    if (commit_off[c + 1] < commit_off[c]) return false;
  if ((uint64_t)commit_off[nc] >= COMMITS_MAX_ITEMS) return false;
  *n = commit_off[nc];
  return true;
}

// One template per commit: commit_tpl[c] < count for every commit, empty ones included.
inline bool commits_check_tpl(uint32_t count, size_t nc, const uint16_t* commit_tpl) {
  if (!commit_tpl) return false;
  for (size_t c = 0; c < nc; ++c)
    if (commit_tpl[c] >= count) return false;
  return true;
}

// Template variants (edc_tmpl_commits_*_alt / _device): every commit, empty ones included, owns
// the window [commit_tpl[c], commit_tpl[c] + alt_span) of the set, alt_span in 1..COMMITS_MAX_ALT_SPAN
// (a variant is one byte), and the whole window lies inside the set.
constexpr uint32_t COMMITS_MAX_ALT_SPAN = 256;

inline bool commits_check_alt_span(uint32_t count, size_t nc, const uint16_t* commit_tpl, uint32_t alt_span) {
  if (!commit_tpl || alt_span < 1 || alt_span > COMMITS_MAX_ALT_SPAN) return false;
  for (size_t c = 0; c < nc; ++c)
    if ((uint64_t)commit_tpl[c] + alt_span > count) return false;
  return true;
}

// item_alt[i] < alt_span for every item; a null item_alt is n zeros.
inline bool commits_check_item_alt(size_t n, const uint8_t* item_alt, uint32_t alt_span) {
  if (alt_span < 1) return false;
  if (!item_alt) return true;
  uint8_t mx = 0;                        // a byte maximum with no early exit: the loop vectorizes 16 items wide
  for (size_t i = 0; i < n; ++i) mx = item_alt[i] > mx ? item_alt[i] : mx;
  return (uint32_t)mx < alt_span;
}

// The holes of a templated commit set (tmpl_check_items without the per-item template array,
// which such a call does not have): var_off[0] == 0, monotone.
inline bool commits_check_holes(size_t n, const uint32_t* var_off) {
  if (!n) return true;
  if (!var_off || var_off[0] != 0) return false;
  for (size_t i = 0; i < n; ++i)
    if (var_off[i + 1] < var_off[i]) return false;
  return true;
}

// Per-item codes (Item::verify_single, 0 = Ok) -> per-commit verdicts: commit c is 1
// (InvalidSignature: Verifier::verify reports a malformed key so too) iff one of its items has a
// non-zero code, else 0; an empty commit is 0. codes may be null (a launch that passed: every item
// Ok). commit_verdicts may be null. Returns the number of commits that are not Ok.
inline size_t commits_reduce(size_t nc, const uint32_t* commit_off, const uint8_t* codes, uint8_t* commit_verdicts) {
  size_t bad = 0;
  for (size_t c = 0; c < nc; ++c) {
    uint8_t any = 0;                     // OR of the commit's codes: no early exit, so the loop vectorizes
    if (codes)
      for (size_t i = commit_off[c]; i < commit_off[c + 1]; ++i) any |= codes[i];
    const uint8_t v = any ? 1 : 0;
    if (commit_verdicts) commit_verdicts[c] = v;
    bad += v;
  }
  return bad;
}

}  // namespace edc
