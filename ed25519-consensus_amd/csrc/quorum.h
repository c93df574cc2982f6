// Quorum commit sets (edc_quorum_*, include/edc.h): a commit set (commits.h) whose items carry a
// voting power and a flag, and whose commits carry a threshold. The host-side checks, the reference
// selection of the checked items (what the device's segmented scan computes) and the reduction from
// (codes, tally, threshold) to per-commit verdicts. Plain C++ with no HIP in it, so it can be
// compiled into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace edc {

constexpr uint8_t QUORUM_ABSENT = 0, QUORUM_COMMIT = 1, QUORUM_NIL = 2;   // EDC_VOTE_*
constexpr int QUORUM_FULL = 0, QUORUM_LIGHT = 1;                          // EDC_QUORUM_*
constexpr uint64_t QUORUM_MAX_POWER = 0x7FFFFFFFFFFFFFFFull;              // one power, and one commit's counted sum
constexpr uint8_t QUORUM_NOT_CHECKED = 255;                               // EDC_NOT_CHECKED
constexpr uint8_t QUORUM_SHORT = 3;                                       // EDC_QUORUM_SHORT

// a + b, UINT64_MAX when it does not fit. Associative and commutative on unsigned values (both
// sides are min(true sum, UINT64_MAX)), so a scan may group the additions in any order.
inline uint64_t quorum_sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? UINT64_MAX : s;
}

inline bool quorum_check_mode(int mode) { return mode == QUORUM_FULL || mode == QUORUM_LIGHT; }

// every flag is EDC_VOTE_ABSENT, _COMMIT or _NIL
inline bool quorum_check_flags(size_t n, const uint8_t* flag) {
  if (n && !flag) return false;
  uint8_t mx = 0;                        // a byte maximum with no early exit: the loop vectorizes
  for (size_t i = 0; i < n; ++i) mx = flag[i] > mx ? flag[i] : mx;
  return mx <= QUORUM_NIL;
}

// every power (counted or not) is at most 2^63 - 1, and so is every commit's sum over its flag-1
// items. The offsets have passed commits_check_offsets, the flags quorum_check_flags.
inline bool quorum_check_powers(size_t nc, const uint32_t* commit_off, const uint64_t* power, const uint8_t* flag) {
  const size_t n = commit_off[nc];
  if (n && !power) return false;
  uint64_t any = 0;
  for (size_t i = 0; i < n; ++i) any |= power[i];
  if (any > QUORUM_MAX_POWER) return false;
  for (size_t c = 0; c < nc; ++c) {
    uint64_t s = 0;
    for (size_t i = commit_off[c]; i < commit_off[c + 1]; ++i)
      s = quorum_sat_add(s, flag[i] == QUORUM_COMMIT ? power[i] : 0);
    if (s > QUORUM_MAX_POWER) return false;
  }
  return true;
}

// The reference selection, on checked inputs. checked[i] (nullable) = 1 iff item i is verified:
//   full mode   flag 1 or 2
//   light mode  flag 1 and the power of the flag-1 items before it in its commit <= threshold[c]
// planned[c] (nullable) = the power of the commit's checked flag-1 items: its tally when all of
// them verify. Returns the number of checked items.
inline size_t quorum_select(size_t nc, const uint32_t* commit_off, const uint64_t* power, const uint8_t* flag,
                            const uint64_t* threshold, int mode, uint8_t* checked, uint64_t* planned) {
  size_t total = 0;
  for (size_t c = 0; c < nc; ++c) {
    uint64_t run = 0;                    // <= 2^63 - 1 by quorum_check_powers
    for (size_t i = commit_off[c]; i < commit_off[c + 1]; ++i) {
      bool chk;
      if (mode == QUORUM_LIGHT) chk = flag[i] == QUORUM_COMMIT && run <= threshold[c];
      else chk = flag[i] != QUORUM_ABSENT;
      if (chk && flag[i] == QUORUM_COMMIT) run += power[i];
      if (checked) checked[i] = chk ? 1 : 0;
      total += chk;
    }
    if (planned) planned[c] = run;
  }
  return total;
}

// Per-commit verdicts. cor[c]: the OR of the codes of the commit's checked items (null: every
// checked item verified). tally[c]: the power of its checked flag-1 items with code 0. Commit c is
// EDC_INVALID_SIGNATURE if cor[c] != 0, else EDC_QUORUM_SHORT if tally[c] <= threshold[c] (strictly
// greater decides: an empty commit is short, also with threshold 0), else EDC_OK.
// commit_verdicts may be null. *n_bad = commits that are not EDC_OK. Returns the set's code: 0 iff
// every commit is, 1 if any commit is invalid, else 3.
inline int quorum_reduce(size_t nc, const uint8_t* cor, const uint64_t* tally, const uint64_t* threshold,
                         uint8_t* commit_verdicts, size_t* n_bad) {
  size_t bad = 0, invalid = 0;
  for (size_t c = 0; c < nc; ++c) {
    const uint8_t v = (cor && cor[c]) ? 1 : tally[c] <= threshold[c] ? QUORUM_SHORT : 0;
    if (commit_verdicts) commit_verdicts[c] = v;
    bad += v != 0;
    invalid += v == 1;
  }
  if (n_bad) *n_bad = bad;
  return invalid ? 1 : bad ? (int)QUORUM_SHORT : 0;
}

// The tally and OR a failed union needs, from the item codes in queue order (QUORUM_NOT_CHECKED
// for the items left out); what the device's tally kernel computes.
inline void quorum_tally(size_t nc, const uint32_t* commit_off, const uint64_t* power, const uint8_t* flag,
                         const uint8_t* codes, uint64_t* tally, uint8_t* cor) {
  for (size_t c = 0; c < nc; ++c) {
    uint64_t t = 0;
    uint8_t o = 0;
    for (size_t i = commit_off[c]; i < commit_off[c + 1]; ++i) {
      if (codes[i] == QUORUM_NOT_CHECKED) continue;
      o |= codes[i];
      if (flag[i] == QUORUM_COMMIT && codes[i] == 0) t += power[i];
    }
    tally[c] = t;
    cor[c] = o;
  }
}

}  // namespace edc
