// Validator-set quorum commit sets (edc_valset_*, include/edc.h): a quorum commit set (quorum.h)
// whose powers come from the registered validator list and whose commits are refused when one
// validator has two checked votes in them. The host-side checks of the powers, the reference join
// of the votes against the list (what the device's resolve kernel computes), the reference
// double-vote scan (what the device's pair set computes) and the reduction to per-commit verdicts.
// Plain C++ with no HIP in it, so it can be compiled into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "quorum.h"

namespace edc {

constexpr uint8_t VALSET_DOUBLE_VOTE = 4;            // EDC_DOUBLE_VOTE
constexpr uint32_t VALSET_NO_POS = 0xFFFFFFFFu;      // pos[i] of a signer that is not a member

// every power is at most 2^63 - 1, and so is their sum
inline bool valset_check_powers(size_t m, const uint64_t* power) {
  if (m && !power) return false;
  uint64_t s = 0;
  for (size_t p = 0; p < m; ++p) {
    if (power[p] > QUORUM_MAX_POWER) return false;
    s = quorum_sat_add(s, power[p]);
  }
  return s <= QUORUM_MAX_POWER;
}

// positions of the m keys (32 bytes each) ordered by their bytes, equal keys by position
inline std::vector<uint32_t> valset_sorted(size_t m, const uint8_t* vk) {
  std::vector<uint32_t> ord(m);
  for (size_t p = 0; p < m; ++p) ord[p] = (uint32_t)p;
  std::sort(ord.begin(), ord.end(), [vk](uint32_t a, uint32_t b) {
    const int c = memcmp(vk + 32 * (size_t)a, vk + 32 * (size_t)b, 32);
    return c ? c < 0 : a < b;
  });
  return ord;
}

// no two positions of the list hold the same key
inline bool valset_keys_distinct(size_t m, const uint8_t* vk) {
  const std::vector<uint32_t> ord = valset_sorted(m, vk);
  for (size_t j = 1; j < m; ++j)
    if (!memcmp(vk + 32 * (size_t)ord[j - 1], vk + 32 * (size_t)ord[j], 32)) return false;
  return true;
}

// The reference join. The list: m distinct keys set_vk with powers set_power. The votes: n items
// given by their key bytes (vk, n x 32) or by their position in the list (key_idx, every entry
// < m); exactly one of the two. Outputs, all nullable: pos[i] = the signer's position or
// VALSET_NO_POS, power[i] = its power or 0, flag_out[i] = flag[i] for a member, QUORUM_ABSENT for
// a signer the list does not know.
inline void valset_resolve(size_t m, const uint8_t* set_vk, const uint64_t* set_power, size_t n, const uint8_t* vk,
                           const uint32_t* key_idx, const uint8_t* flag, uint32_t* pos, uint64_t* power,
                           uint8_t* flag_out) {
  std::vector<uint32_t> ord;
  if (!key_idx) ord = valset_sorted(m, set_vk);
  for (size_t i = 0; i < n; ++i) {
    uint32_t p = VALSET_NO_POS;
    if (key_idx) {
      p = key_idx[i];
    } else {
      const uint8_t* key = vk + 32 * i;
      size_t lo = 0, hi = m;               // first sorted key that is not below `key`
      while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (memcmp(set_vk + 32 * (size_t)ord[mid], key, 32) < 0) lo = mid + 1;
        else hi = mid;
      }
      if (lo < m && !memcmp(set_vk + 32 * (size_t)ord[lo], key, 32)) p = ord[lo];
    }
    if (pos) pos[i] = p;
    if (power) power[i] = p == VALSET_NO_POS ? 0 : set_power[p];
    if (flag_out) flag_out[i] = p == VALSET_NO_POS ? QUORUM_ABSENT : flag[i];
  }
}

// dv[c] = 1 iff two CHECKED items of commit c have the same position (a member: an item whose
// signer is not a member is never checked, and VALSET_NO_POS is left out all the same). Returns
// the number of such commits.
inline size_t valset_double_votes(size_t nc, const uint32_t* commit_off, const uint32_t* pos, const uint8_t* checked,
                                  uint8_t* dv) {
  size_t total = 0;
  std::vector<uint32_t> seen;
  for (size_t c = 0; c < nc; ++c) {
    seen.clear();
    for (size_t i = commit_off[c]; i < commit_off[c + 1]; ++i)
      if (checked[i] && pos[i] != VALSET_NO_POS) seen.push_back(pos[i]);
    std::sort(seen.begin(), seen.end());
    const bool twice = std::adjacent_find(seen.begin(), seen.end()) != seen.end();
    if (dv) dv[c] = twice ? 1 : 0;
    total += twice;
  }
  return total;
}

// Per-commit verdicts: quorum_reduce's, then EDC_DOUBLE_VOTE for every commit with dv[c] != 0,
// whatever else holds for it (dv null: none). commit_verdicts may be null. *n_bad = commits that
// are not EDC_OK. Returns the set's code: 0 iff every commit is, else 1 if any commit is invalid,
// else 4 if any commit holds a double vote, else 3.
inline int valset_reduce(size_t nc, const uint8_t* cor, const uint64_t* tally, const uint64_t* threshold,
                         const uint8_t* dv, uint8_t* commit_verdicts, size_t* n_bad) {
  std::vector<uint8_t> v(nc ? nc : 1);
  quorum_reduce(nc, cor, tally, threshold, v.data(), nullptr);
  size_t bad = 0, invalid = 0, twice = 0;
  for (size_t c = 0; c < nc; ++c) {
    if (dv && dv[c]) v[c] = VALSET_DOUBLE_VOTE;
    bad += v[c] != 0;
    invalid += v[c] == 1;
    twice += v[c] == VALSET_DOUBLE_VOTE;
    if (commit_verdicts) commit_verdicts[c] = v[c];
  }
  if (n_bad) *n_bad = bad;
  return invalid ? 1 : twice ? (int)VALSET_DOUBLE_VOTE : bad ? (int)QUORUM_SHORT : 0;
}

}  // namespace edc
