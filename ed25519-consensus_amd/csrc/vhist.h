// Validator-set history (edc_vhist_*, include/edc.h): the validator set as a base set plus
// per-version updates, so that every commit of a commit set is judged by the set of its own height.
// The host-side checks of a history, its per-position change lists in CSR form (what the device's
// resolve kernel searches), the per-version totals and the reference lookup.
// Plain C++ with no HIP in it, so it can be compiled into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "quorum.h"

namespace edc {

constexpr uint64_t VHIST_NOT_MEMBER = ~0ull;         // EDC_VHIST_NOT_MEMBER

// Position p's change list is the entries [off[p], off[p+1]): ver[] ascending from the base's 0,
// one entry per update of p (an update that restates the state is an entry like any other), pow[]
// the power from that version on or VHIST_NOT_MEMBER. total[v] / members[v]: the sum of the member
// powers and the member count at version v, nv + 1 of each.
struct VHist {
  uint32_t m = 0, nv = 0;
  std::vector<uint32_t> off, ver;
  std::vector<uint64_t> pow;
  std::vector<uint64_t> total;
  std::vector<uint32_t> members;
};

// Checks and builds the history of the registered list of list_m positions, whose keys have the
// identities key_id (list_m of them, equal for equal keys): version 0 is base_power (m entries),
// version v (1..nv) is version v-1 with the updates [upd_off[v-1], upd_off[v]) applied (position
// upd_pos[j] gets upd_power[j]). False, with *why a reason and *out untouched, if there is no list
// or m is not its length, two positions hold the same key, upd_off is not monotone from 0, m plus
// the update count or nv + 1 reaches 2^32, an update position is >= m, a position occurs twice
// inside one version's slice, a power other than VHIST_NOT_MEMBER is above 2^63 - 1 or the member
// powers of a version sum to more than 2^63 - 1.
inline bool vhist_build(size_t list_m, const uint32_t* key_id, size_t m, const uint64_t* base_power, size_t nv,
                        const uint32_t* upd_off, const uint32_t* upd_pos, const uint64_t* upd_power, VHist* out,
                        const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  if (!list_m || !key_id) { *why = "no registered key list (edc_keycache_load)"; return false; }
  if (m != list_m || !base_power) { *why = "one base power per position of the registered key list"; return false; }
  if (nv >= 0xFFFFFFFFull || (nv && !upd_off)) { *why = "validator updates: nv + 1 offsets, fewer than 2^32 - 1 versions"; return false; }
  if (nv && upd_off[0] != 0) { *why = "validator updates: offsets not monotone from 0"; return false; }
  for (size_t v = 0; v < nv; ++v)
    if (upd_off[v + 1] < upd_off[v]) { *why = "validator updates: offsets not monotone from 0"; return false; }
  const size_t nu = nv ? upd_off[nv] : 0;
  if ((uint64_t)m + nu >= (1ull << 32)) { *why = "validator history: positions plus updates reach 2^32"; return false; }
  if (nu && (!upd_pos || !upd_power)) { *why = "null input"; return false; }
  std::vector<uint32_t> ids(key_id, key_id + m);
  std::sort(ids.begin(), ids.end());
  if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) {
    *why = "the registered key list holds a key twice: not a validator set";
    return false;
  }
  VHist h;
  h.m = (uint32_t)m;
  h.nv = (uint32_t)nv;
  h.off.assign(m + 1, 0);
  for (size_t j = 0; j < nu; ++j) {
    if (upd_pos[j] >= m) { *why = "validator updates: a position outside the list"; return false; }
    h.off[upd_pos[j] + 1]++;
  }
  for (size_t p = 0; p < m; ++p) h.off[p + 1] += h.off[p] + 1;        // the base entry and the updates
  h.ver.resize(m + nu);
  h.pow.resize(m + nu);
  h.total.resize(nv + 1);
  h.members.resize(nv + 1);
  std::vector<uint32_t> fill(h.off.begin(), h.off.end() - 1), seen(m, 0);
  std::vector<uint64_t> cur(base_power, base_power + m);
  unsigned __int128 sum = 0;            // a slice's running sum may pass 2^64 before its last update
  uint32_t cnt = 0;
  for (size_t p = 0; p < m; ++p) {
    if (cur[p] != VHIST_NOT_MEMBER) {
      if (cur[p] > QUORUM_MAX_POWER) { *why = "voting power: every power at most 2^63 - 1"; return false; }
      sum += cur[p];
      cnt++;
    }
    h.ver[fill[p]] = 0;
    h.pow[fill[p]++] = cur[p];
  }
  for (size_t v = 0;; ++v) {
    if (sum > QUORUM_MAX_POWER) { *why = "voting power: the members of every version sum to at most 2^63 - 1"; return false; }
    h.total[v] = (uint64_t)sum;
    h.members[v] = cnt;
    if (v == nv) break;
    for (size_t j = upd_off[v]; j < upd_off[v + 1]; ++j) {
      const uint32_t p = upd_pos[j];
      const uint64_t w = upd_power[j];
      if (seen[p] == v + 1) { *why = "validator updates: a position twice in one version"; return false; }
      seen[p] = (uint32_t)(v + 1);
      if (w != VHIST_NOT_MEMBER && w > QUORUM_MAX_POWER) { *why = "voting power: every power at most 2^63 - 1"; return false; }
      if (cur[p] != VHIST_NOT_MEMBER) { sum -= cur[p]; cnt--; }
      if (w != VHIST_NOT_MEMBER) { sum += w; cnt++; }
      cur[p] = w;
      h.ver[fill[p]] = (uint32_t)(v + 1);
      h.pow[fill[p]++] = w;
    }
  }
  *out = std::move(h);
  return true;
}

// the reference lookup: position p's power at version v, the last entry of its list with
// ver <= v (VHIST_NOT_MEMBER: not a member then). p < m.
inline uint64_t vhist_power_at(const VHist& h, uint32_t p, uint32_t v) {
  uint32_t lo = h.off[p], hi = h.off[p + 1] - 1;      // ver[lo] = 0 <= v
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (h.ver[mid] <= v) lo = mid;
    else hi = mid - 1;
  }
  return h.pow[lo];
}

// Trusting pairs (edc_vq_verify with trust_ver, include/edc.h): one commit set judged by two sets at
// once, side A at commit_ver[c] and side B at trust_ver[c]. VQ_NO_TRUST as trust_ver[c] gives commit
// c side A only.
constexpr uint32_t VQ_NO_TRUST = 0xFFFFFFFFu;        // EDC_VQ_NO_TRUST

// every trust version is one of the history's or the sentinel
inline bool vq_trust_check_versions(size_t nc, const uint32_t* trust_ver, uint32_t nv) {
  for (size_t c = 0; c < nc; ++c)
    if (trust_ver[c] > nv && trust_ver[c] != VQ_NO_TRUST) return false;
  return true;
}

// The reference union of two selections over the same n items (checked_a / checked_b: what
// quorum_select gives each side). side[i] (nullable) = bit 0 checked by A | bit 1 checked by B; a
// vote is verified iff side[i] != 0. counts (nullable) = {A, B, both, union}. Returns the union's size.
inline size_t vq_trust_union(size_t n, const uint8_t* checked_a, const uint8_t* checked_b, uint8_t* side,
                             uint64_t counts[4]) {
  uint64_t a = 0, b = 0, ab = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool ca = checked_a[i] != 0, cb = checked_b[i] != 0;
    if (side) side[i] = (uint8_t)((ca ? 1 : 0) | (cb ? 2 : 0));
    a += ca;
    b += cb;
    ab += ca && cb;
  }
  if (counts) {
    counts[0] = a;
    counts[1] = b;
    counts[2] = ab;
    counts[3] = a + b - ab;
  }
  return (size_t)(a + b - ab);
}

// quorum_tally for one side of a pair: the codes are the union's, and the side counts item i iff
// bit `bit` (0: A, 1: B) of side[i] is set, with its own power and flag.
inline void vq_trust_tally(size_t nc, const uint32_t* commit_off, const uint8_t* side, int bit, const uint64_t* power,
                           const uint8_t* flag, const uint8_t* codes, uint64_t* tally, uint8_t* cor) {
  for (size_t c = 0; c < nc; ++c) {
    uint64_t t = 0;
    uint8_t o = 0;
    for (size_t i = commit_off[c]; i < commit_off[c + 1]; ++i) {
      if (codes[i] == QUORUM_NOT_CHECKED || !((side[i] >> bit) & 1)) continue;
      o |= codes[i];
      if (flag[i] == QUORUM_COMMIT && codes[i] == 0) t += power[i];
    }
    tally[c] = t;
    cor[c] = o;
  }
}

// Side B's verdicts: per commit what quorum_reduce gives, EDC_DOUBLE_VOTE (4) where dv[c] != 0 (dv
// null: none), and for a commit whose trust_ver[c] is VQ_NO_TRUST the verdict EDC_OK with tally[c]
// set to 0, whatever the threshold. tally is in / out for that reason. commit_verdicts may be
// null. *n_bad = commits that are not EDC_OK. Returns the side's code: 0, else 1 over 4 over 3.
inline int vq_trust_reduce(size_t nc, const uint32_t* trust_ver, const uint8_t* cor, uint64_t* tally,
                           const uint64_t* threshold, const uint8_t* dv, uint8_t* commit_verdicts, size_t* n_bad) {
  size_t bad = 0, invalid = 0, twice = 0;
  for (size_t c = 0; c < nc; ++c) {
    uint8_t v;
    if (trust_ver[c] == VQ_NO_TRUST) {
      tally[c] = 0;
      v = 0;
    } else {
      v = (cor && cor[c]) ? 1 : tally[c] <= threshold[c] ? QUORUM_SHORT : 0;
      if (dv && dv[c]) v = 4;
    }
    bad += v != 0;
    invalid += v == 1;
    twice += v == 4;
    if (commit_verdicts) commit_verdicts[c] = v;
  }
  if (n_bad) *n_bad = bad;
  return invalid ? 1 : twice ? 4 : bad ? (int)QUORUM_SHORT : 0;
}

// the code of a pair from its sides' codes (each 0, 1, 3 or 4): 0 iff both are, else 1 over 4 over 3
inline int vq_trust_code(int a, int b) {
  if (a == 1 || b == 1) return 1;
  if (a == 4 || b == 4) return 4;
  return (a || b) ? (int)QUORUM_SHORT : 0;
}

}  // namespace edc
