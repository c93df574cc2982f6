// Header hashes (edc_header_*, include/edc.h): the Merkle root of a block header given as its
// ordered leaves, and the byte rules that bind a header to validator-set roots and to another
// header. The host reference: the recursive RFC 6962 root over leaves of any length and the four
// rules, on the byte-wise SHA-256 of valhash.h. The device kernels (sha256.h's streaming leaf hash,
// edc_header.hip) are written separately and are held to this file by the tests.
// Plain C++ with no HIP in it, so it can be compiled into a stand-alone host program.
//
// The function (agreement with CometBFT's Header.Hash() is the intent, stated from memory):
//   root    RFC 6962's MTH with SHA-256 over the header's leaves: no leaf -> SHA-256(""), one leaf
//           -> SHA-256(00 | leaf), n > 1 -> SHA-256(01 | MTH(first k) | MTH(rest)), k the largest
//           power of two below n
//   rule    (leaf L, position P, source S) holds for a header of n leaves iff L < n, leaf L has at
//           least P + 32 bytes and the 32 bytes from P equal S
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "valhash.h"

namespace edc {

constexpr uint32_t HEADER_MAX_LEAVES = 64;            // EDC_HEADER_MAX_LEAVES
constexpr uint32_t HEADER_NONE = 0xFFFFFFFFu;         // EDC_HEADER_NONE
constexpr uint8_t HEADER_BAD_HASH = 1, HEADER_BAD_VALS = 2, HEADER_BAD_NEXT = 4, HEADER_BAD_LINK = 8;

// nh headers: header h owns the leaves [leaf_off[h], leaf_off[h + 1]), leaf j the bytes
// [byte_off[j], byte_off[j + 1])
struct HdrSet {
  size_t nh;
  const uint32_t* leaf_off;
  const uint32_t* byte_off;
  const uint8_t* bytes;
};

// MTH over the n leaves from leaf `first`, by the recursive definition
inline void hdrhash_mth(const HdrSet& s, size_t first, size_t n, uint8_t out[32]) {
  if (n == 0) {
    valhash_sha256(nullptr, 0, out);
    return;
  }
  if (n == 1) {
    const size_t a = s.byte_off[first], b = s.byte_off[first + 1];
    std::vector<uint8_t> in(1 + (b - a));
    in[0] = 0x00;
    if (b > a) memcpy(in.data() + 1, s.bytes + a, b - a);
    valhash_sha256(in.data(), in.size(), out);
    return;
  }
  size_t k = 1;
  while (k * 2 < n) k *= 2;             // the largest power of two below n
  uint8_t in[65];
  in[0] = 0x01;
  hdrhash_mth(s, first, k, in + 1);
  hdrhash_mth(s, first + k, n - k, in + 33);
  valhash_sha256(in, 65, out);
}

inline void hdrhash_root(const HdrSet& s, size_t h, uint8_t out[32]) {
  hdrhash_mth(s, s.leaf_off[h], s.leaf_off[h + 1] - s.leaf_off[h], out);
}

// does the rule (leaf L, position P, source src) hold for header h?
inline bool hdrhash_rule(const HdrSet& s, size_t h, uint32_t L, uint32_t P, const uint8_t src[32]) {
  const size_t n = s.leaf_off[h + 1] - s.leaf_off[h];
  if (L >= n) return false;
  const size_t j = (size_t)s.leaf_off[h] + L;
  const size_t a = s.byte_off[j], b = s.byte_off[j + 1];
  if (b - a < (size_t)P + 32) return false;
  return memcmp(s.bytes + a + P, src, 32) == 0;
}

// The rules of one call; every array is nullable and a HEADER_NONE entry skips its header.
// set_roots: the validator-set root of every history version, 32 bytes each by version (what
// valhash_root gives), read for the versions vals_ver and next_ver name.
struct HdrRules {
  const uint8_t* expect;
  const uint32_t* vals_ver;
  uint32_t vals_leaf, vals_pos;
  const uint32_t* next_ver;
  uint32_t next_leaf, next_pos;
  const uint32_t* link;
  uint32_t link_leaf, link_pos;
  const uint8_t* set_roots;
};

// roots (nh x 32) and bad (nh bytes) of the set under the rules; returns the number of non-zero bytes
inline size_t hdrhash_bind(const HdrSet& s, const HdrRules& r, uint8_t* bad, uint8_t* roots) {
  for (size_t h = 0; h < s.nh; ++h) hdrhash_root(s, h, roots + 32 * h);
  size_t n_bad = 0;
  for (size_t h = 0; h < s.nh; ++h) {
    uint8_t f = 0;
    if (r.expect && memcmp(roots + 32 * h, r.expect + 32 * h, 32)) f |= HEADER_BAD_HASH;
    if (r.vals_ver && r.vals_ver[h] != HEADER_NONE &&
        !hdrhash_rule(s, h, r.vals_leaf, r.vals_pos, r.set_roots + (size_t)32 * r.vals_ver[h]))
      f |= HEADER_BAD_VALS;
    if (r.next_ver && r.next_ver[h] != HEADER_NONE &&
        !hdrhash_rule(s, h, r.next_leaf, r.next_pos, r.set_roots + (size_t)32 * r.next_ver[h]))
      f |= HEADER_BAD_NEXT;
    if (r.link && r.link[h] != HEADER_NONE && !hdrhash_rule(s, h, r.link_leaf, r.link_pos, roots + (size_t)32 * r.link[h]))
      f |= HEADER_BAD_LINK;
    bad[h] = f;
    n_bad += f != 0;
  }
  return n_bad;
}

}  // namespace edc
