// Validator-set hashes (edc_valhash_*, include/edc.h): the Merkle root of a validator set, the value a light client compares with the validators_hash of the
// header it trusts. The host reference: a small byte-wise SHA-256, the member's address, leaf and
// order, the recursive RFC 6962 root and the root of one version of a history. The device kernels
// (sha256.h, edc_valhash.hip) are written separately and are held to this file by the tests.
// Plain C++ with no HIP in it, so it can be compiled into a stand-alone host program.
//
// The function (agreement with CometBFT's ValidatorSet.Hash() is the intent, stated from memory):
//   addr_p  the first 20 bytes of SHA-256(key_p)
//   order   power descending, then addr ascending as byte strings, then position ascending
//   leaf_p  0A 22 0A 20 | key_p | (10 | uvarint(w_p) if w_p > 0), 36 to 46 bytes
//   root    RFC 6962's MTH over the ordered leaves with SHA-256: the empty set -> SHA-256(""), one
//           leaf -> SHA-256(00 | leaf), n > 1 -> SHA-256(01 | MTH(first k) | MTH(rest)), k the
//           largest power of two below n
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "vhist.h"

namespace edc {

constexpr uint32_t VALHASH_MAX_MEMBERS = 4096;       // EDC_VALHASH_MAX_MEMBERS
constexpr size_t VALHASH_ADDR_BYTES = 20;
constexpr size_t VALHASH_LEAF_MAX = 46;

// SHA-256 (FIPS 180-4) of one message held in memory
inline void valhash_sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  static const uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  // the padded length: the message, 0x80, zeros, the 64-bit bit length, a multiple of 64
  const size_t total = (len + 9 + 63) / 64 * 64;
  for (size_t base = 0; base < total; base += 64) {
    uint8_t blk[64];
    for (size_t j = 0; j < 64; ++j) {
      const size_t i = base + j;
      blk[j] = i < len ? msg[i] : i == len ? 0x80 : i >= total - 8 ? (uint8_t)(((uint64_t)len * 8) >> (8 * (total - 1 - i))) : 0;
    }
    uint32_t w[64];
    for (int t = 0; t < 16; ++t)
      w[t] = (uint32_t)blk[4 * t] << 24 | (uint32_t)blk[4 * t + 1] << 16 | (uint32_t)blk[4 * t + 2] << 8 | blk[4 * t + 3];
    for (int t = 16; t < 64; ++t) {
      const uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
      const uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
      w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int t = 0; t < 64; ++t) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  for (int j = 0; j < 8; ++j) {
    out[4 * j] = (uint8_t)(h[j] >> 24);
    out[4 * j + 1] = (uint8_t)(h[j] >> 16);
    out[4 * j + 2] = (uint8_t)(h[j] >> 8);
    out[4 * j + 3] = (uint8_t)h[j];
  }
}

// base-128 little-endian: 1 to 9 bytes for x <= 2^63 - 1 (10 for a larger x). Returns the length.
inline size_t valhash_uvarint(uint64_t x, uint8_t out[10]) {
  size_t n = 0;
  while (x >= 0x80) {
    out[n++] = (uint8_t)(x | 0x80);
    x >>= 7;
  }
  out[n++] = (uint8_t)x;
  return n;
}

inline void valhash_addr(const uint8_t key[32], uint8_t addr[VALHASH_ADDR_BYTES]) {
  uint8_t d[32];
  valhash_sha256(key, 32, d);
  memcpy(addr, d, VALHASH_ADDR_BYTES);
}

// the member's leaf; a power of 0 omits its field, as proto3 does. Returns the length (36 to 46).
inline size_t valhash_leaf(const uint8_t key[32], uint64_t power, uint8_t out[VALHASH_LEAF_MAX]) {
  static const uint8_t head[4] = {0x0A, 0x22, 0x0A, 0x20};
  memcpy(out, head, 4);
  memcpy(out + 4, key, 32);
  size_t n = 36;
  if (power) {
    out[n++] = 0x10;
    n += valhash_uvarint(power, out + n);
  }
  return n;
}

// One member of a set. The order of the leaves: power descending, addr ascending, position ascending.
struct ValhashMember {
  uint32_t pos;
  uint64_t power;
  uint8_t addr[VALHASH_ADDR_BYTES];
};
inline bool valhash_before(const ValhashMember& a, const ValhashMember& b) {
  if (a.power != b.power) return a.power > b.power;
  const int c = memcmp(a.addr, b.addr, VALHASH_ADDR_BYTES);
  return c ? c < 0 : a.pos < b.pos;
}

// The address order of a list of m positions, which no version changes: rank[p] = the place of
// position p by (addr ascending, position ascending); addrs = m x 20 bytes by position. Inside a
// set, power descending then rank ascending is the order of the leaves.
inline void valhash_rank(size_t m, const uint8_t* addrs, uint32_t* rank) {
  std::vector<uint32_t> order(m);
  for (size_t p = 0; p < m; ++p) order[p] = (uint32_t)p;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const int c = memcmp(addrs + (size_t)a * VALHASH_ADDR_BYTES, addrs + (size_t)b * VALHASH_ADDR_BYTES, VALHASH_ADDR_BYTES);
    return c ? c < 0 : a < b;
  });
  for (size_t r = 0; r < m; ++r) rank[order[r]] = (uint32_t)r;
}

// RFC 6962's MTH over the n leaf hashes SHA-256(00 | leaf) in lh (n x 32 bytes), n >= 1, by the
// recursive definition
inline void valhash_mth(const uint8_t* lh, size_t n, uint8_t out[32]) {
  if (n == 1) {
    memcpy(out, lh, 32);
    return;
  }
  size_t k = 1;
  while (k * 2 < n) k *= 2;             // the largest power of two below n
  uint8_t in[65];
  in[0] = 0x01;
  valhash_mth(lh, k, in + 1);
  valhash_mth(lh + 32 * k, n - k, in + 33);
  valhash_sha256(in, 65, out);
}

// The root of the set of n members: position pos[i] of a list whose keys are keys (32 bytes each, by
// position), with power[i]. Any order of the members gives the same root. addrs (nullable): the
// list's addresses by position, 20 bytes each, for a caller that hashes many sets of one list.
inline void valhash_root_of(size_t n, const uint32_t* pos, const uint64_t* power, const uint8_t* keys, uint8_t out[32],
                            const uint8_t* addrs = nullptr) {
  if (!n) {
    valhash_sha256(nullptr, 0, out);
    return;
  }
  std::vector<ValhashMember> mem(n);
  for (size_t i = 0; i < n; ++i) {
    mem[i].pos = pos[i];
    mem[i].power = power[i];
    if (addrs) memcpy(mem[i].addr, addrs + (size_t)pos[i] * VALHASH_ADDR_BYTES, VALHASH_ADDR_BYTES);
    else valhash_addr(keys + (size_t)pos[i] * 32, mem[i].addr);
  }
  std::sort(mem.begin(), mem.end(), valhash_before);
  std::vector<uint8_t> lh(n * 32);
  for (size_t i = 0; i < n; ++i) {
    uint8_t in[1 + VALHASH_LEAF_MAX];
    in[0] = 0x00;
    const size_t len = valhash_leaf(keys + (size_t)mem[i].pos * 32, mem[i].power, in + 1);
    valhash_sha256(in, 1 + len, lh.data() + 32 * i);
  }
  valhash_mth(lh.data(), n, out);
}

// The root of version v (<= h.nv) of the history h over the list whose keys are keys (h.m x 32
// bytes, by position): the members are the positions whose power at v is not VHIST_NOT_MEMBER.
// addrs as valhash_root_of.
inline void valhash_root(const VHist& h, const uint8_t* keys, uint32_t v, uint8_t out[32], const uint8_t* addrs = nullptr) {
  std::vector<uint32_t> pos;
  std::vector<uint64_t> pw;
  for (uint32_t p = 0; p < h.m; ++p) {
    const uint64_t w = vhist_power_at(h, p, v);
    if (w == VHIST_NOT_MEMBER) continue;
    pos.push_back(p);
    pw.push_back(w);
  }
  valhash_root_of(pos.size(), pos.data(), pw.data(), keys, out, addrs);
}

}  // namespace edc
