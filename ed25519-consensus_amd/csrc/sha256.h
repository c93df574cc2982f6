// SHA-256 (FIPS 180-4) for the validator-set hashes (edc_valhash.hip), one message per lane and
// every message built in registers: a 32-byte key (the member's address), a member's leaf and an
// inner node of the Merkle tree. A digest is held as its eight state words, whose big-endian bytes
// are the digest's bytes; memory holds raw bytes as little-endian words, so the key words are
// byte-swapped on the way in and a digest on the way out (sha256_bswap).
// The 16-word message schedule rolls in place; with the 64 rounds unrolled every index is a
// constant and the block stays in registers.
#pragma once
#include <stdint.h>
#include "fe25519.h"  // EDC_HD

namespace edc {

#if defined(__HIP_DEVICE_COMPILE__)
__constant__ uint32_t SHA256_K[64] = {
#else
static const uint32_t SHA256_K[64] = {
#endif
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

EDC_HD uint32_t sha256_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
EDC_HD uint32_t sha256_bswap(uint32_t x) { return __builtin_bswap32(x); }

EDC_HD void sha256_init(uint32_t h[8]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

// one block: w holds its sixteen big-endian words and is used up
EDC_HD void sha256_compress(uint32_t h[8], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) {
      const uint32_t x = w[(t + 1) & 15], y = w[(t + 14) & 15];
      w[t & 15] += (sha256_rotr(x, 7) ^ sha256_rotr(x, 18) ^ (x >> 3)) + w[(t + 9) & 15] +
                   (sha256_rotr(y, 17) ^ sha256_rotr(y, 19) ^ (y >> 10));
    }
    const uint32_t t1 = hh + (sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                        SHA256_K[t] + w[t & 15];
    const uint32_t t2 = (sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// SHA-256 of the empty string
EDC_HD void sha256_empty(uint32_t out[8]) {
  out[0] = 0xe3b0c442u; out[1] = 0x98fc1c14u; out[2] = 0x9afbf4c8u; out[3] = 0x996fb924u;
  out[4] = 0x27ae41e4u; out[5] = 0x649b934cu; out[6] = 0xa495991bu; out[7] = 0x7852b855u;
}

// SHA-256 of a 32-byte key, kw its bytes as eight little-endian words: one block
EDC_HD void sha256_key32(const uint32_t kw[8], uint32_t out[8]) {
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = sha256_bswap(kw[j]);
  w[8] = 0x80000000u;
#pragma unroll
  for (int j = 9; j < 15; ++j) w[j] = 0;
  w[15] = 256;
  sha256_init(out);
  sha256_compress(out, w);
}

// The leaf hash of a member: SHA-256(00 | 0A 22 0A 20 | key | (10 | uvarint(power) if power > 0)),
// 37 to 47 bytes and so one block. kw as above; power <= 2^63 - 1 (a uvarint of at most 9 bytes).
// The bytes behind the key (the field, then the padding's 80: at most 11) are gathered big-endian
// into a 128-bit pair and cut into the words 9 to 11.
EDC_HD void sha256_leaf(const uint32_t kw[8], uint64_t power, uint32_t out[8]) {
  uint64_t thi = 0, tlo = 0;
  uint32_t k = 0;
  auto put = [&](uint32_t b) {
    if (k < 8) thi |= (uint64_t)b << (56 - 8 * k);
    else tlo |= (uint64_t)b << (56 - 8 * (k - 8));
    ++k;
  };
  if (power) {
    put(0x10);
    uint64_t x = power;
    while (x >= 0x80) {
      put(((uint32_t)x & 0x7f) | 0x80);
      x >>= 7;
    }
    put((uint32_t)x);
  }
  put(0x80);
  uint32_t b[8], w[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = sha256_bswap(kw[j]);
  w[0] = 0x000A220Au;
  w[1] = 0x20000000u | (b[0] >> 8);
#pragma unroll
  for (int j = 1; j < 8; ++j) w[1 + j] = (b[j - 1] << 24) | (b[j] >> 8);
  w[9] = (b[7] << 24) | (uint32_t)(thi >> 40);
  w[10] = (uint32_t)(thi >> 8);
  w[11] = ((uint32_t)thi << 24) | (uint32_t)(tlo >> 40);
  w[12] = w[13] = w[14] = 0;
  w[15] = 8 * (36 + k);                 // 00, the 36 bytes up to the key's end, the field: k - 1 bytes
  sha256_init(out);
  sha256_compress(out, w);
}

// An inner node: SHA-256(01 | l | r) over two digests, 65 bytes and so two blocks. out may be l or r.
EDC_HD void sha256_node(const uint32_t l[8], const uint32_t r[8], uint32_t out[8]) {
  uint32_t w[16], h[8];
  w[0] = 0x01000000u | (l[0] >> 8);
#pragma unroll
  for (int j = 1; j < 8; ++j) w[j] = (l[j - 1] << 24) | (l[j] >> 8);
  w[8] = (l[7] << 24) | (r[0] >> 8);
#pragma unroll
  for (int j = 1; j < 8; ++j) w[8 + j] = (r[j - 1] << 24) | (r[j] >> 8);
  const uint32_t last = r[7] << 24;
  sha256_init(h);
  sha256_compress(h, w);
  w[0] = last | 0x00800000u;
#pragma unroll
  for (int j = 1; j < 15; ++j) w[j] = 0;
  w[15] = 65 * 8;
  sha256_compress(h, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = h[j];
}

// The four message bytes be (big-endian, the first byte on top) that start rel bytes into a message
// whose data ends after len bytes: whole inside it as they are, past its end cut, the padding's 80
// behind the last byte, nothing after that. rel and len are small enough for rel + 4 not to wrap.
EDC_HD uint32_t sha256_tail(uint32_t be, uint32_t rel, uint32_t len) {
  if (rel + 4 <= len) return be;
  if (rel > len) return 0;
  const uint32_t nb = len - rel;        // 0..3 bytes of data in this word
  return (be & ~(0xFFFFFFFFu >> (8 * nb))) | (0x80000000u >> (8 * nb));
}

// The leaf hash of a Merkle tree over arbitrary byte strings (edc_header.hip):
// SHA-256(00 | bytes[a .. b)) for any length, 0 included, one block or many. words is the byte
// array as aligned little-endian words (the array starts on a word boundary and its allocation is
// a whole number of words: the word that holds byte b - 1 is read whole). The leaf may start at
// any byte. With the 00 in front, message word W >= 1 is the four bytes from a + 4 W - 1, so every
// word of the message has the same shift against the aligned words: each aligned word is read once,
// joined with the one before it, and byte-swapped. A word without a byte of the leaf is not read,
// and what lies behind the leaf's end in a word that is read is masked away (sha256_tail). The
// padding is the 80 behind the last byte, zeros, and the 64-bit bit length 8 (1 + b - a) in the last
// two words of the last block; 1 + b - a + 9 bytes rounded up to 64 give the block count.
// b < 2^32 - 1024 (the caller checks it), so no sum here wraps.
EDC_HD void sha256_leaf_stream(const uint32_t* words, uint32_t a, uint32_t b, uint32_t out[8]) {
  const uint32_t len = b - a;
  const uint32_t nblk = (len >> 6) + (((len & 63) + 73) >> 6);
  const uint32_t lim = (b + 3) >> 2;    // words with a byte below b
  auto ld = [&](uint32_t j) -> uint32_t { return j < lim ? words[j] : 0u; };
  // the word of a + 4 W - 1 and the shift, for W >= 1: W = 1 is a + 3
  const uint32_t j1 = (a + 3) >> 2, sh = ((a + 3) & 3) * 8;
  uint32_t cur = ld(j1), j = j1;        // cur = words[j], the low part of the next message word
  uint32_t h[8];
  sha256_init(h);
  for (uint32_t k = 0; k < nblk; ++k) {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      if (k == 0 && t == 0) {
        // 00, then the first three bytes: the four bytes from a, one to the right
        const uint32_t i0 = a >> 2, s0 = (a & 3) * 8;
        const uint32_t lo = ld(i0), hi = ld(i0 + 1);
        const uint32_t v = s0 ? (lo >> s0) | (hi << (32 - s0)) : lo;
        w[0] = sha256_tail(sha256_bswap(v), 0, len) >> 8;
      } else {
        const uint32_t nxt = ld(j + 1);
        const uint32_t v = sh ? (cur >> sh) | (nxt << (32 - sh)) : cur;
        w[t] = sha256_tail(sha256_bswap(v), 64 * k + 4 * t - 1, len);
        cur = nxt;
        ++j;
      }
    }
    if (k + 1 == nblk) {
      w[14] |= (len + 1) >> 29;
      w[15] |= (len + 1) << 3;
    }
    sha256_compress(h, w);
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) out[t] = h[t];
}

}  // namespace edc
