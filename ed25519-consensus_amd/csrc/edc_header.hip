// Header hashes (hdrhash.h; edc_header_hashes, edc_header_bind): the Merkle root of many block
// headers at once, each given as its ordered leaves, and the byte rules that bind a header to
// validator-set roots and to another header of the same call.
//
//   k_hd_root   one group of G lanes per header, G the next power of two at or above the launch's
//               largest leaf count (2 to 64), so a group lies inside one wave and 64 / G headers
//               share a wave. Lane j hashes leaf j of its header with sha256_leaf_stream, looping
//               over its own block count (lanes of a wave diverge there). The digests are then
//               reduced level by level: lane i takes the nodes 2 i and 2 i + 1 of the level below
//               from their lanes by cross-lane moves and hashes them with sha256_node; a lone
//               last node is promoted unhashed. The level loop runs log2 G times for every lane of
//               the wave, since a cross-lane move reads only lanes that execute it; a header whose
//               count has reached one node only hands that node on. Level-wise equals RFC 6962's
//               recursion (edc_valhash.hip states why). Lane 0 of the group writes the root; a
//               header with no leaf writes SHA-256 of the empty string.
//   k_hd_bind   one lane per header, after the roots exist: up to four 32-byte compares (the
//               expected hash against the root; three places in the header's leaves against a
//               validator-set root, another one, and the root of another header), the bad byte, and a
//               per-workgroup count of the non-zero bytes added to one counter.
//
// No LDS: a group never leaves its wave, so the reduction needs no barrier and no allocation that
// would bound the occupancy; the moves are ds_bpermute_b32, 16 per level and lane.
// The leaf bytes are read as aligned words at any byte offset (sha256.h, hd_rule); the byte array
// is a whole number of words on the device, zero behind its last byte.
#include "edc_launch.h"
#include "hdrhash.h"                    // the constants only
#include "sha256.h"

namespace edc {

namespace {

constexpr uint32_t HD_THREADS = 256;

__global__ void __launch_bounds__(HD_THREADS) k_hd_root(HeaderSrc s, uint32_t first, uint32_t count, uint32_t lg,
                                                        uint32_t* __restrict__ roots) {
  const uint32_t G = 1u << lg;
  const uint32_t gid = blockIdx.x * HD_THREADS + threadIdx.x;
  const uint32_t hl = gid >> lg, j = gid & (G - 1);
  const bool active = hl < count;
  const uint32_t h = first + (active ? hl : 0);
  const uint32_t l0 = s.leaf_off[h];
  const uint32_t n = active ? s.leaf_off[h + 1] - l0 : 0;   // <= G: the host sized G for the launch
  uint32_t x[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) x[t] = 0;
  if (j < n) sha256_leaf_stream(s.words, s.byte_off[l0 + j], s.byte_off[l0 + j + 1], x);

  const uint32_t lane = threadIdx.x & 63;
  const uint32_t base = lane & ~(G - 1);
  const uint32_t src = base + ((2 * j) & (G - 1));          // j >= G / 2 reads what it never uses
  uint32_t cnt = n;
  for (uint32_t l = 0; l < lg; ++l) {
    uint32_t a[8], b[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      a[t] = (uint32_t)__shfl((int)x[t], (int)src);
      b[t] = (uint32_t)__shfl((int)x[t], (int)(src + 1));
    }
    if (2 * j + 1 < cnt) {
      sha256_node(a, b, x);
    } else if (2 * j < cnt) {
#pragma unroll
      for (int t = 0; t < 8; ++t) x[t] = a[t];
    }
    cnt = (cnt + 1) >> 1;
  }
  if (!active || j) return;
  if (n == 0) sha256_empty(x);
  uint4* out = reinterpret_cast<uint4*>(roots + (size_t)h * 8);
  out[0] = make_uint4(sha256_bswap(x[0]), sha256_bswap(x[1]), sha256_bswap(x[2]), sha256_bswap(x[3]));
  out[1] = make_uint4(sha256_bswap(x[4]), sha256_bswap(x[5]), sha256_bswap(x[6]), sha256_bswap(x[7]));
}

// Does the rule (leaf L, position P, source src: eight words of 32 bytes) hold for header h of n
// leaves? The 32 bytes start at any byte: eight or nine aligned words are read and joined; the
// ninth only when it holds one of the bytes.
__device__ __forceinline__ bool hd_rule(const HeaderSrc& s, uint32_t l0, uint32_t n, uint32_t L, uint32_t P,
                                        const uint32_t* __restrict__ src) {
  if (L >= n) return false;
  const uint32_t a = s.byte_off[l0 + L], b = s.byte_off[l0 + L + 1];
  if ((uint64_t)P + 32 > (uint64_t)(b - a)) return false;
  const uint32_t q = a + P, i = q >> 2, sh = (q & 3) * 8;
  uint32_t cur = s.words[i], d = 0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const uint32_t nxt = (t < 7 || sh) ? s.words[i + t + 1] : 0u;
    const uint32_t v = sh ? (cur >> sh) | (nxt << (32 - sh)) : cur;
    d |= v ^ src[t];
    cur = nxt;
  }
  return d == 0;
}

__global__ void __launch_bounds__(HD_THREADS) k_hd_bind(HeaderSrc s, HeaderBind r, const uint32_t* __restrict__ roots,
                                                        uint8_t* __restrict__ bad, uint32_t* __restrict__ n_bad) {
  const uint32_t h = blockIdx.x * HD_THREADS + threadIdx.x;
  uint32_t f = 0;
  if (h < s.nh) {
    const uint32_t l0 = s.leaf_off[h], n = s.leaf_off[h + 1] - l0;
    if (r.expect) {
      uint32_t d = 0;
#pragma unroll
      for (int t = 0; t < 8; ++t) d |= roots[(size_t)h * 8 + t] ^ r.expect[(size_t)h * 8 + t];
      if (d) f |= HEADER_BAD_HASH;
    }
    if (r.vals_idx) {
      const uint32_t v = r.vals_idx[h];
      if (v != HEADER_NONE && !hd_rule(s, l0, n, r.vals_leaf, r.vals_pos, r.set_roots + (size_t)v * 8)) f |= HEADER_BAD_VALS;
    }
    if (r.next_idx) {
      const uint32_t v = r.next_idx[h];
      if (v != HEADER_NONE && !hd_rule(s, l0, n, r.next_leaf, r.next_pos, r.set_roots + (size_t)v * 8)) f |= HEADER_BAD_NEXT;
    }
    if (r.link) {
      const uint32_t v = r.link[h];
      if (v != HEADER_NONE && !hd_rule(s, l0, n, r.link_leaf, r.link_pos, roots + (size_t)v * 8)) f |= HEADER_BAD_LINK;
    }
    bad[h] = (uint8_t)f;
  }
  const int c = __syncthreads_count(f != 0);
  if (threadIdx.x == 0 && c) atomicAdd(n_bad, (uint32_t)c);
}

}  // namespace

void launch_header_roots(hipStream_t st, const HeaderSrc& src, uint32_t max_leaves, uint8_t* roots) {
  if (!src.nh) return;
  uint32_t lg = 1;
  while ((1u << lg) < max_leaves) ++lg;                     // G = 2 .. 64 for max_leaves <= HEADER_MAX_LEAVES
  const uint32_t per_block = HD_THREADS >> lg;              // headers of one workgroup
  constexpr uint32_t GRID = 1u << 22;                       // workgroups per launch: 2^30 lanes
  const uint64_t blocks = ((uint64_t)src.nh + per_block - 1) / per_block;
  for (uint64_t at = 0; at < blocks; at += GRID) {
    const uint32_t g = (uint32_t)(blocks - at < GRID ? blocks - at : GRID);
    const uint64_t first = at * per_block;
    const uint64_t count = (uint64_t)src.nh - first < (uint64_t)g * per_block ? (uint64_t)src.nh - first : (uint64_t)g * per_block;
    hipLaunchKernelGGL(k_hd_root, dim3(g), dim3(HD_THREADS), 0, st, src, (uint32_t)first, (uint32_t)count, lg,
                       reinterpret_cast<uint32_t*>(roots));
  }
}

void launch_header_bind(hipStream_t st, const HeaderSrc& src, const HeaderBind& rules, const uint8_t* roots, uint8_t* bad,
                        uint32_t* n_bad) {
  if (!src.nh) return;
  hipLaunchKernelGGL(k_hd_bind, dim3((uint32_t)(((uint64_t)src.nh + HD_THREADS - 1) / HD_THREADS)), dim3(HD_THREADS), 0, st, src,
                     rules,
                     reinterpret_cast<const uint32_t*>(roots), bad, n_bad);
}

}  // namespace edc
