// Validator-set hashes (valhash.h; edc_valhash_valset, edc_valhash_vhist, edc_valhash_vhist_match): the
// Merkle root of a validator set, of every requested version of the history at once.
//
//   k_vx_addr   one lane per registered position: SHA-256 of its key, the first 20 bytes out. The
//               address order does not depend on the version; the host ranks the addresses once
//               per key list (at most 65,536 of them) and uploads rank[p] and its inverse.
//   k_vx_root   one workgroup per root. (1) Every position's power at the version, by the search
//               the history's join makes (vh_power_at). (2) The members are compacted into LDS as
//               keys (~power, rank): ascending in that key is power descending, then address
//               ascending, and since ranks are distinct no two keys are equal, so the order the
//               compaction's atomic counter hands out does not reach the result. (3) A bitonic sort
//               of the next power of two of slots; the padding key (~0, ~0) is above every member's.
//               (4) Lane j hashes the leaves 2j and 2j + 1 and their node, so the tree's widest
//               level never exists in LDS. (5) Level by level, between two LDS buffers, a lone last
//               node promoted unhashed. (6) Eight lanes write the root.
//   k_vx_match  one lane per commit: its expected 32 bytes against the root of its version.
//
// Level-wise equals RFC 6962's recursion: MTH splits n leaves at k, the largest power of two below
// n, so its left subtree is a complete tree over a k-aligned run of leaves, which pairing adjacent
// nodes level by level builds as well; the right subtree holds the n - k < k leaves behind a
// boundary every level's pairing respects (k / 2^l is even until the left part is one node), so it
// is built as MTH(n - k) by induction, promoted unhashed while it is alone at its level's odd end,
// and joined to the left root exactly when both are single nodes.
//
// LDS per workgroup, N = the padded slot count: 8 N (~power) + 4 N (rank) + 16 N (N / 2 nodes of
// 32 bytes) = 28 N bytes; the second node buffer (N / 4 nodes) lies over the ~power words, which
// are dead once the leaves are hashed. N = 4096 takes 112 KB of the CU's 160 KB and 8192 does not
// fit: VALHASH_MAX_MEMBERS. A node's eight words lie a buffer's width apart, so the lanes of a
// wave read consecutive words.
#include "edc_launch.h"
#include "sha256.h"
#include "valhash.h"

namespace edc {

namespace {

constexpr uint32_t VX_THREADS = 256;

__global__ void __launch_bounds__(VX_THREADS) k_vx_addr(uint32_t m, const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ reg, uint32_t* __restrict__ addr) {
  const uint32_t p = blockIdx.x * VX_THREADS + threadIdx.x;
  if (p >= m) return;
  const uint4* q = reinterpret_cast<const uint4*>(keys + (size_t)reg[p] * 8);
  const uint4 a = q[0], b = q[1];
  const uint32_t kw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t h[8];
  sha256_key32(kw, h);
#pragma unroll
  for (int j = 0; j < 5; ++j) addr[(size_t)p * 5 + j] = sha256_bswap(h[j]);
}

// the leaf hash of sorted slot i
__device__ __forceinline__ void vx_leaf(const ValhashSrc& src, const uint64_t* s_pw, const uint32_t* s_rk, uint32_t i,
                                        uint32_t out[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(src.keys + (size_t)src.by_rank[s_rk[i]] * 8);
  const uint4 a = q[0], b = q[1];
  const uint32_t kw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  sha256_leaf(kw, ~s_pw[i], out);
}

__global__ void __launch_bounds__(VX_THREADS) k_vx_root(ValhashSrc src, const uint32_t* __restrict__ vers, uint32_t v0,
                                                        uint32_t N, uint32_t* __restrict__ roots) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  __shared__ uint32_t s_n;
  uint64_t* s_pw = reinterpret_cast<uint64_t*>(s_dyn);                   // N keys, high part: ~power
  uint32_t* s_rk = reinterpret_cast<uint32_t*>(s_dyn + (size_t)8 * N);   // N keys, low part: rank
  uint32_t* s_a = reinterpret_cast<uint32_t*>(s_dyn + (size_t)12 * N);   // N / 2 nodes, word t of node j at t sa + j
  uint32_t* s_b = reinterpret_cast<uint32_t*>(s_dyn);                    // N / 4 nodes over s_pw
  const uint32_t sa = N >> 1, sb = N >= 4 ? N >> 2 : 1;
  const uint32_t tid = threadIdx.x;
  const uint32_t v = vers ? vers[blockIdx.x] : v0 + blockIdx.x;

  if (tid == 0) s_n = 0;
  for (uint32_t i = tid; i < N; i += VX_THREADS) {
    s_pw[i] = ~0ull;
    s_rk[i] = ~0u;
  }
  __syncthreads();
  for (uint32_t p = tid; p < src.m; p += VX_THREADS) {
    const uint32_t c = src.reg[p];
    uint64_t w = VHIST_NOT_MEMBER;
    if (src.hist) {
      if (c < src.vh.count) w = vh_power_at(src.vh, src.vh.off[c], src.vh.off[c + 1], v);
    } else if (c < src.vs.count && src.vs.member[c]) {
      w = src.vs.power[c];
    }
    if (w != VHIST_NOT_MEMBER) {
      const uint32_t slot = atomicAdd(&s_n, 1u);
      if (slot < N) {                   // the host checked every version's member count against N
        s_pw[slot] = ~w;
        s_rk[slot] = src.rank[p];
      }
    }
  }
  __syncthreads();
  const uint32_t n = s_n < N ? s_n : N;
  if (n == 0) {
    uint32_t h[8];
    sha256_empty(h);
    if (tid < 8) roots[(size_t)blockIdx.x * 8 + tid] = sha256_bswap(h[tid]);
    return;
  }

  uint32_t np = 2;
  while (np < n) np <<= 1;              // <= N
  for (uint32_t k = 2; k <= np; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < np; i += VX_THREADS) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint64_t pi = s_pw[i], pl = s_pw[l];
          const uint32_t ri = s_rk[i], rl = s_rk[l];
          const bool above = pi > pl || (pi == pl && ri > rl);
          if (above == ((i & k) == 0)) {
            s_pw[i] = pl; s_pw[l] = pi;
            s_rk[i] = rl; s_rk[l] = ri;
          }
        }
      }
      __syncthreads();
    }
  }

  // leaves -> level 1
  uint32_t cnt = n;
  for (uint32_t j = tid; j < (cnt + 1) >> 1; j += VX_THREADS) {
    uint32_t x[8];
    vx_leaf(src, s_pw, s_rk, 2 * j, x);
    if (2 * j + 1 < cnt) {
      uint32_t y[8];
      vx_leaf(src, s_pw, s_rk, 2 * j + 1, y);
      sha256_node(x, y, x);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) s_a[t * sa + j] = x[t];
  }
  __syncthreads();                      // also: s_pw is dead from here on, s_b may be written
  cnt = (cnt + 1) >> 1;
  uint32_t* from = s_a;
  uint32_t* to = s_b;
  uint32_t sf = sa, st = sb;
  while (cnt > 1) {
    for (uint32_t j = tid; j < (cnt + 1) >> 1; j += VX_THREADS) {
      uint32_t x[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) x[t] = from[t * sf + 2 * j];
      if (2 * j + 1 < cnt) {
        uint32_t y[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) y[t] = from[t * sf + 2 * j + 1];
        sha256_node(x, y, x);
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) to[t * st + j] = x[t];
    }
    __syncthreads();
    cnt = (cnt + 1) >> 1;
    uint32_t* const sp = from; from = to; to = sp;
    const uint32_t ss = sf; sf = st; st = ss;
  }
  if (tid < 8) roots[(size_t)blockIdx.x * 8 + tid] = sha256_bswap(from[tid * sf]);
}

__global__ void __launch_bounds__(VX_THREADS) k_vx_match(uint32_t nc, const uint32_t* __restrict__ roots,
                                                         const uint32_t* __restrict__ idx,
                                                         const uint32_t* __restrict__ expect, uint8_t* __restrict__ ok) {
  const uint32_t c = blockIdx.x * VX_THREADS + threadIdx.x;
  if (c >= nc) return;
  const uint4* r = reinterpret_cast<const uint4*>(roots + (size_t)idx[c] * 8);
  const uint4* e = reinterpret_cast<const uint4*>(expect + (size_t)c * 8);
  const uint4 r0 = r[0], r1 = r[1], e0 = e[0], e1 = e[1];
  const uint32_t d = (r0.x ^ e0.x) | (r0.y ^ e0.y) | (r0.z ^ e0.z) | (r0.w ^ e0.w) | (r1.x ^ e1.x) | (r1.y ^ e1.y) |
                     (r1.z ^ e1.z) | (r1.w ^ e1.w);
  ok[c] = d == 0;
}

}  // namespace

void launch_valhash_addr(hipStream_t st, uint32_t m, const uint32_t* keys, const uint32_t* reg, uint8_t* addr) {
  if (!m) return;
  hipLaunchKernelGGL(k_vx_addr, dim3((m + VX_THREADS - 1) / VX_THREADS), dim3(VX_THREADS), 0, st, m, keys, reg,
                     reinterpret_cast<uint32_t*>(addr));
}

hipError_t valhash_init_device() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_vx_root), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(28 * VALHASH_MAX_MEMBERS));
}

hipError_t launch_valhash_roots(hipStream_t st, const ValhashSrc& src, uint32_t nroots, const uint32_t* vers, uint32_t v0,
                                uint32_t max_members, uint8_t* roots) {
  if (!nroots) return hipSuccess;
  if (max_members > VALHASH_MAX_MEMBERS) return hipErrorInvalidValue;
  uint32_t N = 2;
  while (N < max_members) N <<= 1;
  const size_t lds = (size_t)28 * N;    // above 64 KB: valhash_init_device has raised the limit
  constexpr size_t GRID = (size_t)1 << 24;      // roots per launch
  for (size_t at = 0; at < nroots; at += GRID)
    hipLaunchKernelGGL(k_vx_root, dim3((uint32_t)(nroots - at < GRID ? nroots - at : GRID)), dim3(VX_THREADS), lds, st, src,
                       vers ? vers + at : nullptr, v0 + (uint32_t)at, N, reinterpret_cast<uint32_t*>(roots + 32 * at));
  return hipSuccess;
}

void launch_valhash_match(hipStream_t st, uint32_t nc, const uint8_t* roots, const uint32_t* idx, const uint8_t* expect,
                          uint8_t* ok) {
  if (!nc) return;
  hipLaunchKernelGGL(k_vx_match, dim3((nc + VX_THREADS - 1) / VX_THREADS), dim3(VX_THREADS), 0, st, nc,
                     reinterpret_cast<const uint32_t*>(roots), idx, reinterpret_cast<const uint32_t*>(expect), ok);
}

}  // namespace edc
