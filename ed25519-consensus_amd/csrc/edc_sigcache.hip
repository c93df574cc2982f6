// Verified-signature cache kernels (sigcache.h): lookup, order-preserving compaction of the
// misses (per-workgroup ballot counts, scan, scatter + gather; for a cached verifier's queued
// range, gather into the retained arrays at an offset with the offered positions), insert, verdict
// scatter; the masked lookup of the cached quorum commit sets, which probes the checked items only.
// One lane per item; items and records move as uint4.
#include "sigcache.h"

namespace edc {

namespace {

__device__ __forceinline__ void sc_load_item(const uint8_t* __restrict__ vk, const uint8_t* __restrict__ sig,
                                             const uint32_t* __restrict__ k, size_t i, uint4 q[8]) {
  const uint4* a = reinterpret_cast<const uint4*>(vk + i * 32);
  const uint4* b = reinterpret_cast<const uint4*>(sig + i * 64);
  const uint4* c = reinterpret_cast<const uint4*>(k + i * 8);
  q[0] = a[0]; q[1] = a[1];
  q[2] = b[0]; q[3] = b[1]; q[4] = b[2]; q[5] = b[3];
  q[6] = c[0]; q[7] = c[1];
}

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

#define SC_SIPROUND            \
  do {                         \
    v0 += v1; v1 = rotl64(v1, 13); v1 ^= v0; v0 = rotl64(v0, 32); \
    v2 += v3; v3 = rotl64(v3, 16); v3 ^= v2;                      \
    v0 += v3; v3 = rotl64(v3, 21); v3 ^= v0;                      \
    v2 += v1; v1 = rotl64(v1, 17); v1 ^= v2; v2 = rotl64(v2, 32); \
  } while (0)

// SipHash-1-3 of the 128-byte item under the context's key: low bits -> home slot, high 32 ->
// fingerprint. A keyed PRF, so items chosen by the network cannot be aimed at one probe window.
__device__ __forceinline__ uint64_t sc_hash(const uint4 q[8], uint64_t k0, uint64_t k1) {
  uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull;
  uint64_t v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint64_t m0 = (uint64_t)q[j].x | ((uint64_t)q[j].y << 32);
    const uint64_t m1 = (uint64_t)q[j].z | ((uint64_t)q[j].w << 32);
    v3 ^= m0; SC_SIPROUND; v0 ^= m0;
    v3 ^= m1; SC_SIPROUND; v0 ^= m1;
  }
  const uint64_t b = 128ull << 56;
  v3 ^= b; SC_SIPROUND; v0 ^= b;
  v2 ^= 0xff;
  SC_SIPROUND; SC_SIPROUND; SC_SIPROUND;
  return v0 ^ v1 ^ v2 ^ v3;
}

__device__ __forceinline__ uint32_t sc_slot(uint32_t home, uint32_t p) {
  return (home & ~(SC_WINDOW - 1)) | ((home + p) & (SC_WINDOW - 1));
}

__device__ __forceinline__ bool sc_live(const SigCacheView& sc, unsigned long long hd) {
  return hd != 0 && sc.gen - (uint32_t)hd <= sc.keep;
}

// the full 128-byte compare behind every hit
__device__ __forceinline__ bool sc_equal(const uint4* __restrict__ r, const uint4 q[8]) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint4 o = r[j];
    eq &= o.x == q[j].x && o.y == q[j].y && o.z == q[j].z && o.w == q[j].w;
  }
  return eq;
}

// the probe behind every lookup: is the loaded item q a live record?
__device__ __forceinline__ bool sc_probe(const SigCacheView& sc, const uint4 q[8]) {
  const uint64_t h = sc_hash(q, sc.k0, sc.k1);
  const uint32_t fp = (uint32_t)(h >> 32), home = (uint32_t)h & sc.mask;
  for (uint32_t p = 0; p < SC_WINDOW; ++p) {
    const uint32_t slot = sc_slot(home, p);
    const unsigned long long hd = sc.hdr[slot];
    if (hd == 0) break;       // never used: nothing of this item's probe order lies beyond
    if ((uint32_t)(hd >> 32) == fp && sc_live(sc, hd) && sc_equal(sc.rec + (size_t)slot * 8, q)) return true;
  }
  return false;
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_lookup(SigCacheView sc, uint32_t n, const uint8_t* __restrict__ vk,
                                                        const uint8_t* __restrict__ sig,
                                                        const uint32_t* __restrict__ k, uint8_t* __restrict__ hit,
                                                        uint32_t* __restrict__ wg_miss) {
  const uint32_t i = blockIdx.x * SC_BLOCK + threadIdx.x;
  bool miss = false;
  if (i < n) {
    uint4 q[8];
    sc_load_item(vk, sig, k, i, q);
    const bool found = sc_probe(sc, q);
    hit[i] = found ? 1 : 0;
    miss = !found;
  }
  if (wg_miss) {              // uniform: every lane of the workgroup reaches the barrier
    __shared__ uint32_t wsum[SC_BLOCK / 64];
    const uint64_t b = __ballot(miss);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (uint32_t w = 0; w < SC_BLOCK / 64; ++w) s += wsum[w];
      wg_miss[blockIdx.x] = s;
    }
  }
}

// Cached quorum commit sets (edc_cached_*): the lookup of the checked items only. skip[i] != 0
// (skip null: no item is left out) marks an item the selection did not check: its lane touches
// neither the item's bytes nor the table. leave[i] = 1 for an item that is not checked or is a
// live record, else 0 (the byte k_sc_compact reads: what stays is the checked misses, in queue
// order); code[i] = 255 for an item that is not checked, else 0 (the codes of a failed union's
// misses are scattered over it, so hits end as 0); the workgroup's misses and hits among the
// checked. One LDS word per wave as in the kernels around it: both counts are at most 64 and
// share the word (misses low half, hits high half).
__global__ void __launch_bounds__(SC_BLOCK) k_sc_lookup_masked(SigCacheView sc, uint32_t n,
                                                               const uint8_t* __restrict__ skip,
                                                               const uint8_t* __restrict__ vk,
                                                               const uint8_t* __restrict__ sig,
                                                               const uint32_t* __restrict__ k,
                                                               uint8_t* __restrict__ leave, uint8_t* __restrict__ code,
                                                               uint32_t* __restrict__ wg_miss,
                                                               uint32_t* __restrict__ wg_hit) {
  __shared__ uint32_t wsum[SC_BLOCK / 64];
  const uint32_t i = blockIdx.x * SC_BLOCK + threadIdx.x;
  const bool checked = i < n && (!skip || skip[i] == 0);
  bool found = false;
  if (checked) {
    uint4 q[8];
    sc_load_item(vk, sig, k, i, q);
    found = sc_probe(sc, q);
  }
  if (i < n) {
    leave[i] = (!checked || found) ? 1 : 0;
    code[i] = checked ? 0 : 255;
  }
  const uint64_t bm = __ballot(checked && !found), bh = __ballot(checked && found);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(bm) | ((uint32_t)__popcll(bh) << 16);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < SC_BLOCK / 64; ++w) s += wsum[w];    // each half at most SC_BLOCK: no carry between them
    wg_miss[blockIdx.x] = s & 0xFFFFu;
    wg_hit[blockIdx.x] = s >> 16;
  }
}

// one workgroup: exclusive scan of the workgroup counts, SC_SCAN_TILE per pass with a carry
__global__ void __launch_bounds__(SC_SCAN_TILE) k_sc_scan(uint32_t nwg, uint32_t* __restrict__ wg,
                                                          uint32_t* __restrict__ total) {
  __shared__ uint32_t wsum[SC_SCAN_TILE / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nwg; base += SC_SCAN_TILE) {
    const uint32_t t = base + tid;
    const uint32_t v = t < nwg ? wg[t] : 0;
    uint32_t incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t wpre = 0, tile = 0;
    for (uint32_t w = 0; w < SC_SCAN_TILE / 64; ++w) {
      const uint32_t s = wsum[w];
      if (w < wave) wpre += s;
      tile += s;
    }
    if (t < nwg) wg[t] = carry + wpre + incl - v;
    carry += tile;
    __syncthreads();
  }
  if (tid == 0) total[0] = carry;
}

// Order-preserving compaction of the misses of n items, shared by the two kernels below: rank
// inside the workgroup from the waves' ballots, the workgroup's start from the scanned counts.
// Miss j gets pos[j] = base + i and its vk / sig / k in row j of the out arrays.
__device__ __forceinline__ void sc_compact_body(uint32_t n, const uint8_t* __restrict__ hit,
                                                const uint32_t* __restrict__ wg_off, const uint8_t* __restrict__ vk,
                                                const uint8_t* __restrict__ sig, const uint32_t* __restrict__ k,
                                                uint32_t base, uint32_t* __restrict__ pos, uint8_t* __restrict__ out_vk,
                                                uint8_t* __restrict__ out_sig, uint32_t* __restrict__ out_k) {
  __shared__ uint32_t wsum[SC_BLOCK / 64];
  const uint32_t i = blockIdx.x * SC_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool miss = i < n && hit[i] == 0;
  const uint64_t b = __ballot(miss);
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (!miss) return;
  uint32_t j = wg_off[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1));
  for (uint32_t w = 0; w < wave; ++w) j += wsum[w];
  pos[j] = base + i;
  uint4 q[8];
  sc_load_item(vk, sig, k, i, q);
  uint4* da = reinterpret_cast<uint4*>(out_vk + (size_t)j * 32);
  uint4* db = reinterpret_cast<uint4*>(out_sig + (size_t)j * 64);
  uint4* dc = reinterpret_cast<uint4*>(out_k + (size_t)j * 8);
  da[0] = q[0]; da[1] = q[1];
  db[0] = q[2]; db[1] = q[3]; db[2] = q[4]; db[3] = q[5];
  dc[0] = q[6]; dc[1] = q[7];
}

// one cached call: idx[j] = queue index of miss j, the misses gathered to the staging arrays
__global__ void __launch_bounds__(SC_BLOCK) k_sc_compact(uint32_t n, const uint8_t* __restrict__ hit,
                                                         const uint32_t* __restrict__ wg_off,
                                                         const uint8_t* __restrict__ vk,
                                                         const uint8_t* __restrict__ sig,
                                                         const uint32_t* __restrict__ k, uint32_t* __restrict__ idx,
                                                         uint8_t* __restrict__ out_vk, uint8_t* __restrict__ out_sig,
                                                         uint32_t* __restrict__ out_k) {
  sc_compact_body(n, hit, wg_off, vk, sig, k, 0u, idx, out_vk, out_sig, out_k);
}

// one queued range of a cached verifier: miss j of the range lands in row dst0 + j of the retained
// arrays (the caller passes them, and origin, already offset by dst0) and its offered position
// base + i in origin
__global__ void __launch_bounds__(SC_BLOCK) k_sc_gather_range(uint32_t n, const uint8_t* __restrict__ hit,
                                                              const uint32_t* __restrict__ wg_off,
                                                              const uint8_t* __restrict__ vk,
                                                              const uint8_t* __restrict__ sig,
                                                              const uint32_t* __restrict__ k, uint32_t base,
                                                              uint8_t* __restrict__ out_vk, uint8_t* __restrict__ out_sig,
                                                              uint32_t* __restrict__ out_k, uint32_t* __restrict__ origin) {
  sc_compact_body(n, hit, wg_off, vk, sig, k, base, origin, out_vk, out_sig, out_k);
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_insert(SigCacheView sc, uint32_t c, const uint32_t* __restrict__ idx,
                                                        const uint8_t* __restrict__ vk,
                                                        const uint8_t* __restrict__ sig,
                                                        const uint32_t* __restrict__ k,
                                                        const uint8_t* __restrict__ verdict,
                                                        unsigned long long* __restrict__ ctr) {
  const uint32_t j = blockIdx.x * SC_BLOCK + threadIdx.x;
  int res = 0;                // 1: record written, 2: dropped
  if (j < c && (!verdict || verdict[j] == 0)) {
    const size_t i = idx ? idx[j] : j;
    uint4 q[8];
    sc_load_item(vk, sig, k, i, q);
    const uint64_t h = sc_hash(q, sc.k0, sc.k1);
    const uint32_t fp = (uint32_t)(h >> 32), home = (uint32_t)h & sc.mask;
    const unsigned long long mine = ((unsigned long long)fp << 32) | sc.gen;
    res = 2;
    uint32_t p = 0;
    // each round either ends or finds the slot it wanted claimed by another lane of this launch
    // and looks again from there; the round count is bounded, so a lane never spins
    for (uint32_t round = 0; round < 2 * SC_WINDOW && p < SC_WINDOW; ++round) {
      uint32_t cand = SC_WINDOW;
      unsigned long long cand_hd = 0;
      bool dup = false;
      for (uint32_t t = p; t < SC_WINDOW; ++t) {
        const uint32_t slot = sc_slot(home, t);
        const unsigned long long hd = __hip_atomic_load(&sc.hdr[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!sc_live(sc, hd)) {
          if (cand == SC_WINDOW) { cand = t; cand_hd = hd; }
          if (hd == 0) break;
          continue;
        }
        if ((uint32_t)(hd >> 32) == fp && sc_equal(sc.rec + (size_t)slot * 8, q)) { dup = true; break; }
      }
      if (dup) { res = 0; break; }          // an equal live record: nothing to do
      if (cand == SC_WINDOW) break;         // no free or dead slot in the window: dropped
      const uint32_t slot = sc_slot(home, cand);
      const unsigned long long prev = atomicCAS(&sc.hdr[slot], cand_hd, mine);
      if (prev == cand_hd) {                // claimed: only this lane writes the record
        uint4* r = sc.rec + (size_t)slot * 8;
#pragma unroll
        for (int w = 0; w < 8; ++w) r[w] = q[w];
        res = 1;
        break;
      }
      p = cand;
    }
  }
  const uint64_t bi = __ballot(res == 1), bd = __ballot(res == 2);
  if ((threadIdx.x & 63) == 0) {
    if (bi) atomicAdd(&ctr[0], (unsigned long long)__popcll(bi));
    if (bd) atomicAdd(&ctr[1], (unsigned long long)__popcll(bd));
  }
}

__global__ void __launch_bounds__(SC_BLOCK) k_sc_scatter(uint32_t c, const uint32_t* __restrict__ idx,
                                                         const uint8_t* __restrict__ v, uint8_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * SC_BLOCK + threadIdx.x;
  if (j < c) out[idx[j]] = v[j];
}

inline uint32_t sc_blocks(uint32_t n) { return (n + SC_BLOCK - 1) / SC_BLOCK; }

}  // namespace

void launch_sc_lookup(hipStream_t st, const SigCacheView& sc, uint32_t n, const uint8_t* vk, const uint8_t* sig,
                      const uint32_t* k, uint8_t* hit, uint32_t* wg_miss) {
  if (n) hipLaunchKernelGGL(k_sc_lookup, dim3(sc_blocks(n)), dim3(SC_BLOCK), 0, st, sc, n, vk, sig, k, hit, wg_miss);
}

void launch_sc_lookup_masked(hipStream_t st, const SigCacheView& sc, uint32_t n, const uint8_t* skip, const uint8_t* vk,
                             const uint8_t* sig, const uint32_t* k, uint8_t* leave, uint8_t* code, uint32_t* wg_miss,
                             uint32_t* wg_hit) {
  if (n)
    hipLaunchKernelGGL(k_sc_lookup_masked, dim3(sc_blocks(n)), dim3(SC_BLOCK), 0, st, sc, n, skip, vk, sig, k, leave, code,
                       wg_miss, wg_hit);
}

void launch_sc_scan(hipStream_t st, uint32_t nwg, uint32_t* wg_miss, uint32_t* total) {
  hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(SC_SCAN_TILE), 0, st, nwg, wg_miss, total);
}

void launch_sc_compact(hipStream_t st, uint32_t n, const uint8_t* hit, const uint32_t* wg_off, const uint8_t* vk,
                       const uint8_t* sig, const uint32_t* k, uint32_t* idx, uint8_t* out_vk, uint8_t* out_sig,
                       uint32_t* out_k) {
  if (n)
    hipLaunchKernelGGL(k_sc_compact, dim3(sc_blocks(n)), dim3(SC_BLOCK), 0, st, n, hit, wg_off, vk, sig, k, idx, out_vk,
                       out_sig, out_k);
}

void launch_sc_insert(hipStream_t st, const SigCacheView& sc, uint32_t c, const uint32_t* idx, const uint8_t* vk,
                      const uint8_t* sig, const uint32_t* k, const uint8_t* verdict, unsigned long long* ctr) {
  if (c) hipLaunchKernelGGL(k_sc_insert, dim3(sc_blocks(c)), dim3(SC_BLOCK), 0, st, sc, c, idx, vk, sig, k, verdict, ctr);
}

void launch_sc_scatter(hipStream_t st, uint32_t c, const uint32_t* idx, const uint8_t* v, uint8_t* out) {
  if (c) hipLaunchKernelGGL(k_sc_scatter, dim3(sc_blocks(c)), dim3(SC_BLOCK), 0, st, c, idx, v, out);
}

void launch_sc_gather_range(hipStream_t st, uint32_t n, const uint8_t* hit, const uint32_t* wg_off, const uint8_t* vk,
                            const uint8_t* sig, const uint32_t* k, uint32_t base, size_t dst0, uint8_t* out_vk,
                            uint8_t* out_sig, uint32_t* out_k, uint32_t* origin) {
  if (n)
    hipLaunchKernelGGL(k_sc_gather_range, dim3(sc_blocks(n)), dim3(SC_BLOCK), 0, st, n, hit, wg_off, vk, sig, k, base,
                       out_vk + dst0 * 32, out_sig + dst0 * 64, out_k + dst0 * 8, origin + dst0);
}

}  // namespace edc
