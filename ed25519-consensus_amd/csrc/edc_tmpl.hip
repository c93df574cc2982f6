// Templated messages (edc_tmpl_*, include/edc.h; Item::from, reference src/batch.rs:82-94, sees
// message i = head[tpl[i]] || var[var_off[i] .. var_off[i+1]) || tail[tpl[i]]): the message arena
// and its 64-bit offsets are built on the device, and k_challenge runs on them unchanged.
//
//   k_tmpl_len      len_i with validation (flag on a bad index / offset), one sum per workgroup
//   k_tmpl_scan     exclusive scan of the workgroup sums (one workgroup)
//   k_tmpl_expand   msg_off[i] and the bytes: a workgroup's 256 items are one contiguous span of
//                   the arena, written in whole aligned 16-byte stores (byte stores only in the
//                   span's two partial end chunks, which the neighbouring workgroups share)
//   k_tmpl_commit_map  commit sets with one template per commit: the per-item tpl array from the
//                   commit offsets, in front of the three kernels above
//   k_tmpl_commit_map_alt  the same with a variant byte per item: tpl[i] = commit_tpl[c] + item_alt[i];
//                   raises the flag on a byte outside the commit's window
//
// The flag: k_tmpl_len raises it when tpl[i] >= count or var_off[i] <= var_off[i+1] <= var_bytes
// does not hold. The other two kernels read it first and then produce n empty messages, so
// nothing outside the declared arrays is read and nothing outside the workspace written.
#include "edc_common.h"
#include "edc_launch.h"

namespace edc {

constexpr int TMPL_BLOCK = 256;          // items per workgroup
constexpr int TMPL_SCAN_THREADS = 1024;
constexpr uint32_t TMPL_LDS_MAX = 16384; // a set up to this many bytes (offsets + blobs) is staged in LDS

__global__ void __launch_bounds__(TMPL_BLOCK) k_tmpl_len(uint32_t n, TmplView ts, const uint16_t* __restrict__ tpl,
                                                        const uint32_t* __restrict__ var_off, uint64_t var_bytes,
                                                        int* __restrict__ flag, uint64_t* __restrict__ bsum) {
  __shared__ uint64_t s_sum[TMPL_BLOCK];
  const uint32_t tid = threadIdx.x, i = blockIdx.x * TMPL_BLOCK + tid;
  uint64_t len = 0;
  if (i < n) {
    const uint32_t t = tpl[i], a = var_off[i], b = var_off[i + 1];
    if (t >= ts.count || a > b || (uint64_t)b > var_bytes) atomicOr(flag, 1);
    else len = (uint64_t)(ts.head_off[t + 1] - ts.head_off[t]) + (b - a) + (ts.tail_off[t + 1] - ts.tail_off[t]);
  }
  s_sum[tid] = len;
  __syncthreads();
#pragma unroll
  for (int d = TMPL_BLOCK / 2; d >= 1; d >>= 1) {
    if (tid < (uint32_t)d) s_sum[tid] += s_sum[tid + d];
    __syncthreads();
  }
  if (tid == 0) bsum[blockIdx.x] = s_sum[0];
}

// bsum[0, nb) -> its exclusive prefix sums, in place; all zero when the flag is up
__global__ void __launch_bounds__(TMPL_SCAN_THREADS) k_tmpl_scan(uint32_t nb, const int* __restrict__ flag,
                                                                 uint64_t* __restrict__ bsum) {
  __shared__ uint64_t s_part[TMPL_SCAN_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (nb + TMPL_SCAN_THREADS - 1) / TMPL_SCAN_THREADS;
  const uint32_t j0 = tid * per < nb ? tid * per : nb, j1 = j0 + per < nb ? j0 + per : nb;
  const bool bad = *flag != 0;
  uint64_t sum = 0;
  if (!bad)
    for (uint32_t j = j0; j < j1; ++j) sum += bsum[j];
  s_part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < TMPL_SCAN_THREADS; d <<= 1) {
    const uint64_t add = tid >= (uint32_t)d ? s_part[tid - d] : 0;
    __syncthreads();
    s_part[tid] += add;
    __syncthreads();
  }
  uint64_t run = s_part[tid] - sum;
  for (uint32_t j = j0; j < j1; ++j) {
    const uint64_t v = bad ? 0 : bsum[j];
    bsum[j] = run;
    run += v;
  }
}

template <bool LDS>
__global__ void __launch_bounds__(TMPL_BLOCK) k_tmpl_expand(uint32_t n, TmplView ts, const uint16_t* __restrict__ tpl,
                                                           const uint8_t* __restrict__ var,
                                                           const uint32_t* __restrict__ var_off,
                                                           const int* __restrict__ flag,
                                                           const uint64_t* __restrict__ bsum, uint8_t* __restrict__ out,
                                                           uint64_t* __restrict__ msg_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  // all LDS in the dynamic region: the staged set first (16-byte multiple), then the item tables
  const uint32_t set_room = LDS ? (ts.set_bytes + 15u) & ~15u : 0u;
  uint64_t* s_off = reinterpret_cast<uint64_t*>(s_dyn + set_room);                  // 257 span offsets
  uint32_t* s_vo = reinterpret_cast<uint32_t*>(s_off + TMPL_BLOCK + 2);             // 257 hole offsets
  uint16_t* s_t = reinterpret_cast<uint16_t*>(s_vo + TMPL_BLOCK + 4);               // 256 template indices
  const uint32_t tid = threadIdx.x, i0 = blockIdx.x * TMPL_BLOCK;
  const uint32_t cnt = n - i0 < (uint32_t)TMPL_BLOCK ? n - i0 : (uint32_t)TMPL_BLOCK;
  const bool last = i0 + cnt == n;
  if (*flag != 0) {                      // malformed input: n empty messages, nothing else touched
    if (tid < cnt) msg_off[i0 + tid] = 0;
    if (last && tid == 0) msg_off[n] = 0;
    return;
  }
  const uint32_t* HO = ts.head_off;
  const uint32_t* TO = ts.tail_off;
  const uint8_t* H = ts.head;
  const uint8_t* T = ts.tail;
  if (LDS) {
    // the device copy of the set is one piece: head_off | tail_off | head | tail (padded to 16)
    const uint32_t* src = ts.head_off;
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_dyn);
    for (uint32_t w = tid; w < set_room / 4; w += TMPL_BLOCK) dst[w] = src[w];
    HO = dst;
    TO = dst + ts.count + 1;
    H = s_dyn + 8u * (ts.count + 1);
    T = H + ts.head_bytes;
  }
  uint64_t len = 0;
  if (tid < cnt) {
    const uint32_t t = tpl[i0 + tid], a = var_off[i0 + tid], b = var_off[i0 + tid + 1];
    len = (uint64_t)(ts.head_off[t + 1] - ts.head_off[t]) + (b - a) + (ts.tail_off[t + 1] - ts.tail_off[t]);
    s_t[tid] = (uint16_t)t;
    s_vo[tid] = a;
    if (tid == cnt - 1) s_vo[cnt] = b;
  }
  // inclusive scan of the lengths into s_off[1..]
  s_off[tid + 1] = len;
  if (tid == 0) s_off[0] = 0;
  __syncthreads();
  for (int d = 1; d < TMPL_BLOCK; d <<= 1) {
    const uint64_t add = tid >= (uint32_t)d ? s_off[tid + 1 - d] : 0;
    __syncthreads();
    s_off[tid + 1] += add;
    __syncthreads();
  }
  const uint64_t base = bsum[blockIdx.x];
  const uint64_t incl = s_off[tid + 1];
  __syncthreads();
  s_off[tid + 1] = base + incl;
  if (tid == 0) s_off[0] = base;
  if (tid < cnt) msg_off[i0 + tid] = base + incl - len;
  if (last && tid == cnt - 1) msg_off[n] = base + incl;
  __syncthreads();

  const uint64_t B = base, E = s_off[cnt];
  for (uint64_t c = (B >> 4) + tid; c < ((E + 15) >> 4); c += TMPL_BLOCK) {
    const uint64_t p0 = (c << 4) > B ? (c << 4) : B, p1 = (c << 4) + 16 < E ? (c << 4) + 16 : E;
    // the item holding byte p0: the first j with s_off[j + 1] > p0 (p0 < E, so there is one)
    uint32_t lo = 0, hi = cnt - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_off[mid + 1] > p0) hi = mid;
      else lo = mid + 1;
    }
    uint32_t j = lo;
    uint64_t start, end;
    uint32_t ho, hl, vo, vl, to;
    auto item = [&]() {
      const uint32_t t = s_t[j];
      start = s_off[j];
      end = s_off[j + 1];
      ho = HO[t];
      hl = HO[t + 1] - ho;
      vo = s_vo[j];
      vl = s_vo[j + 1] - vo;
      to = TO[t];
    };
    item();
    auto byte_at = [&](uint64_t p) -> uint32_t {
      while (p >= end) {                 // empty items in between are skipped
        ++j;
        item();
      }
      const uint64_t r = p - start;
      if (r < hl) return H[ho + (uint32_t)r];
      if (r < (uint64_t)hl + vl) return var[(size_t)vo + (size_t)(r - hl)];
      return T[to + (uint32_t)(r - hl - vl)];
    };
    if (p1 - p0 == 16) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k >> 2] |= byte_at(p0 + k) << (8 * (k & 3));
      *reinterpret_cast<uint4*>(out + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (uint64_t p = p0; p < p1; ++p) out[p] = (uint8_t)byte_at(p);
    }
  }
}

// Commit sets with one template per commit (edc_tmpl_commits_*): tpl[i] = commit_tpl[c] for the
// commit c that holds item i, i.e. the largest c with commit_off[c] <= i (after a run of repeated
// offsets, the empty commits, that is the one the item is in; commit_off[c + 1] > i). The host has
// checked the offsets (commit_off[0] = 0, monotone, commit_off[nc] = n) and commit_tpl.
constexpr int TMPL_MAP_ITEMS = 8;        // consecutive items per lane: one 16-byte store

// largest c in [lo, hi] with off[c] <= i (off[lo] <= i)
__device__ __forceinline__ uint32_t tmpl_commit_of(const uint32_t* __restrict__ off, uint32_t lo, uint32_t hi, uint32_t i) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(TMPL_BLOCK) k_tmpl_commit_map(uint32_t n, uint32_t nc,
                                                               const uint32_t* __restrict__ commit_off,
                                                               const uint16_t* __restrict__ commit_tpl,
                                                               uint16_t* __restrict__ tpl) {
  // the workgroup's items [g0, g1]: their commits bound every lane's search (two searches over all
  // nc offsets with workgroup-uniform addresses, then a few steps per lane)
  const uint32_t g0 = blockIdx.x * (uint32_t)(TMPL_BLOCK * TMPL_MAP_ITEMS);
  const uint32_t g1 = (n - g0 < (uint32_t)(TMPL_BLOCK * TMPL_MAP_ITEMS) ? n : g0 + TMPL_BLOCK * TMPL_MAP_ITEMS) - 1;
  const uint32_t clo = tmpl_commit_of(commit_off, 0, nc - 1, g0), chi = tmpl_commit_of(commit_off, clo, nc - 1, g1);
  const uint32_t i0 = g0 + threadIdx.x * TMPL_MAP_ITEMS;
  if (i0 >= n) return;
  uint32_t c = tmpl_commit_of(commit_off, clo, chi, i0);
  uint32_t end = commit_off[c + 1], t = commit_tpl[c];
  const uint32_t cnt = n - i0 < (uint32_t)TMPL_MAP_ITEMS ? n - i0 : (uint32_t)TMPL_MAP_ITEMS;
  uint32_t w[TMPL_MAP_ITEMS / 2] = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t j = 0; j < (uint32_t)TMPL_MAP_ITEMS; ++j) {
    if (j < cnt) {
      while (i0 + j >= end) {            // next commit, empty ones skipped; i0 + j < n = commit_off[nc] ends it
        ++c;
        end = commit_off[c + 1];
        t = commit_tpl[c];
      }
      w[j >> 1] |= t << (16 * (j & 1));
    }
  }
  if (cnt == (uint32_t)TMPL_MAP_ITEMS && (reinterpret_cast<uintptr_t>(tpl) & 15u) == 0) {
    *reinterpret_cast<uint4*>(tpl + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)TMPL_MAP_ITEMS; ++j)
      if (j < cnt) tpl[i0 + j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
  }
}

void launch_tmpl_commit_map(hipStream_t st, uint32_t n, uint32_t nc, const uint32_t* commit_off,
                            const uint16_t* commit_tpl, uint16_t* tpl) {
  if (!n || !nc) return;
  const uint32_t per = TMPL_BLOCK * TMPL_MAP_ITEMS;
  hipLaunchKernelGGL(k_tmpl_commit_map, dim3((n + per - 1) / per), dim3(TMPL_BLOCK), 0, st, n, nc, commit_off,
                     commit_tpl, tpl);
}

// Commit sets with template variants (edc_tmpl_commits_*_alt / _device): tpl[i] = commit_tpl[c] +
// item_alt[i], one variant byte per item (null: all zeros). The host has checked the offsets and
// that every commit's window [commit_tpl[c], commit_tpl[c] + alt_span) lies inside the set; the
// variant bytes of a device form are checked here. A byte >= alt_span raises the flag of the
// expansion (which then produces n empty messages) and its item gets the commit's base, so every
// value written is below the set's count whether or not the flag has been read.
__global__ void __launch_bounds__(TMPL_BLOCK) k_tmpl_commit_map_alt(uint32_t n, uint32_t nc,
                                                                   const uint32_t* __restrict__ commit_off,
                                                                   const uint16_t* __restrict__ commit_tpl,
                                                                   uint32_t alt_span,
                                                                   const uint8_t* __restrict__ item_alt,
                                                                   uint16_t* __restrict__ tpl, int* __restrict__ flag) {
  // the workgroup's items [g0, g1] bound the lanes' searches, as in k_tmpl_commit_map
  const uint32_t g0 = blockIdx.x * (uint32_t)(TMPL_BLOCK * TMPL_MAP_ITEMS);
  const uint32_t g1 = (n - g0 < (uint32_t)(TMPL_BLOCK * TMPL_MAP_ITEMS) ? n : g0 + TMPL_BLOCK * TMPL_MAP_ITEMS) - 1;
  const uint32_t clo = tmpl_commit_of(commit_off, 0, nc - 1, g0), chi = tmpl_commit_of(commit_off, clo, nc - 1, g1);
  const uint32_t i0 = g0 + threadIdx.x * TMPL_MAP_ITEMS;
  if (i0 >= n) return;
  uint32_t c = tmpl_commit_of(commit_off, clo, chi, i0);
  uint32_t end = commit_off[c + 1], t = commit_tpl[c];
  const uint32_t cnt = n - i0 < (uint32_t)TMPL_MAP_ITEMS ? n - i0 : (uint32_t)TMPL_MAP_ITEMS;
  // the lane's 8 variant bytes: one 8-byte load where the address is 8-byte aligned, else bytes
  uint32_t a[TMPL_MAP_ITEMS / 4] = {0, 0};
  if (item_alt) {
    const uint8_t* p = item_alt + i0;
    if (cnt == (uint32_t)TMPL_MAP_ITEMS && (reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      a[0] = v.x;
      a[1] = v.y;
    } else {
#pragma unroll
      for (uint32_t j = 0; j < (uint32_t)TMPL_MAP_ITEMS; ++j)
        if (j < cnt) a[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
  }
  bool bad = false;
  uint32_t w[TMPL_MAP_ITEMS / 2] = {0, 0, 0, 0};
#pragma unroll
  for (uint32_t j = 0; j < (uint32_t)TMPL_MAP_ITEMS; ++j) {
    if (j < cnt) {
      while (i0 + j >= end) {            // next commit, empty ones skipped; i0 + j < n = commit_off[nc] ends it
        ++c;
        end = commit_off[c + 1];
        t = commit_tpl[c];
      }
      uint32_t v = (a[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      if (v >= alt_span) {               // outside the window: the commit's base, and the flag
        bad = true;
        v = 0;
      }
      w[j >> 1] |= (t + v) << (16 * (j & 1));   // t + v < count <= 65535
    }
  }
  if (bad) atomicOr(flag, 1);
  if (cnt == (uint32_t)TMPL_MAP_ITEMS && (reinterpret_cast<uintptr_t>(tpl + i0) & 15u) == 0) {
    *reinterpret_cast<uint4*>(tpl + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < (uint32_t)TMPL_MAP_ITEMS; ++j)
      if (j < cnt) tpl[i0 + j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
  }
}

void launch_tmpl_commit_map_alt(hipStream_t st, uint32_t n, uint32_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt, uint16_t* tpl,
                                int* flag) {
  if (!n || !nc) return;
  const uint32_t per = TMPL_BLOCK * TMPL_MAP_ITEMS;
  hipLaunchKernelGGL(k_tmpl_commit_map_alt, dim3((n + per - 1) / per), dim3(TMPL_BLOCK), 0, st, n, nc, commit_off,
                     commit_tpl, alt_span, item_alt, tpl, flag);
}

static size_t tmpl_expand_lds(const TmplView& ts, bool lds) {
  const size_t set_room = lds ? (ts.set_bytes + 15u) & ~15u : 0u;
  return set_room + (TMPL_BLOCK + 2) * sizeof(uint64_t) + (TMPL_BLOCK + 4) * sizeof(uint32_t) +
         TMPL_BLOCK * sizeof(uint16_t);
}

size_t tmpl_scan_words(size_t n) { return (n + TMPL_BLOCK - 1) / TMPL_BLOCK + 1; }

void launch_tmpl_expand(hipStream_t st, uint32_t n, const TmplView& ts, const uint16_t* tpl, const uint8_t* var,
                        const uint32_t* var_off, uint64_t var_bytes, int* flag, uint64_t* bsum, uint8_t* out,
                        uint64_t* msg_off) {
  if (!n) return;
  const uint32_t nb = (n + TMPL_BLOCK - 1) / TMPL_BLOCK;
  hipLaunchKernelGGL(k_tmpl_len, dim3(nb), dim3(TMPL_BLOCK), 0, st, n, ts, tpl, var_off, var_bytes, flag, bsum);
  hipLaunchKernelGGL(k_tmpl_scan, dim3(1), dim3(TMPL_SCAN_THREADS), 0, st, nb, flag, bsum);
  const bool lds = ts.set_bytes <= TMPL_LDS_MAX;
  if (lds)
    hipLaunchKernelGGL(k_tmpl_expand<true>, dim3(nb), dim3(TMPL_BLOCK), tmpl_expand_lds(ts, true), st, n, ts, tpl, var,
                       var_off, flag, bsum, out, msg_off);
  else
    hipLaunchKernelGGL(k_tmpl_expand<false>, dim3(nb), dim3(TMPL_BLOCK), tmpl_expand_lds(ts, false), st, n, ts, tpl, var,
                       var_off, flag, bsum, out, msg_off);
}

}  // namespace edc
