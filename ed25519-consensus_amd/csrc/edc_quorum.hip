// Quorum commit sets (quorum.h; edc_quorum_*): which votes of a commit set are verified, and what
// voting power the verified ones carry.
//
// Selection: a segmented exclusive scan of x[i] = (flag[i] == 1 ? power[i] : 0) over the n items,
// the segments being the commits, compared per item with its commit's threshold. Three launches,
// the scan element being a pair (f, v), f = "a commit starts at or before this item inside the
// scanned range", combined as (f1, v1) + (f2, v2) = (f1 | f2, f2 ? v2 : sat(v1 + v2)):
//   k_q_tile    per workgroup of QR_TILE items: the items' commits (binary search of the offsets),
//               the checks of a device form (flag <= 2, power <= 2^63 - 1), the tile's aggregate
//   k_q_carry   one workgroup: exclusive scan of the tile aggregates -> what each tile's first
//               items inherit from the commit that is open when the tile begins
//   k_q_select  per workgroup: the same local scan plus the carry -> the running sum S[i] including
//               item i; S[i] > 2^63 - 1 raises the error flag (the addition saturates, so an
//               overflowing commit is seen whatever the grouping); the exclusive sum S[i] - x[i]
//               against threshold[c] -> the skip byte k_sc_compact reads (1 = leave out), the
//               workgroup's count of checked items for k_sc_scan, and planned[c]
// A commit may span any number of tiles and a tile may hold any number of commits, empty ones
// included: an empty commit owns no item and so never appears in the scan; its planned[c] stays
// the 0 the caller wrote. Integer arithmetic only. planned[c] is an atomic maximum of S over the
// commit's checked flag-1 items (S does not decrease inside a commit, so that is the sum up to the
// last of them); a maximum does not depend on the order of its operands.
//
// Tally (after a failed union, on the scattered item codes): per commit the sum of power over the
// checked flag-1 items with code 0 and the OR of the checked items' codes, by integer atomic add /
// or, which are order-independent as well.
#include "edc_launch.h"
#include "quorum.h"
#include "sigcache.h"

namespace edc {

static_assert(QR_TILE == SC_BLOCK, "the skip bytes and workgroup counts feed k_sc_scan / k_sc_compact");

namespace {

constexpr uint32_t QR_WAVES = QR_TILE / 64;
constexpr uint32_t QR_CARRY_TILE = 1024;          // tile aggregates one pass of k_q_carry covers

__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, uint32_t d) {
  const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
  return ((uint64_t)hi << 32) | lo;
}

// inclusive segmented scan over the NW waves of a workgroup: on return (f, v) covers the
// workgroup's elements up to this lane; (af, av) = the workgroup's aggregate. wv / wf: NW words of LDS.
template <uint32_t NW>
__device__ __forceinline__ void seg_scan_block(uint32_t& f, uint64_t& v, uint32_t& af, uint64_t& av, uint64_t* wv,
                                               uint32_t* wf) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t uv = shfl_up64(v, d);
    const uint32_t uf = __shfl_up(f, d);
    if (lane >= d) {
      if (!f) v = sat_add(uv, v);
      f |= uf;
    }
  }
  if (lane == 63) {
    wv[wave] = v;
    wf[wave] = f;
  }
  __syncthreads();
  uint32_t pf = 0;
  uint64_t pv = 0;
  af = 0;
  av = 0;
  for (uint32_t w = 0; w < NW; ++w) {
    const uint32_t sf = wf[w];
    const uint64_t sv = wv[w];
    if (w == wave) {
      pf = af;
      pv = av;
    }
    av = sf ? sv : sat_add(av, sv);
    af |= sf;
  }
  if (!f) v = sat_add(pv, v);
  f |= pf;
}

// largest c in [lo, hi] with off[c] <= i (off[lo] <= i)
__device__ __forceinline__ uint32_t commit_of(const uint32_t* __restrict__ off, uint32_t lo, uint32_t hi, uint32_t i) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the scan element of item i < n whose commit is c: a commit starts at i iff i is its first item
__device__ __forceinline__ void item_element(const uint32_t* __restrict__ commit_off, const uint64_t* __restrict__ power,
                                             const uint8_t* __restrict__ flag, uint32_t i, uint32_t c, uint32_t& f,
                                             uint64_t& x) {
  f = commit_off[c] == i ? 1u : 0u;
  x = flag[i] == QUORUM_COMMIT ? power[i] : 0;
}

__global__ void __launch_bounds__(QR_TILE) k_q_tile(uint32_t n, uint32_t nc, const uint32_t* __restrict__ commit_off,
                                                    const uint64_t* __restrict__ power,
                                                    const uint8_t* __restrict__ flag, uint32_t* __restrict__ cidx,
                                                    uint64_t* __restrict__ agg_v, uint32_t* __restrict__ agg_f,
                                                    int* __restrict__ err) {
  __shared__ uint64_t wv[QR_WAVES];
  __shared__ uint32_t wf[QR_WAVES];
  // the workgroup's items [g0, g1]: their commits bound every lane's search
  const uint32_t g0 = blockIdx.x * QR_TILE;
  const uint32_t g1 = (n - g0 < QR_TILE ? n : g0 + QR_TILE) - 1;
  const uint32_t clo = commit_of(commit_off, 0, nc - 1, g0), chi = commit_of(commit_off, clo, nc - 1, g1);
  const uint32_t i = g0 + threadIdx.x;
  uint32_t f = 0;
  uint64_t v = 0;
  if (i < n) {
    const uint32_t c = commit_of(commit_off, clo, chi, i);
    cidx[i] = c;
    item_element(commit_off, power, flag, i, c, f, v);
    if (flag[i] > QUORUM_NIL || power[i] > QUORUM_MAX_POWER) *err = 1;
  }
  uint32_t af;
  uint64_t av;
  seg_scan_block<QR_WAVES>(f, v, af, av, wv, wf);
  if (threadIdx.x == 0) {
    agg_v[blockIdx.x] = av;
    agg_f[blockIdx.x] = af;
  }
}

// one workgroup: carry[t] = the sum the open commit has reached when tile t begins (what the
// tile's items before its first commit start add to their own), QR_CARRY_TILE tiles per pass
__global__ void __launch_bounds__(QR_CARRY_TILE) k_q_carry(uint32_t nt, const uint64_t* __restrict__ agg_v,
                                                           const uint32_t* __restrict__ agg_f,
                                                           uint64_t* __restrict__ carry) {
  __shared__ uint64_t wv[QR_CARRY_TILE / 64];
  __shared__ uint32_t wf[QR_CARRY_TILE / 64];
  __shared__ uint64_t incl[QR_CARRY_TILE];
  const uint32_t tid = threadIdx.x;
  uint64_t cv = 0;
  for (uint32_t base = 0; base < nt; base += QR_CARRY_TILE) {
    const uint32_t t = base + tid;
    uint32_t f = t < nt ? agg_f[t] : 0u;
    uint64_t v = t < nt ? agg_v[t] : 0ull;
    uint32_t af;
    uint64_t av;
    seg_scan_block<QR_CARRY_TILE / 64>(f, v, af, av, wv, wf);
    incl[tid] = f ? v : sat_add(cv, v);
    __syncthreads();
    if (t < nt) carry[t] = tid ? incl[tid - 1] : cv;
    cv = incl[QR_CARRY_TILE - 1];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(QR_TILE) k_q_select(uint32_t n, int light, const uint32_t* __restrict__ commit_off,
                                                      const uint64_t* __restrict__ threshold,
                                                      const uint64_t* __restrict__ power,
                                                      const uint8_t* __restrict__ flag,
                                                      const uint32_t* __restrict__ cidx,
                                                      const uint64_t* __restrict__ carry, uint8_t* __restrict__ skip,
                                                      uint32_t* __restrict__ wg_checked,
                                                      unsigned long long* __restrict__ planned, int* __restrict__ err) {
  __shared__ uint64_t wv[QR_WAVES];
  __shared__ uint32_t wf[QR_WAVES];
  __shared__ uint32_t wcnt[QR_WAVES];
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t f = 0, c = 0xFFFFFFFFu;
  uint64_t x = 0;
  uint8_t fl = QUORUM_ABSENT;
  if (i < n) {
    c = cidx[i];
    fl = flag[i];
    item_element(commit_off, power, flag, i, c, f, x);
  }
  uint64_t v = x;
  uint32_t af;
  uint64_t av;
  seg_scan_block<QR_WAVES>(f, v, af, av, wv, wf);
  const uint64_t S = f ? v : sat_add(carry[blockIdx.x], v);     // the commit's counted power up to and with item i
  bool checked = false, counted = false;
  if (i < n) {
    if (S > QUORUM_MAX_POWER) *err = 1;
    // S has not saturated unless the flag is raised, so S - x is the exclusive sum
    checked = light ? (fl == QUORUM_COMMIT && S - x <= threshold[c]) : (fl == QUORUM_COMMIT || fl == QUORUM_NIL);
    counted = checked && fl == QUORUM_COMMIT;
    skip[i] = checked ? 0 : 1;
  }
  // one maximum per run of counted items of one commit inside a wave: S does not decrease along it
  const uint32_t nc_ = __shfl_down(c, 1);
  const int ncounted = __shfl_down((int)counted, 1);
  if (counted && !(lane < 63 && nc_ == c && ncounted)) atomicMax(&planned[c], (unsigned long long)S);
  const uint64_t b = __ballot(checked);
  if (lane == 0) wcnt[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < QR_WAVES; ++w) s += wcnt[w];
    wg_checked[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(QR_TILE) k_q_tally(uint32_t n, const uint32_t* __restrict__ cidx,
                                                     const uint64_t* __restrict__ power,
                                                     const uint8_t* __restrict__ flag, const uint8_t* __restrict__ code,
                                                     unsigned long long* __restrict__ tally, uint32_t* __restrict__ cor) {
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  if (i >= n) return;
  const uint8_t v = code[i];
  if (v == QUORUM_NOT_CHECKED) return;
  const uint32_t c = cidx[i];
  if (v) atomicOr(&cor[c], (uint32_t)v);
  else if (flag[i] == QUORUM_COMMIT && power[i]) atomicAdd(&tally[c], (unsigned long long)power[i]);
}

}  // namespace

size_t quorum_tiles(size_t n) { return (n + QR_TILE - 1) / QR_TILE; }

void launch_quorum_select(hipStream_t st, uint32_t n, uint32_t nc, int light, const uint32_t* commit_off,
                          const uint64_t* threshold, const uint64_t* power, const uint8_t* flag, uint32_t* cidx,
                          uint64_t* agg_v, uint32_t* agg_f, uint64_t* carry, uint8_t* skip, uint32_t* wg_checked,
                          uint64_t* planned, int* err) {
  if (!n || !nc) return;
  const uint32_t nt = (uint32_t)quorum_tiles(n);
  hipLaunchKernelGGL(k_q_tile, dim3(nt), dim3(QR_TILE), 0, st, n, nc, commit_off, power, flag, cidx, agg_v, agg_f, err);
  hipLaunchKernelGGL(k_q_carry, dim3(1), dim3(QR_CARRY_TILE), 0, st, nt, agg_v, agg_f, carry);
  hipLaunchKernelGGL(k_q_select, dim3(nt), dim3(QR_TILE), 0, st, n, light, commit_off, threshold, power, flag, cidx,
                     carry, skip, wg_checked, reinterpret_cast<unsigned long long*>(planned), err);
}

void launch_quorum_tally(hipStream_t st, uint32_t n, const uint32_t* cidx, const uint64_t* power, const uint8_t* flag,
                         const uint8_t* code, uint64_t* tally, uint32_t* cor) {
  if (!n) return;
  hipLaunchKernelGGL(k_q_tally, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, cidx, power, flag, code,
                     reinterpret_cast<unsigned long long*>(tally), cor);
}

}  // namespace edc
