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
#include "vhist.h"

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

// HAVE_CIDX: a second selection over the same commits (the trusting side of a paired request)
// reads the commit indices the first one wrote instead of searching for them again
template <bool HAVE_CIDX>
__global__ void __launch_bounds__(QR_TILE) k_q_tile(uint32_t n, uint32_t nc, const uint32_t* __restrict__ commit_off,
                                                    const uint64_t* __restrict__ power,
                                                    const uint8_t* __restrict__ flag, uint32_t* __restrict__ cidx,
                                                    uint64_t* __restrict__ agg_v, uint32_t* __restrict__ agg_f,
                                                    int* __restrict__ err) {
  __shared__ uint64_t wv[QR_WAVES];
  __shared__ uint32_t wf[QR_WAVES];
  // the workgroup's items [g0, g1]: their commits bound every lane's search
  const uint32_t g0 = blockIdx.x * QR_TILE;
  uint32_t clo = 0, chi = 0;
  if (!HAVE_CIDX) {
    const uint32_t g1 = (n - g0 < QR_TILE ? n : g0 + QR_TILE) - 1;
    clo = commit_of(commit_off, 0, nc - 1, g0);
    chi = commit_of(commit_off, clo, nc - 1, g1);
  }
  const uint32_t i = g0 + threadIdx.x;
  uint32_t f = 0;
  uint64_t v = 0;
  if (i < n) {
    const uint32_t c = HAVE_CIDX ? cidx[i] : commit_of(commit_off, clo, chi, i);
    if (!HAVE_CIDX) cidx[i] = c;
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

// Trusting pairs (edc_vq_verify with trust_ver): one commit set judged by two sets at once. Each
// side runs the selection above on its own power / flag and leaves its own skip bytes and planned[].
//   k_q_union    per tile, behind both: skip[i] = 1 iff neither side checks item i, side[i] = bit 0
//                checked by A | bit 1 checked by B, the tile's count of union items where
//                k_sc_scan / k_sc_compact read the count of a single selection, and the totals
//                {A, B, both} by one integer atomic add per tile and total (order-independent),
//                spread over QR_UNION_SLOTS triples of words that the host sums, because
//                thousands of tiles adding to the same three words serialize on them
//   k_q_tally2   k_q_tally for both sides in one pass over the union's codes: side s counts item i
//                iff bit s of side[i] is set, with its own power and flag, into its own tally / cor
__global__ void __launch_bounds__(QR_TILE) k_q_union(uint32_t n, const uint8_t* __restrict__ skip_a,
                                                     const uint8_t* __restrict__ skip_b, uint8_t* __restrict__ skip,
                                                     uint8_t* __restrict__ side, uint32_t* __restrict__ wg_checked,
                                                     uint32_t* __restrict__ counts) {
  __shared__ uint32_t wa[QR_WAVES], wb[QR_WAVES], wab[QR_WAVES];
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool a = i < n && skip_a[i] == 0, b = i < n && skip_b[i] == 0;
  if (i < n) {
    skip[i] = (a || b) ? 0 : 1;
    side[i] = (uint8_t)((a ? 1 : 0) | (b ? 2 : 0));
  }
  const uint64_t ba = __ballot(a), bb = __ballot(b);
  if (lane == 0) {
    wa[wave] = (uint32_t)__popcll(ba);
    wb[wave] = (uint32_t)__popcll(bb);
    wab[wave] = (uint32_t)__popcll(ba & bb);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sa = 0, sb = 0, sab = 0;
    for (uint32_t w = 0; w < QR_WAVES; ++w) {
      sa += wa[w];
      sb += wb[w];
      sab += wab[w];
    }
    wg_checked[blockIdx.x] = sa + sb - sab;
    uint32_t* slot = counts + 3 * (blockIdx.x % QR_UNION_SLOTS);
    if (sa) atomicAdd(&slot[0], sa);
    if (sb) atomicAdd(&slot[1], sb);
    if (sab) atomicAdd(&slot[2], sab);
  }
}

__global__ void __launch_bounds__(QR_TILE) k_q_tally2(uint32_t n, const uint32_t* __restrict__ cidx,
                                                      const uint8_t* __restrict__ side,
                                                      const uint64_t* __restrict__ power_a,
                                                      const uint8_t* __restrict__ flag_a,
                                                      const uint64_t* __restrict__ power_b,
                                                      const uint8_t* __restrict__ flag_b,
                                                      const uint8_t* __restrict__ code,
                                                      unsigned long long* __restrict__ tally_a, uint32_t* __restrict__ cor_a,
                                                      unsigned long long* __restrict__ tally_b, uint32_t* __restrict__ cor_b) {
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  if (i >= n) return;
  const uint8_t v = code[i];
  if (v == QUORUM_NOT_CHECKED) return;
  const uint32_t c = cidx[i];
  const uint8_t sd = side[i];
  if (sd & 1) {
    if (v) atomicOr(&cor_a[c], (uint32_t)v);
    else if (flag_a[i] == QUORUM_COMMIT && power_a[i]) atomicAdd(&tally_a[c], (unsigned long long)power_a[i]);
  }
  if (sd & 2) {
    if (v) atomicOr(&cor_b[c], (uint32_t)v);
    else if (flag_b[i] == QUORUM_COMMIT && power_b[i]) atomicAdd(&tally_b[c], (unsigned long long)power_b[i]);
  }
}

// Templated quorum commit sets (edc_tmpl_quorum_*): the selection runs first, and only the checked
// votes are gathered, assembled and hashed. Two kernels around the read-back of the checked count:
//   k_tq_holes   per tile, behind k_q_select: var_off[i] <= var_off[i+1] <= var_bytes for ALL n
//                items (bit 1 of the error flag), and the tile's sum of the checked items' hole
//                lengths, which launch_sc_scan turns into the tile's start in the packed holes
//   k_tq_gather  per tile, once the host knows the checked count m and the flag is clear: checked
//                vote j (queue order) gets idx[j], its key, signature and template index, and
//                g_var_off[j]; the tile's holes are one contiguous span of g_var, written in whole
//                aligned 16-byte stores (byte stores only in the span's two partial end chunks,
//                which the neighbouring tiles share), as k_tmpl_expand writes its arena
// Sums of 32-bit lengths: valid offsets make every sum at most var_off[n] - var_off[0] < 2^32, and
// wrapping addition is associative and commutative, so the grouping does not matter.
__global__ void __launch_bounds__(QR_TILE) k_tq_holes(uint32_t n, const uint8_t* __restrict__ skip,
                                                      const uint32_t* __restrict__ var_off, uint64_t var_bytes,
                                                      uint32_t* __restrict__ wg_hole, int* __restrict__ err) {
  __shared__ uint32_t wsum[QR_WAVES];
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t len = 0;
  if (i < n) {
    const uint32_t a = var_off[i], b = var_off[i + 1];
    if (a > b || (uint64_t)b > var_bytes) atomicOr(err, 2);
    else if (skip[i] == 0) len = b - a;
  }
#pragma unroll
  for (uint32_t d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d);
  if (lane == 0) wsum[wave] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < QR_WAVES; ++w) s += wsum[w];
    wg_hole[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(QR_TILE) k_tq_gather(uint32_t n, uint32_t m, const uint8_t* __restrict__ skip,
                                                       const uint32_t* __restrict__ wg_off,
                                                       const uint32_t* __restrict__ wg_hole,
                                                       const uint8_t* __restrict__ vk, const uint8_t* __restrict__ sig,
                                                       const uint16_t* __restrict__ tpl,
                                                       const uint8_t* __restrict__ var,
                                                       const uint32_t* __restrict__ var_off, uint32_t* __restrict__ idx,
                                                       uint8_t* __restrict__ g_vk, uint8_t* __restrict__ g_sig,
                                                       uint16_t* __restrict__ g_tpl, uint8_t* __restrict__ g_var,
                                                       uint32_t* __restrict__ g_var_off) {
  __shared__ uint32_t wcnt[QR_WAVES], wlen[QR_WAVES];
  __shared__ uint32_t s_go[QR_TILE + 1];       // rank r of the tile: where its hole starts in g_var; [cnt] = the span's end
  __shared__ uint32_t s_src[QR_TILE];          // and where it starts in var
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool checked = i < n && skip[i] == 0;
  uint32_t a = 0, len = 0;
  if (checked) {
    a = var_off[i];
    len = var_off[i + 1] - a;
  }
  const uint64_t bal = __ballot(checked);
  uint32_t incl = len;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(incl, d);
    if (lane >= d) incl += u;
  }
  if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
  if (lane == 63) wlen[wave] = incl;
  __syncthreads();
  uint32_t r = (uint32_t)__popcll(bal & ((1ull << lane) - 1)), cnt = 0, excl = incl - len, tot = 0;
  for (uint32_t w = 0; w < QR_WAVES; ++w) {
    if (w < wave) {
      r += wcnt[w];
      excl += wlen[w];
    }
    cnt += wcnt[w];
    tot += wlen[w];
  }
  const uint32_t B = wg_hole[blockIdx.x];
  if (checked) {
    s_go[r] = B + excl;
    s_src[r] = a;
  }
  if (threadIdx.x == 0) s_go[cnt] = B + tot;
  __syncthreads();
  if (checked) {
    const uint32_t j = wg_off[blockIdx.x] + r;
    idx[j] = i;
    const uint4* sa = reinterpret_cast<const uint4*>(vk + (size_t)i * 32);
    const uint4* sb = reinterpret_cast<const uint4*>(sig + (size_t)i * 64);
    uint4* da = reinterpret_cast<uint4*>(g_vk + (size_t)j * 32);
    uint4* db = reinterpret_cast<uint4*>(g_sig + (size_t)j * 64);
    const uint4 q0 = sa[0], q1 = sa[1], q2 = sb[0], q3 = sb[1], q4 = sb[2], q5 = sb[3];
    da[0] = q0; da[1] = q1;
    db[0] = q2; db[1] = q3; db[2] = q4; db[3] = q5;
    g_tpl[j] = tpl[i];
    g_var_off[j] = B + excl;
    if (j == m - 1) g_var_off[m] = B + excl + len;
  }
  if (!tot) return;
  const uint64_t E = (uint64_t)B + tot;
  for (uint64_t c = (B >> 4) + threadIdx.x; c < ((E + 15) >> 4); c += QR_TILE) {
    const uint64_t p0 = (c << 4) > B ? (c << 4) : B, p1 = (c << 4) + 16 < E ? (c << 4) + 16 : E;
    // the hole holding byte p0: the first rank with s_go[rank + 1] > p0 (p0 < E = s_go[cnt], so there is one)
    uint32_t lo = 0, hi = cnt - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (s_go[mid + 1] > p0) hi = mid;
      else lo = mid + 1;
    }
    uint32_t q = lo;
    auto byte_at = [&](uint64_t p) -> uint32_t {
      while (p >= s_go[q + 1]) ++q;      // empty holes in between are skipped; p < E ends it
      return var[(size_t)s_src[q] + (size_t)(p - s_go[q])];
    };
    if (p1 - p0 == 16) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k >> 2] |= byte_at(p0 + k) << (8 * (k & 3));
      *reinterpret_cast<uint4*>(g_var + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (uint64_t p = p0; p < p1; ++p) g_var[p] = (uint8_t)byte_at(p);
    }
  }
}

// Validator-set quorum commit sets (valset.h; edc_valset_*): the powers are the registered list's,
// and a commit in which one validator has two checked votes is refused. Two kernels around the
// selection above:
//   k_vs_resolve  before it, one lane per item: the signer's cache index (kc_lookup on the key
//                 bytes, or kc_reg on a position), then power / flag as the selection reads them
//                 (a member's power and its flag; 0 and EDC_VOTE_ABSENT for anyone else) and
//                 who[i] = the member's cache index or KC_EMPTY. A flag above 2 is passed through
//                 whoever signed, so that k_q_tile raises the error flag on it. Reads the hash
//                 table, the key words and the per-index power / member bytes, never a comb table.
//   k_vs_pairs    behind it, one lane per checked item: the pair (commit, member) goes into an
//                 open-addressing set by a 64-bit compare-and-swap on an empty slot. A lane that
//                 meets its own pair in the set raises dv[c]. Commit c owns the slots
//                 [2 off[c], 2 off[c+1]) of the set, twice its items, so a probe never leaves the
//                 commit's span, never meets a full span and the set is 16 bytes per item.
// Of two lanes with the same pair exactly one wins the empty slot and the other then finds it there
// (nothing is ever removed and both walk the same slots), so dv[c] = 1 iff some pair occurs twice,
// whatever the order of the lanes; the stores to dv[c] all write 1.
// A trusting pair runs the scan once per side, each with that side's skip bytes, its who[] and a set
// and dv[] of its own: every launch sees one set in which commit c owns [2 off[c], 2 off[c+1]) and
// inserts at most one pair per item of c, so the argument holds per side as it stands: a probe never
// leaves the commit's span and never meets a full span.
// the cache index of item i's signer: by its key bytes (KC_EMPTY for a key the cache does not hold)
// or, with vk null, by its position in the registered list
__device__ __forceinline__ uint32_t signer_index(const KeyCacheView& kc, const uint8_t* __restrict__ vk,
                                                 const uint32_t* __restrict__ key_idx,
                                                 const uint32_t* __restrict__ reg, uint32_t i) {
  if (!vk) return reg[key_idx[i]];      // the host checked key_idx[i] against the list's length
  const uint4* q = reinterpret_cast<const uint4*>(vk + (size_t)i * 32);
  const uint4 a = q[0], b = q[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const int r = kc_lookup(kc, w);
  return r < 0 ? KC_EMPTY : (uint32_t)r;
}

__global__ void __launch_bounds__(QR_TILE) k_vs_resolve(uint32_t n, KeyCacheView kc, ValsetView vs,
                                                        const uint8_t* __restrict__ vk,
                                                        const uint32_t* __restrict__ key_idx,
                                                        const uint32_t* __restrict__ reg,
                                                        const uint8_t* __restrict__ flag, uint64_t* __restrict__ power,
                                                        uint8_t* __restrict__ flag_out, uint32_t* __restrict__ who) {
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = signer_index(kc, vk, key_idx, reg, i);
  const bool member = c < vs.count && vs.member[c];
  const uint8_t fl = flag[i];
  power[i] = member ? vs.power[c] : 0;
  flag_out[i] = (member || fl > QUORUM_NIL) ? fl : QUORUM_ABSENT;
  who[i] = member ? c : KC_EMPTY;
}

// Validator-set history (vhist.h; edc_vhist_*): the join of k_vs_resolve with every commit judged
// by the set of its own version. One lane per item, in front of the selection: the signer's cache
// index as above; the item's commit by the search k_q_tile makes, bounded by the commits of the
// tile's first and last item, so that an empty commit resolves here as it does there and the
// version read is that of the commit k_q_tile then writes to cidx[i]; the signer's change list
// [off[s], off[s+1]) searched for the last entry with ver <= commit_ver[c] (the base entry has
// version 0, so a list of one entry is not searched at all); its pow, or no member for
// VHIST_NOT_MEMBER, an empty list or a cache index past the history. Writes what k_vs_resolve
// writes, so the selection and k_vs_pairs run unchanged behind it. The loads depend on each other
// (key -> index -> offsets -> versions -> power); the searched array is 32-bit versions only.
__global__ void __launch_bounds__(QR_TILE) k_vh_resolve(uint32_t n, uint32_t nc, KeyCacheView kc, VhistView vh,
                                                        const uint32_t* __restrict__ commit_off,
                                                        const uint32_t* __restrict__ commit_ver,
                                                        const uint8_t* __restrict__ vk,
                                                        const uint32_t* __restrict__ key_idx,
                                                        const uint32_t* __restrict__ reg,
                                                        const uint8_t* __restrict__ flag, uint64_t* __restrict__ power,
                                                        uint8_t* __restrict__ flag_out, uint32_t* __restrict__ who) {
  const uint32_t g0 = blockIdx.x * QR_TILE;
  const uint32_t g1 = (n - g0 < QR_TILE ? n : g0 + QR_TILE) - 1;
  const uint32_t clo = commit_of(commit_off, 0, nc - 1, g0), chi = commit_of(commit_off, clo, nc - 1, g1);
  const uint32_t i = g0 + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = signer_index(kc, vk, key_idx, reg, i);
  const uint32_t v = commit_ver[commit_of(commit_off, clo, chi, i)];
  uint64_t pw = VHIST_NOT_MEMBER;
  if (s < vh.count) pw = vh_power_at(vh, vh.off[s], vh.off[s + 1], v);
  const bool member = pw != VHIST_NOT_MEMBER;
  const uint8_t fl = flag[i];
  power[i] = member ? pw : 0;
  flag_out[i] = (member || fl > QUORUM_NIL) ? fl : QUORUM_ABSENT;
  who[i] = member ? s : KC_EMPTY;
}

// Trusting pairs: k_vh_resolve for two versions of one commit. One signer lookup and one commit
// search per vote, one read of the signer's list bounds, then two searches of that same list, for
// commit_ver[c] (side A) and trust_ver[c] (side B); VQ_NO_TRUST makes the signer no member on side
// B without a search. Each side gets the three arrays k_vh_resolve writes. A flag above 2 is passed
// through on both sides, so the selection's check raises it on whichever runs.
__global__ void __launch_bounds__(QR_TILE) k_vh_resolve2(uint32_t n, uint32_t nc, KeyCacheView kc, VhistView vh,
                                                         const uint32_t* __restrict__ commit_off,
                                                         const uint32_t* __restrict__ commit_ver,
                                                         const uint32_t* __restrict__ trust_ver,
                                                         const uint8_t* __restrict__ vk,
                                                         const uint32_t* __restrict__ key_idx,
                                                         const uint32_t* __restrict__ reg,
                                                         const uint8_t* __restrict__ flag, uint64_t* __restrict__ power_a,
                                                         uint8_t* __restrict__ flag_a, uint32_t* __restrict__ who_a,
                                                         uint64_t* __restrict__ power_b, uint8_t* __restrict__ flag_b,
                                                         uint32_t* __restrict__ who_b) {
  const uint32_t g0 = blockIdx.x * QR_TILE;
  const uint32_t g1 = (n - g0 < QR_TILE ? n : g0 + QR_TILE) - 1;
  const uint32_t clo = commit_of(commit_off, 0, nc - 1, g0), chi = commit_of(commit_off, clo, nc - 1, g1);
  const uint32_t i = g0 + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = signer_index(kc, vk, key_idx, reg, i);
  const uint32_t c = commit_of(commit_off, clo, chi, i);
  const uint32_t va = commit_ver[c], vb = trust_ver[c];
  uint64_t pa = VHIST_NOT_MEMBER, pb = VHIST_NOT_MEMBER;
  if (s < vh.count) {
    const uint32_t lo = vh.off[s], end = vh.off[s + 1];
    pa = vh_power_at(vh, lo, end, va);
    if (vb != VQ_NO_TRUST) pb = vh_power_at(vh, lo, end, vb);
  }
  const bool ma = pa != VHIST_NOT_MEMBER, mb = pb != VHIST_NOT_MEMBER;
  const uint8_t fl = flag[i];
  power_a[i] = ma ? pa : 0;
  flag_a[i] = (ma || fl > QUORUM_NIL) ? fl : QUORUM_ABSENT;
  who_a[i] = ma ? s : KC_EMPTY;
  power_b[i] = mb ? pb : 0;
  flag_b[i] = (mb || fl > QUORUM_NIL) ? fl : QUORUM_ABSENT;
  who_b[i] = mb ? s : KC_EMPTY;
}

__global__ void __launch_bounds__(QR_TILE) k_vs_pairs(uint32_t n, const uint32_t* __restrict__ commit_off,
                                                      const uint32_t* __restrict__ cidx,
                                                      const uint8_t* __restrict__ skip,
                                                      const uint32_t* __restrict__ who,
                                                      unsigned long long* __restrict__ set, uint8_t* __restrict__ dv) {
  const uint32_t i = blockIdx.x * QR_TILE + threadIdx.x;
  if (i >= n || skip[i]) return;
  const uint32_t m = who[i];
  if (m == KC_EMPTY) return;
  const uint32_t c = cidx[i];
  const uint32_t a = commit_off[c], slots = 2 * (commit_off[c + 1] - a);      // item i is one of them: slots >= 2
  if (!slots) return;
  unsigned long long* span = set + 2 * (size_t)a;
  const unsigned long long pair = ((unsigned long long)c << 32) | (m + 1);   // never 0, the empty slot
  uint32_t h = (uint32_t)(((uint64_t)(m * 0x9E3779B1u) * slots) >> 32);
  for (uint32_t probe = 0; probe < slots; ++probe) {
    const unsigned long long old = atomicCAS(&span[h], 0ull, pair);
    if (old == 0) return;
    if (old == pair) {
      dv[c] = 1;
      return;
    }
    h = h + 1 == slots ? 0 : h + 1;
  }
}

}  // namespace

size_t quorum_tiles(size_t n) { return (n + QR_TILE - 1) / QR_TILE; }

void launch_tmpl_quorum_holes(hipStream_t st, uint32_t n, const uint8_t* skip, const uint32_t* var_off,
                              uint64_t var_bytes, uint32_t* wg_hole, int* err) {
  if (!n) return;
  hipLaunchKernelGGL(k_tq_holes, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, skip, var_off, var_bytes,
                     wg_hole, err);
}

void launch_tmpl_quorum_gather(hipStream_t st, uint32_t n, uint32_t m, const uint8_t* skip, const uint32_t* wg_off,
                               const uint32_t* wg_hole, const uint8_t* vk, const uint8_t* sig, const uint16_t* tpl,
                               const uint8_t* var, const uint32_t* var_off, uint32_t* idx, uint8_t* g_vk, uint8_t* g_sig,
                               uint16_t* g_tpl, uint8_t* g_var, uint32_t* g_var_off) {
  if (!n || !m) return;
  hipLaunchKernelGGL(k_tq_gather, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, m, skip, wg_off, wg_hole, vk,
                     sig, tpl, var, var_off, idx, g_vk, g_sig, g_tpl, g_var, g_var_off);
}

void launch_quorum_select(hipStream_t st, uint32_t n, uint32_t nc, int light, const uint32_t* commit_off,
                          const uint64_t* threshold, const uint64_t* power, const uint8_t* flag, uint32_t* cidx,
                          uint64_t* agg_v, uint32_t* agg_f, uint64_t* carry, uint8_t* skip, uint32_t* wg_checked,
                          uint64_t* planned, int* err, bool have_cidx) {
  if (!n || !nc) return;
  const uint32_t nt = (uint32_t)quorum_tiles(n);
  if (have_cidx)
    hipLaunchKernelGGL(k_q_tile<true>, dim3(nt), dim3(QR_TILE), 0, st, n, nc, commit_off, power, flag, cidx, agg_v, agg_f,
                       err);
  else
    hipLaunchKernelGGL(k_q_tile<false>, dim3(nt), dim3(QR_TILE), 0, st, n, nc, commit_off, power, flag, cidx, agg_v, agg_f,
                       err);
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

void launch_quorum_union(hipStream_t st, uint32_t n, const uint8_t* skip_a, const uint8_t* skip_b, uint8_t* skip,
                         uint8_t* side, uint32_t* wg_checked, uint32_t* counts) {
  if (!n) return;
  hipLaunchKernelGGL(k_q_union, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, skip_a, skip_b, skip, side,
                     wg_checked, counts);
}

void launch_quorum_tally2(hipStream_t st, uint32_t n, const uint32_t* cidx, const uint8_t* side, const uint64_t* power_a,
                          const uint8_t* flag_a, const uint64_t* power_b, const uint8_t* flag_b, const uint8_t* code,
                          uint64_t* tally_a, uint32_t* cor_a, uint64_t* tally_b, uint32_t* cor_b) {
  if (!n) return;
  hipLaunchKernelGGL(k_q_tally2, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, cidx, side, power_a, flag_a,
                     power_b, flag_b, code, reinterpret_cast<unsigned long long*>(tally_a), cor_a,
                     reinterpret_cast<unsigned long long*>(tally_b), cor_b);
}

void launch_vhist_resolve2(hipStream_t st, uint32_t n, uint32_t nc, const KeyCacheView& kc, const VhistView& vh,
                           const uint32_t* commit_off, const uint32_t* commit_ver, const uint32_t* trust_ver,
                           const uint8_t* vk, const uint32_t* key_idx, const uint32_t* reg, const uint8_t* flag,
                           uint64_t* power_a, uint8_t* flag_a, uint32_t* who_a, uint64_t* power_b, uint8_t* flag_b,
                           uint32_t* who_b) {
  if (!n || !nc) return;
  hipLaunchKernelGGL(k_vh_resolve2, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, nc, kc, vh, commit_off,
                     commit_ver, trust_ver, vk, key_idx, reg, flag, power_a, flag_a, who_a, power_b, flag_b, who_b);
}

void launch_valset_resolve(hipStream_t st, uint32_t n, const KeyCacheView& kc, const ValsetView& vs, const uint8_t* vk,
                           const uint32_t* key_idx, const uint32_t* reg, const uint8_t* flag, uint64_t* power,
                           uint8_t* flag_out, uint32_t* who) {
  if (!n) return;
  hipLaunchKernelGGL(k_vs_resolve, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, kc, vs, vk, key_idx, reg, flag,
                     power, flag_out, who);
}

void launch_vhist_resolve(hipStream_t st, uint32_t n, uint32_t nc, const KeyCacheView& kc, const VhistView& vh,
                          const uint32_t* commit_off, const uint32_t* commit_ver, const uint8_t* vk,
                          const uint32_t* key_idx, const uint32_t* reg, const uint8_t* flag, uint64_t* power,
                          uint8_t* flag_out, uint32_t* who) {
  if (!n || !nc) return;
  hipLaunchKernelGGL(k_vh_resolve, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, nc, kc, vh, commit_off,
                     commit_ver, vk, key_idx, reg, flag, power, flag_out, who);
}

void launch_valset_pairs(hipStream_t st, uint32_t n, const uint32_t* commit_off, const uint32_t* cidx, const uint8_t* skip,
                         const uint32_t* who, uint64_t* set, uint8_t* dv) {
  if (!n) return;
  hipLaunchKernelGGL(k_vs_pairs, dim3((uint32_t)quorum_tiles(n)), dim3(QR_TILE), 0, st, n, commit_off, cidx, skip, who,
                     reinterpret_cast<unsigned long long*>(set), dv);
}

}  // namespace edc
