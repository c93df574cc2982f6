// Host-side launchers for every kernel (one translation unit per kernel family).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "keycache.h"
#include "edc_common.h"
#include "devbuf.h"

namespace edc {
// edc_prep.hip
void launch_challenge(hipStream_t st, uint32_t n, const uint8_t* vk, const uint8_t* sig,
                      const uint8_t* msg, const uint64_t* off, uint32_t* k);
void launch_decompress(hipStream_t st, uint32_t n, const uint8_t* sig, const uint8_t* vk, const uint32_t* key_rep,
                       bool per_sig, uint32_t* pts, uint8_t* itembad, uint8_t* keybad, int* flags,
                       const KeyCacheView& kc, bool split = false, uint32_t klanes = 0);
// R of items [r0, r0 + rcnt) of an n-item batch, and the distinct keys on klanes lanes (0: none;
// launch_decompress: 0 = n, one lane per possible key)
void launch_decompress_range(hipStream_t st, uint32_t n, uint32_t r0, uint32_t rcnt, uint32_t klanes, const uint8_t* sig,
                             const uint8_t* vk, const uint32_t* key_rep, bool per_sig, uint32_t* pts, uint8_t* itembad,
                             uint8_t* keybad, int* flags, const KeyCacheView& kc, bool split = false);
void launch_keys(hipStream_t st, uint32_t n, const uint8_t* vk, uint32_t* table, uint32_t tmask,
                 const uint32_t salt[2], bool force_overflow, uint32_t* slot_key, uint32_t* key_slot_of_sig,
                 uint32_t* key_rep, uint32_t* key_index, unsigned long long* key_acc, int* flags,
                 uint32_t kcap = 0xFFFFFFFFu);
// incremental verifier (edc_verifier_*): find-or-insert of items [n0, n0 + m) against a populated
// table (key indices continue from flags[FLAG_NKEYS]), their key_index, and the decode of the keys
// first seen in the range into row key_index of kpts and, while the context has a key cache, of
// their [2^128] multiples into khi; seed_pass: the sampling pass of launch_keys for a large first
// append
void launch_keys_range(hipStream_t st, uint32_t n0, uint32_t m, const uint8_t* vk, uint32_t* table, uint32_t tmask,
                       const uint32_t salt[2], bool force_overflow, bool seed_pass, uint32_t* slot_key,
                       uint32_t* key_slot_of_sig, uint32_t* key_rep, uint32_t* key_index, unsigned long long* key_acc,
                       uint32_t* kpts, uint32_t* khi, uint8_t* keybad, int* flags, const KeyCacheView& kc);
// start of a verify over n queued items: clears the per-call sums, the result block and counts
void launch_verifier_begin(hipStream_t st, uint32_t n, int* flags, unsigned long long* key_acc,
                           unsigned long long* u_acc, uint8_t* d_out, uint32_t* counts, uint32_t nbin);
// key rows 1 + n + j of the batch layout from kpts (after an overflow: every A_i decoded); split:
// the split layout of edc_common.h, [2^128]B from the cache and the [2^128]A_j rows from khi
void launch_verifier_place_keys(hipStream_t st, uint32_t n, const uint8_t* vk, const uint32_t* kpts, const uint32_t* khi,
                                uint32_t* pts, uint8_t* keybad, int* flags, const KeyCacheView& kc, bool split);
// eager verifier: z_i of items [a, a + cnt) drawn from the seed as launch_coef draws them (queue
// index i: words 4 (i & 3).. of ChaCha block i >> 2), stored as the short scalar of row 1 + i
void launch_z_range(hipStream_t st, const uint32_t seed[8], uint32_t a, uint32_t cnt, uint32_t* scal);
// per-signature key terms (no grouping): m = n, key j is signature j's own key (key_rep = null)
void launch_coef(hipStream_t st, uint32_t n, const uint8_t* sig, const uint32_t* k, const uint8_t* zexp,
                 const uint32_t seed[8], uint64_t zbase, const uint32_t* key_index, uint32_t* scal,
                 unsigned long long* key_acc, unsigned long long* u_acc, uint8_t* itembad, int* flags,
                 bool per_sig, uint32_t* coef_part, bool split = false);
// launch_coef in pieces (chunked host-buffer calls): the per-item pass over items
// [item0, item0 + cnt) (item0 a multiple of COEF_CHUNK) as each chunk lands, then once the
// per-key merge and the coefficient reduction
void launch_coef_range(hipStream_t st, uint32_t n, uint32_t item0, uint32_t cnt, const uint8_t* sig, const uint32_t* k,
                       const uint8_t* zexp, const uint32_t seed[8], uint64_t zbase, const uint32_t* key_index,
                       uint32_t* scal, unsigned long long* key_acc, unsigned long long* u_acc, uint8_t* itembad,
                       int* flags, bool per_sig, uint32_t* coef_part, bool split = false);
void launch_coef_finish(hipStream_t st, uint32_t n, unsigned long long* key_acc, unsigned long long* u_acc,
                        uint32_t* scal, int* flags, bool per_sig, uint32_t* coef_part, bool split = false);
// words of k_coef's per-workgroup key-slot dump for batches of up to cap_n signatures
size_t coef_part_words(size_t cap_n);
// grouped fallback: per-(range, key) / per-range coefficients as listed MSM terms
void launch_range_coef(hipStream_t st, uint32_t n, uint32_t rsize, uint32_t nranges, uint32_t m, bool per_sig,
                       const uint8_t* sig, const uint32_t* k, const uint8_t* zexp, const uint32_t seed[8],
                       uint64_t zbase, const uint32_t* key_index, uint32_t* scal, unsigned long long* key_acc,
                       unsigned long long* u_acc, int* flags, uint32_t* xpt, uint32_t* xrg, uint32_t* xscal);
// several batches in one launch (nr equal ranges of n / nr items, n / nr a multiple of COEF_CHUNK):
// per-item z and s checks, per-(range, key) sums at g * kstride + key (grouped keys; more than
// kstride distinct keys must have set FLAG_OVF: launch_keys' kcap), listed key / B terms
void launch_multi_coef(hipStream_t st, uint32_t n, uint32_t nr, uint32_t kstride, bool per_sig, const uint8_t* sig,
                       const uint32_t* k, const uint32_t seed[8], uint64_t zbase, const uint32_t* key_index,
                       uint32_t* scal, unsigned long long* key_acc, unsigned long long* u_acc, uint8_t* itembad,
                       int* flags, uint32_t* xpt, uint32_t* xrg, uint32_t* xscal);
void launch_range_prebad(hipStream_t st, uint32_t n, uint32_t rsize, const uint8_t* itembad, const uint8_t* itembad_r,
                         const uint8_t* keybad,
                         const uint32_t* key_index, bool per_sig, uint8_t* rbad, const int* flags = nullptr);
void launch_init_basepoint(hipStream_t st, uint32_t* pts);
void launch_sc_reduce_wide(hipStream_t st, uint32_t n, const uint32_t* in, uint32_t* out);
void launch_gather_items(hipStream_t st, uint32_t c, const uint32_t* idx, const uint8_t* vk, const uint8_t* sig,
                         const uint32_t* k, uint8_t* out_vk, uint8_t* out_sig, uint32_t* out_k);
// vk_out[i] = keys[reg[key_idx[i]]] (32 bytes each; key-indexed host submissions)
void launch_expand_keys(hipStream_t st, uint32_t n, const uint32_t* key_idx, const uint32_t* reg,
                        const uint32_t* keys, uint8_t* vk_out);
// per-batch resets in one launch: flags (FLAG_NKEYS = nkeys if >= 0), u_acc, the 256-byte result
// block, table[0..T) = 0xFFFFFFFF, counts[0..nbin) = 0 (T / nbin may be 0)
void launch_init_batch(hipStream_t st, int* flags, int nkeys, unsigned long long* u_acc, uint8_t* d_out, uint32_t* table,
                       uint32_t T, uint32_t* counts, uint32_t nbin);
// edc_tmpl.hip: templated messages. The device copy of a template set is one allocation,
// head_off | tail_off (count + 1 words each) | head | tail, readable up to the next multiple of
// 16 bytes past set_bytes.
struct TmplView {
  const uint32_t *head_off, *tail_off;
  const uint8_t *head, *tail;
  uint32_t count, head_bytes, set_bytes;
};
// lengths (validated: *flag, zeroed by the caller, is raised on a bad index / offset), scan and
// expansion of n items into out / msg_off[n + 1]; out 16-byte aligned, bsum tmpl_scan_words(n) words
void launch_tmpl_expand(hipStream_t st, uint32_t n, const TmplView& ts, const uint16_t* tpl, const uint8_t* var,
                        const uint32_t* var_off, uint64_t var_bytes, int* flag, uint64_t* bsum, uint8_t* out,
                        uint64_t* msg_off);
size_t tmpl_scan_words(size_t n);
// commit sets with one template per commit: tpl[i] = commit_tpl[c] for the commit c holding item i
// (nc + 1 checked offsets, commit_off[nc] = n; empty commits allowed). All device pointers.
void launch_tmpl_commit_map(hipStream_t st, uint32_t n, uint32_t nc, const uint32_t* commit_off,
                            const uint16_t* commit_tpl, uint16_t* tpl);
// the same with template variants: tpl[i] = commit_tpl[c] + item_alt[i] (item_alt null: zeros). The
// windows [commit_tpl[c], commit_tpl[c] + alt_span) are checked by the host; a byte >= alt_span
// raises *flag (the expansion's, cleared by the caller before this launch) and maps to the base.
void launch_tmpl_commit_map_alt(hipStream_t st, uint32_t n, uint32_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt, uint16_t* tpl,
                                int* flag);
// edc_quorum.hip (quorum.h): the selection of a quorum commit set. All device pointers; commit_off
// (nc + 1 checked offsets, commit_off[nc] = n) and threshold (nc) staged by the caller. Outputs:
// skip[i] = 0 iff item i is checked (the byte k_sc_compact reads), wg_checked = checked items per
// workgroup of QR_TILE (= SC_BLOCK) items for launch_sc_scan, planned[c] (zeroed by the caller) =
// the power of commit c's checked flag-1 items, cidx[i] = the commit of item i. *err (zeroed by
// the caller) is raised on a flag above 2, a power above 2^63 - 1 or a commit whose counted sum
// passes 2^63 - 1; the other outputs then mean nothing (every index formed stays inside the arrays).
// agg_v / agg_f / carry: quorum_tiles(n) words each. n = 0 launches nothing.
constexpr uint32_t QR_TILE = 256;
size_t quorum_tiles(size_t n);
void launch_quorum_select(hipStream_t st, uint32_t n, uint32_t nc, int light, const uint32_t* commit_off,
                          const uint64_t* threshold, const uint64_t* power, const uint8_t* flag, uint32_t* cidx,
                          uint64_t* agg_v, uint32_t* agg_f, uint64_t* carry, uint8_t* skip, uint32_t* wg_checked,
                          uint64_t* planned, int* err, bool have_cidx = false);
// trusting pairs (edc_vq_verify with trust_ver): launch_quorum_select runs once per side, the second
// time with have_cidx (cidx is read, not searched for again), each into its own skip bytes and
// planned[]. launch_quorum_union then writes what the back-ends read of ONE selection: skip[i] = 1
// iff neither side checks item i, wg_checked[t] = tile t's union count (for launch_sc_scan),
// side[i] = bit 0 checked by A | bit 1 checked by B, and adds the totals {A, B, both} to one of
// QR_UNION_SLOTS triples of counts (3 * QR_UNION_SLOTS words, zeroed by the caller, who sums them). launch_quorum_tally2 is launch_quorum_tally for both sides in one pass:
// side s counts item i iff bit s of side[i] is set, with its own power and flag.
constexpr uint32_t QR_UNION_SLOTS = 64;
void launch_quorum_union(hipStream_t st, uint32_t n, const uint8_t* skip_a, const uint8_t* skip_b, uint8_t* skip,
                         uint8_t* side, uint32_t* wg_checked, uint32_t* counts);
void launch_quorum_tally2(hipStream_t st, uint32_t n, const uint32_t* cidx, const uint8_t* side, const uint64_t* power_a,
                          const uint8_t* flag_a, const uint64_t* power_b, const uint8_t* flag_b, const uint8_t* code,
                          uint64_t* tally_a, uint32_t* cor_a, uint64_t* tally_b, uint32_t* cor_b);
// after a failed union: code[i] = item i's code, 255 where it was not checked. tally[c] += power of
// the checked flag-1 items with code 0, cor[c] |= the checked items' codes (both zeroed by the caller)
void launch_quorum_tally(hipStream_t st, uint32_t n, const uint32_t* cidx, const uint64_t* power, const uint8_t* flag,
                         const uint8_t* code, uint64_t* tally, uint32_t* cor);
// templated quorum commit sets (edc_tmpl_quorum_*): the gather of the checked votes with their
// holes. launch_tmpl_quorum_holes runs behind the selection, on all n items: *err |= 2 unless
// var_off[i] <= var_off[i+1] <= var_bytes for every item, wg_hole[t] = the hole bytes of tile t's
// checked items (quorum_tiles(n) + 1 words: launch_sc_scan makes them the tiles' starts and the
// total). launch_tmpl_quorum_gather runs once the flag is known clear and m, the checked count,
// is known (0 < m): wg_off / wg_hole are the scanned counts and hole bytes, tpl the all-n template
// array; checked vote j gets idx[j], g_vk / g_sig row j, g_tpl[j] and its hole at g_var_off[j] of
// g_var (16-byte aligned, room for the scanned total), g_var_off[m] = that total.
void launch_tmpl_quorum_holes(hipStream_t st, uint32_t n, const uint8_t* skip, const uint32_t* var_off,
                              uint64_t var_bytes, uint32_t* wg_hole, int* err);
void launch_tmpl_quorum_gather(hipStream_t st, uint32_t n, uint32_t m, const uint8_t* skip, const uint32_t* wg_off,
                               const uint32_t* wg_hole, const uint8_t* vk, const uint8_t* sig, const uint16_t* tpl,
                               const uint8_t* var, const uint32_t* var_off, uint32_t* idx, uint8_t* g_vk, uint8_t* g_sig,
                               uint16_t* g_tpl, uint8_t* g_var, uint32_t* g_var_off);
// validator-set quorum commit sets (valset.h; edc_valset_*). The powers of the registered list,
// indexed by cache index (count entries; a cache index at or past count is no member): power[c],
// member[c] = 1 iff key c is a member, pos[c] = its position in the list.
struct ValsetView {
  const uint64_t* power;
  const uint8_t* member;
  const uint32_t* pos;
  uint32_t count;
};
// launch_valset_resolve runs before the selection, on all n items: item i's signer is looked up by
// its key bytes (vk, 16-byte aligned) or by its position (key_idx into reg, every entry checked by
// the caller; vk null); power[i] / flag_out[i] are the selection's inputs (a flag above 2 is kept
// so that the selection's checks refuse it), who[i] the member's cache index or KC_EMPTY.
// launch_valset_pairs runs behind the selection, on its skip bytes and commit indices: dv[c] (nc
// bytes, zeroed by the caller) = 1 iff two checked items of commit c have the same who; set: 2 n
// words, zeroed by the caller.
void launch_valset_resolve(hipStream_t st, uint32_t n, const KeyCacheView& kc, const ValsetView& vs, const uint8_t* vk,
                           const uint32_t* key_idx, const uint32_t* reg, const uint8_t* flag, uint64_t* power,
                           uint8_t* flag_out, uint32_t* who);
void launch_valset_pairs(hipStream_t st, uint32_t n, const uint32_t* commit_off, const uint32_t* cidx, const uint8_t* skip,
                         const uint32_t* who, uint64_t* set, uint8_t* dv);
// validator-set history (vhist.h; edc_vhist_*). The change lists by cache index: key s owns the
// entries [off[s], off[s+1]) (count + 1 offsets; empty for a key outside the list, and a cache
// index at or past count is no member at any version), ver[] ascending from the base's 0, pow[]
// the power from that version on or VHIST_NOT_MEMBER.
struct VhistView {
  const uint32_t* off;
  const uint32_t* ver;
  const uint64_t* pow;
  uint32_t count;
};
#if defined(__HIPCC__)
// the power of the change list [lo, end) at version v: its last entry with ver <= v (ver[lo] = 0 <= v,
// so a list of one entry is not searched); VHIST_NOT_MEMBER (~0) for an empty list. The one search
// of the history on the device: the join kernels (edc_quorum.hip) and the root kernel
// (edc_valhash.hip) both resolve a power with it.
__device__ __forceinline__ uint64_t vh_power_at(const VhistView& vh, uint32_t lo, uint32_t end, uint32_t v) {
  if (lo >= end) return ~0ull;
  uint32_t hi = end - 1;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (vh.ver[mid] <= v) lo = mid;
    else hi = mid - 1;
  }
  return vh.pow[lo];
}
#endif
// launch_vhist_resolve stands where launch_valset_resolve does and writes the same three arrays,
// with item i judged at commit_ver[c], c the commit of i by commit_off (nc + 1 offsets and nc
// versions on the device, every version checked by the caller against the history).
void launch_vhist_resolve(hipStream_t st, uint32_t n, uint32_t nc, const KeyCacheView& kc, const VhistView& vh,
                          const uint32_t* commit_off, const uint32_t* commit_ver, const uint8_t* vk,
                          const uint32_t* key_idx, const uint32_t* reg, const uint8_t* flag, uint64_t* power,
                          uint8_t* flag_out, uint32_t* who);
// launch_vhist_resolve for a trusting pair: item i judged at commit_ver[c] (side A) and at
// trust_ver[c] (side B; VQ_NO_TRUST: no member on that side), with one signer lookup, one commit
// search and one read of the list bounds for both.
void launch_vhist_resolve2(hipStream_t st, uint32_t n, uint32_t nc, const KeyCacheView& kc, const VhistView& vh,
                           const uint32_t* commit_off, const uint32_t* commit_ver, const uint32_t* trust_ver,
                           const uint8_t* vk, const uint32_t* key_idx, const uint32_t* reg, const uint8_t* flag,
                           uint64_t* power_a, uint8_t* flag_a, uint32_t* who_a, uint64_t* power_b, uint8_t* flag_b,
                           uint32_t* who_b);
// edc_valhash.hip: validator-set hashes (valhash.h; edc_valhash_valset, edc_valhash_vhist,
// edc_valhash_vhist_match). What the root kernel reads: the registered list (m positions, reg[p] the
// cache index of position p, keys the cache's raw key words), the set (hist: the history's change
// lists, else the one set's powers) and the address order (rank[p] of position p; by_rank[r] the
// cache index of the position with rank r).
struct ValhashSrc {
  const uint32_t* keys;
  const uint32_t* reg;
  uint32_t m;
  bool hist;
  VhistView vh;
  ValsetView vs;
  const uint32_t* rank;
  const uint32_t* by_rank;
};
// addr (m x 20 bytes, by position) = the first 20 bytes of SHA-256 of each position's key
void launch_valhash_addr(hipStream_t st, uint32_t m, const uint32_t* keys, const uint32_t* reg, uint8_t* addr);
// One workgroup per root: root j (32 bytes at roots + 32 j) is that of version vers[j], or of
// v0 + j with vers null; a source without a history has one set and ignores the version.
// max_members: no requested version holds more (at most VALHASH_MAX_MEMBERS; the caller checked).
// It sizes the workgroup's LDS, up to the 112 KB valhash_init_device allows: per-device kernel
// attributes (the root kernel's dynamic LDS beyond 64 KB); call on every device a context uses,
// after hipSetDevice, as msm_init_device.
hipError_t valhash_init_device();
hipError_t launch_valhash_roots(hipStream_t st, const ValhashSrc& src, uint32_t nroots, const uint32_t* vers, uint32_t v0,
                          uint32_t max_members, uint8_t* roots);
// ok[c] = 1 iff the 32 bytes at expect + 32 c equal root idx[c]
void launch_valhash_match(hipStream_t st, uint32_t nc, const uint8_t* roots, const uint32_t* idx, const uint8_t* expect,
                          uint8_t* ok);
// edc_header.hip: header hashes (hdrhash.h; edc_header_hashes, edc_header_bind). A header set on
// the device: header h owns the leaves [leaf_off[h], leaf_off[h + 1]) (at most HEADER_MAX_LEAVES),
// leaf j the bytes [byte_off[j], byte_off[j + 1]) of the byte array, which is held as aligned words:
// a whole number of them, zero behind the last byte, so that the word of any byte can be read whole.
struct HeaderSrc {
  uint32_t nh;
  const uint32_t* leaf_off;
  const uint32_t* byte_off;
  const uint32_t* words;
};
// What the rules compare with, all on the device and each array nullable (no rule): expect, nh x 8
// words; vals_idx / next_idx, per header the index into set_roots (8 words each, as
// launch_valhash_roots wrote them) or HEADER_NONE; link, per header the index of another header
// of the set or HEADER_NONE.
struct HeaderBind {
  const uint32_t* expect;
  const uint32_t* vals_idx;
  const uint32_t* next_idx;
  const uint32_t* link;
  const uint32_t* set_roots;
  uint32_t vals_leaf, vals_pos, next_leaf, next_pos, link_leaf, link_pos;
};
// roots (nh x 32 bytes, 16-byte aligned) = the Merkle root of every header; max_leaves: no header
// holds more (the caller checked it against HEADER_MAX_LEAVES). It sizes the lane group of a header.
void launch_header_roots(hipStream_t st, const HeaderSrc& src, uint32_t max_leaves, uint8_t* roots);
// bad[h] = the EDC_HEADER_BAD_* bits of header h under the rules, with roots as written above;
// *n_bad (zeroed by the caller) += the number of non-zero bytes
void launch_header_bind(hipStream_t st, const HeaderSrc& src, const HeaderBind& rules, const uint8_t* roots, uint8_t* bad,
                        uint32_t* n_bad);
// edc_msm.hip: per-device kernel attributes (the scatter's dynamic LDS beyond 64 KB); call on
// every device a context uses, after hipSetDevice
hipError_t msm_init_device();
// The MSM workspace of one slot: every buffer the binning, sort, accumulation and tail kernels pass
// between them. Grown by its owner before a batch is enqueued (edc_api.hip ensure_msm); the
// launchers below take it whole, so a buffer added here reaches every call site.
struct MsmWs {
  uint32_t cap_bins = 0, cap_ranges = 0;   // bins of the per-bin arrays, ranges of win
  size_t cap_entries = 0;                  // digits of entries / sorted
  devbuf::DevBuf<uint32_t> counts, offsets, cursor;
  devbuf::DevBuf<uint2> entries;
  devbuf::DevBuf<uint32_t> sorted;         // entries' point indices sorted by bucket within each bin
  devbuf::DevBuf<uint32_t> slice_W, slice_T, win;
  devbuf::DevBuf<uint32_t> buckets;        // bins x 256 bucket sums (extended)
  devbuf::DevBuf<uint32_t> heads;          // bins x 256 head partials of the segmented accumulation
  devbuf::DevBuf<uint32_t> bucket_end;     // bins x 256 bucket end positions of the sorted entries
};
// edc_msm.hip (counts_zeroed: the caller already cleared ws.counts, e.g. launch_init_batch)
void launch_msm_bin(hipStream_t st, const MsmPlan& P, const MsmTerms& T, uint32_t max_terms, MsmWs& ws, const int* flags,
                    bool counts_zeroed = false);
// per-bin counting sort of the binned entries by bucket (needs only the binning: enqueued right
// after launch_msm_bin, so on a dual-stream slot it overlaps the decode)
void launch_msm_sort(hipStream_t st, const MsmPlan& P, MsmWs& ws);
// accumulation (+ bin reduction) of the sorted entries; launch_msm_sort must have run
void launch_msm_bucket(hipStream_t st, const MsmPlan& P, MsmWs& ws, const uint32_t* pts, int probe_skip = 0,
                       hipEvent_t acc_begin = nullptr, hipEvent_t acc_end = nullptr, bool latency = false,
                       int* stamp_flags = nullptr);   // EDC_BATCH_STAMPS builds: the batch's flags
size_t msm_bucket_words(uint32_t nbin);
void launch_msm_tail(hipStream_t st, const MsmPlan& P, MsmWs& ws, int* flags, int want_compress, uint8_t* out,
                     uint8_t* hout = nullptr, const uint32_t* extra = nullptr);   // extra: an extended point added before the x8
// eager verifier: run (EXT_WORDS words) += the partial point of result block blk; blk = null: run = identity
void launch_point_accum(hipStream_t st, uint32_t* run, const uint8_t* blk);
void launch_msm_range_tail(hipStream_t st, const MsmPlan& P, MsmWs& ws, uint8_t* rverdict);
// several batches in one launch: per range the window combine, Horner, x8 and identity, one
// 256-byte result block per range at out + 256 g (and hout + 256 g)
void launch_msm_multi_tail(hipStream_t st, const MsmPlan& P, MsmWs& ws, const int* flags, const uint8_t* rbad,
                           int want_compress, uint8_t* out, uint8_t* hout);
void launch_combine_records(hipStream_t st, uint32_t g, const uint8_t* recs, uint32_t stride, uint8_t* out);
void launch_combine(hipStream_t st, uint32_t g, const uint8_t* partials, int bad, int want_compress,
                    uint8_t* out);
// 256-byte result block src -> dst (dst may be a peer device's memory)
void launch_copy_block(hipStream_t st, const uint8_t* src, uint8_t* dst);
// g shard result blocks (256 bytes each, device) -> verdict block (as launch_combine)
void launch_combine_blocks(hipStream_t st, uint32_t g, const uint8_t* blocks, int want_compress, uint8_t* out);
size_t msm_entry_capacity(const MsmPlan& P, size_t short_terms, size_t full_terms);
// edc_single.hip
void launch_init_btable(hipStream_t st, uint32_t* btab);
void launch_verify_single(hipStream_t st, uint32_t n, const uint8_t* vk, const uint8_t* sig,
                          const uint32_t* k, const uint32_t* btab, uint32_t* vtab, uint8_t* verdict,
                          const KeyCacheView& kc, const uint32_t* bcomb);
// latency form for short item lists (one quad of lanes per item)
void launch_verify_quad(hipStream_t st, uint32_t n, const uint8_t* vk, const uint8_t* sig, const uint32_t* k,
                        const uint32_t* btab, uint8_t* verdict, const KeyCacheView& kc, const uint32_t* bcomb);
// key cache (edc_single.hip): decode m registered keys -> ext + ok, comb tables of m points
void launch_kc_decode(hipStream_t st, uint32_t m, const uint32_t* keys, uint32_t* ext, uint8_t* ok);
void launch_kc_basepoint(hipStream_t st, uint32_t* ext);
void launch_kc_comb(hipStream_t st, uint32_t m, const uint32_t* ext, uint32_t* comb);
// VerificationKey::try_from for n encodings: code[i] = 0 (Ok) or 2 (MalformedPublicKey)
void launch_vk_validate(hipStream_t st, uint32_t n, const uint8_t* enc, uint8_t* code);
size_t verify_single_scratch_words(size_t n);
void launch_sign(hipStream_t st, uint32_t n, const uint8_t* seeds, const uint32_t* seed_index,
                 const uint8_t* msg, const uint64_t* off, const uint32_t* btab, uint8_t* vk_out,
                 uint8_t* sig_out);
void launch_decode(hipStream_t st, uint32_t n, const uint8_t* enc, uint8_t* xy, uint8_t* ok);
void launch_chacha_fill(hipStream_t st, const uint32_t key[8], uint64_t blk0, uint64_t nblocks,
                        uint32_t* out);
}  // namespace edc
