// Verified-signature cache (include/edc.h, edc_sigcache_*): a device-resident table of the items
// (vk || sig || k, 128 bytes) that already verified on this context.
//
// A consensus node verifies the same vote several times (gossip, the block's commit, the next
// block's last-commit, block sync). Under ZIP215 the verdict is a pure function of (vk, sig, k),
// so a byte-identical item that verified once verifies again: a cached call looks every item up,
// and only the misses, in queue order, form the batch that is decoded, hashed into the MSM and
// verified. k = H(R || A || M) binds the message, so another message is another record.
//
// Layout. Open addressing over `cap` (a power of two) slots, structure of arrays:
//   hdr[slot]  64 bits: fingerprint << 32 | generation the record was inserted in; 0 = never used
//   rec[slot]  8 x uint4: vk (32) || sig (64) || k (32)
// An item hashes (SipHash-1-3 under a per-context 128-bit key, so chosen items cannot pile into
// one window) to 64 bits: the low bits pick its home slot, the high 32 its fingerprint. Probing is
// circular inside the aligned window of SC_WINDOW slots that holds the home slot. An insert takes
// the first slot of its probe order that is never used or dead, so no never-used slot lies between
// a record's home and its place, and a lookup stops at the first never-used header. A hit is a
// live header with the item's fingerprint AND 128 equal bytes: a false hit would accept a
// forgery, a false miss only costs time.
//
// Ageing. The table has a generation (>= 1), bumped by edc_sigcache_advance (once per height). A
// record inserted more than `keep` generations ago is dead: lookups skip it, inserts reuse it.
//
// Concurrency. Lookup and insert never run together: kernel boundaries on one stream for the
// one-call entries; a cached verifier's deferred insert runs on its own stream and records the
// context's event, which every other table access waits for first (edc_api.hip, sc_ev). Inside one
// insert launch a slot is claimed by a 64-bit CAS on its header and only the claimer writes the
// record. A lane that meets a header claimed in the same launch may read a half-written record,
// find it unequal and claim another slot: a duplicate copy, which is harmless. An insert that
// finds no free or dead slot in its window is dropped and counted; it never evicts a live record.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edc {

constexpr uint32_t SC_WINDOW = 32;      // probe window (slots); the smallest table
constexpr uint32_t SC_BLOCK = 256;      // lanes per workgroup of the per-item kernels
constexpr uint32_t SC_SCAN_TILE = 1024; // workgroup counts one pass of the scan covers

struct SigCacheView {
  unsigned long long* hdr;
  uint4* rec;
  uint32_t mask;        // cap - 1
  uint32_t gen, keep;
  uint64_t k0, k1;      // hash key, from the context's secret
};

// hit[i] = 1 iff item i is a live record. wg_miss (nullable): misses of each workgroup of SC_BLOCK items.
void launch_sc_lookup(hipStream_t st, const SigCacheView& sc, uint32_t n, const uint8_t* vk, const uint8_t* sig,
                      const uint32_t* k, uint8_t* hit, uint32_t* wg_miss);
// cached quorum commit sets: the lookup of the items with skip[i] == 0 only (skip null: all n); no
// other item's bytes are read and no table access is made for it. leave[i] = 1 iff item i is not
// checked or is a live record (launch_sc_compact's `hit`), code[i] = 255 iff it is not checked,
// else 0; wg_miss / wg_hit: the checked misses / hits of each workgroup of SC_BLOCK items
void launch_sc_lookup_masked(hipStream_t st, const SigCacheView& sc, uint32_t n, const uint8_t* skip, const uint8_t* vk,
                             const uint8_t* sig, const uint32_t* k, uint8_t* leave, uint8_t* code, uint32_t* wg_miss,
                             uint32_t* wg_hit);
// exclusive scan of the nwg workgroup counts in place; total[0] = their sum
void launch_sc_scan(hipStream_t st, uint32_t nwg, uint32_t* wg_miss, uint32_t* total);
// order-preserving compaction of the misses: idx[j] = queue index of miss j, its vk / sig / k
// gathered to row j of the staging arrays (wg_off: the scanned counts)
void launch_sc_compact(hipStream_t st, uint32_t n, const uint8_t* hit, const uint32_t* wg_off, const uint8_t* vk,
                       const uint8_t* sig, const uint32_t* k, uint32_t* idx, uint8_t* out_vk, uint8_t* out_sig,
                       uint32_t* out_k);
// insert items idx[j] (idx null: j), j < c, whose verdict[j] is 0 (verdict null: all of them);
// ctr[0] += records written, ctr[1] += inserts dropped
void launch_sc_insert(hipStream_t st, const SigCacheView& sc, uint32_t c, const uint32_t* idx, const uint8_t* vk,
                      const uint8_t* sig, const uint32_t* k, const uint8_t* verdict, unsigned long long* ctr);
// out[idx[j]] = v[j], j < c (per-item verdicts of the misses back to their queue positions)
void launch_sc_scatter(hipStream_t st, uint32_t c, const uint32_t* idx, const uint8_t* v, uint8_t* out);
// cached incremental verifier (edc_vfy_set_cached): the misses of one queued range of n items, in
// offered order, appended to the retained arrays from row dst0 on (hit / wg_off: this range's
// lookup flags and scanned workgroup counts); origin[dst0 + j] = base + range index of miss j,
// its position among everything offered since the last reset
void launch_sc_gather_range(hipStream_t st, uint32_t n, const uint8_t* hit, const uint32_t* wg_off, const uint8_t* vk,
                            const uint8_t* sig, const uint32_t* k, uint32_t base, size_t dst0, uint8_t* out_vk,
                            uint8_t* out_sig, uint32_t* out_k, uint32_t* origin);

}  // namespace edc
