// C ABI (include/edc.h): context, workspace and the orchestration of the batch pipeline.
// Every entry point cites the reference API it replaces in include/edc.h.
#include <stdlib.h>
#include <string.h>
#include <string>
#include <random>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>
#include <errno.h>
#include <sys/random.h>
#include <hip/hip_ext.h>
#include "edc.h"
#include "edc_common.h"
#include "edc_launch.h"
#include "vfy_fold.h"
#include "vfy_cached.h"
#include "tmpl.h"
#include "commits.h"
#include "quorum.h"
#include "valset.h"
#include "vhist.h"
#include "valhash.h"
#include "hdrhash.h"
#include "sigcache.h"
#include "devbuf.h"

using namespace edc;
using namespace devbuf;

namespace {

// phases in enqueue order (each bracketed by HIP events on the slot stream)
enum Phase { PH_KEYS, PH_CHALLENGE, PH_COEF, PH_MSM_BIN, PH_DECOMP, PH_MSM_BUCKET, PH_MSM_TAIL, PH_N };
const char* kPhaseNames[PH_N] = {"keys_group", "challenge_sha512", "coef_chacha_scalar", "msm_bin",
                                 "decompress_R", "msm_bucket", "msm_window_final"};

#ifndef EDC_SLOTS
#define EDC_SLOTS 16
#endif
constexpr int kSlots = EDC_SLOTS;  // batches that can be in flight per context
// Timing probes only (make variant VFLAGS=-DEDC_PROBE_SKIP=<mask>, tools/phase_cost.sh): after a
// slot's first batch, skip a phase's launches (its outputs stay from that batch, which the bench
// repeats), to measure what the phase costs inside the pipeline: 2 SHA-512, 4 coefficients,
// 8 binning, 16 decompression, 32 accumulation, 64 bin reduction, 128 window combine + Horner,
// 256 bucket sort. The product build has mask 0.
#ifndef EDC_PROBE_SKIP
#define EDC_PROBE_SKIP 0
#endif
#define EDC_RUN(bit) ((EDC_PROBE_SKIP & (bit)) == 0 || s.probe_runs == 0)
#ifndef EDC_DUAL_STREAM
#define EDC_DUAL_STREAM 2   // slot 0 (synchronous calls) decodes on a second stream; see init_slot
#endif
#ifndef EDC_QUAD_VERIFY_MAX
#define EDC_QUAD_VERIFY_MAX (1u << 14)   // one lane per item beats a quad from ~32k items (r04ad)
#endif
constexpr size_t kQuadVerifyMax = EDC_QUAD_VERIFY_MAX;   // per-item lists up to this size use the quad kernel
constexpr uint32_t kMultiMax = 16;            // batches per edc_batch_submit_multi_device launch
constexpr uint32_t kMultiKeys = 4096;         // distinct keys with per-(batch, key) sums; more -> per signature

}  // namespace

// Templated messages (edc_tmpl_*): what a slot or a verifier needs to turn one call's template set
// and items into a message arena on the device. Grow-only; nothing of a call survives it.
struct TmplWs {
  DevBuf<uint8_t> set;          // the call's template set: head_off | tail_off | head | tail
  DevBuf<uint64_t> bsum;        // the scan's workgroup sums
  DevBuf<uint8_t> in;           // host forms: var_off | tpl | var staged for the expansion
  DevBuf<uint8_t> arena;        // the expanded messages and their offsets (a verifier uses its own)
  DevBuf<uint64_t> off;
  DevBuf<int> flag;             // raised by k_tmpl_len on a malformed item (device forms)
  PinnedBuf<int> h_flag;        // pinned mirror, read at the wait when `check` is set
  bool check = false;
};

// One in-flight batch: its own HIP stream and every per-batch device buffer.
struct Slot {
  // streams and events are declared first: members are destroyed in reverse order, so every buffer
  // of the slot is freed before the streams and events it was used on
  Stream st;
  // EDC_DUAL_STREAM builds: the decode runs on a second stream beside SHA-512 / coefficients /
  // binning (joined before the accumulation)
  Stream st2;
  Event ev_keys, ev_dec;
  Event ev[PH_N + 1];
  Event ev_acc[2];              // timed batches: around k_msm_accum_dma (edc_last_msm_accum)
  size_t cap_n = 0, cap_T = 0;
  DevBuf<uint32_t> k, key_slot, key_index, key_rep;
  // the batch's challenges: k (computed by k_challenge) or a prehashed caller's device array
  // (borrowed)
  const uint32_t* kin = nullptr;
  DevBuf<uint32_t> table, slot_key;
  DevBuf<uint32_t> pts, scal;
  DevBuf<unsigned long long> key_acc, u_acc;
  DevBuf<uint32_t> coef_part;        // k_coef's per-workgroup key slots (merged by k_coef_merge)
  DevBuf<uint8_t> itembad, keybad;   // per-item / per-key failure bits (fallback)
  MsmWs msm;                    // MSM workspace (edc_launch.h), grown on demand by ensure_msm
  DevBuf<int> flags;
  DevBuf<uint8_t> d_out;        // 256-byte result block (kMultiMax of them for a multi-batch launch)
  PinnedBuf<uint8_t> h_out;     // pinned mirror
  PinnedBuf<uint32_t> h_acc;    // pinned: the last bin's offset and count (timed batches' entry count)
  // several batches in one launch (edc_batch_submit_multi_device): per-(batch, key) sums, listed
  // key / B terms, per-batch bad flags; nmulti = batches of the pending launch (0: one batch)
  DevBuf<unsigned long long> mb_acc;
  DevBuf<uint32_t> mb_xpt, mb_xrg, mb_xscal;
  DevBuf<uint8_t> mb_bad;
  uint32_t nmulti = 0;
  uint32_t acc_nbin = 0;        // bins of the last enqueued single-batch MSM (timing report)
  // union-first multi launch (edc_set_multi_union): the launch ran as ONE batch over all nb * n_per
  // items; its arguments are kept (device inputs are borrowed until the wait) to rerun it batch by
  // batch when that union fails
  bool mu_union = false;
  size_t mu_nper = 0;
  const uint8_t *mu_vk = nullptr, *mu_sig = nullptr, *mu_msg = nullptr;
  const uint64_t* mu_off = nullptr;
  const uint32_t* mu_k = nullptr;
  uint8_t mu_seed[32] = {};
  uint64_t mu_zbase = 0;
  int mu_compress = 0;
  // commit set (edc_commits_*): the launch ran as ONE batch over all the commits' items; its
  // boundaries (host, borrowed until the wait) and the device inputs it read are kept, so that the
  // wait can run the grouped fallback on this slot when that union fails
  bool commits = false;
  size_t cm_nc = 0;
  const uint32_t* cm_off = nullptr;
  const uint8_t *cm_vk = nullptr, *cm_sig = nullptr, *cm_msg = nullptr;
  const uint64_t* cm_moff = nullptr;
  uint8_t cm_seed[32] = {};
  // host-buffer submissions (edc_batch_submit): this slot's own device copy of the inputs
  DevBuf<uint8_t> in_vk, in_sig, in_msg;
  DevBuf<uint64_t> in_off;
  DevBuf<uint32_t> in_idx;            // key indices (edc_batch_submit_indexed)
  size_t in_cap_n = 0;
  std::vector<uint64_t> in_rebased;   // offsets rebased to 0 (host side, alive until the slot is reused)
  bool pending = false;         // submitted, not yet waited
  bool timed = false;
  bool per_sig = false;         // this batch skipped key grouping (adaptive grouping)
  uint32_t n_batch = 0;
  int64_t ticket = -1;
  uint32_t probe_runs = 0;      // batches enqueued (EDC_PROBE_SKIP timing builds only)
  TmplWs tw;                    // templated submissions (edc_tmpl_*)
  uint64_t t_submit_us = 0;     // host time of the submission (EDC_BATCH_STAMPS builds only)
};

// Quorum workspace ("Quorum workspace"). What ONE side of a quorum call owns on the
// device and in pinned memory. Every call has side A; a trusting pair (trust_ver of a request) has
// side B too, the same arrays again. Three tiers of allocation: votes (every quorum call), join (the
// validator-set forms), and what only a history (ver) or a pair (skip; all of side B) needs.
struct QuorumSide {
  // votes tier (side_votes_room): the power and flag the selection reads, staged by a host form or
  // written by the join (cap_n votes); the staged thresholds, the selection's plan, the tally
  // kernel's sums and its correction words (cap_c commits)
  size_t cap_n = 0, cap_c = 0;
  DevBuf<uint64_t> power, thr, planned, tally;
  DevBuf<uint8_t> flag;
  DevBuf<uint32_t> cor;
  // join tier (side_join_room): the members' cache indices and the pair set of the double-vote scan,
  // 2 words per vote (join_n votes); the commits' double-vote bytes and the pinned bytes they come
  // back in (join_c commits)
  size_t join_n = 0, join_c = 0;
  DevBuf<uint32_t> who;
  DevBuf<uint64_t> set;
  DevBuf<uint8_t> dv;
  PinnedBuf<uint8_t> hdv;
  DevBuf<uint32_t> ver;         // the commits' versions: a history form's, side B's trust versions
  DevBuf<uint8_t> skip;         // this side's own skip bytes in a pair (side_skip); alone, side A writes sc_hit
};

// The per-call state of the quorum family (quorum.h, valset.h, vhist.h; edc_quorum_*, edc_tmpl_quorum_*,
// edc_cached_*, edc_valset_*, edc_vhist_*, edc_vq_*), all on slot 0's stream. The gathers use the
// sc_* staging.
struct QuorumWs {
  QuorumSide side[2];
  QuorumSide &a = side[0], &b = side[1];
  // both sides read these. With side A's votes tier: the staged offsets (cap_c + 1), the votes'
  // commit indices and the scan's tile words (cap_n votes); the error flag; the pinned words the
  // flag, the checked count, the checked hole bytes (templated forms) and the checked misses and
  // hits (cached forms) come back in
  size_t cap_n = 0, cap_c = 0;
  DevBuf<uint32_t> coff, cidx, aggf;
  DevBuf<uint64_t> aggv, carry;
  DevBuf<int> err;
  PinnedBuf<uint32_t> h;
  // with side A's join tier: the staged key positions and flags of the host forms (join_n votes)
  size_t join_n = 0;
  DevBuf<uint32_t> kidx;
  DevBuf<uint8_t> vflag;
  // pair tier: the union's side byte per vote, its device totals {A, B, both} and the pinned words
  // they come back in
  DevBuf<uint8_t> sideb;
  DevBuf<uint32_t> cnt;
  PinnedBuf<uint32_t> hcnt;
  // templated forms (edc_tmpl_quorum_*): the all-n template array and the staged commit_tpl, the
  // tiles' hole bytes (+ their total, which comes back in h[2]), the gathered template indices /
  // hole offsets / holes of the checked votes, the host form's staged var_off | item_alt | var, the
  // pinned word the arena's size comes back in
  DevBuf<uint16_t> tq_tpl, tq_ctpl, tq_gtpl;
  DevBuf<uint32_t> tq_wgh, tq_gvoff;
  DevBuf<uint8_t> tq_gvar, tq_in;
  PinnedBuf<uint64_t> tq_harena;
  // cached forms (edc_cached_*): the masked lookup's leave-out bytes and base codes, its workgroup
  // counts (misses + total, then hits + total), and for the templated forms, whose first staging
  // area holds the gathered checked list, the second one (miss positions in that list, the misses'
  // vk | sig | k)
  size_t cq_cap_n = 0, cq_cap_g = 0;
  DevBuf<uint8_t> cq_leave, cq_code, cq_g;
  DevBuf<uint32_t> cq_wg, cq_idx;
  // the host copies edc_debug_tmpl_quorum_last, edc_debug_cached_quorum_last, edc_debug_vq_last and
  // edc_debug_vq_trust_last return
  uint64_t tq_last[4] = {}, cq_last[6] = {}, vq_last[8] = {}, vqt_last[4] = {};
  bool tq_have = false, cq_have = false, vq_have = false, vqt_have = false;
};

struct edc_ctx {
  int device = 0;
  std::string err;
  // streams and events are declared first (the slots' own likewise): members are destroyed in
  // reverse order, so every buffer of the context is freed before them.
  // Chunked synchronous host-buffer calls (run_host_chunked): two copy streams and one event per
  // chunk (+ the keys / offsets piece) each, created together on first use
  Stream hcs, hcs2;
  Event hev[9], hev2[9];        // piece 0 + signature chunks / k or message chunks
  // recorded after every deferred insert of a cached verifier (which returns without waiting for
  // it): every other access to the table first orders itself after it, so that lookup and insert
  // never run together across streams either. sc_ev_set: it has been recorded at least once
  Event sc_ev;
  bool sc_ev_set = false;
  DevBuf<uint32_t> btab;        // [1..8]B, affine Niels
  Slot slot[kSlots];
  // staging for the host-pointer entry points (used on slot 0's stream)
  size_t cap_n = 0;
  DevBuf<uint8_t> vk, sig, msg, zexp;
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> kbuf;
  DevBuf<uint8_t> verdicts;
  DevBuf<uint32_t> vtab;        // per-item multiples tables of the per-signature kernel
  DevBuf<uint8_t> aux;          // decode xy / sign outputs / partials
  // shard-partial combination on its own stream, so it never waits behind in-flight batches
  Slot comb;
  DevBuf<uint8_t> comb_in;      // g x 128-byte partial records
  bool timing = false;
  float last_ms[PH_N] = {};
  float last_acc_ms = 0.f;      // k_msm_accum_dma of the last timed batch
  uint32_t last_acc_entries = 0;
  int nlast = 0;
  int64_t next_ticket = 0;
  int nslots = kSlots;          // in-flight slots the submissions rotate over (edc_set_slots)
  // adaptive key grouping (edc_set_key_grouping): mode 0 = auto, 1 = always group, 2 = never
  int key_grouping = 0;
  bool have_key_ratio = false;  // a grouped batch has completed on this context
  double last_key_ratio = 0.0;  // distinct keys / signatures of the last grouped batch
  int ungrouped_run = 0;        // consecutive ungrouped batches since the last grouped one
  int win_bits = 0;             // MSM window width override (edc_set_msm_shape), 0 = by batch size
  uint32_t bin_entries = 0;     // target entries per MSM bin (edc_set_msm_bin_entries), 0 = by batch size
  uint32_t msm_parts = 0;       // MSM parts override (edc_set_msm_shape), 0 = by batch size
  edc_plan_info last_plan = {}; // host copy of the last batch_plan / fold_plan (edc_debug_last_plan)
  bool have_plan = false;
  uint64_t secret = 0;          // key-grouping hash secret (OS randomness, per context)
  uint64_t nbatches = 0;
  // grouped fallback (range MSM) staging, slot 0 only
  size_t fb_cap_terms = 0;
  DevBuf<uint32_t> fb_xpt, fb_xrg, fb_xscal;
  DevBuf<uint8_t> fb_rv;         // per-range verdict | pre-bad flag (2 x ranges + 64 bytes)
  DevBuf<uint32_t> fb_idx;       // items verified one by one
  DevBuf<uint8_t> fb_g;          // their gathered vk | sig | k (fb_cap_g items each)
  size_t fb_cap_g = 0;           // items fb_idx and fb_g are sized for
  uint32_t fb_ranges = 128;     // target range count of the grouped fallback (sweep: profiles/r04/r04ad_fb_sweep.log)
  int fb_bits = 9;              // its window width
  // persistent validator-key cache (keycache.h), replaced by each edc_keycache_load, grown by
  // edc_keycache_add (device arrays hold kc_cap keys; the host keeps the key words and ok bytes
  // to rebuild the hash table and answer duplicates)
  DevBuf<uint32_t> kc_table, kc_keys, kc_comb;
  DevBuf<uint8_t> kc_ok;
  DevBuf<uint32_t> bcomb;       // comb table of B, built with the first cache
  uint32_t kc_m = 0, kc_tmask = 0, kc_cap = 0;
  uint32_t kc_s0 = 0, kc_s1 = 0;        // table hash key, from `secret`
  std::vector<uint32_t> kc_words;       // kc_m x 8 raw key words
  std::vector<uint8_t> kc_okh;          // kc_m decode flags
  DevBuf<uint32_t> kc_reg;      // registered position -> cache index (edc_batch_submit_indexed)
  uint32_t kc_reg_m = 0;
  // split coefficients (edc_common.h) while the key cache covers the batches' keys:
  // key_split 0 = auto, 1 = never; last_uncached = keys the last batch did not find in the cache
  int key_split = 0;
  uint32_t last_uncached = 0;
  // bumped whenever the cache's contents change (load / add / clear): a verifier's queued
  // [2^128] rows are only used by a verify that finds the generation they were built against
  uint64_t kc_gen = 0;
  int multi_union = 1;                  // edc_set_multi_union
  // verified-signature cache (sigcache.h; edc_sigcache_*): the table, its generation, the
  // per-call staging (hit flags, workgroup counts, miss index list, gathered misses, verdicts)
  // and the counters. The one-call entries use it on slot 0's stream; cached verifiers
  // (edc_vfy_set_cached) look up and insert on their own streams, see sc_ev
  DevBuf<unsigned long long> sc_hdr;
  DevBuf<uint4> sc_rec;
  size_t sc_cap = 0;                    // records (a power of two); 0 = no table
  uint32_t sc_gen = 1, sc_keep = 2;
  uint64_t sc_k0 = 0, sc_k1 = 0;        // table hash key, from `secret`
  uint64_t sc_hits = 0, sc_misses = 0;
  DevBuf<unsigned long long> sc_ctr;    // device: records written, inserts dropped
  PinnedBuf<unsigned long long> sc_hctr;   // pinned mirror (+ word 2: the miss count of the last lookup)
  size_t sc_cap_n = 0;
  DevBuf<uint8_t> sc_hit, sc_g, sc_verd, sc_mverd;
  DevBuf<uint32_t> sc_wg, sc_idx;
  // the returned view borrows the table
  SigCacheView sc() const {
    return SigCacheView{sc_hdr, sc_rec, (uint32_t)(sc_cap - 1), sc_gen, sc_keep, sc_k0, sc_k1};
  }
  QuorumWs qw;                  // quorum commit sets and everything built on them, per call (above)
  // validator-set quorum commit sets (valset.h; edc_valset_*). The powers of the registered list
  // (edc_valset_set_powers), by cache index: power, member byte and position on the device for the
  // vs_count keys the cache held then, the positions on the host too (vs_posh) beside the host copy
  // of kc_reg; vs_m members. The per-call workspace is QuorumWs's join tier.
  std::vector<uint32_t> kc_regh, vs_posh;
  DevBuf<uint64_t> vs_power;
  DevBuf<uint8_t> vs_member;
  DevBuf<uint32_t> vs_pos;
  uint32_t vs_count = 0, vs_m = 0;
  ValsetView vs() const { return ValsetView{vs_power, vs_member, vs_pos, vs_count}; }
  // validator-set history (vhist.h; edc_vhist_*), independent of the powers above: the change
  // lists by cache index on the device (vh_count keys the cache held at edc_vhist_set), the
  // history by position (totals, the reference lists) and each cache index's position on the host;
  // vh.m = 0: none. The commits' versions of a call are a QuorumSide's.
  VHist vh;
  std::vector<uint32_t> vh_posh;
  DevBuf<uint32_t> vh_off, vh_ver;
  DevBuf<uint64_t> vh_pow;
  uint32_t vh_count = 0;
  VhistView vhv() const { return VhistView{vh_off, vh_ver, vh_pow, vh_count}; }
  // validator-set hashes (valhash.h; edc_valhash_valset, edc_valhash_vhist, edc_valhash_vhist_match): the
  // address order of the registered list, ranked on the first call after a list is loaded (rank by
  // position, by_rank the cache index of each rank; vx_ranked) and dropped with the history. Per
  // call, on slot 0's stream: the roots, the staged versions | root indices | expected hashes, and
  // the match bytes. No root is kept between calls.
  DevBuf<uint32_t> vx_rank, vx_by_rank, vx_in;
  bool vx_ranked = false;
  DevBuf<uint8_t> vx_roots, vx_ok;
  // header hashes (hdrhash.h; edc_header_hashes, edc_header_bind): per call, on slot 0's stream, the
  // staged set (leaf offsets, byte offsets, the bytes as whole words), the staged rules (expect;
  // vals index | next index | link | the distinct versions), what comes back in one piece
  // (roots | count, 16 bytes | bad) and its pinned host copy. The set roots of the named versions
  // go through vx_roots. Nothing is kept between calls.
  DevBuf<uint32_t> hd_leaf, hd_byte, hd_words, hd_expect, hd_meta;
  DevBuf<uint8_t> hd_out;
  PinnedBuf<uint8_t> hd_host;
  uint64_t mu_hits = 0, mu_reruns = 0;  // union-first launches that passed / were rerun per batch
  // incremental verifiers bound to this context (edc_verifier_create): their streams are drained
  // with the slots' whenever the key cache they read is rebuilt
  std::vector<struct edc_verifier*> verifiers;
  hipStream_t st() const { return slot[0].st; }
  // the returned view borrows the cache
  KeyCacheView kc() const {
    if (!kc_m) return KeyCacheView{nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0};
    return KeyCacheView{kc_table, kc_keys, kc_ok, kc_comb, kc_tmask, kc_m, bcomb, kc_s0, kc_s1};
  }
};

// Incremental batch verifier (include/edc.h, edc_verifier_*): the reference's Verifier as an
// object (src/batch.rs:110-217). Its own workspace slot and streams, the retained bytes of the
// queued items (vk, sig, k) and the z-independent per-item results (R rows of s.pts, key grouping,
// decoded keys in the key area, failure bits, flags) persist from queue to queue.
struct edc_verifier {
  edc_ctx* ctx = nullptr;
  // streams and events are declared first (the slot's own likewise): members are destroyed in
  // reverse order, so every buffer of the verifier is freed before them
  Stream cs;                    // copy stream: an append's copies overlap the previous append's kernels
  Event ev_copy, ev_chal;
  Event ev_cnt, ev_gather;      // cached mode, see below
  Slot s;                       // never the context's slot 0: other calls keep working between queues
  size_t n = 0, cap = 0;        // queued items / items the retained arrays and the key table are sized for
  DevBuf<uint8_t> vk, sig, zexp;
  DevBuf<uint32_t> k;
  DevBuf<uint8_t> msg;          // one append's message arena and offsets (dead once its k exists)
  DevBuf<uint64_t> off;
  bool chal_pending = false;    // ev_chal guards msg / off against the next append's copies
  uint32_t T = 0;               // key table slots in use (a power of two, <= s.cap_T)
  uint32_t salt[2] = {0, 0};    // fixed until reset
  std::vector<uint64_t> rebased;
  // key areas (their own allocation, 2 s.cap_n records): rows [0, cap_n) the decoded keys in
  // key-index order, rows [cap_n, 2 cap_n) their [2^128] multiples (split coefficients)
  DevBuf<uint32_t> karea;
  size_t karea_cap = 0;         // the s.cap_n it was sized for
  // the [2^128] rows are usable while every range since the last reset was queued with a key
  // cache loaded and that cache's generation (edc_ctx::kc_gen) is still hi_gen
  uint64_t hi_gen = 0;
  bool hi_ok = false;
  int last_split = -1;          // plan of the last verify: 1 split, 0 unsplit, -1 none yet
  edc_plan_info last_plan = {}; // plan of the last verify or fold on this verifier (edc_vfy_last_plan)
  bool have_plan = false;
  DevBuf<uint32_t> idx;         // one indexed append's key positions (edc_vfy_queue_indexed)
  // eager mode (edc_vfy_begin_eager): the block's z seed is committed before the items arrive and
  // queue calls fold sum [z_i]R_i of the items [fold.folded, n) into the running point `run`
  // (EXT_WORDS words, then the 256-byte result block of the last fold's MSM); verify's MSM then
  // leaves those R terms out and adds `run` before the x8. Both survive a growth.
  FoldState fold;
  uint8_t eager_seed[32] = {};
  DevBuf<uint32_t> run;
  // cached mode (edc_vfy_set_cached): a queue call stages its range (st_*), looks it up in the
  // context's verified-signature table and appends only the misses; origin[i] = offered position
  // of retained item i. hit / wg: the range's lookup flags and workgroup miss counts (+ total);
  // h_cnt: pinned word the miss count comes back in; ev_cnt: after that copy; ev_gather: after the
  // range's gather, which is the last reader of the staging area; verd / offv: per-item codes of a
  // fallback on the device (retained order, offered order)
  CachedState cached;
  DevBuf<uint32_t> origin;
  DevBuf<uint8_t> st_vk, st_sig, hit;
  DevBuf<uint32_t> st_k, wg;
  size_t st_cap = 0;
  PinnedBuf<uint32_t> h_cnt;
  bool gather_pending = false;
  DevBuf<uint8_t> verd, offv;
};

// A failed HIP call also leaves the thread's last-error state set; it is cleared here, so that a
// later hipGetLastError() after a kernel launch reports only that launch.
#define CK(expr)                                                        \
  do {                                                                  \
    hipError_t e_ = (expr);                                             \
    if (e_ != hipSuccess) {                                             \
      (void)hipGetLastError();                                          \
      ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);     \
      return EDC_ERR_HIP;                                               \
    }                                                                   \
  } while (0)

// Every in-flight slot needs its own hardware queue: kernels of streams that share a queue run
// in order, so one batch's latency-bound tail would stall the bulk kernels of another; hence the
// slot streams are created with an all-CU mask (Stream::create_all_cus).
static int init_slot(edc_ctx* ctx, Slot& s) {
  if (s.st) return 0;
  CK(s.st.create_all_cus(ctx->device));
  CK(s.flags.alloc(FLAG_ALLOC));
  CK(s.d_out.alloc(256 * kMultiMax));
  CK(s.h_out.alloc(256 * kMultiMax));
  CK(s.h_acc.alloc(2));
  for (Event& e : s.ev) CK(e.create());
  for (Event& e : s.ev_acc) CK(e.create());
#if EDC_DUAL_STREAM
  // 1: every slot; 2: slot 0 only (the synchronous calls' slot), so the pipelined slots keep one
  // hardware queue each (past ~16 user queues per GPU the scheduler time-slices them).
  // EDC_SINGLE_STREAM=1 in the environment (measurement only: kernel traces of one batch at a time
  // that must not overlap the decode with SHA-512) keeps every slot on one stream.
  static const bool single_stream = getenv("EDC_SINGLE_STREAM") && getenv("EDC_SINGLE_STREAM")[0] == '1';
  if (!single_stream && (EDC_DUAL_STREAM == 1 || &s == &ctx->slot[0])) {
    CK(s.st2.create_all_cus(ctx->device));
    CK(s.ev_keys.create(hipEventDisableTiming));
    CK(s.ev_dec.create(hipEventDisableTiming));
  }
#endif
  return 0;
}

// The slot claims. A synchronous call runs on slot 0 and a submission on the slot of the next
// ticket; each refuses a slot whose batch has not been waited for (null, ctx->err says why). The
// ticket is taken only once the enqueue has succeeded, so a refused or failed submission leaves
// next_ticket where it was.
static const char kAllSlotsInFlight[] = "all slots in flight: wait for the oldest ticket first";

static Slot* claim_slot0(edc_ctx* ctx) {
  if (ctx->slot[0].pending) { ctx->err = "slot 0 busy: wait for submitted batches first"; return nullptr; }
  return &ctx->slot[0];
}

static Slot* claim_next_slot(edc_ctx* ctx) {
  Slot& s = ctx->slot[ctx->next_ticket % ctx->nslots];
  if (s.pending) { ctx->err = kAllSlotsInFlight; return nullptr; }
  return &s;
}

static int64_t take_ticket(edc_ctx* ctx, Slot& s) {
  s.ticket = ctx->next_ticket;
  return ctx->next_ticket++;
}

// key indices of a host form: every one a position in the registered key list (kc_reg)
static int check_key_idx(edc_ctx* ctx, size_t n, const uint32_t* key_idx) {
  uint32_t mx = 0;
  for (size_t i = 0; i < n; ++i) mx = key_idx[i] > mx ? key_idx[i] : mx;
  if (n && mx >= ctx->kc_reg_m) { ctx->err = "key index outside the registered key list"; return EDC_ERR_ARG; }
  return 0;
}

static int ensure_slot(edc_ctx* ctx, Slot& s, size_t n) {
  int rc = init_slot(ctx, s);
  if (rc) return rc;
  CK(grow_group(s.cap_n, n, item_cap, sync_of(s.st), [&](size_t cap) {
    const size_t T = next_pow2(2 * cap);
    s.cap_T = 0;
    s.msm = MsmWs();   // the MSM workspace goes with the slot's arrays
    hipError_t e = alloc_all(
        sized(s.k, cap * 8), sized(s.key_slot, cap), sized(s.key_index, cap), sized(s.key_rep, cap), sized(s.table, T),
        sized(s.slot_key, T),
        // >= msm_num_points_split(n, m) for any m <= n (split coefficients add m + 1 points)
        sized(s.pts, (3 + 3 * cap) * NIELS_WORDS), sized(s.scal, (3 + 3 * cap) * 8), sized(s.key_acc, cap * KEY_ACC_LIMBS),
        sized(s.u_acc, (cap / COEF_CHUNK + 2) * KEY_ACC_LIMBS),   // one sum per fallback range
        sized(s.coef_part, coef_part_words(cap)),
        sized(s.itembad, 2 * cap),   // [0, cap): s bits (k_coef), [cap, 2 cap): R bits (k_decompress)
        sized(s.keybad, cap));
    if (e != hipSuccess) return e;
    launch_init_basepoint(s.st, s.pts);
    if ((e = hipGetLastError()) == hipSuccess) s.cap_T = T;
    return e;
  }));
  return 0;
}

// MSM workspace for plan P with up to `entries` digits (grow-only; the slot is idle when called)
static int ensure_msm(edc_ctx* ctx, Slot& s, const MsmPlan& P, size_t entries) {
  const uint32_t nbin = P.nbin();
  if (nbin > MSM_MAX_BINS || P.nwin > MSM_MAX_WIN) { ctx->err = "MSM plan too large"; return EDC_ERR_ARG; }
  MsmWs& w = s.msm;
  if (nbin > w.cap_bins || P.nranges > w.cap_ranges) {   // two capacities: each keeps its maximum
    CK(hipStreamSynchronize(s.st));
    const uint32_t nb = nbin > w.cap_bins ? nbin : w.cap_bins;
    const uint32_t nr = P.nranges > w.cap_ranges ? P.nranges : (w.cap_ranges ? w.cap_ranges : 1);
    w.cap_bins = w.cap_ranges = 0;
    CK(alloc_all(sized(w.counts, nb), sized(w.offsets, nb), sized(w.cursor, nb), sized(w.slice_W, (size_t)nb * EXT_WORDS),
                 sized(w.slice_T, (size_t)nb * EXT_WORDS), sized(w.win, (size_t)nr * MSM_MAX_WIN * EXT_WORDS),
                 sized(w.buckets, msm_bucket_words(nb)), sized(w.heads, msm_bucket_words(nb)),
                 sized(w.bucket_end, (size_t)nb * NSLICE)));
    w.cap_bins = nb;
    w.cap_ranges = nr;
  }
  if (entries > w.cap_entries)
    CK(grow_group(w.cap_entries, entries, entry_cap, sync_of(s.st), [&](size_t cap) {
      // + 256 per possible bin: each bin's lane-major region is padded to whole rounds (k_msm_sort)
      return alloc_all(sized(w.entries, cap), sized(w.sorted, cap + 256 * (size_t)MSM_MAX_BINS));
    }));
  return 0;
}

// ---- MSM plans ----
// Window width by batch size: wide windows amortize the 2 x buckets reduction work over many
// points; narrow ones keep enough digits per bucket for small batches. Below 2^13 signatures the
// windows are at most 9 bits (256 signed buckets, 8-bit unsigned top windows), i.e. one slice
// each, so no window-combine pass runs before the Horner pass (~90 us of latency per call).
static int auto_window_bits(size_t n) {
  if (n >= (1u << 19)) return 16;
  if (n >= (1u << 17)) return 15;   // 9 z windows; 14 bits 2 % and 16 bits 15 % slower at 2^17 (r06w)
  if (n >= (1u << 15)) return 13;
  if (n >= (1u << 13)) return 12;
  return 9;
}

// Windows of at most c bits over the 128 bits of a z (short scalars: windows 0..ws-1), then
// windows of at most hi bits over bits 128..252 of the full-width coefficients (< l < 2^253). The
// top window of each kind is unsigned (nothing sits above it, so no carry out): its digit reaches
// 2^bits, hence 2^bits buckets instead of 2^(bits-1). Widths are balanced: a window with only a
// few live bits would send every term's digit to a handful of buckets of one bin, i.e. one
// workgroup. Every slice starts as one bin (nsub = 1; batch_plan may split them).
static void plan_layout(MsmPlan& P) {
  uint32_t bin = 0;
  for (uint32_t w = 0; w < P.nwin; ++w) {
    P.bin0[w] = (uint16_t)bin;
    bin += (uint32_t)P.nslice[w] * P.nsub[w];
  }
  P.bins_per_range = bin;
}

static MsmPlan make_plan(int c, int hi, uint32_t nranges, bool hi_windows = true) {
  MsmPlan P{};
  uint32_t w = 0, off = 0;
  auto add = [&](uint32_t bits, uint32_t buckets) {
    P.off[w] = (uint16_t)off;
    P.bits[w] = (uint8_t)bits;
    P.nslice[w] = (uint16_t)((buckets + NSLICE - 1) / NSLICE);
    P.nsub[w] = 1;
    off += bits;
    ++w;
  };
  const uint32_t ws = (128 + c - 1) / c;
  for (uint32_t i = 0; i < ws; ++i) {
    const uint32_t bits = 128 / ws + (i < 128 % ws ? 1 : 0);
    add(bits, i + 1 == ws ? (1u << bits) : (1u << (bits - 1)));
  }
  P.nwin_short = ws;
  const uint32_t wh = hi_windows ? (125 + hi - 1) / hi : 0;
  for (uint32_t i = 0; i < wh; ++i) {
    const uint32_t bits = 125 / wh + (i < 125 % wh ? 1 : 0);
    add(bits, i + 1 == wh ? (1u << bits) : (1u << (bits - 1)));
  }
  P.nwin = w;
  P.nranges = nranges;
  plan_layout(P);
  return P;
}

// Host-side record of the plan just chosen, for edc_debug_last_plan (tests): no device work.
// target 0: explicit parts, the sub-bin split did not run.
static void note_plan(edc_ctx* ctx, const MsmPlan& P, double target, bool per_sig, bool split, bool few, bool fold) {
  edc_plan_info& I = ctx->last_plan;
  I = edc_plan_info{};
  I.nwin = P.nwin; I.nwin_short = P.nwin_short; I.nranges = P.nranges; I.sum_ranges = P.sum_ranges;
  I.bins_per_range = P.bins_per_range;
  I.per_sig = per_sig; I.split = split; I.few = few; I.fold = fold;
  I.target = target;
  for (uint32_t w = 0; w < P.nwin; ++w) { I.bits[w] = P.bits[w]; I.nsub[w] = P.nsub[w]; I.nslice[w] = P.nslice[w]; }
  ctx->have_plan = true;
}

static uint32_t floor_pow2(double x) {
  uint32_t p = 1;
  while (p * 2.0 <= x && p < 64) p *= 2;
  return p;
}

// Batch plan: few distinct keys (consensus votes; known from the previous grouped batch on this
// context) put the 253-bit B / key coefficients' high bits in 8-bit windows with ~m entries each
// (one bin per window instead of 128 nearly empty ones); otherwise every window has c bits.
// Small batches split the slices of their densest windows into sub-bins (terms interleaved by
// index, summed per slice by k_msm_window) so that every bin holds about the same number of
// entries and ~1-2k workgroups accumulate. edc_set_msm_shape's parts instead split the whole batch.
// Any plan is an exact MSM: the hint and the split only affect speed.
static MsmPlan batch_plan(edc_ctx* ctx, size_t n, bool per_sig, bool split = false) {
  const int c = ctx->win_bits ? ctx->win_bits : auto_window_bits(n);
  const bool few = !per_sig && ctx->have_key_ratio && ctx->last_key_ratio * 16.0 <= 1.0 && n >= 4096;
  MsmPlan P = make_plan(c, few ? 8 : c, 1, !split);
  if (ctx->msm_parts) {
    uint32_t parts = ctx->msm_parts;
    while (parts > 1 && P.bins_per_range * parts > MSM_MAX_BINS) parts /= 2;
    P.nranges = parts;
    P.sum_ranges = parts > 1;
    note_plan(ctx, P, 0.0, per_sig, split, few, false);
    return P;
  }
  // expected entries per slice of each window: short terms (the z_i) use the short windows, full
  // terms (B and the keys: m estimated from the last grouped batch, n per signature) all windows.
  // Only the lower half of two windows' slices is live: in the top short window the full terms'
  // digits are signed, and in the top full window bit 252 is set only by coefficients in
  // [2^252, l), a 2^-125 fraction.
  const double ns = (double)n;
  const double nf = 1.0 + (per_sig ? ns : (ctx->have_key_ratio ? ctx->last_key_ratio * ns : ns));
  double dens[MSM_MAX_WIN], total = 0;
  for (uint32_t w = 0; w < P.nwin; ++w) {
    const double sl = P.nslice[w], half = sl > 1 ? sl / 2 : 1;
    if (split) dens[w] = (ns + 2 * nf) / sl;      // every term short, top windows unsigned
    else if (w + 1 < P.nwin_short) dens[w] = (ns + nf) / sl;
    else if (w + 1 == P.nwin_short) dens[w] = ns / sl + nf / half;
    else if (w + 1 < P.nwin) dens[w] = nf / sl;
    else dens[w] = nf / half;
    total += split ? ns + 2 * nf : (w < P.nwin_short ? ns + nf : nf);
  }
  double target = ctx->bin_entries ? (double)ctx->bin_entries : (total / 1024.0 > 4096.0 ? total / 1024.0 : 4096.0);
  for (;;) {
    for (uint32_t w = 0; w < P.nwin; ++w) P.nsub[w] = (uint8_t)floor_pow2(dens[w] / target);
    plan_layout(P);
    if (P.bins_per_range <= MSM_MAX_BINS) break;
    target *= 2;
  }
  note_plan(ctx, P, target, per_sig, split, few, false);
  return P;
}

static MsmTerms batch_terms(const MsmPlan& P, const Slot& s, uint32_t n, bool split, uint32_t skip = 0) {
  return MsmTerms{n - skip, 0, 0, 0, P.sum_ranges ? P.nranges : 1u, s.scal, nullptr, nullptr, nullptr, split ? 1u : 0u,
                  0u, skip};
}

// Split coefficients need [2^128]A of every key of the batch; the cache holds it for registered
// keys. They are planned while the previous batch found all its keys in the cache (a key missing
// from it still verifies exactly: k_decompress doubles it 128 times, and the next batches go back
// to the wide-coefficient plan until a batch finds every key again).
static bool choose_split(const edc_ctx* ctx) {
  return ctx->kc_m && ctx->bcomb && ctx->key_split == 0 && ctx->last_uncached == 0;
}

// host-staging buffers (inputs of the host-pointer entry points, per-item outputs)
static int ensure_n(edc_ctx* ctx, size_t n) {
  CK(grow_group(ctx->cap_n, n, item_cap, sync_of(ctx->st()), [&](size_t cap) {
    return alloc_all(sized(ctx->vtab, verify_single_scratch_words(cap)), sized(ctx->vk, cap * 32), sized(ctx->sig, cap * 64),
                     sized(ctx->zexp, cap * 16), sized(ctx->off, cap + 1), sized(ctx->kbuf, cap * 8), sized(ctx->verdicts, cap));
  }));
  return 0;
}

static int ensure_msg(edc_ctx* ctx, size_t bytes) {
  CK(grow(ctx->msg, bytes, byte_cap, sync_of(ctx->st())));
  return 0;
}

static int ensure_aux(edc_ctx* ctx, size_t bytes) {
  CK(grow(ctx->aux, bytes, byte_cap, sync_of(ctx->st())));
  return 0;
}

static void seed_words(const uint8_t* seed, uint32_t w[8]) {
  for (int j = 0; j < 8; ++j)
    w[j] = seed ? ((uint32_t)seed[4 * j] | ((uint32_t)seed[4 * j + 1] << 8) | ((uint32_t)seed[4 * j + 2] << 16) |
                   ((uint32_t)seed[4 * j + 3] << 24))
                : 0u;
}

// The message offsets as the kernels read them (0-based): the caller's own when they start at 0,
// else rebased into `keep`, which must outlive the copy that reads it.
static const uint64_t* rebased_offsets(size_t n, const uint64_t* msg_off, std::vector<uint64_t>& keep) {
  if (msg_off[0] == 0) return msg_off;
  keep.resize(n + 1);
  for (size_t i = 0; i <= n; ++i) keep[i] = msg_off[i] - msg_off[0];
  return keep.data();
}

// Stage the message arena + offsets (0-based) into the context's device buffers (slot 0 stream).
static int upload_msgs(edc_ctx* ctx, size_t n, const uint8_t* msg, const uint64_t* msg_off) {
  if (n && !msg_off) { ctx->err = "null msg_off"; return EDC_ERR_ARG; }
  int rc = init_slot(ctx, ctx->slot[0]);
  if (rc) return rc;
  rc = ensure_n(ctx, n);
  if (rc) return rc;
  const size_t mbytes = n ? (size_t)(msg_off[n] - msg_off[0]) : 0;
  if (mbytes && !msg) { ctx->err = "null msg"; return EDC_ERR_ARG; }
  rc = ensure_msg(ctx, mbytes);
  if (rc) return rc;
  if (!n) return 0;
  hipStream_t st = ctx->st();
  if (mbytes) CK(hipMemcpyAsync(ctx->msg, msg + msg_off[0], mbytes, hipMemcpyHostToDevice, st));
  std::vector<uint64_t> tmp;
  const uint64_t* off = rebased_offsets(n, msg_off, tmp);
  CK(hipMemcpyAsync(ctx->off, off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (off != msg_off) CK(hipStreamSynchronize(st));   // tmp does not outlive this call
  return 0;
}

// Stage host items into the context's device buffers on slot 0's stream: keys, signatures and
// either the messages (k null: upload_msgs, which also makes the room) or the 32-byte challenges
// into k_dst, the slot's k array or ctx->kbuf, for which the caller has made the room (its own
// ensure_* calls). No synchronization beyond upload_msgs' own.
static int stage_host(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                      const uint64_t* msg_off, const uint8_t* k = nullptr, uint32_t* k_dst = nullptr) {
  if (n && (!vk || !sig)) { ctx->err = "null input"; return EDC_ERR_ARG; }
  int rc = k ? 0 : upload_msgs(ctx, n, msg, msg_off);
  if (rc || !n) return rc;
  CK(hipMemcpyAsync(ctx->vk, vk, n * 32, hipMemcpyHostToDevice, ctx->st()));
  CK(hipMemcpyAsync(ctx->sig, sig, n * 64, hipMemcpyHostToDevice, ctx->st()));
  if (k) CK(hipMemcpyAsync(k_dst, k, n * 32, hipMemcpyHostToDevice, ctx->st()));
  return 0;
}

// Stage host inputs into slot s's own device buffers on the slot's stream (edc_batch_submit), so
// the copy of one batch overlaps the kernels of the batches already in flight on other slots.
static int ensure_slot_inputs(edc_ctx* ctx, Slot& s, size_t n, size_t mbytes) {
  int rc = init_slot(ctx, s);
  if (rc) return rc;
  CK(grow_group(s.in_cap_n, n, item_cap, sync_of(s.st), [&](size_t cap) {
    return alloc_all(sized(s.in_vk, cap * 32), sized(s.in_sig, cap * 64), sized(s.in_off, cap + 1), sized(s.in_idx, cap));
  }));
  CK(grow(s.in_msg, mbytes, byte_cap, sync_of(s.st)));
  return 0;
}

// Keys and signatures of n > 0 host items onto the device: key_idx given, 4 bytes per item over
// PCIe instead of 32 (d_idx) and the registered keys expanded from them, else the keys themselves;
// then the signatures.
static int stage_keys_sigs(edc_ctx* ctx, hipStream_t st, size_t n, const uint8_t* vk, const uint32_t* key_idx,
                           const uint8_t* sig, uint32_t* d_idx, uint8_t* d_vk, uint8_t* d_sig) {
  if (key_idx) {
    CK(hipMemcpyAsync(d_idx, key_idx, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    launch_expand_keys(st, (uint32_t)n, d_idx, ctx->kc_reg, ctx->kc_keys, d_vk);
    CK(hipGetLastError());
  } else {
    CK(hipMemcpyAsync(d_vk, vk, n * 32, hipMemcpyHostToDevice, st));
  }
  CK(hipMemcpyAsync(d_sig, sig, n * 64, hipMemcpyHostToDevice, st));
  return 0;
}

// One batch's inputs as enqueue_batch, run_batch_sync, batch_with_fallback and fallback_ranges
// read them, all on the device: the items (keys, signatures and either the message arena with its
// 0-based offsets or, k given, the prehashed challenges: then the messages are not read and may be
// null), where z comes from (d_z, else drawn from z_seed at z_base + i), and whether the result
// block carries the compressed check8 (a submission's want_check8; the synchronous helpers set it
// themselves from the check8 they are given).
struct BatchIn {
  const uint8_t *vk, *sig, *msg;
  const uint64_t* off;
  const uint32_t* k;
  const uint8_t* z_seed;
  uint64_t z_base;
  const uint8_t* d_z;
  bool compress;
};

// Messages (k null) or, for prehashed items (reference Item = {vk_bytes, sig, k},
// src/batch.rs:76-80), the 32-byte challenges straight into the slot's k array: 128 B per item
// over PCIe, 100 B with key_idx, and no message bytes. `in` is pointed at the staged items.
static int upload_slot(edc_ctx* ctx, Slot& s, size_t n, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                       const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k, BatchIn& in) {
  if (n && ((!vk && !key_idx) || !sig || (!k && !msg_off))) { ctx->err = "null input"; return EDC_ERR_ARG; }
  const size_t mbytes = n && !k ? (size_t)(msg_off[n] - msg_off[0]) : 0;
  if (mbytes && !msg) { ctx->err = "null msg"; return EDC_ERR_ARG; }
  int rc = ensure_slot_inputs(ctx, s, n, mbytes);
  if (!rc && k) rc = ensure_slot(ctx, s, n);
  if (rc) return rc;
  in.vk = s.in_vk;
  in.sig = s.in_sig;
  in.msg = k ? nullptr : s.in_msg.get();
  in.off = k ? nullptr : s.in_off.get();
  in.k = k ? s.k.get() : nullptr;
  if (!n) return 0;
  hipStream_t st = s.st;
  if (k) {
    if ((rc = stage_keys_sigs(ctx, st, n, vk, key_idx, sig, s.in_idx, s.in_vk, s.in_sig))) return rc;
    CK(hipMemcpyAsync(s.k, k, n * 32, hipMemcpyHostToDevice, st));
    return 0;
  }
  // rebased offsets stay alive in the slot until it is reused
  CK(hipMemcpyAsync(s.in_off, rebased_offsets(n, msg_off, s.in_rebased), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (mbytes) CK(hipMemcpyAsync(s.in_msg, msg + msg_off[0], mbytes, hipMemcpyHostToDevice, st));
  return stage_keys_sigs(ctx, st, n, vk, key_idx, sig, s.in_idx, s.in_vk, s.in_sig);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// caller-supplied device arrays are read with 16-byte loads: every pointer given (null: not given,
// passes) must be aligned; `what` names them in the refusal
static int check_aligned16(edc_ctx* ctx, const char* what, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!aligned16(p)) { ctx->err = std::string(what) + " must be 16-byte aligned"; return EDC_ERR_ARG; }
  return 0;
}
// sub-arrays of one staged piece start at 16-byte boundaries
static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Scalar::from_hash never yields k >= l: the per-item entries refuse such a caller k here, on the
// host; the batch entries refuse it at the wait (FLAG_KARG)
static int k_all_canonical(edc_ctx* ctx, size_t n, const uint8_t* k) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8];
    memcpy(w, k + 32 * i, 32);
    if (!sc_is_canonical(w)) { ctx->err = "prehashed k is not a canonical scalar"; return EDC_ERR_ARG; }
  }
  return 0;
}

static uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Key grouping (the reference's HashMap<VerificationKeyBytes, _>, src/batch.rs:114-137) only
// saves work when keys repeat. When the last grouped batch had almost only distinct keys, the
// key terms stay per signature (A_i with coefficient z_i k_i): the same group element, so the
// same verdict and [8]check, without the hash table and the per-key atomics. Auto mode groups
// every 8th batch anyway, to notice when keys start repeating.
static bool choose_per_sig(const edc_ctx* ctx, size_t n) {
  return ctx->key_grouping == 2 || (ctx->key_grouping == 0 && n >= 4096 && ctx->have_key_ratio &&
                                    ctx->last_key_ratio > 0.5 && ctx->ungrouped_run < 7);
}

// Key lanes of a batch's decode launch. The distinct-key count m is only known on the device, so
// every possible key (m <= n) used to get a lane: at 2^20 votes from 150 validators, 2^20 lanes
// (16,384 waves) that exit at once. Grouped batches now get twice the previous grouped batch's key
// count (at least 4,096 lanes); a batch with more keys loops over them (k_decompress), so the
// hint only affects speed. One key term per signature: m = n exactly.
static uint32_t key_lanes(const edc_ctx* ctx, size_t n, bool per_sig) {
  if (per_sig || !ctx->have_key_ratio) return (uint32_t)n;
  const double m2 = 2.0 * ctx->last_key_ratio * (double)n;
  const size_t lanes = m2 < 4096.0 ? 4096 : (size_t)m2 + 64;
  return (uint32_t)(lanes < n ? lanes : n);
}

// ---- the front of a batch ----
// the header of the batch about to be enqueued on slot s (kin: where its challenges are read)
static void slot_begin(Slot& s, const uint32_t* kin, uint32_t nmulti, bool timed, bool per_sig, uint32_t n) {
  s.kin = kin;
  s.nmulti = nmulti;
  s.timed = timed;
  s.per_sig = per_sig;
  s.n_batch = n;
}
// digit entries and terms of an n-item batch's MSM (wide or split coefficients, edc_common.h)
static size_t batch_entry_room(const MsmPlan& P, size_t n, bool split) {
  return split ? msm_entry_capacity(P, 2 + 3 * n, 0) : msm_entry_capacity(P, n, n + 1);
}
static uint32_t batch_term_count(uint32_t n, bool split) { return split ? 2 + 3 * n : 1 + 2 * n; }

// The key table of one batch: T slots of the slot's hash table and, when it groups its keys, the salt
struct KeyTable {
  uint32_t T = 0, salt[2] = {0, 0};
  bool per_sig = false, force_overflow = false;
};
// Host only: the table of an n-item batch on slot s (refused when the slot's arrays cannot hold
// it). A grouping batch draws a fresh salt, one step of the context's batch counter.
static int key_table(edc_ctx* ctx, const Slot& s, size_t n, bool per_sig, KeyTable& kt) {
  kt.T = (uint32_t)next_pow2(2 * (n < 128 ? 128 : n));
  kt.per_sig = per_sig;
  kt.force_overflow = ctx->key_grouping == 3;
  if (kt.T > s.cap_T) { ctx->err = "hash table capacity"; return EDC_ERR_ARG; }
  if (!per_sig) {
    const uint64_t h = splitmix64(ctx->secret ^ splitmix64(ctx->nbatches++));
    kt.salt[0] = (uint32_t)h;
    kt.salt[1] = (uint32_t)(h >> 32);
  }
  return 0;
}

// The per-batch resets (with the MSM bin counts[0..nbin), or null / 0) and, when grouping, the key
// grouping of the n keys at vk (kstride: launch_keys' kcap). before_keys runs between the two
// launches (the chunked path waits there for its keys to land); false from it ends the front.
static bool no_wait() { return true; }
template <typename F = bool (*)()>
static bool launch_front(hipStream_t st, Slot& s, const KeyTable& kt, uint32_t n, const uint8_t* vk, uint32_t* counts,
                         uint32_t nbin, uint32_t kstride = 0xFFFFFFFFu, F before_keys = no_wait) {
  launch_init_batch(st, s.flags, kt.per_sig ? (int)n : -1, s.u_acc, s.d_out, kt.per_sig ? nullptr : s.table.get(),
                    kt.per_sig ? 0u : kt.T, counts, nbin);
  if (!before_keys()) return false;
  if (!kt.per_sig)
    launch_keys(st, n, vk, s.table, kt.T - 1, kt.salt, kt.force_overflow, s.slot_key, s.key_slot, s.key_rep, s.key_index,
                s.key_acc, s.flags, kstride);
  return true;
}

// Enqueue the per-signature prefix of the pipeline on slot s: key grouping, SHA-512 challenges,
// z and coefficients, ZIP215 decode of R_i and the keys. No host synchronization. With d_k (the
// prehashed entries: the caller's queue-time k, src/batch.rs:76-94) SHA-512 is skipped and the
// messages are not read (d_msg / d_off may be null).
static int enqueue_prefix(edc_ctx* ctx, Slot& s, size_t n, const BatchIn& in, const MsmPlan* P,
                          bool force_per_sig = false, bool split = false) {
  const uint8_t *d_vk = in.vk, *d_sig = in.sig, *d_z = in.d_z;
  const uint32_t* d_k = in.k;
  const bool with_bin = P != nullptr;
  if (n >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  int rc = n ? check_aligned16(ctx, "device vk / sig / z / k arrays", {d_vk, d_sig, d_z, d_k}) : 0;
  if (!rc) rc = ensure_slot(ctx, s, n);
  if (rc) return rc;
  const uint32_t N = (uint32_t)n;
  const bool per_sig = force_per_sig || choose_per_sig(ctx, n);
  KeyTable kt;
  if ((rc = key_table(ctx, s, n, per_sig, kt))) return rc;
  slot_begin(s, d_k ? d_k : s.k.get(), 0, ctx->timing, per_sig, N);
  uint32_t seed[8];
  seed_words(in.z_seed, seed);
  hipStream_t st = s.st;
  auto mark = [&](int ph) {
    if (s.timed) (void)hipEventRecord(s.ev[ph], st);
  };
  mark(PH_KEYS);
  const bool clear_counts = with_bin && EDC_RUN(8);
  launch_front(st, s, kt, N, d_vk, clear_counts ? s.msm.counts.get() : nullptr, clear_counts ? P->nbin() : 0u);
  // dual-stream builds (untimed batches): the decode only needs the key grouping, so it runs on
  // the slot's second stream beside SHA-512 / coefficients / binning; its per-item R bits go to
  // their own array (itembad + cap_n), so no byte is written by both streams.
  // Contract while st2 runs (between ev_keys and the wait on ev_dec below): k_decompress reads
  // d_sig, d_vk, key_rep, flags[FLAG_NKEYS / FLAG_OVF] and the key cache, and writes pts,
  // itembad + cap_n, keybad and flags[FLAG_BAD / FLAG_UNCACHED] (atomics). The kernels enqueued on
  // st in between (coefficients, binning, bucket sort) must not read pts / keybad / itembad + cap_n,
  // write key_rep or FLAG_NKEYS / FLAG_OVF, or plain-store into flags; anything that does must
  // come after the ev_dec wait. tests/test_gpu_prehashed.py compares slot 0 (dual stream) with a
  // pipelined slot (one stream) on batches that fail in the decode and in the s check.
  // The decode is released after SHA-512, not right after the key grouping: both are VALU-bound,
  // and a decode launched first fills the GPU and starves SHA-512 (measured: the challenge took
  // ~1.0 ms beside the decode instead of 0.22 ms alone), so the light coefficient / binning /
  // sort chain queued behind SHA-512 ran after the decode instead of beside it.
  const bool dual = EDC_DUAL_STREAM && s.st2 && !s.timed;
  mark(PH_CHALLENGE);
  if (!d_k && EDC_RUN(2)) launch_challenge(st, N, d_vk, d_sig, in.msg, in.off, s.k);
  if (dual) {
    CK(hipEventRecord(s.ev_keys, st));
    CK(hipStreamWaitEvent(s.st2, s.ev_keys, 0));
    if (EDC_RUN(16))
      launch_decompress(s.st2, N, d_sig, d_vk, s.key_rep, per_sig, s.pts, s.itembad + s.cap_n, s.keybad, s.flags,
                        ctx->kc(), split, key_lanes(ctx, n, per_sig));
    CK(hipEventRecord(s.ev_dec, s.st2));
  }
  mark(PH_COEF);
  if (EDC_RUN(4)) launch_coef(st, N, d_sig, s.kin, d_z, seed, in.z_base, s.key_index, s.scal, s.key_acc, s.u_acc, s.itembad, s.flags,
              per_sig, s.coef_part, split);
  mark(PH_MSM_BIN);
  if (with_bin && EDC_RUN(8))
    launch_msm_bin(st, *P, batch_terms(*P, s, N, split), batch_term_count(N, split), s.msm, s.flags, true);
  // the per-bin bucket sort needs only the binning: before the decode join, so on the dual-stream
  // slot it runs beside the decode instead of after it
  if (with_bin && EDC_RUN(256)) launch_msm_sort(st, *P, s.msm);
  // the points are decoded last, right before the accumulation gathers them, so the freshly
  // written point table (134 MB at 2^20) is still in the Infinity Cache for the random row gathers
  mark(PH_DECOMP);
  if (dual) CK(hipStreamWaitEvent(st, s.ev_dec, 0));
  else if (EDC_RUN(16))
    launch_decompress(st, N, d_sig, d_vk, s.key_rep, per_sig, s.pts, s.itembad + s.cap_n, s.keybad, s.flags, ctx->kc(),
                      split, key_lanes(ctx, n, per_sig));
  CK(hipGetLastError());
  return 0;
}

// Enqueue the whole batch pipeline on slot s (device-resident inputs); no host synchronization.
static int enqueue_batch(edc_ctx* ctx, Slot& s, size_t n, const BatchIn& in, bool latency = false) {
  if (n >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  int rc = ensure_slot(ctx, s, n);
  if (rc) return rc;
  const bool per_sig = choose_per_sig(ctx, n), split = choose_split(ctx);
  const MsmPlan P = batch_plan(ctx, n, per_sig, split);
  rc = ensure_msm(ctx, s, P, batch_entry_room(P, n, split));
  if (rc) return rc;
  rc = enqueue_prefix(ctx, s, n, in, &P, per_sig, split);
  if (rc) return rc;
  hipStream_t st = s.st;
  if (s.timed) (void)hipEventRecord(s.ev[PH_MSM_BUCKET], st);
  launch_msm_bucket(st, P, s.msm, s.pts, s.probe_runs ? EDC_PROBE_SKIP : 0, s.timed ? s.ev_acc[0] : nullptr,
                    s.timed ? s.ev_acc[1] : nullptr, latency, s.flags);
  s.acc_nbin = P.nbin();
  if (s.timed) (void)hipEventRecord(s.ev[PH_MSM_TAIL], st);
  // the final kernel stores the result block to d_out and straight into the pinned h_out
  if (EDC_RUN(128)) launch_msm_tail(st, P, s.msm, s.flags, in.compress, s.d_out, s.h_out);
  if (s.timed) {
    (void)hipEventRecord(s.ev[PH_N], st);
    // the accumulation's entry count (the last bin's offset + count), read at the wait without
    // another sync; queued after the last phase event so that no phase time includes the copies
    if (s.acc_nbin) {
      CK(hipMemcpyAsync(s.h_acc, s.msm.offsets + s.acc_nbin - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      CK(hipMemcpyAsync(s.h_acc + 1, s.msm.counts + s.acc_nbin - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
  }
  CK(hipGetLastError());
  s.pending = true;
  s.probe_runs++;
  return 0;
}

// ---- several batches in one launch sequence (edc_batch_submit_multi_device) ----
// nb consecutive batches of n_per items each (a node verifying several blocks at once, or one
// GPU's shards of consecutive blocks): every per-item kernel runs once over all nb * n_per items,
// so small batches fill the GPU like one large batch, and the MSM is range-tagged (one range per
// batch, the plan of an n_per batch in each) with one Horner, verdict, check8 and partial per
// range. Batch b's z are drawn at z_base + b n_per + i: its results equal a separate
// edc_batch_verify_device / edc_batch_partial_device of batch b at that z_base. The grouped
// fallback's range machinery (k_coef range mode, listed key / B terms) with the key count left
// on the device: per-(batch, key) sums sit at b * kstride + key and the term layout is resolved
// from the key grouping by the binning kernels (MsmTerms::dyn).
static int multi_args(edc_ctx* ctx, uint32_t nb, size_t n_per, const uint8_t* d_vk, const uint8_t* d_sig,
                      const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_k) {
  if (nb < 1 || nb > kMultiMax || n_per == 0 || n_per % COEF_CHUNK) {
    ctx->err = "multi-batch: 1..16 batches of a multiple of 2048 items each";
    return EDC_ERR_ARG;
  }
  if ((size_t)nb * n_per >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  if (check_aligned16(ctx, "device vk / sig / k arrays", {d_vk, d_sig, d_k})) return EDC_ERR_ARG;
  if (!d_k && (!d_msg || !d_off)) { ctx->err = "null msg"; return EDC_ERR_ARG; }
  return 0;
}

static int enqueue_multi(edc_ctx* ctx, Slot& s, uint32_t nb, size_t n_per, const uint8_t* d_vk, const uint8_t* d_sig,
                         const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_k, const uint8_t* z_seed,
                         uint64_t z_base, int want_compress) {
  int rc = multi_args(ctx, nb, n_per, d_vk, d_sig, d_msg, d_off, d_k);
  if (rc) return rc;
  const size_t N = (size_t)nb * n_per;
  rc = ensure_slot(ctx, s, N);
  if (rc) return rc;
  const bool per_sig = choose_per_sig(ctx, N);
  const uint32_t kstride = (uint32_t)(N < kMultiKeys ? N : kMultiKeys);
  MsmPlan P = batch_plan(ctx, n_per, per_sig, false);
  P.nranges = nb;
  P.sum_ranges = 0;
  if (P.bins_per_range * nb > MSM_MAX_BINS) {       // drop the sub-bins of the per-batch plan
    for (uint32_t w = 0; w < P.nwin; ++w) P.nsub[w] = 1;
    plan_layout(P);
  }
  if (P.bins_per_range * nb > MSM_MAX_BINS) { ctx->err = "multi-batch: too many batches for the MSM plan"; return EDC_ERR_ARG; }
  note_plan(ctx, P, ctx->last_plan.target, per_sig, false, ctx->last_plan.few != 0, false);   // as launched: nb ranges
  const size_t nx_max = (size_t)nb * kstride + nb;
  const size_t full_max = (N > (size_t)nb * kstride ? N : (size_t)nb * kstride) + nb;
  rc = ensure_msm(ctx, s, P, msm_entry_capacity(P, N, full_max));
  if (rc) return rc;
  if ((size_t)nb * kstride * KEY_ACC_LIMBS > s.mb_acc.cap() || nx_max > s.mb_xpt.cap() || !s.mb_bad) {
    CK(hipStreamSynchronize(s.st));
    const size_t acc = (size_t)kMultiMax * kMultiKeys * KEY_ACC_LIMBS, terms = (size_t)kMultiMax * kMultiKeys + kMultiMax;
    CK(alloc_all(sized(s.mb_acc, acc), sized(s.mb_xpt, terms), sized(s.mb_xrg, terms), sized(s.mb_xscal, terms * 8),
                 sized(s.mb_bad, kMultiMax)));
  }
  const uint32_t n = (uint32_t)N;
  KeyTable kt;
  if ((rc = key_table(ctx, s, N, per_sig, kt))) return rc;
  uint32_t seed[8];
  seed_words(z_seed, seed);
  hipStream_t st = s.st;
  slot_begin(s, d_k ? d_k : s.k.get(), nb, false, per_sig, n);
  launch_front(st, s, kt, n, d_vk, s.msm.counts, P.nbin(), kstride);
  const bool dual = EDC_DUAL_STREAM && s.st2;       // same contract (and order) as enqueue_prefix
  if (!d_k) launch_challenge(st, n, d_vk, d_sig, d_msg, d_off, s.k);
  if (dual) {
    CK(hipEventRecord(s.ev_keys, st));
    CK(hipStreamWaitEvent(s.st2, s.ev_keys, 0));
    launch_decompress(s.st2, n, d_sig, d_vk, s.key_rep, per_sig, s.pts, s.itembad + s.cap_n, s.keybad, s.flags, ctx->kc(),
                      false, key_lanes(ctx, N, per_sig));
    CK(hipEventRecord(s.ev_dec, s.st2));
  }
  launch_multi_coef(st, n, nb, kstride, per_sig, d_sig, s.kin, seed, z_base, s.key_index, s.scal, s.mb_acc, s.u_acc,
                    s.itembad, s.flags, s.mb_xpt, s.mb_xrg, s.mb_xscal);
  const MsmTerms terms{n, (uint32_t)n_per, 0u, nb, 1u, s.scal, s.mb_xpt, s.mb_xrg, s.mb_xscal, 0u, per_sig ? 3u : 1u};
  launch_msm_bin(st, P, terms, (uint32_t)(N + full_max), s.msm, s.flags, true);
  launch_msm_sort(st, P, s.msm);
  if (dual) CK(hipStreamWaitEvent(st, s.ev_dec, 0));
  else
    launch_decompress(st, n, d_sig, d_vk, s.key_rep, per_sig, s.pts, s.itembad + s.cap_n, s.keybad, s.flags, ctx->kc(),
                      false, key_lanes(ctx, N, per_sig));
  CK(hipMemsetAsync(s.mb_bad, 0, nb, st));
  launch_range_prebad(st, n, (uint32_t)n_per, s.itembad, s.itembad + s.cap_n, s.keybad, s.key_index, per_sig, s.mb_bad,
                      s.flags);
  launch_msm_bucket(st, P, s.msm, s.pts);
  launch_msm_multi_tail(st, P, s.msm, s.flags, s.mb_bad, want_compress, s.d_out, s.h_out);
  CK(hipGetLastError());
  s.pending = true;
  return 0;
}

// Wait for a multi-batch slot: per batch verdict (EDC_OK / EDC_INVALID_SIGNATURE), optional
// check8 (nb x 32), partial (nb x 128) and bad flag; returns EDC_INVALID_SIGNATURE if any failed.
static int finish_multi(edc_ctx* ctx, Slot& s, size_t nb, int* verdicts, uint8_t* check8, uint8_t* partials, int* bad) {
  if (!s.pending || !s.nmulti) { ctx->err = "no multi-batch pending in this slot"; return EDC_ERR_ARG; }
  if (nb != s.nmulti) { ctx->err = "multi-batch count differs from the submission"; return EDC_ERR_ARG; }
  if (s.mu_union) {
    // The launch ran as one batch over all nb * n_per items (z at the same global indices). Its
    // equation is the sum of the nb batches' equations, so when it holds every batch holds (with
    // the probability batch verification itself gives: src/batch.rs:149-217) and each batch's
    // [8]*check is the identity. Otherwise, or when the caller wants the per-batch partials, the
    // launch is rerun range by range on the same slot (the inputs are still borrowed).
    s.mu_union = false;
    CK(hipStreamSynchronize(s.st));
    const int* u = reinterpret_cast<const int*>(s.h_out.get());
    if (u[45]) {
      s.pending = false;
      s.nmulti = 0;
      ctx->err = "prehashed k is not a canonical scalar (must be < l, as Scalar::from_hash returns)";
      return EDC_ERR_ARG;
    }
    if (!u[0] && !u[1] && !partials) {
      s.pending = false;
      s.nmulti = 0;
      if (s.per_sig) {
        ctx->ungrouped_run++;
      } else {
        ctx->ungrouped_run = 0;
        ctx->have_key_ratio = true;
        ctx->last_key_ratio = (double)u[2] / (double)s.n_batch;
      }
      if (ctx->kc_m) ctx->last_uncached = (uint32_t)u[44];
      ctx->mu_hits++;
      for (size_t g = 0; g < nb; ++g) {
        if (verdicts) verdicts[g] = EDC_OK;
        if (bad) bad[g] = 0;
        if (check8) {
          memset(check8 + 32 * g, 0, 32);
          check8[32 * g] = 1;                         // compressed identity
        }
      }
      return EDC_OK;
    }
    ctx->mu_reruns++;
    s.pending = false;
    s.nmulti = 0;
    int rc = enqueue_multi(ctx, s, (uint32_t)nb, s.mu_nper, s.mu_vk, s.mu_sig, s.mu_msg, s.mu_off, s.mu_k, s.mu_seed,
                           s.mu_zbase, s.mu_compress || check8 != nullptr);
    if (rc) return rc;
  }
  s.pending = false;
  s.nmulti = 0;
  CK(hipStreamSynchronize(s.st));
  const int* h0 = reinterpret_cast<const int*>(s.h_out.get());
  if (h0[45]) {
    ctx->err = "prehashed k is not a canonical scalar (must be < l, as Scalar::from_hash returns)";
    return EDC_ERR_ARG;
  }
  if (s.per_sig) {
    ctx->ungrouped_run++;
  } else {
    ctx->ungrouped_run = 0;
    ctx->have_key_ratio = true;
    ctx->last_key_ratio = (double)h0[2] / (double)s.n_batch;
  }
  if (ctx->kc_m) ctx->last_uncached = (uint32_t)h0[44];
  int any = 0;
  for (size_t g = 0; g < nb; ++g) {
    const uint8_t* b = s.h_out + 256 * g;
    const int v = reinterpret_cast<const int*>(b)[0], bd = reinterpret_cast<const int*>(b)[1];
    any |= v;
    if (verdicts) verdicts[g] = v ? EDC_INVALID_SIGNATURE : EDC_OK;
    if (bad) bad[g] = bd;
    if (check8) {
      if (bd) memset(check8 + 32 * g, 0, 32);
      else memcpy(check8 + 32 * g, b + 16, 32);
    }
    if (partials) memcpy(partials + 128 * g, b + 48, 128);
  }
  return any ? EDC_INVALID_SIGNATURE : EDC_OK;
}

#ifdef EDC_BATCH_STAMPS
// diagnostic build: one record per waited batch (ticket, n, host submit / wait-return time in us,
// the device phase stamps of edc_common.h BST_*), read and cleared by edc_debug_batch_stamps
static std::vector<uint32_t> g_bstamps;
static std::mutex g_bstamps_mu;    // contexts on several threads share the log
static uint64_t host_us() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}
extern "C" int edc_debug_batch_stamps(uint32_t* out, size_t cap_words) {
  std::lock_guard<std::mutex> g(g_bstamps_mu);
  const size_t n = std::min(cap_words, g_bstamps.size());
  if (out) memcpy(out, g_bstamps.data(), n * sizeof(uint32_t));
  g_bstamps.clear();
  return (int)(n / (4 + BST_N));
}
#endif

// Wait for slot s and harvest its result block (verdict, bad flag, check8, partial).
static int finish_batch(edc_ctx* ctx, Slot& s, uint8_t check8[32], uint8_t partial[128], int* bad_out) {
  if (!s.pending) { ctx->err = "no batch pending in this slot"; return EDC_ERR_ARG; }
  if (s.nmulti) { ctx->err = "multi-batch ticket: wait with edc_batch_wait_multi"; return EDC_ERR_ARG; }
  if (s.commits) { ctx->err = "commit-set ticket: wait with edc_commits_wait"; return EDC_ERR_ARG; }
  s.pending = false;
  CK(hipStreamSynchronize(s.st));
  if (s.timed) {
    for (int p = 0; p < PH_N; ++p) CK(hipEventElapsedTime(&ctx->last_ms[p], s.ev[p], s.ev[p + 1]));
    ctx->nlast = PH_N;
    CK(hipEventElapsedTime(&ctx->last_acc_ms, s.ev_acc[0], s.ev_acc[1]));
    // digit entries the accumulation added: the last bin's end (queued on s.st at the enqueue)
    ctx->last_acc_entries = s.acc_nbin ? s.h_acc[0] + s.h_acc[1] : 0;
  }
  const int verdict = reinterpret_cast<int*>(s.h_out.get())[0];
  const int bad = reinterpret_cast<int*>(s.h_out.get())[1];
#ifdef EDC_BATCH_STAMPS
  if (&s != &ctx->comb) {
    std::lock_guard<std::mutex> g(g_bstamps_mu);
    g_bstamps.push_back((uint32_t)s.ticket);
    g_bstamps.push_back(s.n_batch);
    g_bstamps.push_back((uint32_t)s.t_submit_us);
    g_bstamps.push_back((uint32_t)host_us());
    for (int k = 0; k < BST_N; ++k) g_bstamps.push_back(reinterpret_cast<uint32_t*>(s.h_out.get())[48 + k]);
  }
#endif
  if (&s != &ctx->comb && s.n_batch) {
    if (s.per_sig) {
      ctx->ungrouped_run++;
    } else {
      ctx->ungrouped_run = 0;
      ctx->have_key_ratio = true;
      ctx->last_key_ratio = (double)reinterpret_cast<int*>(s.h_out.get())[2] / (double)s.n_batch;
    }
    if (ctx->kc_m) ctx->last_uncached = (uint32_t)reinterpret_cast<int*>(s.h_out.get())[44];
  }
  if (&s != &ctx->comb && reinterpret_cast<int*>(s.h_out.get())[45]) {
    ctx->err = "prehashed k is not a canonical scalar (must be < l, as Scalar::from_hash returns)";
    return EDC_ERR_ARG;
  }
  if (s.tw.check) {             // templated device form: the batch ran over n empty messages
    s.tw.check = false;
    if (*s.tw.h_flag) {
      ctx->err = "templated items: template index or hole offsets out of range";
      return EDC_ERR_ARG;
    }
  }
  if (check8) {
    if (bad) memset(check8, 0, 32);
    else memcpy(check8, s.h_out + 16, 32);
  }
  if (partial) memcpy(partial, s.h_out + 48, 128);
  if (bad_out) *bad_out = bad;
  return verdict ? EDC_INVALID_SIGNATURE : EDC_OK;
}

// Synchronous batch on slot 0.
static int run_batch_sync(edc_ctx* ctx, size_t n, BatchIn in, uint8_t check8[32], uint8_t partial[128], int* bad) {
  Slot* s = claim_slot0(ctx);
  if (!s) return EDC_ERR_ARG;
  in.compress = check8 != nullptr;
  // a synchronous call is one batch on an otherwise idle GPU: latency-shaped kernels (see
  // launch_msm_bucket); pipelined submissions keep the work-minimal ones
  int rc = enqueue_batch(ctx, *s, n, in, true);
  if (rc) return rc;
  return finish_batch(ctx, *s, check8, partial, bad);
}

// One submission on the claimed slot (null: refused, ctx->err says why), its items on the device:
// the work-minimal pipeline, and the ticket once that is enqueued.
static int64_t submit_batch(edc_ctx* ctx, Slot* s, size_t n, const BatchIn& in) {
  if (!s) return EDC_ERR_ARG;
  const int rc = enqueue_batch(ctx, *s, n, in);
  return rc ? rc : take_ticket(ctx, *s);
}

// ---- synchronous host-buffer calls, copy overlapped with compute ----
// A host-buffer call (the Rust shim's Verifier::verify, src/batch.rs:149) used to copy every input
// over PCIe and only then start the pipeline: at 2^20 prehashed items 134 MB (~2.5 ms at ~53 GB/s)
// + ~1.6 ms of compute. Here the inputs travel in pieces on a copy stream and each piece's work
// starts as it lands: the keys (and message offsets / caller z) first, so the key grouping and the
// keys' decode run under the signature copy; then the signatures (+ k or the message bytes) in
// chunks, each followed by its R decode (second stream) and its SHA-512 + coefficient pass (slot
// stream). A copy from pageable memory returns only when it has landed, so the calling thread
// issues nothing but copies and events, back to back, while a launcher thread enqueues each
// piece's kernels behind its event. The last chunk is small, so that little remains after the
// last byte: its decode and coefficients, the per-key merge, binning, sort and the MSM. Same
// kernels, same per-item / per-key arithmetic and the same integer sums (order-independent), so
// verdict and [8]*check are bit-identical to the one-piece path (tests/test_gpu_hostchunk.py).
constexpr size_t kHostChunkMin = 1u << 16;   // smaller calls copy in one piece (latency-bound anyway)
constexpr int kHostChunks = 8;               // chunks of signatures (ctx->hev: one event each + piece 0)

static bool host_chunked_ok(const edc_ctx* ctx, size_t n) {
  static const bool off = getenv("EDC_HOST_CHUNKS") && getenv("EDC_HOST_CHUNKS")[0] == '0';   // A/B measurement
  return !off && n >= kHostChunkMin && n < (1ull << 28) && !ctx->timing && ctx->slot[0].st2;
}

// chunk boundaries: kHostChunks - 1 equal chunks, then a last one of ~n/32; every boundary but n
// is a multiple of COEF_CHUNK (k_coef's workgroups start on one)
static std::vector<size_t> host_chunks(size_t n) {
  const size_t last = ((n + 31) / 32 + COEF_CHUNK - 1) / COEF_CHUNK * COEF_CHUNK;
  const size_t body = n > last ? (n - last) / COEF_CHUNK * COEF_CHUNK : 0;
  // body chunks of ~2^18 items: every pageable copy costs ~20-25 us of host time before the next
  // can start (r06c/r06d traces), and a 2^18 decode still ends under the next chunk's copy
  static const int env_chunks = getenv("EDC_HOST_BODY_CHUNKS") ? atoi(getenv("EDC_HOST_BODY_CHUNKS")) : 0;
  size_t k = env_chunks > 0 ? (size_t)env_chunks : (body + (1u << 17)) >> 18;
  if (k < 1) k = 1;
  if (k > kHostChunks - 1) k = kHostChunks - 1;
  const size_t c = ((body + k - 1) / k + COEF_CHUNK - 1) / COEF_CHUNK * COEF_CHUNK;
  std::vector<size_t> b{0};
  while (b.back() < body && c) b.push_back(b.back() + c < body ? b.back() + c : body);
  if (b.back() < n) b.push_back(n);
  return b;
}

// pieces landed so far (the copying thread counts up, the launcher thread waits)
struct HostGate {
  std::mutex m;
  std::condition_variable cv;
  int landed = 0;
  bool abort = false;
  void post(int k) {
    { std::lock_guard<std::mutex> g(m); landed = k; }
    cv.notify_all();
  }
  void stop() {
    { std::lock_guard<std::mutex> g(m); abort = true; }
    cv.notify_all();
  }
  bool wait(int k) {            // false: the copying thread gave up
    std::unique_lock<std::mutex> g(m);
    cv.wait(g, [&] { return landed >= k || abort; });
    return landed >= k;
  }
};

// Enqueue the whole chunked batch on slot 0 (inputs in host memory; k: prehashed challenges or
// null for the message path; z: caller-drawn z or null for the seed). The host buffers and
// `rebased` are read by the copies until the slot's wait.
static int enqueue_host_chunked(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                                const uint64_t* msg_off, const uint8_t* k, const uint8_t* z, const uint8_t* z_seed,
                                int want_compress, std::vector<uint64_t>& rebased) {
  Slot& s = ctx->slot[0];
  const size_t mbytes = k ? 0 : (size_t)(msg_off[n] - msg_off[0]);
  int rc = ensure_n(ctx, n);
  if (!rc) rc = ensure_slot(ctx, s, n);
  if (!rc && !k) rc = ensure_msg(ctx, mbytes);
  if (rc) return rc;
  if (!ctx->hcs) {   // all of them or none: a failure part-way leaves the context as it was
    Stream cs1, cs2;
    Event ev1[9], ev2[9];
    CK(cs1.create(hipStreamNonBlocking));
    CK(cs2.create(hipStreamNonBlocking));
    for (Event& e : ev1) CK(e.create(hipEventDisableTiming));
    for (Event& e : ev2) CK(e.create(hipEventDisableTiming));
    ctx->hcs = std::move(cs1);
    ctx->hcs2 = std::move(cs2);
    std::move(ev1, ev1 + 9, ctx->hev);
    std::move(ev2, ev2 + 9, ctx->hev2);
  }
  const bool per_sig = choose_per_sig(ctx, n), split = choose_split(ctx);
  const MsmPlan P = batch_plan(ctx, n, per_sig, split);
  rc = ensure_msm(ctx, s, P, batch_entry_room(P, n, split));
  if (rc) return rc;
  const uint32_t N = (uint32_t)n;
  KeyTable kt;   // drawn here, on the calling thread: the launcher thread only reads it
  if ((rc = key_table(ctx, s, n, per_sig, kt))) return rc;
  uint32_t seed[8];
  seed_words(z_seed, seed);
  hipStream_t st = s.st, st2 = s.st2, cs = ctx->hcs;
  slot_begin(s, s.k, 0, false, per_sig, N);
  const std::vector<size_t> cb = host_chunks(n);
  const int nchunks = (int)cb.size() - 1;
  if (!k && msg_off[0] != 0) {
    rebased.resize(n + 1);
    for (size_t i = 0; i <= n; ++i) rebased[i] = msg_off[i] - msg_off[0];
  }
  const KeyCacheView kc = ctx->kc();

  // the launcher thread: every kernel, each piece's behind that piece's events. Two copying
  // threads: this one (keys / offsets / z, then the signature chunks) and a second one (the k or
  // message chunks) on its own stream, so that one thread's per-copy host work (~20-25 us per
  // pageable copy before its transfer starts) runs while the other's transfer is on the bus
  static const bool one_copier = getenv("EDC_HOST_COPY_THREADS") && getenv("EDC_HOST_COPY_THREADS")[0] == '1';
  HostGate gate, gate2;
  std::string lerr;
  int lrc = 0;
  std::thread launcher([&] {
    auto fail = [&](const char* what, hipError_t e) {
      (void)hipGetLastError();
      lerr = std::string(what) + ": " + hipGetErrorString(e);
      lrc = EDC_ERR_HIP;
    };
#define LK(expr)                                   \
  do {                                             \
    hipError_t e_ = (expr);                        \
    if (e_ != hipSuccess) return fail(#expr, e_);  \
  } while (0)
    LK(hipSetDevice(ctx->device));
    // the resets run under the keys' copy; the grouping waits for it
    const bool front = launch_front(st, s, kt, N, ctx->vk, s.msm.counts, P.nbin(), 0xFFFFFFFFu, [&] {
      if (!gate.wait(1)) return false;
      const hipError_t e = hipStreamWaitEvent(st, ctx->hev[0], 0);
      if (e != hipSuccess) fail("hipStreamWaitEvent(st, ctx->hev[0], 0)", e);
      return e == hipSuccess;
    });
    if (!front) return;
    LK(hipEventRecord(s.ev_keys, st));
    LK(hipStreamWaitEvent(st2, s.ev_keys, 0));
    launch_decompress_range(st2, N, 0, 0, key_lanes(ctx, n, per_sig), ctx->sig, ctx->vk, s.key_rep, per_sig, s.pts,
                            s.itembad + s.cap_n, s.keybad, s.flags, kc, split);
    for (int c = 0; c < nchunks; ++c) {
      const size_t c0 = cb[c], cnt = cb[c + 1] - cb[c];
      if (!gate.wait(c + 2)) return;
      hipEvent_t ev = ctx->hev[c + 1];
      LK(hipStreamWaitEvent(st2, ev, 0));
      launch_decompress_range(st2, N, (uint32_t)c0, (uint32_t)cnt, 0, ctx->sig, ctx->vk, s.key_rep, per_sig, s.pts,
                              s.itembad + s.cap_n, s.keybad, s.flags, kc, split);
      LK(hipStreamWaitEvent(st, ev, 0));
      if (!one_copier) {
        if (!gate2.wait(c + 1)) return;
        LK(hipStreamWaitEvent(st, ctx->hev2[c], 0));
      }
      if (!k)
        launch_challenge(st, (uint32_t)cnt, ctx->vk + c0 * 32, ctx->sig + c0 * 64, ctx->msg, ctx->off + c0,
                         s.k + c0 * 8);
      launch_coef_range(st, N, (uint32_t)c0, (uint32_t)cnt, ctx->sig, s.k, z ? ctx->zexp : nullptr, seed, 0,
                        s.key_index, s.scal, s.key_acc, s.u_acc, s.itembad, s.flags, per_sig, s.coef_part, split);
    }
    LK(hipEventRecord(s.ev_dec, st2));
    launch_coef_finish(st, N, s.key_acc, s.u_acc, s.scal, s.flags, per_sig, s.coef_part, split);
    launch_msm_bin(st, P, batch_terms(P, s, N, split), batch_term_count(N, split), s.msm, s.flags, true);
    launch_msm_sort(st, P, s.msm);
    LK(hipStreamWaitEvent(st, s.ev_dec, 0));
    launch_msm_bucket(st, P, s.msm, s.pts, 0, nullptr, nullptr, true);
    launch_msm_tail(st, P, s.msm, s.flags, want_compress, s.d_out, s.h_out);
    LK(hipGetLastError());
#undef LK
  });

  // the k / message chunks (second copying thread, or this one after each signature chunk)
  auto copy_second = [&](int c, hipStream_t str, hipEvent_t ev, std::string& err) -> int {
    const size_t c0 = cb[c], cnt = cb[c + 1] - cb[c];
    hipError_t e = hipSuccess;
    if (k) {
      e = hipMemcpyAsync(s.k + c0 * 8, k + c0 * 32, cnt * 32, hipMemcpyHostToDevice, str);
    } else {
      const size_t b0 = (size_t)(msg_off[c0] - msg_off[0]), b1 = (size_t)(msg_off[c0 + cnt] - msg_off[0]);
      if (b1 > b0) e = hipMemcpyAsync(ctx->msg + b0, msg + msg_off[c0], b1 - b0, hipMemcpyHostToDevice, str);
    }
    if (e == hipSuccess && ev) e = hipEventRecord(ev, str);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      err = std::string("host chunk copy: ") + hipGetErrorString(e);
      return EDC_ERR_HIP;
    }
    return 0;
  };
  std::string err2;
  int rc2 = 0;
  std::thread copier2;
  if (!one_copier)
    copier2 = std::thread([&] {
      if (hipSetDevice(ctx->device) != hipSuccess) { rc2 = EDC_ERR_HIP; gate2.stop(); return; }
      for (int c = 0; c < nchunks; ++c) {
        if ((rc2 = copy_second(c, ctx->hcs2, ctx->hev2[c], err2))) { gate2.stop(); return; }
        gate2.post(c + 1);
      }
    });
  // this thread: the copies, back to back, one event per piece
  auto copies = [&]() -> int {
    CK(hipMemcpyAsync(ctx->vk, vk, n * 32, hipMemcpyHostToDevice, cs));
    if (!k)
      CK(hipMemcpyAsync(ctx->off, rebased.empty() ? msg_off : rebased.data(), (n + 1) * sizeof(uint64_t),
                        hipMemcpyHostToDevice, cs));
    if (z) CK(hipMemcpyAsync(ctx->zexp, z, n * 16, hipMemcpyHostToDevice, cs));
    CK(hipEventRecord(ctx->hev[0], cs));
    gate.post(1);
    for (int c = 0; c < nchunks; ++c) {
      const size_t c0 = cb[c], cnt = cb[c + 1] - cb[c];
      CK(hipMemcpyAsync(ctx->sig + c0 * 64, sig + c0 * 64, cnt * 64, hipMemcpyHostToDevice, cs));
      if (one_copier) {
        std::string e1;
        if (int r = copy_second(c, cs, nullptr, e1)) { ctx->err = e1; return r; }
      }
      CK(hipEventRecord(ctx->hev[c + 1], cs));
      gate.post(c + 2);
    }
    return 0;
  };
  rc = copies();
  if (rc) { gate.stop(); gate2.stop(); }
  if (copier2.joinable()) copier2.join();
  if (rc2) gate.stop();
  launcher.join();
  if (rc) return rc;
  if (rc2) { ctx->err = err2; return rc2; }
  if (lrc) { ctx->err = lerr; return lrc; }
  s.acc_nbin = P.nbin();
  s.pending = true;
  return 0;
}

// One synchronous batch from host buffers, chunked when it pays (see above), else staged in one
// piece and run by run_batch_sync.
static int run_host_sync(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t* k, const uint8_t* z, const uint8_t* z_seed,
                         uint8_t check8[32]) {
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  if (n && (!vk || !sig || (k ? false : !msg_off))) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (n && !k && msg_off[n] > msg_off[0] && !msg) { ctx->err = "null msg"; return EDC_ERR_ARG; }
  if (!host_chunked_ok(ctx, n)) {
    int rc = init_slot(ctx, s);
    if (rc) return rc;
    if (k && ((rc = ensure_n(ctx, n)) || (rc = ensure_slot(ctx, s, n)))) return rc;
    if ((rc = stage_host(ctx, n, vk, sig, msg, msg_off, k, s.k))) return rc;
    if (z && n) CK(hipMemcpyAsync(ctx->zexp, z, n * 16, hipMemcpyHostToDevice, ctx->st()));
    const BatchIn in{ctx->vk, ctx->sig, k ? nullptr : ctx->msg.get(), k ? nullptr : ctx->off.get(), k ? s.k.get() : nullptr,
                     z ? nullptr : z_seed, 0, z ? ctx->zexp.get() : nullptr, false};
    return run_batch_sync(ctx, n, in, check8, nullptr, nullptr);
  }
  std::vector<uint64_t> rebased;
  const int rc = enqueue_host_chunked(ctx, n, vk, sig, msg, msg_off, k, z, z_seed, check8 != nullptr, rebased);
  if (rc) {     // nothing may still read the staging buffers or the caller's memory
    (void)hipStreamSynchronize(ctx->hcs);
    (void)hipStreamSynchronize(ctx->hcs2);
    (void)hipStreamSynchronize(s.st2);
    (void)hipStreamSynchronize(s.st);
    s.pending = false;
    return rc;
  }
  return finish_batch(ctx, s, check8, nullptr, nullptr);
}

// ---- templated messages (edc_tmpl_*, include/edc.h) ----
// message i = head[tpl[i]] || var[var_off[i] .. var_off[i+1]) || tail[tpl[i]] (Item::from, reference
// src/batch.rs:82-94, hashes exactly these bytes). The set and the items go to the device as they
// are, three kernels (edc_tmpl.hip) build the arena and its 64-bit offsets there, and from then on
// every entry runs the message path's pipeline on that arena. The arena is sized from
// tmpl_arena_bound, so nothing comes back to the host in between.
struct TmplItems {
  const edc_templates* ts;
  const uint16_t* tpl;
  const uint8_t* var;
  const uint32_t* var_off;
};

template <typename T>
static int tmpl_room(edc_ctx* ctx, hipStream_t st, DevBuf<T>& b, size_t need) {
  CK(grow(b, need, item_cap, sync_of(st)));
  return 0;
}

static int tmpl_check(edc_ctx* ctx, const edc_templates* ts, TmplShape* shape) {
  if (!ts || !tmpl_check_set(ts->count, ts->head, ts->head_off, ts->tail, ts->tail_off, shape)) {
    ctx->err = "template set: count 1..65535, monotone offsets, at most 1 MiB of head and tail bytes";
    return EDC_ERR_ARG;
  }
  return 0;
}

// The (checked) set into w's device copy on stream st.
static int tmpl_upload_set(edc_ctx* ctx, TmplWs& w, hipStream_t st, const edc_templates* ts, const TmplShape& sh,
                           TmplView* view) {
  w.check = false;
  if (!w.flag) CK(w.flag.alloc(1));
  if (!w.h_flag) CK(w.h_flag.alloc(1));
  const size_t nof = (size_t)ts->count + 1, set_bytes = 8 * nof + sh.head_bytes + sh.tail_bytes;
  int rc = tmpl_room(ctx, st, w.set, set_bytes + 16);   // k_tmpl_expand copies whole 16-byte rows
  if (rc) return rc;
  uint8_t* head = w.set + 8 * nof;
  CK(hipMemcpyAsync(w.set, ts->head_off, 4 * nof, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(w.set + 4 * nof, ts->tail_off, 4 * nof, hipMemcpyHostToDevice, st));
  if (sh.head_bytes) CK(hipMemcpyAsync(head, ts->head, sh.head_bytes, hipMemcpyHostToDevice, st));
  if (sh.tail_bytes) CK(hipMemcpyAsync(head + sh.head_bytes, ts->tail, sh.tail_bytes, hipMemcpyHostToDevice, st));
  *view = TmplView{reinterpret_cast<const uint32_t*>(w.set.get()), reinterpret_cast<const uint32_t*>(w.set + 4 * nof), head,
                   head + sh.head_bytes, ts->count, sh.head_bytes, (uint32_t)set_bytes};
  return 0;
}

// The three kernels on st: n items (device arrays) -> out (>= tmpl_arena_bound bytes) and off[n + 1].
// keep_flag: the caller cleared w.flag on st itself and a kernel in front of these may have raised it
// (k_tmpl_commit_map_alt).
static int tmpl_expand(edc_ctx* ctx, TmplWs& w, hipStream_t st, const TmplView& view, size_t n, const uint16_t* d_tpl,
                       const uint8_t* d_var, const uint32_t* d_var_off, size_t var_bytes, uint8_t* out, uint64_t* off,
                       bool keep_flag = false) {
  if (!n) return 0;
  int rc = tmpl_room(ctx, st, w.bsum, tmpl_scan_words(n));
  if (rc) return rc;
  if (!keep_flag) CK(hipMemsetAsync(w.flag, 0, sizeof(int), st));
  launch_tmpl_expand(st, (uint32_t)n, view, d_tpl, d_var, d_var_off, var_bytes, w.flag, w.bsum, out, off);
  CK(hipGetLastError());
  return 0;
}

// Host items (already checked) into w's staging area on st, then the expansion into out / off.
static int tmpl_expand_host(edc_ctx* ctx, TmplWs& w, hipStream_t st, const TmplView& view, size_t n, const TmplItems& it,
                            uint8_t* out, uint64_t* off) {
  if (!n) return 0;
  const size_t var_bytes = it.var_off[n], o_tpl = 4 * (n + 1), o_var = (o_tpl + 2 * n + 15) & ~(size_t)15;
  if (var_bytes && !it.var) { ctx->err = "null var"; return EDC_ERR_ARG; }
  int rc = tmpl_room(ctx, st, w.in, o_var + var_bytes);
  if (rc) return rc;
  CK(hipMemcpyAsync(w.in, it.var_off, 4 * (n + 1), hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(w.in + o_tpl, it.tpl, 2 * n, hipMemcpyHostToDevice, st));
  if (var_bytes) CK(hipMemcpyAsync(w.in + o_var, it.var, var_bytes, hipMemcpyHostToDevice, st));
  return tmpl_expand(ctx, w, st, view, n, reinterpret_cast<const uint16_t*>(w.in + o_tpl), w.in + o_var,
                     reinterpret_cast<const uint32_t*>(w.in.get()), var_bytes, out, off);
}

// w's own arena and offsets for n items of a set with shape sh
static int tmpl_arena_room(edc_ctx* ctx, TmplWs& w, hipStream_t st, size_t n, const TmplShape& sh, size_t var_bytes) {
  int rc = tmpl_room(ctx, st, w.arena, tmpl_arena_bound(n, sh, var_bytes));
  if (rc) return rc;
  return tmpl_room(ctx, st, w.off, n + 1);
}

// What every host form checks before anything is launched: the set, the items, the keys.
static int tmpl_check_host(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                           const TmplItems& it, TmplShape* sh) {
  int rc = tmpl_check(ctx, it.ts, sh);
  if (rc) return rc;
  if (n >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  if (!n) return 0;
  if (!vk == !key_idx) { ctx->err = "exactly one of vk and key_idx"; return EDC_ERR_ARG; }
  if (!sig) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (!tmpl_check_items(it.ts->count, n, it.tpl, it.var_off) || (it.var_off[n] && !it.var)) {
    ctx->err = "templated items: template index or hole offsets out of range";
    return EDC_ERR_ARG;
  }
  if (key_idx) {
    uint32_t mx = 0;
    for (size_t i = 0; i < n; ++i) mx = key_idx[i] > mx ? key_idx[i] : mx;
    if (mx >= ctx->kc_reg_m) { ctx->err = "key index outside the registered key list"; return EDC_ERR_ARG; }
  }
  return 0;
}

// A checked host batch into slot s (as upload_slot): keys or key indices, signatures, and the
// messages expanded into the slot's own arena.
static int tmpl_upload_slot(edc_ctx* ctx, Slot& s, size_t n, const uint8_t* vk, const uint32_t* key_idx,
                            const uint8_t* sig, const TmplItems& it, const TmplShape& sh) {
  int rc = ensure_slot_inputs(ctx, s, n, 0);
  if (rc) return rc;
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, s.tw, s.st, it.ts, sh, &view))) return rc;
  if (!n) return 0;
  if ((rc = tmpl_arena_room(ctx, s.tw, s.st, n, sh, it.var_off[n]))) return rc;
  if ((rc = stage_keys_sigs(ctx, s.st, n, vk, key_idx, sig, s.in_idx, s.in_vk, s.in_sig))) return rc;
  return tmpl_expand_host(ctx, s.tw, s.st, view, n, it, s.tw.arena, s.tw.off);
}

// What the device forms check on the host; the items themselves are checked by k_tmpl_len.
static int tmpl_check_device(edc_ctx* ctx, size_t n, const edc_templates* ts, const uint16_t* d_tpl, const uint8_t* d_var,
                             const uint32_t* d_var_off, size_t var_bytes, TmplShape* sh) {
  int rc = tmpl_check(ctx, ts, sh);
  if (rc) return rc;
  if (n >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  if (var_bytes > 0xFFFFFFFFull) { ctx->err = "var arena must be below 4 GiB"; return EDC_ERR_ARG; }
  if (n && (!d_tpl || !d_var_off || (var_bytes && !d_var))) { ctx->err = "null input"; return EDC_ERR_ARG; }
  return 0;
}

extern "C" {

int edc_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return EDC_ERR_HIP;
  return c;
}

edc_ctx* edc_create(int device) {
  edc_ctx* ctx = new edc_ctx();
  ctx->device = device;
  {
    std::random_device rd;   // OS randomness: the key-grouping hash secret of this context
    ctx->secret = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    const uint64_t ks = splitmix64(ctx->secret ^ 0x6B657963616368ull);   // key-cache table hash key
    ctx->kc_s0 = (uint32_t)ks;
    ctx->kc_s1 = (uint32_t)(ks >> 32);
    ctx->sc_k0 = splitmix64(ctx->secret ^ 0x7369676361636830ull);        // verified-signature table hash key
    ctx->sc_k1 = splitmix64(ctx->secret ^ 0x7369676361636831ull);
  }
  (void)hipGetLastError();   // launch checks below must not see an earlier, unrelated failure
  bool ok = hipSetDevice(device) == hipSuccess && msm_init_device() == hipSuccess && valhash_init_device() == hipSuccess &&
            init_slot(ctx, ctx->slot[0]) == 0 &&
            ctx->btab.alloc(BTAB_TOTAL * NIELS_WORDS) == hipSuccess;
  if (ok) {
    launch_init_btable(ctx->st(), ctx->btab);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->st()) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    edc_destroy(ctx);
    (void)hipGetLastError();
    return nullptr;
  }
  return ctx;
}

// the powers of the registered list (edc_valset_set_powers)
static void free_valset(edc_ctx* ctx) {
  reset_all(ctx->vs_power, ctx->vs_member, ctx->vs_pos);
  ctx->vs_count = ctx->vs_m = 0;
  ctx->vs_posh.clear();
}

// the history of the registered list (edc_vhist_set)
static void free_vhist(edc_ctx* ctx) {
  reset_all(ctx->vh_off, ctx->vh_ver, ctx->vh_pow);
  ctx->vh_count = 0;
  ctx->vh = VHist();
  ctx->vh_posh.clear();
  reset_all(ctx->vx_rank, ctx->vx_by_rank);     // the address order goes where the history goes
  ctx->vx_ranked = false;
}

static void free_keycache(edc_ctx* ctx) {
  reset_all(ctx->kc_table, ctx->kc_keys, ctx->kc_comb, ctx->kc_ok, ctx->kc_reg);
  ctx->kc_reg_m = 0;
  ctx->kc_regh.clear();
  free_valset(ctx);             // the powers and the history belong to the list
  free_vhist(ctx);
  ctx->kc_m = ctx->kc_tmask = ctx->kc_cap = 0;
  ctx->kc_gen++;
  ctx->kc_words.clear();
  ctx->kc_okh.clear();
}

static int sync_all(edc_ctx* ctx) {
  for (Slot& s : ctx->slot)
    if (s.st) CK(hipStreamSynchronize(s.st));
  for (edc_verifier* v : ctx->verifiers) {
    if (v->cs) CK(hipStreamSynchronize(v->cs));
    if (v->s.st) CK(hipStreamSynchronize(v->s.st));
  }
  return 0;
}

void edc_destroy(edc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // every stream that can still touch the context's memory, then the members free themselves
  (void)sync_all(ctx);
  for (hipStream_t st : {(hipStream_t)ctx->comb.st, (hipStream_t)ctx->hcs, (hipStream_t)ctx->hcs2})
    if (st) (void)hipStreamSynchronize(st);
  delete ctx;
}

const char* edc_last_error(const edc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int edc_batch_verify(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                     const uint64_t* msg_off, const uint8_t z_seed[32], uint8_t check8[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return run_host_sync(ctx, n, vk, sig, msg, msg_off, nullptr, nullptr, z_seed, check8);
}

int edc_batch_verify_z(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                       const uint64_t* msg_off, const uint8_t* z, uint8_t check8[32]) {
  if (!ctx || (n && !z)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return run_host_sync(ctx, n, vk, sig, msg, msg_off, nullptr, n ? z : nullptr, nullptr, check8);
}

int edc_batch_verify_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                            const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                            uint64_t z_base, const uint8_t* d_z, uint8_t check8[32]) {
  if (!ctx || (!z_seed && !d_z)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return run_batch_sync(ctx, n, BatchIn{d_vk, d_sig, d_msg, d_msg_off, nullptr, z_seed, z_base, d_z, false},
                        check8, nullptr, nullptr);
}

int64_t edc_batch_submit_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                                uint64_t z_base, const uint8_t* d_z, int want_check8) {
  if (!ctx || (!z_seed && !d_z)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  Slot* s = claim_next_slot(ctx);
#ifdef EDC_BATCH_STAMPS
  if (s) s->t_submit_us = host_us();
#endif
  return submit_batch(ctx, s, n, BatchIn{d_vk, d_sig, d_msg, d_msg_off, nullptr, z_seed, z_base, d_z, want_check8 != 0});
}

// the host submissions: the items are staged by upload_slot, z is drawn from the seed
static int64_t submit_host(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                           const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k, const uint8_t* z_seed,
                           uint64_t z_base, int want_check8) {
  Slot* s = claim_next_slot(ctx);
  if (!s) return EDC_ERR_ARG;
  BatchIn in{nullptr, nullptr, nullptr, nullptr, nullptr, z_seed, z_base, nullptr, want_check8 != 0};
  const int rc = upload_slot(ctx, *s, n, vk, key_idx, sig, msg, msg_off, k, in);
  return rc ? rc : submit_batch(ctx, s, n, in);
}

int64_t edc_batch_submit(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t z_seed[32], uint64_t z_base, int want_check8) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return submit_host(ctx, n, vk, nullptr, sig, msg, msg_off, nullptr, z_seed, z_base, want_check8);
}

int64_t edc_batch_submit_indexed(edc_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sig,
                                 const uint8_t* msg, const uint64_t* msg_off, const uint8_t z_seed[32],
                                 uint64_t z_base, int want_check8) {
  if (!ctx || !z_seed || (n && !key_idx)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if (check_key_idx(ctx, n, key_idx)) return EDC_ERR_ARG;    // before the claim: a refused call takes no ticket
  return submit_host(ctx, n, nullptr, key_idx, sig, msg, msg_off, nullptr, z_seed, z_base, want_check8);
}

int edc_batch_wait(edc_ctx* ctx, int64_t ticket, uint8_t check8[32], uint8_t partial[128], int* bad) {
  if (!ctx || ticket < 0) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  Slot& s = ctx->slot[ticket % ctx->nslots];
  if (!s.pending || s.ticket != ticket) { ctx->err = "unknown or already-waited ticket"; return EDC_ERR_ARG; }
  return finish_batch(ctx, s, check8, partial, bad);
}

int64_t edc_batch_submit_multi_device(edc_ctx* ctx, size_t nb, size_t n_per, const uint8_t* d_vk, const uint8_t* d_sig,
                                      const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                      const uint8_t z_seed[32], uint64_t z_base, int want_check8) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  Slot* sp = claim_next_slot(ctx);
  if (!sp) return EDC_ERR_ARG;
  Slot& s = *sp;
  const uint32_t nbv = (uint32_t)(nb <= kMultiMax ? nb : 0);
  const uint32_t* dk = reinterpret_cast<const uint32_t*>(d_k);
  int rc;
  if (ctx->multi_union) {        // one batch over all items first (finish_multi)
    rc = multi_args(ctx, nbv, n_per, d_vk, d_sig, d_msg, d_msg_off, dk);
    if (!rc)
      rc = enqueue_batch(ctx, s, (size_t)nbv * n_per, BatchIn{d_vk, d_sig, d_msg, d_msg_off, dk, z_seed, z_base, nullptr, false});
    if (rc) return rc;
    s.nmulti = nbv;
    s.mu_union = true;
    s.mu_nper = n_per;
    s.mu_vk = d_vk;
    s.mu_sig = d_sig;
    s.mu_msg = d_msg;
    s.mu_off = d_msg_off;
    s.mu_k = dk;
    memcpy(s.mu_seed, z_seed, 32);
    s.mu_zbase = z_base;
    s.mu_compress = want_check8 != 0;
  } else {
    rc = enqueue_multi(ctx, s, nbv, n_per, d_vk, d_sig, d_msg, d_msg_off, dk, z_seed, z_base, want_check8 != 0);
    if (rc) return rc;
    s.mu_union = false;
  }
  return take_ticket(ctx, s);
}

int edc_batch_wait_multi(edc_ctx* ctx, int64_t ticket, size_t nb, int* verdicts, uint8_t* check8, uint8_t* partials,
                         int* bad) {
  if (!ctx || ticket < 0) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  Slot& s = ctx->slot[ticket % ctx->nslots];
  if (!s.pending || s.ticket != ticket) { ctx->err = "unknown or already-waited ticket"; return EDC_ERR_ARG; }
  return finish_multi(ctx, s, nb, verdicts, check8, partials, bad);
}

int edc_set_multi_union(edc_ctx* ctx, int on) {
  if (!ctx) return EDC_ERR_ARG;
  ctx->multi_union = on ? 1 : 0;
  return 0;
}

int edc_multi_union_stats(const edc_ctx* ctx, uint64_t* passed, uint64_t* rerun) {
  if (!ctx) return EDC_ERR_ARG;
  if (passed) *passed = ctx->mu_hits;
  if (rerun) *rerun = ctx->mu_reruns;
  return 0;
}

int edc_batch_partial_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                             const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                             uint64_t z_base, const uint8_t* d_z, uint8_t partial[128], int* bad) {
  if (!ctx || !partial || (!z_seed && !d_z)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = run_batch_sync(ctx, n, BatchIn{d_vk, d_sig, d_msg, d_msg_off, nullptr, z_seed, z_base, d_z, false}, nullptr,
                          partial, bad);
  return rc < 0 ? rc : 0;
}

// sum of g canonical partial points on the combine stream -> verdict of [8]*sum == 0 (with the
// bad flag), optional compressed check8 and canonical sum
static int combine_points(edc_ctx* ctx, size_t g, const uint8_t* partials, int bad, uint8_t check8[32],
                          uint8_t sum[128]) {
  Slot& s = ctx->comb;
  int rc = init_slot(ctx, s);
  if (rc) return rc;
  if (g * 128 > ctx->comb_in.cap())
    CK(grow(ctx->comb_in, g * 128, [](size_t b) { return b + 1024; }, sync_of(s.st)));
  if (g) CK(hipMemcpyAsync(ctx->comb_in, partials, g * 128, hipMemcpyHostToDevice, s.st));
  CK(hipMemsetAsync(s.d_out, 0, 256, s.st));
  launch_combine(s.st, (uint32_t)g, ctx->comb_in, bad ? 1 : 0, check8 != nullptr, s.d_out);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(s.h_out, s.d_out, 256, hipMemcpyDeviceToHost, s.st));
  s.pending = true;
  s.timed = false;
  return finish_batch(ctx, s, check8, sum, nullptr);
}

int edc_combine_partials(edc_ctx* ctx, size_t g, const uint8_t* partials, int bad_any, uint8_t check8[32]) {
  if (!ctx || (g && !partials)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return combine_points(ctx, g, partials, bad_any, check8, nullptr);
}

int edc_debug_live_allocs(uint64_t out[2]) {
  if (!out) return EDC_ERR_ARG;
  out[0] = HipAlloc::live_dev.load();
  out[1] = HipAlloc::live_host.load();
  return 0;
}

int edc_debug_sc_reduce_wide(edc_ctx* ctx, size_t n, const uint8_t* d_in, uint8_t* d_out) {
  if (!ctx || (n && (!d_in || !d_out)) || n > (1u << 24)) return EDC_ERR_ARG;
  if (n && (!aligned16(d_in) || !aligned16(d_out))) {
    ctx->err = "device buffers must be 16-byte aligned";
    return EDC_ERR_ARG;
  }
  CK(hipSetDevice(ctx->device));
  Slot& s = ctx->slot[0];
  launch_sc_reduce_wide(s.st, (uint32_t)n, reinterpret_cast<const uint32_t*>(d_in), reinterpret_cast<uint32_t*>(d_out));
  CK(hipGetLastError());
  CK(hipStreamSynchronize(s.st));
  return 0;
}

int edc_combine_records_device(edc_ctx* ctx, void* stream, size_t g, const uint8_t* d_records, size_t stride,
                               uint8_t* d_out) {
  if (!ctx || !d_out || (g && !d_records) || stride < 129 || g > 4096) return EDC_ERR_ARG;
  if (!aligned16(d_out)) { ctx->err = "d_out must be 16-byte aligned"; return EDC_ERR_ARG; }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (st) {     // the caller's stream must belong to the context's GPU
    int sdev = -1;
    CK(hipStreamGetDevice(st, &sdev));
    if (sdev != ctx->device) { ctx->err = "stream is not on the context's device"; return EDC_ERR_ARG; }
  }
  // the launch needs the context's device current; the caller's current device is restored
  int prev = -1;
  CK(hipGetDevice(&prev));
  CK(hipSetDevice(ctx->device));
  launch_combine_records(st, (uint32_t)g, d_records, (uint32_t)stride, d_out);
  const hipError_t e = hipGetLastError();
  (void)hipSetDevice(prev);
  CK(e);
  return 0;
}

int edc_challenge(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                  const uint64_t* msg_off, uint8_t* k_out) {
  if (!ctx || (n && !k_out)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = stage_host(ctx, n, vk, sig, msg, msg_off);
  if (rc) return rc;
  if (!n) return 0;
  launch_challenge(ctx->st(), (uint32_t)n, ctx->vk, ctx->sig, ctx->msg, ctx->off, ctx->kbuf);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(k_out, ctx->kbuf, n * 32, hipMemcpyDeviceToHost, ctx->st()));
  CK(hipStreamSynchronize(ctx->st()));
  return 0;
}

int edc_tmpl_expand_device(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint16_t* d_tpl, const uint8_t* d_var,
                           const uint32_t* d_var_off, size_t var_bytes, uint8_t* d_msg_out, size_t msg_cap,
                           uint64_t* d_msg_off_out) {
  if (!ctx) return EDC_ERR_ARG;
  TmplShape sh;
  int rc = tmpl_check_device(ctx, n, ts, d_tpl, d_var, d_var_off, var_bytes, &sh);
  if (rc) return rc;
  if (!d_msg_off_out || (n && !d_msg_out)) { ctx->err = "null output"; return EDC_ERR_ARG; }
  if (n && msg_cap < tmpl_arena_bound(n, sh, var_bytes)) {
    ctx->err = "msg_cap below n (max head + max tail) + var_bytes + 16";
    return EDC_ERR_ARG;
  }
  if (n && !aligned16(d_msg_out)) { ctx->err = "the message arena must be 16-byte aligned"; return EDC_ERR_ARG; }
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  CK(hipSetDevice(ctx->device));
  if ((rc = init_slot(ctx, s))) return rc;
  if (!n) {
    CK(hipMemsetAsync(d_msg_off_out, 0, sizeof(uint64_t), s.st));
    CK(hipStreamSynchronize(s.st));
    return 0;
  }
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, s.tw, s.st, ts, sh, &view))) return rc;
  if ((rc = tmpl_expand(ctx, s.tw, s.st, view, n, d_tpl, d_var, d_var_off, var_bytes, d_msg_out, d_msg_off_out)))
    return rc;
  CK(hipMemcpyAsync(s.tw.h_flag, s.tw.flag, sizeof(int), hipMemcpyDeviceToHost, s.st));
  CK(hipStreamSynchronize(s.st));
  if (*s.tw.h_flag) { ctx->err = "templated items: template index or hole offsets out of range"; return EDC_ERR_ARG; }
  return 0;
}

int edc_tmpl_challenge(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* vk, const uint8_t* sig,
                       const uint16_t* tpl, const uint8_t* var, const uint32_t* var_off, uint8_t* k_out) {
  if (!ctx || (n && !k_out)) return EDC_ERR_ARG;
  const TmplItems it{ts, tpl, var, var_off};
  TmplShape sh;
  int rc = tmpl_check_host(ctx, n, vk, nullptr, sig, it, &sh);
  if (rc) return rc;
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  CK(hipSetDevice(ctx->device));
  if ((rc = init_slot(ctx, s)) || (rc = ensure_n(ctx, n))) return rc;
  if (!n) return 0;
  hipStream_t st = s.st;
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, s.tw, st, ts, sh, &view)) || (rc = tmpl_arena_room(ctx, s.tw, st, n, sh, var_off[n])))
    return rc;
  CK(hipMemcpyAsync(ctx->vk, vk, n * 32, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(ctx->sig, sig, n * 64, hipMemcpyHostToDevice, st));
  if ((rc = tmpl_expand_host(ctx, s.tw, st, view, n, it, s.tw.arena, s.tw.off))) return rc;
  launch_challenge(st, (uint32_t)n, ctx->vk, ctx->sig, s.tw.arena, s.tw.off, ctx->kbuf);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(k_out, ctx->kbuf, n * 32, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return 0;
}

// edc_tmpl_batch_verify (sync: slot 0, latency-shaped kernels, waits into check8) and
// edc_tmpl_batch_submit (the next ticket's slot, returns the ticket)
static int64_t tmpl_batch_run(edc_ctx* ctx, bool sync, const edc_templates* ts, size_t n, const uint8_t* vk,
                              const uint32_t* key_idx, const uint8_t* sig, const uint16_t* tpl, const uint8_t* var,
                              const uint32_t* var_off, const uint8_t* z_seed, uint64_t z_base, bool compress,
                              uint8_t* check8) {
  const TmplItems it{ts, tpl, var, var_off};
  TmplShape sh;
  int rc = tmpl_check_host(ctx, n, vk, key_idx, sig, it, &sh);
  if (rc) return rc;
  Slot* s = sync ? claim_slot0(ctx) : claim_next_slot(ctx);
  if (!s) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if ((rc = tmpl_upload_slot(ctx, *s, n, vk, key_idx, sig, it, sh))) return rc;
  const BatchIn in{s->in_vk, s->in_sig, s->tw.arena, s->tw.off, nullptr, z_seed, z_base, nullptr, compress};
  if (!sync) return submit_batch(ctx, s, n, in);
  if ((rc = enqueue_batch(ctx, *s, n, in, true))) return rc;
  return finish_batch(ctx, *s, check8, nullptr, nullptr);
}

int edc_tmpl_batch_verify(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* vk, const uint32_t* key_idx,
                          const uint8_t* sig, const uint16_t* tpl, const uint8_t* var, const uint32_t* var_off,
                          const uint8_t z_seed[32], uint8_t check8[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return (int)tmpl_batch_run(ctx, true, ts, n, vk, key_idx, sig, tpl, var, var_off, z_seed, 0, check8 != nullptr, check8);
}

int edc_tmpl_batch_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* d_vk,
                                 const uint8_t* d_sig, const uint16_t* d_tpl, const uint8_t* d_var,
                                 const uint32_t* d_var_off, size_t var_bytes, const uint8_t z_seed[32], uint64_t z_base,
                                 const uint8_t* d_z, uint8_t check8[32]) {
  if (!ctx || (!z_seed && !d_z)) return EDC_ERR_ARG;
  TmplShape sh;
  int rc = tmpl_check_device(ctx, n, ts, d_tpl, d_var, d_var_off, var_bytes, &sh);
  if (rc) return rc;
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  CK(hipSetDevice(ctx->device));
  if ((rc = init_slot(ctx, s))) return rc;
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, s.tw, s.st, ts, sh, &view))) return rc;
  if (n) {
    if ((rc = tmpl_arena_room(ctx, s.tw, s.st, n, sh, var_bytes)) ||
        (rc = tmpl_expand(ctx, s.tw, s.st, view, n, d_tpl, d_var, d_var_off, var_bytes, s.tw.arena, s.tw.off)))
      return rc;
    // the flag travels behind the expansion; the wait reads it before it believes the verdict
    CK(hipMemcpyAsync(s.tw.h_flag, s.tw.flag, sizeof(int), hipMemcpyDeviceToHost, s.st));
    s.tw.check = true;
  }
  rc = run_batch_sync(ctx, n, BatchIn{d_vk, d_sig, s.tw.arena, s.tw.off, nullptr, z_seed, z_base, d_z, false},
                      check8, nullptr, nullptr);
  s.tw.check = false;           // also when the batch never reached its wait
  return rc;
}

int64_t edc_tmpl_batch_submit(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* vk, const uint32_t* key_idx,
                              const uint8_t* sig, const uint16_t* tpl, const uint8_t* var, const uint32_t* var_off,
                              const uint8_t z_seed[32], uint64_t z_base, int want_check8) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return tmpl_batch_run(ctx, false, ts, n, vk, key_idx, sig, tpl, var, var_off, z_seed, z_base, want_check8 != 0, nullptr);
}

// The per-item pass over n device items on stream st, the caller having made ensure_n's room:
// Item::from's challenges into ctx->kbuf where the items come with messages (d_k null), then
// Item::verify_single (src/batch.rs:104-107) with one quad of lanes per item (quad: the caller's
// choice, for lists of at most kQuadVerifyMax items, whose pass is latency-bound) or one lane per
// item, the codes into d_codes; h_codes given: copied there and waited for.
static int verify_items(edc_ctx* ctx, hipStream_t st, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                        const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_k, bool quad, uint8_t* d_codes,
                        uint8_t* h_codes) {
  if (!d_k) {
    launch_challenge(st, (uint32_t)n, d_vk, d_sig, d_msg, d_off, ctx->kbuf);
    d_k = ctx->kbuf;
  }
  if (quad)
    launch_verify_quad(st, (uint32_t)n, d_vk, d_sig, d_k, ctx->btab, d_codes, ctx->kc(), ctx->bcomb);
  else
    launch_verify_single(st, (uint32_t)n, d_vk, d_sig, d_k, ctx->btab, ctx->vtab, d_codes, ctx->kc(), ctx->bcomb);
  CK(hipGetLastError());
  if (!h_codes) return 0;
  CK(hipMemcpyAsync(h_codes, d_codes, n, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return 0;
}

// The three entries below take one lane per item at every n.
int edc_verify_prehashed_each(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* k,
                              uint8_t* verdicts) {
  if (!ctx || (n && (!vk || !sig || !k || !verdicts))) return EDC_ERR_ARG;
  if (k_all_canonical(ctx, n, k)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = ensure_n(ctx, n);
  if (rc || !n) return rc;
  if ((rc = stage_host(ctx, n, vk, sig, nullptr, nullptr, k, ctx->kbuf))) return rc;
  return verify_items(ctx, ctx->st(), n, ctx->vk, ctx->sig, nullptr, nullptr, ctx->kbuf, false, ctx->verdicts, verdicts);
}

int edc_verify_each(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                    const uint64_t* msg_off, uint8_t* verdicts) {
  if (!ctx || (n && !verdicts)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = stage_host(ctx, n, vk, sig, msg, msg_off);
  if (rc || !n) return rc;
  return verify_items(ctx, ctx->st(), n, ctx->vk, ctx->sig, ctx->msg, ctx->off, nullptr, false, ctx->verdicts, verdicts);
}

int edc_verify_each_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_msg,
                           const uint64_t* d_msg_off, uint8_t* d_verdicts) {
  if (!ctx || (n && (!d_vk || !d_sig || !d_msg_off || !d_verdicts))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = ensure_n(ctx, n);
  if (rc || !n) return rc;
  if ((rc = verify_items(ctx, ctx->st(), n, d_vk, d_sig, d_msg, d_msg_off, nullptr, false, d_verdicts, nullptr))) return rc;
  CK(hipStreamSynchronize(ctx->st()));
  return 0;
}

// ---- grouped fallback: one MSM pass over ~128 contiguous ranges (edc_set_fallback_shape) ----
static int ensure_fb(edc_ctx* ctx, size_t terms, size_t ranges) {
  CK(grow_group(ctx->fb_cap_terms, terms, term_cap, sync_of(ctx->st()), [&](size_t cap) {
    return alloc_all(sized(ctx->fb_xpt, cap), sized(ctx->fb_xrg, cap), sized(ctx->fb_xscal, cap * 8));
  }));
  CK(grow(ctx->fb_rv, 2 * ranges + 64, exact_cap, sync_of(ctx->st())));
  return 0;
}

// Item::verify_single (src/batch.rs:104-107) for the listed items, with the batch's queue-time k
// (slot s): gathered into the staging buffers, one per-item launch, codes scattered into verdicts.
static int verify_listed(edc_ctx* ctx, Slot& s, const std::vector<uint32_t>& idx, const uint8_t* d_vk,
                         const uint8_t* d_sig, uint8_t* verdicts, int* invalid) {
  const size_t c = idx.size();
  if (!c) return 0;
  int rc = ensure_n(ctx, c);
  if (rc) return rc;
  // gathered copies in their own buffer: the inputs may BE the context's staging buffers (host
  // entry points), and an in-place gather would race (item idx[j] > j is read while slot idx[j]
  // is written by another lane)
  CK(grow_group(ctx->fb_cap_g, c, term_cap, sync_of(s.st), [&](size_t cap) {
    return alloc_all(sized(ctx->fb_idx, cap), sized(ctx->fb_g, cap * 128));
  }));
  uint8_t* g_vk = ctx->fb_g;
  uint8_t* g_sig = g_vk + ctx->fb_cap_g * 32;
  uint32_t* g_k = reinterpret_cast<uint32_t*>(g_sig + ctx->fb_cap_g * 64);
  hipStream_t st = s.st;
  CK(hipMemcpyAsync(ctx->fb_idx, idx.data(), c * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  launch_gather_items(st, (uint32_t)c, ctx->fb_idx, d_vk, d_sig, s.kin, g_vk, g_sig, g_k);
  std::vector<uint8_t> v(c);
  if ((rc = verify_items(ctx, st, c, g_vk, g_sig, nullptr, nullptr, g_k, c <= kQuadVerifyMax, ctx->verdicts, v.data())))
    return rc;
  for (size_t j = 0; j < c; ++j) {
    verdicts[idx[j]] = v[j];
    *invalid += v[j] != 0;
  }
  return 0;
}

// How the grouped fallback cuts n items into ranges.
struct FallbackGeometry {
  size_t rsize;      // items per range, a multiple of COEF_CHUNK (k_coef's workgroups start on one)
  uint32_t G, bpr;   // ranges (none of n = 0 items); MSM bins per range
};

// ~fb_ranges ranges: each range-window bin then holds enough digits to amortize its fixed
// 256-bucket reduction, and a failing range costs no more than a small one in the per-item pass.
// The range count is capped so that the range-tagged plan fits MSM_MAX_BINS (G * bins per range).
static FallbackGeometry fallback_geometry(const edc_ctx* ctx, size_t n) {
  const uint32_t bpr = make_plan(ctx->fb_bits, ctx->fb_bits, 1).bins_per_range;
  if (!n) return FallbackGeometry{0, 0, bpr};
  const uint32_t gmax = MSM_MAX_BINS / bpr;
  const uint32_t granges = ctx->fb_ranges < gmax ? ctx->fb_ranges : gmax;
  const size_t target = (n + granges - 1) / granges;
  const size_t rsize = (target + COEF_CHUNK - 1) / COEF_CHUNK * COEF_CHUNK;
  return FallbackGeometry{rsize, (uint32_t)((n + rsize - 1) / rsize), bpr};
}

// After a failed batch on slot s (its k, decoded points, key grouping and per-item failure bits
// still in place): the batch equation restricted to ~fb_ranges (default 128) contiguous ranges in
// ONE MSM pass (range-tagged bins, fb_bits = 9-bit windows by default), [8]P_g == 0 per range;
// ranges whose check fails or that hold an item with an undecodable R / key or a non-canonical s
// are verified item by item. Items of passing ranges are valid (ZIP215: batch == single, with a
// fresh secret z: see include/edc.h). verdicts (host, n bytes) receive Item::verify_single's code
// for every item. in: the failed batch's items and z seed / base (its k is s.kin; d_z is not read,
// the fallback draws its z from the seed). redid (nullable): whether the prefix was redone on s,
// which overwrites the grouped key state a caller may keep there.
static int fallback_ranges(edc_ctx* ctx, Slot& s, size_t n, const BatchIn& in, bool per_sig, uint32_t m, uint8_t* verdicts,
                           bool* redid = nullptr) {
  const uint8_t *d_vk = in.vk, *d_sig = in.sig, *z_seed = in.z_seed;
  const uint64_t z_base = in.z_base;
  if (redid) *redid = false;
  memset(verdicts, 0, n);
  if (!n) return 0;
  const FallbackGeometry geo = fallback_geometry(ctx, n);
  const size_t rsize = geo.rsize;
  const uint32_t G = geo.G;
  if (!per_sig && (size_t)G * m > s.cap_n) {
    // too many distinct keys for per-(range, key) sums: redo the prefix with one key term per
    // signature (the same group element)
    // (s.kin already holds this batch's k: computed by the first prefix or the caller's)
    if (redid) *redid = true;
    BatchIn again = in;
    again.k = s.kin;
    again.d_z = nullptr;
    int rc = enqueue_prefix(ctx, s, n, again, nullptr, true, false);
    if (rc) return rc;
    CK(hipStreamSynchronize(s.st));
    per_sig = true;
  }
  const MsmPlan P = make_plan(ctx->fb_bits, ctx->fb_bits, G);
  const uint32_t mm = per_sig ? 0u : m;
  const size_t nx = (size_t)G * (mm + 1);
  const uint32_t npoint = (uint32_t)(per_sig ? 2 * n : n);
  int rc = ensure_msm(ctx, s, P, msm_entry_capacity(P, n, (per_sig ? n : 0) + nx));
  if (rc) return rc;
  rc = ensure_fb(ctx, nx, G);
  if (rc) return rc;
  uint32_t seed[8];
  seed_words(z_seed, seed);
  hipStream_t st = s.st;
  launch_range_coef(st, (uint32_t)n, (uint32_t)rsize, G, m, per_sig, d_sig, s.kin, nullptr, seed, z_base, s.key_index,
                    s.scal, s.key_acc, s.u_acc, s.flags, ctx->fb_xpt, ctx->fb_xrg, ctx->fb_xscal);
  const MsmTerms terms{(uint32_t)n, (uint32_t)rsize, npoint, (uint32_t)nx, 1, s.scal, ctx->fb_xpt, ctx->fb_xrg,
                       ctx->fb_xscal};
  launch_msm_bin(st, P, terms, npoint + (uint32_t)nx, s.msm, s.flags);
  launch_msm_sort(st, P, s.msm);
  launch_msm_bucket(st, P, s.msm, s.pts);
  launch_msm_range_tail(st, P, s.msm, ctx->fb_rv);
  CK(hipMemsetAsync(ctx->fb_rv + G, 0, G, st));
  launch_range_prebad(st, (uint32_t)n, (uint32_t)rsize, s.itembad, s.itembad + s.cap_n, s.keybad, s.key_index, per_sig,
                      ctx->fb_rv + G);
  CK(hipGetLastError());
  std::vector<uint8_t> rv(2 * (size_t)G);
  CK(hipMemcpyAsync(rv.data(), ctx->fb_rv, 2 * (size_t)G, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  std::vector<uint32_t> idx;
  for (uint32_t g = 0; g < G; ++g)
    if (rv[g] || rv[G + g])
      for (size_t i = (size_t)g * rsize; i < n && i < (size_t)(g + 1) * rsize; ++i) idx.push_back((uint32_t)i);
  int invalid = 0;
  rc = verify_listed(ctx, s, idx, d_vk, d_sig, verdicts, &invalid);
  if (rc) return rc;
  return invalid;
}

// grouping state of the batch last enqueued on slot s (after it completed)
static int slot_grouping(edc_ctx* ctx, Slot& s, bool* per_sig, uint32_t* m) {
  int f[FLAG_COUNT];
  CK(hipMemcpy(f, s.flags, sizeof(f), hipMemcpyDeviceToHost));
  *per_sig = s.per_sig || f[FLAG_OVF] != 0;
  *m = (uint32_t)f[FLAG_NKEYS];
  return 0;
}

int edc_find_invalid_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                            const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                            size_t leaf, uint8_t* verdicts) {
  (void)leaf;
  if (!ctx || !z_seed || (n && (!d_vk || !d_sig || !d_msg_off || !verdicts))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  if (!n) return 0;
  const BatchIn in{d_vk, d_sig, d_msg, d_msg_off, nullptr, z_seed, 0, nullptr, false};
  int rc = enqueue_prefix(ctx, s, n, in, nullptr);
  if (rc) return rc;
  CK(hipStreamSynchronize(s.st));
  bool per_sig;
  uint32_t m;
  rc = slot_grouping(ctx, s, &per_sig, &m);
  if (rc) return rc;
  return fallback_ranges(ctx, s, n, in, per_sig, m, verdicts);
}

}  // extern "C"

// batch on slot 0, then (on failure) the grouped fallback reusing its state; z from in.z_seed at base 0
static int batch_with_fallback(edc_ctx* ctx, size_t n, const BatchIn& in, uint8_t* verdicts, int* n_invalid,
                               uint8_t check8[32]) {
  if (n_invalid) *n_invalid = 0;
  int rc = run_batch_sync(ctx, n, in, check8, nullptr, nullptr);
  if (rc <= 0) {
    if (rc == 0 && n) memset(verdicts, 0, n);
    return rc;
  }
  Slot& s = ctx->slot[0];
  bool per_sig;
  uint32_t m;
  int r2 = slot_grouping(ctx, s, &per_sig, &m);
  if (r2) return r2;
  r2 = fallback_ranges(ctx, s, n, in, per_sig, m, verdicts);
  if (r2 < 0) return r2;
  if (n_invalid) *n_invalid = r2;
  return EDC_INVALID_SIGNATURE;
}

// nothing of an empty prehashed batch is read, but its k must not be null (null is the message form)
static const uint8_t kNoItems[1] = {0};

extern "C" {

int edc_batch_verify_fallback_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                     const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                                     uint8_t* verdicts, int* n_invalid, uint8_t check8[32]) {
  if (!ctx || !z_seed || (n && (!d_vk || !d_sig || !d_msg_off || !verdicts))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return batch_with_fallback(ctx, n, BatchIn{d_vk, d_sig, d_msg, d_msg_off, nullptr, z_seed, 0, nullptr, false},
                             verdicts, n_invalid, check8);
}

// ---- prehashed items: the reference's batch::Item {vk_bytes, sig, k} (src/batch.rs:76-94) ----
int edc_batch_verify_prehashed(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* k,
                               const uint8_t z_seed[32], const uint8_t* z, uint8_t check8[32]) {
  if (!ctx || (!z_seed && !z) || (n && (!vk || !sig || !k || (!z_seed && !z)))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if (!n)       // empty batch: Ok through the one-piece path (no input is read)
    return run_host_sync(ctx, 0, kNoItems, kNoItems, nullptr, nullptr, kNoItems, nullptr, z ? nullptr : z_seed, check8);
  return run_host_sync(ctx, n, vk, sig, nullptr, nullptr, k, z, z_seed, check8);
}

int edc_batch_verify_prehashed_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                      const uint8_t* d_k, const uint8_t z_seed[32], uint64_t z_base,
                                      const uint8_t* d_z, uint8_t check8[32]) {
  if (!ctx || (!z_seed && !d_z) || (n && (!d_vk || !d_sig || !d_k))) return EDC_ERR_ARG;
  if (check_aligned16(ctx, "d_k / d_z", {d_k, d_z})) return EDC_ERR_ARG;     // before the device is touched
  CK(hipSetDevice(ctx->device));
  const BatchIn in{d_vk, d_sig, nullptr, nullptr, reinterpret_cast<const uint32_t*>(d_k), z_seed, z_base, d_z, false};
  return run_batch_sync(ctx, n, in, check8, nullptr, nullptr);
}

int64_t edc_batch_submit_prehashed_indexed(edc_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sig,
                                           const uint8_t* k, const uint8_t z_seed[32], uint64_t z_base,
                                           int want_check8) {
  if (!ctx || !z_seed || (n && !key_idx)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if (check_key_idx(ctx, n, key_idx)) return EDC_ERR_ARG;    // before the claim: a refused call takes no ticket
  return submit_host(ctx, n, nullptr, key_idx, sig, nullptr, nullptr, n ? k : kNoItems, z_seed, z_base, want_check8);
}

int64_t edc_batch_submit_prehashed(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* k,
                                   const uint8_t z_seed[32], uint64_t z_base, int want_check8) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return submit_host(ctx, n, vk, nullptr, sig, nullptr, nullptr, n ? k : kNoItems, z_seed, z_base, want_check8);
}

int64_t edc_batch_submit_prehashed_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                          const uint8_t* d_k, const uint8_t z_seed[32], uint64_t z_base,
                                          const uint8_t* d_z, int want_check8) {
  if (!ctx || (!z_seed && !d_z) || (n && (!d_vk || !d_sig || !d_k))) return EDC_ERR_ARG;
  if (check_aligned16(ctx, "d_k / d_z", {d_k, d_z})) return EDC_ERR_ARG;     // before the device is touched
  CK(hipSetDevice(ctx->device));
  return submit_batch(ctx, claim_next_slot(ctx), n, BatchIn{d_vk, d_sig, nullptr, nullptr, reinterpret_cast<const uint32_t*>(d_k),
                                                            z_seed, z_base, d_z, want_check8 != 0});
}

int edc_batch_verify_prehashed_fallback(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                                        const uint8_t* k, const uint8_t z_seed[32], uint8_t* verdicts,
                                        int* n_invalid, uint8_t check8[32]) {
  if (!ctx || !z_seed || (n && (!vk || !sig || !k || !verdicts))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  int rc = ensure_n(ctx, n);
  if (rc || (rc = ensure_slot(ctx, s, n)) || (rc = stage_host(ctx, n, vk, sig, nullptr, nullptr, n ? k : kNoItems, s.k)))
    return rc;
  return batch_with_fallback(ctx, n, BatchIn{ctx->vk, ctx->sig, nullptr, nullptr, s.k, z_seed, 0, nullptr, false},
                             verdicts, n_invalid, check8);
}

int edc_batch_verify_prehashed_fallback_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                               const uint8_t* d_k, const uint8_t z_seed[32], uint8_t* verdicts,
                                               int* n_invalid, uint8_t check8[32]) {
  if (!ctx || !z_seed || (n && (!d_vk || !d_sig || !d_k || !verdicts))) return EDC_ERR_ARG;
  if (check_aligned16(ctx, "d_k", {d_k})) return EDC_ERR_ARG;                // before the device is touched
  CK(hipSetDevice(ctx->device));
  return batch_with_fallback(ctx, n, BatchIn{d_vk, d_sig, nullptr, nullptr, reinterpret_cast<const uint32_t*>(d_k), z_seed, 0,
                                             nullptr, false},
                             verdicts, n_invalid, check8);
}

}  // extern "C"

// ---- commit sets (edc_commits_*, include/edc.h): many variable-size batches in one launch ----
// n items cut into nc commits by nc + 1 host offsets, each commit its own batch::Verifier
// (reference src/batch.rs:110-217, the per-commit flow of tests/batch.rs:18-44). The launch is ONE
// batch over all n items, exactly enqueue_batch: the batch equation is linear, so when the union
// holds every commit holds (finish_multi's union-first argument) and nothing else runs. When it
// fails, the wait runs the grouped fallback on the state the batch left in ITS OWN slot and the
// per-item codes are reduced to per-commit verdicts on the host (commits.h).
//
// The fallback on a slot other than 0, with other tickets in flight. What fallback_ranges and
// verify_listed touch: the slot's own arrays and MSM workspace, on the slot's stream only; the
// context's fb_xpt / fb_xrg / fb_xscal / fb_rv / fb_idx / fb_g, verdicts and vtab, also on that
// stream only; and, read-only, btab, bcomb and the key cache, which cannot change while a ticket
// is pending. Both end in hipStreamSynchronize of the slot's stream, and a context belongs to one
// thread, so there is one fallback at a time and each finds the context's buffers idle: whoever
// used them last has synchronized. Their growth paths (ensure_fb, ensure_n, ensure_msm) free
// buffers no enqueued kernel reads: in-flight tickets only read their own slot's buffers (host
// submissions are staged into in_* / tw of their slot, never into the context's vk / sig / msg).
// The grouping state is read on the slot's stream here (slot_grouping's hipMemcpy would wait for
// every in-flight slot).
static int commits_check(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, size_t* n) {
  if (!commits_check_offsets(nc, commit_off, n)) {
    ctx->err = "commit offsets: commit_off[0] = 0, monotone, fewer than 2^28 items";
    return EDC_ERR_ARG;
  }
  return 0;
}

// keys of a host form: exactly one of vk and key_idx, every index inside the registered list
static int commits_check_keys(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint32_t* key_idx) {
  if (!vk == !key_idx) { ctx->err = "exactly one of vk and key_idx"; return EDC_ERR_ARG; }
  return key_idx ? check_key_idx(ctx, n, key_idx) : 0;
}

// messages of n > 0 host items: (msg, msg_off), or the prehashed k (its values are the caller's to check)
static int commits_check_msg_or_k(edc_ctx* ctx, size_t n, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k) {
  if (!msg_off == !k || (msg && k)) { ctx->err = "exactly one of (msg, msg_off) and k"; return EDC_ERR_ARG; }
  if (msg_off && msg_off[n] < msg_off[0]) { ctx->err = "message offsets decrease"; return EDC_ERR_ARG; }
  if (msg_off && msg_off[n] > msg_off[0] && !msg) { ctx->err = "null msg"; return EDC_ERR_ARG; }
  return 0;
}

// the host checks of edc_commits_verify / _submit (nothing is launched before they pass)
static int commits_check_host(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                              const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                              const uint8_t* k, size_t* n) {
  int rc = commits_check(ctx, nc, commit_off, n);
  if (rc || !*n) return rc;
  if ((rc = commits_check_keys(ctx, *n, vk, key_idx))) return rc;
  if (!sig) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if ((rc = commits_check_msg_or_k(ctx, *n, msg, msg_off, k))) return rc;
  if (k) {
    for (size_t i = 0; i < *n; ++i) {      // Scalar::from_hash never yields k >= l
      uint32_t w[8];
      memcpy(w, k + 32 * i, 32);
      if (w[7] >= 0x10000000u && !sc_is_canonical(w)) {   // below 2^252 is below l
        ctx->err = "prehashed k is not a canonical scalar (must be < l, as Scalar::from_hash returns)";
        return EDC_ERR_ARG;
      }
    }
  }
  return 0;
}

// Template variants: every commit's window [commit_tpl[c], commit_tpl[c] + alt_span) inside the set.
static int commits_check_windows(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint16_t* commit_tpl,
                                 uint32_t alt_span) {
  if (!commits_check_alt_span(ts->count, nc, commit_tpl, alt_span)) {
    ctx->err = "template variants: alt_span in 1..256 and commit_tpl[c] + alt_span <= the set's count for every commit";
    return EDC_ERR_ARG;
  }
  return 0;
}

// The host checks of a templated host form. variants: the caller passed alt_span and item_alt
// (edc_tmpl_commits_*_alt, the templated quorum forms), so the windows and the variant bytes are
// checked too, and alt_span = 0 is refused there, never read as "one template per commit".
static int commits_check_tmpl(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                              const uint16_t* commit_tpl, bool variants, uint32_t alt_span, const uint8_t* item_alt,
                              const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var,
                              const uint32_t* var_off, TmplShape* sh, size_t* n) {
  int rc = tmpl_check(ctx, ts, sh);
  if (rc || (rc = commits_check(ctx, nc, commit_off, n))) return rc;
  if (!commits_check_tpl(ts->count, nc, commit_tpl)) {
    ctx->err = "commit templates: one index below the set's count per commit";
    return EDC_ERR_ARG;
  }
  if (*n) {
    if ((rc = commits_check_keys(ctx, *n, vk, key_idx))) return rc;
    if (!sig) { ctx->err = "null input"; return EDC_ERR_ARG; }
    if (!commits_check_holes(*n, var_off) || (var_off[*n] && !var)) {
      ctx->err = "templated items: hole offsets out of range";
      return EDC_ERR_ARG;
    }
  }
  if (!variants) return 0;
  if ((rc = commits_check_windows(ctx, ts, nc, commit_tpl, alt_span))) return rc;
  if (!commits_check_item_alt(*n, item_alt, alt_span)) {
    ctx->err = "template variants: item_alt[i] < alt_span for every item";
    return EDC_ERR_ARG;
  }
  return 0;
}

// What a templated submit of no commits still checks: the set, and with variants the span's range.
static int commits_check_tmpl_empty(edc_ctx* ctx, const edc_templates* ts, bool variants, uint32_t alt_span,
                                    TmplShape* sh) {
  int rc = tmpl_check(ctx, ts, sh);
  if (rc) return rc;
  if (variants && (alt_span < 1 || alt_span > COMMITS_MAX_ALT_SPAN)) {
    ctx->err = "template variants: alt_span in 1..256";
    return EDC_ERR_ARG;
  }
  return 0;
}

// What the device forms of a templated commit set check on the host: the set, the offsets, the
// windows, the pointers. The holes and the variant bytes are checked on the device.
static int commits_check_tmpl_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                     const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_vk,
                                     const uint8_t* d_sig, const uint8_t* d_var, const uint32_t* d_var_off,
                                     size_t var_bytes, TmplShape* sh, size_t* n) {
  int rc = tmpl_check(ctx, ts, sh);
  if (rc || (rc = commits_check(ctx, nc, commit_off, n)) || (rc = commits_check_windows(ctx, ts, nc, commit_tpl, alt_span)))
    return rc;
  if (var_bytes > 0xFFFFFFFFull) { ctx->err = "var arena must be below 4 GiB"; return EDC_ERR_ARG; }
  if (!*n) return 0;
  if (!d_vk || !d_sig || !d_var_off || (var_bytes && !d_var)) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (!aligned16(d_vk) || !aligned16(d_sig) || ((uintptr_t)d_var_off & 3u)) {
    ctx->err = "device vk / sig arrays must be 16-byte aligned, d_var_off 4-byte aligned";
    return EDC_ERR_ARG;
  }
  return 0;
}

// A checked host commit set into slot s (as upload_slot / upload_slot_prehashed) and the union
// batch behind it on the slot's stream.
static int commits_enqueue(edc_ctx* ctx, Slot& s, size_t nc, const uint32_t* commit_off, size_t n, const uint8_t* d_vk,
                           const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_off, const uint32_t* d_k,
                           const uint8_t* z_seed, bool latency) {
  int rc = enqueue_batch(ctx, s, n, BatchIn{d_vk, d_sig, d_msg, d_off, d_k, z_seed, 0, nullptr, false}, latency);
  if (rc) return rc;
  s.commits = true;
  s.cm_nc = nc;
  s.cm_off = commit_off;
  s.cm_vk = d_vk;
  s.cm_sig = d_sig;
  s.cm_msg = d_msg;
  s.cm_moff = d_off;
  memcpy(s.cm_seed, z_seed, 32);
  return 0;
}

static int commits_enqueue_host(edc_ctx* ctx, Slot& s, size_t nc, const uint32_t* commit_off, size_t n,
                                const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg,
                                const uint64_t* msg_off, const uint8_t* k, const uint8_t* z_seed, bool latency) {
  static const uint64_t no_off[1] = {0};
  BatchIn in{};
  // an empty set takes the message form whatever it was given
  const int rc = upload_slot(ctx, s, n, vk, key_idx, sig, msg, n ? msg_off : no_off, n ? k : nullptr, in);
  if (rc) return rc;
  return commits_enqueue(ctx, s, nc, commit_off, n, in.vk, in.sig, in.msg, in.off, in.k, z_seed, latency);
}

// A checked templated commit set into slot s (as tmpl_upload_slot): the per-item template array
// is made on the device from the commit offsets (k_tmpl_commit_map), then the existing expansion.
// Staging area: var_off | tpl | var | commit_off | commit_tpl | item_alt, each at a 16-byte boundary.
// alt_span = 0: one template per commit. alt_span >= 1: the checked variants (k_tmpl_commit_map_alt;
// item_alt, n bytes, is staged unless it is null).
static int commits_enqueue_tmpl(edc_ctx* ctx, Slot& s, const edc_templates* ts, const TmplShape& sh, size_t nc,
                                const uint32_t* commit_off, const uint16_t* commit_tpl, size_t n, const uint8_t* vk,
                                const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                                const uint8_t* z_seed, bool latency, uint32_t alt_span = 0,
                                const uint8_t* item_alt = nullptr) {
  int rc = ensure_slot_inputs(ctx, s, n, 0);
  if (rc) return rc;
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, s.tw, s.st, ts, sh, &view))) return rc;
  if (n) {
    TmplWs& w = s.tw;
    hipStream_t st = s.st;
    const size_t var_bytes = var_off[n];
    const size_t o_tpl = up16(4 * (n + 1)), o_var = up16(o_tpl + 2 * n), o_coff = up16(o_var + var_bytes),
                 o_ctpl = up16(o_coff + 4 * (nc + 1)), o_alt = up16(o_ctpl + 2 * nc);
    if ((rc = tmpl_arena_room(ctx, w, st, n, sh, var_bytes)) ||
        (rc = tmpl_room(ctx, st, w.in, item_alt ? o_alt + n : o_ctpl + 2 * nc)))
      return rc;
    if ((rc = stage_keys_sigs(ctx, st, n, vk, key_idx, sig, s.in_idx, s.in_vk, s.in_sig))) return rc;
    CK(hipMemcpyAsync(w.in, var_off, 4 * (n + 1), hipMemcpyHostToDevice, st));
    if (var_bytes) CK(hipMemcpyAsync(w.in + o_var, var, var_bytes, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(w.in + o_coff, commit_off, 4 * (nc + 1), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(w.in + o_ctpl, commit_tpl, 2 * nc, hipMemcpyHostToDevice, st));
    uint16_t* d_tpl = reinterpret_cast<uint16_t*>(w.in + o_tpl);
    if (alt_span) {
      if (item_alt) CK(hipMemcpyAsync(w.in + o_alt, item_alt, n, hipMemcpyHostToDevice, st));
      // the host has checked every byte, so the kernel never raises the flag here: tmpl_expand clears it as always
      launch_tmpl_commit_map_alt(st, (uint32_t)n, (uint32_t)nc, reinterpret_cast<const uint32_t*>(w.in + o_coff),
                                 reinterpret_cast<const uint16_t*>(w.in + o_ctpl), alt_span,
                                 item_alt ? w.in + o_alt : nullptr, d_tpl, w.flag);
    } else {
      launch_tmpl_commit_map(st, (uint32_t)n, (uint32_t)nc, reinterpret_cast<const uint32_t*>(w.in + o_coff),
                             reinterpret_cast<const uint16_t*>(w.in + o_ctpl), d_tpl);
    }
    CK(hipGetLastError());
    if ((rc = tmpl_expand(ctx, w, st, view, n, d_tpl, w.in + o_var, reinterpret_cast<const uint32_t*>(w.in.get()), var_bytes,
                          w.arena, w.off)))
      return rc;
  }
  return commits_enqueue(ctx, s, nc, commit_off, n, s.in_vk, s.in_sig, s.tw.arena, s.tw.off, nullptr, z_seed, latency);
}

// A templated commit set whose items are device-resident (edc_tmpl_commits_*_device): only
// commit_off and commit_tpl are staged (tpl | commit_off | commit_tpl in the slot's staging area) and
// the set uploaded; keys, signatures, holes and variant bytes are read where the caller has them.
// The device checks the holes and the variant bytes; the flag travels behind the expansion and the
// wait reads it before it believes a verdict (finish_batch, as edc_tmpl_batch_verify_device).
static int commits_enqueue_tmpl_device(edc_ctx* ctx, Slot& s, const edc_templates* ts, const TmplShape& sh, size_t nc,
                                       const uint32_t* commit_off, const uint16_t* commit_tpl, size_t n,
                                       uint32_t alt_span, const uint8_t* d_item_alt, const uint8_t* d_vk,
                                       const uint8_t* d_sig, const uint8_t* d_var, const uint32_t* d_var_off,
                                       size_t var_bytes, const uint8_t* z_seed, bool latency) {
  int rc = init_slot(ctx, s);
  if (rc) return rc;
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, s.tw, s.st, ts, sh, &view))) return rc;
  if (n) {
    TmplWs& w = s.tw;
    hipStream_t st = s.st;
    const size_t o_coff = up16(2 * n), o_ctpl = up16(o_coff + 4 * (nc + 1));
    if ((rc = tmpl_arena_room(ctx, w, st, n, sh, var_bytes)) || (rc = tmpl_room(ctx, st, w.in, o_ctpl + 2 * nc)))
      return rc;
    CK(hipMemcpyAsync(w.in + o_coff, commit_off, 4 * (nc + 1), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(w.in + o_ctpl, commit_tpl, 2 * nc, hipMemcpyHostToDevice, st));
    uint16_t* d_tpl = reinterpret_cast<uint16_t*>(w.in.get());
    CK(hipMemsetAsync(w.flag, 0, sizeof(int), st));
    launch_tmpl_commit_map_alt(st, (uint32_t)n, (uint32_t)nc, reinterpret_cast<const uint32_t*>(w.in + o_coff),
                               reinterpret_cast<const uint16_t*>(w.in + o_ctpl), alt_span, d_item_alt, d_tpl, w.flag);
    CK(hipGetLastError());
    if ((rc = tmpl_expand(ctx, w, st, view, n, d_tpl, d_var, d_var_off, var_bytes, w.arena, w.off, true))) return rc;
    CK(hipMemcpyAsync(w.h_flag, w.flag, sizeof(int), hipMemcpyDeviceToHost, st));
    w.check = true;
  }
  rc = commits_enqueue(ctx, s, nc, commit_off, n, d_vk, d_sig, s.tw.arena, s.tw.off, nullptr, z_seed, latency);
  if (rc) s.tw.check = false;     // the batch never reaches its wait
  return rc;
}

// Wait for a commit-set slot. The union passed: every commit Ok. It failed: the grouped fallback on
// this slot (k, decoded points, grouping, failure bits and z seed of the failed batch; the inputs
// are still borrowed or staged in the slot), then the reduction to commits.
static int commits_finish(edc_ctx* ctx, Slot& s, uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad) {
  const size_t nc = s.cm_nc;
  const uint32_t* off = s.cm_off;
  const size_t n = nc ? off[nc] : 0;
  s.commits = false;
  if (n_bad) *n_bad = 0;
  int rc = finish_batch(ctx, s, nullptr, nullptr, nullptr);
  if (rc < 0) return rc;
  if (rc == EDC_OK) {
    if (commit_verdicts && nc) memset(commit_verdicts, 0, nc);
    if (item_verdicts && n) memset(item_verdicts, 0, n);
    return EDC_OK;
  }
  int f[FLAG_COUNT];
  CK(hipMemcpyAsync(f, s.flags, sizeof(f), hipMemcpyDeviceToHost, s.st));
  CK(hipStreamSynchronize(s.st));
  const bool per_sig = s.per_sig || f[FLAG_OVF] != 0;
  std::vector<uint8_t> own;
  uint8_t* codes = item_verdicts;
  if (!codes) {
    own.resize(n);
    codes = own.data();
  }
  rc = fallback_ranges(ctx, s, n, BatchIn{s.cm_vk, s.cm_sig, s.cm_msg, s.cm_moff, nullptr, s.cm_seed, 0, nullptr, false}, per_sig,
                       (uint32_t)f[FLAG_NKEYS], codes);
  if (rc < 0) return rc;
  const size_t bad = commits_reduce(nc, off, codes, commit_verdicts);
  if (n_bad) *n_bad = (int)bad;
  return bad ? EDC_INVALID_SIGNATURE : EDC_OK;
}

// Where a commit-set call's result goes: the three outputs of a synchronous call (verify), or
// null for "enqueue and return a ticket" (submit). One body per form serves both; the three
// helpers below are every place where the two modes part, on purpose:
//  - a verify of nc == 0 is EDC_OK with *n_bad = 0 before anything else is looked at, a null or
//    refused template set included; a submit of nc == 0 still checks the set, and with variants
//    that alt_span is in 1..256 (commits_check_tmpl_empty), then takes a ticket whose wait gives
//    no verdicts;
//  - a verify claims slot 0 and a submit the next ticket's slot, both after the argument checks,
//    so an argument error is reported before a busy slot;
//  - a verify enqueues latency-shaped kernels (latency = true: one batch on an idle GPU) and waits;
//    a submit enqueues the work-minimal ones and takes its ticket, only after the enqueue succeeded.
struct CommitsOut {
  uint8_t *commit_verdicts, *item_verdicts;
  int* n_bad;
};

static bool commits_nothing(const CommitsOut* out, size_t nc) {
  if (!out || nc) return false;
  if (out->n_bad) *out->n_bad = 0;
  return true;
}

static Slot* commits_claim(edc_ctx* ctx, const CommitsOut* out) { return out ? claim_slot0(ctx) : claim_next_slot(ctx); }

static int64_t commits_done(edc_ctx* ctx, Slot& s, const CommitsOut* out) {
  if (out) return commits_finish(ctx, s, out->commit_verdicts, out->item_verdicts, out->n_bad);
  return take_ticket(ctx, s);
}

// edc_commits_verify_device / _submit_device
static int64_t commits_run_device(edc_ctx* ctx, const CommitsOut* out, size_t nc, const uint32_t* commit_off,
                                  const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_msg,
                                  const uint64_t* d_msg_off, const uint8_t* d_k, const uint8_t* z_seed) {
  if (commits_nothing(out, nc)) return EDC_OK;
  size_t n = 0;
  int rc = nc ? commits_check(ctx, nc, commit_off, &n) : 0;
  if (rc) return rc;
  if (n && (!d_vk || !d_sig || (!d_k && !d_msg_off))) { ctx->err = "null input"; return EDC_ERR_ARG; }
  Slot* s = commits_claim(ctx, out);
  if (!s) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  rc = commits_enqueue(ctx, *s, nc, commit_off, n, d_vk, d_sig, d_k ? nullptr : d_msg, d_k ? nullptr : d_msg_off,
                       reinterpret_cast<const uint32_t*>(d_k), z_seed, out != nullptr);
  if (rc) return rc;
  return commits_done(ctx, *s, out);
}

// edc_commits_verify / _submit
static int64_t commits_run_host(edc_ctx* ctx, const CommitsOut* out, size_t nc, const uint32_t* commit_off,
                                const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg,
                                const uint64_t* msg_off, const uint8_t* k, const uint8_t* z_seed) {
  if (commits_nothing(out, nc)) return EDC_OK;
  size_t n = 0;
  int rc = nc ? commits_check_host(ctx, nc, commit_off, vk, key_idx, sig, msg, msg_off, k, &n) : 0;
  if (rc) return rc;
  Slot* s = commits_claim(ctx, out);
  if (!s) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  rc = commits_enqueue_host(ctx, *s, nc, commit_off, n, vk, key_idx, sig, msg, msg_off, k, z_seed, out != nullptr);
  if (rc) return rc;
  return commits_done(ctx, *s, out);
}

// edc_tmpl_commits_verify / _submit (variants = false: alt_span and item_alt are not looked at)
// and edc_tmpl_commits_verify_alt / _submit_alt (variants = true: the caller's alt_span, checked)
static int64_t commits_run_tmpl(edc_ctx* ctx, const CommitsOut* out, const edc_templates* ts, size_t nc,
                                const uint32_t* commit_off, const uint16_t* commit_tpl, bool variants, uint32_t alt_span,
                                const uint8_t* item_alt, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                                const uint8_t* var, const uint32_t* var_off, const uint8_t* z_seed) {
  if (commits_nothing(out, nc)) return EDC_OK;
  size_t n = 0;
  TmplShape sh;
  int rc = nc ? commits_check_tmpl(ctx, ts, nc, commit_off, commit_tpl, variants, alt_span, item_alt, vk, key_idx, sig, var,
                                   var_off, &sh, &n)
              : commits_check_tmpl_empty(ctx, ts, variants, alt_span, &sh);
  if (rc) return rc;
  Slot* s = commits_claim(ctx, out);
  if (!s) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  rc = commits_enqueue_tmpl(ctx, *s, ts, sh, nc, commit_off, commit_tpl, n, vk, key_idx, sig, var, var_off, z_seed,
                            out != nullptr, variants ? alt_span : 0, item_alt);
  if (rc) return rc;
  return commits_done(ctx, *s, out);
}

// edc_tmpl_commits_verify_device / _submit_device (always with variants)
static int64_t commits_run_tmpl_device(edc_ctx* ctx, const CommitsOut* out, const edc_templates* ts, size_t nc,
                                       const uint32_t* commit_off, const uint16_t* commit_tpl, uint32_t alt_span,
                                       const uint8_t* d_item_alt, const uint8_t* d_vk, const uint8_t* d_sig,
                                       const uint8_t* d_var, const uint32_t* d_var_off, size_t var_bytes,
                                       const uint8_t* z_seed) {
  if (commits_nothing(out, nc)) return EDC_OK;
  size_t n = 0;
  TmplShape sh;
  int rc = nc ? commits_check_tmpl_device(ctx, ts, nc, commit_off, commit_tpl, alt_span, d_vk, d_sig, d_var, d_var_off,
                                          var_bytes, &sh, &n)
              : commits_check_tmpl_empty(ctx, ts, true, alt_span, &sh);
  if (rc) return rc;
  Slot* s = commits_claim(ctx, out);
  if (!s) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  rc = commits_enqueue_tmpl_device(ctx, *s, ts, sh, nc, commit_off, commit_tpl, n, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                   d_var_off, var_bytes, z_seed, out != nullptr);
  if (rc) return rc;
  return commits_done(ctx, *s, out);
}

extern "C" {

int edc_commits_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                              const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                              const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                              int* n_bad_commits) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  const CommitsOut out{commit_verdicts, item_verdicts, n_bad_commits};
  return (int)commits_run_device(ctx, &out, nc, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k, z_seed);
}

int64_t edc_commits_submit_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                  const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off,
                                  const uint8_t* d_k, const uint8_t z_seed[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return commits_run_device(ctx, nullptr, nc, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k, z_seed);
}

int edc_commits_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk, const uint32_t* key_idx,
                       const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k,
                       const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  const CommitsOut out{commit_verdicts, item_verdicts, n_bad_commits};
  return (int)commits_run_host(ctx, &out, nc, commit_off, vk, key_idx, sig, msg, msg_off, k, z_seed);
}

int64_t edc_commits_submit(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                           const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                           const uint8_t* k, const uint8_t z_seed[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return commits_run_host(ctx, nullptr, nc, commit_off, vk, key_idx, sig, msg, msg_off, k, z_seed);
}

int edc_tmpl_commits_verify(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                            const uint16_t* commit_tpl, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                            const uint8_t* var, const uint32_t* var_off, const uint8_t z_seed[32],
                            uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  const CommitsOut out{commit_verdicts, item_verdicts, n_bad_commits};
  return (int)commits_run_tmpl(ctx, &out, ts, nc, commit_off, commit_tpl, false, 0, nullptr, vk, key_idx, sig, var, var_off,
                               z_seed);
}

int64_t edc_tmpl_commits_submit(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, const uint8_t* vk, const uint32_t* key_idx,
                                const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                                const uint8_t z_seed[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return commits_run_tmpl(ctx, nullptr, ts, nc, commit_off, commit_tpl, false, 0, nullptr, vk, key_idx, sig, var, var_off,
                          z_seed);
}

int edc_tmpl_commits_verify_alt(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt,
                                const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                                const uint8_t* var, const uint32_t* var_off, const uint8_t z_seed[32],
                                uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  const CommitsOut out{commit_verdicts, item_verdicts, n_bad_commits};
  return (int)commits_run_tmpl(ctx, &out, ts, nc, commit_off, commit_tpl, true, alt_span, item_alt, vk, key_idx, sig, var,
                               var_off, z_seed);
}

int64_t edc_tmpl_commits_submit_alt(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                    const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt,
                                    const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                                    const uint8_t* var, const uint32_t* var_off, const uint8_t z_seed[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return commits_run_tmpl(ctx, nullptr, ts, nc, commit_off, commit_tpl, true, alt_span, item_alt, vk, key_idx, sig, var,
                          var_off, z_seed);
}

int edc_tmpl_commits_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                   const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                   const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                   const uint32_t* d_var_off, size_t var_bytes, const uint8_t z_seed[32],
                                   uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  const CommitsOut out{commit_verdicts, item_verdicts, n_bad_commits};
  return (int)commits_run_tmpl_device(ctx, &out, ts, nc, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                      d_var_off, var_bytes, z_seed);
}

int64_t edc_tmpl_commits_submit_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                       const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                       const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                       const uint32_t* d_var_off, size_t var_bytes, const uint8_t z_seed[32]) {
  if (!ctx || !z_seed) return EDC_ERR_ARG;
  return commits_run_tmpl_device(ctx, nullptr, ts, nc, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                 d_var_off, var_bytes, z_seed);
}

int edc_commits_wait(edc_ctx* ctx, int64_t ticket, uint8_t* commit_verdicts, uint8_t* item_verdicts,
                     int* n_bad_commits) {
  if (!ctx || ticket < 0) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  Slot& s = ctx->slot[ticket % ctx->nslots];
  if (!s.pending || s.ticket != ticket) { ctx->err = "unknown or already-waited ticket"; return EDC_ERR_ARG; }
  if (!s.commits) { ctx->err = "not a commit-set ticket: wait with edc_batch_wait / edc_batch_wait_multi"; return EDC_ERR_ARG; }
  return commits_finish(ctx, s, commit_verdicts, item_verdicts, n_bad_commits);
}

// One of the two map kernels alone: stage the offsets and templates, time `reps` launches between
// two events, read the map back. variants = false: k_tmpl_commit_map over commit_off | commit_tpl |
// tpl, no flag word. variants = true: k_tmpl_commit_map_alt, with the flag word and the device
// copies of item_alt and tpl_out at the host pointers' offsets from a 16-byte boundary, so a caller
// picks the kernel's wide or narrow access paths by how it places its arrays.
static int debug_commit_map(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint16_t* commit_tpl, bool variants,
                            uint32_t alt_span, const uint8_t* item_alt, uint16_t* tpl_out, int* flagged, int reps,
                            float* ms) {
  size_t n;
  int rc = commits_check(ctx, nc, commit_off, &n);
  if (rc) return rc;
  if (variants && !commits_check_alt_span(65535, nc, commit_tpl, alt_span)) {      // the windows inside the largest set there is
    ctx->err = "template variants: alt_span in 1..256 and commit_tpl[c] + alt_span <= 65535";
    return EDC_ERR_ARG;
  }
  if (n && !tpl_out) { ctx->err = "null output"; return EDC_ERR_ARG; }
  if (!claim_slot0(ctx)) return EDC_ERR_ARG;
  Slot& s = ctx->slot[0];
  CK(hipSetDevice(ctx->device));
  const size_t o_ctpl = up16(4 * (nc + 1));
  size_t o_alt = 0, o_flag = 0, o_tpl = up16(o_ctpl + 2 * nc);
  if (variants) {
    o_alt = o_tpl + ((uintptr_t)item_alt & 15u);
    o_flag = up16(o_alt + n);
    o_tpl = o_flag + 16 + ((uintptr_t)tpl_out & 14u);
  }
  if ((rc = init_slot(ctx, s)) || (rc = ensure_aux(ctx, o_tpl + 2 * n))) return rc;
  hipStream_t st = s.st;
  const uint32_t* d_off = reinterpret_cast<const uint32_t*>(ctx->aux.get());
  const uint16_t* d_ctpl = reinterpret_cast<const uint16_t*>(ctx->aux + o_ctpl);
  uint16_t* d_tpl = reinterpret_cast<uint16_t*>(ctx->aux + o_tpl);
  int* d_flag = reinterpret_cast<int*>(ctx->aux + o_flag);
  CK(hipMemcpyAsync(ctx->aux, commit_off, 4 * (nc + 1), hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(ctx->aux + o_ctpl, commit_tpl, 2 * nc, hipMemcpyHostToDevice, st));
  if (variants) {
    if (item_alt && n) CK(hipMemcpyAsync(ctx->aux + o_alt, item_alt, n, hipMemcpyHostToDevice, st));
    CK(hipMemsetAsync(d_flag, 0, sizeof(int), st));
  }
  CK(hipEventRecord(s.ev[0], st));
  for (int r = 0; r < reps; ++r)
    if (variants)
      launch_tmpl_commit_map_alt(st, (uint32_t)n, (uint32_t)nc, d_off, d_ctpl, alt_span, item_alt ? ctx->aux + o_alt : nullptr,
                                 d_tpl, d_flag);
    else
      launch_tmpl_commit_map(st, (uint32_t)n, (uint32_t)nc, d_off, d_ctpl, d_tpl);
  CK(hipGetLastError());
  CK(hipEventRecord(s.ev[1], st));
  int flag = 0;
  if (n) CK(hipMemcpyAsync(tpl_out, d_tpl, 2 * n, hipMemcpyDeviceToHost, st));
  if (variants) CK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  if (flagged) *flagged = flag != 0;
  if (ms) {
    CK(hipEventElapsedTime(ms, s.ev[0], s.ev[1]));
    *ms /= (float)reps;
  }
  return 0;
}

int edc_debug_tmpl_commit_map(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint16_t* commit_tpl,
                              uint16_t* tpl_out, int reps, float* ms) {
  if (!ctx || !nc || !commit_tpl || reps < 1) return EDC_ERR_ARG;
  return debug_commit_map(ctx, nc, commit_off, commit_tpl, false, 0, nullptr, tpl_out, nullptr, reps, ms);
}

int edc_debug_tmpl_commit_map_alt(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint16_t* commit_tpl,
                                  uint32_t alt_span, const uint8_t* item_alt, uint16_t* tpl_out, int* flagged,
                                  int reps, float* ms) {
  if (!ctx || !nc || !commit_tpl || reps < 1) return EDC_ERR_ARG;
  return debug_commit_map(ctx, nc, commit_off, commit_tpl, true, alt_span, item_alt, tpl_out, flagged, reps, ms);
}

int edc_decompress(edc_ctx* ctx, size_t n, const uint8_t* enc, uint8_t* xy, uint8_t* ok) {
  if (!ctx || (n && (!enc || !xy || !ok))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = ensure_n(ctx, n);
  if (rc) return rc;
  rc = ensure_aux(ctx, n * 64);
  if (rc) return rc;
  if (!n) return 0;
  hipStream_t st = ctx->st();
  CK(hipMemcpyAsync(ctx->vk, enc, n * 32, hipMemcpyHostToDevice, st));
  launch_decode(st, (uint32_t)n, ctx->vk, ctx->aux, ctx->verdicts);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(xy, ctx->aux, n * 64, hipMemcpyDeviceToHost, st));
  CK(hipMemcpyAsync(ok, ctx->verdicts, n, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return 0;
}

int edc_vk_validate(edc_ctx* ctx, size_t n, const uint8_t* vk, uint8_t* codes) {
  if (!ctx || (n && (!vk || !codes))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = ensure_n(ctx, n);
  if (rc) return rc;
  if (!n) return 0;
  hipStream_t st = ctx->st();
  CK(hipMemcpyAsync(ctx->vk, vk, n * 32, hipMemcpyHostToDevice, st));
  launch_vk_validate(st, (uint32_t)n, ctx->vk, ctx->verdicts);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(codes, ctx->verdicts, n, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return 0;
}

int edc_keycache_clear(edc_ctx* ctx) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  for (Slot& s : ctx->slot)
    if (s.pending) { ctx->err = "key cache change with a batch in flight"; return EDC_ERR_ARG; }
  int rc = sync_all(ctx);
  if (rc) return rc;
  free_keycache(ctx);
  return 0;
}

size_t edc_keycache_size(const edc_ctx* ctx) { return ctx ? ctx->kc_m : 0; }

// Appends the distinct new keys `neww` (un x 8 words) to the cache: grows the device arrays
// (capacity doubling; the cached keys keep their indices), decodes the new keys and builds their
// comb tables, builds B's comb table with the first key, and rebuilds the hash table over all
// keys. No batch may be in flight (callers check).
static int kc_append(edc_ctx* ctx, const std::vector<uint32_t>& neww) {
  const uint32_t u0 = ctx->kc_m, un = (uint32_t)(neww.size() / 8), u = u0 + un;
  if (!un) return 0;
  ctx->kc_gen++;                // also on a failure below: the arrays may already have moved
  hipStream_t st = ctx->st();
  const size_t comb_words = (size_t)COMB_ENTRIES * NIELS_WORDS;
  if (u > ctx->kc_cap) {
    uint32_t cap = ctx->kc_cap ? 2 * ctx->kc_cap : 16;
    while (cap < u) cap *= 2;
    if (cap > KC_MAX_KEYS) cap = KC_MAX_KEYS;
    DevBuf<uint32_t> keys, comb;
    DevBuf<uint8_t> okd;
    if (alloc_all(sized(keys, (size_t)cap * 8), sized(okd, cap), sized(comb, (size_t)cap * comb_words)) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "key cache: out of device memory";
      return EDC_ERR_NOMEM;
    }
    if (u0) {
      CK(hipMemcpyAsync(keys, ctx->kc_keys, (size_t)u0 * 8 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      CK(hipMemcpyAsync(okd, ctx->kc_ok, u0, hipMemcpyDeviceToDevice, st));
      CK(hipMemcpyAsync(comb, ctx->kc_comb, (size_t)u0 * comb_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      CK(hipStreamSynchronize(st));
    }
    ctx->kc_keys = std::move(keys);
    ctx->kc_ok = std::move(okd);
    ctx->kc_comb = std::move(comb);
    ctx->kc_cap = cap;
  }
  std::vector<uint32_t> all(ctx->kc_words);   // committed to the context only on success
  all.insert(all.end(), neww.begin(), neww.end());
  const uint32_t T = (uint32_t)next_pow2(2 * (size_t)(u < 8 ? 8 : u));
  std::vector<uint32_t> table(T, KC_EMPTY);
  for (uint32_t c = 0; c < u; ++c) {
    uint32_t h = kc_hash(&all[8 * c], ctx->kc_s0, ctx->kc_s1) & (T - 1);
    while (table[h] != KC_EMPTY) h = (h + 1) & (T - 1);
    table[h] = c;
  }
  // new table and scratch first: a failed allocation leaves the previous cache fully usable
  DevBuf<uint32_t> ntable, ext;   // ext: scratch, freed on return (the stream is synchronized below)
  const bool new_table = T - 1 != ctx->kc_tmask || !ctx->kc_table;
  if ((new_table && ntable.alloc(T) != hipSuccess) || ext.alloc((size_t)(un + 1) * EXT_WORDS) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "key cache: out of device memory";
    return EDC_ERR_NOMEM;
  }
  if (new_table) {
    CK(hipStreamSynchronize(st));
    ctx->kc_table = std::move(ntable);
  }
  CK(hipMemcpyAsync(ctx->kc_table, table.data(), T * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(ctx->kc_keys + (size_t)u0 * 8, neww.data(), neww.size() * sizeof(uint32_t),
                    hipMemcpyHostToDevice, st));
  launch_kc_decode(st, un, ctx->kc_keys + (size_t)u0 * 8, ext, ctx->kc_ok + u0);
  launch_kc_comb(st, un, ext, ctx->kc_comb + (size_t)u0 * comb_words);
  if (!ctx->bcomb) {
    CK(ctx->bcomb.alloc(comb_words));
    uint32_t* bext = ext + (size_t)un * EXT_WORDS;
    launch_kc_basepoint(st, bext);
    launch_kc_comb(st, 1, bext, ctx->bcomb);
  }
  CK(hipGetLastError());
  std::vector<uint8_t> okn(un);
  CK(hipMemcpyAsync(okn.data(), ctx->kc_ok + u0, un, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  ctx->kc_words.swap(all);
  ctx->kc_okh.insert(ctx->kc_okh.end(), okn.begin(), okn.end());
  ctx->kc_m = u;
  ctx->kc_tmask = T - 1;
  ctx->last_uncached = 0;                    // try split coefficients with the new key set
  return 0;
}

// distinct keys of vk (m x 32 bytes) not yet cached, in first-occurrence order; of[i] = the
// cache index key i will have
// (limit: the most keys the cache may then hold; edc_keycache_add checks it after dropping the
// keys that do not decode instead)
static int kc_collect(edc_ctx* ctx, size_t m, const uint8_t* vk, std::vector<uint32_t>& of,
                      std::vector<uint32_t>& neww, size_t limit = KC_MAX_KEYS) {
  std::unordered_map<std::string, uint32_t> idx;
  for (uint32_t c = 0; c < ctx->kc_m; ++c)
    idx.emplace(std::string(reinterpret_cast<const char*>(&ctx->kc_words[8 * c]), 32), c);
  of.resize(m);
  for (size_t i = 0; i < m; ++i) {
    auto it = idx.emplace(std::string(reinterpret_cast<const char*>(vk + 32 * i), 32), (uint32_t)idx.size());
    of[i] = it.first->second;
    if (it.second) {
      if (idx.size() > limit) { ctx->err = "key cache holds at most 65536 keys"; return EDC_ERR_ARG; }
      uint32_t w[8];
      memcpy(w, vk + 32 * i, 32);
      neww.insert(neww.end(), w, w + 8);
    }
  }
  return 0;
}

int64_t edc_keycache_load(edc_ctx* ctx, size_t m, const uint8_t* vk, uint8_t* ok) {
  if (!ctx || (m && !vk)) return EDC_ERR_ARG;
  int rc = edc_keycache_clear(ctx);
  if (rc) return rc;
  if (!m) return 0;
  // distinct keys in first-occurrence order (the cache is keyed on raw bytes, like the batch's
  // HashMap<VerificationKeyBytes, _>, src/batch.rs:114)
  std::vector<uint32_t> of, words;
  if ((rc = kc_collect(ctx, m, vk, of, words))) return rc;
  if ((rc = kc_append(ctx, words))) return rc;
  CK(ctx->kc_reg.alloc(m));
  CK(hipMemcpy(ctx->kc_reg, of.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
  ctx->kc_reg_m = (uint32_t)m;
  ctx->kc_regh = of;
  if (ok)
    for (size_t i = 0; i < m; ++i) ok[i] = ctx->kc_okh[of[i]];
  return ctx->kc_m;
}

int64_t edc_keycache_add(edc_ctx* ctx, size_t m, const uint8_t* vk, uint8_t* ok) {
  if (!ctx || (m && !vk)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  for (Slot& s : ctx->slot)
    if (s.pending) { ctx->err = "key cache change with a batch in flight"; return EDC_ERR_ARG; }
  int rc = sync_all(ctx);
  if (rc) return rc;
  std::vector<uint32_t> of, words;
  if ((rc = kc_collect(ctx, m, vk, of, words, SIZE_MAX))) return rc;
  // keys that fail to decode (VerificationKey::try_from's MalformedPublicKey) are not added: the
  // entry is meant for keys parsed from untrusted input, and a malformed one must not pin 64 KB of
  // comb table. of[] is remapped to the kept keys; a dropped key reports ok = 0.
  const uint32_t u0 = ctx->kc_m, un = (uint32_t)(words.size() / 8);
  std::vector<uint8_t> code(un, 0);
  if (un) {
    hipStream_t st = ctx->st();
    DevBuf<uint8_t> denc, dcode;   // scratch, freed at the end of this block
    if (alloc_all(sized(denc, (size_t)un * 32), sized(dcode, un)) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "key cache: out of device memory";
      return EDC_ERR_NOMEM;
    }
    CK(hipMemcpyAsync(denc, words.data(), (size_t)un * 32, hipMemcpyHostToDevice, st));
    launch_vk_validate(st, un, denc, dcode);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(code.data(), dcode, un, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
  }
  std::vector<uint32_t> keep, remap(un, UINT32_MAX);
  for (uint32_t j = 0; j < un; ++j)
    if (code[j] == EDC_OK) {
      remap[j] = u0 + (uint32_t)(keep.size() / 8);
      keep.insert(keep.end(), &words[8 * j], &words[8 * j] + 8);
    }
  if (u0 + keep.size() / 8 > KC_MAX_KEYS) { ctx->err = "key cache holds at most 65536 keys"; return EDC_ERR_ARG; }
  if ((rc = kc_append(ctx, keep))) return rc;
  if (ok)
    for (size_t i = 0; i < m; ++i) {
      const uint32_t c = of[i] < u0 ? of[i] : remap[of[i] - u0];
      ok[i] = c == UINT32_MAX ? 0 : ctx->kc_okh[c];
    }
  return ctx->kc_m;
}

int edc_sign_device(edc_ctx* ctx, size_t n, const uint8_t* d_seeds, const uint32_t* d_seed_index,
                    const uint8_t* d_msg, const uint64_t* d_msg_off, uint8_t* d_vk_out, uint8_t* d_sig_out) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  launch_sign(ctx->st(), (uint32_t)n, d_seeds, d_seed_index, d_msg, d_msg_off, ctx->btab, d_vk_out, d_sig_out);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->st()));
  return 0;
}

int edc_sign(edc_ctx* ctx, size_t n, const uint8_t* seeds, size_t nseeds, const uint32_t* seed_index,
             const uint8_t* msg, const uint64_t* msg_off, uint8_t* vk_out, uint8_t* sig_out) {
  if (!ctx || (n && (!seeds || !vk_out || !sig_out || !msg_off))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  if (seed_index) {
    for (size_t i = 0; i < n; ++i)
      if (seed_index[i] >= nseeds) { ctx->err = "seed_index out of range"; return EDC_ERR_ARG; }
  } else if (nseeds < n) {
    ctx->err = "need one seed per item when seed_index is NULL";
    return EDC_ERR_ARG;
  }
  int rc = upload_msgs(ctx, n, msg, msg_off);
  if (rc) return rc;
  if (!n) return 0;
  // aux: seeds (nseeds*32) | seed_index (n*4) | vk_out (n*32) | sig_out (n*64)
  const size_t sb = nseeds * 32, ib = seed_index ? n * 4 : 0;
  const size_t sb16 = (sb + 15) & ~(size_t)15, ib16 = (ib + 15) & ~(size_t)15;
  rc = ensure_aux(ctx, sb16 + ib16 + n * 96 + 64);
  if (rc) return rc;
  hipStream_t st = ctx->st();
  uint8_t* d_seeds = ctx->aux;
  uint32_t* d_idx = seed_index ? reinterpret_cast<uint32_t*>(ctx->aux + sb16) : nullptr;
  uint8_t* d_vk = ctx->aux + sb16 + ib16;
  uint8_t* d_sig = d_vk + n * 32;
  CK(hipMemcpyAsync(d_seeds, seeds, sb, hipMemcpyHostToDevice, st));
  if (d_idx) CK(hipMemcpyAsync(d_idx, seed_index, ib, hipMemcpyHostToDevice, st));
  launch_sign(st, (uint32_t)n, d_seeds, d_idx, ctx->msg, ctx->off, ctx->btab, d_vk, d_sig);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(vk_out, d_vk, n * 32, hipMemcpyDeviceToHost, st));
  CK(hipMemcpyAsync(sig_out, d_sig, n * 64, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return 0;
}

int edc_chacha_fill_device(edc_ctx* ctx, const uint8_t key[32], uint64_t blk0, uint64_t nblocks, uint8_t* d_out) {
  if (!ctx || !key || (nblocks && !d_out)) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  uint32_t k[8];
  seed_words(key, k);
  launch_chacha_fill(ctx->st(), k, blk0, nblocks, reinterpret_cast<uint32_t*>(d_out));
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->st()));
  return 0;
}

int edc_set_slots(edc_ctx* ctx, int k) {
  if (!ctx || k < 1 || k > kSlots) return EDC_ERR_ARG;
  for (Slot& s : ctx->slot)
    if (s.pending) { ctx->err = "slot count change with a batch in flight"; return EDC_ERR_ARG; }
  ctx->nslots = k;
  ctx->next_ticket = 0;
  return 0;
}

int edc_set_key_grouping(edc_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 3) return EDC_ERR_ARG;
  ctx->key_grouping = mode;
  ctx->ungrouped_run = 0;
  return 0;
}

int edc_set_key_split(edc_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 1) return EDC_ERR_ARG;
  ctx->key_split = mode;
  return 0;
}

int edc_set_fallback_shape(edc_ctx* ctx, int ranges, int bits) {
  if (!ctx || ranges < 1 || ranges > 1024 || bits < 8 || bits > 13) return EDC_ERR_ARG;
  ctx->fb_ranges = (uint32_t)ranges;
  ctx->fb_bits = bits;
  return 0;
}

int edc_set_msm_shape(edc_ctx* ctx, int bits, int parts) {
  if (!ctx || bits < 0 || (bits && (bits < 8 || bits > 16)) || parts < 0 || parts > 64) return EDC_ERR_ARG;
  ctx->win_bits = bits;
  ctx->msm_parts = (uint32_t)parts;
  return 0;
}

int edc_set_msm_bin_entries(edc_ctx* ctx, int entries) {
  if (!ctx || entries < 0 || (entries && entries < 256)) return EDC_ERR_ARG;
  ctx->bin_entries = (uint32_t)entries;
  return 0;
}

int edc_debug_last_plan(const edc_ctx* ctx, edc_plan_info* out) {
  if (!ctx || !out || !ctx->have_plan) return EDC_ERR_ARG;
  *out = ctx->last_plan;
  return 0;
}

int edc_reserve(edc_ctx* ctx, size_t n) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  const int c = ctx->win_bits ? ctx->win_bits : auto_window_bits(n);
  MsmPlan dense = make_plan(c, c, 1), few = make_plan(c, 8, 1);
  dense.nranges = few.nranges = MSM_MAX_BINS / (dense.bins_per_range > few.bins_per_range ? dense.bins_per_range
                                                                                          : few.bins_per_range);
  if (dense.nranges > 16) dense.nranges = few.nranges = 16;
  const MsmPlan splitp = make_plan(c, c, 1, false);
  size_t e1 = msm_entry_capacity(dense, n, n + 1), e2 = msm_entry_capacity(few, n, n + 1);
  const size_t e3 = msm_entry_capacity(splitp, 2 + 3 * n, 0);   // split coefficients (key cache)
  if (e3 > e1) e1 = e3;
  for (int i = 0; i < ctx->nslots; ++i) {
    Slot& s = ctx->slot[i];
    if (s.pending) { ctx->err = "reserve with a batch in flight"; return EDC_ERR_ARG; }
    int rc = ensure_slot(ctx, s, n);
    if (rc) return rc;
    rc = ensure_msm(ctx, s, dense.nbin() >= few.nbin() ? dense : few, e1 > e2 ? e1 : e2);
    if (rc) return rc;
  }
  return 0;
}

void edc_set_timing(edc_ctx* ctx, int enable) {
  if (ctx) ctx->timing = enable != 0;
}

int edc_last_timings(const edc_ctx* ctx, float* ms, int cap) {
  if (!ctx || !ms) return 0;
  int c = ctx->nlast < cap ? ctx->nlast : cap;
  for (int i = 0; i < c; ++i) ms[i] = ctx->last_ms[i];
  return c;
}

const char* edc_timing_name(int i) { return (i >= 0 && i < PH_N) ? kPhaseNames[i] : ""; }

int edc_last_msm_accum(const edc_ctx* ctx, float* ms, uint64_t* entries) {
  if (!ctx || !ctx->nlast) return EDC_ERR_ARG;
  if (ms) *ms = ctx->last_acc_ms;
  if (entries) *entries = ctx->last_acc_entries;
  return 0;
}

int edc_synchronize(edc_ctx* ctx) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  for (Slot& s : ctx->slot)
    if (s.st) CK(hipStreamSynchronize(s.st));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- verified-signature cache
// sigcache.h: a cached call looks every item up, compacts the misses (queue order) into one
// contiguous batch and hands that batch to the existing entries' own paths (run_batch_sync,
// batch_with_fallback, the per-item kernels), so verdicts and check8 are those entries' on the miss
// list by construction. The miss count needs one 4-byte device-to-host copy and a stream
// synchronization before the MSM can be planned.
// preconditions of every cached entry: a table, and slot 0 (their stream and workspace) idle
static int sc_ready(edc_ctx* ctx) {
  if (!ctx->sc_cap) { ctx->err = "no signature cache on this context (edc_sigcache_create)"; return EDC_ERR_ARG; }
  return claim_slot0(ctx) ? 0 : EDC_ERR_ARG;
}

// Ordering against the deferred inserts of cached verifiers (edc_ctx::sc_ev): work enqueued on st
// after this call starts once the last such insert has run ...
static int sc_order_after_inserts(edc_ctx* ctx, hipStream_t st) {
  if (ctx->sc_ev_set) CK(hipStreamWaitEvent(st, ctx->sc_ev, 0));
  return 0;
}

// ... and the host-side form, for the entries that change or read the table's state from the host
static hipError_t sc_wait_inserts(const edc_ctx* ctx) {
  return ctx->sc_ev_set ? hipEventSynchronize(ctx->sc_ev) : hipSuccess;
}

static int ensure_sc(edc_ctx* ctx, size_t n) {
  CK(grow_group(ctx->sc_cap_n, n, item_cap, sync_of(ctx->st()), [&](size_t cap) {
    return alloc_all(sized(ctx->sc_hit, cap), sized(ctx->sc_g, cap * 128), sized(ctx->sc_verd, cap), sized(ctx->sc_mverd, cap),
                     sized(ctx->sc_wg, cap / SC_BLOCK + 2),   // one count per workgroup + the total
                     sized(ctx->sc_idx, cap));
  }));
  return 0;
}

// The misses of one cached call, in queue order: a contiguous batch (vk, sig, k) and, unless every
// item missed (idx null: the batch is the caller's arrays), their queue positions. o_*: the
// caller's arrays, which idx indexes.
struct ScMiss {
  size_t n = 0;
  const uint32_t* idx = nullptr;
  const uint8_t *vk = nullptr, *sig = nullptr;
  const uint32_t* k = nullptr;
  const uint8_t *o_vk = nullptr, *o_sig = nullptr;
  const uint32_t* o_k = nullptr;
};

static int sc_partition(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig, const uint32_t* d_k,
                        ScMiss* M) {
  *M = ScMiss{};
  M->vk = M->o_vk = d_vk;
  M->sig = M->o_sig = d_sig;
  M->k = M->o_k = d_k;
  if (!n) return 0;
  int rc = ensure_sc(ctx, n);
  if (rc) return rc;
  hipStream_t st = ctx->st();
  if ((rc = sc_order_after_inserts(ctx, st))) return rc;
  const uint32_t N = (uint32_t)n, nwg = (N + SC_BLOCK - 1) / SC_BLOCK;
  launch_sc_lookup(st, ctx->sc(), N, d_vk, d_sig, d_k, ctx->sc_hit, ctx->sc_wg);
  launch_sc_scan(st, nwg, ctx->sc_wg, ctx->sc_wg + nwg);
  CK(hipGetLastError());
  ctx->sc_hctr[2] = 0;
  CK(hipMemcpyAsync(&ctx->sc_hctr[2], ctx->sc_wg + nwg, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  M->n = (size_t)ctx->sc_hctr[2];
  if (M->n > n) { ctx->err = "signature cache: miss count out of range"; return EDC_ERR_HIP; }
  ctx->sc_hits += n - M->n;
  ctx->sc_misses += M->n;
  if (M->n == 0 || M->n == n) return 0;   // nothing to verify / the caller's arrays are the batch
  uint8_t* g_vk = ctx->sc_g;
  uint8_t* g_sig = g_vk + ctx->sc_cap_n * 32;
  uint32_t* g_k = reinterpret_cast<uint32_t*>(g_sig + ctx->sc_cap_n * 64);
  launch_sc_compact(st, N, ctx->sc_hit, ctx->sc_wg, d_vk, d_sig, d_k, ctx->sc_idx, g_vk, g_sig, g_k);
  CK(hipGetLastError());
  M->idx = ctx->sc_idx;
  M->vk = g_vk;
  M->sig = g_sig;
  M->k = g_k;
  return 0;
}

// insert the misses whose d_mverd[j] is 0 (null: all), refresh the counters' host mirror
static int sc_insert(edc_ctx* ctx, const ScMiss& M, const uint8_t* d_mverd) {
  if (!M.n) return 0;
  hipStream_t st = ctx->st();
  launch_sc_insert(st, ctx->sc(), (uint32_t)M.n, M.idx, M.o_vk, M.o_sig, M.o_k, d_mverd, ctx->sc_ctr);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->sc_hctr, ctx->sc_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return 0;
}

// per-item codes of the misses (device, M.n bytes) -> verdicts (host, n bytes); hits are EDC_OK
static int sc_verdicts_out(edc_ctx* ctx, size_t n, const ScMiss& M, const uint8_t* d_mverd, uint8_t* verdicts) {
  hipStream_t st = ctx->st();
  if (!M.n) {
    memset(verdicts, 0, n);
  } else if (!M.idx) {
    CK(hipMemcpyAsync(verdicts, d_mverd, n, hipMemcpyDeviceToHost, st));
  } else {
    CK(hipMemsetAsync(ctx->sc_verd, 0, n, st));
    launch_sc_scatter(st, (uint32_t)M.n, M.idx, d_mverd, ctx->sc_verd);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(verdicts, ctx->sc_verd, n, hipMemcpyDeviceToHost, st));
  }
  return 0;
}

// cached batch on device-resident items; verdicts null: the plain entry, else the fallback entry
static int sc_batch(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_msg,
                    const uint64_t* d_off, const uint8_t* d_k, const uint8_t* z_seed, uint8_t* verdicts, int* n_invalid,
                    uint8_t check8[32], size_t* n_miss) {
  int rc = sc_ready(ctx);
  if (rc) return rc;
  if (n >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  if (n && check_aligned16(ctx, "device vk / sig / k arrays", {d_vk, d_sig, d_k})) return EDC_ERR_ARG;
  if (n_invalid) *n_invalid = 0;
  const uint32_t* k = reinterpret_cast<const uint32_t*>(d_k);
  if (n && !k) {            // Item::from for every item: the record, and so the lookup, needs k
    if ((rc = ensure_n(ctx, n))) return rc;
    launch_challenge(ctx->st(), (uint32_t)n, d_vk, d_sig, d_msg, d_off, ctx->kbuf);
    CK(hipGetLastError());
    k = ctx->kbuf;
  }
  ScMiss M;
  if ((rc = sc_partition(ctx, n, d_vk, d_sig, k, &M))) return rc;
  if (n_miss) *n_miss = M.n;
  // an empty miss list still runs the n = 0 batch, whose k is never read
  const uint32_t* mk = M.n ? M.k : reinterpret_cast<const uint32_t*>(ctx->sc_hdr.get());
  const BatchIn in{M.vk, M.sig, nullptr, nullptr, mk, z_seed, 0, nullptr, false};
  if (!verdicts) {
    rc = run_batch_sync(ctx, M.n, in, check8, nullptr, nullptr);
    if (rc != EDC_OK) return rc;     // a failed batch inserts nothing
    return (rc = sc_insert(ctx, M, nullptr)) ? rc : EDC_OK;
  }
  std::vector<uint8_t> mv(M.n ? M.n : 1);
  const int code = batch_with_fallback(ctx, M.n, in, mv.data(), n_invalid, check8);
  if (code < 0) return code;
  if (M.n) CK(hipMemcpyAsync(ctx->sc_mverd, mv.data(), M.n, hipMemcpyHostToDevice, ctx->st()));
  if ((rc = sc_verdicts_out(ctx, n, M, ctx->sc_mverd, verdicts))) return rc;
  if ((rc = sc_insert(ctx, M, ctx->sc_mverd))) return rc;     // exactly the misses whose code is EDC_OK
  CK(hipStreamSynchronize(ctx->st()));
  return code;
}

extern "C" {

int edc_sigcache_create(edc_ctx* ctx, size_t capacity, int keep) {
  if (!ctx || keep < 0) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  for (Slot& s : ctx->slot)
    if (s.pending) { ctx->err = "signature cache change with a batch in flight"; return EDC_ERR_ARG; }
  int rc = sync_all(ctx);
  if (rc) return rc;
  CK(sc_wait_inserts(ctx));
  reset_all(ctx->sc_hdr, ctx->sc_rec);
  ctx->sc_cap = 0;
  if (!capacity) return 0;
  if (capacity > (1ull << 30)) { ctx->err = "signature cache capacity above 2^30 records"; return EDC_ERR_ARG; }
  const size_t cap = next_pow2(capacity < SC_WINDOW ? SC_WINDOW : capacity);
  if (alloc_all(sized(ctx->sc_hdr, cap), sized(ctx->sc_rec, cap * 8)) != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "signature cache: out of device memory";
    return EDC_ERR_NOMEM;
  }
  if (!ctx->sc_ctr) CK(ctx->sc_ctr.alloc(2));
  if (!ctx->sc_hctr) CK(ctx->sc_hctr.alloc(3));
  CK(hipMemsetAsync(ctx->sc_hdr, 0, cap * sizeof(unsigned long long), ctx->st()));
  CK(hipMemsetAsync(ctx->sc_ctr, 0, 2 * sizeof(unsigned long long), ctx->st()));
  CK(hipStreamSynchronize(ctx->st()));
  ctx->sc_hctr[0] = ctx->sc_hctr[1] = ctx->sc_hctr[2] = 0;
  ctx->sc_cap = cap;
  ctx->sc_gen = 1;
  ctx->sc_keep = keep ? (uint32_t)keep : 2u;
  ctx->sc_hits = ctx->sc_misses = 0;
  return 0;
}

int edc_sigcache_clear(edc_ctx* ctx) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = sc_ready(ctx);
  if (rc) return rc;
  CK(sc_wait_inserts(ctx));
  CK(hipMemsetAsync(ctx->sc_hdr, 0, ctx->sc_cap * sizeof(unsigned long long), ctx->st()));
  CK(hipStreamSynchronize(ctx->st()));
  return 0;
}

int edc_sigcache_advance(edc_ctx* ctx) {
  if (!ctx) return EDC_ERR_ARG;
  if (ctx->sc_gen == 0xFFFFFFFFu) {     // the generation would wrap: start over with an empty table
    int rc = edc_sigcache_clear(ctx);
    if (rc) return rc;
    ctx->sc_gen = 1;
    return 0;
  }
  int rc = sc_ready(ctx);
  if (rc) return rc;
  CK(sc_wait_inserts(ctx));
  ctx->sc_gen++;
  return 0;
}

int edc_sigcache_stats(const edc_ctx* ctx, uint64_t out[6]) {
  if (!ctx || !out || !ctx->sc_cap) return EDC_ERR_ARG;
  // a cached verifier's deferred insert ends with the copy of the counters into their pinned
  // mirror: once it has run the mirror is current
  if (sc_wait_inserts(ctx) != hipSuccess) {
    (void)hipGetLastError();
    return EDC_ERR_HIP;
  }
  out[0] = ctx->sc_cap;
  out[1] = ctx->sc_gen;
  out[2] = ctx->sc_hits;
  out[3] = ctx->sc_misses;
  out[4] = ctx->sc_hctr[0];
  out[5] = ctx->sc_hctr[1];
  return 0;
}

int edc_sigcache_lookup_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_k,
                               uint8_t* d_hit) {
  if (!ctx || (n && (!d_vk || !d_sig || !d_k || !d_hit))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = sc_ready(ctx);
  if (rc) return rc;
  if (n >= (1ull << 28)) { ctx->err = "batch too large for one call (max 2^28 items)"; return EDC_ERR_ARG; }
  if (n && check_aligned16(ctx, "device vk / sig / k arrays", {d_vk, d_sig, d_k})) return EDC_ERR_ARG;
  if ((rc = sc_order_after_inserts(ctx, ctx->st()))) return rc;
  launch_sc_lookup(ctx->st(), ctx->sc(), (uint32_t)n, d_vk, d_sig, reinterpret_cast<const uint32_t*>(d_k), d_hit,
                   nullptr);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->st()));
  return 0;
}

int edc_sigcache_batch_verify_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                     const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                     const uint8_t z_seed[32], uint8_t check8[32], size_t* n_miss) {
  if (!ctx || !z_seed || (n && (!d_vk || !d_sig || (!d_k && !d_msg_off)))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return sc_batch(ctx, n, d_vk, d_sig, d_msg, d_msg_off, d_k, z_seed, nullptr, nullptr, check8, n_miss);
}

int edc_sigcache_batch_verify_fallback_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                              const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                              const uint8_t z_seed[32], uint8_t* verdicts, int* n_invalid,
                                              uint8_t check8[32], size_t* n_miss) {
  if (!ctx || !z_seed || !verdicts || (n && (!d_vk || !d_sig || (!d_k && !d_msg_off)))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  return sc_batch(ctx, n, d_vk, d_sig, d_msg, d_msg_off, d_k, z_seed, verdicts, n_invalid, check8, n_miss);
}

// host items into the context's staging buffers (slot 0's stream): keys, signatures and either
// the message arena or the caller's k (into kbuf)
static int sc_upload(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                     const uint64_t* msg_off, const uint8_t* k) {
  int rc = 0;
  if (k && ((rc = init_slot(ctx, ctx->slot[0])) || (rc = ensure_n(ctx, n)))) return rc;
  return stage_host(ctx, n, vk, sig, msg, msg_off, k, ctx->kbuf);
}

int edc_sigcache_batch_verify(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                              const uint64_t* msg_off, const uint8_t* k, const uint8_t z_seed[32], uint8_t check8[32],
                              size_t* n_miss) {
  if (!ctx || !z_seed || (k != nullptr) == (msg_off != nullptr) || (n && (!vk || !sig))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = sc_ready(ctx);
  if (rc) return rc;
  if ((rc = sc_upload(ctx, n, vk, sig, msg, msg_off, k))) return rc;
  return sc_batch(ctx, n, ctx->vk, ctx->sig, ctx->msg, k ? nullptr : ctx->off,
                  k ? reinterpret_cast<const uint8_t*>(ctx->kbuf.get()) : nullptr, z_seed, nullptr, nullptr, check8, n_miss);
}

int edc_sigcache_verify_each(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                             const uint64_t* msg_off, const uint8_t* k, uint8_t* verdicts, size_t* n_miss) {
  if (!ctx || (k != nullptr) == (msg_off != nullptr) || (n && (!vk || !sig || !verdicts))) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  int rc = sc_ready(ctx);
  if (rc) return rc;
  // a hit is byte-identical to an inserted record, whose k was canonical: checking every k is
  // checking the misses' (Scalar::from_hash never yields k >= l)
  if (k && k_all_canonical(ctx, n, k)) return EDC_ERR_ARG;
  if ((rc = sc_upload(ctx, n, vk, sig, msg, msg_off, k))) return rc;
  hipStream_t st = ctx->st();
  if (n && !k) {
    launch_challenge(st, (uint32_t)n, ctx->vk, ctx->sig, ctx->msg, ctx->off, ctx->kbuf);
    CK(hipGetLastError());
  }
  ScMiss M;
  if ((rc = sc_partition(ctx, n, ctx->vk, ctx->sig, ctx->kbuf, &M))) return rc;
  if (n_miss) *n_miss = M.n;
  if ((rc = verify_items(ctx, st, M.n, M.vk, M.sig, nullptr, nullptr, M.k, M.n <= kQuadVerifyMax, ctx->verdicts, nullptr)))
    return rc;
  if ((rc = sc_verdicts_out(ctx, n, M, ctx->verdicts, verdicts))) return rc;
  if ((rc = sc_insert(ctx, M, ctx->verdicts))) return rc;
  CK(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- quorum commit sets
// quorum.h / edc_quorum.hip: the selection marks the votes that are not checked, the cached
// entries' compaction (sc_* staging, allocated here without a table) gathers the checked ones in
// queue order into one contiguous batch, and that batch runs through batch_with_fallback, so the
// union verdict, check8 and the item codes are edc_batch_verify_prehashed_device's and the grouped
// fallback's on the gathered list by construction. The checked count needs one 8-byte
// device-to-host copy (with the device checks' flag) and a stream synchronization before the MSM
// can be planned. A passing union's tally is planned[]; a failed one scatters the codes back and
// runs the tally kernel. All on slot 0.
// Every form is its checks and staging (*_inputs), then quorum_select_enqueue, what the form adds
// behind the selection, quorum_select_read, quorum_gather and quorum_finish.
// The sync() of one tier's growth: its groups of one dimension (votes, commits) grow together, and
// the stream is drained once in front of the first of them.
struct GrowSync {
  hipStream_t st;
  bool did[2] = {false, false};
  auto once(int d) { return [this, d] { return std::exchange(did[d], true) ? hipSuccess : hipStreamSynchronize(st); }; }
  auto n() { return once(0); }
  auto c() { return once(1); }
};

static int side_votes_room(edc_ctx* ctx, QuorumSide& s, size_t n, size_t nc, GrowSync& g) {
  CK(grow_group(s.cap_c, nc, off_cap, g.c(), [&](size_t cap) {
    return alloc_all(sized(s.thr, cap), sized(s.planned, cap), sized(s.tally, cap), sized(s.cor, cap));
  }));
  CK(grow_group(s.cap_n, n ? n : 1, item_cap, g.n(), [&](size_t cap) { return alloc_all(sized(s.power, cap), sized(s.flag, cap)); }));
  return 0;
}

static int side_join_room(edc_ctx* ctx, QuorumSide& s, size_t n, size_t nc, GrowSync& g) {
  CK(grow_group(s.join_n, n ? n : 1, item_cap, g.n(), [&](size_t cap) { return alloc_all(sized(s.who, cap), sized(s.set, 2 * cap)); }));
  CK(grow_group(s.join_c, nc, off_cap, g.c(), [&](size_t cap) {
    const hipError_t e = s.dv.alloc(cap);
    return e != hipSuccess ? e : s.hdv.alloc(cap);
  }));
  return 0;
}

// Where a side's selection writes its skip bytes: its own array in a pair; alone, side A writes the
// bytes the gathers and the lookup read.
static uint8_t* side_skip(edc_ctx* ctx, const QuorumSide& s, bool pair) { return pair ? s.skip.get() : ctx->sc_hit.get(); }

// votes tier: side A's, and what both sides read
static int ensure_quorum(edc_ctx* ctx, size_t n, size_t nc) {
  QuorumWs& q = ctx->qw;
  GrowSync g{ctx->st()};
  const int rc = side_votes_room(ctx, q.a, n, nc, g);
  if (rc) return rc;
  CK(grow_group(q.cap_c, nc, off_cap, g.c(), [&](size_t cap) { return q.coff.alloc(cap + 1); }));
  CK(grow_group(q.cap_n, n ? n : 1, item_cap, g.n(), [&](size_t cap) {
    const size_t tiles = quorum_tiles(cap);
    return alloc_all(sized(q.cidx, cap), sized(q.aggv, tiles), sized(q.aggf, tiles), sized(q.carry, tiles));
  }));
  if (!q.err) CK(q.err.alloc(1));
  if (!q.h) CK(q.h.alloc(6));
  return 0;
}

// what every form checks on the host first; *n = the item count
static int quorum_check(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* threshold, int mode,
                        size_t* n) {
  int rc = commits_check(ctx, nc, commit_off, n);
  if (rc) return rc;
  if (!threshold) { ctx->err = "null threshold"; return EDC_ERR_ARG; }
  if (!quorum_check_mode(mode)) { ctx->err = "mode is EDC_QUORUM_FULL or EDC_QUORUM_LIGHT"; return EDC_ERR_ARG; }
  return claim_slot0(ctx) ? 0 : EDC_ERR_ARG;
}

// the votes of a host form
static int quorum_check_votes(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* power,
                              const uint8_t* flag) {
  if (!quorum_check_flags(commit_off[nc], flag)) {
    ctx->err = "vote flags: EDC_VOTE_ABSENT, EDC_VOTE_COMMIT or EDC_VOTE_NIL";
    return EDC_ERR_ARG;
  }
  if (!quorum_check_powers(nc, commit_off, power, flag)) {
    ctx->err = "voting power: every power and every commit's counted sum at most 2^63 - 1";
    return EDC_ERR_ARG;
  }
  return 0;
}

// preconditions of every cached quorum entry (edc_cached_*) beyond the uncached form's own
static int cq_ready(edc_ctx* ctx) {
  if (!ctx->sc_cap) { ctx->err = "no signature cache on this context (edc_sigcache_create)"; return EDC_ERR_ARG; }
  return 0;
}

struct QuorumOut {
  uint8_t *commit_verdicts, *item_verdicts;
  uint64_t* tally;
  int* n_bad_commits;
  size_t *n_checked, *n_miss;   // n_miss: the cached entries' (null in the uncached ones)
  uint8_t* check8;
};

// The trusting side (side B) of a paired request: the commits' trust versions (VQ_NO_TRUST: side A
// only) and thresholds, and where side B's verdicts go (all nullable). Host memory. Side B's
// device arrays are the context's tr_* ones, which ensure_trust has sized.
struct QuorumTrust {
  const uint32_t* ver;
  const uint64_t* threshold;
  uint8_t* verdicts;
  uint64_t* tally;
  int* n_bad;
};

// nc == 0: nothing to verify
static int quorum_none(const QuorumOut& out, const QuorumTrust* tr = nullptr) {
  if (out.n_bad_commits) *out.n_bad_commits = 0;
  if (out.n_checked) *out.n_checked = 0;
  if (out.n_miss) *out.n_miss = 0;
  if (tr && tr->n_bad) *tr->n_bad = 0;
  return EDC_OK;
}

// pair tier: side B's votes and join tiers and its versions, each side's own skip bytes, the union's
static int ensure_trust(edc_ctx* ctx, size_t n, size_t nc) {
  QuorumWs& q = ctx->qw;
  QuorumSide& b = q.b;
  GrowSync g{ctx->st()};
  int rc = side_votes_room(ctx, b, n, nc, g);
  if (rc || (rc = side_join_room(ctx, b, n, nc, g))) return rc;
  CK(grow(b.ver, nc, off_cap, g.c()));
  for (DevBuf<uint8_t>* skip : {&q.a.skip, &b.skip, &q.sideb}) CK(grow(*skip, n ? n : 1, item_cap, g.n()));
  if (!q.cnt) CK(q.cnt.alloc(3 * QR_UNION_SLOTS));
  if (!q.hcnt) CK(q.hcnt.alloc(3 * QR_UNION_SLOTS));
  return 0;
}

// What every verify entry does first. True: *rc is the entry's result (a null argument, a cached
// entry without a table, or nc == 0).
static bool quorum_entry_done(edc_ctx* ctx, const uint8_t* z_seed, bool cached, size_t nc, const QuorumOut& out, int* rc) {
  if (!ctx || !z_seed) { *rc = EDC_ERR_ARG; return true; }
  if (cached && (*rc = cq_ready(ctx))) return true;
  if (!nc) { *rc = quorum_none(out); return true; }
  return false;
}

// power and flag of a host form beside the other staged inputs (slot 0's stream)
static int quorum_stage_votes(edc_ctx* ctx, size_t n, size_t nc, const uint64_t* power, const uint8_t* flag) {
  int rc = init_slot(ctx, ctx->slot[0]);
  if (rc || (rc = ensure_quorum(ctx, n, nc)) || !n) return rc;
  CK(hipMemcpyAsync(ctx->qw.a.power, power, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->st()));
  CK(hipMemcpyAsync(ctx->qw.a.flag, flag, n, hipMemcpyHostToDevice, ctx->st()));
  return 0;
}

// The device form's host checks, then k: the caller's, or Item::from for every item, skipped votes
// included (as sc_batch), into kbuf. Shared with edc_cached_quorum_verify_device.
static int quorum_device_inputs(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                const uint64_t* d_power, const uint8_t* d_flag, const uint64_t* threshold, int mode,
                                size_t* n_out, const uint32_t** k_out) {
  size_t n;
  int rc = quorum_check(ctx, nc, commit_off, threshold, mode, &n);
  if (rc) return rc;
  if (n && (!d_vk || !d_sig || (!d_k && !d_msg_off) || !d_power || !d_flag)) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (n && (!aligned16(d_vk) || !aligned16(d_sig) || (d_k && !aligned16(d_k)) || ((uintptr_t)d_power & 7u))) {
    ctx->err = "device vk / sig / k arrays must be 16-byte aligned, d_power 8-byte aligned";
    return EDC_ERR_ARG;
  }
  CK(hipSetDevice(ctx->device));
  const uint32_t* k = reinterpret_cast<const uint32_t*>(d_k);
  if (n && !k) {
    if ((rc = init_slot(ctx, ctx->slot[0])) || (rc = ensure_n(ctx, n))) return rc;
    launch_challenge(ctx->st(), (uint32_t)n, d_vk, d_sig, d_msg, d_msg_off, ctx->kbuf);
    CK(hipGetLastError());
    k = ctx->kbuf;
  }
  *n_out = n;
  *k_out = k;
  return 0;
}

// The host form's checks and staging (keys, signatures, power, flag; k copied or hashed into kbuf,
// all on slot 0's stream). Shared with edc_cached_quorum_verify.
static int quorum_host_inputs(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                              const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                              const uint8_t* k, const uint64_t* power, const uint8_t* flag, const uint64_t* threshold,
                              int mode, size_t* n_out) {
  size_t n;
  int rc = quorum_check(ctx, nc, commit_off, threshold, mode, &n);
  if (rc || (rc = quorum_check_votes(ctx, nc, commit_off, power, flag))) return rc;
  if (n) {
    if ((rc = commits_check_keys(ctx, n, vk, key_idx))) return rc;
    if (!sig) { ctx->err = "null input"; return EDC_ERR_ARG; }
    if ((rc = commits_check_msg_or_k(ctx, n, msg, msg_off, k))) return rc;
    if (k) {                // only a checked vote's k reaches the batch (Scalar::from_hash never yields k >= l)
      std::vector<uint8_t> chk(n);
      quorum_select(nc, commit_off, power, flag, threshold, mode, chk.data(), nullptr);
      for (size_t i = 0; i < n; ++i) {
        uint32_t w[8];
        memcpy(w, k + 32 * i, 32);
        if (chk[i] && w[7] >= 0x10000000u && !sc_is_canonical(w)) {
          ctx->err = "prehashed k is not a canonical scalar (must be < l, as Scalar::from_hash returns)";
          return EDC_ERR_ARG;
        }
      }
    }
  }
  CK(hipSetDevice(ctx->device));
  if ((rc = quorum_stage_votes(ctx, n, nc, power, flag))) return rc;
  hipStream_t st = ctx->st();
  if (k) {
    if ((rc = ensure_n(ctx, n))) return rc;
    if (n) CK(hipMemcpyAsync(ctx->kbuf, k, n * 32, hipMemcpyHostToDevice, st));
  } else if ((rc = upload_msgs(ctx, n, msg, n ? msg_off : nullptr))) {
    return rc;
  }
  if (n) {                  // key indices into cidx, which is free until the selection writes it
    if ((rc = stage_keys_sigs(ctx, st, n, vk, key_idx, sig, ctx->qw.cidx, ctx->vk, ctx->sig))) return rc;
    if (!k) {
      launch_challenge(st, (uint32_t)n, ctx->vk, ctx->sig, ctx->msg, ctx->off, ctx->kbuf);
      CK(hipGetLastError());
    }
  }
  *n_out = n;
  return 0;
}

// One side's selection, as quorum_select_enqueue and the timing hook both launch it, on that side's
// power / flag (side A's may be the caller's own device arrays) against its thresholds into `skip`
// (side_skip) and its plan. Side B's (side_b) reads the commit indices side A's has written.
static void quorum_side_launch(edc_ctx* ctx, hipStream_t st, size_t n, size_t nc, int mode, const QuorumSide& s,
                               const uint64_t* d_power, const uint8_t* d_flag, uint8_t* skip, bool side_b) {
  const QuorumWs& q = ctx->qw;
  launch_quorum_select(st, (uint32_t)n, (uint32_t)nc, mode == QUORUM_LIGHT, q.coff, s.thr, d_power, d_flag, q.cidx, q.aggv,
                       q.aggf, q.carry, skip, ctx->sc_wg, s.planned, q.err, side_b);
}

// Side B's selection of a pair behind side A's, between the clearing of the union's counts and the
// union kernel, which writes the skip bytes and tile counts every back-end reads.
static hipError_t quorum_side_b_launch(edc_ctx* ctx, hipStream_t st, size_t n, size_t nc, int mode) {
  const QuorumWs& q = ctx->qw;
  const QuorumSide& b = q.b;
  const hipError_t e = hipMemsetAsync(q.cnt, 0, 3 * QR_UNION_SLOTS * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  quorum_side_launch(ctx, st, n, nc, mode, b, b.power, b.flag, b.skip, true);
  launch_quorum_union(st, (uint32_t)n, q.a.skip, b.skip, ctx->sc_hit, q.sideb, ctx->sc_wg, q.cnt);
  return hipSuccess;
}

// Workspace, the staged offsets and thresholds, then the selection and the scan of its workgroup
// counts on device-resident power / flag, all enqueued. A form with work of its own behind the
// selection (n > 0 only) enqueues it between this and quorum_select_read.
// tr (a trusting pair; ensure_trust has run and the paired join has written side B's power / flag):
// each side's selection writes its own skip bytes, side B's behind side A's against tr->threshold,
// reading the commit indices and reusing the tile words of side A's (one stream: side A is done
// with them), and both raise the one error flag; the union kernel then writes the skip bytes and
// tile counts every back-end reads, so that the scan, the gathers and the lookup see ONE selection,
// the union's. Its totals {A, B, both} travel to hcnt with the read-back.
static int quorum_select_enqueue(edc_ctx* ctx, size_t n, size_t nc, const uint32_t* commit_off, const uint64_t* threshold,
                                 int mode, const uint64_t* d_power, const uint8_t* d_flag, const QuorumTrust* tr = nullptr) {
  int rc = init_slot(ctx, ctx->slot[0]);
  if (rc || (rc = ensure_quorum(ctx, n, nc)) || (rc = ensure_sc(ctx, n ? n : 1))) return rc;
  hipStream_t st = ctx->st();
  if ((rc = sc_order_after_inserts(ctx, st))) return rc;
  QuorumWs& q = ctx->qw;
  QuorumSide &a = q.a, &b = q.b;
  CK(hipMemsetAsync(a.planned, 0, nc * sizeof(uint64_t), st));
  if (tr) {
    CK(hipMemsetAsync(b.planned, 0, nc * sizeof(uint64_t), st));
    memset(q.hcnt.get(), 0, 3 * QR_UNION_SLOTS * sizeof(uint32_t));
  }
  if (!n) return 0;
  const uint32_t nwg = (uint32_t)quorum_tiles(n);
  CK(hipMemcpyAsync(q.coff, commit_off, (nc + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(a.thr, threshold, nc * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  CK(hipMemsetAsync(q.err, 0, sizeof(int), st));
  quorum_side_launch(ctx, st, n, nc, mode, a, d_power, d_flag, side_skip(ctx, a, tr != nullptr), false);
  if (tr) {
    CK(hipMemcpyAsync(b.thr, tr->threshold, nc * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    CK(quorum_side_b_launch(ctx, st, n, nc, mode));
    CK(hipMemcpyAsync(q.hcnt.get(), q.cnt, 3 * QR_UNION_SLOTS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  launch_sc_scan(st, nwg, ctx->sc_wg, ctx->sc_wg + nwg);
  CK(hipGetLastError());
  q.h[0] = q.h[1] = q.h[2] = 0;
  return 0;
}

// The one read-back behind quorum_select_enqueue: the device checks' flag and the checked count
// (*n_checked, the size of the gathered list), with whatever else the form sent to h. A vote the
// device checks refuse is EDC_ERR_ARG here, before anything is gathered or verified. flag_msg: a
// templated form's all-n checks raise err too (bit 1 for the holes), so it words bit 0 itself.
static int quorum_select_read(edc_ctx* ctx, size_t n, size_t* n_checked, const char* flag_msg = nullptr) {
  *n_checked = 0;
  if (!n) return 0;
  hipStream_t st = ctx->st();
  QuorumWs& q = ctx->qw;
  const uint32_t nwg = (uint32_t)quorum_tiles(n);
  CK(hipMemcpyAsync(&q.h[0], q.err, sizeof(int), hipMemcpyDeviceToHost, st));
  CK(hipMemcpyAsync(&q.h[1], ctx->sc_wg + nwg, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  if (q.h[0] & 2) {
    ctx->err = "templated items: hole offsets out of range";
    return EDC_ERR_ARG;
  }
  if (q.h[0]) {
    ctx->err = "votes: a flag above 2, a power above 2^63 - 1 or a commit whose counted power passes 2^63 - 1";
    if (flag_msg) ctx->err = flag_msg;
    return EDC_ERR_ARG;
  }
  if (q.h[1] > n) { ctx->err = "quorum selection: checked count out of range"; return EDC_ERR_HIP; }
  *n_checked = q.h[1];
  return 0;
}

// the selection with nothing behind it
static int quorum_select_run(edc_ctx* ctx, size_t n, size_t nc, const uint32_t* commit_off, const uint64_t* threshold,
                             int mode, const uint64_t* d_power, const uint8_t* d_flag, size_t* n_checked) {
  int rc = quorum_select_enqueue(ctx, n, nc, commit_off, threshold, mode, d_power, d_flag);
  return rc ? rc : quorum_select_read(ctx, n, n_checked);
}

// Optional stages around the selection (edc_vq_verify): the validator-set join in front of it,
// writing side A's power / flag, and the double-vote scan behind it, whose bytes travel to hdv in
// the selection's read-back. d_vk: the n keys on the device, or null with d_kidx their positions;
// d_flag: the caller's flags; cver (host): the commits' versions, null for the one set;
// host_k: a host form's prehashed k, canonical for the checked votes (quorum_join_check_k).
// trust: the trusting side of a paired request (needs cver), one more optional input of the same
// stages: the paired join writes both sides, the selection and the double-vote scan run per side,
// and the skip bytes are the union's. valset_room has run.
struct QuorumJoin {
  const uint8_t* d_vk;
  const uint32_t* d_kidx;
  const uint8_t* d_flag;
  const uint32_t* cver;
  const uint8_t* host_k;
  std::vector<uint8_t> skip;    // host_k: the skip bytes, read back with the selection
  const QuorumTrust* trust = nullptr;
};

static const char kJoinFlagMsg[] = "votes: a flag above 2 or a commit whose counted power passes 2^63 - 1";

// join tier: side A's, and the host forms' staging (edc_valset_* / edc_vhist_* / edc_vq_*, below)
static int ensure_valset(edc_ctx* ctx, size_t n, size_t nc) {
  QuorumWs& q = ctx->qw;
  GrowSync g{ctx->st()};
  const int rc = side_join_room(ctx, q.a, n, nc, g);
  if (rc) return rc;
  CK(grow_group(q.join_n, n ? n : 1, item_cap, g.n(), [&](size_t cap) { return alloc_all(sized(q.kidx, cap), sized(q.vflag, cap)); }));
  return 0;
}

static int valset_ready(edc_ctx* ctx) {
  if (!ctx->vs_m) { ctx->err = "no voting powers on the registered list (edc_valset_set_powers)"; return EDC_ERR_ARG; }
  return 0;
}

// a history is set and every commit names one of its versions
static int vhist_ready(edc_ctx* ctx, size_t nc, const uint32_t* cver) {
  if (!ctx->vh.m) { ctx->err = "no validator-set history on the registered list (edc_vhist_set)"; return EDC_ERR_ARG; }
  for (size_t c = 0; c < nc; ++c)
    if (cver[c] > ctx->vh.nv) { ctx->err = "commit_ver: a version past the history's last"; return EDC_ERR_ARG; }
  return 0;
}

// Workspace for n items in nc commits on slot 0; everything the selection allocates is allocated
// here, so that nothing the resolve kernel has written moves afterwards.
static int valset_room(edc_ctx* ctx, size_t n, size_t nc, bool hist = false, bool pair = false) {
  int rc = init_slot(ctx, ctx->slot[0]);
  if (rc || (rc = ensure_quorum(ctx, n, nc)) || (rc = ensure_sc(ctx, n ? n : 1))) return rc;
  if (pair && (rc = ensure_trust(ctx, n, nc))) return rc;
  if (hist) CK(grow(ctx->qw.a.ver, nc, off_cap, sync_of(ctx->st())));
  return ensure_valset(ctx, n, nc);
}

// The join kernel of jn, as valset_select_enqueue and the timing hooks both launch it: the one
// set's, the history's (cver) or the paired one (cver and trust), which writes side B's arrays too.
// The history's read coff and each side's ver, which the caller has staged.
static void valset_join_launch(edc_ctx* ctx, hipStream_t st, size_t n, size_t nc, const QuorumJoin& jn) {
  const uint32_t N = (uint32_t)n, NC = (uint32_t)nc;
  const QuorumWs& q = ctx->qw;
  const QuorumSide &a = q.a, &b = q.b;
  if (jn.cver && jn.trust)
    launch_vhist_resolve2(st, N, NC, ctx->kc(), ctx->vhv(), q.coff, a.ver, b.ver, jn.d_vk, jn.d_kidx, ctx->kc_reg, jn.d_flag,
                          a.power, a.flag, a.who, b.power, b.flag, b.who);
  else if (jn.cver)
    launch_vhist_resolve(st, N, NC, ctx->kc(), ctx->vhv(), q.coff, a.ver, jn.d_vk, jn.d_kidx, ctx->kc_reg, jn.d_flag, a.power,
                         a.flag, a.who);
  else
    launch_valset_resolve(st, N, ctx->kc(), ctx->vs(), jn.d_vk, jn.d_kidx, ctx->kc_reg, jn.d_flag, a.power, a.flag, a.who);
}

// One side's double-vote scan of n > 0 votes on its skip bytes (side_skip), members and set, with
// the clearing of its set and bytes, as every call and the timing hooks run it.
static hipError_t valset_pairs_launch(edc_ctx* ctx, hipStream_t st, size_t n, size_t nc, const QuorumSide& s,
                                      const uint8_t* skip) {
  hipError_t e = hipMemsetAsync(s.dv, 0, nc, st);
  if (e != hipSuccess || (e = hipMemsetAsync(s.set, 0, 2 * n * sizeof(uint64_t), st)) != hipSuccess) return e;
  launch_valset_pairs(st, (uint32_t)n, ctx->qw.coff, ctx->qw.cidx, skip, s.who, s.set, s.dv);
  return hipSuccess;
}

// The join, the selection and the double-vote scan of n votes whose keys (jn->d_vk, or jn->d_kidx
// with d_vk null) and flags are on the device, enqueued with the copies quorum_select_read's one
// read-back then brings: each side's double-vote bytes in its hdv and, for a host form's prehashed
// k, the n skip bytes in jn->skip. valset_room has run.
// jn->trust (a trusting pair, with cver): the paired join writes side B's arrays beside side A's,
// the selection runs per side and leaves the union's skip bytes (quorum_select_enqueue), and the
// double-vote scan runs once per side.
static int valset_select_enqueue(edc_ctx* ctx, size_t n, size_t nc, const uint32_t* commit_off, const uint64_t* threshold,
                                 int mode, QuorumJoin* jn) {
  hipStream_t st = ctx->st();
  const QuorumTrust* tr = jn->trust;
  QuorumWs& q = ctx->qw;
  QuorumSide &a = q.a, &b = q.b;
  jn->skip.assign(jn->host_k ? n : 0, 0);
  if (jn->cver && n) {  // the history's join reads the offsets, which the selection stages (again) only behind it
    CK(hipMemcpyAsync(q.coff, commit_off, (nc + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(a.ver, jn->cver, nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (tr) CK(hipMemcpyAsync(b.ver, tr->ver, nc * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  valset_join_launch(ctx, st, n, nc, *jn);
  CK(hipGetLastError());
  int rc = quorum_select_enqueue(ctx, n, nc, commit_off, threshold, mode, a.power, a.flag, tr);
  if (rc) return rc;
  memset(a.hdv, 0, nc);
  if (tr) memset(b.hdv, 0, nc);
  if (n) {
    CK(valset_pairs_launch(ctx, st, n, nc, a, side_skip(ctx, a, tr != nullptr)));
    if (tr) {
      CK(valset_pairs_launch(ctx, st, n, nc, b, b.skip));
      CK(hipMemcpyAsync(b.hdv, b.dv, nc, hipMemcpyDeviceToHost, st));
    }
    CK(hipGetLastError());
    CK(hipMemcpyAsync(a.hdv, a.dv, nc, hipMemcpyDeviceToHost, st));
    if (!jn->skip.empty()) CK(hipMemcpyAsync(jn->skip.data(), ctx->sc_hit, n, hipMemcpyDeviceToHost, st));
  }
  return 0;
}

// valset_select_enqueue and its read-back: *n_checked
static int valset_select(edc_ctx* ctx, size_t n, size_t nc, const uint32_t* commit_off, const uint64_t* threshold,
                         int mode, QuorumJoin* jn, size_t* n_checked) {
  int rc = valset_select_enqueue(ctx, n, nc, commit_off, threshold, mode, jn);
  return rc ? rc : quorum_select_read(ctx, n, n_checked, kJoinFlagMsg);
}

// quorum_select_enqueue, with the join in front and the double-vote scan behind it when jn is given
// (d_power / d_flag are then side A's, which the join writes)
static int quorum_front_enqueue(edc_ctx* ctx, size_t n, size_t nc, const uint32_t* commit_off, const uint64_t* threshold,
                                int mode, const uint64_t* d_power, const uint8_t* d_flag, QuorumJoin* jn) {
  if (jn) return valset_select_enqueue(ctx, n, nc, commit_off, threshold, mode, jn);
  return quorum_select_enqueue(ctx, n, nc, commit_off, threshold, mode, d_power, d_flag);
}

// behind the read-back: Scalar::from_hash never yields k >= l, so a checked vote's k must be canonical
static int quorum_join_check_k(edc_ctx* ctx, const QuorumJoin* jn) {
  if (!jn) return 0;
  // One test per vote on its top word and skip byte, without a branch on the skip byte alone: in light
  // mode the skip bytes change every few dozen votes, and a loop that branched on them took a
  // millisecond longer over 2^20 votes (profiles/valset_refactor_bench.log, the probe section and the
  // earlier sessions; DESIGN.md, "Validator-set requests").
  const uint8_t *skip = jn->skip.data(), *k = jn->host_k;
  for (size_t i = 0, n = jn->skip.size(); i < n; ++i) {
    uint32_t w7, w[8];
    memcpy(&w7, k + 32 * i + 28, 4);
    if (!((w7 >= 0x10000000u) & !skip[i])) continue;
    memcpy(w, k + 32 * i, 32);
    if (!sc_is_canonical(w)) {
      ctx->err = "prehashed k is not a canonical scalar (must be < l, as Scalar::from_hash returns)";
      return EDC_ERR_ARG;
    }
  }
  return 0;
}

// Device arrays of `count` items (keys, signatures, k). idx: where each stands in the list it was
// gathered from; null: it is that list.
struct ItemList {
  const uint8_t *vk, *sig;
  const uint32_t *k, *idx;
  size_t count;
};

// where a gather puts what it keeps: vk | sig | k of cap items each, and the positions
struct GatherArea {
  uint8_t* g;
  size_t cap;
  uint32_t* idx;
};

static GatherArea sc_area(edc_ctx* ctx) { return GatherArea{ctx->sc_g, ctx->sc_cap_n, ctx->sc_idx}; }

// The `keep` items of `in` that leave[] does not mark (wg: its scanned workgroup counts), packed
// into `to` in list order. All kept: `in` itself, nothing moves. None kept: an empty list still
// runs the n = 0 batch, whose k is never read.
static int quorum_gather(edc_ctx* ctx, const ItemList& in, size_t keep, const uint8_t* leave, const uint32_t* wg,
                         const GatherArea& to, ItemList* out) {
  *out = ItemList{in.vk, in.sig, keep ? in.k : reinterpret_cast<const uint32_t*>(ctx->sc_hit.get()), nullptr, keep};
  if (!keep || keep == in.count) return 0;
  uint8_t* g_sig = to.g + to.cap * 32;
  uint32_t* g_k = reinterpret_cast<uint32_t*>(g_sig + to.cap * 64);
  launch_sc_compact(ctx->st(), (uint32_t)in.count, leave, wg, in.vk, in.sig, in.k, to.idx, to.g, g_sig, g_k);
  CK(hipGetLastError());
  *out = ItemList{to.g, g_sig, g_k, to.idx, keep};
  return 0;
}

// What a cached form (edc_cached_*) adds to quorum_finish. The list it hands over holds the checked
// MISSES of a looked-up list `mid`: all n items in the plain forms (mid.idx null), the gathered
// checked votes in the templated ones (mid.idx: their queue positions). quorum_finish's list
// indexes mid's arrays, and the insert reads them. codes: the lookup's base codes of mid's items
// (device; 255 not checked, else 0).
struct QuorumCached {
  size_t n_checked;
  uint8_t* codes;
  ItemList mid;
};

// The gathered list (in queue order; list.idx null when it holds all n items or none) through the
// batch and its fallback, then the tally and the verdicts of all n items / nc commits.
// cq (a cached form): the list is the checked misses; what it proves valid is inserted (every miss
// after a passing union, the misses with code 0 after a failed one) before the last
// synchronization, and a failed union's codes go back over the lookup's base codes, through the
// list's positions in the looked-up list and that list's positions in the queue.
// dv (a validator-set form, host, nc bytes): the commits that hold a double vote (valset_reduce).
// tr (a trusting pair): the list is the union of both sides' checked votes. A passing union makes
// each side's tally its planned[]; a failed one runs the tally kernel for both sides at once, each
// masked by its bit of the side bytes. Side B is reduced with its own double-vote bytes, and the
// return value is taken over both sides.
static int quorum_finish(edc_ctx* ctx, size_t nc, const uint64_t* threshold, size_t n, const ItemList& list,
                         const uint64_t* d_power, const uint8_t* d_flag, const uint8_t* z_seed, const QuorumOut& out,
                         const QuorumCached* cq = nullptr, const uint8_t* dv = nullptr, const QuorumTrust* tr = nullptr) {
  hipStream_t st = ctx->st();
  QuorumWs& q = ctx->qw;
  const int sides = tr ? 2 : 1;
  const size_t m = list.count;
  std::vector<uint8_t> mv(m ? m : 1);
  const BatchIn in{list.vk, list.sig, nullptr, nullptr, list.k, z_seed, 0, nullptr, false};
  const int code = batch_with_fallback(ctx, m, in, mv.data(), nullptr, out.check8);
  if (code < 0) return code;
  const unsigned long long ins0 = cq ? ctx->sc_hctr[0] : 0;
  if (cq && m) {
    if (code != EDC_OK) CK(hipMemcpyAsync(ctx->sc_mverd, mv.data(), m, hipMemcpyHostToDevice, st));
    launch_sc_insert(st, ctx->sc(), (uint32_t)m, list.idx, cq->mid.vk, cq->mid.sig, cq->mid.k,
                     code == EDC_OK ? nullptr : ctx->sc_mverd.get(), ctx->sc_ctr);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->sc_hctr, ctx->sc_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  }
  std::vector<uint64_t> tal[2];
  std::vector<uint8_t> cor[2];
  for (int j = 0; j < sides; ++j) tal[j].resize(nc);
  if (code == EDC_OK) {                 // every checked item verified: the tally is the plan
    for (int j = 0; j < sides; ++j)
      CK(hipMemcpyAsync(tal[j].data(), q.side[j].planned, nc * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (out.item_verdicts && n) CK(hipMemcpyAsync(out.item_verdicts, ctx->sc_hit, n, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    if (out.item_verdicts)
      for (size_t i = 0; i < n; ++i) out.item_verdicts[i] = out.item_verdicts[i] ? QUORUM_NOT_CHECKED : 0;
  } else {                              // m > 0: codes back to queue order, then the tally kernel
    const uint8_t* d_codes = ctx->sc_mverd;
    if (!cq) {
      CK(hipMemcpyAsync(ctx->sc_mverd, mv.data(), m, hipMemcpyHostToDevice, st));
      if (list.idx) {
        CK(hipMemsetAsync(ctx->sc_verd, QUORUM_NOT_CHECKED, n, st));
        launch_sc_scatter(st, (uint32_t)m, list.idx, ctx->sc_mverd, ctx->sc_verd);
        d_codes = ctx->sc_verd;
      }
    } else {                            // sc_mverd holds the misses' codes already
      if (list.idx) {                   // hits keep the base code 0
        launch_sc_scatter(st, (uint32_t)m, list.idx, ctx->sc_mverd, cq->codes);
        d_codes = cq->codes;
      }
      if (cq->mid.idx) {
        CK(hipMemsetAsync(ctx->sc_verd, QUORUM_NOT_CHECKED, n, st));
        launch_sc_scatter(st, (uint32_t)cq->mid.count, cq->mid.idx, d_codes, ctx->sc_verd);
        d_codes = ctx->sc_verd;
      }
    }
    const QuorumSide &a = q.a, &b = q.b;
    for (int j = 0; j < sides; ++j) {
      CK(hipMemsetAsync(q.side[j].tally, 0, nc * sizeof(uint64_t), st));
      CK(hipMemsetAsync(q.side[j].cor, 0, nc * sizeof(uint32_t), st));
    }
    if (tr)
      launch_quorum_tally2(st, (uint32_t)n, q.cidx, q.sideb, d_power, d_flag, b.power, b.flag, d_codes, a.tally, a.cor, b.tally,
                           b.cor);
    else
      launch_quorum_tally(st, (uint32_t)n, q.cidx, d_power, d_flag, d_codes, a.tally, a.cor);
    CK(hipGetLastError());
    std::vector<uint32_t> cor32[2];
    for (int j = 0; j < sides; ++j) {
      cor32[j].resize(nc);
      CK(hipMemcpyAsync(tal[j].data(), q.side[j].tally, nc * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
      CK(hipMemcpyAsync(cor32[j].data(), q.side[j].cor, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if (out.item_verdicts) CK(hipMemcpyAsync(out.item_verdicts, d_codes, n, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    for (int j = 0; j < sides; ++j) {
      cor[j].resize(nc);
      for (size_t c = 0; c < nc; ++c) cor[j][c] = cor32[j][c] ? 1 : 0;
    }
  }
  size_t bad = 0;
  const uint8_t* corp = cor[0].empty() ? nullptr : cor[0].data();
  int res = dv ? valset_reduce(nc, corp, tal[0].data(), threshold, dv, out.commit_verdicts, &bad)
               : quorum_reduce(nc, corp, tal[0].data(), threshold, out.commit_verdicts, &bad);
  if (tr) {
    size_t bad_b = 0;
    const int res_b = vq_trust_reduce(nc, tr->ver, cor[1].empty() ? nullptr : cor[1].data(), tal[1].data(), tr->threshold,
                                      q.b.hdv, tr->verdicts, &bad_b);
    res = vq_trust_code(res, res_b);
    if (tr->tally) memcpy(tr->tally, tal[1].data(), nc * sizeof(uint64_t));
    if (tr->n_bad) *tr->n_bad = (int)bad_b;
    uint64_t a = 0, b = 0, ab = 0;        // the union kernel's totals, spread over its slots
    for (uint32_t j = 0; j < QR_UNION_SLOTS; ++j) {
      a += q.hcnt[3 * j];
      b += q.hcnt[3 * j + 1];
      ab += q.hcnt[3 * j + 2];
    }
    const uint64_t last[4] = {a, b, ab, a + b - ab};
    memcpy(q.vqt_last, last, sizeof(last));
    q.vqt_have = true;
  }
  if (out.tally) memcpy(out.tally, tal[0].data(), nc * sizeof(uint64_t));
  if (out.n_bad_commits) *out.n_bad_commits = (int)bad;
  if (out.n_checked) *out.n_checked = cq ? cq->n_checked : m;
  if (cq) {
    if (out.n_miss) *out.n_miss = m;
    q.cq_last[3] = m;
    q.cq_last[5] = ctx->sc_hctr[0] - ins0;
  }
  return res;
}

// A checked quorum commit set whose items (all: vk, sig, k of the n votes; power, flag) are on the
// device. jn (a validator-set form): power and flag are side A's, which the join writes.
static int quorum_run(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* threshold, int mode,
                      const ItemList& all, const uint64_t* d_power, const uint8_t* d_flag, const uint8_t* z_seed,
                      const QuorumOut& out, QuorumJoin* jn = nullptr) {
  const size_t n = all.count;
  size_t m = 0;
  ItemList list;
  int rc = quorum_front_enqueue(ctx, n, nc, commit_off, threshold, mode, d_power, d_flag, jn);
  if (rc || (rc = quorum_select_read(ctx, n, &m, jn ? kJoinFlagMsg : nullptr)) || (rc = quorum_join_check_k(ctx, jn)) ||
      (rc = quorum_gather(ctx, all, m, ctx->sc_hit, ctx->sc_wg, sc_area(ctx), &list)))
    return rc;
  return quorum_finish(ctx, nc, threshold, n, list, d_power, d_flag, z_seed, out, nullptr, jn ? ctx->qw.a.hdv.get() : nullptr,
                       jn ? jn->trust : nullptr);
}

extern "C" {

int edc_quorum_plan(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* power, const uint8_t* flag,
                    const uint64_t* threshold, int mode, uint8_t* checked, uint64_t* planned, size_t* n_checked) {
  if (!ctx) return EDC_ERR_ARG;
  if (!nc) {
    if (n_checked) *n_checked = 0;
    return EDC_OK;
  }
  size_t n, m = 0;
  int rc = quorum_check(ctx, nc, commit_off, threshold, mode, &n);
  if (rc || (rc = quorum_check_votes(ctx, nc, commit_off, power, flag))) return rc;
  CK(hipSetDevice(ctx->device));
  if ((rc = quorum_stage_votes(ctx, n, nc, power, flag)) ||
      (rc = quorum_select_run(ctx, n, nc, commit_off, threshold, mode, ctx->qw.a.power, ctx->qw.a.flag, &m)))
    return rc;
  hipStream_t st = ctx->st();
  if (planned) CK(hipMemcpyAsync(planned, ctx->qw.a.planned, nc * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (checked && n) CK(hipMemcpyAsync(checked, ctx->sc_hit, n, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  if (checked)
    for (size_t i = 0; i < n; ++i) checked[i] = checked[i] ? 0 : 1;      // the kernel writes the skip byte
  if (n_checked) *n_checked = m;
  return EDC_OK;
}

int edc_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                             const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                             const uint64_t* d_power, const uint8_t* d_flag, const uint64_t* threshold, int mode,
                             const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                             int* n_bad_commits, size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, false, nc, out, &rc)) return rc;
  size_t n;
  const uint32_t* k;
  if ((rc = quorum_device_inputs(ctx, nc, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k, d_power, d_flag, threshold, mode,
                                 &n, &k)))
    return rc;
  return quorum_run(ctx, nc, commit_off, threshold, mode, ItemList{d_vk, d_sig, k, nullptr, n}, d_power, d_flag, z_seed,
                    out);
}

int edc_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk, const uint32_t* key_idx,
                      const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k,
                      const uint64_t* power, const uint8_t* flag, const uint64_t* threshold, int mode,
                      const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                      int* n_bad_commits, size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, false, nc, out, &rc)) return rc;
  size_t n;
  if ((rc = quorum_host_inputs(ctx, nc, commit_off, vk, key_idx, sig, msg, msg_off, k, power, flag, threshold, mode, &n)))
    return rc;
  return quorum_run(ctx, nc, commit_off, threshold, mode, ItemList{ctx->vk, ctx->sig, ctx->kbuf, nullptr, n}, ctx->qw.a.power,
                    ctx->qw.a.flag, z_seed, out);
}

int edc_debug_quorum_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* power,
                            const uint8_t* flag, const uint64_t* threshold, int mode, int reps, float* ms) {
  if (!ctx || reps < 1) return EDC_ERR_ARG;
  if (ms) *ms = 0.f;
  if (!nc) return EDC_OK;
  size_t n, m = 0;
  int rc = quorum_check(ctx, nc, commit_off, threshold, mode, &n);
  if (rc || (rc = quorum_check_votes(ctx, nc, commit_off, power, flag))) return rc;
  CK(hipSetDevice(ctx->device));
  if ((rc = quorum_stage_votes(ctx, n, nc, power, flag)) ||
      (rc = quorum_select_run(ctx, n, nc, commit_off, threshold, mode, ctx->qw.a.power, ctx->qw.a.flag, &m)))
    return rc;
  if (!n) return EDC_OK;
  hipStream_t st = ctx->st();
  Event e0, e1;
  CK(e0.create());
  CK(e1.create());
  CK(hipEventRecord(e0, st));
  for (int r = 0; r < reps; ++r)        // planned is a maximum: repeating the launch leaves it unchanged
    quorum_side_launch(ctx, st, n, nc, mode, ctx->qw.a, ctx->qw.a.power, ctx->qw.a.flag, ctx->sc_hit, false);
  CK(hipGetLastError());
  CK(hipEventRecord(e1, st));
  CK(hipEventSynchronize(e1));
  float t = 0.f;
  CK(hipEventElapsedTime(&t, e0, e1));
  if (ms) *ms = t / (float)reps;
  return EDC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- templated quorum commit sets
// edc_tmpl_quorum_*: select first. The selection needs only power, flag and the offsets, so it runs
// before any message exists; behind it, in front of the one read-back, the all-n template map
// (k_tmpl_commit_map_alt, which checks the variant bytes) and k_tq_holes (which checks the hole
// offsets and sums the checked holes per tile). The read-back then carries the flag, the checked
// count m and the checked hole bytes. k_tq_gather packs the m checked votes (keys, signatures,
// template indices, holes) in queue order, the expansion and SHA-512 run on those m items into an
// arena sized from m (tmpl_quorum_list), and quorum_finish does what it does for every quorum form.
// m == n: nothing is gathered, the caller's arrays are the list. All on slot 0.
// The cached forms (edc_cached_tmpl_quorum_*) look the hashed list up before the batch: see
// cached_tmpl_finish below.
struct TmplQuorumItems {       // device arrays of all n items
  const uint8_t *vk, *sig, *item_alt, *var;
  const uint32_t* var_off;
  size_t var_bytes;
  const uint64_t* power;
  const uint8_t* flag;
};

// The device form's host checks, shared with edc_cached_tmpl_quorum_verify_device.
static int tmpl_quorum_device_inputs(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                     const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                     const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                     const uint32_t* d_var_off, size_t var_bytes, const uint64_t* d_power,
                                     const uint8_t* d_flag, const uint64_t* threshold, int mode, TmplShape* sh, size_t* n,
                                     TmplQuorumItems* it) {
  int rc = commits_check_tmpl_device(ctx, ts, nc, commit_off, commit_tpl, alt_span, d_vk, d_sig, d_var, d_var_off,
                                     var_bytes, sh, n);
  if (rc || (rc = quorum_check(ctx, nc, commit_off, threshold, mode, n))) return rc;
  if (*n && (!d_power || !d_flag)) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (*n && ((uintptr_t)d_power & 7u)) { ctx->err = "d_power must be 8-byte aligned"; return EDC_ERR_ARG; }
  CK(hipSetDevice(ctx->device));
  *it = TmplQuorumItems{d_vk, d_sig, d_item_alt, d_var, d_var_off, var_bytes, d_power, d_flag};
  return 0;
}

// var_off | item_alt | var of n > 0 host items staged in one piece, each at a 16-byte boundary
static int tmpl_quorum_stage_holes(edc_ctx* ctx, size_t n, const uint8_t* item_alt, const uint8_t* var,
                                   const uint32_t* var_off, TmplQuorumItems* it) {
  hipStream_t st = ctx->st();
  const size_t var_bytes = var_off[n], o_alt = up16(4 * (n + 1)), o_var = up16(o_alt + n);
  int rc = tmpl_room(ctx, st, ctx->qw.tq_in, o_var + var_bytes);
  if (rc) return rc;
  CK(hipMemcpyAsync(ctx->qw.tq_in, var_off, 4 * (n + 1), hipMemcpyHostToDevice, st));
  if (item_alt) CK(hipMemcpyAsync(ctx->qw.tq_in + o_alt, item_alt, n, hipMemcpyHostToDevice, st));
  if (var_bytes) CK(hipMemcpyAsync(ctx->qw.tq_in + o_var, var, var_bytes, hipMemcpyHostToDevice, st));
  it->item_alt = item_alt ? ctx->qw.tq_in + o_alt : nullptr;
  it->var = ctx->qw.tq_in + o_var;
  it->var_off = reinterpret_cast<const uint32_t*>(ctx->qw.tq_in.get());
  it->var_bytes = var_bytes;
  return 0;
}

// The host form's checks and staging, shared with edc_cached_tmpl_quorum_verify.
static int tmpl_quorum_host_inputs(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                   const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt,
                                   const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var,
                                   const uint32_t* var_off, const uint64_t* power, const uint8_t* flag,
                                   const uint64_t* threshold, int mode, TmplShape* sh_out, size_t* n_out,
                                   TmplQuorumItems* it_out) {
  TmplShape sh;
  size_t n;
  int rc = commits_check_tmpl(ctx, ts, nc, commit_off, commit_tpl, true, alt_span, item_alt, vk, key_idx, sig, var, var_off,
                              &sh, &n);
  if (rc || (rc = quorum_check(ctx, nc, commit_off, threshold, mode, &n)) ||
      (rc = quorum_check_votes(ctx, nc, commit_off, power, flag)))
    return rc;
  CK(hipSetDevice(ctx->device));
  if ((rc = quorum_stage_votes(ctx, n, nc, power, flag)) || (rc = ensure_n(ctx, n))) return rc;
  hipStream_t st = ctx->st();
  TmplQuorumItems it{ctx->vk, ctx->sig, nullptr, nullptr, nullptr, 0, ctx->qw.a.power, ctx->qw.a.flag};
  if (n) {
    // key indices into cidx, which is free until the selection writes it
    if ((rc = tmpl_quorum_stage_holes(ctx, n, item_alt, var, var_off, &it)) ||
        (rc = stage_keys_sigs(ctx, st, n, vk, key_idx, sig, ctx->qw.cidx, ctx->vk, ctx->sig)))
      return rc;
  }
  *sh_out = sh;
  *n_out = n;
  *it_out = it;
  return 0;
}

// The selection, then the m checked votes gathered and hashed: *list holds them with their k in
// kbuf. From the expansion on, the slot's template workspace is armed (w.check): whoever runs the
// batch on the list ends with tmpl_quorum_done. jn (a validator-set request): the join runs in front
// of the selection and the double-vote scan behind it, in front of the template map.
static int tmpl_quorum_list(edc_ctx* ctx, const edc_templates* ts, const TmplShape& sh, size_t nc,
                            const uint32_t* commit_off, const uint16_t* commit_tpl, uint32_t alt_span, size_t n,
                            const TmplQuorumItems& it, const uint64_t* threshold, int mode, ItemList* list,
                            QuorumJoin* jn = nullptr) {
  Slot& s = ctx->slot[0];
  TmplWs& w = s.tw;
  int rc = init_slot(ctx, s);
  if (rc) return rc;
  hipStream_t st = ctx->st();
  TmplView view;
  if ((rc = tmpl_upload_set(ctx, w, st, ts, sh, &view))) return rc;
  const uint32_t nwg = (uint32_t)quorum_tiles(n);
  if ((rc = tmpl_room(ctx, st, ctx->qw.tq_tpl, n)) || (rc = tmpl_room(ctx, st, ctx->qw.tq_ctpl, nc)) ||
      (rc = tmpl_room(ctx, st, ctx->qw.tq_wgh, (size_t)nwg + 1)))
    return rc;
  if (!ctx->qw.tq_harena) CK(ctx->qw.tq_harena.alloc(1));
  if ((rc = quorum_front_enqueue(ctx, n, nc, commit_off, threshold, mode, it.power, it.flag, jn))) return rc;
  if (n) {                      // behind the selection: the all-n checks and the checked hole bytes
    CK(hipMemcpyAsync(ctx->qw.tq_ctpl, commit_tpl, nc * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    launch_tmpl_commit_map_alt(st, (uint32_t)n, (uint32_t)nc, ctx->qw.coff, ctx->qw.tq_ctpl, alt_span, it.item_alt, ctx->qw.tq_tpl,
                               ctx->qw.err);
    launch_tmpl_quorum_holes(st, (uint32_t)n, ctx->sc_hit, it.var_off, it.var_bytes, ctx->qw.tq_wgh, ctx->qw.err);
    launch_sc_scan(st, nwg, ctx->qw.tq_wgh, ctx->qw.tq_wgh + nwg);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(&ctx->qw.h[2], ctx->qw.tq_wgh + nwg, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  size_t m = 0;
  rc = quorum_select_read(
      ctx, n, &m,
      "votes: a flag above 2, a power or a commit's counted power above 2^63 - 1, or an item_alt[i] >= alt_span");
  if (rc) return rc;
  const size_t holes = m ? ctx->qw.h[2] : 0;
  if (holes > it.var_bytes) { ctx->err = "quorum selection: checked hole bytes out of range"; return EDC_ERR_HIP; }
  ctx->qw.tq_have = true;
  ctx->qw.tq_last[0] = n;
  ctx->qw.tq_last[1] = m;
  ctx->qw.tq_last[2] = ctx->qw.tq_last[3] = 0;
  // an empty list still runs the n = 0 batch, whose k is never read
  *list = ItemList{it.vk, it.sig, reinterpret_cast<const uint32_t*>(ctx->sc_hit.get()), nullptr, m};
  *ctx->qw.tq_harena = 0;
  if (!m) return 0;
  const uint16_t* e_tpl = ctx->qw.tq_tpl;
  const uint8_t* e_var = it.var;
  const uint32_t* e_voff = it.var_off;
  size_t e_bytes = it.var_bytes;
  if (m < n) {
    if ((rc = tmpl_room(ctx, st, ctx->qw.tq_gtpl, m)) || (rc = tmpl_room(ctx, st, ctx->qw.tq_gvoff, m + 1)) ||
        (rc = tmpl_room(ctx, st, ctx->qw.tq_gvar, holes + 16)))
      return rc;
    uint8_t* g_vk = ctx->sc_g;
    uint8_t* g_sig = g_vk + ctx->sc_cap_n * 32;
    launch_tmpl_quorum_gather(st, (uint32_t)n, (uint32_t)m, ctx->sc_hit, ctx->sc_wg, ctx->qw.tq_wgh, it.vk, it.sig,
                              ctx->qw.tq_tpl, it.var, it.var_off, ctx->sc_idx, g_vk, g_sig, ctx->qw.tq_gtpl, ctx->qw.tq_gvar,
                              ctx->qw.tq_gvoff);
    CK(hipGetLastError());
    list->vk = g_vk;
    list->sig = g_sig;
    list->idx = ctx->sc_idx;
    e_tpl = ctx->qw.tq_gtpl;
    e_var = ctx->qw.tq_gvar;
    e_voff = ctx->qw.tq_gvoff;
    e_bytes = holes;
  }
  // Item::from (src/batch.rs:82-94) for the m checked votes alone: the arena is sized from m
  if ((rc = tmpl_arena_room(ctx, w, st, m, sh, holes)) || (rc = ensure_n(ctx, m)) ||
      (rc = tmpl_expand(ctx, w, st, view, m, e_tpl, e_var, e_voff, e_bytes, w.arena, w.off)))
    return rc;
  // k_tmpl_len checks the gathered items again; its flag travels behind the expansion and the
  // batch's wait reads it before it believes a verdict
  CK(hipMemcpyAsync(w.h_flag, w.flag, sizeof(int), hipMemcpyDeviceToHost, st));
  CK(hipMemcpyAsync(ctx->qw.tq_harena.get(), w.off + m, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  w.check = true;
  launch_challenge(st, (uint32_t)m, list->vk, list->sig, w.arena, w.off, ctx->kbuf);
  CK(hipGetLastError());
  list->k = ctx->kbuf;
  ctx->qw.tq_last[2] = m;
  return 0;
}

// behind the batch on tmpl_quorum_list's list; rc: what it returned
static int tmpl_quorum_done(edc_ctx* ctx, int rc) {
  ctx->slot[0].tw.check = false;        // also when the batch never reached its wait
  if (rc >= 0) ctx->qw.tq_last[3] = *ctx->qw.tq_harena;
  return rc;
}

static int tmpl_quorum_run(edc_ctx* ctx, const edc_templates* ts, const TmplShape& sh, size_t nc,
                           const uint32_t* commit_off, const uint16_t* commit_tpl, uint32_t alt_span, size_t n,
                           const TmplQuorumItems& it, const uint64_t* threshold, int mode, const uint8_t* z_seed,
                           const QuorumOut& out) {
  ItemList list;
  int rc = tmpl_quorum_list(ctx, ts, sh, nc, commit_off, commit_tpl, alt_span, n, it, threshold, mode, &list);
  if (rc) return rc;
  return tmpl_quorum_done(ctx, quorum_finish(ctx, nc, threshold, n, list, it.power, it.flag, z_seed, out));
}

extern "C" {

int edc_tmpl_quorum_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                  const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                  const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                  const uint32_t* d_var_off, size_t var_bytes, const uint64_t* d_power,
                                  const uint8_t* d_flag, const uint64_t* threshold, int mode, const uint8_t z_seed[32],
                                  uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally, int* n_bad_commits,
                                  size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, false, nc, out, &rc)) return rc;
  TmplShape sh;
  size_t n;
  TmplQuorumItems it;
  if ((rc = tmpl_quorum_device_inputs(ctx, ts, nc, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                      d_var_off, var_bytes, d_power, d_flag, threshold, mode, &sh, &n, &it)))
    return rc;
  return tmpl_quorum_run(ctx, ts, sh, nc, commit_off, commit_tpl, alt_span, n, it, threshold, mode, z_seed, out);
}

int edc_tmpl_quorum_verify(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                           const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt, const uint8_t* vk,
                           const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                           const uint64_t* power, const uint8_t* flag, const uint64_t* threshold, int mode,
                           const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                           int* n_bad_commits, size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, false, nc, out, &rc)) return rc;
  TmplShape sh;
  size_t n;
  TmplQuorumItems it;
  if ((rc = tmpl_quorum_host_inputs(ctx, ts, nc, commit_off, commit_tpl, alt_span, item_alt, vk, key_idx, sig, var, var_off,
                                    power, flag, threshold, mode, &sh, &n, &it)))
    return rc;
  return tmpl_quorum_run(ctx, ts, sh, nc, commit_off, commit_tpl, alt_span, n, it, threshold, mode, z_seed, out);
}

int edc_debug_tmpl_quorum_last(const edc_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out || !ctx->qw.tq_have) return EDC_ERR_ARG;
  memcpy(out, ctx->qw.tq_last, sizeof(ctx->qw.tq_last));
  return EDC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- cached quorum commit sets
// edc_cached_*: the quorum entries with the verified-signature table between the selection and the
// batch. The selection never looks at the table. k_sc_lookup_masked probes the checked items only
// and leaves a second leave-out byte per item (not checked, or a hit), so ONE compaction takes the
// checked misses straight from the n-item arrays into the staging area, and quorum_finish runs the
// batch on them, inserts what it proves valid and puts the codes back over the lookup's base codes
// (255 not checked, 0 otherwise: a hit ends as 0 with no pass of its own).
// Plain forms: k exists for all n items before the selection, so the lookup rides behind it and
// its counts come back in the selection's one read-back. Templated forms: k exists only for the m
// votes that were gathered and hashed after that read-back, so the lookup runs on the m-item list
// and the miss count needs a second read-back; the misses are compacted into a second staging area
// (the first still holds the gathered list, which the insert and the code scatter index).
static int ensure_cq(edc_ctx* ctx, size_t n) {
  CK(grow_group(ctx->qw.cq_cap_n, n ? n : 1, item_cap, sync_of(ctx->st()), [&](size_t cap) {
    return alloc_all(sized(ctx->qw.cq_leave, cap), sized(ctx->qw.cq_code, cap),
                     sized(ctx->qw.cq_wg, 2 * (cap / SC_BLOCK + 2)));    // misses + total, hits + total
  }));
  return 0;
}

// The lookup of a list (skip: the selection's bytes, null: every item is checked) and the scans of
// its workgroup counts; the miss and hit totals travel to h[3] / h[4].
static int cq_lookup(edc_ctx* ctx, const ItemList& list, const uint8_t* skip) {
  int rc = ensure_cq(ctx, list.count);
  if (rc) return rc;
  hipStream_t st = ctx->st();
  const uint32_t nwg = (uint32_t)((list.count + SC_BLOCK - 1) / SC_BLOCK);
  uint32_t *wm = ctx->qw.cq_wg, *wh = ctx->qw.cq_wg + nwg + 1;
  launch_sc_lookup_masked(st, ctx->sc(), (uint32_t)list.count, skip, list.vk, list.sig, list.k, ctx->qw.cq_leave, ctx->qw.cq_code,
                          wm, wh);
  launch_sc_scan(st, nwg, wm, wm + nwg);
  launch_sc_scan(st, nwg, wh, wh + nwg);
  CK(hipGetLastError());
  ctx->qw.h[3] = ctx->qw.h[4] = 0;
  CK(hipMemcpyAsync(&ctx->qw.h[3], wm + nwg, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  CK(hipMemcpyAsync(&ctx->qw.h[4], wh + nwg, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  return 0;
}

// the counts of a lookup that has been read back: the statistics and the debug record
static int cq_counts(edc_ctx* ctx, size_t n, size_t m, size_t hashed, size_t* miss) {
  const size_t c = m ? ctx->qw.h[3] : 0, h = m ? ctx->qw.h[4] : 0;
  if (c + h != m) { ctx->err = "cached quorum: hits and misses do not add up to the checked count"; return EDC_ERR_HIP; }
  ctx->sc_hits += h;
  ctx->sc_misses += c;
  ctx->qw.cq_have = true;
  ctx->qw.cq_last[0] = n;
  ctx->qw.cq_last[1] = m;
  ctx->qw.cq_last[2] = h;
  ctx->qw.cq_last[3] = c;
  ctx->qw.cq_last[4] = hashed;
  ctx->qw.cq_last[5] = 0;
  *miss = c;
  return 0;
}

// A checked cached quorum commit set whose items (all: vk, sig, k of the n votes; power, flag) are
// on the device; hashed: the items SHA-512 ran over for this call.
static int cached_quorum_run(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* threshold, int mode,
                             const ItemList& all, const uint64_t* d_power, const uint8_t* d_flag, const uint8_t* z_seed,
                             const QuorumOut& out, size_t hashed, QuorumJoin* jn = nullptr) {
  const size_t n = all.count;
  size_t m = 0, c = 0;
  ItemList miss;
  int rc = quorum_front_enqueue(ctx, n, nc, commit_off, threshold, mode, d_power, d_flag, jn);
  if (rc) return rc;
  // behind the selection (and a request's double-vote scan, which reads the selection's skip bytes
  // alone): the masked lookup, whose counts travel in the same read-back
  if (n && (rc = cq_lookup(ctx, all, ctx->sc_hit))) return rc;
  if ((rc = quorum_select_read(ctx, n, &m, jn ? kJoinFlagMsg : nullptr)) || (rc = quorum_join_check_k(ctx, jn)) ||
      (rc = cq_counts(ctx, n, m, hashed, &c)))
    return rc;
  if ((rc = quorum_gather(ctx, all, c, ctx->qw.cq_leave, ctx->qw.cq_wg, sc_area(ctx), &miss))) return rc;
  const QuorumCached cq{m, ctx->qw.cq_code, all};
  return quorum_finish(ctx, nc, threshold, n, miss, d_power, d_flag, z_seed, out, &cq, jn ? ctx->qw.a.hdv.get() : nullptr,
                       jn ? jn->trust : nullptr);
}

// tmpl_quorum_list's list (the m checked votes, their k in kbuf) through the table and the batch:
// the lookup, the second read-back, the counts, the misses gathered, quorum_finish.
static int cached_tmpl_finish(edc_ctx* ctx, size_t nc, const uint64_t* threshold, size_t n, const ItemList& list,
                              const uint64_t* d_power, const uint8_t* d_flag, const uint8_t* z_seed,
                              const QuorumOut& out, const uint8_t* dv = nullptr, const QuorumTrust* tr = nullptr) {
  hipStream_t st = ctx->st();
  const size_t m = list.count;
  int rc;
  if (m) {
    if ((rc = cq_lookup(ctx, list, nullptr))) return rc;
    CK(hipStreamSynchronize(st));       // the second read-back: the miss count sizes the batch
    if (*ctx->slot[0].tw.h_flag) {      // what the batch's wait would find, before anything is counted
      ctx->err = "templated items: template index or hole offsets out of range";
      return EDC_ERR_ARG;
    }
  }
  size_t c = 0;
  if ((rc = cq_counts(ctx, n, m, m, &c))) return rc;
  if (c && c < m) {                     // the second staging area, when something is gathered
    CK(grow_group(ctx->qw.cq_cap_g, m, item_cap, sync_of(st), [&](size_t cap) {
      return alloc_all(sized(ctx->qw.cq_g, cap * 128), sized(ctx->qw.cq_idx, cap));
    }));
  }
  ItemList miss;
  if ((rc = quorum_gather(ctx, list, c, ctx->qw.cq_leave, ctx->qw.cq_wg, GatherArea{ctx->qw.cq_g, ctx->qw.cq_cap_g, ctx->qw.cq_idx}, &miss)))
    return rc;
  const QuorumCached cq{m, ctx->qw.cq_code, list};
  return quorum_finish(ctx, nc, threshold, n, miss, d_power, d_flag, z_seed, out, &cq, dv, tr);
}

static int cached_tmpl_quorum_run(edc_ctx* ctx, const edc_templates* ts, const TmplShape& sh, size_t nc,
                                  const uint32_t* commit_off, const uint16_t* commit_tpl, uint32_t alt_span, size_t n,
                                  const TmplQuorumItems& it, const uint64_t* threshold, int mode, const uint8_t* z_seed,
                                  const QuorumOut& out) {
  ItemList list;
  int rc = tmpl_quorum_list(ctx, ts, sh, nc, commit_off, commit_tpl, alt_span, n, it, threshold, mode, &list);
  if (rc) return rc;
  return tmpl_quorum_done(ctx, cached_tmpl_finish(ctx, nc, threshold, n, list, it.power, it.flag, z_seed, out));
}

extern "C" {

int edc_cached_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                    const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off,
                                    const uint8_t* d_k, const uint64_t* d_power, const uint8_t* d_flag,
                                    const uint64_t* threshold, int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts,
                                    uint8_t* item_verdicts, uint64_t* tally, int* n_bad_commits, size_t* n_checked,
                                    size_t* n_miss, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, n_miss, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, true, nc, out, &rc)) return rc;
  size_t n;
  const uint32_t* k;
  if ((rc = quorum_device_inputs(ctx, nc, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k, d_power, d_flag, threshold, mode,
                                 &n, &k)))
    return rc;
  return cached_quorum_run(ctx, nc, commit_off, threshold, mode, ItemList{d_vk, d_sig, k, nullptr, n}, d_power, d_flag,
                           z_seed, out, d_k ? 0 : n);
}

int edc_cached_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                             const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                             const uint8_t* k, const uint64_t* power, const uint8_t* flag, const uint64_t* threshold,
                             int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                             uint64_t* tally, int* n_bad_commits, size_t* n_checked, size_t* n_miss, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, n_miss, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, true, nc, out, &rc)) return rc;
  size_t n;
  if ((rc = quorum_host_inputs(ctx, nc, commit_off, vk, key_idx, sig, msg, msg_off, k, power, flag, threshold, mode, &n)))
    return rc;
  return cached_quorum_run(ctx, nc, commit_off, threshold, mode, ItemList{ctx->vk, ctx->sig, ctx->kbuf, nullptr, n},
                           ctx->qw.a.power, ctx->qw.a.flag, z_seed, out, k ? 0 : n);
}

int edc_cached_tmpl_quorum_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                         const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                         const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                         const uint32_t* d_var_off, size_t var_bytes, const uint64_t* d_power,
                                         const uint8_t* d_flag, const uint64_t* threshold, int mode,
                                         const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                                         uint64_t* tally, int* n_bad_commits, size_t* n_checked, size_t* n_miss,
                                         uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, n_miss, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, true, nc, out, &rc)) return rc;
  TmplShape sh;
  size_t n;
  TmplQuorumItems it;
  if ((rc = tmpl_quorum_device_inputs(ctx, ts, nc, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                      d_var_off, var_bytes, d_power, d_flag, threshold, mode, &sh, &n, &it)))
    return rc;
  return cached_tmpl_quorum_run(ctx, ts, sh, nc, commit_off, commit_tpl, alt_span, n, it, threshold, mode, z_seed, out);
}

int edc_cached_tmpl_quorum_verify(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                  const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt, const uint8_t* vk,
                                  const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                                  const uint64_t* power, const uint8_t* flag, const uint64_t* threshold, int mode,
                                  const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                                  uint64_t* tally, int* n_bad_commits, size_t* n_checked, size_t* n_miss,
                                  uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, n_miss, check8};
  int rc;
  if (quorum_entry_done(ctx, z_seed, true, nc, out, &rc)) return rc;
  TmplShape sh;
  size_t n;
  TmplQuorumItems it;
  if ((rc = tmpl_quorum_host_inputs(ctx, ts, nc, commit_off, commit_tpl, alt_span, item_alt, vk, key_idx, sig, var,
                                    var_off, power, flag, threshold, mode, &sh, &n, &it)))
    return rc;
  return cached_tmpl_quorum_run(ctx, ts, sh, nc, commit_off, commit_tpl, alt_span, n, it, threshold, mode, z_seed, out);
}

int edc_debug_cached_quorum_last(const edc_ctx* ctx, uint64_t out[6]) {
  if (!ctx || !out || !ctx->qw.cq_have) return EDC_ERR_ARG;
  memcpy(out, ctx->qw.cq_last, sizeof(ctx->qw.cq_last));
  return EDC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- validator-set quorum commit sets
// edc_valset_*: the quorum entries with the join on the device. The registered list carries its
// powers (edc_valset_set_powers); the resolve kernel turns every vote's key bytes (or position)
// into the power and flag the selection reads, in side A's arrays where a host form of the quorum
// entries stages them; the double-vote scan runs behind the selection on its skip bytes, and its
// per-commit bytes come back with the selection's one read-back. Everything after that is the
// quorum entries' own: quorum_gather, then quorum_finish with the double-vote bytes.
// edc_vhist_*: the same entries with every commit judged by the set of its own version (cver, the
// commits' versions on the host; null: the one set of edc_valset_set_powers). Only the join
// differs: the offsets and versions go to the device in front of it, and k_vh_resolve stands where
// k_vs_resolve does.
// The workspace, the launches and the select pair stand with QuorumJoin in the quorum section
// (ensure_valset ... valset_select), where quorum_run and its siblings take the join as an optional
// stage. Here: one body per kind of entry, for these two families and for the requests below.
//   verify   vq_run_plain (messages or k) and, for requests only, vq_run_tmpl
//   resolve  valset_resolve_body, one side or a trusting pair
//   timing   valset_debug_select_body, which launches what valset_select_enqueue launches
// keys (bytes into ctx->vk, or positions into kidx) and flags (vflag) of n > 0 host votes
static int valset_stage_votes(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag) {
  hipStream_t st = ctx->st();
  if (key_idx) {
    CK(hipMemcpyAsync(ctx->qw.kidx, key_idx, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  } else {
    int rc = ensure_n(ctx, n);
    if (rc) return rc;
    CK(hipMemcpyAsync(ctx->vk, vk, n * 32, hipMemcpyHostToDevice, st));
  }
  CK(hipMemcpyAsync(ctx->qw.vflag, flag, n, hipMemcpyHostToDevice, st));
  return 0;
}

// what the host checks of a call on host keys and flags without signatures (resolve, the hook)
static int valset_check_host(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                             const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold, int mode, size_t* n,
                             const uint32_t* cver = nullptr) {
  int rc = quorum_check(ctx, nc, commit_off, threshold, mode, n);
  if (rc || (rc = cver ? vhist_ready(ctx, nc, cver) : valset_ready(ctx))) return rc;
  if (*n) {
    if ((rc = commits_check_keys(ctx, *n, vk, key_idx))) return rc;
    if (!flag) { ctx->err = "null input"; return EDC_ERR_ARG; }
  }
  return 0;
}

extern "C" {

int edc_valset_set_powers(edc_ctx* ctx, size_t m, const uint64_t* power) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  for (Slot& s : ctx->slot)
    if (s.pending) { ctx->err = "voting powers change with a batch in flight"; return EDC_ERR_ARG; }
  int rc = sync_all(ctx);
  if (rc) return rc;
  if (!m && !power) {
    free_valset(ctx);
    return EDC_OK;
  }
  if (!ctx->kc_reg_m) { ctx->err = "no registered key list (edc_keycache_load)"; return EDC_ERR_ARG; }
  if (m != ctx->kc_reg_m || !power) { ctx->err = "one power per position of the registered key list"; return EDC_ERR_ARG; }
  const uint32_t u = ctx->kc_m;
  std::vector<uint64_t> pw(u, 0);
  std::vector<uint8_t> mem(u, 0);
  std::vector<uint32_t> pos(u, VALSET_NO_POS);
  for (size_t p = 0; p < m; ++p) {
    const uint32_t c = ctx->kc_regh[p];
    if (mem[c]) { ctx->err = "the registered key list holds a key twice: not a validator set"; return EDC_ERR_ARG; }
    mem[c] = 1;
    pw[c] = power[p];
    pos[c] = (uint32_t)p;
  }
  if (!valset_check_powers(m, power)) {
    ctx->err = "voting power: every power and their sum at most 2^63 - 1";
    return EDC_ERR_ARG;
  }
  DevBuf<uint64_t> d_pw;          // committed to the context only on success
  DevBuf<uint8_t> d_mem;
  DevBuf<uint32_t> d_pos;
  CK(alloc_all(sized(d_pw, u), sized(d_mem, u), sized(d_pos, u)));
  CK(hipMemcpy(d_pw, pw.data(), u * sizeof(uint64_t), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_mem, mem.data(), u, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_pos, pos.data(), u * sizeof(uint32_t), hipMemcpyHostToDevice));
  ctx->vs_power = std::move(d_pw);
  ctx->vs_member = std::move(d_mem);
  ctx->vs_pos = std::move(d_pos);
  ctx->vs_posh.swap(pos);
  ctx->vs_count = u;
  ctx->vs_m = (uint32_t)m;
  return EDC_OK;
}

int edc_valset_size(const edc_ctx* ctx) { return ctx ? (int)ctx->vs_m : 0; }

}  // extern "C"

// hist: an edc_vhist_* entry, which needs cver
static bool vhist_ver_missing(edc_ctx* ctx, bool hist, const uint32_t* cver) {
  if (hist && !cver) ctx->err = "null commit_ver";
  return hist && !cver;
}

// vhist_ready for the trusting side: every trust version is one of the history's or the sentinel
static int vq_trust_ready(edc_ctx* ctx, size_t nc, const QuorumTrust* tr) {
  if (tr && !vq_trust_check_versions(nc, tr->ver, ctx->vh.nv)) {
    ctx->err = "trust_ver: a version past the history's last that is not EDC_VQ_NO_TRUST";
    return EDC_ERR_ARG;
  }
  return 0;
}

// Every verify entry on messages or k, below the checks of the request's shape that its caller has
// made (edc_vq_verify: vq_entry_done; the edc_valset_* / edc_vhist_* entries: valset_verify_entry):
// the checks of the arrays (n > 0 only), the staging, then quorum_run or cached_quorum_run with the
// join. *hashed: the items SHA-512 runs over.
static int vq_run_plain(edc_ctx* ctx, const edc_vq_request* rq, const QuorumOut& out, const QuorumTrust* tr,
                        size_t* hashed) {
  const size_t nc = rq->nc;
  const bool hist = rq->commit_ver != nullptr;
  size_t n;
  int rc = quorum_check(ctx, nc, rq->commit_off, rq->threshold, rq->mode, &n);
  if (rc || (rc = hist ? vhist_ready(ctx, nc, rq->commit_ver) : valset_ready(ctx)) || (rc = vq_trust_ready(ctx, nc, tr)))
    return rc;
  if (n && (!rq->sig || !rq->flag)) { ctx->err = "null input"; return EDC_ERR_ARG; }
  ItemList all;
  QuorumJoin jn{nullptr, nullptr, nullptr, rq->commit_ver, nullptr, {}, tr};
  if (rq->device) {
    if (n && (!rq->vk || (!rq->k && !rq->msg_off))) { ctx->err = "null input"; return EDC_ERR_ARG; }
    if (n && (!aligned16(rq->vk) || !aligned16(rq->sig) || (rq->k && !aligned16(rq->k)))) {
      ctx->err = "device vk / sig / k arrays must be 16-byte aligned";
      return EDC_ERR_ARG;
    }
    CK(hipSetDevice(ctx->device));
    if ((rc = valset_room(ctx, n, nc, hist, tr != nullptr))) return rc;
    const uint32_t* k = reinterpret_cast<const uint32_t*>(rq->k);
    if (n && !k) {
      if ((rc = ensure_n(ctx, n))) return rc;
      launch_challenge(ctx->st(), (uint32_t)n, rq->vk, rq->sig, rq->msg, rq->msg_off, ctx->kbuf);
      CK(hipGetLastError());
      k = ctx->kbuf;
    }
    all = ItemList{rq->vk, rq->sig, k, nullptr, n};
    jn.d_vk = rq->vk;
    jn.d_flag = rq->flag;
  } else {
    if (n && ((rc = commits_check_keys(ctx, n, rq->vk, rq->key_idx)) ||
              (rc = commits_check_msg_or_k(ctx, n, rq->msg, rq->msg_off, rq->k))))
      return rc;
    CK(hipSetDevice(ctx->device));
    if ((rc = valset_room(ctx, n, nc, hist, tr != nullptr))) return rc;
    hipStream_t st = ctx->st();
    if (rq->k) {
      if ((rc = ensure_n(ctx, n))) return rc;
      if (n) CK(hipMemcpyAsync(ctx->kbuf, rq->k, n * 32, hipMemcpyHostToDevice, st));
    } else if ((rc = upload_msgs(ctx, n, rq->msg, n ? rq->msg_off : nullptr))) {
      return rc;
    }
    if (n) {                  // 4 + 64 + 1 bytes per vote in the key_idx form: the keys are expanded on the device
      CK(hipMemcpyAsync(ctx->qw.vflag, rq->flag, n, hipMemcpyHostToDevice, st));
      if ((rc = stage_keys_sigs(ctx, st, n, rq->vk, rq->key_idx, rq->sig, ctx->qw.kidx, ctx->vk, ctx->sig))) return rc;
      if (!rq->k) {
        launch_challenge(st, (uint32_t)n, ctx->vk, ctx->sig, ctx->msg, ctx->off, ctx->kbuf);
        CK(hipGetLastError());
      }
    }
    all = ItemList{ctx->vk, ctx->sig, ctx->kbuf, nullptr, n};
    jn.d_vk = rq->key_idx ? nullptr : ctx->vk.get();
    jn.d_kidx = ctx->qw.kidx;
    jn.d_flag = ctx->qw.vflag;
    jn.host_k = n ? rq->k : nullptr;
  }
  *hashed = rq->k ? 0 : n;
  if (rq->cached)
    return cached_quorum_run(ctx, nc, rq->commit_off, rq->threshold, rq->mode, all, ctx->qw.a.power, ctx->qw.a.flag, rq->z_seed,
                             out, *hashed, &jn);
  return quorum_run(ctx, nc, rq->commit_off, rq->threshold, rq->mode, all, ctx->qw.a.power, ctx->qw.a.flag, rq->z_seed, out, &jn);
}

// The edc_valset_* / edc_vhist_* verify entries: what they accept and refuse before the arrays are
// looked at is their own, not the request's (a set of empty commits needs no array at all, where
// the request always names its keys), and they leave the request's debug record alone. Then the
// request's plain body on a request with no template set, no table and no trusting side.
static int valset_verify_entry(edc_ctx* ctx, bool hist, bool device, size_t nc, const uint32_t* commit_off,
                               const uint32_t* cver, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                               const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k, const uint8_t* flag,
                               const uint64_t* threshold, int mode, const uint8_t* z_seed, const QuorumOut& out) {
  int rc;
  if (quorum_entry_done(ctx, z_seed, false, nc, out, &rc)) return rc;
  if (vhist_ver_missing(ctx, hist, cver)) return EDC_ERR_ARG;
  edc_vq_request rq;
  memset(&rq, 0, sizeof(rq));
  rq.size = sizeof(rq);
  rq.device = device;
  rq.mode = mode;
  rq.nc = nc;
  rq.commit_off = commit_off;
  rq.commit_ver = cver;
  rq.threshold = threshold;
  rq.z_seed = z_seed;
  rq.vk = vk;
  rq.key_idx = key_idx;
  rq.sig = sig;
  rq.flag = flag;
  rq.msg = msg;
  rq.msg_off = msg_off;
  rq.k = k;
  size_t hashed;
  return vq_run_plain(ctx, &rq, out, nullptr, &hashed);
}

// One side's outputs of a resolve entry, host memory, all nullable.
struct ResolveSide {
  uint32_t* pos;
  uint64_t* power;
  uint8_t *flag, *checked;
  uint64_t* planned;
  uint8_t* dv;
};

// What the resolve entries and the timing hooks do first, on host keys and flags: the checks, the
// workspace, the staging, then valset_select with its read-back. *n: the votes; *m: the checked
// ones (the union's in a pair). tr (edc_vq_trust_*; with hist): the trusting side's versions and
// thresholds, both needed. nc == 0: EDC_OK with nothing done.
static int valset_resolve_select(edc_ctx* ctx, bool hist, size_t nc, const uint32_t* commit_off, const uint32_t* cver,
                                 const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold,
                                 int mode, const QuorumTrust* tr, size_t* n, size_t* m) {
  *n = *m = 0;
  if (!ctx) return EDC_ERR_ARG;
  if (!nc) return EDC_OK;
  if (vhist_ver_missing(ctx, hist, cver)) return EDC_ERR_ARG;
  if (tr && (!tr->ver || !tr->threshold)) { ctx->err = "null trust_ver / trust_threshold"; return EDC_ERR_ARG; }
  int rc = valset_check_host(ctx, nc, commit_off, vk, key_idx, flag, threshold, mode, n, cver);
  if (rc || (rc = vq_trust_ready(ctx, nc, tr))) return rc;
  CK(hipSetDevice(ctx->device));
  if ((rc = valset_room(ctx, *n, nc, hist, tr != nullptr)) || (*n && (rc = valset_stage_votes(ctx, *n, vk, key_idx, flag))))
    return rc;
  QuorumJoin jn{key_idx ? nullptr : ctx->vk.get(), ctx->qw.kidx, ctx->qw.vflag, cver, nullptr, {}, tr};
  return valset_select(ctx, *n, nc, commit_off, threshold, mode, &jn, m);
}

// edc_valset_resolve, edc_vhist_resolve (hist) and edc_vq_trust_resolve (tr, with b and side): the
// join, the selection and the double-vote scan as the verify entries run them, and each side's
// arrays read back (side_skip: a pair's sc_hit holds the union's skip bytes).
static int valset_resolve_body(edc_ctx* ctx, bool hist, size_t nc, const uint32_t* commit_off, const uint32_t* cver,
                               const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold,
                               int mode, const ResolveSide& a, size_t* n_checked, const QuorumTrust* tr = nullptr,
                               const ResolveSide& b = ResolveSide{}, uint8_t* side = nullptr) {
  size_t n, m;
  const int rc = valset_resolve_select(ctx, hist, nc, commit_off, cver, vk, key_idx, flag, threshold, mode, tr, &n, &m);
  if (rc || !nc) {
    if (!rc && n_checked) *n_checked = 0;
    return rc;
  }
  const std::vector<uint32_t>& posh = hist ? ctx->vh_posh : ctx->vs_posh;
  hipStream_t st = ctx->st();
  const QuorumWs& q = ctx->qw;
  const ResolveSide* o[2] = {&a, &b};
  std::vector<uint32_t> who[2];
  auto back = [&](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  const int sides = tr ? 2 : 1;         // array by array, side A's in front of side B's
  for (int j = 0; j < sides; ++j) who[j].resize(o[j]->pos ? n : 0);
  for (int j = 0; j < sides; ++j) CK(back(who[j].data(), q.side[j].who, who[j].size() * sizeof(uint32_t)));
  for (int j = 0; j < sides; ++j) CK(back(o[j]->power, q.side[j].power, n * sizeof(uint64_t)));
  for (int j = 0; j < sides; ++j) CK(back(o[j]->flag, q.side[j].flag, n));
  for (int j = 0; j < sides; ++j) CK(back(o[j]->planned, q.side[j].planned, nc * sizeof(uint64_t)));
  for (int j = 0; j < sides; ++j) CK(back(o[j]->checked, side_skip(ctx, q.side[j], tr != nullptr), n));
  CK(back(side, q.sideb, n));
  CK(hipStreamSynchronize(st));
  for (int j = 0; j < sides; ++j) {
    for (size_t i = 0; i < who[j].size(); ++i) o[j]->pos[i] = who[j][i] == KC_EMPTY ? VALSET_NO_POS : posh[who[j][i]];
    for (size_t i = 0; i < n && o[j]->checked; ++i) o[j]->checked[i] = o[j]->checked[i] ? 0 : 1;      // the kernels write skip bytes
    if (o[j]->dv) memcpy(o[j]->dv, q.side[j].hdv, nc);
  }
  if (n_checked) *n_checked = m;
  return EDC_OK;
}

// Mean times over reps runs of the stages valset_select_enqueue launches, through the helpers it
// launches them with, on host keys and flags: ms[0] the join; with three intervals (the pair's
// hook) ms[1] the selection per side, the union and the scan of its tile counts; the last the
// double-vote scan per side with the clearing of its set and bytes. Every stage rewrites the values
// the selection in front left (planned is a maximum).
static int valset_debug_select_body(edc_ctx* ctx, bool hist, size_t nc, const uint32_t* commit_off, const uint32_t* cver,
                                    const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag,
                                    const uint64_t* threshold, int mode, int reps, int intervals, float* ms,
                                    const QuorumTrust* tr = nullptr) {
  if (!ctx || reps < 1) return EDC_ERR_ARG;
  for (int j = 0; j < intervals && ms; ++j) ms[j] = 0.f;
  size_t n, m;
  const int rc = valset_resolve_select(ctx, hist, nc, commit_off, cver, vk, key_idx, flag, threshold, mode, tr, &n, &m);
  if (rc || !n) return rc;
  hipStream_t st = ctx->st();
  const QuorumSide &a = ctx->qw.a, &b = ctx->qw.side[1];
  const QuorumJoin jn{key_idx ? nullptr : ctx->vk.get(), ctx->qw.kidx, ctx->qw.vflag, cver, nullptr, {}, tr};
  const uint32_t nwg = (uint32_t)quorum_tiles(n);
  Event e[4];
  for (int j = 0; j <= intervals; ++j) CK(e[j].create());
  int at = 0;
  CK(hipEventRecord(e[at++], st));
  for (int r = 0; r < reps; ++r) valset_join_launch(ctx, st, n, nc, jn);        // the offsets and versions are staged
  CK(hipGetLastError());
  CK(hipEventRecord(e[at++], st));
  if (intervals == 3) {
    for (int r = 0; r < reps; ++r) {
      quorum_side_launch(ctx, st, n, nc, mode, a, a.power, a.flag, side_skip(ctx, a, tr != nullptr), false);
      if (tr) CK(quorum_side_b_launch(ctx, st, n, nc, mode));
      launch_sc_scan(st, nwg, ctx->sc_wg, ctx->sc_wg + nwg);
    }
    CK(hipGetLastError());
    CK(hipEventRecord(e[at++], st));
  }
  for (int r = 0; r < reps; ++r) {
    CK(valset_pairs_launch(ctx, st, n, nc, a, side_skip(ctx, a, tr != nullptr)));
    if (tr) CK(valset_pairs_launch(ctx, st, n, nc, b, b.skip));
  }
  CK(hipGetLastError());
  CK(hipEventRecord(e[at], st));
  CK(hipEventSynchronize(e[at]));
  for (int j = 0; j < intervals && ms; ++j) {
    float t = 0.f;
    CK(hipEventElapsedTime(&t, e[j], e[j + 1]));
    ms[j] = t / (float)reps;
  }
  return EDC_OK;
}

extern "C" {

int edc_valset_resolve(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk, const uint32_t* key_idx,
                       const uint8_t* flag, const uint64_t* threshold, int mode, uint32_t* pos, uint64_t* power,
                       uint8_t* flag_out, uint8_t* checked, uint64_t* planned, size_t* n_checked, uint8_t* dv) {
  return valset_resolve_body(ctx, false, nc, commit_off, nullptr, vk, key_idx, flag, threshold, mode,
                             ResolveSide{pos, power, flag_out, checked, planned, dv}, n_checked);
}

int edc_valset_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                    const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off,
                                    const uint8_t* d_k, const uint8_t* d_flag, const uint64_t* threshold, int mode,
                                    const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                                    uint64_t* tally, int* n_bad_commits, size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  return valset_verify_entry(ctx, false, true, nc, commit_off, nullptr, d_vk, nullptr, d_sig, d_msg, d_msg_off, d_k, d_flag,
                             threshold, mode, z_seed, out);
}

int edc_valset_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                             const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                             const uint8_t* k, const uint8_t* flag, const uint64_t* threshold, int mode,
                             const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                             int* n_bad_commits, size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  return valset_verify_entry(ctx, false, false, nc, commit_off, nullptr, vk, key_idx, sig, msg, msg_off, k, flag, threshold,
                             mode, z_seed, out);
}

int edc_debug_valset_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                            const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold, int mode, int reps,
                            float ms[2]) {
  return valset_debug_select_body(ctx, false, nc, commit_off, nullptr, vk, key_idx, flag, threshold, mode, reps, 2, ms);
}

// ---------------------------------------------------------------- validator-set history
// edc_vhist_set checks the history and builds its change lists by position (vhist_build), then
// re-indexes them from position to cache index, as edc_valset_set_powers re-indexes its arrays: key
// s of the cache owns the list of its position, every other key an empty one.
int edc_vhist_set(edc_ctx* ctx, size_t m, const uint64_t* base_power, size_t nv, const uint32_t* upd_off,
                  const uint32_t* upd_pos, const uint64_t* upd_power) {
  if (!ctx) return EDC_ERR_ARG;
  CK(hipSetDevice(ctx->device));
  for (Slot& s : ctx->slot)
    if (s.pending) { ctx->err = "validator-set history changes with a batch in flight"; return EDC_ERR_ARG; }
  int rc = sync_all(ctx);
  if (rc) return rc;
  if (!m && !base_power && !upd_off && !upd_pos && !upd_power) {
    free_vhist(ctx);
    return EDC_OK;
  }
  VHist h;
  const char* why = nullptr;
  if (!vhist_build(ctx->kc_reg_m, ctx->kc_regh.data(), m, base_power, nv, upd_off, upd_pos, upd_power, &h, &why)) {
    ctx->err = why;
    return EDC_ERR_ARG;
  }
  const uint32_t u = ctx->kc_m;
  std::vector<uint32_t> pos(u, VALSET_NO_POS), off(u + 1, 0), ver(h.ver.size());
  std::vector<uint64_t> pw(h.pow.size());
  for (size_t p = 0; p < m; ++p) pos[ctx->kc_regh[p]] = (uint32_t)p;
  for (uint32_t s = 0; s < u; ++s) {
    const uint32_t p = pos[s];
    const uint32_t a = p == VALSET_NO_POS ? 0 : h.off[p], len = p == VALSET_NO_POS ? 0 : h.off[p + 1] - a;
    std::copy_n(h.ver.begin() + a, len, ver.begin() + off[s]);
    std::copy_n(h.pow.begin() + a, len, pw.begin() + off[s]);
    off[s + 1] = off[s] + len;
  }
  DevBuf<uint32_t> d_off, d_ver;          // committed to the context only on success
  DevBuf<uint64_t> d_pw;
  CK(alloc_all(sized(d_off, off.size()), sized(d_ver, ver.size()), sized(d_pw, pw.size())));
  CK(hipMemcpy(d_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_ver, ver.data(), ver.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_pw, pw.data(), pw.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  ctx->vh_off = std::move(d_off);
  ctx->vh_ver = std::move(d_ver);
  ctx->vh_pow = std::move(d_pw);
  ctx->vh_posh.swap(pos);
  ctx->vh_count = u;
  ctx->vh = std::move(h);
  return EDC_OK;
}

int edc_vhist_versions(const edc_ctx* ctx) { return ctx && ctx->vh.m ? (int)ctx->vh.nv + 1 : 0; }

int edc_vhist_totals(const edc_ctx* ctx, uint32_t v0, size_t count, uint64_t* total, uint32_t* members) {
  if (!ctx) return EDC_ERR_ARG;
  const size_t nver = ctx->vh.m ? (size_t)ctx->vh.nv + 1 : 0;
  if (v0 > nver || count > nver - v0) return EDC_ERR_ARG;
  for (size_t j = 0; j < count; ++j) {
    if (total) total[j] = ctx->vh.total[v0 + j];
    if (members) members[j] = ctx->vh.members[v0 + j];
  }
  return EDC_OK;
}

int edc_vhist_resolve(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver, const uint8_t* vk,
                      const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold, int mode, uint32_t* pos,
                      uint64_t* power, uint8_t* flag_out, uint8_t* checked, uint64_t* planned, size_t* n_checked,
                      uint8_t* dv) {
  return valset_resolve_body(ctx, true, nc, commit_off, commit_ver, vk, key_idx, flag, threshold, mode,
                             ResolveSide{pos, power, flag_out, checked, planned, dv}, n_checked);
}

int edc_vhist_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                                   const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_msg,
                                   const uint64_t* d_msg_off, const uint8_t* d_k, const uint8_t* d_flag,
                                   const uint64_t* threshold, int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts,
                                   uint8_t* item_verdicts, uint64_t* tally, int* n_bad_commits, size_t* n_checked,
                                   uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  return valset_verify_entry(ctx, true, true, nc, commit_off, commit_ver, d_vk, nullptr, d_sig, d_msg, d_msg_off, d_k, d_flag,
                             threshold, mode, z_seed, out);
}

int edc_vhist_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                            const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg,
                            const uint64_t* msg_off, const uint8_t* k, const uint8_t* flag, const uint64_t* threshold,
                            int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                            uint64_t* tally, int* n_bad_commits, size_t* n_checked, uint8_t check8[32]) {
  const QuorumOut out{commit_verdicts, item_verdicts, tally, n_bad_commits, n_checked, nullptr, check8};
  return valset_verify_entry(ctx, true, false, nc, commit_off, commit_ver, vk, key_idx, sig, msg, msg_off, k, flag,
                             threshold, mode, z_seed, out);
}

int edc_debug_vhist_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                           const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold,
                           int mode, int reps, float ms[2]) {
  return valset_debug_select_body(ctx, true, nc, commit_off, commit_ver, vk, key_idx, flag, threshold, mode, reps, 2, ms);
}

}  // extern "C"

// ---------------------------------------------------------------- validator-set hashes
// edc_valhash_valset, edc_valhash_vhist, edc_valhash_vhist_match (valhash.h, edc_valhash.hip): what
// they refuse (valhash_ready, then the entry's own arguments), the address order of the list
// (valhash_ranks), then one workgroup per root on slot 0's stream and the read-back. hist: the
// history's versions; else the one set of edc_valset_set_powers.
static int valhash_ready(edc_ctx* ctx, bool hist) {
  CK(hipSetDevice(ctx->device));
  if (!ctx->kc_reg_m) { ctx->err = "no registered key list (edc_keycache_load)"; return EDC_ERR_ARG; }
  const int rc = hist ? vhist_ready(ctx, 0, nullptr) : valset_ready(ctx);
  if (rc) return rc;
  return claim_slot0(ctx) ? 0 : EDC_ERR_ARG;
}

// The address order of the registered list, once per list; run behind every check of an entry, so
// that a refused call has done no device work and changed nothing.
static int valhash_ranks(edc_ctx* ctx) {
  if (ctx->vx_ranked) return 0;
  const uint32_t m = ctx->kc_reg_m;
  hipStream_t st = ctx->st();
  DevBuf<uint8_t> d_addr;
  DevBuf<uint32_t> d_rank, d_by;          // committed to the context only on success
  CK(alloc_all(sized(d_addr, (size_t)m * VALHASH_ADDR_BYTES), sized(d_rank, m), sized(d_by, m)));
  launch_valhash_addr(st, m, ctx->kc_keys, ctx->kc_reg, d_addr);
  CK(hipGetLastError());
  std::vector<uint8_t> addr((size_t)m * VALHASH_ADDR_BYTES);
  CK(hipMemcpyAsync(addr.data(), d_addr, addr.size(), hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  std::vector<uint32_t> rank(m), by(m);
  valhash_rank(m, addr.data(), rank.data());
  for (uint32_t p = 0; p < m; ++p) by[rank[p]] = ctx->kc_regh[p];
  CK(hipMemcpy(d_rank, rank.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_by, by.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice));
  ctx->vx_rank = std::move(d_rank);
  ctx->vx_by_rank = std::move(d_by);
  ctx->vx_ranked = true;
  return 0;
}

static ValhashSrc valhash_src(const edc_ctx* ctx, bool hist) {
  return ValhashSrc{ctx->kc_keys, ctx->kc_reg, ctx->kc_reg_m, hist, ctx->vhv(), ctx->vs(), ctx->vx_rank, ctx->vx_by_rank};
}

// the largest member count among the versions ver[0 .. n), checked against the cap
static int valhash_max_members(edc_ctx* ctx, size_t n, const uint32_t* ver, uint32_t v0, uint32_t* max_members) {
  uint32_t mx = 0;
  for (size_t j = 0; j < n; ++j) mx = std::max(mx, ctx->vh.members[ver ? ver[j] : v0 + j]);
  if (mx > VALHASH_MAX_MEMBERS) { ctx->err = "validator-set hash: a version above EDC_VALHASH_MAX_MEMBERS members"; return EDC_ERR_ARG; }
  *max_members = mx;
  return 0;
}

extern "C" {

int edc_valhash_valset(edc_ctx* ctx, uint8_t out[32]) {
  if (!ctx) return EDC_ERR_ARG;
  int rc = valhash_ready(ctx, false);
  if (rc) return rc;
  if (!out) { ctx->err = "null output"; return EDC_ERR_ARG; }
  if (ctx->vs_m > VALHASH_MAX_MEMBERS) { ctx->err = "validator-set hash: a set above EDC_VALHASH_MAX_MEMBERS members"; return EDC_ERR_ARG; }
  if ((rc = valhash_ranks(ctx))) return rc;
  hipStream_t st = ctx->st();
  CK(grow(ctx->vx_roots, 32, byte_cap, sync_of(st)));
  CK(launch_valhash_roots(st, valhash_src(ctx, false), 1, nullptr, 0, ctx->vs_m, ctx->vx_roots));
  CK(hipGetLastError());
  uint8_t root[32];                     // out is written only by a call that succeeds
  CK(hipMemcpyAsync(root, ctx->vx_roots, 32, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  memcpy(out, root, 32);
  return EDC_OK;
}

int edc_valhash_vhist(edc_ctx* ctx, uint32_t v0, size_t count, uint8_t* out) {
  if (!ctx) return EDC_ERR_ARG;
  int rc = valhash_ready(ctx, true);
  if (rc) return rc;
  const size_t nver = (size_t)ctx->vh.nv + 1;
  if (v0 > nver || count > nver - v0) { ctx->err = "validator-set hashes: a range past the history's last version"; return EDC_ERR_ARG; }
  if (!count) return EDC_OK;
  if (!out) { ctx->err = "null output"; return EDC_ERR_ARG; }
  uint32_t mx;
  if ((rc = valhash_max_members(ctx, count, nullptr, v0, &mx)) || (rc = valhash_ranks(ctx))) return rc;
  hipStream_t st = ctx->st();
  CK(grow(ctx->vx_roots, count * 32, byte_cap, sync_of(st)));
  CK(launch_valhash_roots(st, valhash_src(ctx, true), (uint32_t)count, nullptr, v0, mx, ctx->vx_roots));
  CK(hipGetLastError());
  CK(hipStreamSynchronize(st));         // a failed kernel must not leave part of out written
  CK(hipMemcpy(out, ctx->vx_roots, count * 32, hipMemcpyDeviceToHost));
  return EDC_OK;
}

int edc_valhash_vhist_match(edc_ctx* ctx, size_t nc, const uint32_t* commit_ver, const uint8_t* expect, uint8_t* ok,
                         size_t* n_mismatch) {
  if (!ctx) return EDC_ERR_ARG;
  int rc = valhash_ready(ctx, true);
  if (rc) return rc;
  if (!nc) {
    if (n_mismatch) *n_mismatch = 0;
    return EDC_OK;
  }
  if (!commit_ver || !expect || !ok) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (nc >= (1ull << 32)) { ctx->err = "validator-set hashes: fewer than 2^32 commits"; return EDC_ERR_ARG; }
  if ((rc = vhist_ready(ctx, nc, commit_ver))) return rc;
  // every distinct version is hashed once: the sorted distinct versions, and per commit its place
  std::vector<uint32_t> vers(commit_ver, commit_ver + nc);
  std::sort(vers.begin(), vers.end());
  vers.erase(std::unique(vers.begin(), vers.end()), vers.end());
  const size_t nd = vers.size();
  uint32_t mx;
  if ((rc = valhash_max_members(ctx, nd, vers.data(), 0, &mx)) || (rc = valhash_ranks(ctx))) return rc;
  // staged in one piece: expect (8 nc words, 16-byte aligned) | the commits' root indices | the versions
  std::vector<uint32_t> in(9 * nc + nd);
  memcpy(in.data(), expect, nc * 32);
  for (size_t c = 0; c < nc; ++c)
    in[8 * nc + c] = (uint32_t)(std::lower_bound(vers.begin(), vers.end(), commit_ver[c]) - vers.begin());
  std::copy(vers.begin(), vers.end(), in.begin() + 9 * nc);
  hipStream_t st = ctx->st();
  CK(grow(ctx->vx_roots, nd * 32, byte_cap, sync_of(st)));
  CK(grow(ctx->vx_in, in.size(), item_cap, sync_of(st)));
  CK(grow(ctx->vx_ok, nc, byte_cap, sync_of(st)));
  CK(hipMemcpyAsync(ctx->vx_in, in.data(), in.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  CK(launch_valhash_roots(st, valhash_src(ctx, true), (uint32_t)nd, ctx->vx_in + 9 * nc, 0, mx, ctx->vx_roots));
  launch_valhash_match(st, (uint32_t)nc, ctx->vx_roots, ctx->vx_in + 8 * nc, reinterpret_cast<const uint8_t*>(ctx->vx_in.get()),
                       ctx->vx_ok);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(st));         // a failed kernel must not leave part of ok written
  CK(hipMemcpy(ok, ctx->vx_ok, nc, hipMemcpyDeviceToHost));
  if (n_mismatch) *n_mismatch = (size_t)std::count(ok, ok + nc, (uint8_t)0);
  return EDC_OK;
}

// Measurement hook: mean times over reps launches of the root kernel over every version of the
// history (ms[0]) and of the address kernel over the registered list (ms[1]).
int edc_debug_valhash_ms(edc_ctx* ctx, int reps, float ms[2]) {
  if (!ctx || reps < 1 || !ms) return EDC_ERR_ARG;
  ms[0] = ms[1] = 0.f;
  int rc = valhash_ready(ctx, true);
  if (rc) return rc;
  const size_t nver = (size_t)ctx->vh.nv + 1;
  uint32_t mx;
  if ((rc = valhash_max_members(ctx, nver, nullptr, 0, &mx)) || (rc = valhash_ranks(ctx))) return rc;
  hipStream_t st = ctx->st();
  DevBuf<uint8_t> d_addr;
  CK(d_addr.alloc((size_t)ctx->kc_reg_m * VALHASH_ADDR_BYTES));
  CK(grow(ctx->vx_roots, nver * 32, byte_cap, sync_of(st)));
  Event e[3];
  for (Event& x : e) CK(x.create());
  CK(hipEventRecord(e[0], st));
  for (int r = 0; r < reps; ++r)
    CK(launch_valhash_roots(st, valhash_src(ctx, true), (uint32_t)nver, nullptr, 0, mx, ctx->vx_roots));
  CK(hipGetLastError());
  CK(hipEventRecord(e[1], st));
  for (int r = 0; r < reps; ++r) launch_valhash_addr(st, ctx->kc_reg_m, ctx->kc_keys, ctx->kc_reg, d_addr);
  CK(hipGetLastError());
  CK(hipEventRecord(e[2], st));
  CK(hipEventSynchronize(e[2]));
  for (int j = 0; j < 2; ++j) {
    float t = 0.f;
    CK(hipEventElapsedTime(&t, e[j], e[j + 1]));
    ms[j] = t / (float)reps;
  }
  return EDC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- header hashes
// edc_header_hashes, edc_header_bind (hdrhash.h, edc_header.hip): what they refuse (header_check
// for the set, the entry's own arguments, header_rules_check for the rules; all of it before any
// device work, so that a refused call has changed nothing), the staging of the set (header_stage),
// then on slot 0's stream the set roots of the named versions (the root kernel of the set hashes),
// the header roots, the rules, one read-back into pinned memory and one synchronization.
struct HeaderCall {
  uint32_t nh = 0, nl = 0, nbytes = 0, max_leaves = 0;
  size_t roots_at() const { return 0; }
  size_t count_at() const { return (size_t)32 * nh; }
  size_t bad_at() const { return (size_t)32 * nh + 16; }
  size_t out_bytes() const { return (size_t)33 * nh + 16; }
};

static int header_check(edc_ctx* ctx, const edc_header_set* hs, HeaderCall* hc) {
  if (!hs || hs->size != sizeof(edc_header_set) || hs->reserved) { ctx->err = "header set: NULL, a wrong size or a non-zero reserved"; return EDC_ERR_ARG; }
  *hc = HeaderCall{};
  if (!hs->nh) return 0;
  if (hs->nh >= (1ull << 32)) { ctx->err = "header set: fewer than 2^32 headers"; return EDC_ERR_ARG; }
  if (!hs->leaf_off || !hs->byte_off) { ctx->err = "header set: null offsets"; return EDC_ERR_ARG; }
  if (hs->leaf_off[0]) { ctx->err = "header set: leaf_off starts at 0"; return EDC_ERR_ARG; }
  uint32_t mx = 0;
  for (size_t h = 0; h < hs->nh; ++h) {
    if (hs->leaf_off[h + 1] < hs->leaf_off[h]) { ctx->err = "header set: leaf_off is not monotone"; return EDC_ERR_ARG; }
    mx = std::max(mx, hs->leaf_off[h + 1] - hs->leaf_off[h]);
  }
  if (mx > HEADER_MAX_LEAVES) { ctx->err = "header set: a header above EDC_HEADER_MAX_LEAVES leaves"; return EDC_ERR_ARG; }
  const uint32_t nl = hs->leaf_off[hs->nh];
  if (hs->byte_off[0]) { ctx->err = "header set: byte_off starts at 0"; return EDC_ERR_ARG; }
  for (size_t j = 0; j < nl; ++j)
    if (hs->byte_off[j + 1] < hs->byte_off[j]) { ctx->err = "header set: byte_off is not monotone"; return EDC_ERR_ARG; }
  const uint32_t nbytes = hs->byte_off[nl];
  if (nbytes && !hs->bytes) { ctx->err = "header set: null bytes"; return EDC_ERR_ARG; }
  if (nbytes >= 0xFFFFFFFFu - 1023) { ctx->err = "header set: fewer than 2^32 - 1024 bytes"; return EDC_ERR_ARG; }
  hc->nh = (uint32_t)hs->nh;
  hc->nl = nl;
  hc->nbytes = nbytes;
  hc->max_leaves = mx;
  return 0;
}

// The set on the device and room for what comes back. The byte array is staged as whole words,
// the last one zeroed first, so that the kernels may read the word of any byte.
static int header_stage(edc_ctx* ctx, const edc_header_set* hs, const HeaderCall& hc, HeaderSrc* src) {
  int rc = init_slot(ctx, ctx->slot[0]);
  if (rc) return rc;
  hipStream_t st = ctx->st();
  const size_t nw = ((size_t)hc.nbytes + 3) / 4;
  CK(grow(ctx->hd_leaf, (size_t)hc.nh + 1, off_cap, sync_of(st)));
  CK(grow(ctx->hd_byte, (size_t)hc.nl + 1, off_cap, sync_of(st)));
  CK(grow(ctx->hd_words, nw, item_cap, sync_of(st)));
  CK(grow(ctx->hd_out, hc.out_bytes(), byte_cap, sync_of(st)));
  CK(grow(ctx->hd_host, hc.out_bytes(), byte_cap, sync_of(st)));
  CK(hipMemcpyAsync(ctx->hd_leaf, hs->leaf_off, ((size_t)hc.nh + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(ctx->hd_byte, hs->byte_off, ((size_t)hc.nl + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (nw) {
    CK(hipMemsetAsync(ctx->hd_words + (nw - 1), 0, sizeof(uint32_t), st));
    CK(hipMemcpyAsync(ctx->hd_words, hs->bytes, hc.nbytes, hipMemcpyHostToDevice, st));
  }
  *src = HeaderSrc{hc.nh, ctx->hd_leaf, ctx->hd_byte, ctx->hd_words};
  return 0;
}

// the entries' common front: the context's device, the set, slot 0
static int header_ready(edc_ctx* ctx, const edc_header_set* hs, HeaderCall* hc) {
  CK(hipSetDevice(ctx->device));
  const int rc = header_check(ctx, hs, hc);
  if (rc) return rc;
  return claim_slot0(ctx) ? 0 : EDC_ERR_ARG;
}

extern "C" {

int edc_header_hashes(edc_ctx* ctx, const edc_header_set* hs, uint8_t* out) {
  if (!ctx) return EDC_ERR_ARG;
  HeaderCall hc;
  int rc = header_ready(ctx, hs, &hc);
  if (rc) return rc;
  if (!hc.nh) return EDC_OK;
  if (!out) { ctx->err = "null output"; return EDC_ERR_ARG; }
  HeaderSrc src;
  if ((rc = header_stage(ctx, hs, hc, &src))) return rc;
  hipStream_t st = ctx->st();
  launch_header_roots(st, src, hc.max_leaves, ctx->hd_out);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->hd_host, ctx->hd_out, (size_t)32 * hc.nh, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));         // out is written only by a call that succeeds
  memcpy(out, ctx->hd_host, (size_t)32 * hc.nh);
  return EDC_OK;
}

int edc_header_bind(edc_ctx* ctx, const edc_header_set* hs, const edc_header_rules* r, uint8_t* bad, uint8_t* out,
                    size_t* n_bad) {
  if (!ctx) return EDC_ERR_ARG;
  HeaderCall hc;
  int rc = header_ready(ctx, hs, &hc);
  if (rc) return rc;
  if (!r || r->size != sizeof(edc_header_rules) || r->reserved) { ctx->err = "header rules: NULL, a wrong size or a non-zero reserved"; return EDC_ERR_ARG; }
  if (!hc.nh) {
    if (n_bad) *n_bad = 0;
    return EDC_OK;
  }
  if (!bad) { ctx->err = "null output"; return EDC_ERR_ARG; }
  const size_t nh = hc.nh;
  // every distinct version either array names is hashed once: the sorted distinct versions, and
  // per header its place among them
  const bool by_ver = r->vals_ver || r->next_ver;
  std::vector<uint32_t> vers;
  uint32_t mx = 0;
  if (by_ver) {
    if (!ctx->kc_reg_m) { ctx->err = "no registered key list (edc_keycache_load)"; return EDC_ERR_ARG; }
    if ((rc = vhist_ready(ctx, 0, nullptr))) return rc;
    for (const uint32_t* ver : {r->vals_ver, r->next_ver}) {
      if (!ver) continue;
      for (size_t h = 0; h < nh; ++h) {
        if (ver[h] == EDC_HEADER_NONE) continue;
        if (ver[h] > ctx->vh.nv) { ctx->err = "header rules: a version past the history's last"; return EDC_ERR_ARG; }
        vers.push_back(ver[h]);
      }
    }
    std::sort(vers.begin(), vers.end());
    vers.erase(std::unique(vers.begin(), vers.end()), vers.end());
    if ((rc = valhash_max_members(ctx, vers.size(), vers.data(), 0, &mx))) return rc;
  }
  if (r->link)
    for (size_t h = 0; h < nh; ++h)
      if (r->link[h] != EDC_HEADER_NONE && r->link[h] >= nh) { ctx->err = "header rules: a link past the set's last header"; return EDC_ERR_ARG; }
  const size_t nd = vers.size();
  if ((rc = init_slot(ctx, ctx->slot[0])) || (nd && (rc = valhash_ranks(ctx)))) return rc;
  // staged in one piece: vals index | next index | link | the versions, each part only when asked for
  std::vector<uint32_t> meta;
  size_t at_vals = 0, at_next = 0, at_link = 0, at_vers = 0;
  auto place = [&](const uint32_t* ver, size_t* at) {
    if (!ver) return;
    *at = meta.size();
    for (size_t h = 0; h < nh; ++h)
      meta.push_back(ver[h] == EDC_HEADER_NONE ? EDC_HEADER_NONE
                                               : (uint32_t)(std::lower_bound(vers.begin(), vers.end(), ver[h]) - vers.begin()));
  };
  place(r->vals_ver, &at_vals);
  place(r->next_ver, &at_next);
  if (r->link) {
    at_link = meta.size();
    meta.insert(meta.end(), r->link, r->link + nh);
  }
  at_vers = meta.size();
  meta.insert(meta.end(), vers.begin(), vers.end());

  HeaderSrc src;
  if ((rc = header_stage(ctx, hs, hc, &src))) return rc;
  hipStream_t st = ctx->st();
  if (r->expect) {
    CK(grow(ctx->hd_expect, nh * 8, item_cap, sync_of(st)));
    CK(hipMemcpyAsync(ctx->hd_expect, r->expect, nh * 32, hipMemcpyHostToDevice, st));
  }
  if (!meta.empty()) {
    CK(grow(ctx->hd_meta, meta.size(), item_cap, sync_of(st)));
    CK(hipMemcpyAsync(ctx->hd_meta, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  if (nd) {
    CK(grow(ctx->vx_roots, nd * 32, byte_cap, sync_of(st)));
    CK(launch_valhash_roots(st, valhash_src(ctx, true), (uint32_t)nd, ctx->hd_meta + at_vers, 0, mx, ctx->vx_roots));
  }
  uint8_t* const d_out = ctx->hd_out;
  uint32_t* const d_cnt = reinterpret_cast<uint32_t*>(d_out + hc.count_at());
  CK(hipMemsetAsync(d_cnt, 0, 16, st));
  launch_header_roots(st, src, hc.max_leaves, d_out + hc.roots_at());
  HeaderBind hb{};
  hb.expect = r->expect ? ctx->hd_expect.get() : nullptr;
  hb.vals_idx = r->vals_ver ? ctx->hd_meta + at_vals : nullptr;
  hb.next_idx = r->next_ver ? ctx->hd_meta + at_next : nullptr;
  hb.link = r->link ? ctx->hd_meta + at_link : nullptr;
  hb.set_roots = nd ? reinterpret_cast<const uint32_t*>(ctx->vx_roots.get()) : nullptr;
  hb.vals_leaf = r->vals_leaf; hb.vals_pos = r->vals_pos;
  hb.next_leaf = r->next_leaf; hb.next_pos = r->next_pos;
  hb.link_leaf = r->link_leaf; hb.link_pos = r->link_pos;
  launch_header_bind(st, src, hb, d_out + hc.roots_at(), d_out + hc.bad_at(), d_cnt);
  CK(hipGetLastError());
  // the bad bytes, the count and, when asked for, the roots: one copy, one synchronization
  const size_t from = out ? hc.roots_at() : hc.count_at();
  uint8_t* const host = ctx->hd_host;
  CK(hipMemcpyAsync(host + from, d_out + from, hc.out_bytes() - from, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));         // a failed kernel must not leave part of an output written
  memcpy(bad, host + hc.bad_at(), nh);
  if (out) memcpy(out, host + hc.roots_at(), nh * 32);
  if (n_bad) {
    uint32_t c;
    memcpy(&c, host + hc.count_at(), sizeof(c));
    *n_bad = c;
  }
  return EDC_OK;
}

// Measurement hook: mean times over reps launches of the root kernel over hs (ms[0]) and of the
// bind kernel with all four compares per header, each against the header's own root (expect, and
// the leaves 7, 8 and 4 at position 2), which needs no history (ms[1]).
int edc_debug_header_ms(edc_ctx* ctx, const edc_header_set* hs, int reps, float ms[2]) {
  if (!ctx || reps < 1 || !ms) return EDC_ERR_ARG;
  HeaderCall hc;
  int rc = header_ready(ctx, hs, &hc);
  if (rc) return rc;
  ms[0] = ms[1] = 0.f;
  if (!hc.nh) return EDC_OK;
  HeaderSrc src;
  if ((rc = header_stage(ctx, hs, hc, &src))) return rc;
  hipStream_t st = ctx->st();
  std::vector<uint32_t> own(hc.nh);
  for (uint32_t h = 0; h < hc.nh; ++h) own[h] = h;
  CK(grow(ctx->hd_meta, own.size(), item_cap, sync_of(st)));
  CK(hipMemcpyAsync(ctx->hd_meta, own.data(), own.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  uint8_t* const d_out = ctx->hd_out;
  const uint32_t* const d_roots = reinterpret_cast<const uint32_t*>(d_out + hc.roots_at());
  uint32_t* const d_cnt = reinterpret_cast<uint32_t*>(d_out + hc.count_at());
  CK(hipMemsetAsync(d_cnt, 0, 16, st));
  const HeaderBind hb{d_roots, ctx->hd_meta, ctx->hd_meta, ctx->hd_meta, d_roots, 7, 2, 8, 2, 4, 2};
  Event e[3];
  for (Event& x : e) CK(x.create());
  CK(hipEventRecord(e[0], st));
  for (int i = 0; i < reps; ++i) launch_header_roots(st, src, hc.max_leaves, d_out + hc.roots_at());
  CK(hipGetLastError());
  CK(hipEventRecord(e[1], st));
  for (int i = 0; i < reps; ++i) launch_header_bind(st, src, hb, d_out + hc.roots_at(), d_out + hc.bad_at(), d_cnt);
  CK(hipGetLastError());
  CK(hipEventRecord(e[2], st));
  CK(hipEventSynchronize(e[2]));
  for (int j = 0; j < 2; ++j) {
    float t = 0.f;
    CK(hipEventElapsedTime(&t, e[j], e[j + 1]));
    ms[j] = t / (float)reps;
  }
  return EDC_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- validator-set requests
// edc_vq_verify: the stages above composed behind one request. Every form is the request's checks
// and staging, then the join (QuorumJoin) in front of the selection the form's pipeline already
// enqueues and the double-vote scan behind it:
//   plain            quorum_run with the join: join, selection, scan, one read-back, gather, quorum_finish
//   plain cached     cached_quorum_run with the join: ... scan, masked lookup, one read-back, ...
//   templated        tmpl_quorum_list with the join, then quorum_finish
//   templated cached tmpl_quorum_list with the join, then cached_tmpl_finish
// The plain forms' body, vq_run_plain, stands with the validator-set entries above, which are that
// body on a request of their own making; the templated forms' is vq_run_tmpl here. What is the
// request's alone is in front of the bodies (the structures' sizes, vq_entry_done) and behind them
// (the debug record).
// A host request by key position (key_idx) stages 4 bytes per key and expands the keys on the
// device (stage_keys_sigs), as every host form does; the join still resolves by position. Gathers
// that take the kept keys by position instead were measured level with this (DESIGN.md,
// "Validator-set requests") and are not kept.

// The sizes a structure may name: the one before the trusting pair's fields were appended, and
// today's. With the earlier one the appended fields read as NULL.
constexpr uint32_t VQ_REQUEST_SIZE_0 = offsetof(edc_vq_request, trust_ver);
constexpr uint32_t VQ_RESULT_SIZE_0 = offsetof(edc_vq_result, trust_verdicts);

static bool vq_sizes_ok(const edc_vq_request* rq, const edc_vq_result* rs) {
  return rq && rs && (rq->size == sizeof(edc_vq_request) || rq->size == VQ_REQUEST_SIZE_0) &&
         (rs->size == sizeof(edc_vq_result) || rs->size == VQ_RESULT_SIZE_0);
}

// the checks that read no array, then nc == 0; true: *rc is the entry's result. rq / rs: the
// caller's structures copied into today's layout (vq_sizes_ok has passed unless ctx->err is set here).
static bool vq_entry_done(edc_ctx* ctx, bool sizes_ok, const edc_vq_request* rq, const edc_vq_result* rs,
                          const QuorumOut& out, const QuorumTrust* tr, int* rc) {
  *rc = EDC_ERR_ARG;
  if (!ctx || !rq || !rs) return true;
  if (!sizes_ok) {
    ctx->err = "edc_vq_verify: size is the caller's sizeof of the structure";
    return true;
  }
  if (!rq->trust_ver != !rq->trust_threshold) { ctx->err = "trust_ver and trust_threshold are given together"; return true; }
  if (rq->trust_ver && !rq->commit_ver) { ctx->err = "trust_ver needs commit_ver: a trusting pair needs the history"; return true; }
  if (rq->reserved || rs->reserved || rq->device > 1) { ctx->err = "edc_vq_verify: reserved fields are 0, device is 0 or 1"; return true; }
  if (!rq->z_seed) { ctx->err = "null z_seed"; return true; }
  if (!rq->vk == !rq->key_idx) { ctx->err = "exactly one of vk and key_idx"; return true; }
  if (rq->device && rq->key_idx) { ctx->err = "key_idx is a host form's: a device request passes vk"; return true; }
  if ((rq->msg_off ? 1 : 0) + (rq->k ? 1 : 0) + (rq->ts ? 1 : 0) != 1 || (rq->msg && !rq->msg_off)) {
    ctx->err = "exactly one of (msg, msg_off), k and a template description";
    return true;
  }
  if (!rq->ts && (rq->commit_tpl || rq->alt_span || rq->item_alt || rq->var || rq->var_off || rq->var_bytes)) {
    ctx->err = "template fields without a template set";
    return true;
  }
  if (rq->cached && (*rc = cq_ready(ctx))) return true;
  if (!rq->nc) { *rc = quorum_none(out, tr); return true; }
  return false;
}

// the templated forms: checks, staging, tmpl_quorum_list with the join, the finish
static int vq_run_tmpl(edc_ctx* ctx, const edc_vq_request* rq, const QuorumOut& out, const QuorumTrust* tr) {
  const size_t nc = rq->nc;
  TmplShape sh;
  size_t n;
  int rc;
  if (rq->device)
    rc = commits_check_tmpl_device(ctx, rq->ts, nc, rq->commit_off, rq->commit_tpl, rq->alt_span, rq->vk, rq->sig, rq->var,
                                   rq->var_off, rq->var_bytes, &sh, &n);
  else
    rc = commits_check_tmpl(ctx, rq->ts, nc, rq->commit_off, rq->commit_tpl, true, rq->alt_span, rq->item_alt, rq->vk,
                            rq->key_idx, rq->sig, rq->var, rq->var_off, &sh, &n);
  if (rc || (rc = quorum_check(ctx, nc, rq->commit_off, rq->threshold, rq->mode, &n)) ||
      (rc = rq->commit_ver ? vhist_ready(ctx, nc, rq->commit_ver) : valset_ready(ctx)) || (rc = vq_trust_ready(ctx, nc, tr)))
    return rc;
  if (n && !rq->flag) { ctx->err = "null input"; return EDC_ERR_ARG; }
  CK(hipSetDevice(ctx->device));
  if ((rc = valset_room(ctx, n, nc, rq->commit_ver != nullptr, tr != nullptr))) return rc;
  hipStream_t st = ctx->st();
  TmplQuorumItems it{rq->vk, rq->sig, rq->item_alt, rq->var, rq->var_off, rq->var_bytes, ctx->qw.a.power, ctx->qw.a.flag};
  QuorumJoin jn{rq->vk, nullptr, rq->flag, rq->commit_ver, nullptr, {}, tr};
  if (!rq->device) {
    if ((rc = ensure_n(ctx, n))) return rc;
    it = TmplQuorumItems{ctx->vk, ctx->sig, nullptr, nullptr, nullptr, 0, ctx->qw.a.power, ctx->qw.a.flag};
    if (n) {                    // 4 + 64 + 1 bytes per vote and its hole in the key_idx form
      CK(hipMemcpyAsync(ctx->qw.vflag, rq->flag, n, hipMemcpyHostToDevice, st));
      if ((rc = tmpl_quorum_stage_holes(ctx, n, rq->item_alt, rq->var, rq->var_off, &it)) ||
          (rc = stage_keys_sigs(ctx, st, n, rq->vk, rq->key_idx, rq->sig, ctx->qw.kidx, ctx->vk, ctx->sig)))
        return rc;
    }
    jn.d_vk = rq->key_idx ? nullptr : ctx->vk.get();
    jn.d_kidx = ctx->qw.kidx;
    jn.d_flag = ctx->qw.vflag;
  }
  ItemList list;
  if ((rc = tmpl_quorum_list(ctx, rq->ts, sh, nc, rq->commit_off, rq->commit_tpl, rq->alt_span, n, it, rq->threshold,
                             rq->mode, &list, &jn)))
    return rc;
  return tmpl_quorum_done(ctx, rq->cached ? cached_tmpl_finish(ctx, nc, rq->threshold, n, list, it.power, it.flag,
                                                               rq->z_seed, out, ctx->qw.a.hdv, tr)
                                          : quorum_finish(ctx, nc, rq->threshold, n, list, it.power, it.flag, rq->z_seed,
                                                          out, nullptr, ctx->qw.a.hdv, tr));
}

extern "C" {

int edc_vq_verify(edc_ctx* ctx, const edc_vq_request* rq_in, edc_vq_result* rs_in) {
  size_t m = 0, miss = 0;
  QuorumOut out{nullptr, nullptr, nullptr, nullptr, &m, nullptr, nullptr};
  // the caller's structures in today's layout: fields past an earlier sizeof read as NULL
  edc_vq_request q;
  edc_vq_result r;
  memset(&q, 0, sizeof(q));
  memset(&r, 0, sizeof(r));
  const bool sizes_ok = vq_sizes_ok(rq_in, rs_in);
  if (sizes_ok) {
    memcpy(&q, rq_in, rq_in->size);
    memcpy(&r, rs_in, rs_in->size);
  }
  const edc_vq_request* rq = rq_in ? &q : nullptr;
  const edc_vq_result* rs = rs_in ? &r : nullptr;
  const QuorumTrust trust{q.trust_ver, q.trust_threshold, r.trust_verdicts, r.trust_tally, r.n_bad_trust};
  const QuorumTrust* tr = q.trust_ver ? &trust : nullptr;
  if (sizes_ok)
    out = QuorumOut{rs->commit_verdicts, rs->item_verdicts, rs->tally, rs->n_bad_commits,
                    rs->n_checked ? rs->n_checked : &m, rq->cached ? (rs->n_miss ? rs->n_miss : &miss) : nullptr,
                    rs->check8};
  int rc;
  if (vq_entry_done(ctx, sizes_ok, rq, rs, out, tr, &rc)) return rc;
  size_t hashed = 0;
  rc = rq->ts ? vq_run_tmpl(ctx, rq, out, tr) : vq_run_plain(ctx, rq, out, tr, &hashed);
  if (rc < 0) return rc;
  // the debug record, from the records of the stages that ran
  const uint64_t n = rq->commit_off[rq->nc];
  uint64_t* L = ctx->qw.vq_last;
  L[0] = n;
  L[1] = *out.n_checked;
  L[2] = rq->cached ? ctx->qw.cq_last[2] : 0;
  L[3] = rq->cached ? ctx->qw.cq_last[3] : 0;
  L[4] = rq->ts ? ctx->qw.tq_last[2] : hashed;
  L[5] = rq->cached ? ctx->qw.cq_last[5] : 0;
  L[6] = 0;     // reserved
  L[7] = rq->ts ? ctx->qw.tq_last[3] : 0;
  ctx->qw.vq_have = true;
  return rc;
}

int edc_debug_vq_last(const edc_ctx* ctx, uint64_t out[8]) {
  if (!ctx || !out || !ctx->qw.vq_have) return EDC_ERR_ARG;
  memcpy(out, ctx->qw.vq_last, sizeof(ctx->qw.vq_last));
  return EDC_OK;
}

int edc_debug_vq_trust_last(const edc_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out || !ctx->qw.vqt_have) return EDC_ERR_ARG;
  memcpy(out, ctx->qw.vqt_last, sizeof(ctx->qw.vqt_last));
  return EDC_OK;
}

// edc_vhist_resolve with the trusting side: the paired join, both selections, the union and both
// double-vote scans, as the request runs them.
int edc_vq_trust_resolve(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                         const uint32_t* trust_ver, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag,
                         const uint64_t* threshold, const uint64_t* trust_threshold, int mode, uint32_t* pos, uint64_t* power,
                         uint8_t* flag_out, uint8_t* checked, uint64_t* planned, uint8_t* dv, uint32_t* trust_pos,
                         uint64_t* trust_power, uint8_t* trust_flag_out, uint8_t* trust_checked, uint64_t* trust_planned,
                         uint8_t* trust_dv, uint8_t* side, size_t* n_checked) {
  const QuorumTrust tr{trust_ver, trust_threshold, nullptr, nullptr, nullptr};
  return valset_resolve_body(ctx, true, nc, commit_off, commit_ver, vk, key_idx, flag, threshold, mode,
                             ResolveSide{pos, power, flag_out, checked, planned, dv}, n_checked, &tr,
                             ResolveSide{trust_pos, trust_power, trust_flag_out, trust_checked, trust_planned, trust_dv}, side);
}

// edc_debug_vhist_select for a pair, with the selections between the join and the scans: ms[0] the
// paired join, ms[1] both selections, the union and the scan of its tile counts, ms[2] both
// double-vote scans with the clearing of their sets.
int edc_debug_vq_trust_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                              const uint32_t* trust_ver, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag,
                              const uint64_t* threshold, const uint64_t* trust_threshold, int mode, int reps, float ms[3]) {
  const QuorumTrust tr{trust_ver, trust_threshold, nullptr, nullptr, nullptr};
  return valset_debug_select_body(ctx, true, nc, commit_off, commit_ver, vk, key_idx, flag, threshold, mode, reps, 3, ms, &tr);
}

}  // extern "C"

// ---------------------------------------------------------------- incremental verifier
// Verifier::queue does the per-item work (src/batch.rs:82-94, :127-137) and Verifier::verify(rng)
// only evaluates the equation (:149-217). Here every queue call enqueues, for the appended range
// alone, the copies, SHA-512 -> k, the ZIP215 decode of R_i into its final row 1 + i, the key
// find-or-insert against the persistent table and the decode of the keys first seen in the range.
// verify then runs what depends on z: coefficients, binning, sort, accumulation, reduction, window
// combine and Horner.
// Point layout: the batch layout puts key j at row 1 + n + j, and n is only known at verify. Keys
// are decoded at queue time into a key area and k_verifier_place_keys moves the m rows into place
// at verify: 128 bytes per distinct key, and the MSM then runs the very batch path (same terms,
// same plan, same kernels) as edc_batch_verify_device, so results are bit-identical by construction.
// The listed-terms path would need no move but changes the term order and drops the sub-bin split.
// Split coefficients (edc_common.h): while the context holds a key cache, queue time also leaves
// every new key's [2^128] row in a second key area, and verify places the split layout (2m + 1
// rows from 1 + n). That layout reaches row 2 + n + 2m <= 2 + 3 cap_n, i.e. the whole point
// table, so the key areas are the verifier's own allocation (2 x 128 bytes per item of capacity)
// and no placement can overwrite a row that it, or a later verify of the same queue, still reads.
static uint32_t* verifier_kpts(edc_verifier* v) { return v->karea; }
static uint32_t* verifier_khi(edc_verifier* v) { return v->karea + v->karea_cap * NIELS_WORDS; }

// the split plan is possible for a verify now (choose_split without the one-call path's back-off
// after uncached keys: their doublings were done at queue time)
static bool verifier_split(const edc_verifier* v) {
  const edc_ctx* ctx = v->ctx;
  return ctx->kc_m && ctx->bcomb && ctx->key_split == 0 && v->hi_ok && v->hi_gen == ctx->kc_gen;
}

// flags, key table (sized for the verifier's capacity, with a fresh salt) and the R bits of a
// verifier with nothing queued
static int verifier_clear(edc_verifier* v) {
  edc_ctx* ctx = v->ctx;
  Slot& s = v->s;
  KeyTable kt;
  const int rc = key_table(ctx, s, v->cap, false, kt);
  v->T = kt.T;
  if (rc) return rc;
  v->salt[0] = kt.salt[0];
  v->salt[1] = kt.salt[1];
  launch_init_batch(s.st, s.flags, -1, s.u_acc, s.d_out, s.table, v->T, nullptr, 0);
  CK(hipGetLastError());
  return 0;
}

// Enqueue the z-independent work of items [n0, n0 + m), whose vk / sig / k are in place (or land
// before the slot stream's next event wait): R decode, key find-or-insert, decode of new keys.
static int verifier_enqueue_range(edc_verifier* v, size_t n0, size_t m) {
  edc_ctx* ctx = v->ctx;
  Slot& s = v->s;
  if (!m) return 0;
  // [2^128] rows: the first range after a reset (or a rebuild of everything queued) opens the
  // window; a later range queued without a cache, or against another one, closes it
  const bool cache = ctx->kc_m && ctx->bcomb;
  if (n0 == 0) {
    v->hi_gen = ctx->kc_gen;
    v->hi_ok = cache;
  } else if (!cache || ctx->kc_gen != v->hi_gen) {
    v->hi_ok = false;
  }
  launch_decompress_range(s.st, (uint32_t)(n0 + m), (uint32_t)n0, (uint32_t)m, 0, v->sig, v->vk, s.key_rep, false, s.pts,
                          s.itembad + s.cap_n, s.keybad, s.flags, ctx->kc(), false);
  launch_keys_range(s.st, (uint32_t)n0, (uint32_t)m, v->vk, s.table, v->T - 1, v->salt,
                    ctx->key_grouping == 2 || ctx->key_grouping == 3, n0 == 0, s.slot_key, s.key_slot, s.key_rep,
                    s.key_index, s.key_acc, verifier_kpts(v), verifier_khi(v), s.keybad, s.flags, ctx->kc());
  CK(hipGetLastError());
  return 0;
}

// Room for `need` items. Growing copies the retained bytes, resizes the key table and redoes the
// z-independent work of everything queued (R rows, grouping, key decode) in the new workspace:
// the same kernels over the same bytes, so growth never changes a result.
static int verifier_reserve(edc_verifier* v, size_t need) {
  edc_ctx* ctx = v->ctx;
  Slot& s = v->s;
  if (need <= v->cap && v->vk) return 0;
  if (need >= (1ull << 28)) { ctx->err = "batch too large for one verifier (max 2^28 items)"; return EDC_ERR_ARG; }
  if (s.st) CK(hipStreamSynchronize(s.st));
  if (v->cs) CK(hipStreamSynchronize(v->cs));
  size_t cap = v->cap * 2 > need ? v->cap * 2 : need;
  if (cap < 1) cap = 1;
  // the new arrays are the verifier's only once they are all there and filled
  DevBuf<uint8_t> nvk, nsig, nz;
  DevBuf<uint32_t> nk, norg;
  CK(nvk.alloc(cap * 32));
  CK(nsig.alloc(cap * 64));
  CK(nz.alloc(cap * 16));
  CK(nk.alloc(cap * 8));
  if (v->cached.on) CK(norg.alloc(cap));   // only a cached verifier keeps offered positions
  if (v->n) {
    CK(hipMemcpy(nvk, v->vk, v->n * 32, hipMemcpyDeviceToDevice));
    CK(hipMemcpy(nsig, v->sig, v->n * 64, hipMemcpyDeviceToDevice));
    CK(hipMemcpy(nk, v->k, v->n * 32, hipMemcpyDeviceToDevice));
    if (v->cached.on) CK(hipMemcpy(norg, v->origin, v->n * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  }
  v->origin = std::move(norg);
  v->vk = std::move(nvk);
  v->sig = std::move(nsig);
  v->zexp = std::move(nz);
  v->k = std::move(nk);
  v->cap = cap;
  int rc = ensure_slot(ctx, s, cap);
  if (rc) return rc;
  if (v->karea_cap != s.cap_n) {
    v->karea_cap = 0;
    CK(v->karea.alloc(2 * s.cap_n * NIELS_WORDS));
    v->karea_cap = s.cap_n;
  }
  s.kin = v->k;
  rc = verifier_clear(v);
  if (rc) return rc;
  return verifier_enqueue_range(v, 0, v->n);
}

// The message arena of one append: reused by the next one once its SHA-512 pass has run.
static int verifier_msg_room(edc_verifier* v, size_t m, size_t mbytes) {
  edc_ctx* ctx = v->ctx;
  CK(grow(v->msg, mbytes, byte_cap, sync_of(v->s.st)));
  CK(grow(v->off, m + 1, off_cap, sync_of(v->s.st)));
  return 0;
}

// ---- eager mode (edc_vfy_begin_eager) ----
// Plan of a fold: every term is a 128-bit z, so there are no windows above bit 128 (the layout of
// the split plan), and the slices are split into sub-bins as batch_plan splits them.
static MsmPlan fold_plan(edc_ctx* ctx, size_t cnt) {
  const int c = ctx->win_bits ? ctx->win_bits : auto_window_bits(cnt);
  MsmPlan P = make_plan(c, c, 1, false);
  const double total = (double)cnt * P.nwin;
  double target = ctx->bin_entries ? (double)ctx->bin_entries : (total / 1024.0 > 4096.0 ? total / 1024.0 : 4096.0);
  for (;;) {
    for (uint32_t w = 0; w < P.nwin; ++w) P.nsub[w] = (uint8_t)floor_pow2((double)cnt / P.nslice[w] / target);
    plan_layout(P);
    if (P.bins_per_range <= MSM_MAX_BINS) break;
    target *= 2;
  }
  note_plan(ctx, P, target, false, false, false, true);
  return P;
}

// After a queue call: once enough items are pending, sum [z_i]R_i over the pending range
// [folded, n) as an R-only MSM on the slot stream (z from the committed seed at the items' queue
// indices, the R rows the range's decode left in s.pts) and add the sum into the running point.
// No host synchronization. A range holding an undecodable R has set FLAG_BAD before its fold runs
// (same stream), and k_msm_final then reports the identity as the fold's partial point: the
// running point stays a point of the curve and the batch is rejected by the flag at verify.
static int verifier_fold(edc_verifier* v) {
  size_t a, b;
  if (!fold_due(v->fold, v->n, &a, &b)) return 0;
  edc_ctx* ctx = v->ctx;
  Slot& s = v->s;
  const uint32_t cnt = (uint32_t)(b - a);
  const MsmPlan P = fold_plan(ctx, cnt);
  v->last_plan = ctx->last_plan;
  v->have_plan = true;
  int rc = ensure_msm(ctx, s, P, msm_entry_capacity(P, cnt, 0));
  if (rc) return rc;
  uint32_t seed[8];
  seed_words(v->eager_seed, seed);
  hipStream_t st = s.st;
  launch_z_range(st, seed, (uint32_t)a, cnt, s.scal);
  // one range of cnt short terms, term t = R of item a + t (MsmTerms::skip)
  const MsmTerms terms{cnt, 0x80000000u, cnt, 0u, 1u, s.scal, nullptr, nullptr, nullptr, 0u, 0u, (uint32_t)a};
  launch_msm_bin(st, P, terms, cnt, s.msm, s.flags);
  launch_msm_sort(st, P, s.msm);
  launch_msm_bucket(st, P, s.msm, s.pts, 0, nullptr, nullptr, true, s.flags);
  uint8_t* blk = reinterpret_cast<uint8_t*>(v->run + 64);
  launch_msm_tail(st, P, s.msm, s.flags, 0, blk);
  launch_point_accum(st, v->run, blk);
  CK(hipGetLastError());
  fold_done(v->fold, b);
  return 0;
}

// a failed eager verify has revealed a z-dependent point: no more queue / verify under that seed
static int verifier_spent(edc_verifier* v) {
  if (!(v->fold.eager && v->fold.spent)) return 0;
  v->ctx->err = "eager verifier: the seed is spent after a failed verify (edc_verifier_reset, then edc_vfy_begin_eager)";
  return EDC_ERR_ARG;
}

// ---- cached mode (edc_vfy_set_cached) ----
// A queue call brings its range to the device (the staging area, or a device caller's own arrays),
// looks it up in the context's verified-signature table and appends only the misses, in offered
// order, to the retained arrays; from there on they are queued items like any other, so verify,
// the folds and the fallback run unchanged over the retained items. What a verdict proves valid
// is inserted behind it on the verifier's stream (verifier_insert).

// what a cached queue call of m items needs, checked before anything is copied
static int verifier_cached_check(edc_verifier* v, size_t m) {
  edc_ctx* ctx = v->ctx;
  if (!ctx->sc_cap) {
    ctx->err = "cached verifier: no signature cache on this context (edc_sigcache_create)";
    return EDC_ERR_ARG;
  }
  if (m >= (1ull << 28)) { ctx->err = "batch too large for one verifier (max 2^28 items)"; return EDC_ERR_ARG; }
  if (!cached_room(v->cached, m)) {
    ctx->err = "cached verifier: more than 2^32 - 1 items offered since the last reset";
    return EDC_ERR_ARG;
  }
  return 0;
}

// Staging for a range of m items (vk, sig, k, hit flags, workgroup counts). The previous range's
// gather is the last reader of the old contents: the copy stream waits for it.
static int verifier_stage_room(edc_verifier* v, size_t m) {
  edc_ctx* ctx = v->ctx;
  if (!v->h_cnt) CK(v->h_cnt.alloc(2));
  if (!v->ev_cnt) CK(v->ev_cnt.create(hipEventDisableTiming));
  if (!v->ev_gather) CK(v->ev_gather.create(hipEventDisableTiming));
  CK(grow_group(v->st_cap, m, item_cap, sync_of(v->s.st, v->cs), [&](size_t cap) {
    v->gather_pending = false;   // both streams are drained
    return alloc_all(sized(v->st_vk, cap * 32), sized(v->st_sig, cap * 64), sized(v->st_k, cap * 8), sized(v->hit, cap),
                     sized(v->wg, cap / SC_BLOCK + 2));   // one count per workgroup + the total
  }));
  if (v->gather_pending) CK(hipStreamWaitEvent(v->cs, v->ev_gather, 0));
  return 0;
}

// The rest of a cached queue call, once everything that produces the range's vk / sig / k (at
// s_*) is on the slot stream or ordered before it: lookup, miss count to the host (the call's one
// added synchronization), room for the misses, gather, and the per-item work of the appended
// misses. in_place: s_* are a device caller's arrays, which the gather still reads, so the call
// also waits for the gather.
static int verifier_append_misses(edc_verifier* v, size_t m, const uint8_t* s_vk, const uint8_t* s_sig,
                                  const uint32_t* s_k, bool in_place) {
  edc_ctx* ctx = v->ctx;
  hipStream_t st = v->s.st;
  int rc = sc_order_after_inserts(ctx, st);
  if (rc) return rc;
  const uint32_t M = (uint32_t)m, nwg = (M + SC_BLOCK - 1) / SC_BLOCK;
  launch_sc_lookup(st, ctx->sc(), M, s_vk, s_sig, s_k, v->hit, v->wg);
  launch_sc_scan(st, nwg, v->wg, v->wg + nwg);
  CK(hipGetLastError());
  v->h_cnt[0] = 0xFFFFFFFFu;
  CK(hipMemcpyAsync(v->h_cnt, v->wg + nwg, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  CK(hipEventRecord(v->ev_cnt, st));
  CK(hipEventSynchronize(v->ev_cnt));
  v->chal_pending = false;      // a SHA-512 pass of this range ran before its lookup
  const size_t c = v->h_cnt[0], n0 = v->n;
  if (c > m) { ctx->err = "cached verifier: miss count out of range"; return EDC_ERR_HIP; }
  ctx->sc_hits += m - c;        // the table's statistics count the lookup, whatever becomes of the append
  ctx->sc_misses += c;
  if (c) {
    if ((rc = verifier_reserve(v, n0 + c))) return rc;
    launch_sc_gather_range(st, M, v->hit, v->wg, s_vk, s_sig, s_k, (uint32_t)v->cached.offered, n0, v->vk, v->sig,
                           v->k, v->origin);
    CK(hipGetLastError());
    CK(hipEventRecord(v->ev_gather, st));
    v->gather_pending = true;
    rc = verifier_enqueue_range(v, n0, c);
    // a device caller's arrays are not read after the call returns, also when it fails
    if (in_place) CK(hipEventSynchronize(v->ev_gather));
    if (rc) return rc;
  }
  // the range is appended: only now do the verifier's counts move
  cached_offer(v->cached, m, c);
  v->n = n0 + c;
  return 0;
}

// Enqueue, behind the verdict on the verifier's stream, the insert of the retained items that are
// not records yet: all of them (d_codes null: a verify that passed) or those whose retained-order
// code is EDC_OK (a fallback). The counters' mirror is refreshed behind it and the context's event
// recorded; the call returns without waiting.
static int verifier_insert(edc_verifier* v, const uint8_t* d_codes) {
  edc_ctx* ctx = v->ctx;
  size_t a, b;
  if (!cached_insert_due(v->cached, v->n, &a, &b) || !ctx->sc_cap) return 0;
  hipStream_t st = v->s.st;
  if (!ctx->sc_ev) CK(ctx->sc_ev.create(hipEventDisableTiming));
  int rc = sc_order_after_inserts(ctx, st);
  if (rc) return rc;
  launch_sc_insert(st, ctx->sc(), (uint32_t)(b - a), nullptr, v->vk + a * 32, v->sig + a * 64, v->k + a * 8,
                   d_codes ? d_codes + a : nullptr, ctx->sc_ctr);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(ctx->sc_hctr, ctx->sc_ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  CK(hipEventRecord(ctx->sc_ev, st));
  ctx->sc_ev_set = true;
  cached_insert_done(v->cached, b);
  return 0;
}

// After a failed verify's fallback in cached mode: the retained-order codes (host, n bytes) go to
// the device, are scattered through origin into offered order when `offered` (host) is given
// (hits stay EDC_OK), and mask the insert.
static int verifier_codes_out(edc_verifier* v, const uint8_t* verdicts, uint8_t* offered) {
  edc_ctx* ctx = v->ctx;
  hipStream_t st = v->s.st;
  const size_t n = v->n, N = (size_t)v->cached.offered;
  if (n > v->verd.cap()) CK(grow(v->verd, n, [v](size_t) { return v->cap; }, sync_of(st)));
  CK(hipMemcpyAsync(v->verd, verdicts, n, hipMemcpyHostToDevice, st));
  if (offered) {
    if (N > v->offv.cap()) CK(grow(v->offv, N, item_cap, sync_of(st)));
    CK(hipMemsetAsync(v->offv, 0, N, st));
    launch_sc_scatter(st, (uint32_t)n, v->origin, v->verd, v->offv);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(offered, v->offv, N, hipMemcpyDeviceToHost, st));
  }
  CK(hipStreamSynchronize(st));   // the codes have left / reached the caller's memory; the insert is not waited for
  return verifier_insert(v, v->verd);
}

// One append from host buffers (k: prehashed challenges, or null for the message path; key_idx:
// positions in the registered key list instead of vk, 4 bytes per item over PCIe, expanded into the
// retained vk range on the device). The copies run on the copy stream; the call returns once they
// have left the caller's memory.
static int verifier_queue_host(edc_verifier* v, size_t m, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                               const uint64_t* msg_off, const uint8_t* k, const uint32_t* key_idx = nullptr,
                               const TmplItems* tm = nullptr, const TmplShape* tsh = nullptr) {
  edc_ctx* ctx = v->ctx;
  if (m && ((!vk && !key_idx) || !sig || (!k && !msg_off && !tm))) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (verifier_spent(v)) return EDC_ERR_ARG;
  if (!m) return 0;
  if (key_idx && check_key_idx(ctx, m, key_idx)) return EDC_ERR_ARG;
  // templated items (tm, already checked): the arena is built on the device, sized by its bound
  const size_t mbytes = k ? 0 : tm ? tmpl_arena_bound(m, *tsh, tm->var_off[m]) : (size_t)(msg_off[m] - msg_off[0]);
  if (mbytes && !msg && !tm) { ctx->err = "null msg"; return EDC_ERR_ARG; }
  CK(hipSetDevice(ctx->device));
  const bool cached = v->cached.on;
  int rc = cached ? verifier_cached_check(v, m) : 0;
  if (rc) return rc;
  rc = cached ? verifier_stage_room(v, m) : verifier_reserve(v, v->n + m);
  if (rc) return rc;
  Slot& s = v->s;
  const size_t n0 = v->n;
  // where the range lands: the retained arrays from n0 on, or the staging area (cached mode)
  uint8_t* r_vk = cached ? v->st_vk : v->vk + n0 * 32;
  uint8_t* r_sig = cached ? v->st_sig : v->sig + n0 * 64;
  uint32_t* r_k = cached ? v->st_k : v->k + n0 * 8;
  if (!k) {
    rc = verifier_msg_room(v, m, mbytes);
    if (rc) return rc;
    if (v->chal_pending) CK(hipStreamWaitEvent(v->cs, v->ev_chal, 0));
  }
  // (the previous indexed append's expansion reads v->idx on the copy stream)
  if (key_idx) CK(grow(v->idx, m, item_cap, sync_of(v->cs)));
  if ((rc = stage_keys_sigs(ctx, v->cs, m, vk, key_idx, sig, v->idx, r_vk, r_sig))) return rc;
  if (k) {
    CK(hipMemcpyAsync(r_k, k, m * 32, hipMemcpyHostToDevice, v->cs));
  } else if (tm) {
    TmplView view;
    if ((rc = tmpl_upload_set(ctx, s.tw, v->cs, tm->ts, *tsh, &view)) ||
        (rc = tmpl_expand_host(ctx, s.tw, v->cs, view, m, *tm, v->msg, v->off)))
      return rc;
  } else {
    v->rebased.resize(m + 1);
    for (size_t i = 0; i <= m; ++i) v->rebased[i] = msg_off[i] - msg_off[0];
    CK(hipMemcpyAsync(v->off, v->rebased.data(), (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, v->cs));
    if (mbytes) CK(hipMemcpyAsync(v->msg, msg + msg_off[0], mbytes, hipMemcpyHostToDevice, v->cs));
  }
  CK(hipEventRecord(v->ev_copy, v->cs));
  CK(hipStreamWaitEvent(s.st, v->ev_copy, 0));
  if (!k) {
    launch_challenge(s.st, (uint32_t)m, r_vk, r_sig, v->msg, v->off, r_k);
    CK(hipGetLastError());
    CK(hipEventRecord(v->ev_chal, s.st));
    v->chal_pending = true;
  }
  if (cached) {
    // the lookup runs behind the copies, so the wait for its miss count covers them; after an
    // error the copies are waited for all the same
    rc = verifier_append_misses(v, m, r_vk, r_sig, r_k, false);
    const hipError_t e = hipEventSynchronize(v->ev_copy);
    if (rc) return rc;
    CK(e);
    return verifier_fold(v);
  }
  rc = verifier_enqueue_range(v, n0, m);
  if (rc) return rc;
  CK(hipEventSynchronize(v->ev_copy));   // nothing reads the caller's (or the rebased) buffers after this
  v->n = n0 + m;
  return verifier_fold(v);
}

// The z-dependent part over everything queued, on the verifier's slot; no host synchronization.
// Eager (z_seed = the committed seed): the coefficients still run over all n items (the B and key
// sums need every z_i s_i and z_i k_i), but the MSM leaves out the R terms of the `skip` folded
// items, is planned for the nl = n - skip that remain, and k_msm_final adds the running point
// before the x8: the same group element as the whole batch's MSM.
static int verifier_enqueue_verify(edc_verifier* v, const uint8_t* z_seed, const uint8_t* z, int want_compress,
                                   bool eager = false) {
  edc_ctx* ctx = v->ctx;
  Slot& s = v->s;
  const size_t n = v->n, skip = eager ? v->fold.folded : 0, nl = n - skip;
  const uint32_t N = (uint32_t)n;
  const bool split = verifier_split(v);
  const MsmPlan P = batch_plan(ctx, nl, false, split);
  v->last_plan = ctx->last_plan;
  v->have_plan = true;
  // (after a grouping overflow every signature has its own key term: n of them, n + 1 with B)
  int rc = ensure_msm(ctx, s, P, split ? msm_entry_capacity(P, 2 + nl + 2 * n, 0) : msm_entry_capacity(P, nl, n + 1));
  if (rc) return rc;
  v->last_split = split ? 1 : 0;
  uint32_t seed[8];
  seed_words(z_seed, seed);
  hipStream_t st = s.st;
  if (z) CK(hipMemcpyAsync(v->zexp, z, n * 16, hipMemcpyHostToDevice, st));
  slot_begin(s, v->k, 0, false, false, N);   // per_sig false: an overflow (FLAG_OVF) is resolved on the device
  launch_verifier_begin(st, N, s.flags, s.key_acc, s.u_acc, s.d_out, s.msm.counts, P.nbin());
  launch_coef(st, N, v->sig, v->k, z ? v->zexp : nullptr, seed, 0, s.key_index, s.scal, s.key_acc, s.u_acc, s.itembad,
              s.flags, false, s.coef_part, split);
  launch_msm_bin(st, P, batch_terms(P, s, N, split, (uint32_t)skip), (uint32_t)(split ? 2 + nl + 2 * n : 1 + nl + n),
                 s.msm, s.flags, true);
  launch_msm_sort(st, P, s.msm);
  launch_verifier_place_keys(st, N, v->vk, verifier_kpts(v), verifier_khi(v), s.pts, s.keybad, s.flags, ctx->kc(), split);
  launch_msm_bucket(st, P, s.msm, s.pts, 0, nullptr, nullptr, true, s.flags);
  s.acc_nbin = P.nbin();
  launch_msm_tail(st, P, s.msm, s.flags, want_compress, s.d_out, s.h_out, eager ? v->run : nullptr);
  CK(hipGetLastError());
  s.pending = true;
  return 0;
}

static int verifier_verify(edc_verifier* v, const uint8_t* z_seed, const uint8_t* z, uint8_t check8[32],
                           bool plain = false, bool insert = true) {
  edc_ctx* ctx = v->ctx;
  // eager (edc_vfy_begin_eager): z is already committed; `plain` is the fallback's own verify of a
  // spent eager verifier, which draws fresh z from the caller's seed over every item
  const bool eager = v->fold.eager && !plain;
  if (eager) {
    if (z_seed || z) { ctx->err = "eager verifier: z is committed, pass neither z_seed nor z"; return EDC_ERR_ARG; }
    if (verifier_spent(v)) return EDC_ERR_ARG;
  } else if (!z_seed == !z) {
    ctx->err = "exactly one of z_seed and z";
    return EDC_ERR_ARG;
  }
  CK(hipSetDevice(ctx->device));
  if (!v->n) {                  // the empty equation: [8] * identity
    v->last_split = 0;
    if (check8) {
      memset(check8, 0, 32);
      check8[0] = 1;
    }
    return EDC_OK;
  }
  int rc = verifier_enqueue_verify(v, eager ? v->eager_seed : z_seed, z, check8 != nullptr, eager);
  if (rc) return rc;
  rc = finish_batch(ctx, v->s, check8, nullptr, nullptr);
  if (eager && rc == EDC_INVALID_SIGNATURE) v->fold.spent = true;   // a z-dependent point has left the library
  // cached mode: what this verdict proved valid becomes records, behind the verdict and unwaited
  // (`insert` false: the fallback, which inserts by its per-item codes)
  if (rc == EDC_OK && insert) {
    const int r2 = verifier_insert(v, nullptr);
    if (r2) return r2;
  }
  return rc;
}

extern "C" {

edc_verifier* edc_verifier_create(edc_ctx* ctx, size_t capacity_hint) {
  if (!ctx) return nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
  edc_verifier* v = new edc_verifier();
  v->ctx = ctx;
  ctx->verifiers.push_back(v);
  bool ok = init_slot(ctx, v->s) == 0 && v->cs.create(hipStreamNonBlocking) == hipSuccess &&
            v->ev_copy.create(hipEventDisableTiming) == hipSuccess &&
            v->ev_chal.create(hipEventDisableTiming) == hipSuccess &&
            verifier_reserve(v, capacity_hint ? capacity_hint : 1) == 0 && hipStreamSynchronize(v->s.st) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    edc_verifier_destroy(v);
    return nullptr;
  }
  return v;
}

void edc_verifier_destroy(edc_verifier* v) {
  if (!v) return;
  edc_ctx* ctx = v->ctx;
  (void)hipSetDevice(ctx->device);
  Slot& s = v->s;
  if (v->cs) (void)hipStreamSynchronize(v->cs);
  if (s.st) (void)hipStreamSynchronize(s.st);
  ctx->verifiers.erase(std::remove(ctx->verifiers.begin(), ctx->verifiers.end(), v), ctx->verifiers.end());
  delete v;
}

int edc_verifier_queue(edc_verifier* v, size_t m, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                       const uint64_t* msg_off) {
  if (!v) return EDC_ERR_ARG;
  if (m && !msg_off) { v->ctx->err = "null msg_off"; return EDC_ERR_ARG; }
  return verifier_queue_host(v, m, vk, sig, msg, msg_off, nullptr);
}

int edc_verifier_queue_prehashed(edc_verifier* v, size_t m, const uint8_t* vk, const uint8_t* sig, const uint8_t* k) {
  if (!v) return EDC_ERR_ARG;
  if (m && !k) { v->ctx->err = "null k"; return EDC_ERR_ARG; }
  return verifier_queue_host(v, m, vk, sig, nullptr, nullptr, k);
}

int edc_verifier_queue_device(edc_verifier* v, size_t m, const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_msg,
                              const uint64_t* d_msg_off, const uint8_t* d_k) {
  if (!v) return EDC_ERR_ARG;
  edc_ctx* ctx = v->ctx;
  if (verifier_spent(v)) return EDC_ERR_ARG;
  if (!m) return 0;
  if (!d_vk || !d_sig || (!d_k && (!d_msg || !d_msg_off))) { ctx->err = "null input"; return EDC_ERR_ARG; }
  if (!aligned16(d_vk) || !aligned16(d_sig) || (d_k && !aligned16(d_k))) {
    ctx->err = "device vk / sig / k arrays must be 16-byte aligned";
    return EDC_ERR_ARG;
  }
  CK(hipSetDevice(ctx->device));
  if (v->cached.on) {
    // the caller's vk / sig (and k) are read in place: nothing is staged but the k of the message form
    int rc = verifier_cached_check(v, m);
    if (rc || (rc = verifier_stage_room(v, m))) return rc;
    const uint32_t* k = reinterpret_cast<const uint32_t*>(d_k);
    if (!k) {
      launch_challenge(v->s.st, (uint32_t)m, d_vk, d_sig, d_msg, d_msg_off, v->st_k);
      CK(hipGetLastError());
      k = v->st_k;
    }
    if ((rc = verifier_append_misses(v, m, d_vk, d_sig, k, true))) return rc;
    return verifier_fold(v);
  }
  int rc = verifier_reserve(v, v->n + m);
  if (rc) return rc;
  Slot& s = v->s;
  const size_t n0 = v->n;
  CK(hipMemcpyAsync(v->vk + n0 * 32, d_vk, m * 32, hipMemcpyDeviceToDevice, v->cs));
  CK(hipMemcpyAsync(v->sig + n0 * 64, d_sig, m * 64, hipMemcpyDeviceToDevice, v->cs));
  if (d_k) CK(hipMemcpyAsync(v->k + n0 * 8, d_k, m * 32, hipMemcpyDeviceToDevice, v->cs));
  CK(hipEventRecord(v->ev_copy, v->cs));
  CK(hipStreamWaitEvent(s.st, v->ev_copy, 0));
  if (!d_k) {
    // SHA-512 reads the caller's arena in place (offsets relative to d_msg, as the other _device entries)
    launch_challenge(s.st, (uint32_t)m, v->vk + n0 * 32, v->sig + n0 * 64, d_msg, d_msg_off, v->k + n0 * 8);
    CK(hipGetLastError());
    CK(hipEventRecord(v->ev_chal, s.st));
  }
  rc = verifier_enqueue_range(v, n0, m);
  if (rc) return rc;
  // the caller's device memory is not read after the call returns: the copies have run and, on
  // the message path, so has this range's SHA-512 pass (the decode and key work may still be queued)
  CK(hipEventSynchronize(v->ev_copy));
  if (!d_k) CK(hipEventSynchronize(v->ev_chal));
  v->n = n0 + m;
  return verifier_fold(v);
}

int edc_vfy_queue_indexed(edc_verifier* v, size_t m, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg,
                          const uint64_t* msg_off, const uint8_t* k) {
  if (!v) return EDC_ERR_ARG;
  edc_ctx* ctx = v->ctx;
  if (!k == !msg_off) { ctx->err = "exactly one of msg_off and k"; return EDC_ERR_ARG; }
  if (!ctx->kc_reg_m) { ctx->err = "no registered key list (edc_keycache_load)"; return EDC_ERR_ARG; }
  if (m && !key_idx) { ctx->err = "null key_idx"; return EDC_ERR_ARG; }
  return verifier_queue_host(v, m, nullptr, sig, msg, msg_off, k, key_idx);
}

int edc_vfy_queue_templated(edc_verifier* v, const edc_templates* ts, size_t m, const uint8_t* vk,
                            const uint32_t* key_idx, const uint8_t* sig, const uint16_t* tpl, const uint8_t* var,
                            const uint32_t* var_off) {
  if (!v) return EDC_ERR_ARG;
  edc_ctx* ctx = v->ctx;
  const TmplItems it{ts, tpl, var, var_off};
  TmplShape sh;
  if (key_idx && !ctx->kc_reg_m) { ctx->err = "no registered key list (edc_keycache_load)"; return EDC_ERR_ARG; }
  int rc = tmpl_check_host(ctx, m, vk, key_idx, sig, it, &sh);
  if (rc) return rc;
  return verifier_queue_host(v, m, vk, sig, nullptr, nullptr, nullptr, key_idx, &it, &sh);
}

int edc_vfy_last_split(const edc_verifier* v) { return v && v->last_split >= 0 ? v->last_split : EDC_ERR_ARG; }

int edc_vfy_last_plan(const edc_verifier* v, edc_plan_info* out) {
  if (!v || !out || !v->have_plan) return EDC_ERR_ARG;
  *out = v->last_plan;
  return 0;
}

size_t edc_verifier_size(const edc_verifier* v) { return v ? v->n : 0; }

int edc_verifier_verify(edc_verifier* v, const uint8_t z_seed[32], const uint8_t* z, uint8_t check8[32]) {
  if (!v) return EDC_ERR_ARG;
  return verifier_verify(v, z_seed, z, check8);
}

}  // extern "C"

// edc_verifier_verify_fallback (verdicts: n bytes, retained order); offered (nullable, cached mode):
// the same codes in offered order, hits EDC_OK
static int verifier_fallback(edc_verifier* v, const uint8_t* z_seed, uint8_t* verdicts, int* n_invalid,
                             uint8_t check8[32], uint8_t* offered) {
  edc_ctx* ctx = v->ctx;
  Slot& s = v->s;
  const size_t n = v->n;
  if (n_invalid) *n_invalid = 0;
  // eager mode: the eager verify first (its check8); a spent seed takes the plain verify with the
  // caller's fresh seed instead. Either leaves what the fallback reads: the key rows placed for
  // all n items, the per-item s bits, the grouping flags. The fallback draws its own z from z_seed.
  const bool eager = v->fold.eager && !v->fold.spent;
  int rc = eager ? verifier_verify(v, nullptr, nullptr, check8, false, false)
                 : verifier_verify(v, z_seed, nullptr, check8, true, false);
  if (rc <= 0) {
    if (rc == 0) {
      if (n) memset(verdicts, 0, n);
      if (offered) memset(offered, 0, (size_t)v->cached.offered);
      const int r1 = verifier_insert(v, nullptr);
      if (r1) return r1;
    }
    return rc;
  }
  bool per_sig;
  uint32_t m;
  int r2 = slot_grouping(ctx, s, &per_sig, &m);
  if (r2) return r2;
  // with too many distinct keys for per-(range, key) sums the fallback redoes the prefix with one
  // key term per signature on this slot (fallback_ranges says so), which overwrites the verifier's
  // grouped key state: it is rebuilt below
  bool redo = false;
  r2 = fallback_ranges(ctx, s, n, BatchIn{v->vk, v->sig, nullptr, nullptr, nullptr, z_seed, 0, nullptr, false}, per_sig, m,
                       verdicts, &redo);
  s.kin = v->k;
  if (redo) {
    CK(hipStreamSynchronize(s.st));
    int r3 = verifier_clear(v);
    if (!r3) r3 = verifier_enqueue_range(v, 0, n);
    if (r3) return r3;
  }
  if (r2 < 0) return r2;
  if (v->cached.on) {           // exactly the retained items whose code is EDC_OK become records
    const int r3 = verifier_codes_out(v, verdicts, offered);
    if (r3) return r3;
  }
  if (n_invalid) *n_invalid = r2;
  return EDC_INVALID_SIGNATURE;
}

extern "C" {

int edc_verifier_verify_fallback(edc_verifier* v, const uint8_t z_seed[32], uint8_t* verdicts, int* n_invalid,
                                 uint8_t check8[32]) {
  if (!v || !z_seed || (v->n && !verdicts)) return EDC_ERR_ARG;
  return verifier_fallback(v, z_seed, verdicts, n_invalid, check8, nullptr);
}

int edc_vfy_verify_fallback_offered(edc_verifier* v, const uint8_t z_seed[32], uint8_t* verdicts, int* n_invalid,
                                    uint8_t check8[32]) {
  if (!v) return EDC_ERR_ARG;
  if (!v->cached.on) return edc_verifier_verify_fallback(v, z_seed, verdicts, n_invalid, check8);
  if (!z_seed || (v->cached.offered && !verdicts)) return EDC_ERR_ARG;
  std::vector<uint8_t> retained(v->n ? v->n : 1);
  return verifier_fallback(v, z_seed, retained.data(), n_invalid, check8, verdicts);
}

int edc_verifier_reset(edc_verifier* v) {
  if (!v) return EDC_ERR_ARG;
  edc_ctx* ctx = v->ctx;
  CK(hipSetDevice(ctx->device));
  v->n = 0;
  fold_reset(v->fold);          // the next block commits its own seed (edc_vfy_begin_eager)
  cached_reset(v->cached);      // the counts and the insert watermark start over; the mode stays
  return verifier_clear(v);
}

int edc_vfy_set_cached(edc_verifier* v, int on) {
  if (!v) return EDC_ERR_ARG;
  if (!cached_can_switch(v->cached, v->n)) {
    v->ctx->err = "edc_vfy_set_cached: items are queued (call it after create or edc_verifier_reset)";
    return EDC_ERR_ARG;
  }
  edc_ctx* ctx = v->ctx;
  CK(hipSetDevice(ctx->device));
  // A passing verify may have left its insert running on the verifier's stream, reading the
  // retained arrays. A cached queue call only reaches those arrays through that stream; the plain
  // queue path writes them from the copy stream, which nothing orders behind the insert. So the
  // mode never changes under a pending insert: records are only ever made of bytes that verified.
  CK(hipStreamSynchronize(v->s.st));
  if (on && !v->origin) CK(v->origin.alloc(v->cap));   // one offered position per retained item
  v->cached.on = on != 0;
  return 0;
}

int edc_vfy_cached(const edc_verifier* v) { return v ? (v->cached.on ? 1 : 0) : EDC_ERR_ARG; }

int edc_vfy_cache_counts(const edc_verifier* v, uint64_t* offered, uint64_t* hits) {
  if (!v) return EDC_ERR_ARG;
  if (offered) *offered = v->cached.offered;
  if (hits) *hits = v->cached.hits;
  return 0;
}

int edc_vfy_begin_eager(edc_verifier* v, const uint8_t z_seed[32]) {
  if (!v) return EDC_ERR_ARG;
  edc_ctx* ctx = v->ctx;
  if (v->n) { ctx->err = "edc_vfy_begin_eager: items are queued (call it after create or edc_verifier_reset)"; return EDC_ERR_ARG; }
  uint8_t seed[32];
  if (z_seed) {
    memcpy(seed, z_seed, 32);
  } else {                      // OS randomness, or no eager mode at all: never a fixed seed
    size_t got = 0;
    while (got < sizeof(seed)) {
      const ssize_t r = getrandom(seed + got, sizeof(seed) - got, 0);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) { ctx->err = "edc_vfy_begin_eager: getrandom failed"; return EDC_ERR_HIP; }
      got += (size_t)r;
    }
  }
  CK(hipSetDevice(ctx->device));
  if (!v->run) CK(v->run.alloc(128));   // the running point, then a fold's 256-byte result block
  launch_point_accum(v->s.st, v->run, nullptr);
  CK(hipGetLastError());
  memcpy(v->eager_seed, seed, 32);
  fold_reset(v->fold);
  v->fold.eager = true;
  return 0;
}

int edc_vfy_set_fold(edc_verifier* v, size_t min_items) {
  if (!v) return EDC_ERR_ARG;
  v->fold.min_items = min_items;
  return 0;
}

int edc_vfy_folded(const edc_verifier* v, uint64_t* items, uint64_t* folds) {
  if (!v) return EDC_ERR_ARG;
  if (items) *items = v->fold.folded;
  if (folds) *folds = v->fold.folds;
  return 0;
}

int edc_vfy_eager(const edc_verifier* v) { return v ? (v->fold.eager ? 1 : 0) : EDC_ERR_ARG; }

}  // extern "C"

// ---------------------------------------------------------------- several GPUs, one process
// A consensus node calls Verifier::verify once per block (src/batch.rs:149-217). edc_multi
// splits that one batch over the contexts of several devices: contiguous shards, shard g's z
// drawn at its global queue indices (z_base = shard start), so every shard evaluates its part of
// the same batch equation; each device reduces its shard to one partial point (128 bytes), the
// partials are gathered through the host (they already come back with each shard's verdict) and
// summed on the first device, then x8 and the identity test. One host thread per device drives
// its shard; the same device may appear several times (several contexts on one GPU).
// One in-flight multi-device batch (edc_multi_submit): every shard's 256-byte result block reaches
// `blocks` on the first device, whose combine stream waits for every shard's event and sums the
// partial points there (k_combine_blocks). The host only enqueues, and waits once per batch. How a
// block travels depends on the pair (edc_multi.route, fixed at edc_create_multi):
//  - ROUTE_LOCAL: the shard runs on the first device itself (listed twice): a one-wave kernel on
//    the shard's stream copies it;
//  - ROUTE_PEER: peer access from the shard's device to the first device was enabled: the same
//    kernel stores it over xGMI;
//  - ROUTE_STAGED: no peer access (or forced by edc_multi_debug_force_staged): the shard's final
//    kernel already wrote the block to its slot's pinned host mirror; the combine stream waits for
//    the shard's event and copies that mirror to `blocks` itself. No kernel ever stores to another
//    device's memory without peer access enabled.
struct MultiSlot {
  bool pending = false;
  int64_t ticket = -1;
  bool want = false;
  std::vector<int64_t> shard;        // shard tickets, one per context
  // the owners below are emptied by multi_slot_free with the owning device current (the shards'
  // events each with their shard's device, the rest with the first device)
  std::vector<Event> copied;         // recorded on each shard's slot stream after its block copy
  Event done;                        // first device, after the combine
  DevBuf<uint8_t> blocks;            // first device: ndev x 256 bytes
  DevBuf<uint8_t> d_out;             // first device: 256-byte verdict block
  PinnedBuf<uint8_t> h_out;          // pinned mirror
};

enum { ROUTE_LOCAL = 0, ROUTE_PEER = 1, ROUTE_STAGED = 2 };

struct edc_multi {
  std::vector<edc_ctx*> ctx;
  std::vector<int> route;            // per shard: ROUTE_LOCAL / ROUTE_PEER / ROUTE_STAGED
  std::vector<int> route_auto;       // as found by edc_create_multi (edc_multi_debug_force_staged(0) restores it)
  std::string err;
  MultiSlot ms[kSlots];
  int ring = kSlots;                 // multi-batches in flight = the smallest shard context's slot count
  int64_t next_ticket = 0;
  Stream comb;                       // first device: every batch's combine, in submission order
                                     // (reset by edc_destroy_multi with that device current)
};

struct Shard {
  size_t lo = 0, hi = 0;
  int rc = 0, bad = 0;
  uint8_t partial[128] = {};
};

static void shard_bounds(size_t n, size_t g, std::vector<Shard>& sh) {
  sh.assign(g, Shard());
  for (size_t i = 0; i < g; ++i) {
    sh[i].lo = n * i / g;
    sh[i].hi = n * (i + 1) / g;
  }
}

template <typename F>
static void on_each_device(edc_multi* M, std::vector<Shard>& sh, F&& f) {
  std::vector<std::thread> th;
  for (size_t g = 1; g < sh.size(); ++g) th.emplace_back([&, g] { sh[g].rc = f(M->ctx[g], sh[g]); });
  sh[0].rc = f(M->ctx[0], sh[0]);
  for (auto& t : th) t.join();
}

// shard's part of the batch on its device: staged from the host, then the whole pipeline on
// slot 0 (so that a fallback can reuse its k, points and grouping), partial point + bad flag
static int shard_partial(edc_ctx* c, Shard& s, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t* z_seed) {
  if (hipSetDevice(c->device) != hipSuccess) return EDC_ERR_HIP;
  const size_t m = s.hi - s.lo;
  int rc = stage_host(c, m, vk + 32 * s.lo, sig + 64 * s.lo, msg, msg_off + s.lo);
  if (rc) return rc;
  rc = run_batch_sync(c, m, BatchIn{c->vk, c->sig, c->msg, c->off, nullptr, z_seed, s.lo, nullptr, false}, nullptr, s.partial,
                      &s.bad);
  return rc < 0 ? rc : 0;
}

static int multi_batch(edc_multi* M, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                       const uint64_t* msg_off, const uint8_t* z_seed, uint8_t check8[32], std::vector<Shard>& sh) {
  shard_bounds(n, M->ctx.size(), sh);
  on_each_device(M, sh, [&](edc_ctx* c, Shard& s) { return shard_partial(c, s, vk, sig, msg, msg_off, z_seed); });
  std::vector<uint8_t> parts(128 * sh.size());
  int bad = 0;
  for (size_t g = 0; g < sh.size(); ++g) {
    if (sh[g].rc < 0) {
      M->err = std::string("device ") + std::to_string(M->ctx[g]->device) + ": " + M->ctx[g]->err;
      return sh[g].rc;
    }
    memcpy(&parts[128 * g], sh[g].partial, 128);
    bad |= sh[g].bad;
  }
  edc_ctx* c0 = M->ctx[0];
  if (hipSetDevice(c0->device) != hipSuccess) return EDC_ERR_HIP;
  const int rc = combine_points(c0, sh.size(), parts.data(), bad, check8, nullptr);
  if (rc < 0) M->err = c0->err;
  return rc;
}

#define MCK(expr)                                                       \
  do {                                                                  \
    hipError_t e_ = (expr);                                             \
    if (e_ != hipSuccess) {                                             \
      (void)hipGetLastError();                                          \
      M->err = std::string(#expr) + ": " + hipGetErrorString(e_);       \
      return EDC_ERR_HIP;                                               \
    }                                                                   \
  } while (0)

static int multi_slot_init(edc_multi* M, MultiSlot& ms) {
  for (edc_ctx* c : M->ctx)
    if (c->nslots < M->ring) {   // edc_set_slots on a shard context after edc_create_multi
      M->err = "a shard context has fewer in-flight slots than the multi-device ring";
      return EDC_ERR_ARG;
    }
  if (ms.done) return 0;
  const size_t g = M->ctx.size();
  MCK(hipSetDevice(M->ctx[0]->device));
  // the combines are tiny and in order: one ordinary stream for all of them (the shard contexts'
  // slot streams already hold a hardware queue each)
  if (!M->comb) MCK(M->comb.create(hipStreamNonBlocking));
  MCK(ms.done.create(hipEventDisableTiming));
  MCK(ms.blocks.alloc(256 * g));
  MCK(ms.d_out.alloc(256));
  MCK(ms.h_out.alloc(256));
  ms.copied.clear();
  ms.copied.resize(g);
  for (size_t i = 0; i < g; ++i) {
    MCK(hipSetDevice(M->ctx[i]->device));
    MCK(ms.copied[i].create(hipEventDisableTiming));
  }
  return 0;
}

static void multi_slot_free(edc_multi* M, MultiSlot& ms) {
  if (!ms.done) return;
  (void)hipSetDevice(M->ctx[0]->device);
  (void)hipEventSynchronize(ms.done);
  for (size_t i = 0; i < ms.copied.size(); ++i) {
    (void)hipSetDevice(M->ctx[i]->device);
    ms.copied[i].reset();
  }
  (void)hipSetDevice(M->ctx[0]->device);
  ms = MultiSlot();
}

// After shard g's batch was enqueued on its context (ticket t): copy its result block to the first
// device behind the batch, on the shard's slot stream, and let the combine stream wait for it.
static int multi_link_shard(edc_multi* M, MultiSlot& ms, size_t g, int64_t t) {
  edc_ctx* c = M->ctx[g];
  Slot& s = c->slot[t % c->nslots];
  if (!s.pending || s.ticket != t || !s.d_out) { M->err = "shard ticket has no pending slot"; return EDC_ERR_ARG; }
  MCK(hipSetDevice(c->device));
  const int route = M->route[g];
  if (route != ROUTE_STAGED) {
    launch_copy_block(s.st, s.d_out, ms.blocks + 256 * g);   // hipMemcpyPeerAsync blocks the host here
    MCK(hipGetLastError());
  }
  MCK(hipEventRecord(ms.copied[g], s.st));
  MCK(hipSetDevice(M->ctx[0]->device));
  MCK(hipStreamWaitEvent(M->comb, ms.copied[g], 0));
  // staged: the shard's final kernel stored its block to the slot's pinned host mirror (the slot is
  // not reused before edc_multi_wait has synchronized this combine)
  if (route == ROUTE_STAGED) MCK(hipMemcpyAsync(ms.blocks + 256 * g, s.h_out, 256, hipMemcpyHostToDevice, M->comb));
  return 0;
}

// enqueue the combine of every shard's block on the first device; the batch is then in flight
static int multi_finish_submit(edc_multi* M, MultiSlot& ms, int64_t ticket, int want_check8) {
  MCK(hipSetDevice(M->ctx[0]->device));
  launch_combine_blocks(M->comb, (uint32_t)M->ctx.size(), ms.blocks, want_check8 != 0, ms.d_out);
  MCK(hipGetLastError());
  MCK(hipMemcpyAsync(ms.h_out, ms.d_out, 256, hipMemcpyDeviceToHost, M->comb));
  MCK(hipEventRecord(ms.done, M->comb));
  ms.pending = true;
  ms.ticket = ticket;
  ms.want = want_check8 != 0;
  M->next_ticket++;
  return ticket >= 0 ? 0 : EDC_ERR_ARG;
}

// shard g's submission failed after earlier shards were enqueued: drain those so that their
// contexts' tickets stay consistent, and report the failure
static int multi_abort(edc_multi* M, MultiSlot& ms, size_t failed, bool link_failed, int rc) {
  const std::string why = link_failed ? M->err : std::string(edc_last_error(M->ctx[failed]));
  for (size_t g = 0; g < ms.shard.size(); ++g)
    if (ms.shard[g] >= 0) (void)edc_batch_wait(M->ctx[g], ms.shard[g], nullptr, nullptr, nullptr);
  M->err = std::string("device ") + std::to_string(M->ctx[failed]->device) + ": " + why;
  return rc < 0 ? rc : EDC_ERR_ARG;
}

extern "C" {

edc_multi* edc_create_multi(const int* devices, int ndev) {
  if (!devices || ndev < 1 || ndev > 64) return nullptr;
  edc_multi* M = new edc_multi();
  for (int i = 0; i < ndev; ++i) {
    edc_ctx* c = edc_create(devices[i]);
    if (!c) {
      edc_destroy_multi(M);
      return nullptr;
    }
    M->ctx.push_back(c);
  }
  // contexts sharing one GPU split its kSlots (16) in-flight slots (one hardware queue each), so
  // that a rehearsal with a device listed several times does not oversubscribe the queue scheduler;
  // the multi-batch ring is the smallest share, so a multi submission never finds a shard's slot busy
  M->ring = kSlots;
  for (int i = 0; i < ndev; ++i) {
    int same = 0;
    for (int j = 0; j < ndev; ++j) same += devices[j] == devices[i];
    M->ctx[i]->nslots = kSlots / same > 0 ? kSlots / same : 1;
    if (M->ctx[i]->nslots < M->ring) M->ring = M->ctx[i]->nslots;
  }
  // how each shard's result block reaches the first device (edc_multi_submit): a peer store over
  // xGMI only where peer access from the shard's device to the first device is actually enabled;
  // any other outcome of the enable than success / already-enabled is an error
  M->route.assign(ndev, ROUTE_LOCAL);
  for (int i = 1; i < ndev; ++i) {
    if (devices[i] == devices[0]) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, devices[i], devices[0]) != hipSuccess || !can) {
      (void)hipGetLastError();
      M->route[i] = ROUTE_STAGED;
      continue;
    }
    const hipError_t e = hipSetDevice(devices[i]) == hipSuccess ? hipDeviceEnablePeerAccess(devices[0], 0)
                                                                 : hipErrorInvalidDevice;
    (void)hipGetLastError();
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
      edc_destroy_multi(M);
      return nullptr;
    }
    M->route[i] = ROUTE_PEER;
  }
  M->route_auto = M->route;
  return M;
}

int edc_multi_debug_force_staged(edc_multi* M, int on) {
  if (!M) return EDC_ERR_ARG;
  for (const MultiSlot& ms : M->ms)
    if (ms.pending) { M->err = "route change with a batch in flight"; return EDC_ERR_ARG; }
  for (size_t i = 0; i < M->ctx.size(); ++i) M->route[i] = on ? (int)ROUTE_STAGED : M->route_auto[i];
  return 0;
}

int edc_multi_route(const edc_multi* M, int i) {
  return (M && i >= 0 && i < (int)M->route.size()) ? M->route[i] : EDC_ERR_ARG;
}

void edc_destroy_multi(edc_multi* M) {
  if (!M) return;
  for (MultiSlot& ms : M->ms) multi_slot_free(M, ms);
  if (M->comb) {
    (void)hipSetDevice(M->ctx[0]->device);
    M->comb.reset();
  }
  for (edc_ctx* c : M->ctx) edc_destroy(c);
  delete M;
}

int64_t edc_multi_submit(edc_multi* M, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t z_seed[32], int want_check8) {
  if (!M || !z_seed || (n && (!vk || !sig || !msg_off))) return EDC_ERR_ARG;
  const int64_t ticket = M->next_ticket;
  MultiSlot& ms = M->ms[ticket % M->ring];
  if (ms.pending) { M->err = kAllSlotsInFlight; return EDC_ERR_ARG; }      // a MultiSlot: the claim's message, not its slot
  int rc = multi_slot_init(M, ms);
  if (rc) return rc;
  std::vector<Shard> sh;
  shard_bounds(n, M->ctx.size(), sh);
  ms.shard.assign(sh.size(), -1);
  for (size_t g = 0; g < sh.size(); ++g) {
    const size_t lo = sh[g].lo, m = sh[g].hi - lo;
    const int64_t t = edc_batch_submit(M->ctx[g], m, vk + 32 * lo, sig + 64 * lo, msg, msg_off + lo, z_seed, lo, 0);
    if (t < 0) return multi_abort(M, ms, g, false, (int)t);
    ms.shard[g] = t;
    rc = multi_link_shard(M, ms, g, t);
    if (rc) return multi_abort(M, ms, g, true, rc);
  }
  rc = multi_finish_submit(M, ms, ticket, want_check8);
  return rc ? rc : ticket;
}

int64_t edc_multi_submit_device(edc_multi* M, const size_t* n, const uint8_t* const* d_vk, const uint8_t* const* d_sig,
                                const uint8_t* const* d_msg, const uint64_t* const* d_msg_off,
                                const uint8_t z_seed[32], int want_check8) {
  if (!M || !z_seed || !n || !d_vk || !d_sig || !d_msg || !d_msg_off) return EDC_ERR_ARG;
  const int64_t ticket = M->next_ticket;
  MultiSlot& ms = M->ms[ticket % M->ring];
  if (ms.pending) { M->err = kAllSlotsInFlight; return EDC_ERR_ARG; }      // a MultiSlot: the claim's message, not its slot
  int rc = multi_slot_init(M, ms);
  if (rc) return rc;
  const size_t G = M->ctx.size();
  ms.shard.assign(G, -1);
  uint64_t base = 0;
  for (size_t g = 0; g < G; ++g) {
    const int64_t t = edc_batch_submit_device(M->ctx[g], n[g], d_vk[g], d_sig[g], d_msg[g], d_msg_off[g], z_seed,
                                              base, nullptr, 0);
    if (t < 0) return multi_abort(M, ms, g, false, (int)t);
    ms.shard[g] = t;
    rc = multi_link_shard(M, ms, g, t);
    if (rc) return multi_abort(M, ms, g, true, rc);
    base += n[g];
  }
  rc = multi_finish_submit(M, ms, ticket, want_check8);
  return rc ? rc : ticket;
}

int edc_multi_wait(edc_multi* M, int64_t ticket, uint8_t check8[32]) {
  if (!M || ticket < 0) return EDC_ERR_ARG;
  MultiSlot& ms = M->ms[ticket % M->ring];
  if (!ms.pending || ms.ticket != ticket) { M->err = "unknown or already-waited ticket"; return EDC_ERR_ARG; }
  ms.pending = false;
  int err = 0;
  for (size_t g = 0; g < ms.shard.size(); ++g) {   // retire the shard tickets (grouping statistics)
    const int r = edc_batch_wait(M->ctx[g], ms.shard[g], nullptr, nullptr, nullptr);
    if (r < 0 && !err) {
      err = r;
      M->err = std::string("device ") + std::to_string(M->ctx[g]->device) + ": " + edc_last_error(M->ctx[g]);
    }
  }
  MCK(hipSetDevice(M->ctx[0]->device));
  if (err) {   // the combine may still be running on M->comb: drain it before the slot can be reused
    (void)hipEventSynchronize(ms.done);
    (void)hipGetLastError();
    return err;
  }
  MCK(hipEventSynchronize(ms.done));
  const int verdict = reinterpret_cast<int*>(ms.h_out.get())[0];
  const int bad = reinterpret_cast<int*>(ms.h_out.get())[1];
  if (check8) {
    if (bad || !ms.want) memset(check8, 0, 32);
    else memcpy(check8, ms.h_out + 16, 32);
  }
  return verdict ? EDC_INVALID_SIGNATURE : EDC_OK;
}

int edc_multi_size(const edc_multi* M) { return M ? (int)M->ctx.size() : 0; }

edc_ctx* edc_multi_context(edc_multi* M, int i) {
  return (M && i >= 0 && i < (int)M->ctx.size()) ? M->ctx[i] : nullptr;
}

const char* edc_multi_last_error(const edc_multi* M) { return M ? M->err.c_str() : "null context"; }

int edc_multi_batch_verify(edc_multi* M, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                           const uint64_t* msg_off, const uint8_t z_seed[32], uint8_t check8[32]) {
  if (!M || !z_seed || (n && (!vk || !sig || !msg_off))) return EDC_ERR_ARG;
  std::vector<Shard> sh;
  return multi_batch(M, n, vk, sig, msg, msg_off, z_seed, check8, sh);
}

int edc_multi_batch_verify_fallback(edc_multi* M, size_t n, const uint8_t* vk, const uint8_t* sig,
                                    const uint8_t* msg, const uint64_t* msg_off, const uint8_t z_seed[32],
                                    uint8_t* verdicts, int* n_invalid, uint8_t check8[32]) {
  if (!M || !z_seed || (n && (!vk || !sig || !msg_off || !verdicts))) return EDC_ERR_ARG;
  if (n_invalid) *n_invalid = 0;
  std::vector<Shard> sh;
  const int rc = multi_batch(M, n, vk, sig, msg, msg_off, z_seed, check8, sh);
  if (rc <= 0) {
    if (rc == 0 && n) memset(verdicts, 0, n);
    return rc;
  }
  // every shard whose own partial fails (or that saw a decode / canonicity failure) localizes its
  // invalid items with the grouped fallback, reusing its batch state; the others are all valid
  on_each_device(M, sh, [&](edc_ctx* c, Shard& s) -> int {
    const size_t m = s.hi - s.lo;
    memset(verdicts + s.lo, 0, m);
    if (hipSetDevice(c->device) != hipSuccess) return EDC_ERR_HIP;
    const int ok = combine_points(c, 1, s.partial, s.bad, nullptr, nullptr);
    if (ok <= 0) return ok;
    Slot& sl = c->slot[0];
    bool per_sig;
    uint32_t keys;
    int r = slot_grouping(c, sl, &per_sig, &keys);
    if (r) return r;
    return fallback_ranges(c, sl, m, BatchIn{c->vk, c->sig, c->msg, c->off, nullptr, z_seed, s.lo, nullptr, false}, per_sig, keys,
                           verdicts + s.lo);
  });
  int total = 0;
  for (size_t g = 0; g < sh.size(); ++g) {
    if (sh[g].rc < 0) {
      M->err = std::string("device ") + std::to_string(M->ctx[g]->device) + ": " + M->ctx[g]->err;
      return sh[g].rc;
    }
    total += sh[g].rc;
  }
  if (n_invalid) *n_invalid = total;
  return EDC_INVALID_SIGNATURE;
}

}  // extern "C"
