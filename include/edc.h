/*
 * edc.h -- C ABI of the MI355X (gfx950) ed25519-consensus batch-verification engine.
 *
 * This is the drop-in boundary for ONE hot path of informalsystems/ed25519-consensus 2.1.0:
 * ZIP215 batch verification and its per-signature fallback. Every entry point below replaces a
 * named Rust API of the reference (file:line into the reference tree) and keeps its exact
 * semantics: non-canonical A/R encodings accepted, s must be < l, cofactored equation, batch
 * and single verification agree. A Rust shim binds these symbols.
 *
 * Conventions
 *  - Host buffers are borrowed for the duration of the call; all calls are synchronous.
 *  - Items are in QUEUE order. vk: n*32 bytes, sig: n*64 bytes (R || s), messages are one
 *    arena `msg` with n+1 offsets (message i = msg[msg_off[i] .. msg_off[i+1])).
 *  - Device-resident inputs (the *_device entries): vk / sig / k arrays 16-byte aligned; the
 *    message arena is read in whole aligned 16-byte chunks (the SHA-512 kernel stages each
 *    message through LDS by DMA), i.e. from the 16-byte boundary at or before a message's first
 *    byte to the one after its last byte; those bytes must be mapped (they are never used).
 *    Device allocations (hipMalloc, torch tensors) always satisfy both, as such chunks never cross
 *    a page; host buffers have no such rule (they are staged into the context's own buffers).
 *  - z_i = u128::from_le_bytes(ChaCha20Rng::from_seed(z_seed) keystream[16(z_base+i) ..]),
 *    i.e. gen_u128 (reference src/batch.rs:64-68) drawn in queue order. Batch verification is
 *    sound only when z is unpredictable to the signers: z_seed must come from a CSPRNG, fresh for
 *    every verification (the reference takes `impl RngCore + CryptoRng`). Fixed seeds are for
 *    reproducible tests and benchmarks only.
 *  - Return codes: EDC_OK / EDC_INVALID_SIGNATURE / EDC_MALFORMED_PUBLIC_KEY mirror
 *    ed25519_consensus::Error (reference src/error.rs:7-20); negative = runtime failure
 *    (never mapped to Ok by callers).
 *  - One context = one GPU = one HIP stream. A context must not be used from two threads at
 *    once; use one context per thread (or per GPU / process).
 */
#ifndef EDC_H
#define EDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDC_OK 0
#define EDC_INVALID_SIGNATURE 1      /* Error::InvalidSignature  (src/error.rs:17) */
#define EDC_MALFORMED_PUBLIC_KEY 2   /* Error::MalformedPublicKey (src/error.rs:14) */
#define EDC_ERR_HIP (-1)
#define EDC_ERR_ARG (-2)
#define EDC_ERR_NOMEM (-3)

typedef struct edc_ctx edc_ctx;

/* Number of visible GPUs (hipGetDeviceCount), or a negative error. */
int edc_device_count(void);

/* Create a context bound to one GPU (its own stream, constant tables, grow-only workspace). */
edc_ctx* edc_create(int device);
void edc_destroy(edc_ctx* ctx);
/* Text of the last runtime error on this context ("" if none). */
const char* edc_last_error(const edc_ctx* ctx);

/*
 * batch::Verifier::queue (x n) + Verifier::verify(rng)
 *   reference src/batch.rs:127-137 (queue: k = H(R||A||M), group by raw key bytes)
 *             src/batch.rs:149-217 (verify: decode, z, coalesced MSM, [8]check == 0)
 * Returns EDC_OK if the batch equation holds, EDC_INVALID_SIGNATURE otherwise (including any
 * undecodable A/R or non-canonical s, as the reference). check8 (nullable) receives the
 * compressed [8]*check point when the equation was evaluated (zeros when the batch was
 * rejected before the MSM).
 * Host-buffer synchronous calls (this one, edc_batch_verify_z, edc_batch_verify_prehashed) from
 * 2^16 items copy their inputs in chunks and start each chunk's work as it lands; for the call's
 * duration the engine runs two helper threads of its own on ctx (joined before it returns), so
 * the one-context-per-thread rule below is unchanged. Results equal the one-piece path's.
 */
int edc_batch_verify(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                     const uint8_t* msg, const uint64_t* msg_off, const uint8_t z_seed[32],
                     uint8_t check8[32]);

/* Same, with caller-drawn z (n*16 bytes, LE u128 per item) for RNGs other than ChaCha20. Any z is
 * accepted, here and through the d_z arguments below: how full the MSM's bins and buckets are is
 * then whatever the caller makes it (every item in one bucket, empty windows, z = 0), and results
 * do not depend on it (tests/test_gpu_bucket_shapes.py). */
int edc_batch_verify_z(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                       const uint8_t* msg, const uint64_t* msg_off, const uint8_t* z,
                       uint8_t check8[32]);

/*
 * Device-resident variant (inputs already in this GPU's HBM, e.g. torch tensors). d_z may be
 * NULL (then z comes from z_seed at global indices z_base + i).
 */
int edc_batch_verify_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                            const uint8_t* d_msg, const uint64_t* d_msg_off,
                            const uint8_t z_seed[32], uint64_t z_base, const uint8_t* d_z,
                            uint8_t check8[32]);

/*
 * Asynchronous form of edc_batch_verify_device for streams of batches (a consensus node
 * verifying block after block): edc_batch_submit_device enqueues the whole pipeline on one of the
 * context's in-flight slots (16) and returns a ticket >= 0 (or <0); edc_batch_wait blocks for that
 * ticket and returns its verdict (EDC_OK / EDC_INVALID_SIGNATURE, <0 on runtime failure), with
 * optional check8 (needs want_check8), partial point and bad flag. Tickets must be waited in
 * submission order before their slot is reused; inputs must stay valid until the wait.
 * Whenever *bad is set (an undecodable R or key, or s >= l in the batch) the partial is the
 * IDENTITY, not the shard's check point: a caller combining partials must OR the bad flags and
 * treat a set flag as a rejection (edc_combine_partials' bad_any), never test [8]*partial alone.
 */
int64_t edc_batch_submit_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                const uint8_t* d_msg, const uint64_t* d_msg_off,
                                const uint8_t z_seed[32], uint64_t z_base, const uint8_t* d_z,
                                int want_check8);
int edc_batch_wait(edc_ctx* ctx, int64_t ticket, uint8_t check8[32], uint8_t partial[128], int* bad);

/*
 * Several consecutive batches in ONE launch sequence (a node verifying several blocks' votes at
 * once, or one GPU's shards of consecutive blocks; reference src/batch.rs:149-217 once per batch):
 * nb (1..16) batches of n_per items each (n_per a multiple of 2048), back to back in device
 * memory -- batch b is items [b n_per, (b+1) n_per) of d_vk / d_sig and of the message arena's
 * nb n_per + 1 offsets (or of d_k: nb n_per prehashed challenges, messages unused, d_msg /
 * d_msg_off may be NULL). Batch b's z are drawn at global indices z_base + b n_per + i, so batch
 * by batch its verdict, bad flag, check8 and partial equal edc_batch_verify_device /
 * edc_batch_partial_device of batch b alone at z_base + b n_per (see "Union first" below). Every per-item kernel runs once over all nb n_per items
 * and the MSM is range-tagged (one range per batch), so small batches fill the GPU like one
 * large batch. Waited with edc_batch_wait_multi (same ticket rules as edc_batch_submit_device):
 * verdicts[b] (EDC_OK / EDC_INVALID_SIGNATURE), optional check8 (nb x 32; a launch run batch by
 * batch from the start, edc_set_multi_union(ctx, 0), computes it only with want_check8),
 * partials (nb x 128) and bad flags (nb); returns EDC_INVALID_SIGNATURE if any batch failed.
 *
 * Union first (default; edc_set_multi_union): the launch runs as ONE batch over all nb n_per items
 * (same z). Its equation is the sum of the batches' equations, so when it holds every batch holds
 * -- with the probability batch verification itself gives, as Verifier::verify accepting a batch
 * accepts each of its items -- and every batch reports EDC_OK, bad 0 and the identity as check8.
 * When it fails (or partials are asked for at the wait), the wait reruns the launch batch by batch
 * as above before returning, so failing batches get exactly their own verdict, bad flag and
 * check8. edc_set_multi_union(ctx, 0) always runs batch by batch; edc_multi_union_stats counts the
 * union launches that passed and those rerun.
 */
int64_t edc_batch_submit_multi_device(edc_ctx* ctx, size_t nb, size_t n_per, const uint8_t* d_vk, const uint8_t* d_sig,
                                      const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                      const uint8_t z_seed[32], uint64_t z_base, int want_check8);
int edc_batch_wait_multi(edc_ctx* ctx, int64_t ticket, size_t nb, int* verdicts, uint8_t* check8, uint8_t* partials,
                         int* bad);
int edc_set_multi_union(edc_ctx* ctx, int on);
int edc_multi_union_stats(const edc_ctx* ctx, uint64_t* passed, uint64_t* rerun);

/*
 * Host-buffer form of edc_batch_submit_device (replaces src/batch.rs:149 `Verifier::verify` for a
 * caller streaming consecutive batches from host memory): the inputs are copied into the slot's
 * own device buffers on the slot's stream, so the PCIe transfer of this batch overlaps the kernels
 * of the batches already in flight. Host buffers are borrowed until edc_batch_wait(ticket)
 * returns. Waited with edc_batch_wait; same ticket rules.
 */
int64_t edc_batch_submit(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t z_seed[32], uint64_t z_base, int want_check8);

/*
 * edc_batch_submit for a node whose votes come from its registered validator set: item i's key
 * is key_idx[i], a position in the list last given to edc_keycache_load (4 bytes over PCIe per
 * item instead of 32). The device expands the indices to the raw 32-byte keys, so verdicts and
 * [8]*check equal edc_batch_submit with those keys. An index outside the list -> EDC_ERR_ARG.
 */
int64_t edc_batch_submit_indexed(edc_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sig,
                                 const uint8_t* msg, const uint64_t* msg_off, const uint8_t z_seed[32],
                                 uint64_t z_base, int want_check8);

/*
 * Multi-GPU shard: evaluate this shard's part of the batch equation WITHOUT the cofactor /
 * identity step. partial (128 bytes) = canonical X||Y||Z||T of the shard's check point;
 * *bad = 1 if any item of the shard failed decoding / canonicity, and then the partial is the
 * IDENTITY (deterministic whatever the addition order; the off-curve sum is not): callers must
 * check *bad and pass the OR of the shards' flags to edc_combine_partials, whose verdict is then a
 * rejection. Items are the shard's slice of the global queue starting at global index z_base
 * (device pointers).
 */
int edc_batch_partial_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                             const uint8_t* d_msg, const uint64_t* d_msg_off,
                             const uint8_t z_seed[32], uint64_t z_base, const uint8_t* d_z,
                             uint8_t partial[128], int* bad);

/*
 * Combine g shard partials (g*128 bytes, any order) and the OR of their bad flags into the
 * batch verdict (src/batch.rs:212-216). check8 nullable.
 */
int edc_combine_partials(edc_ctx* ctx, size_t g, const uint8_t* partials, int bad_any,
                         uint8_t check8[32]);

/*
 * Device-side combine of g gathered exchange records (the multi-rank path's all-gather output,
 * already in this GPU's memory): record r at d_records + r*stride holds a shard's canonical
 * 128-byte partial point followed by its bad byte. The sum, x8 and the identity test (reference
 * src/batch.rs:212-216) run as one small kernel ENQUEUED on the caller's HIP stream `stream`
 * (the stream the all-gather ran on, so no host round trip and no synchronization; it must belong
 * to ctx's device, else EDC_ERR_ARG; the calling thread's current device is left unchanged); the 256-byte
 * result block lands in d_out (device, 16-byte aligned): int[0] = 0 Ok / 1 reject, int[1] = bad.
 */
int edc_combine_records_device(edc_ctx* ctx, void* stream, size_t g, const uint8_t* d_records, size_t stride,
                               uint8_t* d_out);

/*
 * VerificationKey::try_from(vk) + VerificationKey::verify(sig, msg) for each item
 *   reference src/verification_key.rs:160-175 (try_from -> MalformedPublicKey)
 *             src/verification_key.rs:225-258 (verify / verify_prehashed)
 * verdicts[i] in {EDC_OK, EDC_INVALID_SIGNATURE, EDC_MALFORMED_PUBLIC_KEY}. Returns 0 or <0.
 */
int edc_verify_each(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                    const uint8_t* msg, const uint64_t* msg_off, uint8_t* verdicts);

/* Device-resident edc_verify_each: verdicts into d_verdicts (n bytes of this GPU's memory). */
int edc_verify_each_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                           const uint8_t* d_msg, const uint64_t* d_msg_off, uint8_t* d_verdicts);

/*
 * Grouped fallback after a failed batch (the caller-driven Item::verify_single loop of
 * reference tests/batch.rs:37-43, src/batch.rs:104-107). The batch equation is linear, so it
 * restricts to any subset of the items: ONE range-tagged MSM pass evaluates it over about 128
 * contiguous ranges by default (edc_set_fallback_shape; same z, same k, the decoded points of the
 * batch prefix); ranges whose
 * [8]*check is not the identity, or that hold an item with an undecodable R / key or a
 * non-canonical s, are verified item by item. verdicts (host, n bytes) receive
 * Item::verify_single's code for every item. Returns the number of invalid items, or <0.
 * `leaf` is ignored (kept for ABI compatibility): range sizes are chosen by the library.
 *
 * Soundness: an item of a passing range is reported valid because its range's batch equation
 * holds, exactly as Verifier::verify accepts a batch (ZIP215: batch == single). Like the
 * reference's batch verification this is probabilistic: it relies on z being unpredictable to
 * whoever made the signatures. z_seed MUST be fresh and secret for every call (e.g. 32 bytes
 * of OS randomness); a known or reused seed lets crafted invalid signatures cancel inside a
 * range and be reported valid.
 */
int edc_find_invalid_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                            const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                            size_t leaf, uint8_t* verdicts);

/*
 * Verifier::verify(rng) and, if it fails, the per-item fallback in one call (the flow of
 * reference tests/batch.rs:18-44): the batch runs once; on failure the grouped fallback above
 * reuses that batch's k, points and grouping instead of recomputing them. Returns EDC_OK
 * (verdicts all 0) or EDC_INVALID_SIGNATURE with verdicts[i] = Item::verify_single's code and
 * *n_invalid (nullable) their count; <0 on runtime failure. check8 (nullable) as
 * edc_batch_verify. Same z_seed requirement as edc_find_invalid_device.
 */
int edc_batch_verify_fallback_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                     const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t z_seed[32],
                                     uint8_t* verdicts, int* n_invalid, uint8_t check8[32]);

/*
 * Prehashed batches: the reference's batch::Item is {vk_bytes, sig, k} (src/batch.rs:76-80) --
 * k = H(R||A||M) mod l is computed once, at Item::from (src/batch.rs:82-94), and
 * Verifier::queue / verify (src/batch.rs:127-137, :149-217) never see the message again. These
 * entries take that k (n*32 bytes, queue order, canonical little-endian scalars < l, as
 * Scalar::from_hash returns) instead of the message arena: SHA-512 is skipped and only
 * 32 + 64 + 32 bytes per item are read. Everything downstream is the message path's pipeline, so
 * verdicts and check8 are bit-identical to edc_batch_verify on the messages those k came from.
 * A k >= l is a broken caller contract: the call returns EDC_ERR_ARG (never a verdict).
 *  - edc_batch_verify_prehashed: host buffers, synchronous; z from z_seed (ChaCha20, as
 *    edc_batch_verify) or, when z_seed is NULL, caller-drawn z (n*16 bytes, LE u128 per item).
 *  - edc_batch_verify_prehashed_device: device buffers; z as edc_batch_verify_device.
 *  - edc_batch_submit_prehashed / _device: asynchronous forms (edc_batch_submit /
 *    edc_batch_submit_device rules; waited with edc_batch_wait). Inputs are borrowed until the wait.
 *  - edc_batch_verify_prehashed_fallback[_device]: the batch and, if it fails, the grouped fallback
 *    of edc_batch_verify_fallback_device (verdicts[i] = Item::verify_single's code, src/batch.rs:104-107).
 * Device k / z arrays must be 16-byte aligned (EDC_ERR_ARG otherwise).
 */
int edc_batch_verify_prehashed(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* k,
                               const uint8_t z_seed[32], const uint8_t* z, uint8_t check8[32]);
int edc_batch_verify_prehashed_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                      const uint8_t* d_k, const uint8_t z_seed[32], uint64_t z_base,
                                      const uint8_t* d_z, uint8_t check8[32]);
int64_t edc_batch_submit_prehashed(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* k,
                                   const uint8_t z_seed[32], uint64_t z_base, int want_check8);
int64_t edc_batch_submit_prehashed_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                          const uint8_t* d_k, const uint8_t z_seed[32], uint64_t z_base,
                                          const uint8_t* d_z, int want_check8);
/*
 * edc_batch_submit_prehashed with the keys given as positions in the list last given to
 * edc_keycache_load (as edc_batch_submit_indexed): 4 + 64 + 32 = 100 bytes per item over PCIe, for
 * a node whose votes come from its registered validator set. Verdicts and check8 equal
 * edc_batch_submit_prehashed with those keys. An index outside the list -> EDC_ERR_ARG.
 */
int64_t edc_batch_submit_prehashed_indexed(edc_ctx* ctx, size_t n, const uint32_t* key_idx, const uint8_t* sig,
                                           const uint8_t* k, const uint8_t z_seed[32], uint64_t z_base,
                                           int want_check8);
int edc_batch_verify_prehashed_fallback(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                                        const uint8_t* k, const uint8_t z_seed[32], uint8_t* verdicts,
                                        int* n_invalid, uint8_t check8[32]);
int edc_batch_verify_prehashed_fallback_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                               const uint8_t* d_k, const uint8_t z_seed[32], uint8_t* verdicts,
                                               int* n_invalid, uint8_t check8[32]);

/*
 * batch::Item::verify_single (reference src/batch.rs:104-107): as edc_verify_each but with the
 * queue-time challenge k (n*32 bytes, canonical scalars) instead of the message. Any k >= l
 * (which Scalar::from_hash never returns) makes the call EDC_ERR_ARG, checked on the host before
 * anything is launched.
 */
int edc_verify_prehashed_each(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                              const uint8_t* k, uint8_t* verdicts);

/*
 * impl From<(VerificationKeyBytes, Signature, &M)> for batch::Item (reference src/batch.rs:82-94):
 * k_i = Scalar::from_hash(Sha512(R_i || A_i || M_i)) as 32 canonical LE bytes per item.
 */
int edc_challenge(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig,
                  const uint8_t* msg, const uint64_t* msg_off, uint8_t* k_out);

/*
 * CompressedEdwardsY::decompress as used by VerificationKey::try_from
 * (reference src/verification_key.rs:166-168): ok[i] = 1 and xy[i] = canonical x || y, or
 * ok[i] = 0 when the encoding is not a curve point. Returns 0 or <0.
 */
int edc_decompress(edc_ctx* ctx, size_t n, const uint8_t* enc, uint8_t* xy, uint8_t* ok);

/*
 * VerificationKey::try_from(VerificationKeyBytes) for n keys at once -- key ingestion, e.g. a
 * validator set or serde-deserialized keys (reference src/verification_key.rs:160-175, :106-109;
 * tests/unit_tests.rs:32-40). codes[i] = EDC_OK or EDC_MALFORMED_PUBLIC_KEY. Returns 0 or <0.
 */
int edc_vk_validate(edc_ctx* ctx, size_t n, const uint8_t* vk, uint8_t* codes);

/*
 * Persistent validator-key cache: the reference's VerificationKey keeps its decoded point
 * (src/verification_key.rs:106-114, :160-175) while batch::Verifier re-decodes every distinct
 * key per verify (src/batch.rs:183-185). edc_keycache_load decodes the m keys (n*32 bytes,
 * duplicates allowed) ONCE and keeps a 64 KB fixed-base table per distinct key in this
 * context, replacing any previous cache. Every later batch / per-item call on the context
 * takes A and [2^128]A of a registered key from the cache, and the per-item fallback computes
 * [s]B - [k]A for it without doublings. Verdicts are identical with and without the cache
 * (an undecodable registered key stays MalformedPublicKey / fails the batch). ok (nullable,
 * m bytes) receives 1 where the key decodes. Returns the number of distinct keys cached
 * (<= 65536) or <0; refused while submitted batches are in flight.
 */
int64_t edc_keycache_load(edc_ctx* ctx, size_t m, const uint8_t* vk, uint8_t* ok);
int edc_keycache_clear(edc_ctx* ctx);
size_t edc_keycache_size(const edc_ctx* ctx);

/*
 * Per-object decoded key (reference src/verification_key.rs:106-114, :160-175: VerificationKey
 * decodes A once at try_from and keeps minus_A for every later verify): adds the keys of vk (m x 32
 * bytes) that are not cached yet to this context's cache WITHOUT replacing it. Cached keys keep
 * their places, so the list last given to edc_keycache_load stays valid for
 * edc_batch_submit_indexed (this call does not change that list). Every later batch or per-item
 * call finds a key added here exactly as one loaded by edc_keycache_load. ok (nullable, m bytes)
 * as edc_keycache_load. The table's hash is keyed by a per-context secret, so keys taken from
 * untrusted input cannot be chosen to collide. Keys that do not decode (try_from's
 * MalformedPublicKey) are NOT added (ok = 0 for them), so untrusted malformed keys cannot pin comb
 * tables. Returns the number of distinct keys now cached or <0; refused while submitted batches
 * are in flight.
 */
int64_t edc_keycache_add(edc_ctx* ctx, size_t m, const uint8_t* vk, uint8_t* ok);

/*
 * SigningKey::from([u8;32]) + SigningKey::sign (reference src/signing_key.rs:118-150,
 * :186-205) -- test/benchmark data source. seed_index (nullable) maps item i to seed
 * seed_index[i] (shared validator keys); vk_out n*32, sig_out n*64.
 */
int edc_sign(edc_ctx* ctx, size_t n, const uint8_t* seeds, size_t nseeds, const uint32_t* seed_index,
             const uint8_t* msg, const uint64_t* msg_off, uint8_t* vk_out, uint8_t* sig_out);
/* Device-pointer variant of edc_sign (all pointers in this GPU's memory). */
int edc_sign_device(edc_ctx* ctx, size_t n, const uint8_t* d_seeds, const uint32_t* d_seed_index,
                    const uint8_t* d_msg, const uint64_t* d_msg_off, uint8_t* d_vk_out,
                    uint8_t* d_sig_out);

/* ChaCha20 keystream blocks [blk0, blk0+nblocks) of key into d_out (64 bytes each), on device. */
int edc_chacha_fill_device(edc_ctx* ctx, const uint8_t key[32], uint64_t blk0, uint64_t nblocks,
                           uint8_t* d_out);

/*
 * Key grouping policy. The reference coalesces signatures by raw key bytes (HashMap,
 * src/batch.rs:114-137) so each distinct key is one MSM term; this only saves work when keys
 * repeat. mode 0 (default, auto): group, unless the last grouped batch on this context had more
 * distinct keys than half its signatures, in which case the next batches (regrouping every 8th)
 * keep one A_i term per signature with coefficient z_i k_i. mode 1: always group. mode 2: never.
 * mode 3 (tests): group, but with a zero probe budget, so every batch takes the on-device
 * overflow path that an adversarial key set would trigger (grouping abandoned mid-batch, one key
 * term per signature). Grouping hashes the raw key bytes under a per-context secret from OS
 * randomness and caps its probes, so chosen keys cannot make it quadratic.
 * Every mode gives the same group element, hence identical verdicts and [8]*check.
 */
int edc_set_key_grouping(edc_ctx* ctx, int mode);

/*
 * Split coefficients with the validator-key cache (edc_keycache_load). While the last batch found
 * every key in the cache, mode 0 (default, auto) writes each 253-bit B / key coefficient as
 * lo + 2^128 hi with hi on the cached [2^128]A (and [2^128]B), so every MSM term is 128 bits and
 * the final Horner chain is ~128 doublings instead of ~250 (lower per-batch latency). A key
 * missing from the cache still verifies exactly (it is doubled on the device) and turns the split
 * off until a batch finds all its keys again. mode 1: never split. Same group element in every
 * mode: identical verdicts and [8]*check. Replaces nothing in the reference (an MSM evaluation
 * order, src/batch.rs:205-210).
 */
int edc_set_key_split(edc_ctx* ctx, int mode);

/*
 * Pippenger shape for this context's batches (tuning / measurement): window width `bits` (8..16)
 * and number of parts a batch's terms are split into (1..64; parts are summed per window). 0 for
 * either picks it from the batch size (default). Results never depend on it.
 */
int edc_set_msm_shape(edc_ctx* ctx, int bits, int parts);

/*
 * Target MSM entries per bin (tuning / measurement; >= 256, 0 = from the batch size, default):
 * with automatic parts, the slices of the densest windows are split into sub-bins of about this
 * many digits each, one workgroup per bin. Results never depend on it
 * (tests/test_gpu_subbins.py).
 */
int edc_set_msm_bin_entries(edc_ctx* ctx, int entries);

/*
 * Test knob (process-wide): at most `max_entries` (0..16384, default 16384) MSM entries per
 * workgroup go through the binning scatter's LDS stage; workgroups with more store each entry
 * directly. 0 forces the direct stores everywhere. Results never depend on it.
 */
int edc_debug_set_scatter_stage(uint32_t max_entries);

/*
 * Test hook: the device's wide scalar reduction (Scalar::from_hash after SHA-512, reference
 * src/batch.rs:86-91) on n caller-chosen 64-byte little-endian integers d_in (device, 16-byte
 * aligned) -> n canonical 32-byte residues mod l in d_out (device, 16-byte aligned), synchronous.
 * Lets tests drive the reduction's fold boundaries, which SHA-512 outputs practically never hit.
 */
int edc_debug_sc_reduce_wide(edc_ctx* ctx, size_t n, const uint8_t* d_in, uint8_t* d_out);

/*
 * Test hook (process-wide): out[0] = live device allocations, out[1] = live pinned host
 * allocations made by this library's contexts, verifiers and multi-device objects. Lets a test
 * assert that create / run / destroy leaked nothing on a device other processes allocate on.
 */
int edc_debug_live_allocs(uint64_t out[2]);

/*
 * Test hook: the Pippenger plan of the last batch on this context, as the host chose it (a copy
 * made where the plan is chosen: no device work, no synchronization). Lets a test assert which
 * plan its batch ran instead of inferring it from the shape: window widths, slices and sub-bins
 * per window, the bin count, and what the choice was made from. Replaces nothing in the reference
 * (an MSM evaluation order, src/batch.rs:205-210).
 *   nwin, nwin_short   windows in all / over the 128 bits of a z_i (the first nwin_short)
 *   nranges            ranges of a multi-batch launch, or parts of one batch (sum_ranges = 1)
 *   bins_per_range     sum over the windows of nslice[w] * nsub[w]
 *   bits / nslice / nsub [w < nwin]   width, 256-bucket slices and sub-bins per slice of window w
 *   target             entries per bin the split finally aimed at (edc_set_msm_bin_entries or the
 *                      size-chosen default, doubled until the plan fits the MSM's 8192 bins);
 *                      0 with explicit parts (edc_set_msm_shape), which are not split
 *   per_sig, split, few   the inputs of the choice: one key term per signature, split
 *                      coefficients, 8-bit high windows for few distinct keys
 *   fold               1: the plan of an eager verifier's fold (R terms only)
 * EDC_ERR_ARG before any plan was made on the context and for NULL.
 */
typedef struct edc_plan_info {
  uint32_t nwin, nwin_short, nranges, sum_ranges, bins_per_range;
  uint32_t per_sig, split, few, fold;
  uint32_t reserved;
  double target;
  uint8_t bits[32], nsub[32];
  uint16_t nslice[32];
} edc_plan_info;
int edc_debug_last_plan(const edc_ctx* ctx, edc_plan_info* out);

/*
 * Shape of the grouped fallback's range MSM (tuning / measurement): about `ranges` contiguous
 * ranges (1..1024, default 32) with `bits`-bit windows (8..13, default 10). The range count is
 * capped so that ranges x bins per range stays within the MSM's 8192 bins (e.g. at most 24 ranges
 * with 13-bit windows). Results never depend on it.
 */
int edc_set_fallback_shape(edc_ctx* ctx, int ranges, int bits);

/*
 * Number of in-flight slots (1..16, default 16) this context's submissions rotate over; each slot
 * holds its own workspace and hardware queue. Contexts that share one GPU (edc_create_multi with
 * a repeated device) get 16 / (contexts on that GPU). Refused while batches are in flight.
 */
int edc_set_slots(edc_ctx* ctx, int k);

/*
 * Pre-allocate the workspaces of every in-flight slot for batches of up to n items (otherwise
 * they grow on first use). Not a reference API: a setup call for streaming callers.
 */
int edc_reserve(edc_ctx* ctx, size_t n);

/*
 * Per-phase device timings of the last batch call (HIP events on the context stream), enabled
 * by edc_set_timing(ctx, 1). Returns the number of phases written (<= cap); names via
 * edc_timing_name(i).
 */
void edc_set_timing(edc_ctx* ctx, int enable);
int edc_last_timings(const edc_ctx* ctx, float* ms, int cap);
const char* edc_timing_name(int i);
/* The last timed batch's accumulation kernel alone (k_msm_accum_dma, between HIP events on its
 * stream): duration in ms and the number of digit entries it added (one signed mixed addition
 * each), for the accumulation's own roofline in bench.py. EDC_ERR_ARG before any timed batch. */
int edc_last_msm_accum(const edc_ctx* ctx, float* ms, uint64_t* entries);

/* Synchronize the context stream (for callers that time around device calls). */
int edc_synchronize(edc_ctx* ctx);

/*
 * Incremental batch verifier: batch::Verifier as an object (reference src/batch.rs:110-217). The
 * reference does the per-item work when an item is queued (Item::from hashes, src/batch.rs:82-94;
 * Verifier::queue groups by key bytes, :127-137) and Verifier::verify(rng) gets its RNG only at the
 * end, where it evaluates the equation (:149-217). A node that receives a block's votes over a whole
 * round queues them as they arrive and pays only the z-dependent part once the last one is in.
 *
 * edc_verifier_create  Verifier::default() (src/batch.rs:110-124), bound to ctx: its own workspace
 *   and streams (never the context's slot 0, so every other call on ctx keeps working between
 *   queue calls; the one-context-per-thread rule covers the context's verifiers too). Arrays and
 *   the key table are sized for capacity_hint items (0: grow on demand); queueing past the
 *   capacity grows the verifier, which never changes a result. Destroy every verifier before its
 *   context. NULL on failure.
 * edc_verifier_queue / _prehashed / _device  Verifier::queue x m (src/batch.rs:127-137) with
 *   Item::from (:82-94): m >= 0 items appended in queue order, from host buffers with their
 *   messages, from host buffers with the caller's k (canonical scalars, as the other prehashed
 *   entries), or from this GPU's memory (d_k nullable; when given the messages are not read;
 *   vk / sig / k 16-byte aligned and the arena mapped in whole 16-byte chunks, as the other _device
 *   entries). Each call enqueues, for the appended range only, the copies, SHA-512 -> k, the ZIP215
 *   decode of R, the key find-or-insert and the decode of keys first seen in the range, and may
 *   return before that work has run; the caller's memory is not read after the call returns. The
 *   verifier keeps vk, sig and k; messages are dead once their k exists. The forms may be mixed.
 *   Returns 0 or <0.
 * edc_verifier_size    Verifier::batch_size.
 * edc_verifier_verify  Verifier::verify(rng) (src/batch.rs:149-217): exactly one of z_seed (z as in
 *   edc_batch_verify) and z (n * 16 bytes drawn by the caller, z_i for queue index i). Runs only
 *   what depends on z -- coefficients and the MSM -- over everything queued. Return codes and
 *   check8 as edc_batch_verify, bit-identical to it on the same items and z; nothing queued is
 *   EDC_OK. A prehashed k >= l makes it return EDC_ERR_ARG. The queue survives the call: more
 *   items may be queued, and a later verify covers everything queued (draw fresh z for it).
 * edc_verifier_verify_fallback  verify and, if it fails, the grouped fallback on the retained k,
 *   points and grouping (the flow of reference tests/batch.rs:18-44): semantics, and the z_seed
 *   warning, of edc_batch_verify_fallback_device. verdicts: n bytes.
 * edc_verifier_reset   forget the items, keep the allocations (Verifier::default() for the next block).
 * edc_set_key_grouping modes 2 and 3 make a verifier take one key term per signature (the path a
 * probe overflow takes: every A_i is decoded at verify).
 *
 * With a registered validator set (edc_keycache_load / _add):
 * Split coefficients. While the context holds a key cache, every queue call also leaves the
 *   [2^128] multiple of each key first seen in it: a copy of the cached record, or 128 doublings
 *   at queue time for a key missing from the cache. verify then plans with split coefficients
 *   (every MSM term at most 128 bits, about 128 Horner doublings instead of about 250) when
 *   edc_set_key_split is 0, a cache is loaded, and every item queued since the last reset was
 *   queued against that same cache. Unlike the one-call entries the verifier does not stop
 *   splitting after uncached keys: their doublings are done before verify is called. In every
 *   key-grouping mode; after a grouping overflow verify takes the per-signature split path.
 *   edc_keycache_load / _add / _clear may run while items are queued: a call that changes the
 *   cache's contents starts a new cache generation (an _add that finds every key already cached
 *   changes nothing), and a verify that finds another generation than the one its rows were built
 *   against, or an item queued with no cache loaded, runs unsplit. Growth and edc_verifier_reset
 *   rebuild / restart against the cache loaded then. Verdict, check8 and fallback codes are
 *   bit-identical either way. The key rows live in the verifier's own allocation: 256 bytes per
 *   item of capacity.
 * edc_vfy_queue_indexed  edc_verifier_queue / _prehashed with the keys given as positions in the
 *   list last passed to edc_keycache_load (4 bytes per item over PCIe instead of 32; the raw key
 *   bytes are expanded into the retained vk range on the device, and the range then takes the
 *   same path as any other). Exactly one of msg_off (with msg) and k. An index outside the list,
 *   or no registered list, is EDC_ERR_ARG with nothing appended. May be mixed with the other
 *   queue forms.
 * edc_vfy_last_split  1 if the last edc_verifier_verify / _verify_fallback on v ran the split
 *   plan, 0 if not; EDC_ERR_ARG before any verify and for NULL.
 * edc_vfy_last_plan   test hook: edc_debug_last_plan for the plan of the last verify or eager fold
 *   on v, whichever came last (a host copy, no device work); EDC_ERR_ARG before either and for NULL.
 *
 * Eager mode: the R terms are summed while the items arrive. z_i depends only on (z_seed, queue
 * index i), so a seed committed when the block starts lets every queue call add [z_i]R_i of its
 * items to a running point on the GPU; verify then runs the coefficients over all n items and an
 * MSM over B, the keys and the short tail of R terms not folded yet, adds the running point and
 * multiplies by 8. The group element is edc_batch_verify's with that seed: verdict and check8 are
 * bit-identical, in every grouping mode, split or not, and whatever the fold granularity. The time
 * from the last vote to the verdict no longer grows with the block; the queue calls cost more in
 * total (many small MSMs instead of one large one).
 * edc_vfy_begin_eager  v enters eager mode and commits this block's seed. Only while nothing is
 *   queued (after create or edc_verifier_reset; EDC_ERR_ARG otherwise). z_seed NULL: the library
 *   draws 32 bytes with getrandom(2); if that fails the call fails (EDC_ERR_HIP) and v stays as it
 *   was, never a fixed seed. z_i for queue index i is what edc_batch_verify draws from that seed.
 *   edc_verifier_reset leaves eager mode: begin again, with a fresh seed, for the next block.
 * edc_verifier_verify(v, NULL, NULL, check8) is the eager verify. Passing z_seed or z in eager
 *   mode is EDC_ERR_ARG (z is committed; caller-drawn z arrays are not available), and NULL / NULL
 *   on a verifier that is not eager stays EDC_ERR_ARG.
 * edc_verifier_verify_fallback(v, z_seed, ...) in eager mode runs the eager verify first (its
 *   check8) and, if it fails, the grouped fallback with the caller's fresh z_seed on the retained
 *   items: the per-item codes equal the non-eager call's.
 * edc_vfy_set_fold  a queue call folds the items not folded yet once at least min_items of them
 *   are pending (0: the library default, 131,072). Results never depend on it.
 * edc_vfy_folded    *items = queued items whose R term is in the running point, *folds = folds
 *   since the last reset (either may be NULL). EDC_ERR_ARG for a NULL verifier.
 * edc_vfy_eager     1 in eager mode, 0 if not, EDC_ERR_ARG for NULL.
 * Soundness. The batch equation needs z unpredictable to the signers when they fix their
 *   signatures (src/batch.rs:149-217 draws it after the last queue). A seed committed before the
 *   items arrive is just as unpredictable to them as long as it stays secret and is used for one
 *   block: pass fresh OS randomness (or NULL) and never reuse, log or derive it from public data.
 *   Nothing that depends on z leaves the library before verify. A verify that returns EDC_OK
 *   reveals only the identity point: more items may be queued and verified again under the same
 *   seed. A verify that returns EDC_INVALID_SIGNATURE reveals a z-dependent point (check8): from
 *   then on the seed is spent, and queue and verify calls on v return EDC_ERR_ARG until
 *   edc_verifier_reset. edc_verifier_verify_fallback is the exception: it draws its own z from
 *   the caller's fresh seed.
 *
 * Cached mode: queue calls skip the items the context's verified-signature table (edc_sigcache_*,
 * below) already vouches for. A node queues a block's votes as they arrive and saw most of them
 * at gossip time: the lookup runs at queue time, where the call already waits for its copies, and
 * a hit costs neither the R decode, nor the key grouping, nor any term of verify's MSM.
 * edc_vfy_set_cached  switches the mode (on != 0). Only while nothing is queued (after create or
 *   edc_verifier_reset; EDC_ERR_ARG otherwise). The mode is configuration: it survives
 *   edc_verifier_reset (eager mode does not). The call waits for an insert that an earlier verify
 *   on v left running. A verifier that is not in cached mode never touches the table.
 * edc_vfy_cached      1 in cached mode, 0 if not, EDC_ERR_ARG for NULL.
 * In cached mode every queue form (edc_verifier_queue / _prehashed / _device,
 *   edc_vfy_queue_indexed) brings its m items to the device (a staging area of the verifier; the
 *   _device form with d_k reads the caller's arrays in place), looks them up, and appends only
 *   the misses, in the order they were offered, as the retained items [n, n + c). The miss count
 *   c comes back to the host inside the call: its one added synchronization (the _device form
 *   also waits for the gather of the misses, the last read of the caller's arrays). Queue index
 *   i, and with it z_i, is the retained index: edc_verifier_verify is bit-identical (verdict and
 *   check8) to edc_batch_verify_prehashed_device on the miss list with z_base = 0, and to
 *   edc_batch_verify of it, also in eager mode with the committed seed and in every grouping and
 *   split mode; caller-drawn z holds one z_i per retained item (edc_verifier_size of them).
 *   Without a table on the context the call returns EDC_ERR_ARG and appends nothing; so does a
 *   call that would take the items offered since the last reset past 2^32 - 1. The lookups count
 *   in the table's hits / misses (edc_sigcache_stats).
 * edc_verifier_size   stays the number of retained items: offered - hits.
 * edc_vfy_cache_counts  *offered = items given to queue calls since the last reset, *hits = how
 *   many of them were skipped as records (either may be NULL). EDC_ERR_ARG for a NULL verifier.
 * Inserts. An edc_verifier_verify that returns EDC_OK inserts the retained items that are not
 *   records yet (the queue survives verify; a later verify inserts only what was queued since). A
 *   verify that fails, eager or not, inserts nothing. edc_verifier_verify_fallback and
 *   edc_vfy_verify_fallback_offered insert exactly the retained items whose code is EDC_OK. The
 *   insert runs on the verifier's stream behind the verdict and the call does not wait for it;
 *   every other use of the table (another verifier's queue call, the edc_sigcache_* entries)
 *   orders itself after it, so a record is never read while it is written.
 * edc_vfy_verify_fallback_offered  edc_verifier_verify_fallback with the codes in the order the
 *   items were offered: verdicts has `offered` bytes, a hit gets EDC_OK, a retained item its
 *   Item::verify_single code (src/batch.rs:104-107). On a verifier that is not in cached mode it
 *   is edc_verifier_verify_fallback, which itself keeps its meaning in cached mode:
 *   edc_verifier_size codes, in retained order.
 * Soundness of cached mode. A hit is worth what the verified-signature cache says below: a
 *   byte-identical (vk, sig, k) verified earlier on this context, one by one or inside a batch
 *   whose equation held. A verify that passes plants records, so its z must be fresh and secret,
 *   also in eager mode, where the seed is committed before the items arrive: with a predictable
 *   seed, crafted items that cancel inside one block would be accepted from then on. In the
 *   prehashed queue forms the caller vouches for k, as in every prehashed entry.
 */
typedef struct edc_verifier edc_verifier;
edc_verifier* edc_verifier_create(edc_ctx* ctx, size_t capacity_hint);
void edc_verifier_destroy(edc_verifier* v);
int edc_verifier_queue(edc_verifier* v, size_t m, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                       const uint64_t* msg_off);
int edc_verifier_queue_prehashed(edc_verifier* v, size_t m, const uint8_t* vk, const uint8_t* sig, const uint8_t* k);
int edc_verifier_queue_device(edc_verifier* v, size_t m, const uint8_t* d_vk, const uint8_t* d_sig,
                              const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k);
size_t edc_verifier_size(const edc_verifier* v);
int edc_verifier_verify(edc_verifier* v, const uint8_t z_seed[32], const uint8_t* z, uint8_t check8[32]);
int edc_verifier_verify_fallback(edc_verifier* v, const uint8_t z_seed[32], uint8_t* verdicts, int* n_invalid,
                                 uint8_t check8[32]);
int edc_verifier_reset(edc_verifier* v);
int edc_vfy_queue_indexed(edc_verifier* v, size_t m, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg,
                          const uint64_t* msg_off, const uint8_t* k);
int edc_vfy_last_split(const edc_verifier* v);
int edc_vfy_last_plan(const edc_verifier* v, edc_plan_info* out);
int edc_vfy_begin_eager(edc_verifier* v, const uint8_t z_seed[32]);
int edc_vfy_set_fold(edc_verifier* v, size_t min_items);
int edc_vfy_folded(const edc_verifier* v, uint64_t* items, uint64_t* folds);
int edc_vfy_eager(const edc_verifier* v);
int edc_vfy_set_cached(edc_verifier* v, int on);
int edc_vfy_cached(const edc_verifier* v);
int edc_vfy_cache_counts(const edc_verifier* v, uint64_t* offered, uint64_t* hits);
int edc_vfy_verify_fallback_offered(edc_verifier* v, const uint8_t z_seed[32], uint8_t* verdicts, int* n_invalid,
                                    uint8_t check8[32]);

/*
 * Templated messages: a block's votes from shared heads and tails plus a per-item hole. In a
 * canonical vote the type, height, round, block id and chain id are the same for every validator
 * and only a short field in the middle (the timestamp) differs, so the messages that Item::from
 * hashes (reference src/batch.rs:82-94: k = H(R || A || M)) are described as
 *     msg_i = head[tpl[i]] || var[var_off[i] .. var_off[i+1]) || tail[tpl[i]]
 * and assembled on the GPU: about 4 + 64 + 2 + 4 + |hole| bytes per vote over PCIe instead of a
 * whole message and an 8-byte offset, and no hashing on the host. Everything behind the assembled
 * arena is the message path of Verifier::queue / verify (src/batch.rs:127-217): k, verdict and
 * check8 are bit-identical to edc_challenge / edc_batch_verify[_device] / edc_verifier_queue on the
 * materialised messages with the same keys and z.
 *
 * edc_templates  the set of one call: `count` (1..65535) templates, template t's head is
 *   head[head_off[t] .. head_off[t+1]) and its tail likewise (count + 1 monotone offsets each; a
 *   head or tail may be empty; head and tail blobs together at most 1 MiB). Always host memory,
 *   borrowed like the call's other host buffers; the library copies it to the device. Nothing of it
 *   persists on the context: the height is part of the message, so the set changes every block.
 * Items: tpl[i] (uint16_t) < count; the hole bytes packed back to back in `var` (below 4 GiB) with
 *   n + 1 offsets var_off, var_off[0] = 0, monotone; a hole may be empty.
 * Host forms check the set and the items before anything is launched: any violation is EDC_ERR_ARG
 *   with nothing launched, appended or inserted. Exactly one of vk (n x 32 bytes) and key_idx
 *   (positions in the list last given to edc_keycache_load, as edc_batch_submit_indexed; an index
 *   outside the list is EDC_ERR_ARG).
 * Device forms take d_tpl / d_var / d_var_off in this GPU's memory and var_bytes, the declared size
 *   of d_var. The device checks tpl[i] < count and var_off[i] <= var_off[i+1] <= var_bytes; on any
 *   violation the messages are assembled as n empty messages, nothing outside the declared arrays
 *   is read, and the call returns EDC_ERR_ARG, never a verdict.
 * The assembled arena is sized without a read-back from the bound
 *   n (longest head + longest tail) + var_bytes + 16.
 *
 * edc_tmpl_expand_device  Item::from's message bytes (src/batch.rs:82-94) only: the arena into
 *   d_msg_out (16-byte aligned, msg_cap bytes; EDC_ERR_ARG if msg_cap is below the bound above) and
 *   the n + 1 uint64_t offsets into d_msg_off_out, ready for every *_device entry that takes a
 *   message arena (the fallback, edc_verify_each_device, the edc_sigcache_* and multi-GPU entries,
 *   whose Verifier::queue / verify, src/batch.rs:127-217, then run on it). Synchronous.
 * edc_tmpl_challenge  edc_challenge (Item::from, src/batch.rs:82-94) for templated messages: the k
 *   that Verifier::queue / verify (src/batch.rs:127-217) would take for each item; host buffers.
 * edc_tmpl_batch_verify  edc_batch_verify (Item::from, src/batch.rs:82-94, hashed on the device;
 *   Verifier::queue x n + verify, src/batch.rs:127-217); host buffers, synchronous, copied in one
 *   piece.
 * edc_tmpl_batch_verify_device  edc_batch_verify_device (src/batch.rs:82-94, :127-217) with the
 *   messages assembled into the context's workspace first; z as edc_batch_verify_device.
 * edc_tmpl_batch_submit  edc_batch_submit / edc_batch_submit_indexed (src/batch.rs:82-94,
 *   :127-217): staged into the slot's own buffers, waited with edc_batch_wait; host buffers, the
 *   set included, are borrowed until the wait.
 * edc_vfy_queue_templated  edc_verifier_queue / edc_vfy_queue_indexed (Item::from, src/batch.rs:82-94,
 *   and Verifier::queue x m, :127-137; verify, :149-217, later covers the items like any other):
 *   appends m items to an incremental verifier. Once the arena is on the device the range takes the
 *   path of edc_verifier_queue, so it works in eager and cached mode and mixes with the other queue
 *   forms. key_idx without a registered list is EDC_ERR_ARG with nothing appended.
 * A NULL ctx / verifier is EDC_ERR_ARG; n = 0 returns what the message entry returns for n = 0.
 */
typedef struct edc_templates {      /* host memory, borrowed for the call */
  uint32_t count;
  const uint8_t* head; const uint32_t* head_off;   /* count + 1 */
  const uint8_t* tail; const uint32_t* tail_off;   /* count + 1 */
} edc_templates;
int edc_tmpl_expand_device(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint16_t* d_tpl, const uint8_t* d_var,
                           const uint32_t* d_var_off, size_t var_bytes, uint8_t* d_msg_out, size_t msg_cap,
                           uint64_t* d_msg_off_out);
int edc_tmpl_challenge(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* vk, const uint8_t* sig,
                       const uint16_t* tpl, const uint8_t* var, const uint32_t* var_off, uint8_t* k_out);
int edc_tmpl_batch_verify(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* vk, const uint32_t* key_idx,
                          const uint8_t* sig, const uint16_t* tpl, const uint8_t* var, const uint32_t* var_off,
                          const uint8_t z_seed[32], uint8_t check8[32]);
int edc_tmpl_batch_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* d_vk,
                                 const uint8_t* d_sig, const uint16_t* d_tpl, const uint8_t* d_var,
                                 const uint32_t* d_var_off, size_t var_bytes, const uint8_t z_seed[32], uint64_t z_base,
                                 const uint8_t* d_z, uint8_t check8[32]);
int64_t edc_tmpl_batch_submit(edc_ctx* ctx, const edc_templates* ts, size_t n, const uint8_t* vk, const uint32_t* key_idx,
                              const uint8_t* sig, const uint16_t* tpl, const uint8_t* var, const uint32_t* var_off,
                              const uint8_t z_seed[32], uint64_t z_base, int want_check8);
int edc_vfy_queue_templated(edc_verifier* v, const edc_templates* ts, size_t m, const uint8_t* vk,
                            const uint32_t* key_idx, const uint8_t* sig, const uint16_t* tpl, const uint8_t* var,
                            const uint32_t* var_off);

/*
 * Commit sets: many variable-size batches in one launch. Block sync, a light client catching up
 * and a node replaying a chain hold thousands of commits, each its own batch::Verifier (reference
 * src/batch.rs:110-217) over the ~150 precommits of one height, each with its own verdict (the
 * per-commit flow of reference tests/batch.rs:18-44). A commit set is n items in queue order with
 * nc + 1 offsets commit_off (uint32_t, host memory): commit_off[0] = 0, monotone,
 * commit_off[nc] = n < 2^28; commit c is items [commit_off[c], commit_off[c+1]), empty commits
 * allowed. It is verified as nc independent Verifiers:
 *  - commit_verdicts (host, nc bytes, nullable): commit c's EDC_OK or EDC_INVALID_SIGNATURE, what
 *    edc_batch_verify_device returns for commit c alone with a fresh seed (Verifier::verify,
 *    src/batch.rs:149-217, reports a malformed key as InvalidSignature too; an empty Verifier
 *    verifies, so an empty commit is EDC_OK).
 *  - item_verdicts (host, n bytes, nullable): Item::verify_single's code (src/batch.rs:104-107) of
 *    every item, as edc_batch_verify_fallback_device; all zeros when the launch passes.
 *  - *n_bad_commits (nullable): the number of commits that are not EDC_OK.
 *  - Returns EDC_OK if every commit passed, EDC_INVALID_SIGNATURE if any did not, <0 on a runtime
 *    or argument failure.
 * Union first: the launch runs as ONE batch over all n items, item i drawing z at index i of
 * z_seed's stream: exactly the pipeline of edc_batch_verify_device, no kernel and no
 * synchronization more. Its equation is the sum of the commits' equations, so when it holds every
 * commit holds, with the probability batch verification itself gives (the argument of
 * edc_batch_submit_multi_device). When it fails, the grouped fallback of
 * edc_batch_verify_fallback_device runs on the state the failed batch left in its slot (k, decoded
 * points, key grouping, failure bits, the same z_seed; nothing is uploaded or hashed again), and a
 * commit is EDC_INVALID_SIGNATURE iff one of its items has a non-zero code.
 * Soundness: as edc_batch_verify_fallback_device (edc_find_invalid_device above). An item of a
 * passing range, and a commit of a passing launch, is reported valid because a batch equation
 * holds; this relies on z being unpredictable to whoever made the signatures. z_seed MUST be fresh
 * and secret for every call (e.g. 32 bytes of OS randomness); a known or reused seed lets crafted
 * invalid signatures cancel inside a launch or a range and be reported valid.
 *
 * edc_commits_verify_device  Verifier::queue x n + verify per commit (src/batch.rs:127-137,
 *   :149-217) on device-resident inputs; synchronous, on slot 0 like the other synchronous entries.
 *   Device arrays as the other *_device entries (same alignment rules); d_k nullable: when given,
 *   the messages are not read (d_msg / d_msg_off may be NULL).
 * edc_commits_verify  the host-buffer form (src/batch.rs:127-137, :149-217): exactly one of vk and
 *   key_idx (positions in the list last given to edc_keycache_load), exactly one of
 *   (msg, msg_off) and k (prehashed, canonical scalars < l). Staged into the slot in one piece.
 * edc_tmpl_commits_verify  templated messages (above; Item::from, src/batch.rs:82-94, then
 *   src/batch.rs:127-137, :149-217) with ONE TEMPLATE PER COMMIT: commit_tpl[c] (uint16_t, host,
 *   nc entries, each < ts->count) is the template of every item of commit c, as height and block
 *   id are the commit's. The items carry only sig, their hole (var, var_off as the edc_tmpl_*
 *   entries) and vk or key_idx; the per-item template array is made on the device.
 * edc_commits_submit / edc_tmpl_commits_submit / edc_commits_submit_device  the asynchronous forms
 *   (src/batch.rs:127-137, :149-217 per commit), under the rules of edc_batch_submit /
 *   edc_batch_submit_device: a ticket >= 0 (or <0), inputs (commit_off too) borrowed until the
 *   wait, tickets waited in submission order.
 * edc_commits_wait  waits for the ticket; if the union failed, the grouped fallback
 *   (src/batch.rs:104-107 per item) runs ON THE TICKET'S OWN SLOT, where the inputs are still
 *   staged or borrowed, while other tickets stay in flight on theirs. A commit-set ticket given to
 *   edc_batch_wait or edc_batch_wait_multi, and a batch or multi-batch ticket given to
 *   edc_commits_wait, is EDC_ERR_ARG and stays pending. With nc = 1 this is the streamed
 *   batch-with-fallback that the streaming entries (edc_batch_submit*, whose edc_batch_wait returns
 *   one bit) never had: a failed batch gets its per-item codes without a second upload.
 * Every argument is checked on the host before anything is launched; a violation is EDC_ERR_ARG
 *   with nothing launched: NULL ctx or z_seed, both or neither of a one-of pair, commit_off[0] != 0,
 *   a decreasing offset, n >= 2^28, commit_tpl[c] >= count, a template set or hole offsets the
 *   edc_tmpl_* host forms refuse, a key index outside the registered list, a prehashed k >= l in
 *   the host forms (a device d_k is checked by the batch itself: EDC_ERR_ARG from the call / the
 *   wait, never a verdict). nc = 0 returns EDC_OK from the synchronous forms (commit_off is not
 *   read); the asynchronous forms return a ticket whose wait returns EDC_OK.
 * edc_debug_tmpl_commit_map  test / measurement hook: the commit-to-item template map alone
 *   (tpl_out[i] = commit_tpl[c] for the commit c holding item i; host arrays, checked as above),
 *   run `reps` times between HIP events; *ms (nullable) = the mean kernel time.
 */
int edc_commits_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                              const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                              const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                              int* n_bad_commits);
int edc_commits_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk, const uint32_t* key_idx,
                       const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k,
                       const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits);
int edc_tmpl_commits_verify(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                            const uint16_t* commit_tpl, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                            const uint8_t* var, const uint32_t* var_off, const uint8_t z_seed[32],
                            uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits);
int64_t edc_commits_submit(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                           const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                           const uint8_t* k, const uint8_t z_seed[32]);
int64_t edc_tmpl_commits_submit(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, const uint8_t* vk, const uint32_t* key_idx,
                                const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                                const uint8_t z_seed[32]);
int64_t edc_commits_submit_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                  const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off,
                                  const uint8_t* d_k, const uint8_t z_seed[32]);
int edc_commits_wait(edc_ctx* ctx, int64_t ticket, uint8_t* commit_verdicts, uint8_t* item_verdicts,
                     int* n_bad_commits);
int edc_debug_tmpl_commit_map(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint16_t* commit_tpl,
                              uint16_t* tpl_out, int reps, float* ms);

/*
 * Templated commit sets with per-item template variants, and their device-resident forms. A real
 * commit does not fit one template: a precommit for nil signs another block id than a precommit
 * for the block, and the sign bytes start with their own length, so a vote whose hole (the
 * timestamp) encodes a byte longer or shorter has another first head byte. Two more inputs
 * describe that at one byte per vote:
 *   alt_span (1..256, one per call): every commit c, empty ones included, owns the window
 *     [commit_tpl[c], commit_tpl[c] + alt_span) of the set; commit_tpl[c] + alt_span <= ts->count.
 *   item_alt[i] (uint8_t, n entries, < alt_span; NULL = all zeros): the template of item i is
 *     commit_tpl[c] + item_alt[i] for the commit c that holds it.
 * With alt_span = 1 and item_alt = NULL every entry below is the one-template-per-commit call: the
 * same verdicts and item codes. Everything behind the per-item template array is unchanged (the
 * expansion, SHA-512, union first, the fallback at the wait on the ticket's own slot, the
 * reduction to commits), so for the same keys and z_seed the commit verdicts, item verdicts and
 * n_bad_commits are bit-identical to edc_commits_verify on the materialised messages. Results,
 * return values and the soundness requirement on z_seed are those of the commit-set entries above;
 * commit_off, commit_tpl and the template set are host memory in every form.
 *
 * edc_tmpl_commits_verify_alt  edc_tmpl_commits_verify with variants (Item::from,
 *   src/batch.rs:82-94, then Verifier::queue x n + verify per commit, src/batch.rs:127-137,
 *   :149-217; the item codes are Item::verify_single's, src/batch.rs:104-107); host buffers,
 *   synchronous. item_alt is staged into the slot beside commit_off and commit_tpl.
 * edc_tmpl_commits_submit_alt  the asynchronous host form (src/batch.rs:82-94, :127-137, :149-217
 *   per commit; :104-107 per item at the wait): a ticket for edc_commits_wait under its ticket
 *   rules; the inputs, item_alt included, are borrowed until the wait.
 *   Host forms check everything before anything is launched, as edc_tmpl_commits_verify does, and
 *   in addition: alt_span outside 1..256, a window that leaves the set, an item_alt[i] >= alt_span.
 *   Any violation is EDC_ERR_ARG with nothing launched.
 * edc_tmpl_commits_verify_device  the items in this GPU's memory (src/batch.rs:82-94, :127-137,
 *   :149-217 per commit; :104-107 per item): d_vk (n x 32) and d_sig (n x 64) 16-byte aligned as
 *   the other *_device entries, d_var / d_var_off / var_bytes as edc_tmpl_batch_verify_device,
 *   d_item_alt n bytes of any alignment (NULL = all zeros). Only commit_off, commit_tpl and the set
 *   are copied; the arrays are read in place. The host checks the offsets, alt_span and the
 *   windows (EDC_ERR_ARG, nothing launched); the device checks the holes and d_item_alt[i] <
 *   alt_span. On a violation the messages are assembled as n empty messages, nothing outside the
 *   declared arrays is read, no template index at or above ts->count is formed, and the call
 *   returns EDC_ERR_ARG, never a verdict; the context stays usable. Synchronous, on slot 0.
 * edc_tmpl_commits_submit_device  its asynchronous form (src/batch.rs:82-94, :127-137, :149-217;
 *   :104-107 at the wait): a ticket for edc_commits_wait; the device arrays and commit_off stay
 *   the caller's until the wait, which returns EDC_ERR_ARG where the synchronous form would.
 * edc_debug_tmpl_commit_map_alt  test / measurement hook: the map with variants alone
 *   (tpl_out[i] = commit_tpl[c] + item_alt[i]; host arrays; offsets and alt_span checked as above,
 *   the variant bytes by the device), run `reps` times between HIP events. *flagged (nullable) = 1
 *   if the device found an item_alt[i] >= alt_span; such an item gets its commit's base. The device
 *   copies of item_alt and tpl_out start at the host pointers' offsets from a 16-byte boundary, so
 *   a test reaches the kernel's unaligned paths by offsetting its arrays. *ms as above.
 * nc = 0 and a NULL ctx or z_seed: as the commit-set entries above.
 */
int edc_tmpl_commits_verify_alt(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt,
                                const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                                const uint8_t* var, const uint32_t* var_off, const uint8_t z_seed[32],
                                uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits);
int64_t edc_tmpl_commits_submit_alt(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt,
                                const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig,
                                const uint8_t* var, const uint32_t* var_off, const uint8_t z_seed[32]);
int edc_tmpl_commits_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                const uint32_t* d_var_off, size_t var_bytes, const uint8_t z_seed[32],
                                uint8_t* commit_verdicts, uint8_t* item_verdicts, int* n_bad_commits);
int64_t edc_tmpl_commits_submit_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                const uint32_t* d_var_off, size_t var_bytes, const uint8_t z_seed[32]);
int edc_debug_tmpl_commit_map_alt(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint16_t* commit_tpl,
                                uint32_t alt_span, const uint8_t* item_alt, uint16_t* tpl_out, int* flagged,
                                int reps, float* ms);

/*
 * Quorum commit sets: tally voting power and verify only the votes that are needed. A consensus
 * node does not ask "does every signature of commit c verify" but "did validators holding more
 * than the required voting power sign this block": CometBFT's VerifyCommit (every vote that
 * carries a signature is verified, only the votes for the block count), VerifyCommitLight (votes
 * for the block are verified only until the tally passes 2/3 of the set's power) and
 * VerifyCommitLightTrusting (the same against 1/3 of a trusted set's power). The reference crate
 * has no such API and none of its APIs changes meaning: every vote that is checked is one
 * batch::Item (src/batch.rs:76-94) in ONE batch::Verifier (queue + verify, src/batch.rs:127-137,
 * :149-217), and its code is Item::verify_single's (src/batch.rs:104-107).
 *
 * A quorum commit set is a commit set as defined above (n items in queue order, nc + 1 offsets
 * commit_off in host memory, the same limits; a commit lists EVERY validator of its set) with
 *   power[i]      uint64_t, n entries: the voting power of item i's validator. Every power is at
 *                 most 2^63 - 1, and so is the sum of the counted (flag 1) powers of one commit.
 *   flag[i]       uint8_t, n entries: EDC_VOTE_ABSENT (no signature: never verified, never counted;
 *                 its vk / sig / message bytes are never interpreted), EDC_VOTE_COMMIT (a precommit
 *                 for the block: verified, counted) or EDC_VOTE_NIL (a precommit for nil: verified
 *                 in full mode, never counted). Any other value is an argument error.
 *   threshold[c]  uint64_t, nc entries, host memory. Commit c has its quorum iff its tally is
 *                 STRICTLY GREATER than threshold[c]: pass floor(2T/3) for a commit of a set with
 *                 total power T, floor(T/3) for the trusting check.
 *   mode          EDC_QUORUM_FULL (VerifyCommit): the checked items are those with flag 1 or 2.
 *                 EDC_QUORUM_LIGHT (VerifyCommitLight): item i is checked iff its flag is 1 and the
 *                 sum of power over the flag-1 items before it in its commit is <= threshold[c],
 *                 i.e. the quorum was not yet reached when the loop arrives at it. The trusting
 *                 check is light mode with the trusted set's powers and EDC_VOTE_ABSENT for the
 *                 signers that set does not know.
 * Only the checked items are verified. They are gathered in queue order into one batch, checked
 * item j drawing z at index j of z_seed's stream: the union verdict and check8 (nullable) are
 * bit-identical to edc_batch_verify_prehashed_device on the gathered (vk, sig, k) list with
 * z_base = 0 (the contract of the verified-signature cache for its miss list), and when that union
 * fails the grouped fallback runs on that list as edc_batch_verify_fallback_device. Soundness and
 * the requirement on z_seed (fresh and secret for every call) are those of the commit-set entries.
 * Outputs (host, all nullable):
 *   item_verdicts    n bytes: Item::verify_single's code of a checked item, EDC_NOT_CHECKED for
 *                    every other item.
 *   tally            uint64_t, nc: the sum of power over the checked items with flag 1 and code EDC_OK.
 *   commit_verdicts  nc bytes: EDC_INVALID_SIGNATURE if any checked item of the commit has a non-zero
 *                    code (also when the commit is short only because that item's power is missing);
 *                    otherwise EDC_QUORUM_SHORT if tally[c] <= threshold[c]; otherwise EDC_OK. "Strictly
 *                    greater" decides the empty case: an empty or all-absent commit has tally 0 and is
 *                    EDC_QUORUM_SHORT, also with threshold 0.
 *   *n_bad_commits   the commits that are not EDC_OK.   *n_checked  the size of the gathered list.
 * Return value: EDC_OK iff every commit is EDC_OK; EDC_INVALID_SIGNATURE if any commit is
 * EDC_INVALID_SIGNATURE; otherwise EDC_QUORUM_SHORT; <0 on a runtime or argument failure.
 *
 * edc_quorum_plan  the selection alone, on host arrays (no signatures): checked[i] (n bytes, 0 / 1),
 *   planned[c] (the tally commit c gets if every checked item verifies) and *n_checked, all
 *   nullable. It runs the kernels every form below runs, so a caller can size its work with it.
 * edc_quorum_verify_device  the items in this GPU's memory: d_vk, d_sig and d_msg / d_msg_off or d_k
 *   as edc_commits_verify_device (16-byte aligned), d_power 8-byte aligned, d_flag of any
 *   alignment; commit_off and threshold on the host. Synchronous, on slot 0 (EDC_ERR_ARG while a
 *   submitted batch is pending there). Without d_k, k is hashed for all n items first, skipped
 *   votes included: their messages must be mapped like any other.
 * edc_quorum_verify  host buffers: exactly one of vk and key_idx, exactly one of (msg, msg_off) and
 *   k, as edc_commits_verify; power and flag are staged beside them. A prehashed k must be
 *   canonical for the checked items only.
 * Argument checks: a violation is EDC_ERR_ARG with nothing verified and no output written. The host
 *   forms (plan included) check the offsets, the flags, the power bounds and the per-commit sums
 *   before anything is launched. The device form checks the offsets on the host and the flags,
 *   bounds and sums ON THE DEVICE, before anything is gathered: on a violation no index outside the
 *   declared arrays is formed, the call returns EDC_ERR_ARG, never a verdict, and the context stays
 *   usable. nc = 0 returns EDC_OK (no array is read); a NULL ctx or z_seed is EDC_ERR_ARG. These
 *   entries need no verified-signature table on the context.
 * edc_debug_quorum_select  measurement hook: the selection kernels alone on host arrays (checked as
 *   edc_quorum_plan), run `reps` times between HIP events; *ms (nullable) = the mean time.
 * Out of scope for these entries: asynchronous submit / wait forms; templated forms are the
 *   edc_tmpl_quorum_* entries below; the incremental verifier and the multi-GPU engine have no
 *   quorum entries.
 */
#define EDC_QUORUM_SHORT 3           /* every checked vote verified, tally <= threshold */
#define EDC_NOT_CHECKED 255          /* item_verdicts: the vote was not verified */
#define EDC_VOTE_ABSENT 0
#define EDC_VOTE_COMMIT 1
#define EDC_VOTE_NIL 2
#define EDC_QUORUM_FULL 0
#define EDC_QUORUM_LIGHT 1
int edc_quorum_plan(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* power, const uint8_t* flag,
                    const uint64_t* threshold, int mode, uint8_t* checked, uint64_t* planned, size_t* n_checked);
int edc_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                             const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                             const uint64_t* d_power, const uint8_t* d_flag, const uint64_t* threshold, int mode,
                             const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                             int* n_bad_commits, size_t* n_checked, uint8_t check8[32]);
int edc_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk, const uint32_t* key_idx,
                      const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* k,
                      const uint64_t* power, const uint8_t* flag, const uint64_t* threshold, int mode,
                      const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                      int* n_bad_commits, size_t* n_checked, uint8_t check8[32]);
int edc_debug_quorum_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint64_t* power,
                            const uint8_t* flag, const uint64_t* threshold, int mode, int reps, float* ms);

/*
 * Templated quorum commit sets: hash only the votes that are checked. The two halves above meet
 * here: the votes are templated (shared heads and tails plus a hole and a variant byte per vote,
 * as edc_tmpl_commits_verify_alt / _device take them) and the verdict is a quorum verdict (power,
 * flag, threshold and mode as edc_quorum_verify / _device take them). The template inputs (ts,
 * commit_tpl, alt_span, item_alt, var, var_off, var_bytes) mean exactly what they mean for
 * edc_tmpl_commits_verify_alt / edc_tmpl_commits_verify_device, the quorum inputs and all outputs
 * exactly what they mean for edc_quorum_verify / edc_quorum_verify_device; commit_off, commit_tpl,
 * threshold and the template set are host memory in both forms.
 *
 * Equality contract: for the same keys, powers, flags, thresholds, mode and z_seed every output
 * (the return value, commit_verdicts, item_verdicts, tally, *n_bad_commits, *n_checked and check8)
 * equals what edc_quorum_verify[_device] gives on the materialised messages
 * head[t] || hole || tail[t]. Equivalently, the union verdict and check8 are those of
 * edc_batch_verify_prehashed_device on the gathered checked list with z_base = 0. Every checked
 * vote is one batch::Item (Item::from, src/batch.rs:82-94) in ONE batch::Verifier (queue and
 * verify, src/batch.rs:127-137, :149-217), and its code is Item::verify_single's
 * (src/batch.rs:104-107). Soundness and the requirement on z_seed are those of the quorum entries.
 *
 * Select first: the selection needs only power, flag and the offsets, so it runs before any
 * message exists. Only the checked votes are gathered, in queue order (key, signature, template
 * index and hole), only their messages are assembled and only they are hashed; the arena is sized
 * after the read-back of the checked count, from n_checked and not from n. A vote that is not
 * checked has its vk, sig and hole BYTES never interpreted: noise there changes no output (its
 * variant byte and its hole offsets are still checked, see below). The call adds no stream
 * synchronization to the one edc_quorum_verify_device has for the checked count. When every vote
 * is checked nothing is gathered; when none is, the n = 0 batch runs.
 *
 * edc_tmpl_quorum_verify_device  the items in this GPU's memory: d_vk, d_sig, d_item_alt, d_var,
 *   d_var_off, var_bytes as edc_tmpl_commits_verify_device, d_power and d_flag as
 *   edc_quorum_verify_device. Synchronous, on slot 0 (EDC_ERR_ARG while a submitted batch is
 *   pending there). The host checks the offsets, the set, alt_span and the windows (EDC_ERR_ARG,
 *   nothing launched). The device checks the flags, the powers and the per-commit sums as the
 *   quorum entries do, and, for ALL n items and not only the checked ones, d_item_alt[i] < alt_span
 *   and var_off[i] <= var_off[i+1] <= var_bytes: so EDC_ERR_ARG does not depend on the mode or on
 *   which votes the thresholds select. The flag travels in the read-back of the checked count; on a
 *   violation nothing is gathered, no index outside the declared arrays is formed, and the call
 *   returns EDC_ERR_ARG, never a verdict; the context stays usable.
 * edc_tmpl_quorum_verify  host buffers: exactly one of vk and key_idx (positions in the list last
 *   given to edc_keycache_load), staged in one piece beside power and flag. Everything is checked on
 *   the host before anything is launched, the union of the checks of edc_tmpl_commits_verify_alt
 *   and edc_quorum_verify: the one-of pair, an index outside the registered list, the set,
 *   alt_span, the windows, item_alt[i] < alt_span, the hole offsets, the flags, the power bounds.
 * nc = 0 returns EDC_OK (no array is read); a NULL ctx or z_seed is EDC_ERR_ARG.
 * edc_debug_tmpl_quorum_last  test hook, a host copy (no device work): out = {n, n_checked, the
 *   items the expansion and SHA-512 ran over, the arena bytes assembled} of the last templated
 *   quorum call on the context that reached its selection. EDC_ERR_ARG before any such call and
 *   for NULL.
 */
int edc_tmpl_quorum_verify(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                           const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt, const uint8_t* vk,
                           const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                           const uint64_t* power, const uint8_t* flag, const uint64_t* threshold, int mode,
                           const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                           int* n_bad_commits, size_t* n_checked, uint8_t check8[32]);
int edc_tmpl_quorum_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                  const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                  const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                  const uint32_t* d_var_off, size_t var_bytes, const uint64_t* d_power,
                                  const uint8_t* d_flag, const uint64_t* threshold, int mode, const uint8_t z_seed[32],
                                  uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally, int* n_bad_commits,
                                  size_t* n_checked, uint8_t check8[32]);
int edc_debug_tmpl_quorum_last(const edc_ctx* ctx, uint64_t out[4]);

/*
 * Verified-signature cache: skip the items that already verified on this context. A consensus
 * node verifies the same vote several times: once when it arrives by gossip
 * (VerificationKey::verify, src/verification_key.rs:225-258, or Item::verify_single,
 * src/batch.rs:104-107), again inside the block's commit (Verifier::verify, src/batch.rs:149-217),
 * again as the next block's last-commit and again in block sync. Under ZIP215 batch and single
 * verification agree and the verdict is a pure function of (vk_bytes, sig, k), so a byte-identical
 * item that verified before verifies again. The reference keeps no such table; nothing of its API
 * changes meaning.
 *
 * The table lives in this GPU's memory, one per context: open addressing with a bounded probe
 * window (32 slots), hashed under a key derived from the context's secret so that items chosen
 * by the network cannot be aimed at one window. A slot is an 8-byte header (fingerprint and the
 * generation of the insert; 0 = never used) and the 128-byte record vk || sig || k, k the
 * canonical challenge H(R || A || M) mod l: it binds the message, so a different message is a
 * different record. A hit is a live header AND 128 equal bytes, never a fingerprint alone. An
 * insert that finds no free or expired slot in its window is dropped and counted; it never evicts
 * a live record. Ageing is by generation: edc_sigcache_advance (once per height) bumps the table's
 * generation, and a record inserted more than `keep` generations ago is dead: lookups do not
 * return it and inserts reuse its slot.
 *
 * Semantics of the cached entries. The items that miss, in queue order, form the batch that is
 * verified: miss j (0-based among the misses) draws z_j at index j of z_seed's stream, so verdict
 * and check8 are bit-identical to edc_batch_verify_prehashed_device on the miss list with
 * z_base = 0; no miss returns what that entry returns for n = 0. *n_miss (nullable) receives the
 * number of misses. They run on slot 0 (refused while submitted batches are in flight, as the
 * other synchronous calls), and return EDC_ERR_ARG while the context has no table. A prehashed
 * k >= l in an item that misses is EDC_ERR_ARG with nothing inserted.
 *
 * Soundness. A hit means that a byte-identical (vk, sig, k) verified earlier on this context,
 *   either one by one or inside a batch whose equation held: it carries the probability that
 *   batch verification itself gives, no more. z_seed must therefore be fresh and secret for every
 *   call: with a predictable seed, crafted items that cancel inside one batch would be planted as
 *   records and accepted from then on, although they would not verify on their own. In the
 *   prehashed forms the caller vouches for k, as in every prehashed entry: a record is only as
 *   good as the k it was inserted with. The table is per context and never shared: what one
 *   context verified says nothing to another.
 *
 * edc_sigcache_create  a table of `capacity` records (rounded up to a power of two, at least 32;
 *   136 bytes of device memory each), replacing any existing table; capacity 0 only frees it.
 *   keep 0 means the default, 2. Refused while batches are in flight. EDC_ERR_NOMEM if the device
 *   cannot hold it (the context then has no table).
 * edc_sigcache_clear   empties the table (generation and counters stay).
 * edc_sigcache_advance bumps the generation (a node calls it once per height).
 * edc_sigcache_stats   out = {capacity, generation, hits, misses, inserted, dropped}: items the
 *   cached verify entries found / did not find, records written, inserts dropped for a full window
 *   (lookups and inserts of cached verifiers, edc_vfy_set_cached, included; the call waits for an
 *   insert such a verifier left running).
 * edc_sigcache_lookup_device  d_hit[i] = 1 iff item i is a live record (device arrays, 16-byte
 *   aligned vk / sig / k; d_hit n bytes); changes neither the table nor the counters.
 * edc_sigcache_batch_verify_device  Verifier::queue x n + Verifier::verify(rng) (reference
 *   src/batch.rs:127-217) over the items not verified before. d_k nullable: when given, the
 *   messages are not read (d_msg / d_msg_off may be NULL); otherwise k is hashed for every item
 *   first. When the miss batch passes, every miss is inserted; when it fails, nothing is.
 * edc_sigcache_batch_verify  the host-buffer form (src/batch.rs:127-217): exactly one of
 *   (msg, msg_off) and k.
 * edc_sigcache_batch_verify_fallback_device  the batch and, if it fails, the grouped fallback of
 *   edc_batch_verify_fallback_device on the miss list (src/batch.rs:127-217, :104-107): verdicts
 *   (host, n bytes) receive Item::verify_single's code for every item, hits EDC_OK; *n_invalid
 *   (nullable) their count. Exactly the misses whose code is EDC_OK are inserted. z_seed as
 *   edc_find_invalid_device.
 * edc_sigcache_verify_each  Item::verify_single (src/batch.rs:104-107) / VerificationKey::verify
 *   (src/verification_key.rs:225-258) for the misses only, with the per-item kernels of
 *   edc_verify_each; host buffers, exactly one of (msg, msg_off) and k. verdicts[i] as
 *   edc_verify_each (hits EDC_OK); the misses that are EDC_OK are inserted. This is the
 *   gossip-time feed of the table.
 */
int edc_sigcache_create(edc_ctx* ctx, size_t capacity, int keep);
int edc_sigcache_clear(edc_ctx* ctx);
int edc_sigcache_advance(edc_ctx* ctx);
int edc_sigcache_stats(const edc_ctx* ctx, uint64_t out[6]);
int edc_sigcache_lookup_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_k,
                               uint8_t* d_hit);
int edc_sigcache_batch_verify_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                     const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                     const uint8_t z_seed[32], uint8_t check8[32], size_t* n_miss);
int edc_sigcache_batch_verify(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                              const uint64_t* msg_off, const uint8_t* k, const uint8_t z_seed[32], uint8_t check8[32],
                              size_t* n_miss);
int edc_sigcache_batch_verify_fallback_device(edc_ctx* ctx, size_t n, const uint8_t* d_vk, const uint8_t* d_sig,
                                              const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_k,
                                              const uint8_t z_seed[32], uint8_t* verdicts, int* n_invalid,
                                              uint8_t check8[32], size_t* n_miss);
int edc_sigcache_verify_each(edc_ctx* ctx, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                             const uint64_t* msg_off, const uint8_t* k, uint8_t* verdicts, size_t* n_miss);

/*
 * Cached quorum commit sets: skip checked votes that already verified. The quorum entries and the
 * verified-signature cache are meant for the same moment: a live node has verified almost every
 * precommit of a block at gossip time (edc_sigcache_verify_each), and when the block's commit
 * arrives it runs VerifyCommit or VerifyCommitLight over those same votes; the same holds for the
 * next block's last-commit and for block sync. The motivating flow is CometBFT's
 * VerifyCommitLightWithCache / VerifyCommitLightTrustingWithCache, named here from memory and not
 * checked against a source tree. The reference crate has no such API and none of its APIs changes
 * meaning: every vote that is verified is one batch::Item (src/batch.rs:76-94) in ONE
 * batch::Verifier (queue + verify, src/batch.rs:127-137, :149-217), and its code is
 * Item::verify_single's (src/batch.rs:104-107).
 *
 * Inputs and outputs mean exactly what they mean for edc_quorum_verify[_device] and
 * edc_tmpl_quorum_verify[_device]. The one new output, size_t* n_miss (nullable), receives the size
 * of the list that was actually verified.
 *
 * Contract.
 * Selection. checked[i] and *n_checked are those of edc_quorum_plan for the same powers, flags,
 *   thresholds and mode, whatever the table holds: the selection never looks at the table. A hit
 *   still counts towards the running sum of light mode, as CometBFT's loop tallies a cached vote
 *   like any other.
 * Hit. A checked item that is a live record (a live header and 128 equal bytes, as
 *   edc_sigcache_lookup_device defines it) is a hit. A hit is not verified, its code is EDC_OK, and
 *   its power counts if its flag is 1. Items that are not checked are never looked up, never
 *   interpreted and never inserted.
 * Miss list. The checked misses, in queue order, form ONE batch; miss j draws z at index j of
 *   z_seed's stream. The union verdict and check8 are bit-identical to
 *   edc_batch_verify_prehashed_device on that list with z_base = 0, and if the union fails the
 *   grouped fallback runs on that list. n_miss = 0 runs the n = 0 batch.
 * Outputs. item_verdicts[i] is EDC_NOT_CHECKED (255) for an item that is not checked, 0 for a hit
 *   and Item::verify_single's code for a miss. tally, commit_verdicts, *n_bad_commits and the return
 *   value are derived from those codes exactly as the quorum section defines.
 * Inserts. Exactly the misses whose code is EDC_OK are inserted: all misses when the union passes,
 *   only the OK misses when it fails. Valid nil votes of full mode are inserted too. The insert
 *   finishes before the call returns.
 * Statistics. edc_sigcache_stats hits and misses grow by the lookups of the checked items only.
 * Equality contract. With a table in which no checked item is a record, every output equals the
 *   uncached entry's on the same inputs, check8 included, and n_miss == n_checked. With any table
 *   whose records were planted by verification on this context, every output except check8 and
 *   n_miss equals the uncached entry's.
 * Errors. No table on the context returns EDC_ERR_ARG with nothing written. Every argument check
 *   of the uncached forms applies, on the host for the host forms and on the device for the device
 *   forms; for the templated forms this means all n items, not only the checked ones. A violation
 *   returns EDC_ERR_ARG: no verdict is given, nothing is inserted, no counter changes, no index
 *   outside the declared arrays is formed, and the context stays usable. A prehashed k must be
 *   canonical for the checked items, as today. nc = 0 returns EDC_OK with no array read; a NULL ctx
 *   or z_seed is EDC_ERR_ARG. The calls are synchronous on slot 0, and EDC_ERR_ARG while a batch is
 *   pending there.
 * Soundness of a cached quorum. A hit lends its voting power to a quorum on the strength of an
 *   earlier verification on this context, one by one or inside a batch whose equation held: it
 *   carries the probability that batch verification itself gives, no more. z_seed must be fresh and
 *   secret for every call, because a passing call plants records: with a predictable seed, crafted
 *   votes that cancel inside one batch would be planted and would lend their power to every later
 *   quorum. The table is per context and never shared. In the prehashed forms the caller vouches
 *   for k.
 *
 * Stream synchronizations. In the plain forms k exists for all n items before the selection, so the
 *   masked lookup runs behind the selection and its miss and hit counts travel in the selection's
 *   one read-back: edc_cached_quorum_verify_device adds no stream synchronization to what
 *   edc_quorum_verify_device has. In the templated forms k exists only for the votes that were
 *   gathered and hashed after that read-back, so the lookup runs on the checked list and the miss
 *   count needs a SECOND read-back and stream synchronization before the batch can be planned.
 *
 * edc_cached_quorum_verify_device  edc_quorum_verify_device through the table (src/batch.rs:76-94,
 *   :104-107, :127-137, :149-217).
 * edc_cached_quorum_verify  edc_quorum_verify through the table (src/batch.rs:76-94, :104-107,
 *   :127-137, :149-217).
 * edc_cached_tmpl_quorum_verify_device  edc_tmpl_quorum_verify_device through the table
 *   (src/batch.rs:76-94, :104-107, :127-137, :149-217): SHA-512 runs over the n_checked gathered
 *   votes, the batch over the n_miss of them that are no records.
 * edc_cached_tmpl_quorum_verify  edc_tmpl_quorum_verify through the table (src/batch.rs:76-94,
 *   :104-107, :127-137, :149-217).
 * edc_debug_cached_quorum_last  test hook, a host copy (no device work): out = {n, n_checked, the
 *   hits among the checked, n_miss, the items SHA-512 ran over, the records the call inserted} of
 *   the last cached quorum call on the context that reached its selection. EDC_ERR_ARG before any
 *   such call and for NULL.
 * Not built: asynchronous submit / wait forms, the incremental verifier and the multi-GPU engine
 *   have no cached quorum entries.
 */
int edc_cached_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                    const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off,
                                    const uint8_t* d_k, const uint64_t* d_power, const uint8_t* d_flag,
                                    const uint64_t* threshold, int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts,
                                    uint8_t* item_verdicts, uint64_t* tally, int* n_bad_commits, size_t* n_checked,
                                    size_t* n_miss, uint8_t check8[32]);
int edc_cached_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                             const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                             const uint8_t* k, const uint64_t* power, const uint8_t* flag, const uint64_t* threshold,
                             int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                             uint64_t* tally, int* n_bad_commits, size_t* n_checked, size_t* n_miss, uint8_t check8[32]);
int edc_cached_tmpl_quorum_verify_device(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                         const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* d_item_alt,
                                         const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_var,
                                         const uint32_t* d_var_off, size_t var_bytes, const uint64_t* d_power,
                                         const uint8_t* d_flag, const uint64_t* threshold, int mode,
                                         const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                                         uint64_t* tally, int* n_bad_commits, size_t* n_checked, size_t* n_miss,
                                         uint8_t check8[32]);
int edc_cached_tmpl_quorum_verify(edc_ctx* ctx, const edc_templates* ts, size_t nc, const uint32_t* commit_off,
                                  const uint16_t* commit_tpl, uint32_t alt_span, const uint8_t* item_alt, const uint8_t* vk,
                                  const uint32_t* key_idx, const uint8_t* sig, const uint8_t* var, const uint32_t* var_off,
                                  const uint64_t* power, const uint8_t* flag, const uint64_t* threshold, int mode,
                                  const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                                  uint64_t* tally, int* n_bad_commits, size_t* n_checked, size_t* n_miss,
                                  uint8_t check8[32]);
int edc_debug_cached_quorum_last(const edc_ctx* ctx, uint64_t out[6]);

/*
 * Validator-set quorum commit sets: powers and double votes resolved on the GPU. The quorum entries
 * take a power and a flag per vote, which the caller has to work out before every call: for
 * VerifyCommit a copy of the set's powers, for VerifyCommitLightTrusting a join of every signer's
 * key against the trusted set ("EDC_VOTE_ABSENT for the signers that set does not know") and, in
 * the same loop, CometBFT's check that no validator of the trusted set is seen twice in one commit
 * (named here from memory, as the calls above are, and not checked against a source tree). These
 * entries keep the powers with the registered key list and do the join and that check on the
 * device. The reference crate has no such API and none of its APIs changes meaning: every vote
 * that is checked is one batch::Item (src/batch.rs:76-94) in ONE batch::Verifier (queue + verify,
 * src/batch.rs:127-137, :149-217), and its code is Item::verify_single's (src/batch.rs:104-107).
 *
 * edc_valset_set_powers  power[p] (uint64_t, m entries, host) is the voting power of position p of
 *   the list last given to edc_keycache_load; the keys of that list are from then on the MEMBERS of
 *   the validator set. EDC_ERR_ARG with nothing changed if m differs from that list's length, if
 *   there is no list, if two positions of the list hold the same key (a validator set has distinct
 *   keys), if a power is above 2^63 - 1 or if the powers sum to more than 2^63 - 1; refused while
 *   batches are in flight, as edc_keycache_load is. The powers live on the device, indexed by cache
 *   index, beside a member byte and the inverse map from cache index to position.
 *   edc_keycache_load and edc_keycache_clear drop them; edc_keycache_add keeps them, and a key it
 *   adds is not a member. m = 0 with a NULL power clears them.
 * edc_valset_size  the member count; 0 when no powers are set (and for NULL).
 *
 * The join. Item i's signer is given by its key bytes or, in the host forms, by its position
 * key_idx[i] in the registered list. With the powers set,
 *   pos[i]       the registered position of the signer, 0xFFFFFFFF when its key is not a member;
 *   power[i]     the member's power, 0 for anyone else;
 *   flag_out[i]  flag[i] for a member, EDC_VOTE_ABSENT for anyone else.
 * checked[i], planned[c] and *n_checked are exactly edc_quorum_plan's for (power, flag_out) with the
 * same offsets, thresholds and mode.
 * Double-vote rule. dv[c] = 1 iff two CHECKED items of commit c resolve to the same member. It is
 *   the loop's own rule: in light mode a second vote that arrives after the quorum is not checked
 *   and raises nothing, one that is checked does; in full mode every signed vote is checked, and a
 *   commit vote and a nil vote from one validator are a double vote too. The same validator in two
 *   different commits is none, and two non-members never are.
 * edc_valset_resolve  the join, the selection and the double-vote scan alone, on host arrays (no
 *   signatures): exactly one of vk (n x 32) and key_idx; outputs pos (uint32_t, n), power (n),
 *   flag_out (n), checked (n bytes, 0 / 1), planned (nc), *n_checked and dv (nc bytes), all
 *   nullable. It is to these entries what edc_quorum_plan is to the quorum entries and runs the
 *   kernels they run.
 *
 * edc_valset_quorum_verify_device / edc_valset_quorum_verify  the arguments of
 *   edc_quorum_verify_device / edc_quorum_verify without d_power / power. Inputs and outputs keep
 *   their meaning, with three changes:
 *   - item i's power and flag are the joined power[i] and flag_out[i]. A non-member's vk, sig and
 *     message bytes are never interpreted and its code is EDC_NOT_CHECKED (without d_k its message
 *     is hashed with every other and must be mapped like any other);
 *   - a commit with dv[c] = 1 has the verdict EDC_DOUBLE_VOTE whatever else holds for it. Its
 *     checked items are still verified and still get their codes, so the gathered list does not
 *     depend on dv; its tally is the sum as defined and carries no meaning;
 *   - the return value is EDC_OK iff every commit is EDC_OK; else EDC_INVALID_SIGNATURE if any
 *     commit is EDC_INVALID_SIGNATURE; else EDC_DOUBLE_VOTE if any commit is EDC_DOUBLE_VOTE; else
 *     EDC_QUORUM_SHORT. *n_bad_commits counts every commit that is not EDC_OK.
 * Equality contract. On a set with no double vote every output, check8 included, equals what
 *   edc_quorum_verify[_device] gives for the same keys, z_seed, thresholds and mode when it is
 *   handed the joined power / flag_out. With double votes every output except the verdicts of those
 *   commits, *n_bad_commits and the return value still equals it.
 * Stream synchronizations. The join runs before the selection, the double-vote scan behind it on
 *   its skip bytes and commit indices, and dv travels in the selection's one read-back:
 *   edc_valset_quorum_verify_device adds no stream synchronization to what edc_quorum_verify_device
 *   has. The scan's workspace is 16 bytes per item and a byte per commit, grow-only.
 * Argument checks. The host checks the offsets, the mode, the one-of pairs, that the key indices
 *   lie inside the registered list and that powers are set (without powers: EDC_ERR_ARG). The device
 *   checks a flag above 2, for members and non-members alike, and the bound on a commit's counted
 *   sum: duplicates can push one commit past 2^63 - 1, which is EDC_ERR_ARG for the call. Both forms
 *   rely on the device for these, because the powers exist only there. On a violation nothing is
 *   gathered, no output is written, no index outside the declared arrays is formed and the context
 *   stays usable. A host form's prehashed k must be canonical for the checked items only. nc = 0
 *   returns EDC_OK (no array is read); a NULL ctx or z_seed is EDC_ERR_ARG. The calls are synchronous
 *   on slot 0 (EDC_ERR_ARG while a submitted batch is pending there). The key_idx host form
 *   resolves by position, with no hash lookup, and stages 4 + 64 + 1 bytes per vote plus k or the
 *   message.
 * edc_debug_valset_select  measurement hook: on host arrays checked as edc_valset_resolve, the join
 *   kernel and the double-vote scan (with the clearing of its workspace) alone, each run `reps`
 *   times between HIP events; ms (nullable) = {the join's mean time, the scan's}.
 * Not built: asynchronous submit / wait, incremental-verifier and multi-GPU forms. The templated and
 *   cached forms are built as requests (edc_vq_verify, below), not as further forms of these entries.
 */
#define EDC_DOUBLE_VOTE 4            /* two checked votes of one commit from the same member */
int edc_valset_set_powers(edc_ctx* ctx, size_t m, const uint64_t* power);
int edc_valset_size(const edc_ctx* ctx);
int edc_valset_resolve(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk, const uint32_t* key_idx,
                       const uint8_t* flag, const uint64_t* threshold, int mode, uint32_t* pos, uint64_t* power,
                       uint8_t* flag_out, uint8_t* checked, uint64_t* planned, size_t* n_checked, uint8_t* dv);
int edc_valset_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* d_vk,
                                    const uint8_t* d_sig, const uint8_t* d_msg, const uint64_t* d_msg_off,
                                    const uint8_t* d_k, const uint8_t* d_flag, const uint64_t* threshold, int mode,
                                    const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                                    uint64_t* tally, int* n_bad_commits, size_t* n_checked, uint8_t check8[32]);
int edc_valset_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                             const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                             const uint8_t* k, const uint8_t* flag, const uint64_t* threshold, int mode,
                             const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts, uint64_t* tally,
                             int* n_bad_commits, size_t* n_checked, uint8_t check8[32]);
int edc_debug_valset_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint8_t* vk,
                            const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold, int mode, int reps,
                            float ms[2]);

/*
 * Validator-set history: every commit judged by the set of its own height. edc_valset_set_powers
 * holds one set, and a call judges every commit against it; on a chain the set moves with almost
 * every block (CometBFT's validator updates, named from memory as above), and a commit set that
 * spans many heights would have to be cut at every change. These entries keep the HISTORY of the
 * set with the registered key list: a base set plus per-version updates. Every commit names the
 * version it is judged by, and the device resolves each vote's membership and power at that
 * version. Selection, double-vote scan, gather, batch and tally are the validator-set entries' own
 * and run behind the join unchanged; the reference crate's APIs keep their meaning as stated there.
 *
 * Versions. Positions are those of the list last given to edc_keycache_load, which is the union of
 *   every key that is a member at any version. Version 0 is base_power[p] for p < m. Version v
 *   (1..nv) is version v-1 with the updates [upd_off[v-1], upd_off[v]) applied: position upd_pos[j]
 *   gets the power upd_power[j]. EDC_VHIST_NOT_MEMBER, in the base or in an update, means the
 *   position is not a member from that version on, until a later update gives it a power. A power
 *   of 0 is a member without weight: its flag counts and it can double-vote. An update that
 *   restates the current state is allowed and changes no version's set (it is one more entry in
 *   that position's change list).
 * edc_vhist_set  sets the history (m base powers; nv versions of updates: upd_off has nv + 1
 *   entries, upd_pos / upd_power upd_off[nv]; all host). It is independent of
 *   edc_valset_set_powers: both may be set, and the edc_valset_* entries never read the history.
 *   edc_keycache_load and edc_keycache_clear drop it; edc_keycache_add keeps it, and a key it adds
 *   is not a member at any version. m = 0 with NULL arrays clears it. Refused while batches are in
 *   flight, as edc_valset_set_powers is. EDC_ERR_ARG with nothing changed if m differs from the
 *   registered list's length or there is no list, if a key occurs twice in the list, if upd_off is
 *   not monotone from 0, if an update position is >= m, if a position occurs twice inside one
 *   version's slice, if a power other than the sentinel is above 2^63 - 1, if the member powers of
 *   any version sum to more than 2^63 - 1, or if m plus the update count reaches 2^32. On the
 *   device the history is one change list per key in CSR form, indexed by cache index: 32-bit
 *   versions (ascending, the base as version 0) and, apart from them, 64-bit powers; 12 bytes per
 *   position and per update.
 * edc_vhist_versions  nv + 1; 0 when no history is set (and for NULL).
 * edc_vhist_totals  for the versions v0 .. v0 + count - 1: total[j] = the sum of the member powers,
 *   members[j] = the member count (both nullable) -- what a caller derives thresholds from
 *   (floor(2T/3), or floor(T/3) for the trusting check). Computed on the host when the history is
 *   set. A range outside the history is EDC_ERR_ARG.
 *
 * The join. With c the commit of item i and v = commit_ver[c] (uint32_t, nc entries, host):
 *   pos[i]       the signer's registered position if it is a member at version v, else 0xFFFFFFFF;
 *   power[i]     its power at v, else 0;
 *   flag_out[i]  flag[i] for a member at v, else EDC_VOTE_ABSENT.
 *   A flag above 2 is passed through whoever signed, so that the selection's check raises it.
 *   commit_ver[c] > nv is EDC_ERR_ARG, checked on the host; versions may repeat and come in any
 *   order across commits. checked, planned and *n_checked are edc_quorum_plan's on
 *   (power, flag_out); dv[c] is the double-vote rule above over the members of commit c's version.
 * edc_vhist_resolve  edc_valset_resolve with the history's join.
 * edc_vhist_quorum_verify_device / edc_vhist_quorum_verify  the arguments of
 *   edc_valset_quorum_verify_device / edc_valset_quorum_verify with commit_ver after commit_off.
 *   Verdicts, the order of the return value (1 over 4 over 3), argument checks (a missing history
 *   where those name missing powers), the canonical-k rule of the host form and the stream
 *   synchronizations are theirs: the offsets and versions are copied to the device in front of the
 *   join kernel, and no stream synchronization is added.
 * Equality contract. Apart from the verdicts of double-vote commits, *n_bad_commits and the return
 *   value, every output, check8 included, equals what edc_quorum_verify[_device] gives when handed
 *   the joined power / flag_out. With nv = 0 and no sentinel in the base every output, the
 *   EDC_DOUBLE_VOTE verdicts included, equals what edc_valset_quorum_verify[_device] gives after
 *   edc_valset_set_powers(base_power).
 * edc_debug_vhist_select  edc_debug_valset_select with the history's join kernel in ms[0].
 * Not built: asynchronous submit / wait, incremental-verifier and multi-GPU forms. The templated and
 *   cached forms are built as requests (edc_vq_verify, below), not as further forms of these entries.
 */
#define EDC_VHIST_NOT_MEMBER 0xFFFFFFFFFFFFFFFFull
int edc_vhist_set(edc_ctx* ctx, size_t m, const uint64_t* base_power, size_t nv, const uint32_t* upd_off,
                  const uint32_t* upd_pos, const uint64_t* upd_power);
int edc_vhist_versions(const edc_ctx* ctx);
int edc_vhist_totals(const edc_ctx* ctx, uint32_t v0, size_t count, uint64_t* total, uint32_t* members);
int edc_vhist_resolve(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver, const uint8_t* vk,
                      const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold, int mode, uint32_t* pos,
                      uint64_t* power, uint8_t* flag_out, uint8_t* checked, uint64_t* planned, size_t* n_checked,
                      uint8_t* dv);
int edc_vhist_quorum_verify_device(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                                   const uint8_t* d_vk, const uint8_t* d_sig, const uint8_t* d_msg,
                                   const uint64_t* d_msg_off, const uint8_t* d_k, const uint8_t* d_flag,
                                   const uint64_t* threshold, int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts,
                                   uint8_t* item_verdicts, uint64_t* tally, int* n_bad_commits, size_t* n_checked,
                                   uint8_t check8[32]);
int edc_vhist_quorum_verify(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                            const uint8_t* vk, const uint32_t* key_idx, const uint8_t* sig, const uint8_t* msg,
                            const uint64_t* msg_off, const uint8_t* k, const uint8_t* flag, const uint64_t* threshold,
                            int mode, const uint8_t z_seed[32], uint8_t* commit_verdicts, uint8_t* item_verdicts,
                            uint64_t* tally, int* n_bad_commits, size_t* n_checked, uint8_t check8[32]);
int edc_debug_vhist_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                           const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag, const uint64_t* threshold,
                           int mode, int reps, float ms[2]);

/*
 * Validator-set requests: the validator-set and history entries above, the templated forms and the
 * verified-signature table behind ONE entry that takes a request structure. The matrix
 * {one set, history} x {messages, k, templates} x {plain, cached} x {host, device} is closed here;
 * no flat entry is added for it. The reference crate's APIs keep their meaning: every vote that is
 * verified is one batch::Item (src/batch.rs:76-94) in ONE batch::Verifier (src/batch.rs:127-137,
 * :149-217), and its code is Item::verify_single's (src/batch.rs:104-107).
 *
 * Both structures begin with `size`, the caller's sizeof of the structure, so that fields can be
 * appended later; a value that is neither today's sizeof nor the sizeof before the trusting pair's
 * fields were appended (the structure up to and without trust_ver / trust_verdicts) is EDC_ERR_ARG.
 * With the earlier sizeof the appended fields read as NULL. Reserved fields must be 0.
 *
 * edc_vq_request
 *   device      0: the per-item arrays (vk / key_idx, sig, flag, msg, msg_off, k, item_alt, var,
 *               var_off) are host memory. 1: they are in this GPU's memory under the rules of the
 *               *_device entries (vk / sig / k 16-byte aligned, var_off 4-byte aligned, msg_off
 *               8-byte aligned; item_alt and var need no alignment). commit_off, commit_ver,
 *               threshold, commit_tpl and the template set are host memory in both forms.
 *   nc, commit_off, threshold, mode, z_seed   as edc_quorum_verify.
 *   commit_ver  NULL: every commit is judged by the one set of edc_valset_set_powers. Non-NULL
 *               (nc entries): by the history of edc_vhist_set, as edc_vhist_quorum_verify.
 *   vk, key_idx exactly one; key_idx (positions in the registered list) in the host form only.
 *   sig, flag   n x 64 bytes; one flag byte per vote, as edc_valset_quorum_verify.
 *   messages    exactly one of: msg_off (n + 1 offsets into msg, which may be NULL when every
 *               message is empty); k (n x 32, prehashed); ts (a template set) with commit_tpl,
 *               alt_span, item_alt, var, var_off and, in the device form, var_bytes, which mean
 *               exactly what they mean for edc_tmpl_quorum_verify[_device] (the host form takes
 *               var_off[n] for var_bytes). Fields of a group that is not used must be NULL / 0.
 *   cached      non-zero: the call runs through the context's verified-signature table.
 * edc_vq_result  commit_verdicts (nc), item_verdicts (n), tally (nc), n_bad_commits, n_checked,
 *   n_miss, check8 (32 bytes): all nullable, with the meaning they have for the entries above.
 *   n_miss is written only when `cached`.
 *
 * Contract, every clause an equality against an entry above.
 *   Join, selection, double votes: the checked bytes, planned[], dv[], pos, power and flag_out are
 *     edc_valset_resolve's (edc_vhist_resolve's with commit_ver) for the same inputs, whatever the
 *     message form and whatever the table holds: a hit still counts towards light mode's running
 *     sum and still is a checked vote for the double-vote rule, whose scan runs on the selection's
 *     skip bytes before any lookup.
 *   No templates, not cached: every output equals edc_valset_quorum_verify[_device] /
 *     edc_vhist_quorum_verify[_device] on the same inputs.
 *   Templated: every output equals the same request with (msg, msg_off) holding the materialised
 *     messages head[t] || hole || tail[t]. Select first, as edc_tmpl_quorum_*: only the checked
 *     votes are gathered, assembled and hashed, and the arena is sized from n_checked. The all-n
 *     checks of item_alt and the hole offsets apply to members and non-members alike; a
 *     non-member's key, signature and hole bytes are never interpreted. No stream synchronization
 *     is added to edc_tmpl_quorum_verify_device's; dv travels in the selection's one read-back.
 *   Cached: hit, miss list, inserts, statistics and errors are those of "Cached quorum commit
 *     sets", applied to the joined power / flag_out. Apart from the verdicts of double-vote
 *     commits, *n_bad_commits and the return value, every output equals
 *     edc_cached_quorum_verify[_device] (with templates edc_cached_tmpl_quorum_verify[_device])
 *     handed those joined arrays. A commit with dv[c] = 1 is EDC_DOUBLE_VOTE whatever else holds;
 *     its checked misses are still verified, and inserted if valid. The plain cached form adds no
 *     synchronization; the templated one keeps the existing second read-back and nothing more.
 *   Return value: EDC_OK iff every commit is EDC_OK; else 1 over 4 over 3, as edc_valset_*.
 * Keys by position. With key_idx the join resolves by position, with no hash lookup, and 4 bytes per
 *   key cross PCIe; the n keys are then expanded on the device from the registered list, as in every
 *   other host form. Gathers that take only the kept votes' keys by position were built and measured
 *   level with this, so the simpler path stands ("Validator-set requests").
 * Errors: the union of what the composed entries check, on the host for host forms and on the
 *   device for device forms (flags above 2, a commit's counted power, item_alt, hole offsets).
 *   Further: a wrong `size`, a non-zero reserved field, both or neither of a one-of group, key_idx
 *   with device = 1, `cached` without a table, commit_ver without a history, no commit_ver without
 *   powers. A violation returns EDC_ERR_ARG with no verdict, nothing inserted, no counter changed
 *   and no index formed outside the declared arrays; the context stays usable. nc = 0 returns
 *   EDC_OK with no array read (after the checks that read no array). Synchronous on slot 0, refused
 *   while a batch is pending there.
 * edc_debug_vq_last  test hook, a host copy (no device work): out = {n, n_checked, hits, n_miss,
 *   items SHA-512 ran over, records inserted, 0 (reserved), arena bytes} of the last request that
 *   returned a verdict; EDC_ERR_ARG before any. For a trusting pair n_checked is the union's.
 *
 * Trusting pairs: one commit judged by two sets at once. A light client that skips from a trusted
 * height H to a later height H' asks two questions of the commit of H' (CometBFT's non-adjacent
 * verification, named from memory): do the signers that the trusted set of H knows carry more than
 * 1/3 of that set's power, and do the signers carry more than 2/3 of the commit's own set. A
 * request answers both in one call and verifies every vote once.
 *   trust_ver        (uint32_t, nc entries, host) NULL: no trusting side, the request runs exactly as
 *                    described above. Needs commit_ver. Entry c is a version <= nv of the history, or
 *                    EDC_VQ_NO_TRUST, which gives commit c side A only (an adjacent hop).
 *   trust_threshold  (uint64_t, nc entries, host) given iff trust_ver is.
 *   trust_verdicts (nc), trust_tally (nc), n_bad_trust  side B's commit_verdicts, tally and
 *                    *n_bad_commits; nullable, not written when trust_ver is NULL.
 * Let A be the same request without the trust fields and B the same request with
 * commit_ver := trust_ver and threshold := trust_threshold; `mode` is shared.
 *   Selection: side A's pos, power, flag_out, checked bytes, planned and dv are edc_vhist_resolve's
 *     for A, side B's are edc_vhist_resolve's for B. A vote is verified iff either side checks it,
 *     and *n_checked is the size of that union (in full mode: every signed vote of a member of
 *     either set).
 *   Verdicts: commit_verdicts, tally and *n_bad_commits equal request A's; trust_verdicts,
 *     trust_tally and *n_bad_trust equal request B's. Each side's OR of codes, tally and
 *     double-vote rule run over that side's checked votes and that side's members only, also when
 *     the union batch fails: item codes are Item::verify_single's and depend on nothing else.
 *   item_verdicts[i] is the code of vote i if either side checks it, else EDC_NOT_CHECKED; it equals
 *     A's where A checks the vote and B's where B does.
 *   check8, the verdict path and the z indices are bit-identical to
 *     edc_batch_verify_prehashed_device on the union list in queue order with z_base = 0.
 *   A commit whose trust_ver[c] is EDC_VQ_NO_TRUST: B checks none of its votes,
 *     trust_verdicts[c] = EDC_OK, trust_tally[c] = 0, and it raises no B-side double vote.
 *   Return value: EDC_OK iff every verdict of both arrays is EDC_OK; else 1 over 4 over 3, taken
 *     over both arrays.
 *   Templated: only the union is gathered, assembled and hashed, the arena is sized from the union
 *     count, and every output equals the paired request on the materialised messages.
 *   Cached: the lookup runs on the union, and a hit counts as verified for both sides. n_miss is the
 *     number of union votes that are no live record; valid misses are inserted; commit-level outputs
 *     equal the uncached paired request's. The selection and both double-vote scans never look at
 *     the table.
 *   No stream synchronization is added: both sides' double-vote bytes and the union's totals ride in
 *     the selection's one read-back, both planned arrays in the copy that brings side A's, and the
 *     cached templated form keeps its existing second read-back and nothing more.
 *   Errors (EDC_ERR_ARG): trust_ver without commit_ver; trust_ver without trust_threshold or the
 *     reverse; trust_ver[c] > nv other than the sentinel. The device checks of flags and of a
 *     commit's counted power apply to each side (duplicates can push either past 2^63 - 1). On any
 *     violation nothing is gathered, written, inserted or counted, and the context stays usable.
 * edc_vq_trust_resolve  edc_vhist_resolve with trust_ver and trust_threshold: the paired join, both
 *   selections, the union and both double-vote scans as the request runs them, on host keys and
 *   flags without signatures. pos .. dv are side A's, trust_pos .. trust_dv side B's, side[i] =
 *   bit 0 checked by A | bit 1 checked by B, *n_checked the union's size. All outputs nullable.
 * edc_debug_vq_trust_last  test hook, a host copy: out = {checked by A, checked by B, checked by
 *   both, union} of the last paired request that returned a verdict; EDC_ERR_ARG before any. Every
 *   paired request pays for these totals: the union kernel adds them per tile (three integer
 *   atomics spread over 64 slots), and 768 bytes come back in the selection's read-back.
 * edc_debug_vq_trust_select  mean milliseconds over reps runs: ms[0] the paired join, ms[1] both
 *   selections with the union and the scan of its tile counts, ms[2] both double-vote scans.
 */
#define EDC_VQ_NO_TRUST 0xFFFFFFFFu
typedef struct edc_vq_request {
  uint32_t size;               /* sizeof(edc_vq_request) */
  uint32_t device;
  int32_t mode;                /* EDC_QUORUM_FULL / EDC_QUORUM_LIGHT */
  uint32_t cached;
  uint32_t alt_span;
  uint32_t reserved;
  size_t nc;
  const uint32_t* commit_off;
  const uint32_t* commit_ver;
  const uint64_t* threshold;
  const uint8_t* z_seed;
  const uint8_t* vk;
  const uint32_t* key_idx;
  const uint8_t* sig;
  const uint8_t* flag;
  const uint8_t* msg;
  const uint64_t* msg_off;
  const uint8_t* k;
  const edc_templates* ts;
  const uint16_t* commit_tpl;
  const uint8_t* item_alt;
  const uint8_t* var;
  const uint32_t* var_off;
  size_t var_bytes;
  const uint32_t* trust_ver;
  const uint64_t* trust_threshold;
} edc_vq_request;
typedef struct edc_vq_result {
  uint32_t size;               /* sizeof(edc_vq_result) */
  uint32_t reserved;
  uint8_t* commit_verdicts;
  uint8_t* item_verdicts;
  uint64_t* tally;
  int* n_bad_commits;
  size_t* n_checked;
  size_t* n_miss;
  uint8_t* check8;
  uint8_t* trust_verdicts;
  uint64_t* trust_tally;
  int* n_bad_trust;
} edc_vq_result;
int edc_vq_verify(edc_ctx* ctx, const edc_vq_request* rq, edc_vq_result* rs);
int edc_debug_vq_last(const edc_ctx* ctx, uint64_t out[8]);
int edc_vq_trust_resolve(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                         const uint32_t* trust_ver, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag,
                         const uint64_t* threshold, const uint64_t* trust_threshold, int mode, uint32_t* pos, uint64_t* power,
                         uint8_t* flag_out, uint8_t* checked, uint64_t* planned, uint8_t* dv, uint32_t* trust_pos,
                         uint64_t* trust_power, uint8_t* trust_flag_out, uint8_t* trust_checked, uint64_t* trust_planned,
                         uint8_t* trust_dv, uint8_t* side, size_t* n_checked);
int edc_debug_vq_trust_last(const edc_ctx* ctx, uint64_t out[4]);
int edc_debug_vq_trust_select(edc_ctx* ctx, size_t nc, const uint32_t* commit_off, const uint32_t* commit_ver,
                              const uint32_t* trust_ver, const uint8_t* vk, const uint32_t* key_idx, const uint8_t* flag,
                              const uint64_t* threshold, const uint64_t* trust_threshold, int mode, int reps, float ms[3]);

/*
 * Validator-set hashes: the Merkle root of a validator set, of every version of the history on the
 * GPU. The quorum entries above judge a commit BY a set; a light client gets that set from an
 * untrusted provider, and before it may judge by it, it must check that the set hashes to the
 * validators_hash of the header it trusts. These entries compute that hash where the sets already
 * live, and only 32 bytes per version (or one byte per commit) cross PCIe. Not an API of the
 * reference crate, whose APIs keep their meaning as stated there.
 *
 * The function. The library's contract is these bytes. Agreement with CometBFT's
 * ValidatorSet.Hash() is the intent, but it is stated from memory, as the sections above are, and
 * no chain data was at hand to check it against. For a set S of members (position p of the
 * registered list, its 32-byte key key_p, its power w_p <= 2^63 - 1):
 *   Address  addr_p = the first 20 bytes of SHA-256(key_p).
 *   Order    The members are ordered by power descending, then addr ascending as byte strings. A tie
 *            on both is broken by position ascending (the history and the one set reject a list
 *            that holds a key twice, so this needs a 160-bit collision).
 *   Leaf     leaf_p = 0A 22 0A 20 | key_p | (10 | uvarint(w_p) if w_p > 0, else nothing). The
 *            uvarint is base-128, little-endian, 1 to 9 bytes. A leaf is 36 to 46 bytes, so with the
 *            00 prefix it is always one SHA-256 block. A member of power 0 ("a member without
 *            weight") omits the field, as proto3 does.
 *   Root     RFC 6962's MTH with SHA-256 over the ordered leaves: the empty set -> SHA-256 of the
 *            empty string; one leaf -> SHA-256(00 | leaf); n > 1 -> SHA-256(01 | MTH(first k) |
 *            MTH(rest)), with k the largest power of two below n.
 *   Members  The members of version v are the positions whose power at v is not
 *            EDC_VHIST_NOT_MEMBER. The one-set form takes the members of edc_valset_set_powers
 *            exactly as the edc_valset_* join defines them.
 * Member cap. One workgroup sorts and hashes one set in LDS, so a set holds at most
 *   EDC_VALHASH_MAX_MEMBERS = 4096 members (28 bytes of LDS per padded slot, 112 KB of the CU's
 *   160 KB). A call that asks for a version above the cap is EDC_ERR_ARG, with nothing
 *   written. Larger sets are not built.
 *
 * edc_valhash_valset  out = the root of the one set of edc_valset_set_powers.
 * edc_valhash_vhist  out (count x 32 host bytes) = the roots of the versions v0 .. v0 + count - 1.
 *   The range rules are edc_vhist_totals': v0 > nv + 1 or count > nv + 1 - v0 is EDC_ERR_ARG.
 * edc_valhash_vhist_match  expect (nc x 32 host bytes) holds the validators_hash of each commit's
 *   header: ok[c] = 1 iff the root of version commit_ver[c] equals the 32 bytes at expect + 32 c,
 *   else 0; *n_mismatch (nullable) = the number of zeros. Versions may repeat and come in any
 *   order; each distinct version is hashed once. The compare runs on the device and nc bytes come
 *   back. commit_ver[c] > nv is EDC_ERR_ARG, checked on the host. The return value is EDC_OK
 *   whether or not everything matches: a mismatch is data.
 * Errors of all three: EDC_ERR_ARG with nothing written and the context usable when there is no
 *   registered key list, no history (edc_valhash_valset: no powers), or a required output or input is
 *   NULL. With those in place count = 0 and nc = 0 return EDC_OK, read no array and write only
 *   *n_mismatch = 0. Synchronous on slot 0 and refused while a batch is pending there.
 * What is kept. The address order does not depend on the version: the first call after a key list
 *   is loaded hashes every key on the device and ranks the addresses once; edc_keycache_load,
 *   edc_keycache_clear and clearing the history drop the ranks, edc_keycache_add keeps them (a key
 *   it adds is a member of no version). No root is kept between calls: every call hashes what it is
 *   asked for from the history as it stands.
 * edc_debug_valhash_ms  measurement hook: mean times over reps launches of the root kernel over
 *   every version of the history (ms[0]) and of the address kernel over the list (ms[1]).
 * Not built: sets above the cap (a multi-workgroup sort), asynchronous, incremental and multi-GPU
 *   forms, device-resident outputs.
 */
#define EDC_VALHASH_MAX_MEMBERS 4096
int edc_valhash_valset(edc_ctx* ctx, uint8_t out[32]);
int edc_valhash_vhist(edc_ctx* ctx, uint32_t v0, size_t count, uint8_t* out);
int edc_valhash_vhist_match(edc_ctx* ctx, size_t nc, const uint32_t* commit_ver, const uint8_t* expect, uint8_t* ok,
                         size_t* n_mismatch);
int edc_debug_valhash_ms(edc_ctx* ctx, int reps, float ms[2]);

/*
 * Header hashes: the Merkle root of many block headers at once, bound to validator-set roots and
 * to each other. The set hashes above give the root a light client compares with the
 * validators_hash of the header it trusts; these entries hash the header itself, so that nothing
 * between a vote and the set it is judged by is taken on faith: the expected bytes of
 * edc_valhash_vhist_match come out of a header whose own hash is checked, the block id the votes
 * sign is that hash, and the walk backwards from a trusted header to older ones (header h carries
 * the hash of header h - 1 in its last_block_id) is a chain of such hashes. Not an API of the
 * reference crate, whose APIs keep their meaning as stated there.
 *
 * The function. The library's contract is these bytes. Agreement with CometBFT's Header.Hash() is
 * the intent, but it is stated from memory, as the sections above are, and no chain data was at hand
 * to check it against. The library parses no protobuf: a header is given as its ordered LEAVES,
 * opaque byte strings of any length, 0 included (for CometBFT the 14 encoded fields). The hash of a
 * header of n leaves is RFC 6962's MTH with SHA-256 over them: no leaf -> SHA-256 of the empty
 * string; one leaf -> SHA-256(00 | leaf); n > 1 -> SHA-256(01 | MTH(first k) | MTH(rest)), with k
 * the largest power of two below n. A leaf hash takes one SHA-256 block up to 54 bytes, two up to
 * 118, three up to 182, and so on. A header holds at most EDC_HEADER_MAX_LEAVES = 64 leaves (one
 * lane per leaf, one header inside one wave).
 *
 * edc_header_set  nh headers in host memory: header h owns the leaves leaf_off[h] .. leaf_off[h + 1]
 *   - 1, leaf j is bytes[byte_off[j] .. byte_off[j + 1]). Both offset arrays start at 0 and are
 *   monotone; leaves are packed in any way the offsets allow (back to back, at any byte alignment).
 *   bytes may be NULL when byte_off[last] = 0. byte_off[last] < 2^32 - 1024.
 * edc_header_hashes  out (nh x 32 host bytes) = the hash of every header. Needs no key list and no
 *   history.
 * edc_header_bind  hashes every header and answers up to four questions per header; bad[h] is the
 *   OR of the bits of the questions whose answer is no, 0 for a header every rule accepts;
 *   *n_bad (nullable) = the number of non-zero bytes; out (nullable) = the hashes, as
 *   edc_header_hashes gives them.
 *     expect     EDC_HEADER_BAD_HASH iff the header's hash differs from the 32 bytes at expect + 32 h.
 *     byte rule  (leaf L, position P, source root S): holds iff L < n, leaf L has at least P + 32
 *                bytes, and the 32 bytes from position P equal S. Otherwise the rule's bit is set.
 *     vals_ver   S = the root of history version vals_ver[h], exactly as edc_valhash_vhist returns
 *                it, at (vals_leaf, vals_pos): EDC_HEADER_BAD_VALS.
 *     next_ver   the same at (next_leaf, next_pos): EDC_HEADER_BAD_NEXT.
 *     link       S = this call's own hash of header link[h] of THIS SET, at (link_leaf, link_pos):
 *                EDC_HEADER_BAD_LINK. Links may point forwards or backwards in the array, may
 *                repeat, and may name the header itself.
 *   A rule whose array is NULL sets no bit, and an entry EDC_HEADER_NONE skips its header. For
 *   CometBFT the caller passes leaves 7 (validators_hash) and 8 (next_validators_hash) at position
 *   2, behind the bytes 0A 20, and for the link leaf 4 (last_block_id) at position 2. Each distinct
 *   version named by vals_ver or next_ver is hashed once, by the root kernel of the set hashes. The
 *   return value is EDC_OK whether or not every rule holds: a mismatch is data.
 * Errors: EDC_ERR_ARG with nothing written and the context usable for a wrong size or a non-zero
 *   reserved in either structure; a NULL ctx, hs or r, or a NULL required output (out of
 *   edc_header_hashes, bad); a NULL offset array, offsets that do not start at 0 or are not
 *   monotone, NULL bytes with byte_off[last] > 0, byte_off[last] >= 2^32 - 1024 or nh >= 2^32; a header
 *   above EDC_HEADER_MAX_LEAVES leaves; a version above the history's last other than the
 *   sentinel; a non-NULL vals_ver or next_ver without a registered key list and a history
 *   (edc_keycache_load, edc_vhist_set), even when every entry is the sentinel; a named version above
 *   EDC_VALHASH_MAX_MEMBERS members; a link[h] >= nh other than the sentinel. nh = 0 returns EDC_OK,
 *   reads no array and writes only *n_bad = 0. Synchronous on slot 0 and refused while a batch is
 *   pending there.
 * edc_debug_header_ms  measurement hook: mean times over reps launches of the root kernel over hs
 *   (ms[0]) and of the bind kernel (ms[1]) with all four compares per header, each against the
 *   header's own hash (expect, and leaves 7, 8 and 4 at position 2), so it needs no history.
 * Not built: device-resident inputs or outputs; asynchronous and multi-GPU forms; headers above 64
 *   leaves; parsing protobuf in the library; reading the block id out of a template head (the
 *   caller builds the heads from the same commit it passes as expect).
 */
#define EDC_HEADER_MAX_LEAVES 64
#define EDC_HEADER_NONE 0xFFFFFFFFu
#define EDC_HEADER_BAD_HASH 1   /* root != expect                                   */
#define EDC_HEADER_BAD_VALS 2   /* 32 bytes at (vals_leaf, vals_pos) != set root     */
#define EDC_HEADER_BAD_NEXT 4   /* 32 bytes at (next_leaf, next_pos) != next root    */
#define EDC_HEADER_BAD_LINK 8   /* 32 bytes at (link_leaf, link_pos) != linked root  */

typedef struct edc_header_set {
  uint32_t size;             /* sizeof(edc_header_set); anything else: EDC_ERR_ARG */
  uint32_t reserved;         /* 0 */
  size_t nh;                 /* headers */
  const uint32_t* leaf_off;  /* nh + 1, from 0, monotone: header h owns leaves [leaf_off[h], leaf_off[h+1]) */
  const uint32_t* byte_off;  /* leaf_off[nh] + 1, from 0, monotone: leaf j = bytes[byte_off[j] .. byte_off[j+1]) */
  const uint8_t* bytes;      /* may be NULL when byte_off[last] == 0 */
} edc_header_set;

typedef struct edc_header_rules {
  uint32_t size, reserved;
  const uint8_t* expect;       /* nh x 32 or NULL: the hash each header must have */
  const uint32_t* vals_ver;    /* nh or NULL: history version whose root the header names; EDC_HEADER_NONE skips a header */
  uint32_t vals_leaf, vals_pos;
  const uint32_t* next_ver;    /* the same, for next_validators_hash */
  uint32_t next_leaf, next_pos;
  const uint32_t* link;        /* nh or NULL: index of another header OF THIS SET whose root the header names; EDC_HEADER_NONE skips */
  uint32_t link_leaf, link_pos;
} edc_header_rules;

int edc_header_hashes(edc_ctx* ctx, const edc_header_set* hs, uint8_t* out /* nh x 32 */);
int edc_header_bind(edc_ctx* ctx, const edc_header_set* hs, const edc_header_rules* r,
                    uint8_t* bad /* nh bytes */, uint8_t* out /* nh x 32, nullable */, size_t* n_bad /* nullable */);
int edc_debug_header_ms(edc_ctx* ctx, const edc_header_set* hs, int reps, float ms[2]);

/*
 * Several GPUs in one process (a node verifying each block's votes across all of its MI355X):
 * one batch::Verifier::verify (reference src/batch.rs:149-217) split into contiguous shards, one
 * per listed device (a device may be listed more than once: several contexts on one GPU). Shard g
 * draws its z at its global queue indices, evaluates its part of the batch equation to one
 * partial point (128 bytes); the partials are gathered through the host and combined on the
 * first device (x8, identity). Verdicts and check8 are bit-identical to edc_batch_verify on one
 * device for any device list. Host buffers as edc_batch_verify; synchronous (the pipelined,
 * device-to-device form is edc_multi_submit / edc_multi_wait below).
 */
typedef struct edc_multi edc_multi;
edc_multi* edc_create_multi(const int* devices, int ndev);
void edc_destroy_multi(edc_multi* m);
int edc_multi_size(const edc_multi* m);
/* per-device context i (e.g. to load the validator-key cache on every device) */
edc_ctx* edc_multi_context(edc_multi* m, int i);
const char* edc_multi_last_error(const edc_multi* m);
int edc_multi_batch_verify(edc_multi* m, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                           const uint64_t* msg_off, const uint8_t z_seed[32], uint8_t check8[32]);
/*
 * Pipelined form of edc_multi_batch_verify for a node verifying block after block across its
 * GPUs (reference src/batch.rs:149-217, one Verifier::verify per block): edc_multi_submit splits
 * the batch into contiguous shards, enqueues each on its device's next in-flight slot (host
 * inputs copied on that slot's stream, as edc_batch_submit) and returns a ticket >= 0 without
 * waiting. Each shard's 128-byte partial point (with its bad flag) reaches the first device, where
 * a combine on its own stream sums the partials (x8, identity) as soon as the last shard lands:
 * by a peer store over xGMI when peer access from the shard's device to the first device could be
 * enabled at edc_create_multi, otherwise through the shard slot's pinned host mirror (a 256-byte
 * host-to-device copy on the combine stream); edc_create_multi fails (NULL) if enabling a
 * possible peer access fails. edc_multi_wait blocks for the ticket and returns EDC_OK /
 * EDC_INVALID_SIGNATURE / <0 with optional check8 (needs want_check8). Up to R batches in flight,
 * R = 16 / (contexts sharing the busiest listed GPU), e.g. 16 for distinct devices, 8 for [0, 0];
 * tickets are waited in submission order; host buffers are borrowed until the
 * wait. edc_multi_submit_device takes per-device slices already resident in each device's HBM:
 * n[g] items at d_vk[g], d_sig[g], d_msg[g], d_msg_off[g] form shard g, with global queue indices
 * (for z) starting at n[0] + ... + n[g-1]. Verdicts and check8 equal edc_batch_verify of the
 * concatenated batch on one device.
 */
int64_t edc_multi_submit(edc_multi* m, size_t n, const uint8_t* vk, const uint8_t* sig, const uint8_t* msg,
                         const uint64_t* msg_off, const uint8_t z_seed[32], int want_check8);
int64_t edc_multi_submit_device(edc_multi* m, const size_t* n, const uint8_t* const* d_vk,
                                const uint8_t* const* d_sig, const uint8_t* const* d_msg,
                                const uint64_t* const* d_msg_off, const uint8_t z_seed[32], int want_check8);
int edc_multi_wait(edc_multi* m, int64_t ticket, uint8_t check8[32]);
/*
 * How shard i's result block reaches the first device: 0 = same GPU (local copy), 1 = peer store
 * over xGMI (peer access enabled), 2 = staged through pinned host memory. <0 for a bad index.
 * Test knob: edc_multi_debug_force_staged(m, 1) routes every shard through host memory (the
 * fallback a device pair without peer access takes); 0 restores the routes edc_create_multi found.
 * Refused while batches are in flight. Status: distinct-device lists have not run on hardware in
 * this repository's tests (the pool's boxes hold one GPU); the staged and local routes have.
 */
int edc_multi_route(const edc_multi* m, int i);
int edc_multi_debug_force_staged(edc_multi* m, int on);
/*
 * edc_multi_batch_verify and, on failure, the grouped fallback on every shard whose own partial
 * fails (edc_batch_verify_fallback_device semantics): verdicts (host, n bytes) = Item::verify_single
 * codes, *n_invalid their count. Returns EDC_OK / EDC_INVALID_SIGNATURE / <0.
 */
int edc_multi_batch_verify_fallback(edc_multi* m, size_t n, const uint8_t* vk, const uint8_t* sig,
                                    const uint8_t* msg, const uint64_t* msg_off, const uint8_t z_seed[32],
                                    uint8_t* verdicts, int* n_invalid, uint8_t check8[32]);

#ifdef __cplusplus
}
#endif

#endif /* EDC_H */
