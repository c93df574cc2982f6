"""ed25519-consensus on MI355X -- Python host mirror of the reference's verification API.

The reference (informalsystems/ed25519-consensus 2.1.0) is Rust; no Rust toolchain exists in
this image, so the host side above the C ABI (include/edc.h, built as csrc/libedc.so) is this
module (the Rust binding a maintainer would add is in INTEGRATION.md). Names, argument meaning and error behaviour follow the
reference:

    reference                                   here
    ---------------------------------------     -------------------------------------------
    Error::{MalformedPublicKey, InvalidSignature, InvalidSliceLength}  (src/error.rs:7-20)
                                                 MalformedPublicKey / InvalidSignature /
                                                 InvalidSliceLength exceptions
    Signature (src/signature.rs)                 Signature
    VerificationKeyBytes (src/verification_key.rs:32-87)      VerificationKeyBytes
    VerificationKey::try_from / verify (:160-258)            VerificationKey
    batch::Item, Item::verify_single (src/batch.rs:75-107)   batch.Item
    batch::Verifier::{new, queue, verify} (:110-217)         batch.Verifier (everything at verify),
                                                             batch.StreamVerifier (per-item work at queue)
    SigningKey (src/signing_key.rs; test-data source)        SigningKey

All arithmetic runs in hand-written gfx950 kernels. There is NO CPU fallback: importing works
without a GPU (so the ABI can be inspected), but any verification call raises if the HIP
library or a GPU is missing.
"""
import ctypes
import os
import secrets
import sys
import threading
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libedc.so")

EDC_OK = 0
EDC_INVALID_SIGNATURE = 1
EDC_MALFORMED_PUBLIC_KEY = 2
# quorum commit sets (include/edc.h, edc_quorum_*)
EDC_QUORUM_SHORT = 3
NOT_CHECKED = 255
VOTE_ABSENT, VOTE_COMMIT, VOTE_NIL = 0, 1, 2
QUORUM_FULL, QUORUM_LIGHT = 0, 1
# validator-set quorum commit sets (include/edc.h, edc_valset_*)
EDC_DOUBLE_VOTE = 4
NO_POS = 0xFFFFFFFF
# validator-set history (edc_vhist_*): the power of a position that is not a member
VHIST_NOT_MEMBER = 0xFFFFFFFFFFFFFFFF
NO_TRUST = 0xFFFFFFFF              # EDC_VQ_NO_TRUST: a commit of a trusting pair judged by its own set only

# every symbol include/edc.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "edc_device_count", "edc_create", "edc_destroy", "edc_last_error", "edc_batch_verify",
    "edc_batch_verify_z", "edc_batch_verify_device", "edc_batch_partial_device", "edc_combine_partials",
    "edc_batch_submit_device", "edc_batch_wait", "edc_verify_each", "edc_verify_each_device",
    "edc_find_invalid_device", "edc_verify_prehashed_each", "edc_challenge", "edc_decompress", "edc_sign",
    "edc_sign_device", "edc_chacha_fill_device", "edc_reserve", "edc_set_timing", "edc_last_timings", "edc_timing_name",
    "edc_synchronize", "edc_vk_validate", "edc_keycache_load", "edc_keycache_clear", "edc_keycache_size",
    "edc_keycache_add", "edc_set_multi_union", "edc_multi_union_stats", "edc_batch_submit_prehashed_indexed",
    "edc_last_msm_accum",
    "edc_set_key_grouping", "edc_set_key_split", "edc_batch_submit", "edc_batch_submit_indexed", "edc_batch_verify_fallback_device",
    "edc_set_msm_shape", "edc_set_msm_bin_entries", "edc_set_fallback_shape", "edc_create_multi", "edc_destroy_multi", "edc_multi_size",
    "edc_multi_context", "edc_multi_last_error", "edc_multi_batch_verify", "edc_multi_batch_verify_fallback",
    "edc_multi_submit", "edc_multi_submit_device", "edc_multi_wait", "edc_set_slots", "edc_debug_set_scatter_stage",
    "edc_batch_verify_prehashed", "edc_batch_verify_prehashed_device", "edc_batch_submit_prehashed",
    "edc_batch_submit_prehashed_device", "edc_batch_verify_prehashed_fallback",
    "edc_batch_verify_prehashed_fallback_device", "edc_multi_route", "edc_multi_debug_force_staged",
    "edc_batch_submit_multi_device", "edc_batch_wait_multi", "edc_combine_records_device", "edc_debug_sc_reduce_wide",
    "edc_verifier_create", "edc_verifier_destroy", "edc_verifier_queue", "edc_verifier_queue_prehashed",
    "edc_verifier_queue_device", "edc_verifier_size", "edc_verifier_verify", "edc_verifier_verify_fallback",
    "edc_verifier_reset", "edc_vfy_queue_indexed", "edc_vfy_last_split", "edc_vfy_last_plan",
    "edc_vfy_begin_eager", "edc_vfy_set_fold", "edc_vfy_folded", "edc_vfy_eager",
    "edc_vfy_set_cached", "edc_vfy_cached", "edc_vfy_cache_counts", "edc_vfy_verify_fallback_offered",
    "edc_sigcache_create", "edc_sigcache_clear", "edc_sigcache_advance", "edc_sigcache_stats",
    "edc_sigcache_lookup_device", "edc_sigcache_batch_verify_device", "edc_sigcache_batch_verify",
    "edc_sigcache_batch_verify_fallback_device", "edc_sigcache_verify_each",
    "edc_tmpl_expand_device", "edc_tmpl_challenge", "edc_tmpl_batch_verify", "edc_tmpl_batch_verify_device",
    "edc_tmpl_batch_submit", "edc_vfy_queue_templated",
    "edc_commits_verify_device", "edc_commits_verify", "edc_tmpl_commits_verify", "edc_commits_submit",
    "edc_tmpl_commits_submit", "edc_commits_submit_device", "edc_commits_wait", "edc_debug_tmpl_commit_map",
    "edc_tmpl_commits_verify_alt", "edc_tmpl_commits_submit_alt", "edc_tmpl_commits_verify_device",
    "edc_tmpl_commits_submit_device", "edc_debug_tmpl_commit_map_alt",
    "edc_debug_live_allocs", "edc_debug_last_plan",
    "edc_quorum_plan", "edc_quorum_verify_device", "edc_quorum_verify", "edc_debug_quorum_select",
    "edc_tmpl_quorum_verify", "edc_tmpl_quorum_verify_device", "edc_debug_tmpl_quorum_last",
    "edc_cached_quorum_verify_device", "edc_cached_quorum_verify", "edc_cached_tmpl_quorum_verify_device",
    "edc_cached_tmpl_quorum_verify", "edc_debug_cached_quorum_last",
    "edc_valset_set_powers", "edc_valset_size", "edc_valset_resolve", "edc_valset_quorum_verify_device",
    "edc_valset_quorum_verify", "edc_debug_valset_select",
    "edc_vhist_set", "edc_vhist_versions", "edc_vhist_totals", "edc_vhist_resolve", "edc_vhist_quorum_verify_device",
    "edc_vhist_quorum_verify", "edc_debug_vhist_select",
    "edc_vq_verify", "edc_debug_vq_last",
    "edc_vq_trust_resolve", "edc_debug_vq_trust_last", "edc_debug_vq_trust_select",
    "edc_valhash_valset", "edc_valhash_vhist", "edc_valhash_vhist_match", "edc_debug_valhash_ms",
    "edc_header_hashes", "edc_header_bind", "edc_debug_header_ms",
]
# header hashes (include/edc.h, edc_header_*)
HEADER_MAX_LEAVES = 64
HEADER_NONE = 0xFFFFFFFF
HEADER_BAD_HASH, HEADER_BAD_VALS, HEADER_BAD_NEXT, HEADER_BAD_LINK = 1, 2, 4, 8


class EdcHeaderSet(ctypes.Structure):
    """struct edc_header_set (include/edc.h): headers as their ordered leaves, host memory."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("nh", ctypes.c_size_t),
                ("leaf_off", ctypes.c_void_p), ("byte_off", ctypes.c_void_p), ("bytes", ctypes.c_void_p)]


class EdcHeaderRules(ctypes.Structure):
    """struct edc_header_rules (include/edc.h): what each header is compared with; arrays nullable."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("expect", ctypes.c_void_p),
                ("vals_ver", ctypes.c_void_p), ("vals_leaf", ctypes.c_uint32), ("vals_pos", ctypes.c_uint32),
                ("next_ver", ctypes.c_void_p), ("next_leaf", ctypes.c_uint32), ("next_pos", ctypes.c_uint32),
                ("link", ctypes.c_void_p), ("link_leaf", ctypes.c_uint32), ("link_pos", ctypes.c_uint32)]


class EdcTemplates(ctypes.Structure):
    """struct edc_templates (include/edc.h): one call's template set, host memory."""
    _fields_ = [("count", ctypes.c_uint32),
                ("head", ctypes.c_char_p), ("head_off", ctypes.POINTER(ctypes.c_uint32)),
                ("tail", ctypes.c_char_p), ("tail_off", ctypes.POINTER(ctypes.c_uint32))]


class EdcVqRequest(ctypes.Structure):
    """struct edc_vq_request (include/edc.h): one validator-set request. Pointers are plain addresses:
    host buffers for device = 0, device addresses for device = 1."""
    _fields_ = [("size", ctypes.c_uint32), ("device", ctypes.c_uint32), ("mode", ctypes.c_int32),
                ("cached", ctypes.c_uint32), ("alt_span", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("nc", ctypes.c_size_t), ("commit_off", ctypes.c_void_p), ("commit_ver", ctypes.c_void_p),
                ("threshold", ctypes.c_void_p), ("z_seed", ctypes.c_void_p), ("vk", ctypes.c_void_p),
                ("key_idx", ctypes.c_void_p), ("sig", ctypes.c_void_p), ("flag", ctypes.c_void_p),
                ("msg", ctypes.c_void_p), ("msg_off", ctypes.c_void_p), ("k", ctypes.c_void_p),
                ("ts", ctypes.c_void_p), ("commit_tpl", ctypes.c_void_p), ("item_alt", ctypes.c_void_p),
                ("var", ctypes.c_void_p), ("var_off", ctypes.c_void_p), ("var_bytes", ctypes.c_size_t),
                ("trust_ver", ctypes.c_void_p), ("trust_threshold", ctypes.c_void_p)]


class EdcVqResult(ctypes.Structure):
    """struct edc_vq_result (include/edc.h): where a validator-set request writes; all nullable."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("commit_verdicts", ctypes.c_void_p),
                ("item_verdicts", ctypes.c_void_p), ("tally", ctypes.c_void_p), ("n_bad_commits", ctypes.c_void_p),
                ("n_checked", ctypes.c_void_p), ("n_miss", ctypes.c_void_p), ("check8", ctypes.c_void_p),
                ("trust_verdicts", ctypes.c_void_p), ("trust_tally", ctypes.c_void_p), ("n_bad_trust", ctypes.c_void_p)]


class EdcPlanInfo(ctypes.Structure):
    """struct edc_plan_info (include/edc.h): the MSM plan of the last batch, as the host chose it."""
    _fields_ = [("nwin", ctypes.c_uint32), ("nwin_short", ctypes.c_uint32), ("nranges", ctypes.c_uint32),
                ("sum_ranges", ctypes.c_uint32), ("bins_per_range", ctypes.c_uint32),
                ("per_sig", ctypes.c_uint32), ("split", ctypes.c_uint32), ("few", ctypes.c_uint32),
                ("fold", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("target", ctypes.c_double),
                ("bits", ctypes.c_uint8 * 32), ("nsub", ctypes.c_uint8 * 32), ("nslice", ctypes.c_uint16 * 32)]

    def as_dict(self):
        w = int(self.nwin)
        d = {k: int(getattr(self, k)) for k in ("nwin", "nwin_short", "nranges", "sum_ranges", "bins_per_range")}
        d.update({k: bool(getattr(self, k)) for k in ("per_sig", "split", "few", "fold")})
        d.update(target=float(self.target), bits=list(self.bits[:w]), nsub=list(self.nsub[:w]),
                 nslice=list(self.nslice[:w]))
        return d


class Error(Exception):
    """ed25519_consensus::Error (reference src/error.rs:7-20)."""


class MalformedSecretKey(Error):
    pass


class MalformedPublicKey(Error):
    pass


class InvalidSignature(Error):
    pass


class InvalidSliceLength(Error):
    pass


class QuorumShort(Error):
    """Every checked vote of the commit verified, but its tally is not above the threshold
    (EDC_QUORUM_SHORT; CometBFT's ErrNotEnoughVotingPowerSigned). Not an error of the reference crate."""


class DoubleVote(Error):
    """Two checked votes of one commit come from the same member of the validator set
    (EDC_DOUBLE_VOTE; CometBFT's double-vote error). Not an error of the reference crate."""


class EngineError(RuntimeError):
    """HIP/runtime failure. Never interpreted as a verification verdict."""


_CODE_TO_ERR = {EDC_INVALID_SIGNATURE: InvalidSignature, EDC_MALFORMED_PUBLIC_KEY: MalformedPublicKey}

_lib = None
_lib_lock = threading.Lock()


def load_library(path=None):
    """Load csrc/libedc.so and declare argument types. Raises if it is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        # an explicit path is a measurement hook for tools/ (A/B builds); the product loads LIB_PATH
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise EngineError(f"HIP extension not built: {p} (run __graft_entry__.build())")
        _share_torch_hip_runtime()
        lib = ctypes.CDLL(p)
        c_sz, c_u8p, c_u64p, c_vp = ctypes.c_size_t, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
        lib.edc_device_count.restype = ctypes.c_int
        lib.edc_create.restype = c_vp
        lib.edc_create.argtypes = [ctypes.c_int]
        lib.edc_destroy.argtypes = [c_vp]
        lib.edc_last_error.restype = ctypes.c_char_p
        lib.edc_last_error.argtypes = [c_vp]
        lib.edc_batch_verify.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, c_vp]
        lib.edc_batch_verify_z.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, c_vp]
        lib.edc_batch_verify_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_u8p, ctypes.c_uint64, c_vp, c_vp]
        lib.edc_batch_partial_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_u8p, ctypes.c_uint64, c_vp,
                                                 c_vp, ctypes.POINTER(ctypes.c_int)]
        lib.edc_combine_partials.argtypes = [c_vp, c_sz, c_u8p, ctypes.c_int, c_vp]
        if hasattr(lib, "edc_combine_records_device"):      # absent from older A/B builds (--lib)
            lib.edc_combine_records_device.argtypes = [c_vp, c_vp, c_sz, c_vp, c_sz, c_vp]
        if hasattr(lib, "edc_debug_sc_reduce_wide"):
            lib.edc_debug_sc_reduce_wide.argtypes = [c_vp, c_sz, c_vp, c_vp]
        if hasattr(lib, "edc_debug_live_allocs"):            # absent from older A/B builds (--lib)
            lib.edc_debug_live_allocs.argtypes = [c_u64p]
        if hasattr(lib, "edc_debug_last_plan"):              # absent from older A/B builds (--lib)
            lib.edc_debug_last_plan.argtypes = [c_vp, ctypes.POINTER(EdcPlanInfo)]
            lib.edc_vfy_last_plan.argtypes = [c_vp, ctypes.POINTER(EdcPlanInfo)]
        lib.edc_batch_submit_device.restype = ctypes.c_int64
        lib.edc_batch_submit_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_u8p, ctypes.c_uint64, c_vp,
                                                ctypes.c_int]
        lib.edc_batch_submit.restype = ctypes.c_int64
        lib.edc_batch_submit.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, ctypes.c_uint64, ctypes.c_int]
        lib.edc_batch_submit_indexed.restype = ctypes.c_int64
        lib.edc_batch_submit_indexed.argtypes = [c_vp, c_sz, ctypes.POINTER(ctypes.c_uint32), c_u8p, c_u8p, c_u64p,
                                                 c_u8p, ctypes.c_uint64, ctypes.c_int]
        lib.edc_batch_wait.argtypes = [c_vp, ctypes.c_int64, c_vp, c_vp, ctypes.POINTER(ctypes.c_int)]
        if hasattr(lib, "edc_batch_verify_prehashed"):       # absent from older A/B builds (tools/)
            lib.edc_batch_verify_prehashed.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p, c_vp]
            lib.edc_batch_verify_prehashed_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_u8p, ctypes.c_uint64,
                                                              c_vp, c_vp]
            lib.edc_batch_submit_prehashed.restype = ctypes.c_int64
            lib.edc_batch_submit_prehashed.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u8p, ctypes.c_uint64,
                                                       ctypes.c_int]
            lib.edc_batch_submit_prehashed_device.restype = ctypes.c_int64
            lib.edc_batch_submit_prehashed_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_u8p, ctypes.c_uint64,
                                                              c_vp, ctypes.c_int]
            lib.edc_batch_verify_prehashed_fallback.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u8p, c_vp,
                                                                ctypes.POINTER(ctypes.c_int), c_vp]
            lib.edc_batch_verify_prehashed_fallback_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_u8p, c_vp,
                                                                       ctypes.POINTER(ctypes.c_int), c_vp]
        lib.edc_verify_each.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_vp]
        lib.edc_verify_each_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]
        lib.edc_find_invalid_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_u8p, c_sz, c_vp]
        lib.edc_batch_verify_fallback_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_u8p, c_vp,
                                                         ctypes.POINTER(ctypes.c_int), c_vp]
        lib.edc_set_msm_shape.argtypes = [c_vp, ctypes.c_int, ctypes.c_int]
        lib.edc_set_msm_bin_entries.argtypes = [c_vp, ctypes.c_int]
        if hasattr(lib, "edc_debug_set_scatter_stage"):      # absent from older A/B builds (tools/)
            lib.edc_debug_set_scatter_stage.argtypes = [ctypes.c_uint32]
        lib.edc_set_fallback_shape.argtypes = [c_vp, ctypes.c_int, ctypes.c_int]
        lib.edc_create_multi.restype = c_vp
        lib.edc_create_multi.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        lib.edc_destroy_multi.argtypes = [c_vp]
        lib.edc_multi_size.argtypes = [c_vp]
        lib.edc_multi_context.restype = c_vp
        lib.edc_multi_context.argtypes = [c_vp, ctypes.c_int]
        lib.edc_multi_last_error.restype = ctypes.c_char_p
        lib.edc_multi_last_error.argtypes = [c_vp]
        lib.edc_multi_batch_verify.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, c_vp]
        lib.edc_multi_batch_verify_fallback.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, c_vp,
                                                        ctypes.POINTER(ctypes.c_int), c_vp]
        lib.edc_multi_submit.restype = ctypes.c_int64
        lib.edc_multi_submit.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, ctypes.c_int]
        lib.edc_multi_submit_device.restype = ctypes.c_int64
        lib.edc_multi_submit_device.argtypes = [c_vp, ctypes.POINTER(c_sz), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp),
                                                ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), c_u8p, ctypes.c_int]
        lib.edc_multi_wait.argtypes = [c_vp, ctypes.c_int64, c_vp]
        if hasattr(lib, "edc_batch_submit_multi_device"):
            lib.edc_batch_submit_multi_device.restype = ctypes.c_int64
            lib.edc_batch_submit_multi_device.argtypes = [c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_u8p,
                                                          ctypes.c_uint64, ctypes.c_int]
            lib.edc_batch_wait_multi.argtypes = [c_vp, ctypes.c_int64, c_sz, ctypes.POINTER(ctypes.c_int), c_vp, c_vp,
                                                 ctypes.POINTER(ctypes.c_int)]
        if hasattr(lib, "edc_multi_route"):
            lib.edc_multi_route.argtypes = [c_vp, ctypes.c_int]
            lib.edc_multi_debug_force_staged.argtypes = [c_vp, ctypes.c_int]
        lib.edc_set_slots.argtypes = [c_vp, ctypes.c_int]
        lib.edc_verify_prehashed_each.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_vp]
        lib.edc_challenge.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_vp]
        lib.edc_decompress.argtypes = [c_vp, c_sz, c_u8p, c_vp, c_vp]
        lib.edc_sign.argtypes = [c_vp, c_sz, c_u8p, c_sz, c_vp, c_u8p, c_u64p, c_vp, c_vp]
        lib.edc_sign_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]
        lib.edc_chacha_fill_device.argtypes = [c_vp, c_u8p, ctypes.c_uint64, ctypes.c_uint64, c_vp]
        lib.edc_reserve.argtypes = [c_vp, c_sz]
        lib.edc_set_timing.argtypes = [c_vp, ctypes.c_int]
        lib.edc_last_timings.restype = ctypes.c_int
        lib.edc_last_timings.argtypes = [c_vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
        lib.edc_timing_name.restype = ctypes.c_char_p
        lib.edc_timing_name.argtypes = [ctypes.c_int]
        lib.edc_synchronize.argtypes = [c_vp]
        lib.edc_vk_validate.argtypes = [c_vp, c_sz, c_u8p, c_vp]
        lib.edc_keycache_load.restype = ctypes.c_int64
        lib.edc_keycache_load.argtypes = [c_vp, c_sz, c_u8p, c_vp]
        if hasattr(lib, "edc_keycache_add"):                 # absent from older A/B builds (tools/)
            lib.edc_set_multi_union.restype = ctypes.c_int
            lib.edc_set_multi_union.argtypes = [c_vp, ctypes.c_int]
            lib.edc_multi_union_stats.restype = ctypes.c_int
            lib.edc_multi_union_stats.argtypes = [c_vp, ctypes.POINTER(ctypes.c_uint64),
                                                  ctypes.POINTER(ctypes.c_uint64)]
            lib.edc_keycache_add.restype = ctypes.c_int64
            lib.edc_keycache_add.argtypes = [c_vp, c_sz, c_u8p, c_vp]
            lib.edc_last_msm_accum.restype = ctypes.c_int
            lib.edc_last_msm_accum.argtypes = [c_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)]
            lib.edc_batch_submit_prehashed_indexed.restype = ctypes.c_int64
            lib.edc_batch_submit_prehashed_indexed.argtypes = [c_vp, c_sz, ctypes.POINTER(ctypes.c_uint32), c_u8p,
                                                               c_u8p, c_u8p, ctypes.c_uint64, ctypes.c_int]
        lib.edc_keycache_clear.argtypes = [c_vp]
        lib.edc_keycache_size.restype = c_sz
        lib.edc_keycache_size.argtypes = [c_vp]
        lib.edc_set_key_grouping.argtypes = [c_vp, ctypes.c_int]
        lib.edc_set_key_split.argtypes = [c_vp, ctypes.c_int]
        if hasattr(lib, "edc_verifier_create"):              # absent from older A/B builds (tools/)
            lib.edc_verifier_create.restype = c_vp
            lib.edc_verifier_create.argtypes = [c_vp, c_sz]
            lib.edc_verifier_destroy.restype = None
            lib.edc_verifier_destroy.argtypes = [c_vp]
            lib.edc_verifier_queue.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p]
            lib.edc_verifier_queue_prehashed.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p]
            lib.edc_verifier_queue_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp]
            lib.edc_verifier_size.restype = c_sz
            lib.edc_verifier_size.argtypes = [c_vp]
            lib.edc_verifier_verify.argtypes = [c_vp, c_u8p, c_u8p, c_vp]
            lib.edc_verifier_verify_fallback.argtypes = [c_vp, c_u8p, c_vp, ctypes.POINTER(ctypes.c_int), c_vp]
            lib.edc_verifier_reset.argtypes = [c_vp]
        if hasattr(lib, "edc_vfy_queue_indexed"):            # absent from older A/B builds (tools/)
            lib.edc_vfy_queue_indexed.argtypes = [c_vp, c_sz, ctypes.POINTER(ctypes.c_uint32), c_u8p, c_u8p, c_u64p,
                                                  c_u8p]
            lib.edc_vfy_last_split.argtypes = [c_vp]
        if hasattr(lib, "edc_vfy_begin_eager"):              # absent from older A/B builds (tools/)
            lib.edc_vfy_begin_eager.argtypes = [c_vp, c_u8p]
            lib.edc_vfy_set_fold.argtypes = [c_vp, c_sz]
            lib.edc_vfy_folded.argtypes = [c_vp, c_u64p, c_u64p]
            lib.edc_vfy_eager.argtypes = [c_vp]
        if hasattr(lib, "edc_vfy_set_cached"):               # absent from older A/B builds (tools/)
            lib.edc_vfy_set_cached.argtypes = [c_vp, ctypes.c_int]
            lib.edc_vfy_cached.argtypes = [c_vp]
            lib.edc_vfy_cache_counts.argtypes = [c_vp, c_u64p, c_u64p]
            lib.edc_vfy_verify_fallback_offered.argtypes = [c_vp, c_u8p, c_vp, ctypes.POINTER(ctypes.c_int), c_vp]
        if hasattr(lib, "edc_sigcache_create"):              # absent from older A/B builds (tools/)
            c_szp = ctypes.POINTER(c_sz)
            lib.edc_sigcache_create.argtypes = [c_vp, c_sz, ctypes.c_int]
            lib.edc_sigcache_clear.argtypes = [c_vp]
            lib.edc_sigcache_advance.argtypes = [c_vp]
            lib.edc_sigcache_stats.argtypes = [c_vp, c_u64p]
            lib.edc_sigcache_lookup_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]
            lib.edc_sigcache_batch_verify_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_u8p, c_vp,
                                                             c_szp]
            lib.edc_sigcache_batch_verify.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, c_u8p, c_vp, c_szp]
            lib.edc_sigcache_batch_verify_fallback_device.argtypes = [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_u8p,
                                                                      c_vp, ctypes.POINTER(ctypes.c_int), c_vp, c_szp]
            lib.edc_sigcache_verify_each.argtypes = [c_vp, c_sz, c_u8p, c_u8p, c_u8p, c_u64p, c_u8p, c_vp, c_szp]
        if hasattr(lib, "edc_tmpl_expand_device"):           # absent from older A/B builds (tools/)
            c_tsp, c_u16p = ctypes.POINTER(EdcTemplates), ctypes.POINTER(ctypes.c_uint16)
            c_u32p = ctypes.POINTER(ctypes.c_uint32)
            lib.edc_tmpl_expand_device.argtypes = [c_vp, c_tsp, c_sz, c_vp, c_vp, c_vp, c_sz, c_vp, c_sz, c_vp]
            lib.edc_tmpl_challenge.argtypes = [c_vp, c_tsp, c_sz, c_u8p, c_u8p, c_u16p, c_u8p, c_u32p, c_vp]
            lib.edc_tmpl_batch_verify.argtypes = [c_vp, c_tsp, c_sz, c_u8p, c_u32p, c_u8p, c_u16p, c_u8p, c_u32p, c_u8p,
                                                  c_vp]
            lib.edc_tmpl_batch_verify_device.argtypes = [c_vp, c_tsp, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_u8p,
                                                         ctypes.c_uint64, c_vp, c_vp]
            lib.edc_tmpl_batch_submit.restype = ctypes.c_int64
            lib.edc_tmpl_batch_submit.argtypes = [c_vp, c_tsp, c_sz, c_u8p, c_u32p, c_u8p, c_u16p, c_u8p, c_u32p, c_u8p,
                                                  ctypes.c_uint64, ctypes.c_int]
            lib.edc_vfy_queue_templated.argtypes = [c_vp, c_tsp, c_sz, c_u8p, c_u32p, c_u8p, c_u16p, c_u8p, c_u32p]
        if hasattr(lib, "edc_commits_verify"):               # absent from older A/B builds (tools/)
            c_tsp, c_u16p = ctypes.POINTER(EdcTemplates), ctypes.POINTER(ctypes.c_uint16)
            c_u32p, c_ip = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)
            lib.edc_commits_verify_device.argtypes = [c_vp, c_sz, c_u32p, c_vp, c_vp, c_vp, c_vp, c_vp, c_u8p, c_vp,
                                                      c_vp, c_ip]
            lib.edc_commits_verify.argtypes = [c_vp, c_sz, c_u32p, c_u8p, c_u32p, c_u8p, c_u8p, c_u64p, c_u8p, c_u8p,
                                               c_vp, c_vp, c_ip]
            lib.edc_tmpl_commits_verify.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, c_u8p, c_u32p, c_u8p, c_u8p,
                                                    c_u32p, c_u8p, c_vp, c_vp, c_ip]
            lib.edc_commits_submit.restype = ctypes.c_int64
            lib.edc_commits_submit.argtypes = [c_vp, c_sz, c_u32p, c_u8p, c_u32p, c_u8p, c_u8p, c_u64p, c_u8p, c_u8p]
            lib.edc_tmpl_commits_submit.restype = ctypes.c_int64
            lib.edc_tmpl_commits_submit.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, c_u8p, c_u32p, c_u8p, c_u8p,
                                                    c_u32p, c_u8p]
            lib.edc_commits_submit_device.restype = ctypes.c_int64
            lib.edc_commits_submit_device.argtypes = [c_vp, c_sz, c_u32p, c_vp, c_vp, c_vp, c_vp, c_vp, c_u8p]
            lib.edc_commits_wait.argtypes = [c_vp, ctypes.c_int64, c_vp, c_vp, c_ip]
            lib.edc_debug_tmpl_commit_map.argtypes = [c_vp, c_sz, c_u32p, c_u16p, c_u16p, ctypes.c_int,
                                                      ctypes.POINTER(ctypes.c_float)]
        if hasattr(lib, "edc_tmpl_commits_verify_alt"):      # absent from older A/B builds (tools/)
            c_tsp, c_u16p = ctypes.POINTER(EdcTemplates), ctypes.POINTER(ctypes.c_uint16)
            c_u32p, c_ip, c_u32 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.c_uint32
            lib.edc_tmpl_commits_verify_alt.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, c_u32, c_vp, c_u8p, c_u32p,
                                                        c_u8p, c_u8p, c_u32p, c_u8p, c_vp, c_vp, c_ip]
            lib.edc_tmpl_commits_submit_alt.restype = ctypes.c_int64
            lib.edc_tmpl_commits_submit_alt.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, c_u32, c_vp, c_u8p, c_u32p,
                                                        c_u8p, c_u8p, c_u32p, c_u8p]
            lib.edc_tmpl_commits_verify_device.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, c_u32, c_vp, c_vp, c_vp,
                                                           c_vp, c_vp, c_sz, c_u8p, c_vp, c_vp, c_ip]
            lib.edc_tmpl_commits_submit_device.restype = ctypes.c_int64
            lib.edc_tmpl_commits_submit_device.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, c_u32, c_vp, c_vp, c_vp,
                                                           c_vp, c_vp, c_sz, c_u8p]
            lib.edc_debug_tmpl_commit_map_alt.argtypes = [c_vp, c_sz, c_u32p, c_u16p, c_u32, c_vp, c_vp, c_ip,
                                                          ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        if hasattr(lib, "edc_quorum_verify"):                # absent from older A/B builds (tools/)
            c_u32p, c_ip, c_szp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(c_sz)
            lib.edc_quorum_plan.argtypes = [c_vp, c_sz, c_u32p, c_u64p, c_u8p, c_u64p, ctypes.c_int, c_vp, c_vp, c_szp]
            lib.edc_quorum_verify_device.argtypes = [c_vp, c_sz, c_u32p, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                     c_u64p, ctypes.c_int, c_u8p, c_vp, c_vp, c_vp, c_ip, c_szp, c_vp]
            lib.edc_quorum_verify.argtypes = [c_vp, c_sz, c_u32p, c_u8p, c_u32p, c_u8p, c_u8p, c_u64p, c_u8p, c_u64p,
                                              c_u8p, c_u64p, ctypes.c_int, c_u8p, c_vp, c_vp, c_vp, c_ip, c_szp, c_vp]
            lib.edc_debug_quorum_select.argtypes = [c_vp, c_sz, c_u32p, c_u64p, c_u8p, c_u64p, ctypes.c_int,
                                                    ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        if hasattr(lib, "edc_tmpl_quorum_verify"):           # absent from older A/B builds (tools/)
            c_tsp, c_u16p = ctypes.POINTER(EdcTemplates), ctypes.POINTER(ctypes.c_uint16)
            c_u32p, c_ip, c_szp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(c_sz)
            lib.edc_tmpl_quorum_verify.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, ctypes.c_uint32, c_vp, c_u8p, c_u32p,
                                                   c_u8p, c_u8p, c_u32p, c_u64p, c_u8p, c_u64p, ctypes.c_int, c_u8p,
                                                   c_vp, c_vp, c_vp, c_ip, c_szp, c_vp]
            lib.edc_tmpl_quorum_verify_device.argtypes = [c_vp, c_tsp, c_sz, c_u32p, c_u16p, ctypes.c_uint32, c_vp, c_vp,
                                                          c_vp, c_vp, c_vp, c_sz, c_vp, c_vp, c_u64p, ctypes.c_int, c_u8p,
                                                          c_vp, c_vp, c_vp, c_ip, c_szp, c_vp]
            lib.edc_debug_tmpl_quorum_last.argtypes = [c_vp, c_u64p]
        if hasattr(lib, "edc_cached_quorum_verify"):         # absent from older A/B builds (tools/)
            # the uncached twins' arguments with n_miss in front of check8
            for name in ("edc_quorum_verify_device", "edc_quorum_verify", "edc_tmpl_quorum_verify_device",
                         "edc_tmpl_quorum_verify"):
                a = list(getattr(lib, name).argtypes)
                getattr(lib, name.replace("edc_", "edc_cached_", 1)).argtypes = a[:-1] + [ctypes.POINTER(c_sz), a[-1]]
            lib.edc_debug_cached_quorum_last.argtypes = [c_vp, c_u64p]
        if hasattr(lib, "edc_valset_quorum_verify"):         # absent from older A/B builds (tools/)
            # the quorum twins' arguments without the power array
            a = list(lib.edc_quorum_verify_device.argtypes)
            lib.edc_valset_quorum_verify_device.argtypes = a[:8] + a[9:]
            a = list(lib.edc_quorum_verify.argtypes)
            lib.edc_valset_quorum_verify.argtypes = a[:9] + a[10:]
            lib.edc_valset_set_powers.argtypes = [c_vp, c_sz, c_u64p]
            lib.edc_valset_size.argtypes = [c_vp]
            lib.edc_valset_resolve.argtypes = [c_vp, c_sz, c_u32p, c_u8p, c_u32p, c_u8p, c_u64p, ctypes.c_int, c_vp, c_vp,
                                               c_vp, c_vp, c_vp, c_szp, c_vp]
            lib.edc_debug_valset_select.argtypes = [c_vp, c_sz, c_u32p, c_u8p, c_u32p, c_u8p, c_u64p, ctypes.c_int,
                                                    ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        if hasattr(lib, "edc_vhist_quorum_verify"):          # absent from older A/B builds (tools/)
            # the validator-set twins' arguments with the commits' versions behind the offsets
            for name in ("edc_valset_resolve", "edc_valset_quorum_verify_device", "edc_valset_quorum_verify",
                         "edc_debug_valset_select"):
                a = list(getattr(lib, name).argtypes)
                getattr(lib, name.replace("valset", "vhist")).argtypes = a[:3] + [c_u32p] + a[3:]
            lib.edc_vhist_set.argtypes = [c_vp, c_sz, c_u64p, c_sz, c_u32p, c_u32p, c_u64p]
            lib.edc_vhist_versions.argtypes = [c_vp]
            lib.edc_vhist_totals.argtypes = [c_vp, ctypes.c_uint32, c_sz, c_u64p, c_u32p]
        if hasattr(lib, "edc_vq_verify"):                    # absent from older A/B builds (tools/)
            lib.edc_vq_verify.argtypes = [c_vp, ctypes.POINTER(EdcVqRequest), ctypes.POINTER(EdcVqResult)]
            lib.edc_debug_vq_last.argtypes = [c_vp, c_u64p]
        if hasattr(lib, "edc_vq_trust_resolve"):             # absent from older A/B builds (tools/)
            lib.edc_vq_trust_resolve.argtypes = [c_vp, c_sz, c_u32p, c_u32p, c_u32p, c_u8p, c_u32p, c_u8p, c_u64p, c_u64p,
                                                 ctypes.c_int] + [c_vp] * 13 + [c_szp]
            lib.edc_debug_vq_trust_last.argtypes = [c_vp, c_u64p]
            lib.edc_debug_vq_trust_select.argtypes = [c_vp, c_sz, c_u32p, c_u32p, c_u32p, c_u8p, c_u32p, c_u8p, c_u64p,
                                                      c_u64p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        if hasattr(lib, "edc_valhash_vhist"):                # absent from older A/B builds (tools/)
            lib.edc_valhash_valset.argtypes = [c_vp, c_vp]
            lib.edc_valhash_vhist.argtypes = [c_vp, ctypes.c_uint32, c_sz, c_vp]
            lib.edc_valhash_vhist_match.argtypes = [c_vp, c_sz, c_u32p, c_vp, c_vp, c_szp]
            lib.edc_debug_valhash_ms.argtypes = [c_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        if hasattr(lib, "edc_header_bind"):                  # absent from older A/B builds (tools/)
            c_hsp = ctypes.POINTER(EdcHeaderSet)
            lib.edc_header_hashes.argtypes = [c_vp, c_hsp, c_vp]
            lib.edc_header_bind.argtypes = [c_vp, c_hsp, ctypes.POINTER(EdcHeaderRules), c_vp, c_vp, c_szp]
            lib.edc_debug_header_ms.argtypes = [c_vp, c_hsp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
        if path is None:
            _lib = lib
        return lib


def _share_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64 (SONAME libamdhip64.so.7). If torch is in this
    process, pre-load exactly that file so libedc.so's DT_NEEDED libamdhip64.so.7 binds to the
    same HIP runtime instead of /opt/rocm's copy (two runtimes in one process cannot share the
    device). Without torch, the system ROCm runtime is used."""
    torch = sys.modules.get("torch")
    if torch is None:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def _arena(msgs):
    """Flatten messages into (arena bytes, uint64 offsets[n+1])."""
    offs = (ctypes.c_uint64 * (len(msgs) + 1))()
    total = 0
    for i, m in enumerate(msgs):
        offs[i] = total
        total += len(m)
    offs[len(msgs)] = total
    return b"".join(bytes(m) for m in msgs) or b"\0", offs


def _joined(*lists):
    """Each list of byte strings as one buffer; an empty list as one zero byte, so that the C side
    gets a pointer it never reads, not null."""
    return tuple(b"".join(x) or b"\0" for x in lists)


def _tmpl_items(tpl, holes, var_off=None):
    """(uint16 tpl[n], var bytes, uint32 var_off[n+1]) of a templated call: the holes packed back to
    back. var_off overrides the offsets computed from the holes (tests of the refusals)."""
    n = len(tpl)
    t = (ctypes.c_uint16 * max(n, 1))(*tpl)
    if var_off is None:
        var_off, total = [0], 0
        for h in holes:
            total += len(h)
            var_off.append(total)
    off = (ctypes.c_uint32 * (n + 1))(*var_off)
    return t, b"".join(bytes(h) for h in holes) or b"\0", off


def _tmpl_keys(n, vks, key_idx):
    """(vk bytes or None, uint32 key_idx[n] or None) as the templated host entries take them."""
    vkb = None if vks is None else (b"".join(_as_bytes(x, 32) for x in vks) or b"\0")
    idx = None if key_idx is None else (ctypes.c_uint32 * max(n, 1))(*key_idx)
    return vkb, idx


class Engine:
    """One C-ABI context = one GPU = one HIP stream (include/edc.h)."""

    def __init__(self, device=None, lib_path=None):
        self.lib = load_library(lib_path)
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        cnt = self.lib.edc_device_count()
        if cnt <= 0:
            raise EngineError("no HIP device visible; the MI355X path has no CPU fallback")
        self.device = device
        self.ctx = self.lib.edc_create(device)
        if not self.ctx:
            raise EngineError(f"edc_create({device}) failed")
        self._lock = threading.Lock()
        self._kc_keys = set()          # host mirror of the key cache's key bytes (keycache_missing)
        self._host_inflight = {}        # ticket -> host buffers borrowed by edc_batch_submit
        self._commits_inflight = {}     # ticket -> (nc, n, keep) of a submitted commit set (_commits_call)
        self._verifiers = weakref.WeakSet()   # open batch.StreamVerifier objects (destroyed before the context)

    def close(self):
        if self.ctx:
            for sv in list(getattr(self, "_verifiers", [])):
                sv.close()
            self.lib.edc_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise EngineError(f"edc error {rc}: {self.lib.edc_last_error(self.ctx).decode()}")
        return rc

    # ---- bulk entry points (bytes in, verdicts out) ----
    def batch_verify(self, vks, sigs, msgs, z_seed=None, z=None, want_check8=False):
        n = len(vks)
        arena, offs = _arena(msgs)
        vkb, sigb = _joined(vks, sigs)
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            if z is not None:
                rc = self.lib.edc_batch_verify_z(self.ctx, n, vkb, sigb, arena, offs, bytes(z) or b"\0", check8)
            else:
                rc = self.lib.edc_batch_verify(self.ctx, n, vkb, sigb, arena, offs, bytes(z_seed), check8)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def batch_verify_prehashed(self, vks, sigs, ks, z_seed=None, z=None, want_check8=False):
        """Batch of prehashed items {vk_bytes, sig, k} (edc_batch_verify_prehashed): the reference's
        Verifier::verify over Items whose k was computed at Item::from (src/batch.rs:76-94)."""
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self.lib.edc_batch_verify_prehashed(
                self.ctx, len(vks), *_joined(vks, sigs, ks),
                bytes(z_seed) if z is None else None, (bytes(z) or b"\0") if z is not None else None, check8)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def _batch_submit(self, fn, n, bufs, z_base, want_check8):
        """One host submission: fn(ctx, n, *bufs, z_base, want_check8) -> ticket; bufs, the staged host
        buffers with the z seed last, are kept alive here until batch_wait(ticket)."""
        with self._lock:
            t = fn(self.ctx, n, *bufs, z_base, 1 if want_check8 else 0)
            if t < 0:
                self._check(t)
            self._host_inflight[t] = bufs
        return t

    def batch_submit_prehashed(self, vks, sigs, ks, z_seed, z_base=0, want_check8=False):
        """Asynchronous prehashed batch from host buffers (edc_batch_submit_prehashed)."""
        return self._batch_submit(self.lib.edc_batch_submit_prehashed, len(vks), (*_joined(vks, sigs, ks), bytes(z_seed)),
                                  z_base, want_check8)

    def batch_submit_prehashed_indexed(self, key_idx, sigs, ks, z_seed, z_base=0, want_check8=False):
        """edc_batch_submit_prehashed with keys given as positions in the last keycache_load list
        (100 bytes per item over PCIe)."""
        n = len(sigs)
        idx = (ctypes.c_uint32 * max(n, 1))(*key_idx)
        return self._batch_submit(self.lib.edc_batch_submit_prehashed_indexed, n, (idx, *_joined(sigs, ks), bytes(z_seed)),
                                  z_base, want_check8)

    def batch_verify_prehashed_fallback(self, vks, sigs, ks, z_seed):
        """(code, per-item Item::verify_single codes, number invalid, check8) of a prehashed batch."""
        n = len(vks)
        check8 = ctypes.create_string_buffer(32)
        v = ctypes.create_string_buffer(max(n, 1))
        cnt = ctypes.c_int(0)
        with self._lock:
            rc = self.lib.edc_batch_verify_prehashed_fallback(self.ctx, n, *_joined(vks, sigs, ks), bytes(z_seed), v,
                                                              ctypes.byref(cnt), check8)
        self._check(rc)
        return rc, list(v.raw[:n]), cnt.value, check8.raw

    def batch_submit(self, vks, sigs, msgs, z_seed, z_base=0, want_check8=False):
        """Asynchronous host-buffer batch (edc_batch_submit): returns a ticket; the staged host
        buffers are kept alive here until batch_wait(ticket)."""
        return self._batch_submit(self.lib.edc_batch_submit, len(vks), (*_joined(vks, sigs), *_arena(msgs), bytes(z_seed)),
                                  z_base, want_check8)

    def batch_submit_indexed(self, key_idx, sigs, msgs, z_seed, z_base=0, want_check8=False):
        """edc_batch_submit with keys given as positions in the last keycache_load list."""
        n = len(sigs)
        idx = (ctypes.c_uint32 * max(n, 1))(*key_idx)
        return self._batch_submit(self.lib.edc_batch_submit_indexed, n, (idx, *_joined(sigs), *_arena(msgs), bytes(z_seed)),
                                  z_base, want_check8)

    # ---- templated messages (edc_tmpl_*): msg_i = head[tpl[i]] || hole_i || tail[tpl[i]] ----
    def tmpl_expand_device(self, templates, n, d_tpl, d_var, d_var_off, var_bytes, d_msg_out, msg_cap, d_msg_off_out):
        """Materialise the arena and its n + 1 uint64 offsets into caller device buffers
        (edc_tmpl_expand_device; device pointers as ints)."""
        ts, _keep = templates.struct()
        with self._lock:
            rc = self.lib.edc_tmpl_expand_device(self.ctx, ctypes.byref(ts), n, d_tpl, d_var, d_var_off, var_bytes,
                                                 d_msg_out, msg_cap, d_msg_off_out)
        self._check(rc)

    def tmpl_challenge(self, templates, vks, sigs, tpl, holes, var_off=None):
        """edc_challenge for templated messages: the k of every item."""
        n = len(sigs)
        ts, _keep = templates.struct()
        t, var, off = _tmpl_items(tpl, holes, var_off)
        out = ctypes.create_string_buffer(max(32 * n, 1))
        with self._lock:
            self._check(self.lib.edc_tmpl_challenge(self.ctx, ctypes.byref(ts), n, b"".join(vks) or b"\0",
                                                    b"".join(sigs) or b"\0", t, var, off, out))
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def batch_verify_templated(self, templates, sigs, tpl, holes, z_seed, vks=None, key_idx=None, want_check8=False,
                               var_off=None):
        """edc_tmpl_batch_verify: (code, check8 or None). Exactly one of vks and key_idx (positions
        in the last keycache_load list)."""
        n = len(sigs)
        ts, _keep = templates.struct()
        t, var, off = _tmpl_items(tpl, holes, var_off)
        vkb, idx = _tmpl_keys(n, vks, key_idx)
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self.lib.edc_tmpl_batch_verify(self.ctx, ctypes.byref(ts), n, vkb, idx, b"".join(sigs) or b"\0", t, var,
                                                off, bytes(z_seed), check8)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def batch_verify_templated_device(self, templates, n, d_vk, d_sig, d_tpl, d_var, d_var_off, var_bytes, z_seed,
                                      z_base=0, d_z=None, want_check8=False):
        """edc_tmpl_batch_verify_device (device pointers as ints): (code, check8 or None)."""
        ts, _keep = templates.struct()
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self.lib.edc_tmpl_batch_verify_device(self.ctx, ctypes.byref(ts), n, d_vk, d_sig, d_tpl, d_var,
                                                       d_var_off, var_bytes, bytes(z_seed), z_base, d_z, check8)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def batch_submit_templated(self, templates, sigs, tpl, holes, z_seed, z_base=0, vks=None, key_idx=None,
                               want_check8=False, var_off=None):
        """edc_tmpl_batch_submit: a ticket for batch_wait; the host buffers, the set included, are
        kept alive here until then."""
        n = len(sigs)
        ts, keep = templates.struct()
        t, var, off = _tmpl_items(tpl, holes, var_off)
        vkb, idx = _tmpl_keys(n, vks, key_idx)
        bufs = (ts, keep, vkb, idx, b"".join(sigs) or b"\0", t, var, off, bytes(z_seed))
        with self._lock:
            tk = self.lib.edc_tmpl_batch_submit(self.ctx, ctypes.byref(ts), n, vkb, idx, bufs[4], t, var, off, bufs[8],
                                                z_base, 1 if want_check8 else 0)
            if tk < 0:
                self._check(tk)
            self._host_inflight[tk] = bufs
        return tk

    # ---- commit sets (edc_commits_*): many variable-size batches in one launch ----
    # commit_off: nc + 1 offsets, commit c = items [commit_off[c], commit_off[c+1]). Every result is
    # (code, [verdict per commit], [Item::verify_single code per item], number of commits not Ok).
    @staticmethod
    def _commit_offsets(commit_off):
        off = [int(x) for x in commit_off]
        if any(x < 0 or x >= 1 << 32 for x in off):
            raise ValueError("commit offsets are uint32")
        nc = max(len(off) - 1, 0)
        return nc, (ctypes.c_uint32 * max(len(off), 1))(*off)

    def _commits_out(self, nc, n):
        return ctypes.create_string_buffer(max(nc, 1)), ctypes.create_string_buffer(max(n, 1)), ctypes.c_int(0)

    @staticmethod
    def _commits_result(rc, nc, n, out):
        return rc, list(out[0].raw[:nc]), list(out[1].raw[:n]), out[2].value

    # The forms' own arguments as _commits_call and _quorum_call take them: (nc, n, the arguments
    # between ctx and z_seed, whatever else they point into).
    def _commits_host(self, commit_off, sigs, vks, key_idx, msgs, ks):
        n = len(sigs)
        nc, off = self._commit_offsets(commit_off)
        vkb, idx = _tmpl_keys(n, vks, key_idx)
        arena, moff = _arena(msgs) if msgs is not None else (None, None)
        kb = None if ks is None else (b"".join(ks) or b"\0")
        return nc, n, (nc, off, vkb, idx, b"".join(sigs) or b"\0", arena, moff, kb)

    def _commits_device(self, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k):
        nc, off = self._commit_offsets(commit_off)
        p = self._dev_ptr
        return nc, off[nc] if nc else 0, (nc, off, p(d_vk), p(d_sig), p(d_msg), p(d_msg_off), p(d_k))

    # Template variants: every commit owns the window [commit_tpl[c], commit_tpl[c] + alt_span) of the
    # set and item i takes template commit_tpl[c] + item_alt[i] (item_alt None: all zeros).
    @staticmethod
    def _item_alt(item_alt):
        if item_alt is None:
            return None
        if any(not 0 <= int(a) <= 255 for a in item_alt):
            raise ValueError("item_alt entries are uint8")
        return bytes(bytearray(int(a) for a in item_alt)) or b"\0"

    def _commits_tmpl_host(self, templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off, alt=None):
        """alt: None for the one-template forms, (alt_span, item_alt) for the forms with variants."""
        n = len(sigs)
        nc, off = self._commit_offsets(commit_off)
        ts, keep = templates.struct()
        _, var, voff = _tmpl_items([0] * n, holes, var_off)
        ctpl = (ctypes.c_uint16 * max(nc, 1))(*commit_tpl)
        vkb, idx = _tmpl_keys(n, vks, key_idx)
        variants = () if alt is None else (alt[0], self._item_alt(alt[1]))
        return nc, n, (ctypes.byref(ts), nc, off, ctpl, *variants, vkb, idx, b"".join(sigs) or b"\0", var, voff), keep

    @staticmethod
    def _dev_ptr(x):
        """A device pointer given as an int, None, or a torch tensor (its data_ptr())."""
        return x.data_ptr() if hasattr(x, "data_ptr") else x

    def _commits_tmpl_device(self, templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var, d_var_off,
                             var_bytes):
        nc, off = self._commit_offsets(commit_off)
        ts, keep = templates.struct()
        ctpl = (ctypes.c_uint16 * max(nc, 1))(*commit_tpl)
        p = self._dev_ptr
        return nc, off[nc] if nc else 0, (ctypes.byref(ts), nc, off, ctpl, alt_span, p(d_item_alt), p(d_vk), p(d_sig),
                                          p(d_var), p(d_var_off), var_bytes), (keep, d_item_alt, d_vk, d_sig, d_var, d_var_off)

    def _commits_call(self, fn, form, z_seed, submit=False):
        """A verify fn(ctx, *form's arguments, z_seed, <the three outputs>) -> the result tuple, or a
        submit fn(ctx, *form's arguments, z_seed) -> its ticket, recorded as (nc, n, keep) until
        commits_wait: keep is the form and the seed, all the entry may still read. A refused submit
        records nothing."""
        nc, n, args = form[:3]
        seed = bytes(z_seed)
        if submit:
            with self._lock:
                t = fn(self.ctx, *args, seed)
                if t < 0:
                    self._check(t)
                self._commits_inflight[t] = (nc, n, (form, seed))
            return t
        out = self._commits_out(nc, n)
        with self._lock:
            rc = fn(self.ctx, *args, seed, out[0], out[1], ctypes.byref(out[2]))
        self._check(rc)
        return self._commits_result(rc, nc, n, out)

    def commits_verify(self, commit_off, sigs, z_seed, vks=None, key_idx=None, msgs=None, ks=None):
        """edc_commits_verify: host buffers, synchronous. Exactly one of vks and key_idx (positions
        in the last keycache_load list), exactly one of msgs and ks (prehashed)."""
        return self._commits_call(self.lib.edc_commits_verify, self._commits_host(commit_off, sigs, vks, key_idx, msgs, ks),
                                  z_seed)

    def commits_submit(self, commit_off, sigs, z_seed, vks=None, key_idx=None, msgs=None, ks=None):
        """edc_commits_submit: a ticket for commits_wait; the host buffers are kept alive here until then."""
        return self._commits_call(self.lib.edc_commits_submit, self._commits_host(commit_off, sigs, vks, key_idx, msgs, ks),
                                  z_seed, submit=True)

    def commits_verify_templated(self, templates, commit_off, commit_tpl, sigs, holes, z_seed, vks=None, key_idx=None,
                                 var_off=None):
        """edc_tmpl_commits_verify: one template per commit (commit_tpl[c]); the items carry their
        signature, hole and key or key index."""
        form = self._commits_tmpl_host(templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off)
        return self._commits_call(self.lib.edc_tmpl_commits_verify, form, z_seed)

    def commits_submit_templated(self, templates, commit_off, commit_tpl, sigs, holes, z_seed, vks=None, key_idx=None,
                                 var_off=None):
        """edc_tmpl_commits_submit: a ticket for commits_wait."""
        form = self._commits_tmpl_host(templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off)
        return self._commits_call(self.lib.edc_tmpl_commits_submit, form, z_seed, submit=True)

    def commits_verify_templated_alt(self, templates, commit_off, commit_tpl, alt_span, item_alt, sigs, holes, z_seed,
                                     vks=None, key_idx=None, var_off=None):
        """edc_tmpl_commits_verify_alt: commits_verify_templated with a variant byte per item."""
        form = self._commits_tmpl_host(templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off,
                                       (alt_span, item_alt))
        return self._commits_call(self.lib.edc_tmpl_commits_verify_alt, form, z_seed)

    def commits_submit_templated_alt(self, templates, commit_off, commit_tpl, alt_span, item_alt, sigs, holes, z_seed,
                                     vks=None, key_idx=None, var_off=None):
        """edc_tmpl_commits_submit_alt: a ticket for commits_wait."""
        form = self._commits_tmpl_host(templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off,
                                       (alt_span, item_alt))
        return self._commits_call(self.lib.edc_tmpl_commits_submit_alt, form, z_seed, submit=True)

    def commits_verify_templated_device(self, templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig,
                                        d_var, d_var_off, var_bytes, z_seed):
        """edc_tmpl_commits_verify_device: keys, signatures, holes and variant bytes as torch tensors
        or device pointers (ints; d_item_alt None: all zeros); commit_off, commit_tpl and the set on the host."""
        form = self._commits_tmpl_device(templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                         d_var_off, var_bytes)
        return self._commits_call(self.lib.edc_tmpl_commits_verify_device, form, z_seed)

    def commits_submit_templated_device(self, templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig,
                                        d_var, d_var_off, var_bytes, z_seed):
        """edc_tmpl_commits_submit_device: a ticket for commits_wait; the device arrays (kept alive
        here when given as tensors) stay the caller's until then."""
        form = self._commits_tmpl_device(templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                         d_var_off, var_bytes)
        return self._commits_call(self.lib.edc_tmpl_commits_submit_device, form, z_seed, submit=True)

    def commits_verify_device(self, commit_off, d_vk, d_sig, d_msg, d_msg_off, z_seed, d_k=None):
        """edc_commits_verify_device (device pointers as ints; d_k given: the messages are not read)."""
        return self._commits_call(self.lib.edc_commits_verify_device,
                                  self._commits_device(commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k), z_seed)

    def commits_submit_device(self, commit_off, d_vk, d_sig, d_msg, d_msg_off, z_seed, d_k=None):
        """edc_commits_submit_device: a ticket for commits_wait; the device arrays stay the caller's."""
        return self._commits_call(self.lib.edc_commits_submit_device,
                                  self._commits_device(commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k), z_seed, submit=True)

    def commits_wait(self, ticket):
        """edc_commits_wait: the results of a submitted commit set; a failed union runs its
        fallback here, on the ticket's own slot. The ticket's host buffers are released."""
        with self._lock:
            if ticket not in self._commits_inflight:
                raise EngineError(f"ticket {ticket} is not a commit-set ticket in flight")
            nc, n = self._commits_inflight[ticket][:2]
            out = self._commits_out(nc, n)
            rc = self.lib.edc_commits_wait(self.ctx, ticket, out[0], out[1], ctypes.byref(out[2]))
            self._commits_inflight.pop(ticket, None)
        self._check(rc)
        return self._commits_result(rc, nc, n, out)

    # ---- quorum commit sets (edc_quorum_*): tally voting power, verify only the votes needed ----
    # powers / flags: one per item; thresholds: one per commit; light: EDC_QUORUM_LIGHT, else _FULL.
    @staticmethod
    def _quorum_votes(n, nc, powers, flags, thresholds):
        powers, flags, thresholds = [int(x) for x in powers], [int(x) for x in flags], [int(x) for x in thresholds]
        if len(powers) != n or len(flags) != n or len(thresholds) != nc:
            raise ValueError("one power and flag per item, one threshold per commit")
        if any(x < 0 or x >= 1 << 64 for x in powers + thresholds) or any(x < 0 or x > 255 for x in flags):
            raise ValueError("powers and thresholds are uint64, flags uint8")
        return ((ctypes.c_uint64 * max(n, 1))(*powers), bytes(flags) or b"\0",
                (ctypes.c_uint64 * max(nc, 1))(*thresholds))

    def quorum_plan(self, commit_off, powers, flags, thresholds, light=True):
        """edc_quorum_plan: the selection alone -> ([checked 0/1 per item], [planned tally per commit], n_checked)."""
        nc, off = self._commit_offsets(commit_off)
        n = off[nc] if nc else 0
        pw, fl, th = self._quorum_votes(n, nc, powers, flags, thresholds)
        checked = ctypes.create_string_buffer(max(n, 1))
        planned = (ctypes.c_uint64 * max(nc, 1))()
        cnt = ctypes.c_size_t(0)
        with self._lock:
            rc = self.lib.edc_quorum_plan(self.ctx, nc, off, pw, fl, th, int(bool(light)), checked, planned,
                                          ctypes.byref(cnt))
        self._check(rc)
        return list(checked.raw[:n]), list(planned[:nc]), cnt.value

    @staticmethod
    def _quorum_thresholds(nc, thresholds):
        thresholds = [int(x) for x in thresholds]
        if len(thresholds) != nc:
            raise ValueError("one threshold per commit")
        return (ctypes.c_uint64 * max(nc, 1))(*thresholds)

    @staticmethod
    def _quorum_result(rc, nc, n, out, cached):
        res = {"code": rc, "commit_verdicts": list(out[0].raw[:nc]), "item_verdicts": list(out[1].raw[:n]),
               "tally": list(out[2][:nc]), "n_bad_commits": out[3].value, "n_checked": out[4].value,
               "check8": out[6].raw}
        if cached:
            res["n_miss"] = out[5].value
        return res

    def _quorum_call(self, fn, cached, form, votes, z_seed, light):
        """fn(ctx, *form's arguments, power, flag, threshold, mode, z_seed, <out-parameters>) -> the
        result dict. form: (nc, n, the arguments, whatever they point into); votes: (power, flag,
        threshold) as fn takes them. A cached fn has the miss out-parameter and its dict the n_miss key."""
        nc, n, args = form[:3]
        out = (ctypes.create_string_buffer(max(nc, 1)), ctypes.create_string_buffer(max(n, 1)),
               (ctypes.c_uint64 * max(nc, 1))(), ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0),
               ctypes.create_string_buffer(32))
        counts = [ctypes.byref(x) for x in out[3:6 if cached else 5]]
        with self._lock:
            rc = fn(self.ctx, *args, *votes, int(bool(light)), bytes(z_seed), out[0], out[1], out[2], *counts, out[6])
        self._check(rc)
        return self._quorum_result(rc, nc, n, out, cached)

    def _quorum_host(self, fn, cached, form, powers, flags, thresholds, z_seed, light):
        """The host call shape: powers, flags and thresholds are sequences."""
        return self._quorum_call(fn, cached, form, self._quorum_votes(form[1], form[0], powers, flags, thresholds), z_seed,
                                 light)

    def _quorum_device(self, fn, cached, form, d_power, d_flag, thresholds, z_seed, light):
        """The device call shape: powers and flags are on the device, thresholds a sequence."""
        votes = self._dev_ptr(d_power), self._dev_ptr(d_flag), self._quorum_thresholds(form[0], thresholds)
        return self._quorum_call(fn, cached, form, votes, z_seed, light)

    def quorum_verify(self, commit_off, sigs, powers, flags, thresholds, z_seed, light=True, vks=None, key_idx=None,
                      msgs=None, ks=None):
        """edc_quorum_verify: host buffers, synchronous. Exactly one of vks and key_idx, exactly one
        of msgs and ks, as commits_verify. Returns a dict: code, commit_verdicts, item_verdicts
        (NOT_CHECKED for the votes left out), tally, n_bad_commits, n_checked, check8."""
        form = self._commits_host(commit_off, sigs, vks, key_idx, msgs, ks)
        return self._quorum_host(self.lib.edc_quorum_verify, False, form, powers, flags, thresholds, z_seed, light)

    def quorum_verify_device(self, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_power, d_flag, thresholds, z_seed,
                             light=True, d_k=None):
        """edc_quorum_verify_device: the items, powers (uint64) and flags (uint8) as torch tensors or
        device pointers; commit_off and thresholds on the host. d_k given: the messages are not read."""
        form = self._commits_device(commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k)
        return self._quorum_device(self.lib.edc_quorum_verify_device, False, form, d_power, d_flag, thresholds, z_seed, light)

    # ---- templated quorum commit sets (edc_tmpl_quorum_*): select first, hash only the checked votes ----
    def quorum_verify_templated(self, templates, commit_off, commit_tpl, sigs, holes, powers, flags, thresholds, z_seed,
                                light=True, alt_span=1, item_alt=None, vks=None, key_idx=None, var_off=None):
        """edc_tmpl_quorum_verify: host buffers, synchronous; templates, commit_tpl, alt_span, item_alt
        and holes as commits_verify_templated_alt, powers / flags / thresholds as quorum_verify.
        Exactly one of vks and key_idx. Returns the dict quorum_verify returns."""
        form = self._commits_tmpl_host(templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off,
                                       (alt_span, item_alt))
        return self._quorum_host(self.lib.edc_tmpl_quorum_verify, False, form, powers, flags, thresholds, z_seed, light)

    def quorum_verify_templated_device(self, templates, commit_off, commit_tpl, d_vk, d_sig, d_var, d_var_off, var_bytes,
                                       d_power, d_flag, thresholds, z_seed, light=True, alt_span=1, d_item_alt=None):
        """edc_tmpl_quorum_verify_device: keys, signatures, holes, variant bytes, powers (uint64) and
        flags (uint8) as torch tensors or device pointers (d_item_alt None: all zeros); commit_off,
        commit_tpl, thresholds and the set on the host. Returns the dict quorum_verify returns."""
        form = self._commits_tmpl_device(templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                         d_var_off, var_bytes)
        return self._quorum_device(self.lib.edc_tmpl_quorum_verify_device, False, form, d_power, d_flag, thresholds, z_seed,
                                   light)

    # ---- cached quorum commit sets (edc_cached_*): checked votes that are live records of the
    # verified-signature table (sigcache_create) are not verified again; the results gain n_miss ----
    def quorum_verify_cached(self, commit_off, sigs, powers, flags, thresholds, z_seed, light=True, vks=None,
                             key_idx=None, msgs=None, ks=None):
        """edc_cached_quorum_verify: quorum_verify through the verified-signature table. Returns
        quorum_verify's dict plus n_miss, the size of the list that was verified."""
        form = self._commits_host(commit_off, sigs, vks, key_idx, msgs, ks)
        return self._quorum_host(self.lib.edc_cached_quorum_verify, True, form, powers, flags, thresholds, z_seed, light)

    def quorum_verify_cached_device(self, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_power, d_flag, thresholds, z_seed,
                                    light=True, d_k=None):
        """edc_cached_quorum_verify_device: quorum_verify_device through the verified-signature table."""
        form = self._commits_device(commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k)
        return self._quorum_device(self.lib.edc_cached_quorum_verify_device, True, form, d_power, d_flag, thresholds, z_seed,
                                   light)

    def quorum_verify_templated_cached(self, templates, commit_off, commit_tpl, sigs, holes, powers, flags, thresholds,
                                       z_seed, light=True, alt_span=1, item_alt=None, vks=None, key_idx=None,
                                       var_off=None):
        """edc_cached_tmpl_quorum_verify: quorum_verify_templated through the verified-signature table."""
        form = self._commits_tmpl_host(templates, commit_off, commit_tpl, sigs, holes, vks, key_idx, var_off,
                                       (alt_span, item_alt))
        return self._quorum_host(self.lib.edc_cached_tmpl_quorum_verify, True, form, powers, flags, thresholds, z_seed, light)

    def quorum_verify_templated_cached_device(self, templates, commit_off, commit_tpl, d_vk, d_sig, d_var, d_var_off,
                                              var_bytes, d_power, d_flag, thresholds, z_seed, light=True, alt_span=1,
                                              d_item_alt=None):
        """edc_cached_tmpl_quorum_verify_device: quorum_verify_templated_device through the
        verified-signature table."""
        form = self._commits_tmpl_device(templates, commit_off, commit_tpl, alt_span, d_item_alt, d_vk, d_sig, d_var,
                                         d_var_off, var_bytes)
        return self._quorum_device(self.lib.edc_cached_tmpl_quorum_verify_device, True, form, d_power, d_flag, thresholds,
                                   z_seed, light)

    def cached_quorum_last(self):
        """edc_debug_cached_quorum_last: (n, n_checked, hits among the checked, n_miss, items SHA-512
        ran over, records inserted) of the last cached quorum call on this engine."""
        out = (ctypes.c_uint64 * 6)()
        with self._lock:
            rc = self.lib.edc_debug_cached_quorum_last(self.ctx, out)
        self._check(rc)
        return tuple(out)

    def tmpl_quorum_last(self):
        """edc_debug_tmpl_quorum_last: (n, n_checked, items expanded and hashed, arena bytes assembled)
        of the last templated quorum call on this engine."""
        out = (ctypes.c_uint64 * 4)()
        with self._lock:
            rc = self.lib.edc_debug_tmpl_quorum_last(self.ctx, out)
        self._check(rc)
        return tuple(out)

    # ---- validator-set quorum commit sets (edc_valset_*): the powers are the registered list's, the
    # join of the votes against it and the double-vote check run on the GPU ----
    def valset_set_powers(self, powers):
        """edc_valset_set_powers: one power per position of the last keycache_load list; None or []
        clears them. Returns the member count."""
        powers = [int(x) for x in (powers or [])]
        if any(x < 0 or x >= 1 << 64 for x in powers):
            raise ValueError("powers are uint64")
        pw = (ctypes.c_uint64 * len(powers))(*powers) if powers else None
        with self._lock:
            self._check(self.lib.edc_valset_set_powers(self.ctx, len(powers), pw))
        return self.valset_size()

    def valset_size(self):
        return int(self.lib.edc_valset_size(self.ctx))

    @staticmethod
    def _valset_flags(n, flags):
        flags = [int(x) for x in flags]
        if len(flags) != n:
            raise ValueError("one flag per item")
        if any(x < 0 or x > 255 for x in flags):
            raise ValueError("flags are uint8")
        return bytes(flags) or b"\0"

    def valset_resolve(self, commit_off, flags, thresholds, light=True, vks=None, key_idx=None):
        """edc_valset_resolve: the join, the selection and the double-vote scan alone -> a dict: pos
        (NO_POS for a signer that is no member), power, flag, checked, planned, n_checked, dv."""
        return self._valset_resolve(self.lib.edc_valset_resolve, commit_off, None, flags, thresholds, light, vks, key_idx)

    def _valset_args(self, commit_off, versions, flags, thresholds, vks, key_idx, trust_versions=None,
                     trust_thresholds=None):
        """(nc, n, the arguments the resolve entries and the timing hooks take between nc and mode):
        the offsets, the commits' versions (None: the one set; a pair's trust versions behind them),
        the keys, the flags and the thresholds (a pair's trust thresholds behind them)."""
        nc, off = self._commit_offsets(commit_off)
        n = off[nc] if nc else 0
        ver = [self._vhist_versions_arg(nc, v) for v in (versions, trust_versions) if v is not None]
        vkb, idx = _tmpl_keys(n, vks, key_idx)
        fl = self._valset_flags(n, flags)
        th = [self._quorum_thresholds(nc, t) for t in (thresholds, trust_thresholds) if t is not None]
        return nc, n, (off, *ver, vkb, idx, fl, *th)

    @staticmethod
    def _valset_side(nc, n):
        """One side's outputs of a resolve entry (pos, power, flag_out, checked, planned, dv) and the
        function that turns them into that side's dict after the call."""
        o = ((ctypes.c_uint32 * max(n, 1))(), (ctypes.c_uint64 * max(n, 1))(), ctypes.create_string_buffer(max(n, 1)),
             ctypes.create_string_buffer(max(n, 1)), (ctypes.c_uint64 * max(nc, 1))(), ctypes.create_string_buffer(max(nc, 1)))

        def result():
            return {"pos": list(o[0][:n]), "power": list(o[1][:n]), "flag": list(o[2].raw[:n]),
                    "checked": list(o[3].raw[:n]), "planned": list(o[4][:nc]), "dv": list(o[5].raw[:nc])}
        return o, result

    def _valset_resolve(self, fn, commit_off, versions, flags, thresholds, light, vks, key_idx):
        """fn: edc_valset_resolve (versions None) or edc_vhist_resolve, which takes them behind the offsets"""
        nc, n, args = self._valset_args(commit_off, versions, flags, thresholds, vks, key_idx)
        o, result = self._valset_side(nc, n)
        cnt = ctypes.c_size_t(0)
        with self._lock:
            rc = fn(self.ctx, nc, *args, int(bool(light)), *o[:5], ctypes.byref(cnt), o[5])
        self._check(rc)
        return dict(result(), n_checked=cnt.value)

    def quorum_verify_valset(self, commit_off, sigs, flags, thresholds, z_seed, light=True, vks=None, key_idx=None,
                             msgs=None, ks=None):
        """edc_valset_quorum_verify: quorum_verify with the powers of the registered validator set
        (valset_set_powers). A commit with two checked votes of one member is EDC_DOUBLE_VOTE.
        Returns the dict quorum_verify returns."""
        form = self._commits_host(commit_off, sigs, vks, key_idx, msgs, ks)
        votes = self._valset_flags(form[1], flags), self._quorum_thresholds(form[0], thresholds)
        return self._quorum_call(self.lib.edc_valset_quorum_verify, False, form, votes, z_seed, light)

    def quorum_verify_valset_device(self, commit_off, d_vk, d_sig, d_msg, d_msg_off, d_flag, thresholds, z_seed,
                                    light=True, d_k=None):
        """edc_valset_quorum_verify_device: quorum_verify_device without d_power."""
        form = self._commits_device(commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k)
        votes = self._dev_ptr(d_flag), self._quorum_thresholds(form[0], thresholds)
        return self._quorum_call(self.lib.edc_valset_quorum_verify_device, False, form, votes, z_seed, light)

    def valset_select_ms(self, commit_off, flags, thresholds, light=True, vks=None, key_idx=None, reps=20):
        """edc_debug_valset_select: mean times of the join kernel and of the double-vote scan, in milliseconds."""
        nc, _, args = self._valset_args(commit_off, None, flags, thresholds, vks, key_idx)
        ms = (ctypes.c_float * 2)()
        with self._lock:
            rc = self.lib.edc_debug_valset_select(self.ctx, nc, *args, int(bool(light)), reps, ms)
        self._check(rc)
        return ms[0], ms[1]

    # ---- validator-set history (edc_vhist_*): a base set plus per-version updates; every commit is
    # judged by the set of the version it names ----
    def vhist_set(self, base_powers, updates=()):
        """edc_vhist_set: base_powers, one per position of the last keycache_load list (VHIST_NOT_MEMBER
        or None: no member), and updates, one list of (position, power) pairs per version 1..nv.
        base_powers None or []: clears the history. Returns the number of versions."""
        def u64(x):
            x = VHIST_NOT_MEMBER if x is None else int(x)
            if x < 0 or x >= 1 << 64:
                raise ValueError("powers are uint64")
            return x
        base = [u64(x) for x in (base_powers or [])]
        updates = [[(int(p), u64(w)) for p, w in u] for u in updates]
        flat = [x for u in updates for x in u]
        if any(p < 0 or p >= 1 << 32 for p, _ in flat) or len(flat) >= 1 << 32:
            raise ValueError("update positions and their count are uint32")
        if not base:
            if updates:
                raise ValueError("updates without a base set")
            args = (0, None, 0, None, None, None)
        else:
            off = [0]
            for u in updates:
                off.append(off[-1] + len(u))
            args = (len(base), (ctypes.c_uint64 * len(base))(*base), len(updates), (ctypes.c_uint32 * len(off))(*off),
                    (ctypes.c_uint32 * max(len(flat), 1))(*[p for p, _ in flat]),
                    (ctypes.c_uint64 * max(len(flat), 1))(*[w for _, w in flat]))
        with self._lock:
            self._check(self.lib.edc_vhist_set(self.ctx, *args))
        return self.vhist_versions()

    def vhist_versions(self):
        return int(self.lib.edc_vhist_versions(self.ctx))

    def vhist_totals(self, v0=0, count=None):
        """edc_vhist_totals -> (totals, member counts) of the versions v0 .. v0 + count - 1 (count None:
        up to the last)."""
        if count is None:
            count = max(self.vhist_versions() - v0, 0)
        total, members = (ctypes.c_uint64 * max(count, 1))(), (ctypes.c_uint32 * max(count, 1))()
        self._check(self.lib.edc_vhist_totals(self.ctx, v0, count, total, members))
        return list(total[:count]), list(members[:count])

    # ---- validator-set hashes (edc_valhash_*): the Merkle root of a set, as include/edc.h states it ----
    def valset_hash(self):
        """edc_valhash_valset: the 32-byte root of the one set of valset_set_powers."""
        out = ctypes.create_string_buffer(32)
        with self._lock:
            self._check(self.lib.edc_valhash_valset(self.ctx, out))
        return out.raw

    def vhist_hashes(self, v0=0, count=None):
        """edc_valhash_vhist -> the roots of the versions v0 .. v0 + count - 1 of the history (count
        None: up to the last), 32 bytes each."""
        if count is None:
            count = max(self.vhist_versions() - v0, 0)
        out = ctypes.create_string_buffer(max(32 * count, 1))
        with self._lock:
            self._check(self.lib.edc_valhash_vhist(self.ctx, v0, count, out))
        return [out.raw[32 * j:32 * j + 32] for j in range(count)]

    def vhist_hash_match(self, commit_versions, expect):
        """edc_valhash_vhist_match: expect[c] (32 bytes, the validators_hash of commit c's header) against
        the root of version commit_versions[c], compared on the device -> (ok, n_mismatch): one
        0 / 1 per commit and the number of zeros."""
        expect = [bytes(e) for e in expect]
        nc = len(expect)
        if any(len(e) != 32 for e in expect):
            raise InvalidSliceLength("expect: 32 bytes per commit")
        ver = self._vhist_versions_arg(nc, commit_versions)
        ok, bad = ctypes.create_string_buffer(max(nc, 1)), ctypes.c_size_t(0)
        with self._lock:
            self._check(self.lib.edc_valhash_vhist_match(self.ctx, nc, ver, b"".join(expect) or b"\0", ok, ctypes.byref(bad)))
        return list(ok.raw[:nc]), int(bad.value)

    def valhash_ms(self, reps=20):
        """edc_debug_valhash_ms: mean times (ms) of the root kernel over every version of the history
        and of the address kernel over the registered list."""
        ms = (ctypes.c_float * 2)()
        with self._lock:
            self._check(self.lib.edc_debug_valhash_ms(self.ctx, reps, ms))
        return {"roots": float(ms[0]), "addresses": float(ms[1])}

    # ---- header hashes (edc_header_*): the Merkle root of a header given as its ordered leaves ----
    @staticmethod
    def _header_set(headers):
        """headers: a list of lists of bytes -> (EdcHeaderSet, the buffers it points into)"""
        headers = [[bytes(x) for x in h] for h in headers]
        leaf_off, byte_off = [0], [0]
        for h in headers:
            leaf_off.append(leaf_off[-1] + len(h))
            for x in h:
                byte_off.append(byte_off[-1] + len(x))
        if leaf_off[-1] >= 1 << 32 or byte_off[-1] >= 1 << 32:
            raise ValueError("leaf and byte offsets are uint32")
        lo, bo = (ctypes.c_uint32 * len(leaf_off))(*leaf_off), (ctypes.c_uint32 * len(byte_off))(*byte_off)
        data = ctypes.create_string_buffer(b"".join(x for h in headers for x in h), max(byte_off[-1], 1))
        hs = EdcHeaderSet(ctypes.sizeof(EdcHeaderSet), 0, len(headers), ctypes.addressof(lo), ctypes.addressof(bo),
                          ctypes.addressof(data) if byte_off[-1] else None)
        return hs, (lo, bo, data)

    def header_hashes(self, headers):
        """edc_header_hashes: headers, a list of lists of bytes (each header's ordered leaves) -> the
        32-byte Merkle root of each."""
        hs, keep = self._header_set(headers)
        nh = len(headers)
        out = ctypes.create_string_buffer(max(32 * nh, 1))
        with self._lock:
            self._check(self.lib.edc_header_hashes(self.ctx, ctypes.byref(hs), out))
        return [out.raw[32 * h:32 * h + 32] for h in range(nh)]

    def header_bind(self, headers, expect=None, vals=None, nexts=None, link=None, vals_at=(7, 2), next_at=(8, 2),
                    link_at=(4, 2)):
        """edc_header_bind: hashes every header and holds it to the rules given. expect: 32 bytes per
        header; vals / nexts: per header the history version whose validator-set root the header
        names at (leaf, position) vals_at / next_at; link: per header the index of the header of this
        list whose root it names at link_at. None in place of a list: no such rule; None (or
        HEADER_NONE) as an entry: that header is skipped. -> (bad, n_bad, roots): per header the
        HEADER_BAD_* bits, the number of non-zero ones, the 32-byte roots."""
        hs, keep = self._header_set(headers)
        nh = len(headers)

        def u32s(name, xs):
            if xs is None:
                return None
            xs = [HEADER_NONE if x is None else int(x) for x in xs]
            if len(xs) != nh:
                raise ValueError("%s: one entry per header" % name)
            if any(x < 0 or x >= 1 << 32 for x in xs):
                raise ValueError("%s: entries are uint32" % name)
            return (ctypes.c_uint32 * max(nh, 1))(*xs)
        exp = None
        if expect is not None:
            expect = [bytes(e) for e in expect]
            if len(expect) != nh or any(len(e) != 32 for e in expect):
                raise InvalidSliceLength("expect: 32 bytes per header")
            exp = ctypes.create_string_buffer(b"".join(expect), max(32 * nh, 1))
        arrs = [u32s("vals", vals), u32s("nexts", nexts), u32s("link", link)]
        addr = lambda a: ctypes.addressof(a) if a is not None else None
        r = EdcHeaderRules(ctypes.sizeof(EdcHeaderRules), 0, addr(exp), addr(arrs[0]), vals_at[0], vals_at[1],
                           addr(arrs[1]), next_at[0], next_at[1], addr(arrs[2]), link_at[0], link_at[1])
        bad, out, n_bad = ctypes.create_string_buffer(max(nh, 1)), ctypes.create_string_buffer(max(32 * nh, 1)), ctypes.c_size_t(0)
        with self._lock:
            self._check(self.lib.edc_header_bind(self.ctx, ctypes.byref(hs), ctypes.byref(r), bad, out, ctypes.byref(n_bad)))
        return list(bad.raw[:nh]), int(n_bad.value), [out.raw[32 * h:32 * h + 32] for h in range(nh)]

    def header_ms(self, headers, reps=20):
        """edc_debug_header_ms: mean times (ms) of the root kernel and of the bind kernel over headers."""
        hs, keep = self._header_set(headers)
        ms = (ctypes.c_float * 2)()
        with self._lock:
            self._check(self.lib.edc_debug_header_ms(self.ctx, ctypes.byref(hs), reps, ms))
        return {"roots": float(ms[0]), "bind": float(ms[1])}

    @staticmethod
    def _vhist_versions_arg(nc, versions):
        versions = [int(v) for v in versions]
        if len(versions) != nc:
            raise ValueError("one version per commit")
        if any(v < 0 or v >= 1 << 32 for v in versions):
            raise ValueError("versions are uint32")
        return (ctypes.c_uint32 * max(nc, 1))(*versions)

    def _vhist_form(self, form, versions):
        """form with the commits' versions behind the offsets, as the edc_vhist_* entries take them"""
        nc, n, args = form
        return nc, n, args[:2] + (self._vhist_versions_arg(nc, versions),) + args[2:]

    def vhist_resolve(self, commit_off, versions, flags, thresholds, light=True, vks=None, key_idx=None):
        """edc_vhist_resolve: valset_resolve with every commit judged at its own version."""
        return self._valset_resolve(self.lib.edc_vhist_resolve, commit_off, versions, flags, thresholds, light, vks,
                                    key_idx)

    def quorum_verify_vhist(self, commit_off, versions, sigs, flags, thresholds, z_seed, light=True, vks=None,
                            key_idx=None, msgs=None, ks=None):
        """edc_vhist_quorum_verify: quorum_verify_valset with commit c judged by version versions[c] of
        the validator-set history (vhist_set). Returns the dict quorum_verify returns."""
        form = self._vhist_form(self._commits_host(commit_off, sigs, vks, key_idx, msgs, ks), versions)
        votes = self._valset_flags(form[1], flags), self._quorum_thresholds(form[0], thresholds)
        return self._quorum_call(self.lib.edc_vhist_quorum_verify, False, form, votes, z_seed, light)

    def quorum_verify_vhist_device(self, commit_off, versions, d_vk, d_sig, d_msg, d_msg_off, d_flag, thresholds, z_seed,
                                   light=True, d_k=None):
        """edc_vhist_quorum_verify_device: quorum_verify_valset_device with the commits' versions (host)."""
        form = self._vhist_form(self._commits_device(commit_off, d_vk, d_sig, d_msg, d_msg_off, d_k), versions)
        votes = self._dev_ptr(d_flag), self._quorum_thresholds(form[0], thresholds)
        return self._quorum_call(self.lib.edc_vhist_quorum_verify_device, False, form, votes, z_seed, light)

    def vhist_select_ms(self, commit_off, versions, flags, thresholds, light=True, vks=None, key_idx=None, reps=20):
        """edc_debug_vhist_select: mean times of the history's join kernel and of the double-vote scan,
        in milliseconds."""
        nc, _, args = self._valset_args(commit_off, versions, flags, thresholds, vks, key_idx)
        ms = (ctypes.c_float * 2)()
        with self._lock:
            rc = self.lib.edc_debug_vhist_select(self.ctx, nc, *args, int(bool(light)), reps, ms)
        self._check(rc)
        return ms[0], ms[1]

    # ---- validator-set requests (edc_vq_verify): the validator-set and history entries, templates and
    # the verified-signature table behind one request ----
    def vq_verify(self, commit_off, flags, thresholds, z_seed, light=True, versions=None, cached=False, device=False,
                  vks=None, key_idx=None, sigs=None, msgs=None, ks=None, msg_off=None, templates=None, commit_tpl=None,
                  alt_span=1, item_alt=None, holes=None, var_off=None, var_bytes=None, raw=None, trust_versions=None,
                  trust_thresholds=None):
        """edc_vq_verify. device=False: vks / sigs / msgs / ks / holes are sequences of bytes, key_idx /
        flags / item_alt sequences of ints, as the sibling host methods take them. device=True: vks,
        sigs, flags, msgs (the arena, with msg_off), ks, item_alt, holes (the hole bytes) and var_off
        are torch tensors or device pointers, and var_bytes is given. commit_off, versions (None: the
        one set of valset_set_powers), thresholds, commit_tpl and templates are host values in both.
        Exactly one of vks and key_idx; exactly one of msgs, ks and templates. Returns the dict
        quorum_verify returns, with n_miss when cached. raw: a dict of request field -> value that
        overrides what was built (tests of the refusals).
        trust_versions / trust_thresholds (one per commit, host; NO_TRUST: that commit has no trusting
        side) make the request a trusting pair: every commit is also judged by the set of its trust
        version against its trust threshold, the union of the votes either side selects is verified
        once, and the dict gains trust_verdicts, trust_tally and n_bad_trust."""
        nc, off = self._commit_offsets(commit_off)
        n = off[nc] if nc else 0
        th = self._quorum_thresholds(nc, thresholds)
        ver = None if versions is None else self._vhist_versions_arg(nc, versions)
        tver = None if trust_versions is None else self._vhist_versions_arg(nc, trust_versions)
        tth = None if trust_thresholds is None else self._quorum_thresholds(nc, trust_thresholds)
        seed = bytes(z_seed)
        keep = [off, th, ver, seed, tver, tth]
        rq = EdcVqRequest(size=ctypes.sizeof(EdcVqRequest), device=int(bool(device)), mode=int(bool(light)),
                          cached=int(bool(cached)), nc=nc)

        def addr(x):
            if x is None:
                return None
            if device:
                return self._dev_ptr(x)
            keep.append(x)
            return ctypes.cast(x, ctypes.c_void_p).value if isinstance(x, bytes) else ctypes.addressof(x)

        rq.commit_off, rq.threshold, rq.z_seed = ctypes.addressof(off), ctypes.addressof(th), \
            ctypes.cast(seed, ctypes.c_void_p).value
        rq.commit_ver = None if ver is None else ctypes.addressof(ver)
        rq.trust_ver = None if tver is None else ctypes.addressof(tver)
        rq.trust_threshold = None if tth is None else ctypes.addressof(tth)
        if device:
            rq.vk, rq.sig, rq.flag, rq.msg, rq.msg_off, rq.k = (addr(x) for x in (vks, sigs, flags, msgs, msg_off, ks))
            if templates is not None:
                rq.item_alt, rq.var, rq.var_off, rq.var_bytes = addr(item_alt), addr(holes), addr(var_off), int(var_bytes)
            keep += [vks, sigs, flags, msgs, msg_off, ks, item_alt, holes, var_off]
        else:
            vkb, idx = _tmpl_keys(n, vks, key_idx)
            rq.vk, rq.key_idx = addr(vkb), addr(idx)
            rq.sig = addr(None if sigs is None else (b"".join(sigs) or b"\0"))
            rq.flag = addr(None if flags is None else self._valset_flags(n, flags))
            if msgs is not None:
                arena, moff = _arena(msgs)
                rq.msg, rq.msg_off = addr(arena), addr(moff)
            if ks is not None:
                rq.k = addr(b"".join(ks) or b"\0")
            if templates is not None:
                _, var, voff = _tmpl_items([0] * n, holes, var_off)
                rq.item_alt, rq.var, rq.var_off = addr(self._item_alt(item_alt)), addr(var), addr(voff)
        if templates is not None:
            ts, tkeep = templates.struct()
            ctpl = (ctypes.c_uint16 * max(nc, 1))(*commit_tpl)
            keep += [ts, tkeep, ctpl]
            rq.ts, rq.commit_tpl, rq.alt_span = ctypes.addressof(ts), ctypes.addressof(ctpl), int(alt_span)
        for name, value in (raw or {}).items():
            if name != "result_size":
                setattr(rq, name, value)
        out = (ctypes.create_string_buffer(max(nc, 1)), ctypes.create_string_buffer(max(n, 1)),
               (ctypes.c_uint64 * max(nc, 1))(), ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0),
               ctypes.create_string_buffer(32))
        tout = (ctypes.create_string_buffer(max(nc, 1)), (ctypes.c_uint64 * max(nc, 1))(), ctypes.c_int(0))
        rs = EdcVqResult(ctypes.sizeof(EdcVqResult), 0, *(ctypes.addressof(x) for x in out + tout))
        if raw and "result_size" in raw:
            rs.size = raw["result_size"]
        with self._lock:
            rc = self.lib.edc_vq_verify(self.ctx, ctypes.byref(rq), ctypes.byref(rs))
        self._check(rc)
        res = self._quorum_result(rc, nc, n, out, bool(cached))
        if rq.trust_ver:
            res.update(trust_verdicts=list(tout[0].raw[:nc]), trust_tally=list(tout[1][:nc]), n_bad_trust=tout[2].value)
        return res

    def vq_last(self):
        """edc_debug_vq_last: (n, n_checked, hits, n_miss, items SHA-512 ran over, records inserted, 0
        (reserved), arena bytes) of the last validator-set request on this engine."""
        out = (ctypes.c_uint64 * 8)()
        with self._lock:
            rc = self.lib.edc_debug_vq_last(self.ctx, out)
        self._check(rc)
        return tuple(out)

    def vq_trust_last(self):
        """edc_debug_vq_trust_last: (checked by A, checked by B, checked by both, union) of the last
        trusting pair that returned a verdict on this engine."""
        out = (ctypes.c_uint64 * 4)()
        with self._lock:
            rc = self.lib.edc_debug_vq_trust_last(self.ctx, out)
        self._check(rc)
        return tuple(out)

    def vq_trust_resolve(self, commit_off, versions, trust_versions, flags, thresholds, trust_thresholds, light=True,
                         vks=None, key_idx=None):
        """edc_vq_trust_resolve: the paired join, both selections, the union and both double-vote scans
        alone -> a dict: "a" and "b", each the dict vhist_resolve returns for that side (without
        n_checked), "side" (bit 0 checked by A, bit 1 checked by B) and "n_checked" (the union's)."""
        nc, n, args = self._valset_args(commit_off, versions, flags, thresholds, vks, key_idx, trust_versions,
                                        trust_thresholds)
        (a, result_a), (b, result_b) = self._valset_side(nc, n), self._valset_side(nc, n)
        side, cnt = ctypes.create_string_buffer(max(n, 1)), ctypes.c_size_t(0)
        with self._lock:
            rc = self.lib.edc_vq_trust_resolve(self.ctx, nc, *args, int(bool(light)),
                                               *(ctypes.addressof(x) for x in a + b + (side,)), ctypes.byref(cnt))
        self._check(rc)
        return {"a": result_a(), "b": result_b(), "side": list(side.raw[:n]), "n_checked": cnt.value}

    def vq_trust_select_ms(self, commit_off, versions, trust_versions, flags, thresholds, trust_thresholds, light=True,
                           vks=None, key_idx=None, reps=20):
        """edc_debug_vq_trust_select: mean milliseconds of the paired join, of both selections with the
        union and its scan, and of both double-vote scans."""
        nc, _, args = self._valset_args(commit_off, versions, flags, thresholds, vks, key_idx, trust_versions,
                                        trust_thresholds)
        ms = (ctypes.c_float * 3)()
        with self._lock:
            rc = self.lib.edc_debug_vq_trust_select(self.ctx, nc, *args, int(bool(light)), reps, ms)
        self._check(rc)
        return ms[0], ms[1], ms[2]

    def quorum_select_ms(self, commit_off, powers, flags, thresholds, light=True, reps=20):
        """edc_debug_quorum_select: mean time of the selection kernels alone, in milliseconds."""
        nc, off = self._commit_offsets(commit_off)
        n = off[nc] if nc else 0
        pw, fl, th = self._quorum_votes(n, nc, powers, flags, thresholds)
        ms = ctypes.c_float(0)
        with self._lock:
            rc = self.lib.edc_debug_quorum_select(self.ctx, nc, off, pw, fl, th, int(bool(light)), reps, ctypes.byref(ms))
        self._check(rc)
        return ms.value

    def batch_submit_multi_device(self, nb, n_per, d_vk, d_sig, d_msg, d_off, z_seed, z_base=0, d_k=None,
                                  want_check8=False):
        """nb consecutive batches of n_per items in one launch sequence (edc_batch_submit_multi_device);
        device pointers as ints. Returns a ticket for batch_wait_multi."""
        with self._lock:
            t = self.lib.edc_batch_submit_multi_device(self.ctx, nb, n_per, d_vk, d_sig, d_msg, d_off, d_k,
                                                       bytes(z_seed), z_base, 1 if want_check8 else 0)
        self._check(t)
        return t

    def batch_wait_multi(self, ticket, nb, want_partials=False):
        """(code, [verdict per batch], [check8 per batch], [partial per batch] or None, [bad per batch]).
        Asking for the partials makes a union-first launch run batch by batch (edc_set_multi_union)."""
        v = (ctypes.c_int * nb)()
        bad = (ctypes.c_int * nb)()
        c8 = ctypes.create_string_buffer(32 * nb)
        parts = ctypes.create_string_buffer(128 * nb) if want_partials else None
        with self._lock:
            rc = self.lib.edc_batch_wait_multi(self.ctx, ticket, nb, v, c8, parts, bad)
        self._check(rc)
        return (rc, list(v), [c8.raw[32 * g:32 * g + 32] for g in range(nb)],
                [parts.raw[128 * g:128 * g + 128] for g in range(nb)] if want_partials else None, list(bad))

    def set_multi_union(self, on):
        """Multi-batch launches verify the union of their batches first (default on)."""
        self._check(self.lib.edc_set_multi_union(self.ctx, 1 if on else 0))

    def multi_union_stats(self):
        """(union-first launches that passed, launches rerun batch by batch) on this context."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.edc_multi_union_stats(self.ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def batch_wait(self, ticket, want_check8=False):
        """Verdict of a submitted batch: (code, check8 or None); the ticket's host buffers are released."""
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self.lib.edc_batch_wait(self.ctx, ticket, check8, None, None)
            self._host_inflight.pop(ticket, None)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def verify_each(self, vks, sigs, msgs):
        n = len(vks)
        arena, offs = _arena(msgs)
        out = ctypes.create_string_buffer(max(n, 1))
        with self._lock:
            self._check(self.lib.edc_verify_each(self.ctx, n, *_joined(vks, sigs), arena, offs, out))
        return list(out.raw[:n])

    def verify_prehashed_each(self, vks, sigs, ks):
        n = len(vks)
        out = ctypes.create_string_buffer(max(n, 1))
        with self._lock:
            self._check(self.lib.edc_verify_prehashed_each(self.ctx, n, *_joined(vks, sigs, ks), out))
        return list(out.raw[:n])

    def challenge(self, vks, sigs, msgs):
        n = len(vks)
        arena, offs = _arena(msgs)
        out = ctypes.create_string_buffer(max(32 * n, 1))
        with self._lock:
            self._check(self.lib.edc_challenge(self.ctx, n, *_joined(vks, sigs), arena, offs, out))
        return [out.raw[32 * i:32 * i + 32] for i in range(n)]

    def decompress(self, encs):
        n = len(encs)
        xy = ctypes.create_string_buffer(max(64 * n, 1))
        ok = ctypes.create_string_buffer(max(n, 1))
        with self._lock:
            self._check(self.lib.edc_decompress(self.ctx, n, b"".join(encs) or b"\0", xy, ok))
        return [(bool(ok.raw[i]), xy.raw[64 * i:64 * i + 32], xy.raw[64 * i + 32:64 * i + 64]) for i in range(n)]

    def vk_validate(self, encs):
        """VerificationKey::try_from for many keys (src/verification_key.rs:160-175): codes 0 / 2."""
        n = len(encs)
        out = ctypes.create_string_buffer(max(n, 1))
        with self._lock:
            self._check(self.lib.edc_vk_validate(self.ctx, n, b"".join(encs) or b"\0", out))
        return list(out.raw[:n])

    def keycache_load(self, encs):
        """Register validator keys (decoded once per context, comb tables kept on the GPU).
        Returns (number of distinct keys cached, per-key ok list)."""
        n = len(encs)
        ok = ctypes.create_string_buffer(max(n, 1))
        with self._lock:
            u = self._check(self.lib.edc_keycache_load(self.ctx, n, b"".join(encs) or b"\0", ok))
            self._kc_keys = set(bytes(e) for e in encs)      # load caches every distinct key
        return u, [bool(b) for b in ok.raw[:n]]

    def keycache_add(self, encs):
        """Add keys to the context's cache without replacing it (a VerificationKey's decoded point,
        kept for every later verify: src/verification_key.rs:106-114). Returns (number of distinct
        keys now cached, per-key ok list)."""
        n = len(encs)
        ok = ctypes.create_string_buffer(max(n, 1))
        with self._lock:
            u = self._check(self.lib.edc_keycache_add(self.ctx, n, b"".join(encs) or b"\0", ok))
            oks = [bool(b) for b in ok.raw[:n]]
            self._kc_keys.update(bytes(e) for e, o in zip(encs, oks) if o)   # add keeps decodable keys only
        return u, oks

    def keycache_missing(self, encs):
        """The distinct keys of encs that the context's key cache does not hold yet (host-side
        mirror of the cache's key set, no device call)."""
        return set(bytes(e) for e in encs) - self._kc_keys

    def set_key_grouping(self, mode):
        """0 auto (default), 1 always group keys, 2 never (one A term per signature), 3 test mode:
        grouping abandoned on the device (the adversarial-key overflow path)."""
        self._check(self.lib.edc_set_key_grouping(self.ctx, int(mode)))

    def set_key_split(self, mode):
        """0 auto (default): split B / key coefficients at bit 128 onto the key cache's [2^128]A
        while the cache covers the batches' keys; 1 never."""
        self._check(self.lib.edc_set_key_split(self.ctx, int(mode)))

    def set_msm_shape(self, bits=0, parts=0):
        """Pippenger window width (8..16) and parts (1..64); 0 = chosen from the batch size."""
        self._check(self.lib.edc_set_msm_shape(self.ctx, int(bits), int(parts)))

    def set_msm_bin_entries(self, entries=0):
        """Target MSM entries per bin (>= 256); 0 = chosen from the batch size."""
        self._check(self.lib.edc_set_msm_bin_entries(self.ctx, int(entries)))

    def last_plan(self):
        """The MSM plan of the last batch on this context as a dict (edc_debug_last_plan; test hook):
        nwin, nwin_short, nranges, sum_ranges, bins_per_range, bits / nslice / nsub per window, the
        entry target finally used, and per_sig / split / few / fold. EngineError before any batch."""
        info = EdcPlanInfo()
        self._check(self.lib.edc_debug_last_plan(self.ctx, ctypes.byref(info)))
        return info.as_dict()

    def keycache_clear(self):
        with self._lock:
            self._check(self.lib.edc_keycache_clear(self.ctx))
            self._kc_keys = set()

    def keycache_size(self):
        return int(self.lib.edc_keycache_size(self.ctx))

    def sign(self, seeds, msgs, seed_index=None):
        n = len(msgs)
        arena, offs = _arena(msgs)
        vk = ctypes.create_string_buffer(max(32 * n, 1))
        sig = ctypes.create_string_buffer(max(64 * n, 1))
        idx = None
        if seed_index is not None:
            idx = (ctypes.c_uint32 * n)(*seed_index)
        with self._lock:
            self._check(self.lib.edc_sign(self.ctx, n, b"".join(seeds), len(seeds), idx, arena, offs, vk, sig))
        vkb, sgb = vk.raw, sig.raw    # one copy each (.raw copies the whole buffer on every access)
        return [vkb[32 * i:32 * i + 32] for i in range(n)], [sgb[64 * i:64 * i + 64] for i in range(n)]

    # ---- verified-signature cache (include/edc.h, edc_sigcache_*) ----
    def sigcache_create(self, capacity, keep=0):
        """A device table of `capacity` verified items (rounded up to a power of two), replacing any
        existing one; capacity 0 frees it. keep: generations a record stays alive (0: default, 2)."""
        with self._lock:
            self._check(self.lib.edc_sigcache_create(self.ctx, int(capacity), int(keep)))

    def sigcache_clear(self):
        with self._lock:
            self._check(self.lib.edc_sigcache_clear(self.ctx))

    def sigcache_advance(self):
        """Bump the table's generation (once per height)."""
        with self._lock:
            self._check(self.lib.edc_sigcache_advance(self.ctx))

    def sigcache_stats(self):
        out = (ctypes.c_uint64 * 6)()
        self._check(self.lib.edc_sigcache_stats(self.ctx, out))
        return dict(zip(("capacity", "generation", "hits", "misses", "inserted", "dropped"), (int(x) for x in out)))

    def sigcache_lookup(self, n, d_vk, d_sig, d_k, d_hit):
        """d_hit[i] = 1 iff item i is a live record (edc_sigcache_lookup_device; device pointers as
        ints, d_hit n bytes). Changes neither the table nor the counters."""
        with self._lock:
            self._check(self.lib.edc_sigcache_lookup_device(self.ctx, n, d_vk, d_sig, d_k, d_hit))

    @staticmethod
    def _msgs_or_ks(n, msgs, ks):
        if (msgs is None) == (ks is None):
            raise ValueError("cached verification takes either msgs or ks")
        if len(msgs if ks is None else ks) != n:
            raise ValueError("lists of different lengths")
        if ks is not None:
            return None, None, _joined(ks)[0]
        arena, offs = _arena(msgs)
        return arena, offs, None

    def batch_verify_cached(self, vks, sigs, msgs=None, ks=None, z_seed=None):
        """Batch verification of the items not verified before on this engine
        (edc_sigcache_batch_verify): (code, check8, n_miss). The misses, in queue order, are the
        batch; when it passes they are inserted. z_seed None: fresh OS randomness (it must be
        fresh and secret: include/edc.h, Soundness)."""
        n = len(vks)
        arena, offs, kb = self._msgs_or_ks(n, msgs, ks)
        seed = secrets.token_bytes(32) if z_seed is None else _as_bytes(z_seed, 32)
        check8 = ctypes.create_string_buffer(32)
        miss = ctypes.c_size_t(0)
        with self._lock:
            rc = self.lib.edc_sigcache_batch_verify(self.ctx, n, *_joined(vks, sigs), arena, offs, kb, seed, check8,
                                                    ctypes.byref(miss))
        self._check(rc)
        return rc, check8.raw, miss.value

    def batch_verify_cached_fallback(self, n, d_vk, d_sig, d_msg=None, d_msg_off=None, d_k=None, z_seed=None):
        """edc_sigcache_batch_verify_fallback_device on device-resident items (pointers as ints; d_k
        or the messages): (code, per-item Item::verify_single codes, n_invalid, check8, n_miss)."""
        seed = secrets.token_bytes(32) if z_seed is None else _as_bytes(z_seed, 32)
        check8 = ctypes.create_string_buffer(32)
        v = ctypes.create_string_buffer(max(n, 1))
        cnt = ctypes.c_int(0)
        miss = ctypes.c_size_t(0)
        with self._lock:
            rc = self.lib.edc_sigcache_batch_verify_fallback_device(self.ctx, n, d_vk, d_sig, d_msg, d_msg_off, d_k,
                                                                    seed, v, ctypes.byref(cnt), check8,
                                                                    ctypes.byref(miss))
        self._check(rc)
        return rc, list(v.raw[:n]), cnt.value, check8.raw, miss.value

    def verify_each_cached(self, vks, sigs, msgs=None, ks=None):
        """Per-item verification of the items not verified before (edc_sigcache_verify_each), the
        gossip-time feed of the table: (verdict codes, n_miss). Valid misses are inserted."""
        n = len(vks)
        arena, offs, kb = self._msgs_or_ks(n, msgs, ks)
        out = ctypes.create_string_buffer(max(n, 1))
        miss = ctypes.c_size_t(0)
        with self._lock:
            self._check(self.lib.edc_sigcache_verify_each(self.ctx, n, *_joined(vks, sigs), arena, offs, kb, out,
                                                          ctypes.byref(miss)))
        return list(out.raw[:n]), miss.value

    def combine_records_device(self, stream, g, d_records, stride, d_out):
        """Enqueue the combine of g gathered 129-byte exchange records (device memory) on `stream`
        (a raw HIP stream handle); the 256-byte result block lands in d_out (device)."""
        with self._lock:
            self._check(self.lib.edc_combine_records_device(self.ctx, ctypes.c_void_p(stream), g,
                                                            ctypes.c_void_p(d_records), stride, ctypes.c_void_p(d_out)))

    def combine_partials(self, partials, bad_any, want_check8=True):
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self._check(self.lib.edc_combine_partials(self.ctx, len(partials), b"".join(partials) or b"\0",
                                                           1 if bad_any else 0, check8))
        return rc, (check8.raw if check8 is not None else None)


class MultiEngine:
    """Several GPUs in one process (include/edc.h edc_create_multi): each batch is split into
    contiguous shards, one per listed device; partial points are combined on the first device.
    A device may be listed several times (several contexts on one GPU)."""

    def __init__(self, devices):
        self.lib = load_library()
        if self.lib.edc_device_count() <= 0:
            raise EngineError("no HIP device visible; the MI355X path has no CPU fallback")
        arr = (ctypes.c_int * len(devices))(*devices)
        self.m = self.lib.edc_create_multi(arr, len(devices))
        if not self.m:
            raise EngineError(f"edc_create_multi({list(devices)}) failed")
        self.devices = list(devices)
        self._lock = threading.Lock()
        self._inflight = {}

    def close(self):
        if self.m:
            self.lib.edc_destroy_multi(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise EngineError(f"edc error {rc}: {self.lib.edc_multi_last_error(self.m).decode()}")
        return rc

    def batch_verify(self, vks, sigs, msgs, z_seed, want_check8=False):
        arena, offs = _arena(msgs)
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self.lib.edc_multi_batch_verify(self.m, len(vks), b"".join(vks) or b"\0", b"".join(sigs) or b"\0",
                                                 arena, offs, bytes(z_seed), check8)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def batch_submit(self, vks, sigs, msgs, z_seed, want_check8=False):
        """Pipelined multi-device batch (edc_multi_submit): returns a ticket; the host buffers are
        kept alive here until batch_wait(ticket)."""
        arena, offs = _arena(msgs)
        bufs = (b"".join(vks) or b"\0", b"".join(sigs) or b"\0", arena, offs, bytes(z_seed))
        with self._lock:
            t = self.lib.edc_multi_submit(self.m, len(vks), bufs[0], bufs[1], bufs[2], bufs[3], bufs[4],
                                          1 if want_check8 else 0)
            self._check(t)
            self._inflight[t] = bufs
        return t

    def batch_submit_device(self, shards, z_seed, want_check8=False):
        """edc_multi_submit_device: shards[g] = (n, d_vk, d_sig, d_msg, d_msg_off) as device pointers
        (ints) on device g; returns a ticket."""
        G = len(shards)
        n = (ctypes.c_size_t * G)(*[s[0] for s in shards])
        ptr = lambda k: (ctypes.c_void_p * G)(*[s[k] for s in shards])
        with self._lock:
            t = self.lib.edc_multi_submit_device(self.m, n, ptr(1), ptr(2), ptr(3), ptr(4), bytes(z_seed),
                                                 1 if want_check8 else 0)
            self._check(t)
        return t

    def batch_wait(self, ticket, want_check8=False):
        check8 = ctypes.create_string_buffer(32) if want_check8 else None
        with self._lock:
            rc = self.lib.edc_multi_wait(self.m, ticket, check8)
            self._inflight.pop(ticket, None)
        self._check(rc)
        return rc, (check8.raw if check8 is not None else None)

    def route(self, i):
        """How shard i's result block reaches the first device: 0 local, 1 peer (xGMI), 2 host-staged."""
        return self._check(self.lib.edc_multi_route(self.m, int(i)))

    def force_staged(self, on=True):
        """Test knob: route every shard's result block through pinned host memory (the no-peer path)."""
        with self._lock:
            self._check(self.lib.edc_multi_debug_force_staged(self.m, 1 if on else 0))

    def batch_verify_fallback(self, vks, sigs, msgs, z_seed):
        """(code, per-item verify_single codes, number invalid, check8)."""
        n = len(vks)
        arena, offs = _arena(msgs)
        check8 = ctypes.create_string_buffer(32)
        v = ctypes.create_string_buffer(max(n, 1))
        cnt = ctypes.c_int(0)
        with self._lock:
            rc = self.lib.edc_multi_batch_verify_fallback(self.m, n, b"".join(vks) or b"\0", b"".join(sigs) or b"\0",
                                                          arena, offs, bytes(z_seed), v, ctypes.byref(cnt), check8)
        self._check(rc)
        return rc, list(v.raw[:n]), cnt.value, check8.raw


def debug_live_allocs():
    """edc_debug_live_allocs: (live device allocations, live pinned allocations) of this process's library objects."""
    out = (ctypes.c_uint64 * 2)()
    if load_library().edc_debug_live_allocs(out) != 0:
        raise EngineError("edc_debug_live_allocs failed")
    return int(out[0]), int(out[1])


_default_engine = None
_default_lock = threading.Lock()


def default_engine():
    global _default_engine
    with _default_lock:
        if _default_engine is None:
            _default_engine = Engine()
        return _default_engine


# ------------------------------------------------------------------ reference types
def _as_bytes(x, n):
    b = bytes(x)
    if len(b) != n:
        raise InvalidSliceLength()
    return b


_L = (1 << 252) + 27742317777372353535851937790883648493    # the group order l


def _canonical_k(k):
    """A prehashed challenge as the reference's Item holds it: Scalar::from_hash output, < l
    (src/batch.rs:82-94). Anything else is an argument error, never a verdict."""
    b = _as_bytes(k, 32)
    if int.from_bytes(b, "little") >= _L:
        raise ValueError("prehashed k is not a canonical scalar (must be < l)")
    return b


class Signature:
    """reference src/signature.rs:8-62: 64 bytes R || s, not validated at parse time."""

    __slots__ = ("R_bytes", "s_bytes")

    def __init__(self, data):
        b = _as_bytes(data, 64)
        self.R_bytes, self.s_bytes = b[:32], b[32:]

    def to_bytes(self):
        return self.R_bytes + self.s_bytes

    def __bytes__(self):
        return self.to_bytes()

    def __eq__(self, other):
        return isinstance(other, Signature) and self.to_bytes() == other.to_bytes()

    def __hash__(self):
        return hash(self.to_bytes())

    def __repr__(self):
        return f"Signature(R_bytes={self.R_bytes.hex()}, s_bytes={self.s_bytes.hex()})"


class VerificationKeyBytes:
    """reference src/verification_key.rs:32-87: raw 32 bytes; Hash/Eq on the bytes."""

    __slots__ = ("_b",)

    def __init__(self, data):
        if isinstance(data, (VerificationKeyBytes, VerificationKey)):
            data = data.to_bytes()
        self._b = _as_bytes(data, 32)

    def to_bytes(self):
        return self._b

    def as_bytes(self):
        return self._b

    def __bytes__(self):
        return self._b

    def __eq__(self, other):
        return isinstance(other, VerificationKeyBytes) and self._b == other._b

    def __lt__(self, other):
        return self._b < other._b

    def __hash__(self):
        return hash(self._b)

    def __repr__(self):
        return f"VerificationKeyBytes({self._b.hex()})"


class VerificationKey:
    """reference src/verification_key.rs:106-258. try_from decodes A on the GPU once and keeps it:
    the reference stores minus_A in the object (:111-114, :160-175); here the decoded point and its
    fixed-base table go into the engine's key cache (edc_keycache_add), where every later verify,
    batch or fallback of that engine finds them (`cached`). keep_decoded=False only validates;
    True always adds; None (the default) adds while the engine's cache holds fewer than
    AUTO_CACHE_KEYS keys, so keys parsed from untrusted input cannot grow device memory without
    bound. Keys that do not decode are never added (edc_keycache_add)."""

    AUTO_CACHE_KEYS = 1024          # 64 MB of comb tables
    # Cost of the default (keep_decoded=None): a call that adds new keys rebuilds the cache's hash
    # table, decodes the new keys' comb tables and synchronises every slot of the engine (it may
    # not run while batches are in flight; it then only validates). Ingesting keys that are
    # already cached adds nothing.

    __slots__ = ("A_bytes", "_engine", "cached")

    def __init__(self, vkb, engine, cached=False):
        self.A_bytes = vkb
        self._engine = engine
        self.cached = cached

    @classmethod
    def try_from(cls, data, engine=None, keep_decoded=None):
        r = cls.try_from_many([data], engine, keep_decoded)[0]
        if isinstance(r, MalformedPublicKey):
            raise r
        return r

    @classmethod
    def try_from_many(cls, keys, engine=None, keep_decoded=None):
        """Batched key ingestion: [VerificationKey or MalformedPublicKey()] per input, one launch
        (keep_decoded: also add the keys to the engine's key cache; None: while it stays under
        AUTO_CACHE_KEYS)."""
        vkbs = [k if isinstance(k, VerificationKeyBytes) else VerificationKeyBytes(k) for k in keys]
        eng = engine or default_engine()
        encs = [v.to_bytes() for v in vkbs]
        if keep_decoded is None:      # keys already cached cost nothing: only new ones count
            keep_decoded = eng.keycache_size() + len(eng.keycache_missing(encs)) <= cls.AUTO_CACHE_KEYS
        cached = False
        if keep_decoded and encs:
            try:
                _, oks = eng.keycache_add(encs)
                codes = [EDC_OK if o else EDC_MALFORMED_PUBLIC_KEY for o in oks]
                cached = True
            except EngineError:        # cache full, or batches in flight: validate only
                codes = eng.vk_validate(encs)
        else:
            codes = eng.vk_validate(encs)
        return [cls(v, eng, cached) if c == EDC_OK else MalformedPublicKey() for v, c in zip(vkbs, codes)]


    def to_bytes(self):
        return self.A_bytes.to_bytes()

    def verify(self, signature, msg):
        """VerificationKey::verify (src/verification_key.rs:225-233)."""
        sig = signature if isinstance(signature, Signature) else Signature(signature)
        code = self._engine.verify_each([self.to_bytes()], [sig.to_bytes()], [bytes(msg)])[0]
        if code != EDC_OK:
            raise _CODE_TO_ERR[code]()


class SigningKey:
    """reference src/signing_key.rs (test-data source): seed -> key; sign on the GPU."""

    __slots__ = ("seed", "_engine", "_vk")

    def __init__(self, seed=None, engine=None):
        self.seed = _as_bytes(seed, 32) if seed is not None else secrets.token_bytes(32)
        self._engine = engine or default_engine()
        self._vk = None

    @classmethod
    def new(cls, rng=None, engine=None):
        seed = rng.token_bytes(32) if hasattr(rng, "token_bytes") else secrets.token_bytes(32)
        return cls(seed, engine)

    def verification_key_bytes(self):
        if self._vk is None:
            vks, _ = self._engine.sign([self.seed], [b""])
            self._vk = VerificationKeyBytes(vks[0])
        return self._vk

    def sign(self, msg):
        vks, sigs = self._engine.sign([self.seed], [bytes(msg)])
        self._vk = VerificationKeyBytes(vks[0])
        return Signature(sigs[0])


class batch:  # namespace mirroring `ed25519_consensus::batch`
    class Item:
        """reference src/batch.rs:75-107. k = H(R||A||M) is computed at construction on the GPU
        (Item::from), so verify_single is decoupled from the message."""

        __slots__ = ("vk_bytes", "sig", "k", "_msg")

        def __init__(self, vk_bytes, sig, msg=None, k=None):
            self.vk_bytes = vk_bytes if isinstance(vk_bytes, VerificationKeyBytes) else VerificationKeyBytes(vk_bytes)
            self.sig = sig if isinstance(sig, Signature) else Signature(sig)
            if msg is None and k is None:
                raise ValueError("an Item needs its message or its challenge k")
            self._msg = bytes(msg) if msg is not None else None
            self.k = _canonical_k(k) if k is not None else None

        @classmethod
        def from_tuple(cls, tup):
            return cls(*tup)

        @classmethod
        def prehashed(cls, vk_bytes, sig, k):
            """The reference's Item as it is stored, {vk_bytes, sig, k} (src/batch.rs:76-80): k was
            computed at Item::from (e.g. by another process), the message is not needed again."""
            return cls(vk_bytes, sig, None, k)

        @staticmethod
        def hash_many(items, engine=None):
            """Item::from's k = H(R||A||M) mod l (src/batch.rs:82-94) for every item still without
            one, in ONE GPU launch."""
            eng = engine or default_engine()
            need = [it for it in items if it.k is None]
            if need:
                ks = eng.challenge([it.vk_bytes.to_bytes() for it in need], [it.sig.to_bytes() for it in need],
                                   [it._msg for it in need])
                for it, k in zip(need, ks):
                    it.k = k
            return items

        def verify_single(self, engine=None):
            eng = engine or default_engine()
            if self.k is None:
                self.k = eng.challenge([self.vk_bytes.to_bytes()], [self.sig.to_bytes()], [self._msg])[0]
            code = eng.verify_prehashed_each([self.vk_bytes.to_bytes()], [self.sig.to_bytes()], [self.k])[0]
            if code != EDC_OK:
                raise _CODE_TO_ERR[code]()

        @staticmethod
        def verify_single_many(items, engine=None):
            """Fallback for many items in ONE GPU launch; returns per-item verdict codes."""
            eng = engine or default_engine()
            batch.Item.hash_many(items, eng)
            return eng.verify_prehashed_each([it.vk_bytes.to_bytes() for it in items],
                                             [it.sig.to_bytes() for it in items], [it.k for it in items])

        @staticmethod
        def verify_single_many_cached(items, engine=None):
            """verify_single_many through the engine's verified-signature cache
            (Engine.verify_each_cached): items verified before are not verified again, valid new
            ones are remembered. Returns per-item verdict codes."""
            eng = engine or default_engine()
            batch.Item.hash_many(items, eng)
            return eng.verify_each_cached([it.vk_bytes.to_bytes() for it in items],
                                          [it.sig.to_bytes() for it in items], ks=[it.k for it in items])[0]

    class Templates:
        """A block's template set (struct edc_templates): message i of a templated call is
        heads[tpl[i]] + hole_i + tails[tpl[i]]. 1..65535 templates; a head or tail may be empty."""

        def __init__(self, heads, tails):
            if len(heads) != len(tails) or not 1 <= len(heads) <= 65535:
                raise ValueError("Templates: 1..65535 heads and as many tails")
            self.heads = [bytes(h) for h in heads]
            self.tails = [bytes(t) for t in tails]

        @property
        def count(self):
            return len(self.heads)

        def materialize(self, tpl, var_list):
            """The messages as bytes, built on the host (tests and documentation)."""
            if len(tpl) != len(var_list):
                raise ValueError("materialize: lists of different lengths")
            return [self.heads[t] + bytes(v) + self.tails[t] for t, v in zip(tpl, var_list)]

        def struct(self):
            """(EdcTemplates, the buffers it points into: keep them alive for the call)."""
            def blob(parts):
                off = (ctypes.c_uint32 * (len(parts) + 1))()
                total = 0
                for i, p in enumerate(parts):
                    off[i] = total
                    total += len(p)
                off[len(parts)] = total
                return b"".join(parts) or b"\0", off
            head, head_off = blob(self.heads)
            tail, tail_off = blob(self.tails)
            return EdcTemplates(self.count, head, head_off, tail, tail_off), (head, head_off, tail, tail_off)

    class Verifier:
        """reference src/batch.rs:110-217. Items are kept in queue order; grouping by key
        bytes, hashing and the coalesced MSM run on the GPU inside verify()."""

        def __init__(self, engine=None):
            self._engine = engine
            self._vks, self._sigs, self._msgs, self._ks = [], [], [], []

        @classmethod
        def new(cls, engine=None):
            return cls(engine)

        @property
        def batch_size(self):
            return len(self._vks)

        def queue(self, item, sig=None, msg=None):
            if sig is not None:
                item = batch.Item(item, sig, msg)
            elif isinstance(item, tuple):
                item = batch.Item(*item)
            self._vks.append(item.vk_bytes.to_bytes())
            self._sigs.append(item.sig.to_bytes())
            self._msgs.append(item._msg)
            self._ks.append(item.k)

        def verify_detailed(self, rng=None):
            """Returns (code, check8): check8 = compressed [8]*check (None when rejected before
            the MSM). rng: a 32-byte ChaCha20 seed, an object with fill_bytes(n)/token_bytes(n),
            or None (fresh OS randomness). Items that carry their k (prehashed, as the reference's
            Item always does) go through edc_batch_verify_prehashed; otherwise SHA-512 runs on the
            GPU inside the batch."""
            eng = self._engine or default_engine()
            n = len(self._vks)
            if isinstance(rng, (bytes, bytearray)) and len(rng) == 32:
                zkw = {"z_seed": bytes(rng)}
            elif rng is None:
                zkw = {"z_seed": secrets.token_bytes(32)}
            else:   # gen_u128 per item in queue order (src/batch.rs:64-68)
                draw = rng.fill_bytes if hasattr(rng, "fill_bytes") else rng.token_bytes
                zkw = {"z": b"".join(bytes(draw(16)) for _ in range(n))}
            if any(m is None for m in self._msgs) or (n and all(k is not None for k in self._ks)):
                if any(k is None for k in self._ks):     # mixed queue: hash the rest in one launch
                    need = [i for i, k in enumerate(self._ks) if k is None]
                    ks = eng.challenge([self._vks[i] for i in need], [self._sigs[i] for i in need],
                                       [self._msgs[i] for i in need])
                    for i, k in zip(need, ks):
                        self._ks[i] = k
                return eng.batch_verify_prehashed(self._vks, self._sigs, self._ks, want_check8=True, **zkw)
            return eng.batch_verify(self._vks, self._sigs, self._msgs, want_check8=True, **zkw)

        def verify(self, rng=None):
            """Verifier::verify: returns None on success, raises InvalidSignature otherwise."""
            code, _ = self.verify_detailed(rng)
            if code != EDC_OK:
                raise InvalidSignature()

        def verify_cached(self, rng=None):
            """Verifier::verify through the engine's verified-signature cache
            (Engine.batch_verify_cached): only the items not verified before on that engine are
            verified, and remembered when their batch passes. Returns the number of misses, raises
            InvalidSignature otherwise. rng: a 32-byte ChaCha20 seed or None (fresh OS randomness);
            z drawn by a caller's RNG object cannot follow the miss list and is refused."""
            if rng is None:
                seed = None
            elif isinstance(rng, (bytes, bytearray)) and len(rng) == 32:
                seed = bytes(rng)
            else:
                raise ValueError("verify_cached takes a 32-byte seed or None, not caller-drawn z")
            eng = self._engine or default_engine()
            if any(k is None for k in self._ks):
                if any(m is None for m in self._msgs):   # mixed queue: hash the rest in one launch
                    need = [i for i, k in enumerate(self._ks) if k is None]
                    ks = eng.challenge([self._vks[i] for i in need], [self._sigs[i] for i in need],
                                       [self._msgs[i] for i in need])
                    for i, k in zip(need, ks):
                        self._ks[i] = k
                    code, _, n_miss = eng.batch_verify_cached(self._vks, self._sigs, ks=self._ks, z_seed=seed)
                else:
                    code, _, n_miss = eng.batch_verify_cached(self._vks, self._sigs, msgs=self._msgs, z_seed=seed)
            else:
                code, _, n_miss = eng.batch_verify_cached(self._vks, self._sigs, ks=self._ks, z_seed=seed)
            if code != EDC_OK:
                raise InvalidSignature()
            return n_miss

    @staticmethod
    def verify_many(verifiers, z_seed=None, engine=None):
        """Verifier::verify for many Verifiers in ONE launch (a commit set, edc_commits_verify): one
        bool per verifier, True where Verifier::verify would return Ok. The verifiers' items run as
        one batch; only if that fails are the failing verifiers found (include/edc.h, "Commit
        sets"). z_seed: 32 bytes, or None for fresh OS randomness (anything else than a fresh secret
        seed is for reproducible tests only). Nothing to verify needs no engine."""
        verifiers = list(verifiers)
        for v in verifiers:
            if not isinstance(v, batch.Verifier):
                raise TypeError("verify_many takes batch.Verifier objects")
        if z_seed is None:
            z_seed = secrets.token_bytes(32)
        elif not isinstance(z_seed, (bytes, bytearray)) or len(z_seed) != 32:
            raise ValueError("z_seed: 32 bytes or None")
        off = [0]
        for v in verifiers:
            off.append(off[-1] + v.batch_size)
        if off[-1] >= 1 << 28:
            raise ValueError("verify_many: fewer than 2^28 items in one call")
        if off[-1] == 0:
            return [True] * len(verifiers)
        eng = engine or next((v._engine for v in verifiers if v._engine is not None), None) or default_engine()
        vks = [x for v in verifiers for x in v._vks]
        sigs = [x for v in verifiers for x in v._sigs]
        msgs = [x for v in verifiers for x in v._msgs]
        if all(m is not None for m in msgs):
            res = eng.commits_verify(off, sigs, z_seed, vks=vks, msgs=msgs)
        else:                                    # some items carry only their k: hash the rest in one launch
            ks = [x for v in verifiers for x in v._ks]
            need = [i for i, k in enumerate(ks) if k is None]
            if need:
                for i, k in zip(need, eng.challenge([vks[i] for i in need], [sigs[i] for i in need],
                                                    [msgs[i] for i in need])):
                    ks[i] = k
            res = eng.commits_verify(off, sigs, z_seed, vks=vks, ks=ks)
        return [c == EDC_OK for c in res[1]]

    @staticmethod
    def verify_quorum(verifiers, powers, flags, thresholds, light=True, z_seed=None, engine=None, cached=False,
                      versions=None, trust_versions=None, trust_thresholds=None):
        """Quorum check of many commits in ONE launch (a quorum commit set, edc_quorum_verify; not an
        API of the reference). verifiers: one batch.Verifier per commit, holding an item for EVERY
        validator of its set (any bytes for an absent one); powers / flags: one list per verifier, one
        entry per item (VOTE_ABSENT, VOTE_COMMIT, VOTE_NIL); thresholds: one per verifier, a commit
        has its quorum iff its tally is strictly greater. light=True verifies votes for the block
        only until the threshold is passed (VerifyCommitLight), False every vote that carries a
        signature (VerifyCommit). Returns (commit verdicts, tallies, item codes per verifier): a
        verdict is EDC_OK, EDC_INVALID_SIGNATURE or EDC_QUORUM_SHORT, an item code Item::verify_single's
        or NOT_CHECKED. z_seed as verify_many. cached=True goes through the engine's verified-signature
        table (Engine.sigcache_create; edc_cached_quorum_verify): checked votes that already verified
        on the engine are not verified again and count as EDC_OK, and what this call proves valid is
        remembered. The return value has the same form.
        powers=None takes the powers from the engine's registered validator set
        (Engine.valset_set_powers; edc_valset_quorum_verify): a vote whose key is no member of it
        counts as absent, and a commit with two checked votes of one member gets EDC_DOUBLE_VOTE.
        versions (one per verifier, with powers=None only) judges every commit by that version of the
        engine's validator-set history (Engine.vhist_set; edc_vhist_quorum_verify) instead.
        trust_versions / trust_thresholds (one per verifier, with versions only; NO_TRUST for a commit
        without a trusting side) judge every commit by a second set as well and verify each vote
        once (a trusting pair, edc_vq_verify): the return value is then (commit verdicts, tallies, item
        codes per verifier, trust verdicts, trust tallies)."""
        verifiers = list(verifiers)
        if (trust_versions is None) != (trust_thresholds is None) or (trust_versions is not None and versions is None):
            raise ValueError("verify_quorum: trust_versions and trust_thresholds go together, and with versions")
        if trust_versions is not None:
            trust_versions, trust_thresholds = [int(v) for v in trust_versions], list(trust_thresholds)
            if len(trust_versions) != len(verifiers) or len(trust_thresholds) != len(verifiers):
                raise ValueError("verify_quorum: one trust version and trust threshold per verifier")
        if versions is not None:
            if powers is not None or cached:
                raise ValueError("verify_quorum: versions go with powers=None and have no cached form")
            versions = [int(v) for v in versions]
            if len(versions) != len(verifiers):
                raise ValueError("verify_quorum: one version per verifier")
        if powers is None:
            if cached:
                raise ValueError("verify_quorum: the registered validator set has no cached form")
            powers = [[0] * v.batch_size if isinstance(v, batch.Verifier) else [] for v in verifiers]
            from_set = True
        else:
            from_set = False
        for v in verifiers:
            if not isinstance(v, batch.Verifier):
                raise TypeError("verify_quorum takes batch.Verifier objects")
        powers, flags, thresholds = [list(p) for p in powers], [list(f) for f in flags], list(thresholds)
        if len(powers) != len(verifiers) or len(flags) != len(verifiers) or len(thresholds) != len(verifiers):
            raise ValueError("verify_quorum: one powers list, flags list and threshold per verifier")
        if z_seed is None:
            z_seed = secrets.token_bytes(32)
        elif not isinstance(z_seed, (bytes, bytearray)) or len(z_seed) != 32:
            raise ValueError("z_seed: 32 bytes or None")
        off = [0]
        for v, p, f in zip(verifiers, powers, flags):
            if len(p) != v.batch_size or len(f) != v.batch_size:
                raise ValueError("verify_quorum: one power and flag per queued item")
            off.append(off[-1] + v.batch_size)
        if off[-1] >= 1 << 28:
            raise ValueError("verify_quorum: fewer than 2^28 items in one call")
        if not verifiers:
            return ([], [], [], [], []) if trust_versions is not None else ([], [], [])
        eng = engine or next((v._engine for v in verifiers if v._engine is not None), None) or default_engine()
        vks = [x for v in verifiers for x in v._vks]
        sigs = [x for v in verifiers for x in v._sigs]
        msgs = [x for v in verifiers for x in v._msgs]
        pw, fl = [x for p in powers for x in p], [x for f in flags for x in f]
        if from_set:
            def run(off, sigs, pw, fl, thresholds, z_seed, **kw):
                if trust_versions is not None:
                    return eng.vq_verify(off, fl, thresholds, z_seed, versions=versions, sigs=sigs,
                                         trust_versions=trust_versions, trust_thresholds=trust_thresholds, **kw)
                if versions is not None:
                    return eng.quorum_verify_vhist(off, versions, sigs, fl, thresholds, z_seed, **kw)
                return eng.quorum_verify_valset(off, sigs, fl, thresholds, z_seed, **kw)
        else:
            run = eng.quorum_verify_cached if cached else eng.quorum_verify
        if all(m is not None for m in msgs):
            res = run(off, sigs, pw, fl, thresholds, z_seed, light=light, vks=vks, msgs=msgs)
        else:                                    # some items carry only their k: hash the rest in one launch
            ks = [x for v in verifiers for x in v._ks]
            need = [i for i, k in enumerate(ks) if k is None]
            if need:
                for i, k in zip(need, eng.challenge([vks[i] for i in need], [sigs[i] for i in need],
                                                    [msgs[i] for i in need])):
                    ks[i] = k
            res = run(off, sigs, pw, fl, thresholds, z_seed, light=light, vks=vks, ks=ks)
        codes = [res["item_verdicts"][off[c]:off[c + 1]] for c in range(len(verifiers))]
        if trust_versions is not None:
            return res["commit_verdicts"], res["tally"], codes, res["trust_verdicts"], res["trust_tally"]
        return res["commit_verdicts"], res["tally"], codes

    @staticmethod
    def validator_set_hashes(versions=None, expect=None, engine=None):
        """The Merkle root of the validator sets verify_quorum judges by (edc_valhash_*; not an API of
        the reference): what a light client compares with the validators_hash of the header it
        trusts before it judges a commit by a set it was handed. versions=None: the root of every
        version of the engine's validator-set history (Engine.vhist_set), or, on an engine without a
        history, [the root of its one set] (Engine.valset_set_powers). versions a list: the root of
        each, in that order; a version is hashed once however often it occurs. With expect (32 bytes
        per entry of versions) the compare runs on the device and the return value is
        (ok, n_mismatch): ok[c] = 1 iff the root of versions[c] equals expect[c]."""
        eng = engine or default_engine()
        if expect is not None:
            if versions is None:
                raise ValueError("validator_set_hashes: expect goes with versions")
            return eng.vhist_hash_match(list(versions), list(expect))
        if versions is None:
            return eng.vhist_hashes() if eng.vhist_versions() else [eng.valset_hash()]
        versions = [int(v) for v in versions]
        roots, run = {}, []
        for v in sorted(set(versions)) + [None]:             # consecutive runs, one call each
            if run and v != run[-1] + 1:
                roots.update(zip(run, eng.vhist_hashes(run[0], len(run))))
                run = []
            run.append(v)
        return [roots[v] for v in versions]

    @staticmethod
    def _header_engine(name, engine):
        eng = engine if engine is not None else default_engine()
        if not isinstance(eng, Engine):
            raise ValueError("%s: engine is no Engine" % name)
        return eng

    @staticmethod
    def header_hashes(headers, engine=None):
        """The hash of block headers (edc_header_hashes; not an API of the reference): headers is a
        list of headers, each the list of its ordered leaves as bytes (cometbft_header_leaves builds
        the 14 of a CometBFT header) -> the 32-byte RFC 6962 Merkle root of each."""
        return batch._header_engine("header_hashes", engine).header_hashes(headers)

    @staticmethod
    def verify_headers(headers, expect=None, vals=None, nexts=None, link=None, vals_at=(7, 2), next_at=(8, 2),
                       link_at=(4, 2), engine=None):
        """Hashes every header and binds it (edc_header_bind; not an API of the reference): to the hash
        it must have (expect, what the votes of its commit sign), to the validator-set roots of the
        engine's history (vals, nexts: per header a version of Engine.vhist_set, compared with the 32
        bytes at (leaf, position) vals_at / next_at) and to another header of the list (link: per
        header the index of the header whose hash it carries at link_at, as a header carries its
        predecessor's in last_block_id). None for a list: no such rule; None as an entry: that header
        is skipped. -> (bad, n_bad, roots): per header 0 or the HEADER_BAD_* bits of the rules that do
        not hold, the number of non-zero entries, the hashes."""
        return batch._header_engine("verify_headers", engine).header_bind(headers, expect, vals, nexts, link, vals_at, next_at,
                                                                          link_at)

    @staticmethod
    def cometbft_header_leaves(version_block=0, version_app=0, chain_id="", height=0, time_seconds=0, time_nanos=0,
                               last_block_hash=b"", last_parts_total=0, last_parts_hash=b"", last_commit_hash=b"",
                               data_hash=b"", validators_hash=b"", next_validators_hash=b"", consensus_hash=b"",
                               app_hash=b"", last_results_hash=b"", evidence_hash=b"", proposer_address=b""):
        """The 14 leaves of a CometBFT header, in the order Header.Hash() hashes them, from the field
        values: pure Python, no device work. The proto3 encodings are stated from memory, as
        include/edc.h states the hash; the contract is the bytes written here. uvarint is base-128,
        little-endian; a negative int64 is its 64-bit two's complement (10 bytes). Zero and empty
        fields are omitted everywhere, so a leaf may be empty; only the part-set header inside the
        block id is always emitted.
           0  version               (08 uvarint(block) if block != 0) | (10 uvarint(app) if app != 0)
           1  chain_id              0A uvarint(len) utf-8 bytes, or nothing for ""
           2  height                08 uvarint(height), or nothing for 0
           3  time                  (08 uvarint(seconds) if seconds != 0) | (10 uvarint(nanos) if nanos != 0)
           4  last_block_id         (0A uvarint(len) hash if hash) | 12 uvarint(len(P)) P, with the part-set
                                    header P = (08 uvarint(total) if total != 0) | (12 uvarint(len) hash if
                                    hash); 12 00 for an empty one. With two 32-byte hashes and total < 128
                                    this is 72 bytes and the block hash starts at position 2.
           5..12 last_commit_hash, data_hash, validators_hash, next_validators_hash, consensus_hash,
                 app_hash, last_results_hash, evidence_hash: 0A uvarint(len) bytes, or nothing when empty;
                 a 32-byte hash starts at position 2, behind 0A 20
          13  proposer_address      the same"""
        def uv(x):
            x = int(x) & 0xFFFFFFFFFFFFFFFF
            out = bytearray()
            while x >= 0x80:
                out.append((x & 0x7F) | 0x80)
                x >>= 7
            out.append(x)
            return bytes(out)
        num = lambda tag, x: bytes([tag]) + uv(x) if int(x) != 0 else b""
        blob = lambda tag, b: bytes([tag]) + uv(len(b)) + bytes(b) if len(b) else b""
        parts = num(0x08, last_parts_total) + blob(0x12, last_parts_hash)
        return [
            num(0x08, version_block) + num(0x10, version_app),
            blob(0x0A, chain_id.encode() if isinstance(chain_id, str) else bytes(chain_id)),
            num(0x08, height),
            num(0x08, time_seconds) + num(0x10, time_nanos),
            blob(0x0A, last_block_hash) + b"\x12" + uv(len(parts)) + parts,
            blob(0x0A, last_commit_hash), blob(0x0A, data_hash), blob(0x0A, validators_hash),
            blob(0x0A, next_validators_hash), blob(0x0A, consensus_hash), blob(0x0A, app_hash),
            blob(0x0A, last_results_hash), blob(0x0A, evidence_hash), blob(0x0A, proposer_address),
        ]

    class StreamVerifier:
        """reference src/batch.rs:110-217 with the reference's division of work: queue() does the
        per-item work on the GPU as items arrive (copy, SHA-512 -> k, ZIP215 decode of R, key
        grouping, decode of new keys; edc_verifier_queue*), and verify(rng) only evaluates the
        equation (edc_verifier_verify). Results equal batch.Verifier's on the same items and z.
        The queue survives verify(); reset() starts the next block with the same allocations.
        eager=True (or begin_eager()) commits the block's z seed up front, so that queue calls also
        sum the [z_i]R_i terms on the GPU and verify() runs an MSM over B, the keys and the short
        unfolded tail only (edc_vfy_begin_eager; soundness in include/edc.h).
        cached=True (or set_cached()) makes queue calls skip the items the engine's
        verified-signature table already vouches for (Engine.sigcache_create): only the misses
        are retained and verified, and what verify() proves valid is remembered
        (edc_vfy_set_cached; soundness in include/edc.h)."""

        def __init__(self, engine=None, capacity=0, eager=False, cached=False):
            self._engine = engine or default_engine()
            self._always_eager = bool(eager)
            self._v = self._engine.lib.edc_verifier_create(self._engine.ctx, int(capacity))
            if not self._v:
                raise EngineError("edc_verifier_create failed: "
                                  + self._engine.lib.edc_last_error(self._engine.ctx).decode())
            self._engine._verifiers.add(self)
            if cached:
                self.set_cached(True)
            if eager:
                self.begin_eager()

        @classmethod
        def new(cls, engine=None, capacity=0, eager=False, cached=False):
            return cls(engine, capacity, eager, cached)

        def set_cached(self, on=True):
            """Switch cached mode. Only while nothing is queued; the mode survives reset()."""
            eng = self._engine
            with eng._lock:
                rc = eng.lib.edc_vfy_set_cached(self._handle(), 1 if on else 0)
            eng._check(rc)

        @property
        def cached(self):
            return self._engine.lib.edc_vfy_cached(self._handle()) == 1

        @property
        def cache_counts(self):
            """(items offered to queue calls since the last reset, how many were skipped as hits);
            batch_size is their difference."""
            offered, hits = ctypes.c_uint64(0), ctypes.c_uint64(0)
            eng = self._engine
            eng._check(eng.lib.edc_vfy_cache_counts(self._handle(), ctypes.byref(offered), ctypes.byref(hits)))
            return int(offered.value), int(hits.value)

        def begin_eager(self, seed=None):
            """Enter eager mode for this block with a committed 32-byte z seed (None: fresh OS
            randomness drawn by the library). Only while nothing is queued."""
            eng = self._engine
            with eng._lock:
                rc = eng.lib.edc_vfy_begin_eager(self._handle(), None if seed is None else _as_bytes(seed, 32))
            eng._check(rc)

        @property
        def eager(self):
            return self._engine.lib.edc_vfy_eager(self._handle()) == 1

        @property
        def folded(self):
            """(items whose R term is in the running point, folds since the last reset)."""
            items, folds = ctypes.c_uint64(0), ctypes.c_uint64(0)
            eng = self._engine
            eng._check(eng.lib.edc_vfy_folded(self._handle(), ctypes.byref(items), ctypes.byref(folds)))
            return int(items.value), int(folds.value)

        def set_fold(self, min_items):
            """Fold once at least min_items queued items are pending (0: the library default);
            results never depend on it."""
            eng = self._engine
            eng._check(eng.lib.edc_vfy_set_fold(self._handle(), int(min_items)))

        def close(self):
            if getattr(self, "_v", None):
                if self._engine.ctx:
                    self._engine.lib.edc_verifier_destroy(self._v)
                self._v = None
                self._engine._verifiers.discard(self)

        def __del__(self):
            try:
                self.close()
            except Exception:
                pass

        def _handle(self):
            if not self._v:
                raise EngineError("StreamVerifier is closed")
            return self._v

        @property
        def batch_size(self):
            return int(self._engine.lib.edc_verifier_size(self._handle()))

        def queue(self, item, sig=None, msg=None):
            """Verifier::queue: a batch.Item or a (vk, sig, msg) tuple."""
            if sig is not None:
                item = batch.Item(item, sig, msg)
            elif isinstance(item, tuple):
                item = batch.Item(*item)
            vk, sg = item.vk_bytes.to_bytes(), item.sig.to_bytes()
            if item.k is not None:
                self.queue_many([vk], [sg], ks=[item.k])
            else:
                self.queue_many([vk], [sg], msgs=[item._msg])

        def queue_many(self, vks, sigs, msgs=None, ks=None):
            """Append len(vks) items in order: with their messages, or prehashed with their k."""
            n = len(vks)
            if (msgs is None) == (ks is None):
                raise ValueError("queue_many takes either msgs or ks")
            if len(sigs) != n or len(msgs if ks is None else ks) != n:
                raise ValueError("queue_many: lists of different lengths")
            if not n:
                return
            eng, v = self._engine, self._handle()
            vkb = b"".join(_as_bytes(x, 32) for x in vks)
            sgb = b"".join(_as_bytes(x, 64) for x in sigs)
            with eng._lock:
                if ks is not None:
                    rc = eng.lib.edc_verifier_queue_prehashed(v, n, vkb, sgb, b"".join(_as_bytes(x, 32) for x in ks))
                else:
                    arena, offs = _arena(msgs)
                    rc = eng.lib.edc_verifier_queue(v, n, vkb, sgb, arena, offs)
            eng._check(rc)

        def queue_indexed(self, key_idx, sigs, msgs=None, ks=None):
            """queue_many with the keys given as positions in the list last passed to
            Engine.keycache_load (4 bytes per item over PCIe; edc_vfy_queue_indexed)."""
            n = len(key_idx)
            if (msgs is None) == (ks is None):
                raise ValueError("queue_indexed takes either msgs or ks")
            if len(sigs) != n or len(msgs if ks is None else ks) != n:
                raise ValueError("queue_indexed: lists of different lengths")
            if not n:
                return
            eng, v = self._engine, self._handle()
            idx = (ctypes.c_uint32 * n)(*key_idx)
            sgb = b"".join(_as_bytes(x, 64) for x in sigs)
            with eng._lock:
                if ks is not None:
                    rc = eng.lib.edc_vfy_queue_indexed(v, n, idx, sgb, None, None,
                                                       b"".join(_as_bytes(x, 32) for x in ks))
                else:
                    arena, offs = _arena(msgs)
                    rc = eng.lib.edc_vfy_queue_indexed(v, n, idx, sgb, arena, offs, None)
            eng._check(rc)

        def queue_templated(self, templates, sigs, tpl, holes, vks=None, key_idx=None, var_off=None):
            """Append len(sigs) items whose messages are templates.materialize(tpl, holes), assembled
            on the GPU (edc_vfy_queue_templated). Exactly one of vks and key_idx."""
            n = len(sigs)
            eng, v = self._engine, self._handle()
            ts, _keep = templates.struct()
            t, var, off = _tmpl_items(tpl, holes, var_off)
            vkb, idx = _tmpl_keys(n, vks, key_idx)
            sgb = b"".join(_as_bytes(x, 64) for x in sigs) or b"\0"
            with eng._lock:
                rc = eng.lib.edc_vfy_queue_templated(v, ctypes.byref(ts), n, vkb, idx, sgb, t, var, off)
            eng._check(rc)

        @property
        def last_split(self):
            """1 if the last verify ran with split coefficients, 0 if not (edc_vfy_last_split);
            EngineError before any verify."""
            eng = self._engine
            return eng._check(eng.lib.edc_vfy_last_split(self._handle()))

        @property
        def last_plan(self):
            """Engine.last_plan() for the last verify or eager fold of this verifier, whichever came
            last (edc_vfy_last_plan); EngineError before either."""
            eng, info = self._engine, EdcPlanInfo()
            eng._check(eng.lib.edc_vfy_last_plan(self._handle(), ctypes.byref(info)))
            return info.as_dict()

        def queue_device(self, n, d_vk, d_sig, d_msg=None, d_msg_off=None, d_k=None):
            """Append n items already in this GPU's memory (device pointers; d_k or the messages)."""
            eng = self._engine
            with eng._lock:
                rc = eng.lib.edc_verifier_queue_device(self._handle(), n, d_vk, d_sig, d_msg, d_msg_off, d_k)
            eng._check(rc)

        def verify_detailed(self, rng=None):
            """(code, check8) as batch.Verifier.verify_detailed: rng is a 32-byte ChaCha20 seed, an
            object with fill_bytes(n) / token_bytes(n) (z drawn per item in queue order,
            src/batch.rs:64-68), or None (fresh OS randomness). In eager mode z is already
            committed: rng must be None."""
            eng, v = self._engine, self._handle()
            n = self.batch_size
            seed = z = None
            if self.eager:
                if rng is not None:
                    raise ValueError("eager StreamVerifier: z was committed by begin_eager, verify takes rng=None")
            elif isinstance(rng, (bytes, bytearray)) and len(rng) == 32:
                seed = bytes(rng)
            elif rng is None:
                seed = secrets.token_bytes(32)
            else:
                draw = rng.fill_bytes if hasattr(rng, "fill_bytes") else rng.token_bytes
                z = b"".join(bytes(draw(16)) for _ in range(n)) or b"\0"
            check8 = ctypes.create_string_buffer(32)
            with eng._lock:
                rc = eng.lib.edc_verifier_verify(v, seed, z, check8)
            eng._check(rc)
            return rc, check8.raw

        def verify(self, rng=None):
            """Verifier::verify: returns None on success, raises InvalidSignature otherwise."""
            code, _ = self.verify_detailed(rng)
            if code != EDC_OK:
                raise InvalidSignature()

        def verify_with_fallback(self, z_seed):
            """(code, per-item Item::verify_single codes, check8): verify and, when it fails, the
            grouped fallback on the retained k, points and grouping. z_seed must be fresh and
            secret (include/edc.h, edc_find_invalid_device)."""
            eng, v = self._engine, self._handle()
            n = self.batch_size
            verdicts = ctypes.create_string_buffer(max(n, 1))
            cnt = ctypes.c_int(0)
            check8 = ctypes.create_string_buffer(32)
            with eng._lock:
                rc = eng.lib.edc_verifier_verify_fallback(v, bytes(z_seed), verdicts, ctypes.byref(cnt), check8)
            eng._check(rc)
            return rc, list(verdicts.raw[:n]), check8.raw

        def verify_with_fallback_offered(self, z_seed):
            """verify_with_fallback with the codes in the order the items were offered to queue
            calls (edc_vfy_verify_fallback_offered): (code, codes over the offered items, check8).
            A hit of the table gets 0, a retained item its Item::verify_single code."""
            eng, v = self._engine, self._handle()
            n = self.cache_counts[0] if self.cached else self.batch_size
            verdicts = ctypes.create_string_buffer(max(n, 1))
            cnt = ctypes.c_int(0)
            check8 = ctypes.create_string_buffer(32)
            with eng._lock:
                rc = eng.lib.edc_vfy_verify_fallback_offered(v, bytes(z_seed), verdicts, ctypes.byref(cnt), check8)
            eng._check(rc)
            return rc, list(verdicts.raw[:n]), check8.raw

        def reset(self):
            """Forget the queued items, keep the allocations. Leaves eager mode, unless the object was
            made with eager=True: then the next block begins eagerly with a fresh OS seed."""
            eng = self._engine
            with eng._lock:
                rc = eng.lib.edc_verifier_reset(self._handle())
            eng._check(rc)
            if self._always_eager:
                self.begin_eager()
