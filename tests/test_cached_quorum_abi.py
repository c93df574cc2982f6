"""CPU: the cached quorum commit-set entries (include/edc.h, edc_cached_*) exist in the header, the
library and the Python surface; a NULL context is an argument error on each with nothing written;
the header section states the contract. No compute calls (no GPU here).

The host-side checks of these entries are the uncached forms' own (commits.h / tmpl.h / quorum.h,
held under sanitizers by test_commits_abi / test_tmpl_abi / test_quorum_abi) plus "is there a
table", so there is no new host-logic header and no new stand-alone program."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

ENTRIES = ["edc_cached_quorum_verify_device", "edc_cached_quorum_verify", "edc_cached_tmpl_quorum_verify_device",
           "edc_cached_tmpl_quorum_verify", "edc_debug_cached_quorum_last"]
TWINS = {"edc_cached_quorum_verify_device": "edc_quorum_verify_device", "edc_cached_quorum_verify": "edc_quorum_verify",
         "edc_cached_tmpl_quorum_verify_device": "edc_tmpl_quorum_verify_device",
         "edc_cached_tmpl_quorum_verify": "edc_tmpl_quorum_verify"}


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


def _args(code, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert m, f"include/edc.h does not declare {name}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_library_and_abi_list(edc):
    code = _code()
    lib = edc.load_library()
    for s in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?edc_ctx\s*\*\s*ctx\s*," % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    # one section: after the verified-signature cache's declarations, before the multi-GPU section,
    # with no other declaration in between
    first, last = min(code.index(s + "(") for s in ENTRIES), max(code.index(s + "(") for s in ENTRIES)
    assert code.index("edc_sigcache_verify_each(") < first and last < code.index("edc_create_multi(")
    between = set(re.findall(r"\b(edc_[a-z0-9_]+)\s*\(", code[first:last + 40]))
    assert between == set(ENTRIES)
    declared = set(re.findall(r"\b(edc_[a-z0-9_]+)\s*\(", code))
    assert sorted(s for s in declared if s.startswith("edc_cached_")) == sorted(ENTRIES[:4])


def test_arguments_are_the_uncached_twins_plus_n_miss():
    code = _code()
    for cached, plain in TWINS.items():
        a, b = _args(code, cached), _args(code, plain)
        assert a == b[:-1] + ["size_t* n_miss", b[-1]], cached
    assert _args(code, "edc_debug_cached_quorum_last") == ["const edc_ctx* ctx", "uint64_t out[6]"]


def test_header_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    a = doc.index("Cached quorum commit sets: skip checked votes that already verified")
    assert doc.index("int edc_sigcache_verify_each(") < a
    sec = doc[a:doc.index("int edc_cached_quorum_verify_device(")]
    for phrase in ("whatever the table holds", "the selection never looks at the table",
                   "A hit still counts towards the running sum of light mode",
                   "a live header and 128 equal bytes", "A hit is not verified, its code is EDC_OK",
                   "never looked up, never interpreted and never inserted",
                   "The checked misses, in queue order, form ONE batch", "miss j draws z at index j",
                   "edc_batch_verify_prehashed_device on that list with z_base = 0", "n_miss = 0 runs the n = 0 batch",
                   "EDC_NOT_CHECKED (255) for an item that is not checked, 0 for a hit",
                   "Exactly the misses whose code is EDC_OK are inserted", "Valid nil votes of full mode are inserted too",
                   "The insert finishes before the call returns",
                   "grow by the lookups of the checked items only",
                   "every output equals the uncached entry's on the same inputs, check8 included, and n_miss == n_checked",
                   "every output except check8 and n_miss equals the uncached entry's",
                   "No table on the context returns EDC_ERR_ARG with nothing written",
                   "all n items, not only the checked ones", "nothing is inserted, no counter changes",
                   "nc = 0 returns EDC_OK with no array read", "EDC_ERR_ARG while a batch is pending there",
                   "adds no stream synchronization", "SECOND read-back",
                   "VerifyCommitLightWithCache", "The reference crate has no such API"):
        assert phrase in sec, phrase
    m = re.search(r"Soundness of a cached quorum\. A hit lends its voting power.*?caller vouches for k", sec)
    assert m, "the Soundness paragraph of the cached quorum section is missing"
    for phrase in ("earlier verification on this context", "batch whose equation held", "fresh and secret",
                   "a passing call plants records", "per context"):
        assert phrase in m.group(0), phrase
    # each entry cites the reference lines the quorum entries cite
    for s in ENTRIES[:4]:
        m = re.search(r" %s (edc_\w+ through the table.*?)(?= edc_cached_\w+ | edc_debug_cached_quorum_last test hook)" % s, sec)
        assert m, s
        for cite in ("src/batch.rs:76-94", ":104-107", ":127-137", ":149-217"):
            assert cite in m.group(1), (s, cite)
    for gone in ("asynchronous", "incremental verifier", "multi-GPU"):
        assert gone in sec[sec.index("Not built"):], gone
    # the existing sections still say what the existing tests quote
    assert "These entries need no verified-signature table on the context" in doc
    assert "templated forms are the edc_tmpl_quorum_ entries below" in doc


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    ctpl = (ctypes.c_uint16 * 1)(0)
    thr = (ctypes.c_uint64 * 1)(0)
    pw = (ctypes.c_uint64 * 1)(0)
    hoff = (ctypes.c_uint32 * 2)(0, 0)
    moff = (ctypes.c_uint64 * 2)(0, 0)
    ts = edc.EdcTemplates(1, b"h", hoff, b"t", hoff)
    cnt, miss, nb = ctypes.c_size_t(7), ctypes.c_size_t(7), ctypes.c_int(7)
    c8 = ctypes.create_string_buffer(b"\x07" * 32, 32)
    last = (ctypes.c_uint64 * 6)(*[7] * 6)
    tail = (None, None, None, ctypes.byref(nb), ctypes.byref(cnt), ctypes.byref(miss), c8)
    assert lib.edc_cached_quorum_verify_device(None, 1, off, None, None, None, None, None, None, None, thr, 1, seed,
                                               *tail) == -2
    assert lib.edc_cached_quorum_verify(None, 1, off, None, None, None, None, moff, None, pw, b"\0", thr, 1, seed,
                                        *tail) == -2
    assert lib.edc_cached_tmpl_quorum_verify_device(None, ctypes.byref(ts), 1, off, ctpl, 1, None, None, None, None, None, 0,
                                                    None, None, thr, 1, seed, *tail) == -2
    assert lib.edc_cached_tmpl_quorum_verify(None, ctypes.byref(ts), 1, off, ctpl, 1, None, None, None, None, None, hoff, pw,
                                             b"\0", thr, 1, seed, *tail) == -2
    assert lib.edc_debug_cached_quorum_last(None, last) == -2
    assert (cnt.value, miss.value, nb.value, c8.raw, list(last)) == (7, 7, 7, b"\x07" * 32, [7] * 6)     # nothing written


def test_python_surface(edc):
    pairs = {"quorum_verify_cached": "quorum_verify", "quorum_verify_cached_device": "quorum_verify_device",
             "quorum_verify_templated_cached": "quorum_verify_templated",
             "quorum_verify_templated_cached_device": "quorum_verify_templated_device"}
    for cached, plain in pairs.items():
        assert callable(getattr(edc.Engine, cached)), cached
        a, b = inspect.signature(getattr(edc.Engine, cached)), inspect.signature(getattr(edc.Engine, plain))
        assert [(p.name, p.default) for p in a.parameters.values()] == [(p.name, p.default) for p in b.parameters.values()], cached
    assert callable(edc.Engine.cached_quorum_last)
    p = inspect.signature(edc.batch.verify_quorum).parameters
    assert p["cached"].default is False
    assert list(p)[:4] == ["verifiers", "powers", "flags", "thresholds"]
    for cached in (False, True):                                                 # empty input: no engine is touched
        assert edc.batch.verify_quorum([], [], [], [], cached=cached) == ([], [], [])
