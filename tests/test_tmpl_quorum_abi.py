"""CPU: the templated quorum commit-set entries (edc_tmpl_quorum_*) exist in the header, the library
and the Python surface; a NULL context is an argument error on each with nothing written; the header
section states the equality contract and "select first". No compute calls (no GPU here).

The host-side checks of these entries are calls to the existing commits.h / tmpl.h / quorum.h
functions (held under sanitizers by test_commits_abi / test_tmpl_abi / test_quorum_abi), so there is
no new host-logic header and no new stand-alone program."""
import ctypes
import re
import os

from conftest import ROOT

ENTRIES = ["edc_tmpl_quorum_verify", "edc_tmpl_quorum_verify_device", "edc_debug_tmpl_quorum_last"]


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    for s in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?edc_ctx\s*\*\s*ctx\s*," % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    for s in ENTRIES[:2]:
        assert re.search(r"\b%s\s*\(\s*edc_ctx\s*\*\s*ctx\s*,\s*const\s+edc_templates\s*\*\s*ts\s*,\s*size_t\s+nc\s*,"
                         r"\s*const\s+uint32_t\s*\*\s*commit_off\s*,\s*const\s+uint16_t\s*\*\s*commit_tpl\s*,"
                         r"\s*uint32_t\s+alt_span\s*," % s, code), s
    # after the quorum entries, before the verified-signature cache
    assert code.index("edc_debug_quorum_select(") < min(code.index(s + "(") for s in ENTRIES)
    assert max(code.index(s + "(") for s in ENTRIES) < code.index("edc_sigcache_create(")


def test_header_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    sec = doc[doc.index("Templated quorum commit sets: hash only the votes that are checked"):
              doc.index("int edc_tmpl_quorum_verify(")]
    assert "Equality contract" in sec and "equals what edc_quorum_verify[_device] gives on the materialised messages" in sec
    for out in ("return value", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8"):
        assert out in sec[sec.index("Equality contract"):sec.index("Select first")], out
    assert "edc_batch_verify_prehashed_device on the gathered checked list with z_base = 0" in sec
    assert "Select first" in sec and "runs before any message exists" in sec
    assert "sized after the read-back of the checked count, from n_checked and not from n" in sec
    assert "BYTES never interpreted" in sec and "adds no stream synchronization" in sec
    assert "for ALL n items" in sec and "does not depend on the mode" in sec
    for cite in ("src/batch.rs:82-94", "src/batch.rs:127-137", ":149-217", "src/batch.rs:104-107"):
        assert cite in sec, cite
    # the quorum section points here instead of calling templated forms out of scope
    q = doc[doc.index("Quorum commit sets: tally voting power"):doc.index("int edc_quorum_plan(")]
    assert "templated forms are the edc_tmpl_quorum_ entries below" in q[q.index("Out of scope"):]


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    ctpl = (ctypes.c_uint16 * 1)(0)
    thr = (ctypes.c_uint64 * 1)(0)
    pw = (ctypes.c_uint64 * 1)(0)
    hoff = (ctypes.c_uint32 * 2)(0, 0)
    ts = edc.EdcTemplates(1, b"h", hoff, b"t", hoff)
    cnt, nb = ctypes.c_size_t(7), ctypes.c_int(7)
    last = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    assert lib.edc_tmpl_quorum_verify(None, ctypes.byref(ts), 1, off, ctpl, 1, None, None, None, None, None, hoff, pw, b"\0",
                                      thr, 1, seed, None, None, None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_tmpl_quorum_verify_device(None, ctypes.byref(ts), 1, off, ctpl, 1, None, None, None, None, None, 0, None,
                                             None, thr, 1, seed, None, None, None, ctypes.byref(nb), ctypes.byref(cnt),
                                             None) == -2
    assert lib.edc_debug_tmpl_quorum_last(None, last) == -2
    assert (cnt.value, nb.value, list(last)) == (7, 7, [7, 7, 7, 7])            # nothing written


def test_python_surface(edc):
    for name in ("quorum_verify_templated", "quorum_verify_templated_device", "tmpl_quorum_last"):
        assert callable(getattr(edc.Engine, name))
    import inspect
    p = list(inspect.signature(edc.Engine.quorum_verify_templated).parameters)
    assert p[1:10] == ["templates", "commit_off", "commit_tpl", "sigs", "holes", "powers", "flags", "thresholds", "z_seed"]
    for kw in ("light", "alt_span", "item_alt", "vks", "key_idx"):
        assert kw in p
    assert callable(edc.batch.verify_quorum)                                     # stays as it is
