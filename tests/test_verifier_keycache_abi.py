"""CPU: the incremental verifier's entries for a registered validator set exist in the C ABI and
in Python (no compute calls, no GPU)."""
import os
import re

from conftest import ROOT

NEW_SYMBOLS = ["edc_vfy_queue_indexed", "edc_vfy_last_split"]


def _header():
    src = open(os.path.join(ROOT, "include", "edc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_new_entries():
    src = _header()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*(const\s+)?edc_verifier\s*\*" % s, src), s


def test_library_exports_the_new_symbols(edc):
    lib = edc.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS


def test_null_handles_are_argument_errors(edc):
    lib = edc.load_library()
    assert lib.edc_vfy_queue_indexed(None, 0, None, None, None, None, None) == -2
    assert lib.edc_vfy_last_split(None) == -2


def test_stream_verifier_surface(edc):
    sv = edc.batch.StreamVerifier
    assert callable(getattr(sv, "queue_indexed", None))
    assert isinstance(getattr(sv, "last_split", None), property)
