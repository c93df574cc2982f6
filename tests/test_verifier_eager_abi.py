"""CPU: the eager incremental verifier's entries exist in the C ABI and in Python (no compute calls,
no GPU)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

NEW_SYMBOLS = ["edc_vfy_begin_eager", "edc_vfy_set_fold", "edc_vfy_folded", "edc_vfy_eager"]


def _header():
    src = open(os.path.join(ROOT, "include", "edc.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_new_entries():
    src = _header()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*(const\s+)?edc_verifier\s*\*" % s, src), s


def test_header_documents_soundness():
    src = open(os.path.join(ROOT, "include", "edc.h")).read()
    assert "Soundness" in src and "spent" in src


def test_library_exports_the_new_symbols(edc):
    lib = edc.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS


def test_null_handles_are_argument_errors(edc):
    lib = edc.load_library()
    items, folds = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.edc_vfy_eager(None) == -2
    assert lib.edc_vfy_folded(None, ctypes.byref(items), ctypes.byref(folds)) == -2
    assert (items.value, folds.value) == (7, 7)
    assert lib.edc_vfy_begin_eager(None, bytes(32)) == -2
    assert lib.edc_vfy_set_fold(None, 1) == -2


def test_stream_verifier_surface(edc):
    sv = edc.batch.StreamVerifier
    assert "eager" in inspect.signature(sv.__init__).parameters
    assert inspect.signature(sv.__init__).parameters["eager"].default is False
    assert "seed" in inspect.signature(sv.begin_eager).parameters
    assert callable(getattr(sv, "set_fold", None))
    assert isinstance(getattr(sv, "folded", None), property)
    assert isinstance(getattr(sv, "eager", None), property)
