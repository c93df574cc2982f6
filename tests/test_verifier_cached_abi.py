"""CPU: the cached incremental verifier's entries exist in the C ABI and in Python, a NULL verifier
is an argument error on each, the header states what cached mode is worth, and the host-side
bookkeeping (csrc/vfy_cached.h) holds under AddressSanitizer + UndefinedBehaviorSanitizer in a
stand-alone program. No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

from conftest import ROOT

NEW_SYMBOLS = ["edc_vfy_set_cached", "edc_vfy_cached", "edc_vfy_cache_counts", "edc_vfy_verify_fallback_offered"]


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*(const\s+)?edc_verifier\s*\*" % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS


def test_null_verifier_is_an_argument_error(edc):
    lib = edc.load_library()
    offered, hits, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(7)
    buf = ctypes.create_string_buffer(32)
    assert lib.edc_vfy_set_cached(None, 1) == -2
    assert lib.edc_vfy_cached(None) == -2
    assert lib.edc_vfy_cache_counts(None, ctypes.byref(offered), ctypes.byref(hits)) == -2
    assert (offered.value, hits.value) == (7, 7)
    assert lib.edc_vfy_verify_fallback_offered(None, bytes(32), buf, ctypes.byref(cnt), buf) == -2


def test_stream_verifier_surface(edc):
    sv = edc.batch.StreamVerifier
    for f in (sv.__init__, sv.new):
        p = inspect.signature(f).parameters
        assert "cached" in p and p["cached"].default is False
        assert p["eager"].default is False
    assert isinstance(getattr(sv, "cached", None), property)
    assert isinstance(getattr(sv, "cache_counts", None), property)
    assert "on" in inspect.signature(sv.set_cached).parameters
    assert "z_seed" in inspect.signature(sv.verify_with_fallback_offered).parameters


def test_header_states_soundness_of_cached_mode():
    doc = " ".join(_header().replace("*", " ").split())
    m = re.search(r"Soundness of cached mode\. A hit is worth.*?every prehashed entry\.", doc)
    assert m, "include/edc.h: the soundness paragraph of cached mode is missing"
    par = m.group(0)
    for phrase in ("byte-identical (vk, sig, k)", "batch whose equation held", "plants records", "fresh and secret",
                   "also in eager mode", "caller vouches for k"):
        assert phrase in par, phrase
    assert "Item::verify_single code (src/batch.rs:104-107)" in doc


def test_bookkeeping_under_sanitizers(tmp_path):
    assert shutil.which("g++"), "a host C++ compiler is needed to build the stand-alone check"
    exe = str(tmp_path / "vfy_cached")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "ed25519-consensus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "vfy_cached_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and "Sanitizer" not in p.stderr, p.stderr[-2000:]
