"""CPU: the validator-set hashes (include/edc.h, "Validator-set hashes"). csrc/valhash.h, the host
reference, and csrc/sha256.h, the kernels' register-level SHA-256 compiled for the host and reduced
level by level as the root kernel reduces, in a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer, against the model of tests/valhash_model.py (hashlib and Python integers);
the model against values worked out by hand and against its fixture; the header, the library and the
Python surface. No compute calls (no GPU here)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

import valhash_model as vm
from conftest import ROOT, golden
from test_sanitizers import SAN

CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")
ENTRIES = ["edc_valhash_valset", "edc_valhash_vhist", "edc_valhash_vhist_match", "edc_debug_valhash_ms"]
# the edges of every uvarint length 1..9: 2^(7k) - 1 and 2^(7k), up to 2^63 - 1
UVARINTS = sorted({0, 1, vm.MAX_POWER} | {(1 << (7 * k)) - 1 for k in range(1, 10)} | {1 << (7 * k) for k in range(1, 9)})


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("valhash") / "valhash")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC,     # sha256.h: #pragma unroll
                           os.path.join(ROOT, "tests", "native", "valhash_main.cpp"), "-o", exe])
    return exe


def run(program, tmp_path, lines):
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([program, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    out = p.stdout.splitlines()
    assert out[-1] == "ok %d" % len(lines)
    return out[:-1]


def test_model_by_hand():
    assert vm.sha256(b"").hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    assert vm.sha256(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    assert [vm.uvarint(x).hex() for x in (0, 1, 127, 128, 300, 16383, 16384)] == \
        ["00", "01", "7f", "8001", "ac02", "ff7f", "808001"]
    assert vm.uvarint(vm.MAX_POWER) == b"\xff" * 8 + b"\x7f"
    assert [len(vm.uvarint(x)) for x in UVARINTS] == [1, 1, 1] + [k for k in range(2, 10) for _ in (0, 1)]
    k = bytes(range(32))
    assert vm.leaf(k, 0) == bytes([0x0A, 0x22, 0x0A, 0x20]) + k and len(vm.leaf(k, vm.MAX_POWER)) == 46
    assert vm.leaf(k, 300) == bytes([0x0A, 0x22, 0x0A, 0x20]) + k + bytes([0x10, 0xAC, 0x02])
    # RFC 6962 on 0, 1, 2, 3 and 5 leaves, written out
    L = [bytes([i]) * 36 for i in range(5)]
    h, lh = vm.sha256, [vm.sha256(b"\x00" + x) for x in L]
    node = lambda a, b: h(b"\x01" + a + b)
    assert vm.mth([]) == h(b"") and vm.mth(L[:1]) == lh[0] and vm.mth(L[:2]) == node(lh[0], lh[1])
    assert vm.mth(L[:3]) == node(node(lh[0], lh[1]), lh[2])
    assert vm.mth(L) == node(node(node(lh[0], lh[1]), node(lh[2], lh[3])), lh[4])
    # the order: power descending, then address ascending, then position
    keys = vm.make_keys(4)
    by_addr = sorted(range(4), key=lambda p: vm.address(keys[p]))
    assert [m[0] for m in vm.ordered([(p, keys[p], 5) for p in range(4)])] == by_addr
    assert [m[0] for m in vm.ordered([(p, keys[p], p) for p in range(4)])] == [3, 2, 1, 0]
    assert [m[0] for m in vm.ordered([(0, keys[0], 1), (1, keys[0], 1)])] == [0, 1]
    # the replayer: leaves, rejoins, a restated state, a position that never joins
    N = vm.NOT_MEMBER
    assert vm.replay([1, N, 3], [[(0, N)], [(0, 7), (2, 3)], []]) == [[1, N, 3], [N, N, 3], [7, N, 3], [7, N, 3]]


def test_fixture_is_what_the_model_makes():
    assert golden("valhash.json") == vm.golden()


def test_sha256_and_uvarint(program, tmp_path):
    rnd = random.Random("valhash sha")
    msgs = [b"", b"abc"] + [bytes(rnd.randrange(256) for _ in range(n)) for n in (55, 56, 63, 64, 65, 119, 120, 128, 300)]
    out = run(program, tmp_path, ["sha %s" % (m.hex() or "-") for m in msgs] + ["uv %d" % x for x in UVARINTS])
    assert out[:len(msgs)] == [vm.sha256(m).hex() for m in msgs]
    assert out[len(msgs):] == [vm.uvarint(x).hex() for x in UVARINTS]


def _sets():
    """member counts 0..17 with mixed powers; powers at every uvarint length; power 0; all equal; ascending"""
    rnd = random.Random("valhash sets")
    keys = vm.make_keys(40)
    sets = [[(p, keys[p], rnd.choice([0, 1, 5, 5, 9, 200, 1 << 20])) for p in range(n)] for n in range(18)]
    sets.append([(0, keys[0], vm.MAX_POWER)])
    sets.append([(p, keys[p], w) for p, w in enumerate(x for x in UVARINTS if x < 1 << 56)])
    sets.append([(p, keys[p], 0) for p in range(5)])
    sets.append([(p, keys[p], 77) for p in range(33)])
    sets.append([(p, keys[p], p + 1) for p in range(40)])
    return sets


def test_roots_recursive_and_levelwise(program, tmp_path):
    sets = _sets()
    lines = ["root %d %s" % (len(s), " ".join("%s %d" % (k.hex(), w) for _, k, w in s)) for s in sets]
    for s, line in zip(sets, run(program, tmp_path, lines)):
        want = vm.root(s).hex()
        assert line.split() == [want, want], (len(s), line)      # valhash.h's recursion; sha256.h level by level


def test_history_roots(program, tmp_path):
    rnd = random.Random("valhash hist")
    N = vm.NOT_MEMBER
    lines, want = [], []
    for m in (1, 2, 5, 9):
        keys = vm.make_keys(m, b"hist%d" % m)
        base = [rnd.choice([N, 0, 3, 10]) for _ in range(m)]
        updates = [[(p, rnd.choice([N, 0, 1, 4, 10])) for p in rnd.sample(range(m), rnd.randrange(0, min(m, 3) + 1))]
                   for _ in range(12)]
        flat = " ".join("%d %s" % (len(u), " ".join("%d %d" % pw for pw in u)) for u in updates)
        lines.append("hist %d %s %s %d %s" % (m, " ".join(k.hex() for k in keys), " ".join(map(str, base)), len(updates), flat))
        want.append(" ".join(r.hex() for r in vm.history_roots(keys, base, updates)))
    assert run(program, tmp_path, lines) == want


def test_header_library_and_python_surface(edc):
    head = open(os.path.join(ROOT, "include", "edc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    lib = edc.load_library()
    assert sorted(set(re.findall(r"\b(edc_(?:debug_)?valhash_[a-z0-9_]+)\s*\(", code))) == sorted(ENTRIES)
    for s in ENTRIES:
        assert hasattr(lib, s) and s in edc.ABI_SYMBOLS
        assert code.index("edc_debug_vq_trust_select(") < code.index(s + "(") < code.index("edc_create_multi(")
    assert re.search(r"#define\s+EDC_VALHASH_MAX_MEMBERS\s+4096\b", code)
    doc = " ".join(head.replace("*", " ").split())
    sec = doc[doc.index("Validator-set hashes: the Merkle root"):doc.index("#define EDC_VALHASH_MAX_MEMBERS")]
    for words in ("stated from memory", "first 20 bytes of SHA-256(key_p)", "power descending, then addr ascending",
                  "broken by position ascending", "0A 22 0A 20 | key_p | (10 | uvarint(w_p) if w_p > 0",
                  "largest power of two below n", "EDC_VALHASH_MAX_MEMBERS = 4096", "a mismatch is data",
                  "edc_keycache_add keeps them"):
        assert words in sec, words
    for name in ("valset_hash", "vhist_hashes", "vhist_hash_match", "valhash_ms"):
        assert callable(getattr(edc.Engine, name))
    assert callable(edc.batch.validator_set_hashes)
    with pytest.raises(ValueError):
        edc.batch.validator_set_hashes(expect=[bytes(32)], engine=object())
    # a NULL context is an argument error, with nothing written
    out, ok, bad = ctypes.create_string_buffer(b"\x07" * 32, 32), ctypes.create_string_buffer(b"\x07", 1), ctypes.c_size_t(7)
    ms = (ctypes.c_float * 2)(7, 7)
    ver = (ctypes.c_uint32 * 1)(0)
    assert lib.edc_valhash_valset(None, out) == -2 and lib.edc_valhash_vhist(None, 0, 1, out) == -2
    assert lib.edc_valhash_vhist_match(None, 1, ver, bytes(32), ok, ctypes.byref(bad)) == -2
    assert lib.edc_debug_valhash_ms(None, 1, ms) == -2
    assert (out.raw, ok.raw, bad.value, ms[0], ms[1]) == (b"\x07" * 32, b"\x07", 7, 7.0, 7.0)
