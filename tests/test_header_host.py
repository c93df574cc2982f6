"""CPU: the header hashes (include/edc.h, "Header hashes"). csrc/hdrhash.h, the host reference, and
the streaming leaf hash of csrc/sha256.h compiled for the host and reduced level by level as the root
kernel reduces, in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, against
the model of tests/header_model.py (hashlib); the model against values worked out by hand and against
its fixture; the header, the library and the Python surface; cometbft_header_leaves against bytes
written out by hand. No compute calls (no GPU here)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

import header_model as hm
from conftest import ROOT, golden
from test_sanitizers import SAN

CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")
ENTRIES = ["edc_header_hashes", "edc_header_bind", "edc_debug_header_ms"]
COUNTS = list(range(18)) + [31, 32, 33, 63, 64]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("header") / "header")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC,      # sha256.h: #pragma unroll
                           os.path.join(ROOT, "tests", "native", "header_main.cpp"), "-o", exe])
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
    h = hm.sha256
    assert h(b"").hex() == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"
    # RFC 6962 on 0, 1, 2, 3 and 5 leaves of different lengths, the empty one among them, written out
    L = [b"", b"a", b"bc" * 40, bytes(range(55)), b"\x00" * 200]
    lh = [h(b"\x00" + x) for x in L]
    node = lambda a, b: h(b"\x01" + a + b)
    assert hm.mth([]) == h(b"") and hm.mth(L[:1]) == lh[0] == h(b"\x00") and hm.mth(L[:2]) == node(lh[0], lh[1])
    assert hm.mth(L[:3]) == node(node(lh[0], lh[1]), lh[2])
    assert hm.mth(L) == node(node(node(lh[0], lh[1]), node(lh[2], lh[3])), lh[4])
    # the byte rule: the leaf exists, holds P + 32 bytes, and they are the source
    s = bytes(range(100, 132))
    hd = [b"x", b"\x0a\x20" + s, b"\x0a\x20" + s[:31]]
    assert hm.rule(hd, 1, 2, s) and not hm.rule(hd, 1, 1, s) and not hm.rule(hd, 1, 3, s)
    assert not hm.rule(hd, 2, 2, s) and not hm.rule(hd, 3, 2, s) and not hm.rule(hd, 0, 0, s)
    assert hm.rule([s], 0, 0, s) and not hm.rule([hm.flip(s, 31)], 0, 0, s)
    # the four rules and their bits
    r = [hm.mth(x) for x in ([b"q"], [b"\x0a\x20" + hm.mth([b"q"])])]
    two = [[b"q"], [b"\x0a\x20" + r[0]]]
    assert hm.bind(two, expect=r, link=[None, 0], link_at=(0, 2)) == ([0, 0], 0, r)
    assert hm.bind(two, expect=[r[1], r[1]], link=[0, 1], link_at=(0, 2))[:2] == ([hm.BAD_HASH | hm.BAD_LINK, hm.BAD_LINK], 2)
    assert hm.bind(two, vals=[hm.NONE, 0], nexts=[None, 1], set_roots=[r[0], r[1]], vals_at=(0, 2), next_at=(0, 2))[0] == \
        [0, hm.BAD_NEXT]
    assert (hm.BAD_HASH, hm.BAD_VALS, hm.BAD_NEXT, hm.BAD_LINK, hm.NONE, hm.MAX_LEAVES) == (1, 2, 4, 8, 0xFFFFFFFF, 64)
    # a shaped header: 14 leaves, a 72-byte block id, the hashes behind 0A 20
    rnd = random.Random(1)
    sh = hm.shaped(rnd, 300, b"\x11" * 32, b"\x22" * 32, b"\x33" * 32)
    assert len(sh) == 14 and len(sh[4]) == 72 and sh[2] == b"\x08\xac\x02"
    assert (sh[4][:2], sh[4][2:34], sh[7], sh[8][2:]) == (b"\x0a\x20", b"\x11" * 32, b"\x0a\x20" + b"\x22" * 32, b"\x33" * 32)


def test_fixture_is_what_the_model_makes():
    g = golden("header.json")
    assert g == hm.golden()
    assert 24 <= len(g["headers"]) <= 48 and g["n_bad"] == sum(1 for f in g["bad"] if f) > 0
    seen = 0
    for f in g["bad"]:
        seen |= f
    assert seen == 15 and 0 in g["bad"]                      # every bit occurs, and headers without any


def _hdr(skip, leaves):
    return "hdr %d %d %s" % (skip, len(leaves), " ".join(x.hex() or "-" for x in leaves))


def test_leaf_lengths_and_alignments(program, tmp_path):
    """every length of the list as a single leaf at every start offset mod 4, and all of them packed
    back to back in one header, whose starts then fall on all four alignments as well"""
    rnd = random.Random("header lengths")
    cases = [(skip, [bytes(rnd.randrange(256) for _ in range(n))]) for n in hm.LENGTHS for skip in range(4)]
    packed = [bytes(rnd.randrange(256) for _ in range(n)) for n in hm.LENGTHS]
    starts = {sum(len(x) for x in packed[:j]) % 4 for j in range(len(packed))}
    assert starts == {0, 1, 2, 3}
    cases += [(skip, packed) for skip in range(4)] + [(skip, packed[::-1]) for skip in range(4)]
    cases.append((0, [b""] * 5))
    cases.append((0, [bytes(72)]))
    for (skip, leaves), line in zip(cases, run(program, tmp_path, [_hdr(*c) for c in cases])):
        want = hm.mth(leaves).hex()
        assert line.split() == [want, want], (skip, [len(x) for x in leaves], line)   # hdrhash.h; sha256.h level by level


def test_leaf_counts(program, tmp_path):
    rnd = random.Random("header counts")
    cases = [(n % 4, hm.random_leaves(rnd, n)) for n in COUNTS]
    cases += [(1, hm.random_leaves(rnd, n, [0])) for n in (1, 2, 7)]          # every leaf empty
    for (skip, leaves), line in zip(cases, run(program, tmp_path, [_hdr(*c) for c in cases])):
        want = hm.mth(leaves).hex()
        assert line.split() == [want, want], (len(leaves), line)


def _bind_line(headers, expect, rules, set_roots):
    """rules: three of None or (leaf, pos, entries)"""
    parts = ["bind %d" % len(headers)]
    for h in headers:
        parts.append("%d %s" % (len(h), " ".join(x.hex() or "-" for x in h)) if h else "0")
    parts.append("E " + (" ".join(e.hex() for e in expect) if expect else "-"))
    for r in rules:
        parts.append("-" if r is None else "%d %d %s" % (r[0], r[1], " ".join(str(hm.NONE if x is None else x) for x in r[2])))
    parts.append("%d %s" % (len(set_roots), " ".join(s.hex() for s in set_roots)))
    return " ".join(p for p in parts if p)


def test_rules_of_the_host_reference(program, tmp_path):
    g = hm.golden()
    un = bytes.fromhex
    headers = [[un(x) for x in h] for h in g["headers"]]
    expect = [un(e) for e in g["expect"]]
    import valhash_model as vm
    set_roots = vm.history_roots([un(k) for k in g["keys"]], g["base"], [[tuple(pw) for pw in u] for u in g["updates"]])
    rnd = random.Random("header host rules")
    small, sv, sn, sl = hm.chain(rnd, 6, set_roots)
    short = [list(h) for h in small]
    short[2][7] = short[2][7][:33]                             # P + 31 bytes
    short[3] = short[3][:7]                                    # the rule's leaf index = the leaf count
    cases = [
        (headers, expect, [(7, 2, g["vals"]), (8, 2, g["nexts"]), (4, 2, g["link"])]),
        (headers, None, [None, None, None]),
        (small, None, [(7, 2, sv), None, (4, 2, sl)]),
        (short, None, [(7, 2, sv), (8, 2, sn), (4, 2, sl)]),
        (small, None, [(7, 1, sv), (8, 3, sn), (4, 0, sl)]),     # other positions: nothing matches
        (small[::-1], None, [None, None, (4, 2, [1, 2, 3, 4, 5, None])]),   # the array reversed: forward links
    ]
    lines = [_bind_line(h, e, r, set_roots) for h, e, r in cases]
    for (h, e, r), line in zip(cases, run(program, tmp_path, lines)):
        kw = {}
        for name, at, rule in zip(("vals", "nexts", "link"), ("vals_at", "next_at", "link_at"), r):
            if rule is not None:
                kw[name], kw[at] = rule[2], (rule[0], rule[1])
        bad, n_bad, roots = hm.bind(h, expect=e, set_roots=set_roots, **kw)
        got = line.split()
        assert got[0] == bytes(bad).hex() and int(got[1]) == n_bad and got[2:] == [x.hex() for x in roots]
    assert hm.bind(short, vals=sv, nexts=sn, link=sl, set_roots=set_roots)[0] == \
        [0, 0, hm.BAD_VALS, 14, hm.BAD_LINK, 0]                # a changed header also changes the root its successor names
    assert hm.bind(small[::-1], link=[1, 2, 3, 4, 5, None])[:2] == ([0] * 6, 0)


def test_header_library_and_python_surface(edc):
    head = open(os.path.join(ROOT, "include", "edc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    lib = edc.load_library()
    assert sorted(set(re.findall(r"\b(edc_(?:debug_)?header_[a-z0-9_]+)\s*\(", code))) == sorted(ENTRIES)
    for s in ENTRIES:
        assert hasattr(lib, s) and s in edc.ABI_SYMBOLS
        assert code.index("edc_debug_valhash_ms(") < code.index(s + "(") < code.index("edc_create_multi(")
    for name, value in (("MAX_LEAVES", "64"), ("NONE", "0xFFFFFFFFu"), ("BAD_HASH", "1"), ("BAD_VALS", "2"), ("BAD_NEXT", "4"),
                        ("BAD_LINK", "8")):
        assert re.search(r"#define\s+EDC_HEADER_%s\s+%s\b" % (name, value), code), name
    assert (edc.HEADER_MAX_LEAVES, edc.HEADER_NONE) == (hm.MAX_LEAVES, hm.NONE)
    assert (edc.HEADER_BAD_HASH, edc.HEADER_BAD_VALS, edc.HEADER_BAD_NEXT, edc.HEADER_BAD_LINK) == (1, 2, 4, 8)
    doc = " ".join(head.replace("*", " ").split())
    sec = doc[doc.index("Header hashes: the Merkle root"):doc.index("#define EDC_HEADER_MAX_LEAVES")]
    for words in ("stated from memory", "largest power of two below n", "a mismatch is data", "EDC_HEADER_MAX_LEAVES = 64",
                  "L < n, leaf L has at least P + 32 bytes", "may name the header itself", "writes only n_bad = 0"):
        assert words in sec, words
    # the structures as the header lays them out on a 64-bit host
    assert (ctypes.sizeof(edc.EdcHeaderSet), ctypes.sizeof(edc.EdcHeaderRules)) == (40, 64)
    for name in ("header_hashes", "header_bind", "header_ms"):
        assert callable(getattr(edc.Engine, name))
    assert callable(edc.batch.header_hashes) and callable(edc.batch.verify_headers) and callable(edc.batch.cometbft_header_leaves)
    for call in (lambda: edc.batch.header_hashes([[b"x"]], engine=object()), lambda: edc.batch.verify_headers([[b"x"]], engine=object())):
        with pytest.raises(ValueError):
            call()
    # a NULL context is an argument error, with nothing written
    hs, keep = edc.Engine._header_set([[b"leaf"]])
    rules = edc.EdcHeaderRules(ctypes.sizeof(edc.EdcHeaderRules), 0)
    out, bad, n_bad = ctypes.create_string_buffer(b"\x07" * 32, 32), ctypes.create_string_buffer(b"\x07", 1), ctypes.c_size_t(7)
    ms = (ctypes.c_float * 2)(7, 7)
    assert lib.edc_header_hashes(None, ctypes.byref(hs), out) == -2
    assert lib.edc_header_bind(None, ctypes.byref(hs), ctypes.byref(rules), bad, out, ctypes.byref(n_bad)) == -2
    assert lib.edc_debug_header_ms(None, ctypes.byref(hs), 1, ms) == -2
    assert (out.raw, bad.raw, n_bad.value, ms[0], ms[1]) == (b"\x07" * 32, b"\x07", 7, 7.0, 7.0)


def test_cometbft_header_leaves_by_hand(edc):
    leaves = edc.batch.cometbft_header_leaves
    h32 = lambda b: bytes([b]) * 32
    full = leaves(version_block=11, version_app=1, chain_id="test-chain", height=300, time_seconds=1700000000,
                  time_nanos=5, last_block_hash=h32(1), last_parts_total=1, last_parts_hash=h32(2), last_commit_hash=h32(3),
                  data_hash=h32(4), validators_hash=h32(5), next_validators_hash=h32(6), consensus_hash=h32(7),
                  app_hash=b"\xaa\xbb", last_results_hash=h32(9), evidence_hash=h32(10), proposer_address=bytes([12]) * 20)
    assert full == [
        bytes([0x08, 0x0B, 0x10, 0x01]),
        bytes([0x0A, 0x0A]) + b"test-chain",
        bytes([0x08, 0xAC, 0x02]),                             # 300: a two-byte varint
        bytes([0x08, 0x80, 0xE2, 0xCF, 0xAA, 0x06, 0x10, 0x05]),   # 1700000000 = 0x6553F100
        bytes([0x0A, 0x20]) + h32(1) + bytes([0x12, 0x24, 0x08, 0x01, 0x12, 0x20]) + h32(2),
        bytes([0x0A, 0x20]) + h32(3), bytes([0x0A, 0x20]) + h32(4), bytes([0x0A, 0x20]) + h32(5), bytes([0x0A, 0x20]) + h32(6),
        bytes([0x0A, 0x20]) + h32(7), bytes([0x0A, 0x02, 0xAA, 0xBB]), bytes([0x0A, 0x20]) + h32(9), bytes([0x0A, 0x20]) + h32(10),
        bytes([0x0A, 0x14]) + bytes([12]) * 20,
    ]
    assert len(full) == 14 and len(full[4]) == 72 and full[7][2:] == h32(5) and full[4][2:34] == h32(1)
    # zero and empty fields are omitted; the part-set header is always emitted
    assert leaves() == [b"", b"", b"", b"", bytes([0x12, 0x00])] + [b""] * 9
    zero = leaves(version_block=11, chain_id="c", height=0, time_nanos=7, last_parts_total=3, app_hash=b"", validators_hash=h32(5))
    assert zero[0] == bytes([0x08, 0x0B]) and zero[1] == bytes([0x0A, 0x01, 0x63]) and zero[2] == b"" and zero[10] == b""
    assert zero[3] == bytes([0x10, 0x07]) and zero[4] == bytes([0x12, 0x02, 0x08, 0x03]) and zero[7] == bytes([0x0A, 0x20]) + h32(5)
    assert leaves(last_parts_hash=h32(2))[4] == bytes([0x12, 0x22, 0x12, 0x20]) + h32(2)
    assert leaves(last_block_hash=h32(1))[4] == bytes([0x0A, 0x20]) + h32(1) + bytes([0x12, 0x00])
    assert leaves(height=128)[2] == bytes([0x08, 0x80, 0x01]) and leaves(height=127)[2] == bytes([0x08, 0x7F])
    assert leaves(height=-1)[2] == bytes([0x08]) + b"\xff" * 9 + b"\x01"      # int64: two's complement, 10 bytes
    assert leaves(last_parts_total=300)[4] == bytes([0x12, 0x03, 0x08, 0xAC, 0x02])
