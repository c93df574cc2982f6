"""CPU: the quorum commit-set entries (edc_quorum_*) exist in the header, the library and the Python
surface; a NULL context is an argument error on each; the constants exist; the host-side logic of
csrc/quorum.h holds under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program;
and tests/golden/quorum.json agrees with the model and the rule of its generator and contains every
situation it was laid out for. No compute calls (no GPU here)."""
import ctypes
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT, golden
from test_sanitizers import SAN

ENTRIES = ["edc_quorum_plan", "edc_quorum_verify_device", "edc_quorum_verify"]
CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")


def gen_quorum():
    spec = importlib.util.spec_from_file_location("gen_quorum", os.path.join(GOLDEN, "gen_quorum.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    declared = sorted(set(re.findall(r"\b(edc_quorum_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(ENTRIES)
    for s in ENTRIES + ["edc_debug_quorum_select"]:
        assert re.search(r"\bint\s+%s\s*\(\s*edc_ctx\s*\*\s*ctx\s*," % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    for name, value in [("EDC_QUORUM_SHORT", 3), ("EDC_NOT_CHECKED", 255), ("EDC_VOTE_ABSENT", 0), ("EDC_VOTE_COMMIT", 1),
                        ("EDC_VOTE_NIL", 2), ("EDC_QUORUM_FULL", 0), ("EDC_QUORUM_LIGHT", 1)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code), name


def test_header_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    sec = doc[doc.index("Quorum commit sets: tally voting power"):doc.index("int edc_quorum_plan(")]
    for call in ("VerifyCommit ", "VerifyCommitLight ", "VerifyCommitLightTrusting"):
        assert call in sec
    assert "The reference crate has no such API and none of its APIs changes meaning" in sec
    assert "STRICTLY GREATER" in sec and "also with threshold 0" in sec
    assert "src/batch.rs:104-107" in sec and "src/batch.rs:127-137" in sec
    for out_of_scope in ("asynchronous", "templated", "incremental verifier", "multi-GPU"):
        assert out_of_scope in sec[sec.index("Out of scope"):]


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    thr = (ctypes.c_uint64 * 1)(0)
    pw = (ctypes.c_uint64 * 1)(0)
    cnt, nb, ms = ctypes.c_size_t(7), ctypes.c_int(7), ctypes.c_float(7)
    assert lib.edc_quorum_plan(None, 1, off, pw, b"\0", thr, 1, None, None, ctypes.byref(cnt)) == -2
    assert lib.edc_quorum_verify_device(None, 1, off, None, None, None, None, None, None, None, thr, 1, seed, None, None,
                                        None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_quorum_verify(None, 1, off, None, None, None, None, None, None, pw, b"\0", thr, 1, seed, None, None,
                                 None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_debug_quorum_select(None, 1, off, pw, b"\0", thr, 1, 1, ctypes.byref(ms)) == -2
    assert (cnt.value, nb.value, ms.value) == (7, 7, 7.0)            # nothing written


def test_python_surface(edc):
    for name in ("quorum_plan", "quorum_verify", "quorum_verify_device"):
        assert callable(getattr(edc.Engine, name))
    assert callable(edc.batch.verify_quorum)
    assert issubclass(edc.QuorumShort, edc.Error)
    assert (edc.EDC_QUORUM_SHORT, edc.NOT_CHECKED) == (3, 255)
    assert (edc.VOTE_ABSENT, edc.VOTE_COMMIT, edc.VOTE_NIL) == (0, 1, 2)
    assert (edc.QUORUM_FULL, edc.QUORUM_LIGHT) == (0, 1)
    # what needs no GPU, and what is refused before one is touched
    assert edc.batch.verify_quorum([], [], [], []) == ([], [], [])
    v = edc.batch.Verifier()
    v.queue((bytes(32), bytes(64), b"m"))
    for bad in [dict(powers=[[1, 2]], flags=[[1]], thresholds=[0]), dict(powers=[[1]], flags=[[1]], thresholds=[]),
                dict(powers=[[1]], flags=[[1]], thresholds=[0], z_seed=b"short")]:
        with pytest.raises(ValueError):
            edc.batch.verify_quorum([v], **bad)
    with pytest.raises(TypeError):
        edc.batch.verify_quorum([object()], [[1]], [[1]], [0])


def test_model_on_small_cases():
    """The model against cases worked out by hand from the header's definitions."""
    g = gen_quorum()
    off, power, flag = [0, 4, 4, 6], [5, 5, 5, 5, 7, 7], [1, 1, 1, 1, 0, 2]
    # threshold equal to the running sum: the next item is still checked; a tally equal to the threshold is short
    chk, planned = g.select(off, power, flag, [10, 0, 0], g.LIGHT)
    assert (chk, planned) == ([1, 1, 1, 0, 0, 0], [15, 0, 0])
    chk, planned = g.select(off, power, flag, [10, 0, 0], g.FULL)
    assert (chk, planned) == ([1, 1, 1, 1, 0, 1], [20, 0, 0])
    j = g.judge(off, power, flag, [15, 0, 0], g.LIGHT, [0] * 6)
    assert j["tally"] == [20, 0, 0] and j["commit_verdicts"] == [g.OK, g.SHORT, g.SHORT] and j["code"] == g.SHORT
    assert j["item_verdicts"] == [0, 0, 0, 0, 255, 255] and j["n_checked"] == 4 and j["n_bad_commits"] == 2
    j = g.judge(off, power, flag, [20, 0, 0], g.LIGHT, [0] * 6)
    assert j["commit_verdicts"][0] == g.SHORT                        # 20 is not strictly greater than 20
    # a bad vote before the quorum: invalid, its power missing from the tally; a bad nil vote counts in full mode only
    j = g.judge(off, power, flag, [9, 0, 0], g.LIGHT, [1, 0, 0, 0, 0, 1])
    assert j["checked"] == [1, 1, 0, 0, 0, 0] and j["tally"][0] == 5 and j["commit_verdicts"] == [g.INVALID, g.SHORT, g.SHORT]
    j = g.judge(off, power, flag, [9, 0, 0], g.FULL, [0, 0, 0, 0, 1, 1])
    assert j["commit_verdicts"] == [g.OK, g.SHORT, g.INVALID] and j["item_verdicts"][4:] == [255, 1] and j["code"] == g.INVALID
    assert not g.check_args([0, 1], [1], [3], [0]) and not g.check_args([0, 1], [2**63], [0], [0])
    assert not g.check_args([0, 2], [2**62, 2**62], [1, 1], [0]) and g.check_args([0, 2], [2**62, 2**62], [1, 2], [0])


def test_fixture_is_what_the_generator_makes():
    g, fx = gen_quorum(), golden("quorum.json")
    assert fx["rule"] == g.RULE
    for name in g.RULE["sets"]:
        want = g.expected(name)
        got = dict(fx["sets"][name])
        got.pop("situations", None)
        assert got == want, name
    gc = g._gen_commits()
    b = gc.build("mixed_a")
    off = b["commit_off"]
    power, flag, thr = g.votes("mixed_a", off, gc)
    codes = g.item_codes("mixed_a")
    found = g.situations(off, power, flag, thr, codes, b["corpus_commit"])
    found["garbage"] = [i for i, vk, sig in g.garbage("mixed_a", gc) if flag[i] == g.ABSENT and len(vk) == 32 and len(sig) == 64]
    assert found == fx["sets"]["mixed_a"]["situations"]
    for kind in ("after", "before", "missing", "nil_bad", "garbage", "corpus"):
        assert found[kind], kind
    # the listed situations, spelled out on the fixture's own numbers
    full, light = fx["sets"]["mixed_a"]["full"], fx["sets"]["mixed_a"]["light"]
    c = found["after"][0]
    assert (light["commit_verdicts"][c], full["commit_verdicts"][c]) == (g.OK, g.INVALID)
    c = found["missing"][0]
    assert light["commit_verdicts"][c] == g.INVALID and light["tally"][c] <= thr[c] < light["planned"][c]
    i = found["nil_bad"][0]
    assert flag[i] == g.NIL and codes[i] != g.OK
    assert hashlib.sha256(bytes(g.select(off, power, flag, thr, g.LIGHT)[0])).hexdigest() == light["checked_sha256"]
    # every bad item of commits.json is accounted for
    assert sorted(i for i, c in enumerate(codes) if c) == [346, 645, 700, 800, 2047]


def test_quorum_host_logic_sanitized(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "quorum")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "quorum_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    status, checks = p.stdout.split()
    assert status == "ok" and int(checks) > 1000
