"""CPU: the validator-set quorum entries (include/edc.h, edc_valset_*) exist in the header, the library
and the Python surface; EDC_DOUBLE_VOTE is 4; a NULL context is an argument error on each entry; the
header section states the double-vote rule, the equality contract and what is not built; the model
of tests/golden/gen_valset.py holds on cases worked out by hand and agrees with valset.json; and the
host-side logic of csrc/valset.h, in a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer, agrees with that model on a few hundred random small sets. No compute
calls (no GPU here)."""
import ctypes
import importlib.util
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT, golden
from test_sanitizers import SAN

ENTRIES = ["edc_valset_set_powers", "edc_valset_size", "edc_valset_resolve", "edc_valset_quorum_verify_device",
           "edc_valset_quorum_verify", "edc_debug_valset_select"]
CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")


def gen_valset():
    spec = importlib.util.spec_from_file_location("gen_valset", os.path.join(GOLDEN, "gen_valset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    declared = sorted(set(re.findall(r"\b(edc_(?:debug_)?valset_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(ENTRIES)
    for s in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?edc_ctx\s*\*\s*ctx\s*[,)]" % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    assert re.search(r"#define\s+EDC_DOUBLE_VOTE\s+4\b", code)
    # where the section stands, and that it took no name of its neighbours
    assert code.index("edc_debug_cached_quorum_last(") < code.index("edc_valset_set_powers(")
    assert code.index("edc_debug_valset_select(") < code.index("edc_create_multi(")
    # the verify entries are the quorum entries' without the power array
    def args(name):
        a = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    assert args("edc_valset_quorum_verify_device") == [x for x in args("edc_quorum_verify_device") if x != "const uint64_t* d_power"]
    assert args("edc_valset_quorum_verify") == [x for x in args("edc_quorum_verify") if x != "const uint64_t* power"]


def test_header_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    sec = doc[doc.index("Validator-set quorum commit sets: powers and double votes"):doc.index("#define EDC_DOUBLE_VOTE")]
    assert "The reference crate has no such API and none of its APIs changes meaning" in sec
    for cite in ("src/batch.rs:76-94", "src/batch.rs:127-137", ":149-217", "src/batch.rs:104-107"):
        assert cite in sec
    rule = sec[sec.index("Double-vote rule."):sec.index("edc_valset_resolve the join")]
    assert "dv[c] = 1 iff two CHECKED items of commit c resolve to the same member" in rule
    assert "after the quorum is not checked" in rule and "a commit vote and a nil vote from one validator" in rule
    assert "two different commits is none" in rule and "two non-members never are" in rule
    eq = sec[sec.index("Equality contract."):sec.index("Stream synchronizations.")]
    assert "every output, check8 included, equals" in eq and "joined power / flag_out" in eq
    assert "except the verdicts of those commits, n_bad_commits and the return value" in eq
    assert "adds no stream synchronization" in sec
    assert "else EDC_INVALID_SIGNATURE if any" in sec and "else EDC_DOUBLE_VOTE if any" in sec
    nb = sec[sec.index("Not built:"):]
    for form in ("templated", "cached", "asynchronous", "incremental-verifier", "multi-GPU"):
        assert form in nb


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    thr = (ctypes.c_uint64 * 1)(0)
    pw = (ctypes.c_uint64 * 1)(0)
    cnt, nb = ctypes.c_size_t(7), ctypes.c_int(7)
    ms = (ctypes.c_float * 2)(7, 7)
    assert lib.edc_valset_set_powers(None, 1, pw) == -2
    assert lib.edc_valset_size(None) == 0
    assert lib.edc_valset_resolve(None, 1, off, None, None, b"\0", thr, 1, None, None, None, None, None, ctypes.byref(cnt),
                                  None) == -2
    assert lib.edc_valset_quorum_verify_device(None, 1, off, None, None, None, None, None, None, thr, 1, seed, None, None,
                                               None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_valset_quorum_verify(None, 1, off, None, None, None, None, None, None, b"\0", thr, 1, seed, None, None,
                                        None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_debug_valset_select(None, 1, off, None, None, b"\0", thr, 1, 1, ms) == -2
    assert (cnt.value, nb.value, ms[0], ms[1]) == (7, 7, 7.0, 7.0)            # nothing written


def test_python_surface(edc):
    for name in ("valset_set_powers", "valset_size", "valset_resolve", "quorum_verify_valset", "quorum_verify_valset_device",
                 "valset_select_ms"):
        assert callable(getattr(edc.Engine, name))
    assert issubclass(edc.DoubleVote, edc.Error) and not issubclass(edc.DoubleVote, edc.QuorumShort)
    assert (edc.EDC_DOUBLE_VOTE, edc.NO_POS) == (4, 0xFFFFFFFF)
    # what is refused before a GPU is touched
    v = edc.batch.Verifier()
    v.queue((bytes(32), bytes(64), b"m"))
    with pytest.raises(ValueError):
        edc.batch.verify_quorum([v], None, [[1]], [0], cached=True)
    with pytest.raises(ValueError):
        edc.batch.verify_quorum([v], None, [[1, 1]], [0])
    assert edc.batch.verify_quorum([], None, [], []) == ([], [], [])


def test_model_on_small_cases():
    """The model against cases worked out by hand from the header's definitions."""
    g = gen_valset()
    keys, powers = [bytes([i]) * 32 for i in (1, 2, 3)], [5, 5, 7]
    x = b"\x09" * 32
    assert g.resolve(keys, powers, [1, 2, 1, 1], vks=[keys[2], x, keys[0], keys[2]]) == \
        ([2, g.NO_POS, 0, 2], [7, 0, 5, 7], [1, 0, 1, 1])
    assert g.resolve(keys, powers, [1, 2, 0], key_idx=[1, 1, 0]) == ([1, 1, 0], [5, 5, 5], [1, 2, 0])
    # light mode, threshold 7: member 2 (7) then member 2 again: 7 <= 7, so the second is checked
    p = g.plan(keys, powers, [0, 3], [1, 1, 1], [7], g.LIGHT, vks=[keys[2], keys[2], keys[0]])
    assert (p["checked"], p["planned"], p["dv"]) == ([1, 1, 0], [14], [1])
    p = g.plan(keys, powers, [0, 3], [1, 1, 1], [6], g.LIGHT, vks=[keys[2], keys[2], keys[0]])
    assert (p["checked"], p["planned"], p["dv"]) == ([1, 0, 0], [7], [0])
    p = g.plan(keys, powers, [0, 3], [1, 1, 1], [6], g.FULL, vks=[keys[2], keys[2], keys[0]])
    assert (p["checked"], p["dv"]) == ([1, 1, 1], [1])
    # commit + nil in full mode; the same validator in two commits; strangers
    assert g.plan(keys, powers, [0, 2], [1, 2], [0], g.FULL, key_idx=[1, 1])["dv"] == [1]
    assert g.plan(keys, powers, [0, 2], [1, 2], [0], g.LIGHT, key_idx=[1, 1])["dv"] == [0]
    assert g.plan(keys, powers, [0, 1, 2], [1, 1], [0, 0], g.FULL, key_idx=[1, 1])["dv"] == [0, 0]
    assert g.plan(keys, powers, [0, 2], [1, 1], [0], g.FULL, vks=[x, x]) == \
        {"pos": [g.NO_POS] * 2, "power": [0, 0], "flag": [0, 0], "checked": [0, 0], "planned": [0], "n_checked": 0, "dv": [0]}
    # the verdicts and the precedence of the return value
    j = g.judge(keys, powers, [0, 2, 3, 4], [1, 1, 1, 1], [0, 0, 20], g.FULL, [0, 0, 0, 0], key_idx=[0, 0, 1, 2])
    assert j["commit_verdicts"] == [4, 0, 3] and j["code"] == 4 and j["n_bad_commits"] == 2 and j["tally"][0] == 10
    assert j["quorum_verdicts"] == [0, 0, 3] and j["quorum_code"] == 3
    j = g.judge(keys, powers, [0, 2, 3, 4], [1, 1, 1, 1], [0, 0, 20], g.FULL, [0, 1, 1, 0], key_idx=[0, 0, 1, 2])
    assert j["commit_verdicts"] == [4, 1, 3] and j["code"] == 1 and j["item_verdicts"] == [0, 1, 1, 0]
    j = g.judge(keys, powers, [0, 2, 3], [1, 1, 1], [0, 0], g.FULL, [0, 0, 0], key_idx=[0, 0, 1])
    assert j["commit_verdicts"] == [4, 0] and j["code"] == 4
    # the rules of the powers and of the votes
    assert g.check_powers(keys, powers) and not g.check_powers(keys, powers[:2]) and not g.check_powers([], [])
    assert not g.check_powers(keys[:2] + keys[:1], powers) and not g.check_powers(keys, [1, 2**63, 1])
    assert g.check_powers(keys, [2**63 - 3, 1, 1]) and not g.check_powers(keys, [2**63 - 2, 1, 1])
    big = [2**62, 1, 1]
    pos, power, flag_out = g.resolve(keys, big, [1, 1], key_idx=[0, 0])
    assert not g.check_args([0, 2], [1, 1], power, flag_out) and g.check_args([0, 1, 2], [1, 1], power, flag_out)
    pos, power, flag_out = g.resolve(keys, big, [3], vks=[x])
    assert flag_out == [0] and not g.check_args([0, 1], [3], power, flag_out)        # a flag of 3 on a non-member


def test_fixture_is_what_the_generator_makes():
    g, fx = gen_valset(), golden("valset.json")
    assert fx["powers"] == g.POWERS and sorted(fx["cases"]) == sorted(g.CASES)
    for name in g.CASES:
        assert fx["cases"][name] == g.expected(name), name
    c = fx["cases"]
    assert (c["second_before_quorum"]["light"]["dv"], c["second_after_quorum"]["light"]["dv"]) == ([1], [0])
    assert c["second_after_quorum"]["full"]["dv"] == [1]
    assert (c["commit_and_nil"]["full"]["dv"], c["commit_and_nil"]["light"]["dv"]) == ([1], [0])
    assert c["two_commits_one_validator"]["full"]["dv"] == [0, 0] and c["strangers_twice"]["full"]["dv"] == [0]
    assert c["last_commit_then_empty"]["light"]["commit_verdicts"] == [0, 3, 4, 3, 3]
    assert (c["with_invalid"]["full"]["code"], c["with_short"]["full"]["code"]) == (1, 4)
    assert c["double_and_bad"]["full"]["commit_verdicts"] == [4, 0] and c["double_and_bad"]["full"]["item_verdicts"][1] == 1


def _random_case(rnd, g):
    """One small set: a list of 1..6 keys (sometimes with a repeated key or powers that do not fit),
    commits of 0..6 votes with non-members, duplicates, every flag (sometimes a 3), by key or by position."""
    m = rnd.randrange(1, 7)
    keys = [rnd.randbytes(32) for _ in range(m)]
    kind = rnd.randrange(12)
    if kind == 0 and m > 1:
        keys[rnd.randrange(1, m)] = keys[0]
    powers = [rnd.randrange(0, 10) for _ in range(m)]
    if kind == 1:
        powers[rnd.randrange(m)] = rnd.choice([2**63, 2**64 - 1])
    if kind == 2:
        powers = [2**63 // m + 1] * m                      # every power fits, their sum does not
    if kind == 3:
        powers[0] = 2**62 + 7                              # fits; a commit that counts it twice does not
    nc = rnd.randrange(0, 6)
    off = [0]
    for _ in range(nc):
        off.append(off[-1] + rnd.choice([0, 0, 1, 2, 3, 4, 6]))
    n = off[-1]
    form = rnd.randrange(2)
    mode = rnd.randrange(2)
    flip = bytearray(keys[0])
    flip[rnd.randrange(32)] ^= 1 << rnd.randrange(8)
    strangers = [bytes(32), bytes(flip), rnd.randbytes(32)]
    who = [rnd.randrange(m) if form or rnd.randrange(3) else None for _ in range(n)]
    vks = [keys[w] if w is not None else rnd.choice(strangers) for w in who]
    flag = [rnd.choice([0, 1, 1, 1, 1, 2]) for _ in range(n)]
    if kind == 4 and n:
        flag[rnd.randrange(n)] = 3
    thr = [rnd.choice([0, 4, 9, 14, 2**62, 2**64 - 1]) for _ in range(nc)]
    codes = [rnd.choice([0, 0, 0, 0, 1]) for _ in range(n)]
    return dict(keys=keys, powers=powers, off=off, mode=mode, form=form, who=who, vks=vks, flag=flag, thr=thr, codes=codes)


def _case_text(c):
    parts = [len(c["keys"]), *[k.hex() for k in c["keys"]], *c["powers"], len(c["off"]) - 1, *c["off"], c["mode"], c["form"]]
    parts += c["who"] if c["form"] else [v.hex() for v in c["vks"]]
    parts += [*c["flag"], *c["thr"], *c["codes"]]
    return " ".join(str(p) for p in parts)


def _model_line(g, c):
    if not g.check_powers(c["keys"], c["powers"]):
        return [0]
    kw = dict(key_idx=c["who"]) if c["form"] else dict(vks=c["vks"])
    pos, power, flag_out = g.resolve(c["keys"], c["powers"], c["flag"], **kw)
    if not g.check_args(c["off"], c["flag"], power, flag_out):
        return [1, 0]
    j = g.judge(c["keys"], c["powers"], c["off"], c["flag"], c["thr"], c["mode"], c["codes"], **kw)
    return [1, 1, *j["pos"], *j["power"], *j["flag"], *j["checked"], *j["planned"], j["n_checked"], *j["dv"],
            *j["item_verdicts"], *j["tally"], *j["commit_verdicts"], j["n_bad_commits"], j["code"]]


def test_valset_host_logic_sanitized(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    g = gen_valset()
    rnd = random.Random("valset host logic")
    cases = [_random_case(rnd, g) for _ in range(400)]
    want = [_model_line(g, c) for c in cases]
    # the random sets contain what they are meant to
    assert sum(1 for w in want if w == [0]) > 20 and sum(1 for w in want if w == [1, 0]) > 10
    full = [(c, g.judge(c["keys"], c["powers"], c["off"], c["flag"], c["thr"], c["mode"], c["codes"],
                        **(dict(key_idx=c["who"]) if c["form"] else dict(vks=c["vks"]))))
            for c, w in zip(cases, want) if len(w) > 2]
    assert sum(1 for _, j in full if any(j["dv"])) > 20 and sum(1 for _, j in full if g.NO_POS in j["pos"]) > 20
    assert sum(1 for c, _ in full if 0 in [b - a for a, b in zip(c["off"], c["off"][1:])]) > 20
    assert {j["code"] for _, j in full} == {0, 1, 3, 4}
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(_case_text(c) for c in cases) + "\n")
    exe = str(tmp_path / "valset")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "valset_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases)
    for c, w, line in zip(cases, want, lines):
        assert [int(x) for x in line.split()] == w, _case_text(c)
