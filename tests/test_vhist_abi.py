"""CPU: the validator-set history entries (include/edc.h, edc_vhist_*) exist in the header, the library
and the Python surface, between the validator-set section and the multi-GPU one; a NULL context is an
argument error on each entry; the header section states the versions, the join, the equality
contract and what is not built; the model of tests/golden/gen_vhist.py holds on histories worked
out by hand and agrees with vhist.json; and the host-side logic of csrc/vhist.h, in a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer, agrees with that model on a few hundred
random small histories, every refusal of edc_vhist_set among them. No compute calls (no GPU here)."""
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

ENTRIES = ["edc_vhist_set", "edc_vhist_versions", "edc_vhist_totals", "edc_vhist_resolve",
           "edc_vhist_quorum_verify_device", "edc_vhist_quorum_verify", "edc_debug_vhist_select"]
CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")


def gen_vhist():
    spec = importlib.util.spec_from_file_location("gen_vhist", os.path.join(GOLDEN, "gen_vhist.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    declared = sorted(set(re.findall(r"\b(edc_(?:debug_)?vhist_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(ENTRIES)
    for s in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(\s*(const\s+)?edc_ctx\s*\*\s*ctx\s*[,)]" % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
        # between the validator-set section and the multi-GPU one
        assert code.index("edc_debug_valset_select(") < code.index(s + "(") < code.index("edc_create_multi(")
    assert re.search(r"#define\s+EDC_VHIST_NOT_MEMBER\s+0xFFFFFFFFFFFFFFFFull\b", code)
    # the verify entries are the validator-set twins' with the commits' versions behind the offsets
    def args(name):
        a = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1)
        return [" ".join(x.split()) for x in a.split(",")]
    for twin in ("edc_valset_quorum_verify_device", "edc_valset_quorum_verify", "edc_valset_resolve", "edc_debug_valset_select"):
        a = args(twin)
        at = a.index("const uint32_t* commit_off") + 1
        assert args(twin.replace("valset", "vhist")) == a[:at] + ["const uint32_t* commit_ver"] + a[at:]


def test_header_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    sec = doc[doc.index("Validator-set history: every commit judged by the set of its own height"):
              doc.index("#define EDC_VHIST_NOT_MEMBER")]
    # the validator-set section before it stands as it was
    assert doc.index("forms of these entries. /") < doc.index("Validator-set history: every commit judged")
    ver = sec[sec.index("Versions."):sec.index("edc_vhist_set sets the history")]
    assert "Version 0 is base_power[p]" in ver and "with the updates [upd_off[v-1], upd_off[v]) applied" in ver
    assert "not a member from that version on, until a later update gives it a power" in ver
    assert "A power of 0 is a member without weight" in ver and "restates the current state is allowed" in ver
    st = sec[sec.index("edc_vhist_set sets the history"):sec.index("edc_vhist_versions nv + 1")]
    assert "independent of edc_valset_set_powers" in st and "never read the history" in st
    assert "edc_keycache_load and edc_keycache_clear drop it; edc_keycache_add keeps it" in st
    for why in ("differs from the registered list's length or there is no list", "a key occurs twice",
                "not monotone from 0", "update position is >= m", "twice inside one version's slice",
                "other than the sentinel is above 2^63 - 1", "sum to more than 2^63 - 1", "reaches 2^32"):
        assert why in st, why
    join = sec[sec.index("The join."):sec.index("edc_vhist_resolve edc_valset_resolve")]
    assert "if it is a member at version v, else 0xFFFFFFFF" in join and "else EDC_VOTE_ABSENT" in join
    assert "commit_ver[c] > nv is EDC_ERR_ARG" in join and "repeat and come in any order" in join
    eq = sec[sec.index("Equality contract."):sec.index("edc_debug_vhist_select")]
    assert "every output, check8 included, equals what edc_quorum_verify[_device] gives" in eq
    assert "With nv = 0 and no sentinel in the base every output" in eq and "EDC_DOUBLE_VOTE verdicts included" in eq
    assert "no stream synchronization is added" in sec and "(1 over 4 over 3)" in sec
    nb = sec[sec.index("Not built:"):]
    for form in ("templated", "cached", "asynchronous", "incremental-verifier", "multi-GPU"):
        assert form in nb


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    ver = (ctypes.c_uint32 * 1)(0)
    thr = (ctypes.c_uint64 * 1)(0)
    pw = (ctypes.c_uint64 * 1)(7)
    mem = (ctypes.c_uint32 * 1)(7)
    cnt, nb = ctypes.c_size_t(7), ctypes.c_int(7)
    ms = (ctypes.c_float * 2)(7, 7)
    assert lib.edc_vhist_set(None, 1, pw, 0, None, None, None) == -2
    assert lib.edc_vhist_versions(None) == 0
    assert lib.edc_vhist_totals(None, 0, 1, pw, mem) == -2
    assert lib.edc_vhist_resolve(None, 1, off, ver, None, None, b"\0", thr, 1, None, None, None, None, None,
                                 ctypes.byref(cnt), None) == -2
    assert lib.edc_vhist_quorum_verify_device(None, 1, off, ver, None, None, None, None, None, None, thr, 1, seed, None,
                                              None, None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_vhist_quorum_verify(None, 1, off, ver, None, None, None, None, None, None, b"\0", thr, 1, seed, None,
                                       None, None, ctypes.byref(nb), ctypes.byref(cnt), None) == -2
    assert lib.edc_debug_vhist_select(None, 1, off, ver, None, None, b"\0", thr, 1, 1, ms) == -2
    assert (cnt.value, nb.value, ms[0], ms[1], pw[0], mem[0]) == (7, 7, 7.0, 7.0, 7, 7)            # nothing written


def test_python_surface(edc):
    for name in ("vhist_set", "vhist_versions", "vhist_totals", "vhist_resolve", "quorum_verify_vhist",
                 "quorum_verify_vhist_device", "vhist_select_ms"):
        assert callable(getattr(edc.Engine, name))
    assert edc.VHIST_NOT_MEMBER == 2**64 - 1
    # what is refused before a GPU is touched
    v = edc.batch.Verifier()
    v.queue((bytes(32), bytes(64), b"m"))
    with pytest.raises(ValueError):
        edc.batch.verify_quorum([v], [[1]], [[1]], [0], versions=[0])
    with pytest.raises(ValueError):
        edc.batch.verify_quorum([v], None, [[1]], [0], versions=[0], cached=True)
    with pytest.raises(ValueError):
        edc.batch.verify_quorum([v], None, [[1]], [0], versions=[0, 1])
    assert edc.batch.verify_quorum([], None, [], [], versions=[]) == ([], [], [])


def test_model_on_small_cases():
    """The model against histories worked out by hand from the header's definitions."""
    g = gen_vhist()
    N, keys = g.NOT_MEMBER, g.KEYS
    # absent at the base, joins at version 2, leaves at 4, rejoins at 5
    c = g.HISTORIES["join_leave_rejoin"]
    h = g.from_updates(keys, c["base"], c["updates"])
    assert h["nv"] == 6
    assert [g.power_at(h, 2, v) for v in range(7)] == [N, N, 9, 9, N, 4, 4]
    assert [g.lookup(h, 2, v) for v in range(7)] == [N, N, 9, 9, N, 4, 4]
    assert h["total"] == [17, 17, 26, 27, 18, 22, 22] and h["members"] == [3, 3, 4, 4, 3, 4, 4]
    assert h["off"] == [0, 2, 3, 7, 8] and h["ver"] == [0, 3, 0, 0, 2, 4, 5, 0] and h["pow"] == [5, 6, 5, N, 9, N, 4, 7]
    # the join at versions 1, 2, 4 and 5 of four commits of the same two votes: position 2, then 0
    off, ver, flag = [0, 2, 4, 6, 8], [1, 2, 4, 5], [1, 2] * 4
    pos, power, fl = g.resolve(keys, h, off, ver, flag, key_idx=[2, 0] * 4)
    assert pos == [g.NO_POS, 0, 2, 0, g.NO_POS, 0, 2, 0]
    assert power == [0, 5, 9, 5, 0, 6, 4, 6] and fl == [0, 2, 1, 2, 0, 2, 1, 2]
    assert g.resolve(keys, h, off, ver, flag, vks=[keys[2], keys[0]] * 4) == (pos, power, fl)
    # a flag above 2 passes through whoever signed; a stranger is no member at any version
    assert g.resolve(keys, h, [0, 2], [0], [3, 1], vks=[keys[2], b"\x99" * 32]) == ([g.NO_POS] * 2, [0, 0], [3, 0])
    # an update at exactly v = 3, seen from v - 1, v and v + 1
    c = g.HISTORIES["update_at_v"]
    h = g.from_updates(keys, c["base"], c["updates"])
    assert [g.power_at(h, 1, v) for v in (2, 3, 4)] == [2, 20, 20] == [g.lookup(h, 1, v) for v in (2, 3, 4)]
    assert h["total"] == [10, 10, 10, 28, 28] and h["members"] == [4] * 5
    # a member with power 0: a member (its flag counts, it can double-vote), without weight
    c = g.HISTORIES["zero_power"]
    h = g.from_updates(keys, c["base"], c["updates"])
    assert h["total"] == [3, 0, 0] and h["members"] == [2, 2, 1]
    p = g.plan(keys, h, [0, 2, 4], [0, 2], [1, 2, 1, 2], [0, 0], g.FULL, key_idx=[0, 0, 0, 0])
    assert (p["pos"], p["power"], p["flag"]) == ([0, 0, g.NO_POS, g.NO_POS], [0] * 4, [1, 2, 0, 0])
    assert (p["checked"], p["dv"]) == ([1, 1, 0, 0], [1, 0])
    # restating the state changes no version, and is one more entry of the list
    c = g.HISTORIES["restated"]
    h = g.from_updates(keys, c["base"], c["updates"])
    assert h["states"][0] == h["states"][1] and h["total"] == [15, 15, 16] and h["off"] == [0, 2, 4, 6, 7]
    # the verdicts: a double vote only where the signer is a member at the commit's version
    h = g.from_updates(keys, [5, 5, N, 7], [[(2, 9)]])
    j = g.judge(keys, h, [0, 2, 4], [0, 1], [1, 1, 1, 1], [0, 0], g.FULL, [0, 0, 0, 0], key_idx=[2, 2, 2, 2])
    assert j["commit_verdicts"] == [g.SHORT, g.DOUBLE_VOTE] and j["code"] == g.DOUBLE_VOTE
    assert j["item_verdicts"] == [g.NOT_CHECKED, g.NOT_CHECKED, 0, 0] and j["dv"] == [0, 1]
    # the refusals of edc_vhist_set
    b = lambda *a: g.build(*a)
    assert b(None, 4, [1] * 4, [], [], []) == "list" and b(keys, 3, [1] * 3, [], [], []) == "length"
    assert b(keys, 4, [1] * 4, [1, 1], [], []) == "offsets" and b(keys, 4, [1] * 4, [0, 2, 1], [0, 1], [1, 1]) == "offsets"
    assert b(keys, 4, [1] * 4, [0, 2**32 - 4], [], []) == "count"
    assert b(keys[:3] + keys[:1], 4, [1] * 4, [], [], []) == "keys"
    assert b(keys, 4, [1] * 4, [0, 1], [4], [1]) == "position"
    assert b(keys, 4, [1, 2**63, 1, 1], [], [], []) == "power" and b(keys, 4, [1] * 4, [0, 1], [0], [2**64 - 2]) == "power"
    assert b(keys, 4, [2**62] * 2 + [N, N], [], [], []) == "sum"
    assert b(keys, 4, [2**62, 2**62 - 1, N, N], [0, 0, 1], [3], [1]) == "sum"
    assert b(keys, 4, [2**62, 2**62 - 1, N, 0], [0, 2], [3, 0], [2**62, N])["total"] == [2**63 - 1, 2**63 - 1]
    assert b(keys, 4, [1] * 4, [0, 2], [1, 1], [2, 3]) == "twice"
    assert b(keys, 4, [1] * 4, [0, 1, 2], [1, 1], [2, 3])["total"] == [4, 5, 6]


def test_fixture_is_what_the_generator_makes():
    g, fx = gen_vhist(), golden("vhist.json")
    assert fx["not_member"] == g.NOT_MEMBER and sorted(fx["histories"]) == sorted(g.HISTORIES)
    for name in g.HISTORIES:
        assert fx["histories"][name] == g.recorded(name), name
    assert fx["histories"]["join_leave_rejoin"]["members"] == [3, 3, 4, 4, 3, 4, 4]
    assert fx["histories"]["zero_power"]["total"] == [3, 0, 0]


WHY = {"list": "no registered key list", "length": "one base power per position", "offsets": "not monotone from 0",
       "count": "reach 2^32", "keys": "holds a key twice", "position": "a position outside the list",
       "power": "every power at most 2^63 - 1", "sum": "sum to at most 2^63 - 1", "twice": "twice in one version"}


def _random_history(rnd, g):
    """One small history: 1..6 positions, 0..8 versions of 0..3 updates each (joins, leaves, zeros, restated
    states), sometimes with exactly one of the defects edc_vhist_set refuses."""
    N = g.NOT_MEMBER
    m = rnd.randrange(1, 7)
    ids = rnd.sample(range(1000), m)
    nv = rnd.choice([0, 0, 1, 2, 3, 5, 8])
    pw = lambda: rnd.choice([N, 0, 1, 5, 9, rnd.randrange(100)])
    base = [pw() for _ in range(m)]
    off, pos, power = [0], [], []
    for _ in range(nv):
        for p in rnd.sample(range(m), rnd.randrange(0, min(m, 3) + 1)):
            pos.append(p)
            power.append(pw())
        off.append(len(pos))
    c = dict(ids=ids, base=base, off=off if nv else [], pos=pos, power=power)
    kind = rnd.choice(g.REFUSALS + (None,) * 9)
    if kind == "list":
        c["ids"] = []
    elif kind == "length":
        c["base"] = base + [1] if rnd.randrange(2) else base[:-1]
    elif kind == "offsets" and nv:
        if rnd.randrange(2):
            c["off"] = [1] + off[1:]
        else:
            c["off"] = off[:-1] + [off[-2] - 1] if off[-2] else [1] + off[1:]
    elif kind == "count":
        c.update(off=[0, 2**32 - m], pos=[], power=[])
    elif kind == "keys" and m > 1:
        c["ids"][rnd.randrange(1, m)] = ids[0]
    elif kind == "position" and pos:
        c["pos"][rnd.randrange(len(pos))] = rnd.choice([m, m + 1, 2**32 - 1])
    elif kind == "power":
        if pos and rnd.randrange(2):
            c["power"][rnd.randrange(len(pos))] = rnd.choice([2**63, 2**64 - 2])
        else:
            c["base"][rnd.randrange(m)] = rnd.choice([2**63, 2**64 - 2])
    elif kind == "sum" and m > 1:
        if pos:                                  # every power fits, one version's sum does not
            j = rnd.randrange(len(pos))
            c["base"][(pos[j] + 1) % m] = 2**62
            c["power"][j] = 2**62
            for k in range(len(pos)):            # and nothing takes either away again
                if k != j and pos[k] in (pos[j], (pos[j] + 1) % m):
                    c["power"][k] = 2**62
        else:
            c["base"][0] = c["base"][1] = 2**62
    elif kind == "twice":
        slices = [v for v in range(nv) if off[v + 1] - off[v] >= 2]
        if slices:
            v = rnd.choice(slices)
            c["pos"][off[v]] = pos[off[v] + 1]
    c["query"] = [(rnd.randrange(max(len(c["base"]), 1)), rnd.randrange(nv + 1)) for _ in range(4)]
    return c


def _case_text(c):
    q = [x for pv in c["query"] for x in pv]
    parts = [len(c["ids"]), *c["ids"], len(c["base"]), *c["base"], len(c["off"]), *c["off"], len(c["pos"]), *c["pos"],
             *c["power"], len(q), *q]
    return " ".join(str(p) for p in parts)


def _model(g, c):
    keys = [i.to_bytes(32, "little") for i in c["ids"]]
    return g.build(keys, len(c["base"]), c["base"], c["off"], c["pos"], c["power"])


def test_vhist_host_logic_sanitized(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    g = gen_vhist()
    rnd = random.Random("vhist host logic")
    cases = [_random_history(rnd, g) for _ in range(400)]
    want = [_model(g, c) for c in cases]
    # every refusal is hit, and most histories are accepted: with joins, leaves, zeros and long lists
    assert {w for w in want if isinstance(w, str)} == set(g.REFUSALS)
    good = [w for w in want if not isinstance(w, str)]
    assert len(good) > 200
    assert sum(1 for h in good if g.NOT_MEMBER in h["pow"][1:]) > 50 and sum(1 for h in good if h["nv"] >= 5) > 30
    assert sum(1 for h in good if len(set(h["members"])) > 1) > 50
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(_case_text(c) for c in cases) + "\n")
    exe = str(tmp_path / "vhist")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "vhist_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases)
    for c, w, line in zip(cases, want, lines):
        if isinstance(w, str):
            assert line.startswith("0 ") and WHY[w] in line, (w, line, c)
            continue
        answers = [g.power_at(w, p, v) for p, v in c["query"]]
        assert [g.lookup(w, p, v) for p, v in c["query"]] == answers
        exp = [1, *w["off"], *w["ver"], *w["pow"], *w["total"], *w["members"], *answers]
        assert [int(x) for x in line.split()] == exp, (c, line)
