"""No GPU: the trusting pair of a validator-set request (include/edc.h: trust_ver / trust_threshold of
edc_vq_request, edc_vq_trust_resolve, edc_debug_vq_trust_last): declared, exported, listed, the ctypes
mirrors laid out as the C compiler lays them out, and the plain-C++ reference of the union, the
per-side tally and the two-sided reduction (csrc/vhist.h) against a Python model."""
import ctypes
import os
import random
import re
import subprocess

from conftest import ROOT
from test_sanitizers import SAN

CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")
ENTRIES = ("edc_vq_trust_resolve", "edc_debug_vq_trust_last", "edc_debug_vq_trust_select")
NO_TRUST = 0xFFFFFFFF


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    assert re.search(r"int\s+edc_vq_trust_resolve\s*\(\s*edc_ctx\s*\*\s*ctx,\s*size_t\s+nc,\s*const\s+uint32_t\s*\*\s*commit_off,"
                     r"\s*const\s+uint32_t\s*\*\s*commit_ver,\s*const\s+uint32_t\s*\*\s*trust_ver,", code)
    assert re.search(r"int\s+edc_debug_vq_trust_last\s*\(\s*const\s+edc_ctx\s*\*\s*ctx,\s*uint64_t\s+out\[4\]\s*\)", code)
    assert re.search(r"#define\s+EDC_VQ_NO_TRUST\s+0xFFFFFFFFu", code)
    assert edc.NO_TRUST == NO_TRUST
    for s in ENTRIES:
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    # behind the request entry it extends
    assert code.index("edc_debug_vq_last(") < code.index("edc_vq_trust_resolve(")
    doc = " ".join(_header().replace("*", " ").split())
    for phrase in ("Both structures begin with `size`", "With the earlier sizeof the appended fields read as NULL",
                   "Return value: EDC_OK iff every verdict of both arrays is EDC_OK; else 1 over 4 over 3",
                   "A vote is verified iff either side checks it"):
        assert phrase in doc, phrase


def test_structure_mirrors_match_the_compiler(edc, tmp_path):
    """sizeof and every field offset of the ctypes mirrors against a C program compiled with the header;
    the trust fields are the last ones: two pointers on the request, three on the result"""
    mirrors = {"edc_vq_request": edc.EdcVqRequest, "edc_vq_result": edc.EdcVqResult}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "edc.h"', "int main(void) {"]
    for cname, py in mirrors.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    want = {}
    for cname, py in mirrors.items():
        want[cname] = str(ctypes.sizeof(py))
        for f, _ in py._fields_:
            want[f"{cname}.{f}"] = str(getattr(py, f).offset)
    assert got == want
    assert [f for f, _ in edc.EdcVqRequest._fields_][-3:] == ["var_bytes", "trust_ver", "trust_threshold"]
    assert [f for f, _ in edc.EdcVqResult._fields_][-4:] == ["check8", "trust_verdicts", "trust_tally", "n_bad_trust"]
    assert ctypes.sizeof(edc.EdcVqRequest) - edc.EdcVqRequest.trust_ver.offset == 16
    assert ctypes.sizeof(edc.EdcVqResult) - edc.EdcVqResult.trust_verdicts.offset == 24


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    assert lib.edc_debug_vq_trust_last(None, (ctypes.c_uint64 * 4)()) == -2
    assert lib.edc_vq_trust_resolve(None, 0, *([None] * 8), 1, *([None] * 14)) == -2
    assert lib.edc_debug_vq_trust_select(None, 0, *([None] * 8), 1, 1, None) == -2
    rq = edc.EdcVqRequest(size=ctypes.sizeof(edc.EdcVqRequest))
    rs = edc.EdcVqResult(size=ctypes.sizeof(edc.EdcVqResult))
    assert lib.edc_vq_verify(None, ctypes.byref(rq), ctypes.byref(rs)) == -2


def test_integration_guide_lists_the_names():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in ENTRIES[:2] + ("trust_ver", "trust_threshold", "trust_verdicts", "trust_tally", "n_bad_trust", "EDC_VQ_NO_TRUST",
                            "NO_TRUST", "vq_trust_resolve", "vq_trust_last", "trust_versions", "trust_thresholds"):
        assert s in doc, s


def test_batch_verify_quorum_refuses_half_a_pair(edc):
    """batch.verify_quorum: the trust arguments go together, with versions, one per verifier; all of it
    is refused before an engine is touched"""
    import pytest
    vq = edc.batch.verify_quorum
    with pytest.raises(ValueError, match="go together"):
        vq([], None, [], [], versions=[], trust_versions=[])
    with pytest.raises(ValueError, match="go together"):
        vq([], None, [], [], versions=[], trust_thresholds=[])
    with pytest.raises(ValueError, match="with versions"):
        vq([], None, [], [], trust_versions=[], trust_thresholds=[])
    with pytest.raises(ValueError, match="one trust version and trust threshold per verifier"):
        vq([], None, [], [], versions=[], trust_versions=[0], trust_thresholds=[0])
    with pytest.raises(ValueError, match="one trust version and trust threshold per verifier"):
        vq([], None, [], [], versions=[], trust_versions=[], trust_thresholds=[5])
    # no verifiers: the five values of a pair, the three of a request without one
    assert vq([], None, [], [], versions=[], trust_versions=[], trust_thresholds=[]) == ([], [], [], [], [])
    assert vq([], None, [], [], versions=[]) == ([], [], [])


# ---------------------------------------------------------------- the plain-C++ reference
def _select(off, power, flag, thr, light):
    checked = []
    for c in range(len(off) - 1):
        run = 0
        for i in range(off[c], off[c + 1]):
            chk = (flag[i] == 1 and run <= thr[c]) if light else flag[i] != 0
            if chk and flag[i] == 1:
                run += power[i]
            checked.append(int(chk))
    return checked


def _side(off, checked, power, flag, codes, thr, dv, tver=None):
    """one side's tally, verdicts, bad count and code from the union's item codes"""
    tally, verdicts = [], []
    for c in range(len(off) - 1):
        items = [i for i in range(off[c], off[c + 1]) if checked[i]]
        t = sum(power[i] for i in items if flag[i] == 1 and codes[i] == 0)
        v = 1 if any(codes[i] for i in items) else 3 if t <= thr[c] else 0
        if dv[c]:
            v = 4
        if tver is not None and tver[c] == NO_TRUST:
            t, v = 0, 0
        tally.append(t)
        verdicts.append(v)
    return tally, verdicts, sum(1 for v in verdicts if v), next((c for c in (1, 4, 3) if c in verdicts), 0)


def _random_case(rnd):
    nv = rnd.randrange(4)
    nc = rnd.randrange(1, 6)
    off = [0]
    for _ in range(nc):
        off.append(off[-1] + rnd.choice([0, 1, 2, 5, 9]))
    n = off[-1]
    tver = [rnd.choice([NO_TRUST, NO_TRUST, rnd.randrange(nv + 1), rnd.randrange(nv + 3)]) for _ in range(nc)]
    flag = [rnd.choice([0, 1, 1, 1, 2]) for _ in range(n)]
    pa = [rnd.choice([0, 1, 3, 10]) for _ in range(n)]
    pb = [rnd.choice([0, 2, 5, 10]) for _ in range(n)]
    fa = [f if rnd.random() < 0.8 else 0 for f in flag]
    fb = [f if rnd.random() < 0.6 else 0 for f in flag]
    for c in range(nc):                     # the join leaves nothing on side B of a commit without one
        if tver[c] == NO_TRUST:
            for i in range(off[c], off[c + 1]):
                pb[i], fb[i] = 0, 0
    ta = [rnd.choice([0, 4, 12, 30]) for _ in range(nc)]
    tb = [rnd.choice([0, 2, 6, 15]) for _ in range(nc)]
    codes = [1 if rnd.random() < 0.1 else 0 for _ in range(n)]
    dva = [int(rnd.random() < 0.15) for _ in range(nc)]
    dvb = [0 if tver[c] == NO_TRUST else int(rnd.random() < 0.15) for c in range(nc)]
    return dict(nv=nv, off=off, tver=tver, pa=pa, fa=fa, pb=pb, fb=fb, ta=ta, tb=tb, mode=rnd.randrange(2), codes=codes,
                dva=dva, dvb=dvb)


def _case_text(c):
    arr = lambda xs: "%d %s" % (len(xs), " ".join(str(x) for x in xs))
    return " ".join([str(c["nv"]), arr(c["off"]), arr(c["tver"]), arr(c["pa"]), arr(c["fa"]), arr(c["pb"]), arr(c["fb"]),
                     arr(c["ta"]), arr(c["tb"]), str(c["mode"]), arr(c["codes"]), arr(c["dva"]), arr(c["dvb"])])


def _model_line(c):
    off, n = c["off"], c["off"][-1]
    ca = _select(off, c["pa"], c["fa"], c["ta"], c["mode"] == 1)
    cb = _select(off, c["pb"], c["fb"], c["tb"], c["mode"] == 1)
    side = [a | (b << 1) for a, b in zip(ca, cb)]
    both = sum(1 for s in side if s == 3)
    counts = [sum(ca), sum(cb), both, sum(ca) + sum(cb) - both]
    assert counts[3] == sum(1 for s in side if s)
    A = _side(off, ca, c["pa"], c["fa"], c["codes"], c["ta"], c["dva"])
    B = _side(off, cb, c["pb"], c["fb"], c["codes"], c["tb"], c["dvb"], c["tver"])
    ok = int(all(v <= c["nv"] or v == NO_TRUST for v in c["tver"]))
    pair = next((x for x in (1, 4, 3) if x in (A[3], B[3])), 0)
    out = [ok] + side + counts
    for S in (A, B):
        out += S[0] + S[1] + [S[2], S[3]]
    return " ".join(str(x) for x in out + [pair])


def test_plain_cpp_reference_matches_the_model(tmp_path):
    rnd = random.Random("vq trust reference")
    cases = [_random_case(rnd) for _ in range(300)]
    want = [_model_line(c) for c in cases]
    # the cases reach every verdict on both sides, the sentinel, refused versions and all three kinds of vote
    assert {w.split()[-1] for w in want} == {"0", "1", "3", "4"}
    assert {w.split()[0] for w in want} == {"0", "1"}
    assert any(NO_TRUST in c["tver"] for c in cases)
    src = tmp_path / "cases.txt"
    src.write_text("\n".join(_case_text(c) for c in cases) + "\n")
    exe = str(tmp_path / "vq_trust")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "vq_trust_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(cases)
    for c, w, line in zip(cases, want, lines):
        assert " ".join(line.split()) == w, c
