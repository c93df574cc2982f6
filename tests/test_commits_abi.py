"""CPU: the commit-set entries (edc_commits_*, edc_tmpl_commits_*) exist in the C ABI and in Python, a
NULL context is an argument error on each, the header cites the reference for each, the host-side
checks and the reduction (csrc/commits.h) hold under AddressSanitizer + UndefinedBehaviorSanitizer
in a stand-alone program, batch.verify_many answers what needs no GPU and refuses bad arguments,
and the golden file agrees with its generator's rules. No compute calls (no GPU here)."""
import ctypes
import hashlib
import importlib.util
import inspect
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT, golden

ENTRIES = ["edc_commits_verify_device", "edc_commits_verify", "edc_tmpl_commits_verify", "edc_commits_submit",
           "edc_tmpl_commits_submit", "edc_commits_submit_device", "edc_commits_wait"]
NEW_SYMBOLS = ENTRIES + ["edc_debug_tmpl_commit_map"]


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def gen_commits():
    spec = importlib.util.spec_from_file_location("gen_commits", os.path.join(GOLDEN, "gen_commits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*edc_ctx\s*\*\s*ctx\s*," % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    # the argument lists the entries were specified with
    assert re.search(r"int\s+edc_commits_verify_device\s*\(\s*edc_ctx\s*\*\s*ctx,\s*size_t\s+nc,\s*const\s+uint32_t\s*\*\s*"
                     r"commit_off,\s*const\s+uint8_t\s*\*\s*d_vk,\s*const\s+uint8_t\s*\*\s*d_sig,\s*const\s+uint8_t\s*\*\s*"
                     r"d_msg,\s*const\s+uint64_t\s*\*\s*d_msg_off,\s*const\s+uint8_t\s*\*\s*d_k,\s*const\s+uint8_t\s+"
                     r"z_seed\[32\],\s*uint8_t\s*\*\s*commit_verdicts,\s*uint8_t\s*\*\s*item_verdicts,\s*int\s*\*\s*"
                     r"n_bad_commits\s*\)", code)
    assert re.search(r"int\s+edc_commits_wait\s*\(\s*edc_ctx\s*\*\s*ctx,\s*int64_t\s+ticket,\s*uint8_t\s*\*\s*commit_verdicts,"
                     r"\s*uint8_t\s*\*\s*item_verdicts,\s*int\s*\*\s*n_bad_commits\s*\)", code)
    for s in ("edc_commits_submit", "edc_tmpl_commits_submit", "edc_commits_submit_device"):
        assert re.search(r"int64_t\s+%s\s*\(" % s, code), s


def test_header_cites_the_reference_and_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    sec = doc[doc.index("Commit sets: many variable-size batches"):doc.index("int edc_commits_verify_device(")]
    assert "src/batch.rs:110-217" in sec and "tests/batch.rs:18-44" in sec
    # one paragraph per entry (the three asynchronous forms share one), each with its reference lines
    leads = ["edc_commits_verify_device Verifier::queue", "edc_commits_verify the host-buffer form",
             "edc_tmpl_commits_verify templated messages",
             "edc_commits_submit / edc_tmpl_commits_submit / edc_commits_submit_device the asynchronous forms",
             "edc_commits_wait waits for the ticket", "Every argument is checked"]
    pos = [sec.index(lead) for lead in leads]
    assert pos == sorted(pos)
    for lead, a, e in zip(leads, pos, pos[1:]):
        assert re.search(r"src/batch\.rs:(127-137|104-107)", sec[a:e]), lead
    # soundness of the fallback, and what nc = 1 is
    assert "z_seed MUST be fresh and secret for every call" in sec
    assert re.search(r"With nc = 1 this is the streamed batch-with-fallback", sec)


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    ts, _keep = edc.batch.Templates([b"h"], [b"t"]).struct()
    p = ctypes.byref(ts)
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    tpl = (ctypes.c_uint16 * 1)(0)
    cv, iv, nb = ctypes.create_string_buffer(1), ctypes.create_string_buffer(1), ctypes.c_int(7)
    assert lib.edc_commits_verify_device(None, 1, off, None, None, None, None, None, seed, cv, iv, ctypes.byref(nb)) == -2
    assert lib.edc_commits_verify(None, 1, off, None, None, None, None, None, None, seed, cv, iv, ctypes.byref(nb)) == -2
    assert lib.edc_tmpl_commits_verify(None, p, 1, off, tpl, None, None, None, None, None, seed, cv, iv,
                                       ctypes.byref(nb)) == -2
    assert lib.edc_commits_submit(None, 1, off, None, None, None, None, None, None, seed) == -2
    assert lib.edc_tmpl_commits_submit(None, p, 1, off, tpl, None, None, None, None, None, seed) == -2
    assert lib.edc_commits_submit_device(None, 1, off, None, None, None, None, None, seed) == -2
    assert lib.edc_commits_wait(None, 0, cv, iv, ctypes.byref(nb)) == -2
    assert lib.edc_debug_tmpl_commit_map(None, 1, off, tpl, None, 1, None) == -2
    assert nb.value == 7


def test_python_surface(edc):
    for name in ["commits_verify", "commits_submit", "commits_wait", "commits_verify_templated",
                 "commits_submit_templated", "commits_verify_device", "commits_submit_device"]:
        assert callable(getattr(edc.Engine, name, None)), name
    for f in (edc.Engine.commits_verify, edc.Engine.commits_submit, edc.Engine.commits_verify_templated,
              edc.Engine.commits_submit_templated):
        p = inspect.signature(f).parameters
        assert p["vks"].default is None and p["key_idx"].default is None
    p = inspect.signature(edc.batch.verify_many).parameters
    assert list(p) == ["verifiers", "z_seed", "engine"] and p["z_seed"].default is None and p["engine"].default is None


def test_verify_many_without_a_gpu(edc):
    vm = edc.batch.verify_many
    assert vm([]) == []
    assert vm([], z_seed=bytes(32)) == []
    # empty Verifiers verify (Verifier::verify of nothing is Ok): no engine is needed for that
    assert vm([edc.batch.Verifier(), edc.batch.Verifier()]) == [True, True]
    assert vm(iter([edc.batch.Verifier()]), z_seed=bytes(32)) == [True]
    for bad_seed in (bytes(31), bytes(33), "seed", 7):
        with pytest.raises(ValueError):
            vm([], z_seed=bad_seed)
    for not_verifiers in ([None], [edc.batch.Verifier(), (bytes(32), bytes(64), b"m")], ["v"]):
        with pytest.raises(TypeError):
            vm(not_verifiers)
    with pytest.raises(TypeError):
        vm(None)


def test_golden_commits_follow_the_generator(edc):
    """What the file states about its sets is what gen_commits.py's rules give (the oracle's part,
    the signatures and verdicts, is recorded in the file and checked on the GPU)."""
    gen = gen_commits()
    g = golden("commits.json")
    assert sorted(g["sets"]) == sorted(gen.SETS) and g["nkeys"] == gen.NKEYS == 150
    assert bytes.fromhex(g["z_seed"]) == gen.Z_SEED
    heads, tails = gen.templates()
    assert len(heads) == len(tails) == 4
    for name in gen.SETS:
        s, b = g["sets"][name], gen.build(name)
        assert s["sizes"] == gen.layout(name)["sizes"] and s["n"] == len(b["msgs"]) == b["commit_off"][-1] < 5000
        nc = len(s["sizes"])
        assert len(s["commit_verdicts"]) == nc == len(b["commit_tpl"]), name     # every commit has an oracle verdict
        assert set(s["commit_verdicts"]) <= {0, 1} and s["n_bad_commits"] == sum(s["commit_verdicts"])
        # a commit is bad iff one of its items is
        codes = [0] * s["n"]
        for i, c in s["item_codes"].items():
            codes[int(i)] = c
        for c, (a, e) in enumerate(zip(b["commit_off"], b["commit_off"][1:])):
            assert s["commit_verdicts"][c] == (1 if any(codes[a:e]) else 0), (name, c)
        # messages are the materialised templates with a 12-byte hole
        t = edc.batch.Templates(heads, tails)
        assert t.materialize(b["tpl"], b["holes"]) == b["msgs"] and {len(h) for h in b["holes"]} <= {12}
        assert len(hashlib.sha256(b"".join(b["msgs"])).hexdigest()) == 64
    assert g["sets"]["valid"]["sizes"] == [0, 1, 150, 7, 2049, 0] and g["sets"]["valid"]["n_bad_commits"] == 0
    for name, item in (("mixed_a", 2047), ("mixed_b", 2048)):
        s, b = g["sets"][name], gen.build(name)
        assert 4096 < s["n"] < 4400
        assert s["item_codes"] == {"346": 1, "645": 1, "700": 2, "800": 1, str(item): 1}
        off = b["commit_off"]
        c20 = off.index(2040)
        assert off[c20 + 1] == 2060 and s["commit_verdicts"][c20] == 1                 # the commit across item 2048
        assert s["commit_verdicts"][c20 - 1] == 0 and s["commit_verdicts"][c20 + 1] == 0   # its neighbours
        assert 346 in off and 646 in off                                                # first / last item of a commit
        c = b["corpus_commit"]
        assert off[c + 1] - off[c] == 196 and s["commit_verdicts"][c] == 0
        assert s["n_bad_commits"] == 5
    small, big = g["sets"]["tmap_small"], g["sets"]["tmap_big"]
    assert len(small["sizes"]) == 600 and set(small["sizes"]) == set(range(6))
    assert small["sizes"][0] == small["sizes"][-1] == 0
    assert big["sizes"] == [3000]
    assert small["n_bad_commits"] == big["n_bad_commits"] == 0


def test_host_checks_under_sanitizers(tmp_path):
    assert shutil.which("g++"), "a host C++ compiler is needed to build the stand-alone check"
    exe = str(tmp_path / "commits_main")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "ed25519-consensus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "commits_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and "Sanitizer" not in p.stderr, p.stderr[-2000:]
