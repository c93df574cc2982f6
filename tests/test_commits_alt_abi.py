"""CPU: templated commit sets with per-item template variants and their device forms
(edc_tmpl_commits_*_alt, edc_tmpl_commits_*_device, edc_debug_tmpl_commit_map_alt) exist in the C
ABI with the argument lists they were specified with and in Python, a NULL context is an argument
error on each with the result pointers left alone, the header cites the reference for each, the
new host-side checks (csrc/commits.h) hold under AddressSanitizer + UndefinedBehaviorSanitizer in a
stand-alone program, and the golden file agrees with its generator's rules. No compute calls."""
import ctypes
import hashlib
import importlib.util
import inspect
import os
import re
import shutil
import subprocess

from conftest import GOLDEN, ROOT, golden

ENTRIES = ["edc_tmpl_commits_verify_alt", "edc_tmpl_commits_submit_alt", "edc_tmpl_commits_verify_device",
           "edc_tmpl_commits_submit_device", "edc_debug_tmpl_commit_map_alt"]

HEAD = r"edc_ctx\s*\*\s*ctx,\s*const\s+edc_templates\s*\*\s*ts,\s*size_t\s+nc,\s*const\s+uint32_t\s*\*\s*commit_off,\s*" \
       r"const\s+uint16_t\s*\*\s*commit_tpl,\s*uint32_t\s+alt_span,\s*"
HOST = HEAD + r"const\s+uint8_t\s*\*\s*item_alt,\s*const\s+uint8_t\s*\*\s*vk,\s*const\s+uint32_t\s*\*\s*key_idx,\s*" \
              r"const\s+uint8_t\s*\*\s*sig,\s*const\s+uint8_t\s*\*\s*var,\s*const\s+uint32_t\s*\*\s*var_off,\s*" \
              r"const\s+uint8_t\s+z_seed\[32\]"
DEVICE = HEAD + r"const\s+uint8_t\s*\*\s*d_item_alt,\s*const\s+uint8_t\s*\*\s*d_vk,\s*const\s+uint8_t\s*\*\s*d_sig,\s*" \
                r"const\s+uint8_t\s*\*\s*d_var,\s*const\s+uint32_t\s*\*\s*d_var_off,\s*size_t\s+var_bytes,\s*" \
                r"const\s+uint8_t\s+z_seed\[32\]"
RESULTS = r",\s*uint8_t\s*\*\s*commit_verdicts,\s*uint8_t\s*\*\s*item_verdicts,\s*int\s*\*\s*n_bad_commits\s*\)"
SIGNATURES = {
    "edc_tmpl_commits_verify_alt": r"int\s+edc_tmpl_commits_verify_alt\s*\(\s*" + HOST + RESULTS,
    "edc_tmpl_commits_submit_alt": r"int64_t\s+edc_tmpl_commits_submit_alt\s*\(\s*" + HOST + r"\s*\)",
    "edc_tmpl_commits_verify_device": r"int\s+edc_tmpl_commits_verify_device\s*\(\s*" + DEVICE + RESULTS,
    "edc_tmpl_commits_submit_device": r"int64_t\s+edc_tmpl_commits_submit_device\s*\(\s*" + DEVICE + r"\s*\)",
    "edc_debug_tmpl_commit_map_alt":
        r"int\s+edc_debug_tmpl_commit_map_alt\s*\(\s*edc_ctx\s*\*\s*ctx,\s*size_t\s+nc,\s*const\s+uint32_t\s*\*\s*commit_off,"
        r"\s*const\s+uint16_t\s*\*\s*commit_tpl,\s*uint32_t\s+alt_span,\s*const\s+uint8_t\s*\*\s*item_alt,\s*uint16_t\s*\*\s*"
        r"tpl_out,\s*int\s*\*\s*flagged,\s*int\s+reps,\s*float\s*\*\s*ms\s*\)",
}


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def gen_alt():
    spec = importlib.util.spec_from_file_location("gen_commits_alt", os.path.join(GOLDEN, "gen_commits_alt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    for s in ENTRIES:
        assert re.search(SIGNATURES[s], code), f"include/edc.h does not declare {s} with the specified arguments"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    # declared behind the existing commit-set entries, which stay where they were
    assert code.index("edc_debug_tmpl_commit_map(") < min(code.index(s + "(") for s in ENTRIES)


def test_header_cites_the_reference_and_states_the_contract():
    doc = " ".join(_header().replace("*", " ").split())
    sec = doc[doc.index("Templated commit sets with per-item template variants"):
              doc.index("int edc_tmpl_commits_verify_alt(")]
    leads = ["edc_tmpl_commits_verify_alt edc_tmpl_commits_verify with variants",
             "edc_tmpl_commits_submit_alt the asynchronous host form",
             "edc_tmpl_commits_verify_device the items in this GPU's memory",
             "edc_tmpl_commits_submit_device its asynchronous form",
             "edc_debug_tmpl_commit_map_alt test / measurement hook"]
    pos = [sec.index(lead) for lead in leads]
    assert pos == sorted(pos)
    for lead, a, e in zip(leads, pos, pos[1:]):               # the four verifying entries
        par = sec[a:e]
        assert "src/batch.rs:82-94" in par and ":127-137" in par and ":149-217" in par and ":104-107" in par, lead
    # the rules of the window, and what alt_span = 1 is
    assert "commit_tpl[c] + alt_span <= ts->count" in sec and "NULL = all zeros" in sec
    assert "With alt_span = 1 and item_alt = NULL every entry below is the one-template-per-commit call" in sec
    assert "bit-identical to edc_commits_verify on the materialised messages" in sec
    assert "never a verdict" in sec and "nothing launched" in sec


def test_null_context_is_an_argument_error(edc):
    lib = edc.load_library()
    ts, _keep = edc.batch.Templates([b"h"], [b"t"]).struct()
    p = ctypes.byref(ts)
    seed = bytes(32)
    off = (ctypes.c_uint32 * 2)(0, 0)
    tpl = (ctypes.c_uint16 * 1)(0)
    cv, iv, nb = ctypes.create_string_buffer(b"\x55", 1), ctypes.create_string_buffer(b"\x66", 1), ctypes.c_int(7)
    out, flagged = (ctypes.c_uint16 * 1)(0x7777), ctypes.c_int(9)
    res = (cv, iv, ctypes.byref(nb))
    assert lib.edc_tmpl_commits_verify_alt(None, p, 1, off, tpl, 1, None, None, None, None, None, None, seed, *res) == -2
    assert lib.edc_tmpl_commits_submit_alt(None, p, 1, off, tpl, 1, None, None, None, None, None, None, seed) == -2
    assert lib.edc_tmpl_commits_verify_device(None, p, 1, off, tpl, 1, None, None, None, None, None, 0, seed, *res) == -2
    assert lib.edc_tmpl_commits_submit_device(None, p, 1, off, tpl, 1, None, None, None, None, None, 0, seed) == -2
    assert lib.edc_debug_tmpl_commit_map_alt(None, 1, off, tpl, 1, None, out, ctypes.byref(flagged), 1, None) == -2
    assert (cv.raw, iv.raw, nb.value, out[0], flagged.value) == (b"\x55", b"\x66", 7, 0x7777, 9)


def test_python_surface(edc):
    for name in ["commits_verify_templated_alt", "commits_submit_templated_alt", "commits_verify_templated_device",
                 "commits_submit_templated_device"]:
        assert callable(getattr(edc.Engine, name, None)), name
    for f in (edc.Engine.commits_verify_templated_alt, edc.Engine.commits_submit_templated_alt):
        p = inspect.signature(f).parameters
        assert list(p)[:6] == ["self", "templates", "commit_off", "commit_tpl", "alt_span", "item_alt"]
        assert p["vks"].default is None and p["key_idx"].default is None
    for f in (edc.Engine.commits_verify_templated_device, edc.Engine.commits_submit_templated_device):
        assert list(inspect.signature(f).parameters) == ["self", "templates", "commit_off", "commit_tpl", "alt_span",
                                                         "d_item_alt", "d_vk", "d_sig", "d_var", "d_var_off", "var_bytes",
                                                         "z_seed"]
    # the existing methods keep their signatures
    p = inspect.signature(edc.Engine.commits_verify_templated).parameters
    assert list(p) == ["self", "templates", "commit_off", "commit_tpl", "sigs", "holes", "z_seed", "vks", "key_idx", "var_off"]
    assert list(inspect.signature(edc.batch.verify_many).parameters) == ["verifiers", "z_seed", "engine"]


def test_golden_commits_alt_follow_the_generator(edc):
    """What the file states about its sets is what gen_commits_alt.py's rules give (the oracle's
    part, the signatures and codes, is recorded in the file and checked on the GPU)."""
    gen = gen_alt()
    g = golden("commits_alt.json")
    assert os.path.getsize(os.path.join(GOLDEN, "commits_alt.json")) < 64 * 1024
    assert sorted(g["sets"]) == sorted(gen.SETS) and g["nkeys"] == gen.NKEYS == 150 and g["alt_span"] == gen.ALT_SPAN == 4
    assert bytes.fromhex(g["z_seed"]) == gen.Z_SEED
    # the set of 8: two heights x {block, nil} x {short, long prefix}; one empty head, one empty tail;
    # hole lengths 0, 11, 12, 13; a non-empty head starts with the length of what follows it
    heads, tails = gen.templates()
    assert len(heads) == len(tails) == 8 == 2 * gen.ALT_SPAN
    assert [len(h) for h in heads].count(0) == 1 and [len(t) for t in tails].count(0) == 1
    assert sorted(gen.HOLE_OF_ALT) == [0, 11, 12, 13]
    for t, (h, tl) in enumerate(zip(heads, tails)):
        if h:
            assert h[0] == len(h) + gen.HOLE_OF_ALT[t % 4] + len(tl) - 1
    assert len({(h, tl) for h, tl in zip(heads, tails)}) == 8
    T = edc.batch.Templates(heads, tails)
    for name in gen.SETS:
        s, b = g["sets"][name], gen.build(name)
        nc, n = len(b["sizes"]), s["n"]
        assert s["sizes"] == b["sizes"] and n == len(b["tpl"]) == b["commit_off"][-1] == len(b["alt"]) < 5000
        assert set(b["commit_tpl"]) <= {0, 4} and len(b["commit_tpl"]) == nc
        assert all(a < gen.ALT_SPAN for a in b["alt"])
        for c, (a, e) in enumerate(zip(b["commit_off"], b["commit_off"][1:])):
            assert b["tpl"][a:e] == [b["commit_tpl"][c] + x for x in b["alt"][a:e]]
        assert {len(h) for h in b["holes"]} <= set(gen.HOLE_OF_ALT)
        assert [len(h) for h in b["holes"]] == [gen.HOLE_OF_ALT[a] for a in b["alt"]]
        assert T.materialize(b["tpl"], b["holes"]) == b["msgs"]
        d = gen.digests(b)
        assert (s["alt_sha256"], s["tpl_sha256"]) == (d["alt_sha256"], d["tpl_sha256"])
        if name in gen.SIGNED:
            assert s["msg_sha256"] == hashlib.sha256(b"".join(b["msgs"])).hexdigest()
            assert len(s["commit_verdicts"]) == nc and s["n_bad_commits"] == sum(s["commit_verdicts"])
            codes = [0] * n
            for i, c in s["item_codes"].items():
                codes[int(i)] = c
            for c, (a, e) in enumerate(zip(b["commit_off"], b["commit_off"][1:])):
                assert s["commit_verdicts"][c] == (1 if any(codes[a:e]) else 0), (name, c)
        else:
            assert "commit_verdicts" not in s and "sig_sha256" not in s                # map-only
    small = g["sets"]["small"]
    assert len(small["sizes"]) == 600 and set(small["sizes"]) == set(range(6))
    assert small["sizes"][:3] == [0, 0, 0] and small["sizes"][-2:] == [0, 0] and small["sizes"][100:104] == [0] * 4
    assert sorted(int(k[4:]) for k in g["sets"] if k.startswith("edge")) == [1, 7, 8, 9, 2047, 2048, 2049, 4100]
    for k, s in g["sets"].items():
        if k.startswith("edge"):
            assert s["n"] == int(k[4:])
            if s["n"] >= 2047:                                                      # every variant occurs
                assert set(gen.build(k, messages=False)["alt"]) == {0, 1, 2, 3}
    big = gen.build("edge4100", messages=False)["commit_off"]
    assert 2048 in big and 4096 in big and 2045 in big                                # workgroup boundaries, and inside a lane
    assert g["sets"]["edge4100"]["item_codes"] == {} and g["sets"]["edge4100"]["n_bad_commits"] == 0
    mixed, mb = g["sets"]["mixed"], gen.build("mixed")
    first, last, key, sl = gen.bad_items("mixed", mb)
    assert len(mixed["sizes"]) == 40 and mixed["sizes"][0] == mixed["sizes"][-1] == 0
    assert mixed["item_codes"] == {str(first): 1, str(last): 1, str(key): 2, str(sl): 1} and mixed["n_bad_commits"] == 4
    assert first in mb["commit_off"] and last + 1 in mb["commit_off"]
    assert len(set(mb["alt"])) == 4


def test_host_checks_under_sanitizers(tmp_path):
    assert shutil.which("g++"), "a host C++ compiler is needed to build the stand-alone check"
    exe = str(tmp_path / "commits_alt_main")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "ed25519-consensus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "commits_alt_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and "Sanitizer" not in p.stderr, p.stderr[-2000:]
