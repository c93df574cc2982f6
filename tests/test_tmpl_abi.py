"""CPU: the templated-message entries (edc_tmpl_*, edc_vfy_queue_templated) exist in the C ABI and in
Python, a NULL context / verifier is an argument error on each, Templates.materialize builds the
bytes the device must build, the golden file agrees with the oracle, and the host-side checks
(csrc/tmpl.h) hold under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program.
No compute calls (no GPU here)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

from conftest import ROOT, golden

NEW_SYMBOLS = ["edc_tmpl_expand_device", "edc_tmpl_challenge", "edc_tmpl_batch_verify", "edc_tmpl_batch_verify_device",
               "edc_tmpl_batch_submit", "edc_vfy_queue_templated"]


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(\s*edc_(ctx|verifier)\s*\*\s*\w+\s*,\s*const\s+edc_templates\s*\*" % s, code), \
            f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    assert re.search(r"typedef\s+struct\s+edc_templates\s*\{[^}]*count[^}]*head_off[^}]*tail_off[^}]*\}\s*edc_templates", code)
    # no new name under the two pinned prefixes
    assert not [s for s in NEW_SYMBOLS if s.startswith(("edc_verifier_", "edc_sigcache_"))]


def test_header_cites_the_reference_for_each_entry():
    doc = " ".join(_header().replace("*", " ").split())
    for s in NEW_SYMBOLS:
        m = re.search(r"\b%s\b (.*?)(?= edc_tmpl_\w+ | edc_vfy_queue_templated |A NULL ctx)" % s, doc)
        assert m, s
        assert "src/batch.rs:82-94" in m.group(1), s
        assert re.search(r":127-(137|217)", m.group(1)), s


def test_null_handle_is_an_argument_error(edc):
    lib = edc.load_library()
    ts, _keep = edc.batch.Templates([b"h"], [b"t"]).struct()
    p = ctypes.byref(ts)
    seed, buf = bytes(32), ctypes.create_string_buffer(32)
    assert lib.edc_tmpl_expand_device(None, p, 0, None, None, None, 0, None, 0, None) == -2
    assert lib.edc_tmpl_challenge(None, p, 0, None, None, None, None, None, buf) == -2
    assert lib.edc_tmpl_batch_verify(None, p, 0, None, None, None, None, None, None, seed, buf) == -2
    assert lib.edc_tmpl_batch_verify_device(None, p, 0, None, None, None, None, None, 0, seed, 0, None, buf) == -2
    assert lib.edc_tmpl_batch_submit(None, p, 0, None, None, None, None, None, None, seed, 0, 0) == -2
    assert lib.edc_vfy_queue_templated(None, p, 0, None, None, None, None, None, None) == -2


def test_python_surface(edc):
    for name in ["tmpl_expand_device", "tmpl_challenge", "batch_verify_templated", "batch_verify_templated_device",
                 "batch_submit_templated"]:
        assert callable(getattr(edc.Engine, name, None)), name
    assert callable(getattr(edc.batch.StreamVerifier, "queue_templated", None))
    for f in (edc.Engine.batch_verify_templated, edc.Engine.batch_submit_templated,
              edc.batch.StreamVerifier.queue_templated):
        p = inspect.signature(f).parameters
        assert p["vks"].default is None and p["key_idx"].default is None
    st = edc.EdcTemplates
    assert issubclass(st, ctypes.Structure)
    assert [f[0] for f in st._fields_] == ["count", "head", "head_off", "tail", "tail_off"]
    assert ctypes.sizeof(st) == 40 and st.head.offset == 8 and st.tail_off.offset == 32


def test_materialize_and_struct(edc):
    t = edc.batch.Templates([b"AB", b"", b"xyz"], [b"!", b"tail", b""])
    assert t.count == 3
    assert t.materialize([0, 1, 2, 1, 0], [b"--", b"", b"q", b"mid", b""]) == \
        [b"AB--!", b"tail", b"xyzq", b"midtail", b"AB!"]
    assert t.materialize([], []) == []
    ts, keep = t.struct()
    assert ts.count == 3 and list(ts.head_off[0:4]) == [0, 2, 2, 5] and list(ts.tail_off[0:4]) == [0, 1, 5, 5]
    assert ctypes.string_at(ts.head, 5) == b"ABxyz" and ctypes.string_at(ts.tail, 5) == b"!tail"
    for bad in ([], [b""] * 65536):
        try:
            edc.batch.Templates(bad, bad)
            raise AssertionError("expected ValueError")
        except ValueError:
            pass
    try:
        t.materialize([0], [])
        raise AssertionError("expected ValueError")
    except ValueError:
        pass


def test_golden_templates_against_the_oracle(edc, oracle):
    g = golden("templates.json")
    z_seed = bytes.fromhex(g["z_seed"])
    names = [c["name"] for c in g["cases"]]
    assert names == ["votes", "votes_flipped", "lengths"]
    for c in g["cases"]:
        t = edc.batch.Templates([bytes.fromhex(h) for h in c["heads"]], [bytes.fromhex(x) for x in c["tails"]])
        msgs = t.materialize(c["tpl"], [bytes.fromhex(h) for h in c["holes"]])
        vks = [bytes.fromhex(c["keys"][j]) for j in c["key_idx"]]
        sigs = [bytes.fromhex(s) for s in c["sigs"]]
        assert len(msgs) == len(sigs) <= 300
        for vk, s, m, k in zip(vks, sigs, msgs, c["k"]):
            assert oracle.challenge(s[:32], vk, m).to_bytes(32, "little").hex() == k
        code, check8 = oracle.batch_verify_seeded(list(zip(vks, sigs, msgs)), z_seed)
        assert (code, check8.hex()) == (c["batch_code"], c["check8"])
        assert [oracle.verify(vk, s, m) for vk, s, m in zip(vks, sigs, msgs)] == c["single"]
    votes, flipped, lengths = g["cases"]
    assert votes["batch_code"] == 0 and set(votes["single"]) == {0} and len(votes["heads"]) <= 4
    assert all(len(bytes.fromhex(h)) == 12 for h in votes["holes"])
    assert flipped["batch_code"] == 1 and flipped["check8"] != votes["check8"]
    assert flipped["single"] == [1 if i == 10 else 0 for i in range(32)]
    assert [a != b for a, b in zip(votes["holes"], flipped["holes"])] == [i == 10 for i in range(32)]
    # every boundary length, each by several splits (0 has one: all three parts empty)
    t = [(len(lengths["heads"][j]) // 2, len(lengths["tails"][j]) // 2) for j in lengths["tpl"]]
    tot = [hl + len(h) // 2 + tl for (hl, tl), h in zip(t, lengths["holes"])]
    for L in [0, 1, 15, 16, 17, 47, 48, 111, 112, 175, 176, 300]:
        splits = {(hl, L - hl - tl, tl) for (hl, tl), x in zip(t, tot) if x == L}
        assert len(splits) >= (1 if L == 0 else 3), (L, splits)      # a 1-byte message has exactly 3
        # all hole, all head (empty hole and tail), all tail (empty head and hole)
        assert {(0, L, 0), (L, 0, 0), (0, 0, L)} <= splits, (L, splits)
    assert {15, 16, 17} <= {hl for hl, _ in t} and {15, 16, 17} <= {tl for _, tl in t}
    assert lengths["batch_code"] == 0 and set(lengths["single"]) == {0}


def test_host_checks_under_sanitizers(tmp_path):
    assert shutil.which("g++"), "a host C++ compiler is needed to build the stand-alone check"
    exe = str(tmp_path / "tmpl_main")
    subprocess.check_call(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "ed25519-consensus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "tmpl_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok" and "Sanitizer" not in p.stderr, p.stderr[-2000:]
