"""No GPU: the validator-set request entry (include/edc.h, edc_vq_verify / edc_debug_vq_last): declared,
exported, listed, and the ctypes mirrors of its two structures laid out as the C compiler lays them out."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("edc_vq_verify", "edc_debug_vq_last")


def _header():
    return open(os.path.join(ROOT, "include", "edc.h")).read()


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = edc.load_library()
    assert re.search(r"int\s+edc_vq_verify\s*\(\s*edc_ctx\s*\*\s*ctx,\s*const\s+edc_vq_request\s*\*\s*rq,\s*edc_vq_result\s*\*\s*rs\s*\)",
                     code)
    assert re.search(r"int\s+edc_debug_vq_last\s*\(\s*const\s+edc_ctx\s*\*\s*ctx,\s*uint64_t\s+out\[8\]\s*\)", code)
    for s in ENTRIES:
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS
    # behind the entries it composes
    assert code.index("edc_debug_vhist_select(") < code.index("edc_vq_verify(")


def test_header_names_what_is_still_not_built():
    doc = " ".join(_header().replace("*", " ").split())
    assert "Not built: templated, cached" not in doc
    assert doc.count("Not built: asynchronous submit / wait, incremental-verifier and multi-GPU forms. The templated and "
                     "cached forms are built as requests (edc_vq_verify, below), not as further forms of these entries.") == 2
    for phrase in ("Both structures begin with `size`", "exactly one of: msg_off", "Return value: EDC_OK iff every commit is EDC_OK; else 1 over 4 over 3",
                   "Keys by position"):
        assert phrase in doc, phrase


def test_structure_mirrors_match_the_compiler(edc, tmp_path):
    """sizeof and every field offset of the ctypes mirrors against a C program compiled with the header"""
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
    # the header's fields, in order, are the mirror's
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for cname, py in mirrors.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert names == [f for f, _ in py._fields_]


def test_null_arguments_are_argument_errors(edc):
    lib = edc.load_library()
    rq = edc.EdcVqRequest(size=ctypes.sizeof(edc.EdcVqRequest))
    rs = edc.EdcVqResult(size=ctypes.sizeof(edc.EdcVqResult))
    assert lib.edc_vq_verify(None, ctypes.byref(rq), ctypes.byref(rs)) == -2
    assert lib.edc_debug_vq_last(None, (ctypes.c_uint64 * 8)()) == -2


def test_integration_guide_lists_the_entry():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in ENTRIES + ("EdcVqRequest", "EdcVqResult", "vq_verify", "vq_last"):
        assert s in doc, s
