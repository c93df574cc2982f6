"""CPU: the plan report hooks (edc_debug_last_plan, edc_vfy_last_plan; include/edc.h) exist in the
header, the library and the Python surface, refuse NULL without writing, and the ctypes mirror has
the layout of struct edc_plan_info. No compute calls (no GPU here); tests/test_gpu_subbins.py reads
plans through them on the GPU."""
import ctypes
import os
import re

from conftest import ROOT

NEW_SYMBOLS = ["edc_debug_last_plan", "edc_vfy_last_plan"]


def test_header_library_and_abi_list(edc):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "edc.h")).read(), flags=re.S)
    lib = edc.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), f"include/edc.h does not declare {s}"
        assert hasattr(lib, s), f"libedc.so does not export {s}"
        assert s in edc.ABI_SYMBOLS


def test_plan_report_without_gpu(edc):
    """edc_debug_last_plan / edc_vfy_last_plan: NULL is an argument error and writes nothing; the
    ctypes mirror has the layout of struct edc_plan_info (ten 32-bit words, the double target, then
    bits[32], nsub[32] and nslice[32])."""
    lib = edc.load_library()
    info = edc.EdcPlanInfo()
    info.nwin = 7
    assert lib.edc_debug_last_plan(None, ctypes.byref(info)) == -2
    assert lib.edc_vfy_last_plan(None, ctypes.byref(info)) == -2
    assert info.nwin == 7
    assert ctypes.sizeof(edc.EdcPlanInfo) == 40 + 8 + 32 + 32 + 64
    assert (edc.EdcPlanInfo.target.offset, edc.EdcPlanInfo.bits.offset, edc.EdcPlanInfo.nslice.offset) == (40, 48, 112)
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "edc.h")).read())
    assert ("uint32_t nwin, nwin_short, nranges, sum_ranges, bins_per_range; uint32_t per_sig, split, few, fold; "
            "uint32_t reserved; double target; uint8_t bits[32], nsub[32]; uint16_t nslice[32]; } edc_plan_info;") in src
    assert callable(edc.Engine.last_plan) and isinstance(edc.batch.StreamVerifier.last_plan, property)
    info.nwin, info.few, info.target = 2, 1, 256.0
    info.nsub[0], info.nsub[1], info.nsub[2] = 16, 1, 9
    d = info.as_dict()
    assert d["nsub"] == [16, 1] and d["few"] is True and d["split"] is False and d["target"] == 256.0
