"""CPU: the test-only device library of tests/native/devcheck.hip (built by csrc/Makefile with
libedc.so) exists after build(), holds a gfx950 code object and exports dc_run and no other
function. No compute calls (no GPU here); tests/test_gpu_device_math.py drives it on the GPU."""
import ctypes
import os
import shutil
import subprocess

from conftest import ROOT

SO = os.path.join(ROOT, "tests", "native", "libedc_devcheck.so")


def test_devcheck_library_is_built_for_gfx950():
    assert os.path.exists(SO), "tests/native/libedc_devcheck.so is missing (run __graft_entry__.build())"
    assert b"gfx950" in open(SO, "rb").read()


def test_devcheck_exports_dc_run_only(edc):
    edc.load_library()                     # the HIP runtime libedc.so uses serves this library too
    lib = ctypes.CDLL(SO)
    assert hasattr(lib, "dc_run")
    assert not hasattr(lib, "edc_create")  # nothing of the product ABI
    if shutil.which("nm"):                 # binutils present: dc_run is the only exported function
        syms = subprocess.run(["nm", "-D", "--defined-only", SO], capture_output=True, text=True, check=True)
        funcs = [ln.split()[-1] for ln in syms.stdout.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TtWw"]
        assert funcs == ["dc_run"], funcs
    # argument errors come back without touching a device
    lib.dc_run.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                           ctypes.c_uint32]
    assert lib.dc_run(-1, 0, None, 0, None, 0) < 0
    assert lib.dc_run(0, 0, None, 18, None, 9) == 0
    assert lib.dc_run(0, 0, None, 17, None, 9) < 0
