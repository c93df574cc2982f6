"""CPU: the buffer / stream / event owners and growth helpers of csrc/devbuf.h under ASan + UBSan.

tests/native/devbuf_main.cpp includes only devbuf.h, with a malloc-backed allocator policy that counts
live allocations and can fail the k-th one. It is built as tests/test_sanitizers.py builds its program
(-fsanitize=address,undefined -fno-sanitize-recover=all) and runs as a child process; no sanitizer
runtime is preloaded into Python. The program checks: no reallocation while need <= cap; every capacity
policy at 0, 1, 1023, 1024, 1025, 4095, 4096, 4097; a failure of each allocation of a five-buffer group
(all empty, capacity 0, live count back down, next call works); moves; and that the allocator's own
live count is 0 at exit (leaks are counted there, not by LeakSanitizer)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_sanitizers import SAN

CSRC = os.path.join(ROOT, "ed25519-consensus_amd", "csrc")


def test_devbuf_owners_and_growth_sanitized(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "devbuf")
    subprocess.check_call(["g++", *SAN, "-std=c++17", "-Wall", "-Werror", "-Wno-self-move", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "devbuf_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-4000:])
    status, checks = p.stdout.split()
    assert status == "ok" and int(checks) > 500
