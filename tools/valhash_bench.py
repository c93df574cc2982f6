"""Validator-set hashes on the GPU against the host reference, in one run (include/edc.h, edc_valhash_*).

The history workload of the quorum benches: 150 keys, 6,991 versions, 4 power updates per version
(here the updates change the powers, so the order of the leaves moves from version to version).
The two sides are alternated inside one run and the medians of --reps timings are reported:
  roots     edc_valhash_vhist over all versions (wall time of the call: launch, kernel, 32 bytes per
            version back)  |  csrc/valhash.h on one host thread (tools/valhash_host.cpp, built here
            with the host compiler at -O2; the addresses hashed once, outside the timed part, as
            the library ranks them once per key list)
  kernels   the root kernel and the address kernel alone (edc_debug_valhash_ms, HIP events)
  match     edc_valhash_vhist_match for one commit per version, every expectation right, and as a
            fraction of the edc_vq_verify request it would precede (the README's 1.70 ms:
            device-resident, prehashed, light mode)
hashlib (tests/valhash_model.py) only checks the roots of both sides; it is not timed.

  python tools/valhash_bench.py [--keys 150] [--versions 6991] [--updates 4] [--reps 20]
"""
import argparse
import ctypes
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import valhash_model as vm  # noqa: E402

VQ_REQUEST_MS = 1.70        # README: edc_vq_verify, history, device-resident, prehashed, light mode


def host_library(tmp):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise SystemExit("no host compiler for the host reference")
    so = os.path.join(tmp, "valhash_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "ed25519-consensus_amd", "csrc"),
                           os.path.join(ROOT, "tools", "valhash_host.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)
    lib.valhash_host_roots.argtypes = [ctypes.c_size_t, ctypes.c_char_p, u64p, ctypes.c_size_t, u32p, u32p, u64p, ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_double)]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=150)
    ap.add_argument("--versions", type=int, default=6991)
    ap.add_argument("--updates", type=int, default=4, help="power updates per version")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    m, nver, per = args.keys, args.versions, args.updates
    nv = nver - 1
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    rnd = random.Random("valhash bench")
    keys, _ = eng.sign([rnd.randbytes(32) for _ in range(m)], [b""] * m)
    base = [rnd.randrange(1, 1 << 20) for _ in range(m)]
    updates = [[(p, rnd.randrange(1, 1 << 20)) for p in rnd.sample(range(m), per)] for _ in range(nv)]
    eng.keycache_load(keys)
    assert eng.vhist_set(base, updates) == nver

    off = [0]
    for u in updates:
        off.append(off[-1] + len(u))
    flat = [x for u in updates for x in u]
    arr = lambda t, x: (t * max(len(x), 1))(*x)
    h_args = (m, b"".join(keys), arr(ctypes.c_uint64, base), nv, arr(ctypes.c_uint32, off),
              arr(ctypes.c_uint32, [p for p, _ in flat]), arr(ctypes.c_uint64, [w for _, w in flat]))
    h_out, h_sec = ctypes.create_string_buffer(32 * nver), (ctypes.c_double * 2)()
    g_out = ctypes.create_string_buffer(32 * nver)

    with tempfile.TemporaryDirectory() as tmp:
        host = host_library(tmp)

        def gpu_roots():
            t = time.perf_counter()
            eng._check(eng.lib.edc_valhash_vhist(eng.ctx, 0, nver, g_out))
            return (time.perf_counter() - t) * 1e3

        def host_roots():
            assert host.valhash_host_roots(*h_args, h_out, h_sec) == 0
            return h_sec[1] * 1e3, h_sec[0] * 1e3

        first = gpu_roots()                                    # with the address kernel and the ranking
        want = b"".join(vm.history_roots(keys, base, updates))
        host_roots()
        assert g_out.raw == want and h_out.raw == want, "roots differ from the model"
        for _ in range(args.warmup):
            gpu_roots()
            host_roots()
        g_ms, h_ms, h_addr = [], [], []
        for _ in range(args.reps):                             # alternated
            g_ms.append(gpu_roots())
            a, b = host_roots()
            h_ms.append(a)
            h_addr.append(b)
        assert g_out.raw == want and h_out.raw == want

    kern = eng.valhash_ms(args.reps)
    ver = arr(ctypes.c_uint32, list(range(nver)))
    ok, bad = ctypes.create_string_buffer(nver), ctypes.c_size_t(0)

    def match():
        t = time.perf_counter()
        eng._check(eng.lib.edc_valhash_vhist_match(eng.ctx, nver, ver, want, ok, ctypes.byref(bad)))
        return (time.perf_counter() - t) * 1e3
    for _ in range(args.warmup):
        match()
    m_ms = [match() for _ in range(args.reps)]
    assert bad.value == 0 and ok.raw == b"\x01" * nver
    eng.close()

    med = statistics.median
    res = {
        "workload": {"keys": m, "versions": nver, "updates_per_version": per, "reps": args.reps},
        "gpu_roots_call_ms": round(med(g_ms), 4), "gpu_roots_call_ms_min_max": [round(min(g_ms), 4), round(max(g_ms), 4)],
        "gpu_first_call_ms": round(first, 4),
        "host_roots_ms": round(med(h_ms), 4), "host_roots_ms_min_max": [round(min(h_ms), 4), round(max(h_ms), 4)],
        "host_addresses_ms": round(med(h_addr), 4),
        "host_over_gpu": round(med(h_ms) / med(g_ms), 2),
        "root_kernel_ms": round(kern["roots"], 4), "address_kernel_ms": round(kern["addresses"], 4),
        "match_call_ms": round(med(m_ms), 4), "match_over_vq_request": round(med(m_ms) / VQ_REQUEST_MS, 3),
        "vq_request_ms_from_readme": VQ_REQUEST_MS,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
