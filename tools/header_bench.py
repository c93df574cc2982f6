"""Header hashes on the GPU against the host reference, in one run (include/edc.h, edc_header_*).

6,991 headers of 14 CometBFT-shaped leaves (tests/header_model.py; about 430 bytes a header, the
72-byte block id among them), bound to the history workload of the quorum benches: 150 keys, 6,991
versions, 4 power updates per version. Header i names the set root of version i as its
validators_hash, of version i + 1 as its next_validators_hash, and the hash of header i - 1 in its
block id: the links form a chain. expect is given and every rule holds.
The two sides are alternated inside one run and the medians of --reps timings are reported:
  bind      edc_header_bind, all four rules (wall time of the call: staging, the 6,991 set roots,
            the header roots, the compares, 33 bytes per header back)  |  csrc/hdrhash.h on one host
            thread (tools/header_host.cpp, built here with the host compiler at -O2; a portable
            byte-wise SHA-256 without SHA instructions; the set roots are handed to it, so its time
            is the headers' alone)
  hashes    edc_header_hashes  |  the roots alone on the host
  kernels   the root kernel and the bind kernel alone (edc_debug_header_ms, HIP events)
hashlib (tests/header_model.py) only checks the roots of both sides; it is not timed.

  python tools/header_bench.py [--keys 150] [--versions 6991] [--updates 4] [--reps 20] [--log PATH]
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
import header_model as hm  # noqa: E402


def host_library(tmp):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise SystemExit("no host compiler for the host reference")
    so = os.path.join(tmp, "header_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "ed25519-consensus_amd", "csrc"),
                           os.path.join(ROOT, "tools", "header_host.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.header_host_run.argtypes = [ctypes.c_size_t] + [vp] * 10 + [ctypes.POINTER(ctypes.c_double)]
    lib.header_host_run.restype = ctypes.c_size_t
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=150)
    ap.add_argument("--versions", type=int, default=6991)
    ap.add_argument("--updates", type=int, default=4, help="power updates per version")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "header_bench.log"))
    args = ap.parse_args()
    m, nver, per = args.keys, args.versions, args.updates
    nv = nver - 1
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    rnd = random.Random("header bench")
    keys, _ = eng.sign([rnd.randbytes(32) for _ in range(m)], [b""] * m)
    base = [rnd.randrange(1, 1 << 20) for _ in range(m)]
    updates = [[(p, rnd.randrange(1, 1 << 20)) for p in rnd.sample(range(m), per)] for _ in range(nv)]
    eng.keycache_load(keys)
    assert eng.vhist_set(base, updates) == nver
    set_roots = eng.vhist_hashes()

    nh = nver
    headers, last = [], rnd.randbytes(32)
    for i in range(nh):
        headers.append(hm.shaped(rnd, i + 1, last, set_roots[i], set_roots[min(i + 1, nv)]))
        last = hm.mth(headers[-1])
    want = [hm.mth(h) for h in headers]
    vals, nexts, link = list(range(nh)), [min(i + 1, nv) for i in range(nh)], [hm.NONE] + list(range(nh - 1))

    hs, keep = eng._header_set(headers)
    u32 = lambda xs: (ctypes.c_uint32 * len(xs))(*xs)
    a_vals, a_next, a_link = u32(vals), u32(nexts), u32(link)
    expect, sroots = b"".join(want), b"".join(set_roots)
    e_buf, s_buf = ctypes.create_string_buffer(expect, len(expect)), ctypes.create_string_buffer(sroots, len(sroots))
    addr = ctypes.addressof
    rules = pkg.EdcHeaderRules(ctypes.sizeof(pkg.EdcHeaderRules), 0, addr(e_buf), addr(a_vals), 7, 2, addr(a_next), 8, 2,
                               addr(a_link), 4, 2)
    g_out, g_bad, g_n = ctypes.create_string_buffer(32 * nh), ctypes.create_string_buffer(nh), ctypes.c_size_t(0)
    h_out, h_bad, h_sec = ctypes.create_string_buffer(32 * nh), ctypes.create_string_buffer(nh), (ctypes.c_double * 2)()

    with tempfile.TemporaryDirectory() as tmp:
        host = host_library(tmp)

        def gpu_bind():
            t = time.perf_counter()
            eng._check(eng.lib.edc_header_bind(eng.ctx, ctypes.byref(hs), ctypes.byref(rules), g_bad, g_out, ctypes.byref(g_n)))
            return (time.perf_counter() - t) * 1e3

        def gpu_hashes():
            t = time.perf_counter()
            eng._check(eng.lib.edc_header_hashes(eng.ctx, ctypes.byref(hs), g_out))
            return (time.perf_counter() - t) * 1e3

        def host_run():
            n = host.header_host_run(nh, hs.leaf_off, hs.byte_off, hs.bytes, addr(e_buf), addr(a_vals), addr(a_next), addr(a_link),
                                     addr(s_buf), h_out, h_bad, h_sec)
            assert n == 0
            return h_sec[0] * 1e3, h_sec[1] * 1e3

        first = gpu_bind()                                     # with the address kernel and the ranking
        host_run()
        assert g_out.raw == expect and h_out.raw == expect, "roots differ from the model"
        assert g_bad.raw == bytes(nh) == h_bad.raw and g_n.value == 0
        for _ in range(args.warmup):
            gpu_bind()
            gpu_hashes()
            host_run()
        gb, gh, hb, hh = [], [], [], []
        for _ in range(args.reps):                             # alternated
            gb.append(gpu_bind())
            gh.append(gpu_hashes())
            a, b = host_run()
            hh.append(a)
            hb.append(b)
        assert g_out.raw == expect and g_bad.raw == bytes(nh)

    kern = eng.header_ms(headers, args.reps)
    eng.close()
    med = statistics.median
    mm = lambda x: [round(min(x), 4), round(max(x), 4)]
    res = {
        "workload": {"headers": nh, "leaves": 14, "bytes": len(keep[2]), "keys": m, "versions": nver,
                     "updates_per_version": per, "reps": args.reps},
        "gpu_bind_call_ms": round(med(gb), 4), "gpu_bind_call_ms_min_max": mm(gb), "gpu_first_call_ms": round(first, 4),
        "gpu_hashes_call_ms": round(med(gh), 4), "gpu_hashes_call_ms_min_max": mm(gh),
        "host_bind_ms": round(med(hb), 4), "host_bind_ms_min_max": mm(hb),
        "host_hashes_ms": round(med(hh), 4), "host_hashes_ms_min_max": mm(hh),
        "host_over_gpu_bind": round(med(hb) / med(gb), 2), "host_over_gpu_hashes": round(med(hh) / med(gh), 2),
        "root_kernel_ms": round(kern["roots"], 4), "bind_kernel_ms": round(kern["bind"], 4),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
