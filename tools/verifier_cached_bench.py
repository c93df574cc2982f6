"""Latency of the cached incremental verifier (edc_vfy_set_cached) against the plain incremental
verifier and the one-call cached entry (edc_sigcache_batch_verify_device), alternated in one
process on the same data: configs[2] (150 validators, 120-byte messages) prehashed in HBM, a table
of 4n records, the batch queued in 16 pieces with edc_verifier_queue_device (d_k given), at 2^20
and 2^17 items, hit ratios 0, 0.5, 0.9 and 1.0 (hits spread over the queue by a multiplicative
hash of the index). Per repetition the table is cleared and the hits are planted again (untimed)
before each configuration that reads the table. Three host-clock times per verifier
configuration, each ending in a device that is idle or a call that synchronizes:
  verify_*_ms   verify() alone, started on an idle device (the votes arrived earlier)
  queue_*_ms    the 16 queue calls, until the device is idle
  cycle_*_ms    reset, the 16 queue calls and verify()
and onecall_ms for the one-call entry (its whole cycle is the call). insert_drain_ms is the wait
for the cached verifier's deferred insert after verify() returned. Medians of --reps; one JSON
line per (size, ratio).
  python tools/verifier_cached_bench.py [--reps 20] [--warmup 3] [--sizes 1048576,131072] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

RATIOS = (0.0, 0.5, 0.9, 1.0)
PIECES = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1048576,131072")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    lib, ctx = eng.lib, eng.ctx
    dev = torch.device("cuda:0")
    zseed = bytes([0x33]) * 32
    n_keys, msg_len = bench.CONFIGS["c3"][1], bench.CONFIGS["c3"][2]
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        vk, sig, msg, off = bench.make_workload(pkg, eng, torch, dev, n, n_keys, msg_len, 0)
        torch.cuda.synchronize()
        hk = (ctypes.c_uint8 * (32 * n))()
        hvk, hsig, hmsg = vk.cpu().numpy(), sig.cpu().numpy(), msg.cpu().numpy()
        hoff = off.cpu().numpy().astype("uint64")
        at = lambda arr: ctypes.cast(arr.ctypes.data, ctypes.c_char_p)       # noqa: E731
        eng._check(lib.edc_challenge(ctx, n, at(hvk), at(hsig), at(hmsg),
                                     ctypes.cast(hoff.ctypes.data, ctypes.POINTER(ctypes.c_uint64)), hk))
        k = torch.frombuffer(hk, dtype=torch.uint8).to(dev)
        vk2, sig2, k2 = vk.view(n, 32), sig.view(n, 64), k.view(n, 32)
        eng.sigcache_create(4 * n)
        bounds = [n * p // PIECES for p in range(PIECES + 1)]
        miss = ctypes.c_size_t(0)
        vc, vp = lib.edc_verifier_create(ctx, n), lib.edc_verifier_create(ctx, n)
        assert vc and vp
        eng._check(lib.edc_vfy_set_cached(vc, 1))

        def onecall(tv, ts, tk, m):
            rc = lib.edc_sigcache_batch_verify_device(ctx, m, tv.data_ptr(), ts.data_ptr(), None, None, tk.data_ptr(),
                                                      zseed, None, ctypes.byref(miss))
            assert rc == 0, (rc, lib.edc_last_error(ctx))
            return miss.value

        def cycle(v):
            """(verify, 16 queue calls until idle, whole cycle, wait for what verify left enqueued) in ms"""
            t0 = time.perf_counter()
            eng._check(lib.edc_verifier_reset(v))
            tq = time.perf_counter()
            for p in range(PIECES):
                p0, p1 = bounds[p], bounds[p + 1]
                if p1 > p0:
                    eng._check(lib.edc_verifier_queue_device(v, p1 - p0, vk.data_ptr() + 32 * p0, sig.data_ptr() + 64 * p0,
                                                             None, None, k.data_ptr() + 32 * p0))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rc = lib.edc_verifier_verify(v, zseed, None, None)
            t2 = time.perf_counter()
            assert rc == 0, (rc, lib.edc_last_error(ctx))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            return (t2 - t1) * 1e3, (t1 - tq) * 1e3, (t2 - t0) * 1e3, (t3 - t2) * 1e3

        for ratio in RATIOS:
            h = (torch.arange(n, dtype=torch.int64, device=dev) * 2654435761) % (1 << 32)
            is_hit = h < int(ratio * (1 << 32))
            hit_rows = is_hit.nonzero().flatten()
            hv, hs, hkk = (t[hit_rows].contiguous() for t in (vk2, sig2, k2))
            n_hit = int(hit_rows.numel())
            n_missing = n - n_hit
            torch.cuda.synchronize()

            def plant():
                eng.sigcache_clear()
                assert onecall(hv, hs, hkk, n_hit) == n_hit

            rc_, rp_, ro_ = [], [], []
            for rep in range(a.warmup + a.reps):
                plant()
                p = cycle(vp)                       # never touches the table
                c = cycle(vc)                       # its verify inserts the misses: plant again below
                assert lib.edc_verifier_size(vc) == n_missing, (lib.edc_verifier_size(vc), n_missing)
                plant()
                t0 = time.perf_counter()
                got = onecall(vk, sig, k, n)
                o = (time.perf_counter() - t0) * 1e3
                assert got == n_missing, (got, n_missing)
                if rep >= a.warmup:
                    rc_.append(c), rp_.append(p), ro_.append(o)
            st = eng.sigcache_stats()
            med = lambda rs, i: round(statistics.median(r[i] for r in rs), 4)     # noqa: E731
            line = {"n": n, "hit_ratio": ratio, "n_miss": n_missing, "pieces": PIECES, "reps": a.reps,
                    "verify_cached_ms": med(rc_, 0), "verify_cached_ms_min": round(min(r[0] for r in rc_), 4),
                    "verify_plain_ms": med(rp_, 0), "verify_plain_ms_min": round(min(r[0] for r in rp_), 4),
                    "onecall_ms": round(statistics.median(ro_), 4), "onecall_ms_min": round(min(ro_), 4),
                    "queue_cached_ms": med(rc_, 1), "queue_plain_ms": med(rp_, 1),
                    "cycle_cached_ms": med(rc_, 2), "cycle_plain_ms": med(rp_, 2),
                    "insert_drain_ms": med(rc_, 3), "dropped": st["dropped"]}
            lines.append(line)
            print(json.dumps(line), flush=True)
        lib.edc_verifier_destroy(vc)
        lib.edc_verifier_destroy(vp)
        eng.sigcache_create(0)
        del vk, sig, msg, off, k
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/verifier_cached_bench.py --reps %d --warmup %d --sizes %s\n" % (a.reps, a.warmup, a.sizes))
            for line in lines:
                f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
