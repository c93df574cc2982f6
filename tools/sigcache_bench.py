"""Cost and gain of the verified-signature cache (edc_sigcache_batch_verify_device) against the plain
prehashed batch entry (edc_batch_verify_prehashed_device) in the same process on the same data:
configs[2] (150 validators, 120-byte messages) prehashed in HBM, at 2^20 and 2^17 items, with
hit ratios 0, 0.5, 0.9 and 1.0 (hits spread over the queue by a multiplicative hash of the index).
Per repetition the table is cleared and the hits are planted again (untimed), then the cached call
and the plain call on the whole batch are timed one after the other (host clock around the
synchronous calls); medians of --reps. plain_miss_ms is the plain entry on the miss list alone:
what a cache with free lookups would cost. One JSON line per (size, ratio).
  python tools/sigcache_bench.py [--reps 20] [--warmup 3] [--sizes 1048576,131072] [--out FILE]"""
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
        miss = ctypes.c_size_t(0)

        def cached(tv, ts, tk, m):
            rc = lib.edc_sigcache_batch_verify_device(ctx, m, tv.data_ptr(), ts.data_ptr(), None, None, tk.data_ptr(),
                                                      zseed, None, ctypes.byref(miss))
            assert rc == 0, (rc, lib.edc_last_error(ctx))
            return miss.value

        def plain(tv, ts, tk, m):
            rc = lib.edc_batch_verify_prehashed_device(ctx, m, tv.data_ptr(), ts.data_ptr(), tk.data_ptr(), zseed, 0,
                                                       None, None)
            assert rc == 0, (rc, lib.edc_last_error(ctx))

        def timed(fn, *args):
            t0 = time.perf_counter()
            r = fn(*args)
            return (time.perf_counter() - t0) * 1e3, r

        for ratio in RATIOS:
            h = (torch.arange(n, dtype=torch.int64, device=dev) * 2654435761) % (1 << 32)
            is_hit = h < int(ratio * (1 << 32))
            hit_rows, miss_rows = is_hit.nonzero().flatten(), (~is_hit).nonzero().flatten()
            hv, hs, hkk = (t[hit_rows].contiguous() for t in (vk2, sig2, k2))
            mv, ms, mk = (t[miss_rows].contiguous() for t in (vk2, sig2, k2))
            n_hit, n_missing = int(hit_rows.numel()), int(miss_rows.numel())
            torch.cuda.synchronize()
            tc, tp, tm = [], [], []
            for rep in range(a.warmup + a.reps):
                eng.sigcache_clear()
                assert cached(hv, hs, hkk, n_hit) == n_hit          # plant the hits (untimed)
                c, got = timed(cached, vk, sig, k, n)
                assert got == n_missing, (got, n_missing)
                p, _ = timed(plain, vk, sig, k, n)
                m, _ = timed(plain, mv, ms, mk, n_missing)
                if rep >= a.warmup:
                    tc.append(c), tp.append(p), tm.append(m)
            st = eng.sigcache_stats()
            line = {"n": n, "hit_ratio": ratio, "n_miss": n_missing, "reps": a.reps,
                    "cached_ms": round(statistics.median(tc), 4), "cached_ms_min": round(min(tc), 4),
                    "plain_ms": round(statistics.median(tp), 4), "plain_ms_min": round(min(tp), 4),
                    "plain_miss_ms": round(statistics.median(tm), 4),
                    "cached_minus_plain_ms": round(statistics.median(tc) - statistics.median(tp), 4),
                    "cached_minus_plain_miss_ms": round(statistics.median(tc) - statistics.median(tm), 4),
                    "dropped": st["dropped"]}
            lines.append(line)
            print(json.dumps(line), flush=True)
        eng.sigcache_create(0)
        del vk, sig, msg, off, k
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/sigcache_bench.py --reps %d --warmup %d --sizes %s\n" % (a.reps, a.warmup, a.sizes))
            for line in lines:
                f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
