"""Latency of the incremental verifier's last step: verify() alone, after the batch was queued in
16 pieces (edc_verifier_queue* then edc_verifier_verify), against the one-call entries a caller
had before, in the same process on the same data (reference src/batch.rs:127-137 queue, :149-217
verify). Per size (150 validators, 120-byte messages):
  one-call     edc_batch_verify_device (device inputs), edc_batch_verify and
               edc_batch_verify_prehashed (host inputs)
  verifier     queued from host memory with messages, from host memory prehashed, from device
               memory; the device is idle when verify() starts (the votes arrived earlier)
Warm-up calls first, then the median of --reps repetitions; queue_verify_ms is the whole cycle
(reset, 16 queue calls, verify) and gives the total throughput beside the latency.
  python tools/verifier_bench.py [--reps 20] [--warmup 3] [--sizes 150,131072,1048576] [--out FILE]
--keycache: the leg for a registered validator set instead. Per size: the queue cycle (host memory,
prehashed) with no key cache, then with the 150 validators loaded (edc_keycache_load), where queue
time also leaves the [2^128] rows and verify() runs with split coefficients, then queued by key
index (edc_vfy_queue_indexed); edc_batch_verify_device with the cache loaded beside them. Per cycle:
verify() alone, the mean host time of a queue call and the 16 queue calls until the device is idle.
--lib PATH loads another build of libedc.so (A/B against an older build, which lacks the indexed
entry and runs verify() unsplit).
--eager: the leg for the eager mode (edc_vfy_begin_eager) instead: per size the plain queue cycle,
then the eager one at every fold granularity of --fold (a sweep: --fold 2048,8192,32768,131072),
each with verify() alone, the 16 queue calls in total and the whole cycle. An older build given
with --lib reports the plain cycle only."""
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

PIECES = 16


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4), round(min(ts), 4)


def keycache_leg(a, pkg, eng, torch, dev):
    lib, ctx = eng.lib, eng.ctx
    zseed = bytes([0x33]) * 32
    u8p, u64p, u32p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    indexed = hasattr(lib, "edc_vfy_queue_indexed")
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        vk, sig, msg, off = bench.make_workload(pkg, eng, torch, dev, n, 150, 120, 0)
        torch.cuda.synchronize()
        hvk, hsig, hmsg = vk.cpu().numpy(), sig.cpu().numpy(), msg.cpu().numpy()
        hoff = off.cpu().numpy().astype("uint64")
        hk = (ctypes.c_uint8 * (32 * n))()
        at = lambda arr, byte: ctypes.cast(arr.ctypes.data + byte, u8p)       # noqa: E731
        eng._check(lib.edc_challenge(ctx, n, at(hvk, 0), at(hsig, 0), at(hmsg, 0),
                                     ctypes.cast(hoff.ctypes.data, u64p), hk))
        hk_addr = ctypes.addressof(hk)
        nkeys = min(n, 150)                                  # item i is signed by validator i mod 150
        validators = [hvk.reshape(-1)[32 * j:32 * j + 32].tobytes() for j in range(nkeys)]
        hidx = (ctypes.c_uint32 * n)(*[i % 150 for i in range(n)])
        hidx_addr = ctypes.addressof(hidx)
        bounds = [n * p // PIECES for p in range(PIECES + 1)]
        v = lib.edc_verifier_create(ctx, n)
        assert v

        def q_prehashed(p0, p1):
            return lib.edc_verifier_queue_prehashed(v, p1 - p0, at(hvk, 32 * p0), at(hsig, 64 * p0),
                                                    ctypes.cast(hk_addr + 32 * p0, u8p))

        def q_indexed(p0, p1):
            return lib.edc_vfy_queue_indexed(v, p1 - p0, ctypes.cast(hidx_addr + 4 * p0, u32p), at(hsig, 64 * p0), None,
                                             None, ctypes.cast(hk_addr + 32 * p0, u8p))

        def cycle(qfn):
            """reset, queue in 16 pieces, idle device, verify: (verify, mean queue call, queue until idle) ms"""
            eng._check(lib.edc_verifier_reset(v))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = 0
            for p in range(PIECES):
                if bounds[p + 1] > bounds[p]:
                    eng._check(qfn(bounds[p], bounds[p + 1]))
                    calls += 1
            tq = time.perf_counter()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rc = lib.edc_verifier_verify(v, zseed, None, None)
            t2 = time.perf_counter()
            assert rc == 0, rc
            return (t2 - t1) * 1e3, (tq - t0) * 1e3 / calls, (t1 - t0) * 1e3

        def measure(out, label, qfn):
            for _ in range(a.warmup):
                cycle(qfn)
            rs = [cycle(qfn) for _ in range(a.reps)]
            out[f"verify_after_queue_{label}_ms"] = round(statistics.median(r[0] for r in rs), 4)
            out[f"verify_after_queue_{label}_ms_min"] = round(min(r[0] for r in rs), 4)
            out[f"queue_call_{label}_ms"] = round(statistics.median(r[1] for r in rs), 4)
            out[f"queue_until_idle_{label}_ms"] = round(statistics.median(r[2] for r in rs), 4)

        def one_device():
            assert lib.edc_batch_verify_device(ctx, n, vk.data_ptr(), sig.data_ptr(), msg.data_ptr(), off.data_ptr(),
                                               zseed, 0, None, None) == 0

        out = {"n": n, "keycache": True, "lib": os.path.basename(a.lib) if a.lib else "libedc.so", "validators": 150,
               "pieces": PIECES, "reps": a.reps}
        eng.keycache_clear()
        measure(out, "prehashed_nocache", q_prehashed)       # no [2^128] rows at queue time
        eng.keycache_load(validators)
        out["batch_verify_device_keycache_ms"], out["batch_verify_device_keycache_ms_min"] = median_ms(
            one_device, a.warmup, a.reps)
        measure(out, "prehashed_keycache", q_prehashed)
        if indexed:
            out["last_split"] = lib.edc_vfy_last_split(v)
            measure(out, "indexed_keycache", q_indexed)
        lib.edc_verifier_destroy(v)
        eng.keycache_clear()
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del vk, sig, msg, off
    return lines


def eager_leg(a, pkg, eng, torch, dev):
    """Per size: the queue cycle (host memory, prehashed, 16 pieces) on a plain verifier, then in
    eager mode (edc_vfy_begin_eager: the R terms are folded at queue time) at each fold granularity
    of --fold (0 = the library default). Per cycle: verify() alone on an idle device, the 16 queue
    calls until the device is idle, and the whole cycle (reset, begin, queue, verify)."""
    lib, ctx = eng.lib, eng.ctx
    zseed = bytes([0x33]) * 32
    u8p, u64p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
    has_eager = hasattr(lib, "edc_vfy_begin_eager")
    folds = [int(x) for x in a.fold.split(",")]
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        vk, sig, msg, off = bench.make_workload(pkg, eng, torch, dev, n, 150, 120, 0)
        torch.cuda.synchronize()
        hvk, hsig, hmsg = vk.cpu().numpy(), sig.cpu().numpy(), msg.cpu().numpy()
        hoff = off.cpu().numpy().astype("uint64")
        hk = (ctypes.c_uint8 * (32 * n))()
        at = lambda arr, byte: ctypes.cast(arr.ctypes.data + byte, u8p)       # noqa: E731
        eng._check(lib.edc_challenge(ctx, n, at(hvk, 0), at(hsig, 0), at(hmsg, 0),
                                     ctypes.cast(hoff.ctypes.data, u64p), hk))
        hk_addr = ctypes.addressof(hk)
        bounds = [n * p // PIECES for p in range(PIECES + 1)]
        v = lib.edc_verifier_create(ctx, n)
        assert v

        def cycle(eager):
            """(verify, 16 queue calls until idle, whole cycle) in ms"""
            t0 = time.perf_counter()
            eng._check(lib.edc_verifier_reset(v))
            if eager:
                eng._check(lib.edc_vfy_begin_eager(v, zseed))
            tq = time.perf_counter()
            for p in range(PIECES):
                if bounds[p + 1] > bounds[p]:
                    eng._check(lib.edc_verifier_queue_prehashed(v, bounds[p + 1] - bounds[p], at(hvk, 32 * bounds[p]),
                                                                at(hsig, 64 * bounds[p]),
                                                                ctypes.cast(hk_addr + 32 * bounds[p], u8p)))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rc = lib.edc_verifier_verify(v, None if eager else zseed, None, None)
            t2 = time.perf_counter()
            assert rc == 0, rc
            return (t2 - t1) * 1e3, (t1 - tq) * 1e3, (t2 - t0) * 1e3

        def measure(out, label, eager):
            for _ in range(a.warmup):
                cycle(eager)
            rs = [cycle(eager) for _ in range(a.reps)]
            out[f"verify_{label}_ms"] = round(statistics.median(r[0] for r in rs), 4)
            out[f"verify_{label}_ms_min"] = round(min(r[0] for r in rs), 4)
            out[f"queue_total_{label}_ms"] = round(statistics.median(r[1] for r in rs), 4)
            out[f"cycle_{label}_ms"] = round(statistics.median(r[2] for r in rs), 4)

        out = {"n": n, "eager_leg": True, "lib": os.path.basename(a.lib) if a.lib else "libedc.so", "validators": 150,
               "pieces": PIECES, "reps": a.reps}
        measure(out, "plain", False)
        for f in folds if has_eager else []:
            eng._check(lib.edc_vfy_set_fold(v, f))
            label = f"eager_fold{f}" if f else "eager"
            measure(out, label, True)
            items, nfold = ctypes.c_uint64(0), ctypes.c_uint64(0)
            eng._check(lib.edc_vfy_folded(v, ctypes.byref(items), ctypes.byref(nfold)))
            out[f"folded_{label}"] = [int(items.value), int(nfold.value)]
        lib.edc_verifier_destroy(v)
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del vk, sig, msg, off
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="150,131072,1048576")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--keycache", action="store_true", help="the registered-validator-set leg (see above)")
    ap.add_argument("--lib", default=None, help="another build of libedc.so to measure")
    ap.add_argument("--eager", action="store_true", help="the eager-mode leg (plain and eager cycles side by side)")
    ap.add_argument("--fold", default="0", help="--eager: fold granularities to measure, 0 = the library default")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    pkg = bench.load_pkg()
    eng = pkg.Engine(0, lib_path=a.lib)
    lib, ctx = eng.lib, eng.ctx
    zseed = bytes([0x33]) * 32
    u8p, u64p = ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)
    lines = []
    if a.keycache:
        lines = keycache_leg(a, pkg, eng, torch, dev)
    elif a.eager:
        lines = eager_leg(a, pkg, eng, torch, dev)
    for n in [] if a.keycache or a.eager else [int(x) for x in a.sizes.split(",")]:
        vk, sig, msg, off = bench.make_workload(pkg, eng, torch, dev, n, 150, 120, 0)
        torch.cuda.synchronize()
        hvk, hsig, hmsg = vk.cpu().numpy(), sig.cpu().numpy(), msg.cpu().numpy()
        hoff = off.cpu().numpy().astype("uint64")
        hk = (ctypes.c_uint8 * (32 * n))()
        at = lambda arr, byte: ctypes.cast(arr.ctypes.data + byte, u8p)       # noqa: E731
        eng._check(lib.edc_challenge(ctx, n, at(hvk, 0), at(hsig, 0), at(hmsg, 0),
                                     ctypes.cast(hoff.ctypes.data, u64p), hk))
        hk_addr = ctypes.addressof(hk)
        dk = torch.frombuffer(bytearray(hk), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        bounds = [n * p // PIECES for p in range(PIECES + 1)]

        def one_device():
            assert lib.edc_batch_verify_device(ctx, n, vk.data_ptr(), sig.data_ptr(), msg.data_ptr(), off.data_ptr(),
                                               zseed, 0, None, None) == 0

        def one_host():
            assert lib.edc_batch_verify(ctx, n, at(hvk, 0), at(hsig, 0), at(hmsg, 0),
                                        ctypes.cast(hoff.ctypes.data, u64p), zseed, None) == 0

        def one_prehashed():
            assert lib.edc_batch_verify_prehashed(ctx, n, at(hvk, 0), at(hsig, 0), ctypes.cast(hk_addr, u8p), zseed, None,
                                                  None) == 0

        v = lib.edc_verifier_create(ctx, n)
        assert v

        def q_host(p0, p1):
            return lib.edc_verifier_queue(v, p1 - p0, at(hvk, 32 * p0), at(hsig, 64 * p0), at(hmsg, 0),
                                          ctypes.cast(hoff.ctypes.data + 8 * p0, u64p))

        def q_prehashed(p0, p1):
            return lib.edc_verifier_queue_prehashed(v, p1 - p0, at(hvk, 32 * p0), at(hsig, 64 * p0),
                                                    ctypes.cast(hk_addr + 32 * p0, u8p))

        def q_device(p0, p1):
            return lib.edc_verifier_queue_device(v, p1 - p0, vk.data_ptr() + 32 * p0, sig.data_ptr() + 64 * p0,
                                                 msg.data_ptr(), off.data_ptr() + 8 * p0, None)

        def q_device_k(p0, p1):
            return lib.edc_verifier_queue_device(v, p1 - p0, vk.data_ptr() + 32 * p0, sig.data_ptr() + 64 * p0, None, None,
                                                 dk.data_ptr() + 32 * p0)

        def cycle(qfn):
            """reset, queue in 16 pieces, idle device, verify: (verify ms, whole cycle ms)"""
            t0 = time.perf_counter()
            eng._check(lib.edc_verifier_reset(v))
            for p in range(PIECES):
                if bounds[p + 1] > bounds[p]:
                    eng._check(qfn(bounds[p], bounds[p + 1]))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rc = lib.edc_verifier_verify(v, zseed, None, None)
            t2 = time.perf_counter()
            assert rc == 0, rc
            return (t2 - t1) * 1e3, (t2 - t0) * 1e3

        out = {"n": n, "validators": 150, "msg_len": 120, "pieces": PIECES, "reps": a.reps}
        for label, fn in (("batch_verify_device_ms", one_device), ("batch_verify_host_ms", one_host),
                          ("batch_verify_prehashed_host_ms", one_prehashed)):
            out[label], out[label + "_min"] = median_ms(fn, a.warmup, a.reps)
        for label, qfn in (("host_msgs", q_host), ("host_prehashed", q_prehashed), ("device_msgs", q_device),
                           ("device_prehashed", q_device_k)):
            for _ in range(a.warmup):
                cycle(qfn)
            rs = [cycle(qfn) for _ in range(a.reps)]
            out[f"verify_after_queue_{label}_ms"] = round(statistics.median(r[0] for r in rs), 4)
            out[f"verify_after_queue_{label}_ms_min"] = round(min(r[0] for r in rs), 4)
            tot = statistics.median(r[1] for r in rs)
            out[f"queue_verify_{label}_ms"] = round(tot, 4)
            out[f"queue_verify_{label}_sigs_per_s"] = round(n / (tot * 1e-3), 1)
        lib.edc_verifier_destroy(v)
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del vk, sig, msg, off, dk
    eng.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
