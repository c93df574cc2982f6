"""Validator-set quorum commit sets against the quorum entries, in one run (include/edc.h, edc_valset_*).

The votes of tools/quorum_bench.py (2^20 votes from 150 validators, 120-byte messages, 6,991 commits
of 150 items, every validator with power 1, every vote a commit vote, threshold floor(2T/3)): no
commit holds a double vote, so both sides verify the same list. The 150 keys are registered with
their powers; the comparator is handed a power array joined beforehand, so it gets the join for
free. Entries are alternated inside one run and the medians of --reps timings are reported:
  device_*     edc_valset_quorum_verify_device  |  edc_quorum_verify_device, prehashed (d_k) and
               with messages, light and full mode
  host_idx_*   edc_valset_quorum_verify  |  edc_quorum_verify, key_idx forms on host arrays, prehashed
  kernels      the join kernel and the double-vote scan alone (edc_debug_valset_select, HIP events),
               by key bytes and by position

  python tools/valset_quorum_bench.py [--n 1048576] [--reps 20]
"""
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

MSG = 120


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=150)
    ap.add_argument("--commit", type=int, default=150, help="items per commit (at most --keys: no double vote)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n, keys, per = args.n, args.keys, args.commit
    assert per <= keys
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    lib = eng.lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    cp = lambda a, t=ctypes.c_char_p: a.ctypes.data_as(t)
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

    nc = (n + per - 1) // per
    off_np = np.minimum(np.arange(nc + 1, dtype=np.int64) * per, n).astype(np.uint32)
    commit_off = cp(off_np, u32p)
    sizes = np.diff(off_np.astype(np.int64))
    thr_np = (2 * sizes // 3).astype(np.uint64)                  # equal powers of 1: T = the commit's size
    thr = cp(thr_np, u64p)
    power_np, flag_np = np.ones(n, dtype=np.uint64), np.ones(n, dtype=np.uint8)

    d_msg = bench.chacha_device(pkg, eng, torch, bytes([0x22]) * 32, 0, (n * MSG + 63) // 64 + 1, dev)
    d_off = torch.arange(0, n + 1, dtype=torch.int64, device=dev) * MSG
    seeds = bench.chacha_device(pkg, eng, torch, bytes([0x11]) * 32, 0, (keys * 32 + 63) // 64, dev)[: keys * 32]
    kidx = (torch.arange(0, n, dtype=torch.int64, device=dev) % per % keys).to(torch.int32)
    d_vk = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    eng._check(lib.edc_sign_device(eng.ctx, n, vp(seeds), vp(kidx), vp(d_msg), vp(d_off), vp(d_vk), vp(d_sig)))
    torch.cuda.synchronize()
    h_vk, h_sig, h_msg, h_off = d_vk.cpu().numpy(), d_sig.cpu().numpy(), d_msg.cpu().numpy(), d_off.cpu().numpy().astype(np.uint64)
    k_np = np.zeros(n * 32, dtype=np.uint8)
    eng._check(lib.edc_challenge(eng.ctx, n, cp(h_vk), cp(h_sig), cp(h_msg), cp(h_off, u64p), cp(k_np)))
    d_k = torch.from_numpy(k_np).to(dev)
    d_power = torch.from_numpy(power_np.view(np.int64)).to(dev)
    d_flag = torch.from_numpy(flag_np).to(dev)
    idx_np = kidx.cpu().numpy().astype(np.uint32)
    torch.cuda.synchronize()

    # the validator set: the keys of the first commit, in its order, one power each
    eng.keycache_load([h_vk[32 * p: 32 * p + 32].tobytes() for p in range(per)])
    assert eng.valset_set_powers([1] * per) == per

    zseed = bytes([0x33]) * 32
    eng._check(lib.edc_reserve(eng.ctx, n))
    nbad, nchk = ctypes.c_int(0), ctypes.c_size_t(0)
    tally = (ctypes.c_uint64 * nc)()
    cv = ctypes.create_string_buffer(nc)
    checked, c8 = {}, {}

    def device(valset, mode, prehashed):
        fn = lib.edc_valset_quorum_verify_device if valset else lib.edc_quorum_verify_device
        votes = (vp(d_flag),) if valset else (vp(d_power), vp(d_flag))
        out8 = ctypes.create_string_buffer(32)

        def f():
            rc = fn(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), None if prehashed else vp(d_msg),
                    None if prehashed else vp(d_off), vp(d_k) if prehashed else None, *votes, thr, mode, zseed, cv, None,
                    tally, ctypes.byref(nbad), ctypes.byref(nchk), out8)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            checked[mode] = nchk.value
            c8[(valset, mode, prehashed)] = out8.raw
        return f

    def host_idx(valset, mode):
        fn = lib.edc_valset_quorum_verify if valset else lib.edc_quorum_verify
        votes = (cp(flag_np),) if valset else (cp(power_np, u64p), cp(flag_np))

        def f():
            rc = fn(eng.ctx, nc, commit_off, None, cp(idx_np, u32p), cp(h_sig), None, None, cp(k_np), *votes, thr, mode, zseed,
                    cv, None, tally, ctypes.byref(nbad), ctypes.byref(nchk), None)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
        return f

    calls = {}
    for mode, label in ((1, "light"), (0, "full")):
        for pre in (True, False):
            for valset in (True, False):
                calls["device_%s%s_%s" % (label, "_prehashed" if pre else "", "valset" if valset else "quorum")] = device(valset, mode, pre)
        for valset in (True, False):
            calls["host_idx_%s_%s" % (label, "valset" if valset else "quorum")] = host_idx(valset, mode)
    for f in calls.values():
        for _ in range(args.warmup):
            f()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    assert all(c8[(True, m, p)] == c8[(False, m, p)] for m in (0, 1) for p in (True, False))      # the same list was verified
    kern = {}
    t = (ctypes.c_float * 2)()
    for mode, label in ((1, "light"), (0, "full")):
        eng._check(lib.edc_debug_valset_select(eng.ctx, nc, commit_off, cp(h_vk), None, cp(flag_np), thr, mode, 50, t))
        kern[label + "_by_key"] = {"resolve_us": round(t[0] * 1e3, 2), "double_vote_us": round(t[1] * 1e3, 2)}
        eng._check(lib.edc_debug_valset_select(eng.ctx, nc, commit_off, None, cp(idx_np, u32p), cp(flag_np), thr, mode, 50, t))
        kern[label + "_by_position"] = {"resolve_us": round(t[0] * 1e3, 2), "double_vote_us": round(t[1] * 1e3, 2)}
    sel = ctypes.c_float(0)
    eng._check(lib.edc_debug_quorum_select(eng.ctx, nc, commit_off, cp(power_np, u64p), cp(flag_np), thr, 1, 50, ctypes.byref(sel)))
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    ratio = {k[:-7]: round(med[k] / med[k[:-7] + "_quorum"], 4) for k in med if k.endswith("_valset")}
    out = {
        "n": n, "validators": keys, "commits": nc, "items_per_commit": per, "msg_bytes": MSG, "reps": args.reps,
        "checked": {"light": checked[1], "full": checked[0]},
        "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "valset_over_quorum": ratio, "kernels_us": kern, "select_kernels_us_light": round(sel.value * 1e3, 2),
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
