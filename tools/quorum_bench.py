"""Quorum commit sets against the plain commit-set call, in one run (include/edc.h, edc_quorum_*).

BASELINE configs[2]-like votes (2^20 votes from 150 validators, 120-byte messages) cut into 6,991
commits of 150 items, every validator with the same power, every vote a commit vote and the
threshold floor(2T/3) of each commit's power: light mode checks 101 of every 150 votes. Entries are
alternated inside one run and the medians of --reps timings are reported:
  light / full       edc_quorum_verify_device  |  edc_commits_verify_device on the same set
  *_prehashed        the same three with d_k: what is left when no vote is hashed (the message
                     forms hash every vote, the skipped ones included)
  select             the selection kernels alone (edc_debug_quorum_select, HIP events)

  python tools/quorum_bench.py [--n 1048576] [--reps 20]
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
    ap.add_argument("--commit", type=int, default=150, help="items per commit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    n, keys, per = args.n, args.keys, args.commit
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    lib = eng.lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    nc = (n + per - 1) // per
    off_np = np.minimum(np.arange(nc + 1, dtype=np.int64) * per, n).astype(np.uint32)
    commit_off = off_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    sizes = np.diff(off_np.astype(np.int64))
    thr_np = (2 * sizes // 3).astype(np.uint64)                  # equal powers of 1: T = the commit's size
    thr = thr_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
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
    eng._check(lib.edc_challenge(eng.ctx, n, h_vk.ctypes.data_as(ctypes.c_char_p), h_sig.ctypes.data_as(ctypes.c_char_p),
                                 h_msg.ctypes.data_as(ctypes.c_char_p), h_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                 k_np.ctypes.data_as(ctypes.c_char_p)))
    d_k = torch.from_numpy(k_np).to(dev)
    d_power = torch.from_numpy(power_np.view(np.int64)).to(dev)
    d_flag = torch.from_numpy(flag_np).to(dev)
    torch.cuda.synchronize()

    zseed = bytes([0x33]) * 32
    eng._check(lib.edc_reserve(eng.ctx, n))
    nbad, nchk = ctypes.c_int(0), ctypes.c_size_t(0)
    tally = (ctypes.c_uint64 * nc)()
    cv = ctypes.create_string_buffer(nc)
    checked = {}

    def quorum(mode, prehashed):
        def f():
            rc = lib.edc_quorum_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), None if prehashed else vp(d_msg),
                                              None if prehashed else vp(d_off), vp(d_k) if prehashed else None, vp(d_power),
                                              vp(d_flag), thr, mode, zseed, cv, None, tally, ctypes.byref(nbad),
                                              ctypes.byref(nchk), None)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            checked[mode] = nchk.value
        return f

    def commits(prehashed):
        def f():
            rc = lib.edc_commits_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), None if prehashed else vp(d_msg),
                                               None if prehashed else vp(d_off), vp(d_k) if prehashed else None, zseed, cv,
                                               None, ctypes.byref(nbad))
            assert rc == 0, (rc, lib.edc_last_error(eng.ctx))
        return f

    calls = {"light": quorum(1, False), "full": quorum(0, False), "commits": commits(False),
             "light_prehashed": quorum(1, True), "full_prehashed": quorum(0, True), "commits_prehashed": commits(True)}
    for f in calls.values():
        for _ in range(args.warmup):
            f()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    sel = {}
    for mode, label in ((1, "light"), (0, "full")):
        t = ctypes.c_float(0)
        eng._check(lib.edc_debug_quorum_select(eng.ctx, nc, commit_off, power_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                               flag_np.ctypes.data_as(ctypes.c_char_p), thr, mode, 50, ctypes.byref(t)))
        sel[label] = round(t.value * 1e3, 2)
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    out = {
        "n": n, "validators": keys, "commits": nc, "items_per_commit": per, "msg_bytes": MSG, "reps": args.reps,
        "checked": {"light": checked[1], "full": checked[0]}, "checked_fraction_light": round(checked[1] / n, 4),
        "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "light_over_commits": round(med["light"] / med["commits"], 4),
        "full_over_commits": round(med["full"] / med["commits"], 4),
        "light_prehashed_over_commits_prehashed": round(med["light_prehashed"] / med["commits_prehashed"], 4),
        "full_prehashed_over_commits_prehashed": round(med["full_prehashed"] / med["commits_prehashed"], 4),
        "hashing_all_votes_ms": round(med["light"] - med["light_prehashed"], 3),
        "select_kernels_us": sel,
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
