"""Templated quorum commit sets against what a caller had to do before them, in one run
(include/edc.h, edc_tmpl_quorum_*).

BASELINE configs[2]-like votes (2^20 votes from 150 validators, 120-byte sign bytes) cut into 6,991
commits of 150 items, every validator with the same power, every vote a commit vote and the
threshold floor(2T/3) of each commit's power: light mode checks 101 of every 150 votes. The sign
bytes are 4 templates (64-byte head, 44-byte tail, one template per commit) around a 12-byte hole.
Everything is device-resident. Entries are alternated inside one run and the medians of --reps
timings are reported:
  a_light / a_full   edc_tmpl_quorum_verify_device: select first, hash only the checked votes
  b_light / b_full   edc_tmpl_expand_device of all n votes into a caller arena, then
                     edc_quorum_verify_device on that arena (hashes every vote)
  c_commits          edc_tmpl_commits_verify_device (every vote verified, no voting power)

  python tools/tmpl_quorum_bench.py [--n 1048576] [--reps 20]
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

HEAD, HOLE, TAIL, NTPL = 64, 12, 44, 4
MSG = HEAD + HOLE + TAIL


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
    ctpl_np = (np.arange(nc) % NTPL).astype(np.uint16)
    commit_tpl = ctpl_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))

    blob = bench.chacha_device(pkg, eng, torch, bytes([0x44]) * 32, 0, (NTPL * MSG + 63) // 64 + 1, dev).cpu().numpy().tobytes()
    heads = [blob[t * HEAD:(t + 1) * HEAD] for t in range(NTPL)]
    tails = [blob[NTPL * HEAD + t * TAIL:NTPL * HEAD + (t + 1) * TAIL] for t in range(NTPL)]
    T = pkg.batch.Templates(heads, tails)
    ts, _keep = T.struct()

    var_bytes = n * HOLE
    d_var = bench.chacha_device(pkg, eng, torch, bytes([0x22]) * 32, 0, (var_bytes + 63) // 64 + 1, dev)
    d_voff = (torch.arange(0, n + 1, dtype=torch.int64, device=dev) * HOLE).to(torch.int32)
    d_tpl = (torch.arange(0, n, dtype=torch.int64, device=dev) // per % NTPL).to(torch.int16)
    cap = n * MSG + 64
    d_msg = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def expand():
        rc = lib.edc_tmpl_expand_device(eng.ctx, ctypes.byref(ts), n, vp(d_tpl), vp(d_var), vp(d_voff), var_bytes, vp(d_msg),
                                        cap, vp(d_off))
        assert rc == 0, (rc, lib.edc_last_error(eng.ctx))
    expand()
    seeds = bench.chacha_device(pkg, eng, torch, bytes([0x11]) * 32, 0, (keys * 32 + 63) // 64, dev)[: keys * 32]
    kidx = (torch.arange(0, n, dtype=torch.int64, device=dev) % per % keys).to(torch.int32)
    d_vk = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    eng._check(lib.edc_sign_device(eng.ctx, n, vp(seeds), vp(kidx), vp(d_msg), vp(d_off), vp(d_vk), vp(d_sig)))
    d_power = torch.ones(n, dtype=torch.int64, device=dev)
    d_flag = torch.ones(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    zseed = bytes([0x33]) * 32
    eng._check(lib.edc_reserve(eng.ctx, n))
    nbad, nchk = ctypes.c_int(0), ctypes.c_size_t(0)
    tally = (ctypes.c_uint64 * nc)()
    cv = ctypes.create_string_buffer(nc)
    checked, hashed = {}, {}

    def tq(mode):
        def f():
            rc = lib.edc_tmpl_quorum_verify_device(eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl, 1, None, vp(d_vk),
                                                   vp(d_sig), vp(d_var), vp(d_voff), var_bytes, vp(d_power), vp(d_flag), thr,
                                                   mode, zseed, cv, None, tally, ctypes.byref(nbad), ctypes.byref(nchk), None)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            checked[mode] = nchk.value
        return f

    def today(mode):
        def f():
            expand()
            rc = lib.edc_quorum_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), vp(d_msg), vp(d_off), None,
                                              vp(d_power), vp(d_flag), thr, mode, zseed, cv, None, tally, ctypes.byref(nbad),
                                              ctypes.byref(nchk), None)
            assert rc == 0 and nbad.value == 0 and nchk.value == checked[mode], (rc, lib.edc_last_error(eng.ctx))
        return f

    def commits():
        rc = lib.edc_tmpl_commits_verify_device(eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl, 1, None, vp(d_vk),
                                                vp(d_sig), vp(d_var), vp(d_voff), var_bytes, zseed, cv, None, ctypes.byref(nbad))
        assert rc == 0, (rc, lib.edc_last_error(eng.ctx))

    calls = {"a_light": tq(1), "a_full": tq(0), "b_light": today(1), "b_full": today(0), "c_commits": commits}
    for name, f in calls.items():
        for _ in range(args.warmup):
            f()
        if name.startswith("a_"):
            hashed[name] = list(eng.tmpl_quorum_last())
    ms = {k: [] for k in calls}
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    out = {
        "n": n, "validators": keys, "commits": nc, "items_per_commit": per, "msg_bytes": MSG, "hole_bytes": HOLE,
        "templates": NTPL, "reps": args.reps,
        "checked": {"light": checked[1], "full": checked[0]}, "checked_fraction_light": round(checked[1] / n, 4),
        "last": hashed,                              # n, n_checked, items expanded and hashed, arena bytes
        "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "a_light_over_b_light": round(med["a_light"] / med["b_light"], 4),
        "a_full_over_b_full": round(med["a_full"] / med["b_full"], 4),
        "a_light_over_c_commits": round(med["a_light"] / med["c_commits"], 4),
        "saved_ms_light": round(med["b_light"] - med["a_light"], 3),
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
