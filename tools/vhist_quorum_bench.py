"""Validator-set history against the one-set validator-set entries, in one run (include/edc.h, edc_vhist_*).

The votes of tools/valset_quorum_bench.py (2^20 votes from 150 validators, 120-byte messages, 6,991
commits of 150 items, every validator with power 1, every vote a commit vote, threshold floor(2T/3)).
Entries are alternated inside one run and the medians of --reps timings are reported:
  entries      every commit at its own version (commit c at version c, 6,990 versions of --updates
               power updates each, which restate the power 1: the change lists grow, the sets do
               not, so both sides return the same outputs):
               edc_vhist_quorum_verify_device  |  edc_valset_quorum_verify_device, prehashed (d_k)
               and with messages, light and full mode; edc_vhist_quorum_verify  |
               edc_valset_quorum_verify, key_idx forms on host arrays, prehashed
  kernels      the history's join kernel alone (edc_debug_vhist_select, HIP events) with change lists
               of 1, 8 and 64 entries per position, by key bytes and by position, against
               k_vs_resolve alone (edc_debug_valset_select)
  caller       64 commits of 64 distinct versions as 64 x (edc_valset_set_powers +
               edc_valset_quorum_verify_device), what a caller does today, against one
               edc_vhist_quorum_verify_device call on the same commits

  python tools/vhist_quorum_bench.py [--n 1048576] [--reps 20]
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
    ap.add_argument("--updates", type=int, default=4, help="power updates per version")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n, keys = args.n, args.keys
    per = keys
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    lib = eng.lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    at = lambda t, byte: ctypes.c_void_p(t.data_ptr() + byte)
    cp = lambda a, t=ctypes.c_char_p: a.ctypes.data_as(t)
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

    nc = (n + per - 1) // per
    off_np = np.minimum(np.arange(nc + 1, dtype=np.int64) * per, n).astype(np.uint32)
    commit_off = cp(off_np, u32p)
    sizes = np.diff(off_np.astype(np.int64))
    thr_np = (2 * sizes // 3).astype(np.uint64)                  # equal powers of 1: T = the commit's size
    thr = cp(thr_np, u64p)
    flag_np = np.ones(n, dtype=np.uint8)

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
    d_flag = torch.from_numpy(flag_np).to(dev)
    idx_np = kidx.cpu().numpy().astype(np.uint32)
    torch.cuda.synchronize()

    # the validator set: the keys of the first commit, in its order, power 1 each at every version
    eng.keycache_load([h_vk[32 * p: 32 * p + 32].tobytes() for p in range(per)])
    assert eng.valset_set_powers([1] * per) == per

    def set_history(nv, per_version):
        """nv versions; version v restates the power 1 of per_version positions"""
        upd_off = (np.arange(nv + 1, dtype=np.int64) * per_version).astype(np.uint32)
        upd_pos = (np.arange(nv * per_version, dtype=np.int64) % per).astype(np.uint32)
        upd_pw = np.ones(max(nv * per_version, 1), dtype=np.uint64)
        base = np.ones(per, dtype=np.uint64)
        eng._check(lib.edc_vhist_set(eng.ctx, per, cp(base, u64p), nv, cp(upd_off, u32p), cp(upd_pos, u32p), cp(upd_pw, u64p)))
        assert eng.vhist_versions() == nv + 1 and eng.vhist_totals(nv, 1) == ([per], [per])

    set_history(nc - 1, args.updates)
    ver_np = np.arange(nc, dtype=np.uint32)                      # commit c at version c
    commit_ver = cp(ver_np, u32p)
    list_len = 1 + (nc - 1) * args.updates / per

    zseed = bytes([0x33]) * 32
    eng._check(lib.edc_reserve(eng.ctx, n))
    nbad, nchk = ctypes.c_int(0), ctypes.c_size_t(0)
    tally = (ctypes.c_uint64 * nc)()
    cv = ctypes.create_string_buffer(nc)
    checked, c8 = {}, {}

    def device(hist, mode, prehashed):
        fn = lib.edc_vhist_quorum_verify_device if hist else lib.edc_valset_quorum_verify_device
        ver = (commit_ver,) if hist else ()
        out8 = ctypes.create_string_buffer(32)

        def f():
            rc = fn(eng.ctx, nc, commit_off, *ver, vp(d_vk), vp(d_sig), None if prehashed else vp(d_msg),
                    None if prehashed else vp(d_off), vp(d_k) if prehashed else None, vp(d_flag), thr, mode, zseed, cv, None,
                    tally, ctypes.byref(nbad), ctypes.byref(nchk), out8)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            checked[mode] = nchk.value
            c8[(hist, mode, prehashed)] = out8.raw
        return f

    def host_idx(hist, mode):
        fn = lib.edc_vhist_quorum_verify if hist else lib.edc_valset_quorum_verify
        ver = (commit_ver,) if hist else ()

        def f():
            rc = fn(eng.ctx, nc, commit_off, *ver, None, cp(idx_np, u32p), cp(h_sig), None, None, cp(k_np), cp(flag_np), thr, mode,
                    zseed, cv, None, tally, ctypes.byref(nbad), ctypes.byref(nchk), None)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
        return f

    calls = {}
    for mode, label in ((1, "light"), (0, "full")):
        for pre in (True, False):
            for hist in (True, False):
                calls["device_%s%s_%s" % (label, "_prehashed" if pre else "", "vhist" if hist else "valset")] = device(hist, mode, pre)
        for hist in (True, False):
            calls["host_idx_%s_%s" % (label, "vhist" if hist else "valset")] = host_idx(hist, mode)

    # what a caller does today: cut at every change of the set. 64 commits of 64 versions.
    cut = min(64, nc)
    one = np.ones(per, dtype=np.uint64)
    two = np.array([0, per], dtype=np.uint32)

    def cut_calls():
        for c in range(cut):
            a = int(off_np[c])
            eng._check(lib.edc_valset_set_powers(eng.ctx, per, cp(one, u64p)))
            rc = lib.edc_valset_quorum_verify_device(eng.ctx, 1, cp(two, u32p), at(d_vk, 32 * a), at(d_sig, 64 * a), None, None,
                                                     at(d_k, 32 * a), at(d_flag, a), cp(thr_np[c:c + 1], u64p), 1, zseed, cv, None,
                                                     tally, ctypes.byref(nbad), ctypes.byref(nchk), None)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))

    def one_call():
        rc = lib.edc_vhist_quorum_verify_device(eng.ctx, cut, commit_off, commit_ver, vp(d_vk), vp(d_sig), None, None, vp(d_k),
                                                vp(d_flag), thr, 1, zseed, cv, None, tally, ctypes.byref(nbad),
                                                ctypes.byref(nchk), None)
        assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
    # the cut pair alternates in a loop of its own: 64 small calls let the GPU's clocks drop, which
    # the large calls that follow would pay for
    ms = {}
    for group in (calls, {"cut64_valset_set_and_verify": cut_calls, "cut64_vhist_one_call": one_call}):
        for f in group.values():
            for _ in range(args.warmup):
                f()
        ms.update({k: [] for k in group})
        for _ in range(args.reps):                   # alternate, so drift hits every entry alike
            for name, f in group.items():
                t0 = time.perf_counter()
                f()
                ms[name].append((time.perf_counter() - t0) * 1e3)
    assert all(c8[(True, m, p)] == c8[(False, m, p)] for m in (0, 1) for p in (True, False))      # the same list was verified

    # the join kernels alone, in the same run: change lists of 1, 8 and 64 entries per position
    kern = {}
    t = (ctypes.c_float * 2)()
    for length in (1, 8, 64):
        set_history(length - 1, per)                 # every version restates every position
        kver_np = (np.arange(nc, dtype=np.int64) % length).astype(np.uint32)
        row = {}
        for label, kv, ki in (("by_key", cp(h_vk), None), ("by_position", None, cp(idx_np, u32p))):
            eng._check(lib.edc_debug_vhist_select(eng.ctx, nc, commit_off, cp(kver_np, u32p), kv, ki, cp(flag_np), thr, 1, 50, t))
            row["vhist_" + label + "_us"] = round(t[0] * 1e3, 2)
            eng._check(lib.edc_debug_valset_select(eng.ctx, nc, commit_off, kv, ki, cp(flag_np), thr, 1, 50, t))
            row["valset_" + label + "_us"] = round(t[0] * 1e3, 2)
        kern["list_%d" % length] = row
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    ratio = {k[:-6]: round(med[k] / med[k[:-6] + "_valset"], 4) for k in med if k.endswith("_vhist")}
    out = {
        "n": n, "validators": keys, "commits": nc, "items_per_commit": per, "msg_bytes": MSG, "reps": args.reps,
        "versions": nc, "updates_per_version": args.updates, "entries_per_change_list": round(list_len, 1),
        "checked": {"light": checked[1], "full": checked[0]},
        "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "vhist_over_valset": ratio,
        "cut64_set_and_verify_over_one_call": round(med["cut64_valset_set_and_verify"] / med["cut64_vhist_one_call"], 2),
        "join_kernels_us": kern,
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
