"""Cached quorum commit sets against the uncached quorum calls, in one run (include/edc.h, edc_cached_*).

The README's quorum workload: BASELINE configs[2]-like votes (2^20 votes from 150 validators,
120-byte sign bytes) cut into 6,991 commits of 150 items, every validator with the same power,
every vote a commit vote, threshold floor(2T/3): light mode checks 101 of every 150 votes. The
sign bytes are 4 templates (64-byte head, 44-byte tail, one template per commit) around a 12-byte
hole, so that the same votes serve the plain prehashed forms and the templated ones. Everything is
device-resident; the table holds 4n records.

Per mode (light, full) and hit ratio (the share of the CHECKED votes that are live records), two
calls are timed alternately, --reps times, and the medians reported:
  plain      edc_quorum_verify_device (prehashed)       | edc_cached_quorum_verify_device (prehashed)
  templated  edc_tmpl_quorum_verify_device              | edc_cached_tmpl_quorum_verify_device
Before EVERY timed cached call, outside the timed region, the table is cleared and the chosen
records are planted again (edc_sigcache_batch_verify_device on their gathered copy), since a
cached call leaves its misses behind as records. Each timing is a host clock around one
synchronous call. A median of 20 alternated calls shows a difference of several percent on a quiet
machine; it does not show one of a percent or two, and the spread (min and max) is printed so that
a reader can judge. Ratios below 1 mean the cached call is faster.

  python tools/quorum_cached_bench.py [--n 1048576] [--reps 20] [--ratios 0,0.5,0.9,1.0]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ratios", default="0,0.5,0.9,1.0")
    args = ap.parse_args()
    n, keys, per = args.n, args.keys, args.commit
    ratios = [float(x) for x in args.ratios.split(",")]
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
    power_np, flag_np = np.ones(n, dtype=np.uint64), np.ones(n, dtype=np.uint8)

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
    eng._check(lib.edc_tmpl_expand_device(eng.ctx, ctypes.byref(ts), n, vp(d_tpl), vp(d_var), vp(d_voff), var_bytes, vp(d_msg),
                                          cap, vp(d_off)))
    seeds = bench.chacha_device(pkg, eng, torch, bytes([0x11]) * 32, 0, (keys * 32 + 63) // 64, dev)[: keys * 32]
    kidx = (torch.arange(0, n, dtype=torch.int64, device=dev) % per % keys).to(torch.int32)
    d_vk = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    eng._check(lib.edc_sign_device(eng.ctx, n, vp(seeds), vp(kidx), vp(d_msg), vp(d_off), vp(d_vk), vp(d_sig)))
    torch.cuda.synchronize()
    h_vk, h_sig, h_msg = d_vk.cpu().numpy(), d_sig.cpu().numpy(), d_msg.cpu().numpy()
    h_off = d_off.cpu().numpy().astype(np.uint64)
    k_np = np.zeros(n * 32, dtype=np.uint8)
    eng._check(lib.edc_challenge(eng.ctx, n, h_vk.ctypes.data_as(ctypes.c_char_p), h_sig.ctypes.data_as(ctypes.c_char_p),
                                 h_msg.ctypes.data_as(ctypes.c_char_p), h_off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                 k_np.ctypes.data_as(ctypes.c_char_p)))
    d_k = torch.from_numpy(k_np).to(dev)
    d_power = torch.from_numpy(power_np.view(np.int64)).to(dev)
    d_flag = torch.from_numpy(flag_np).to(dev)
    del d_msg, h_msg
    torch.cuda.synchronize()

    zseed = bytes([0x33]) * 32
    eng._check(lib.edc_reserve(eng.ctx, n))
    eng.sigcache_create(4 * n)
    nbad, nchk, nmiss = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    tally = (ctypes.c_uint64 * nc)()
    cv = ctypes.create_string_buffer(nc)
    tail = lambda: (cv, None, tally, ctypes.byref(nbad), ctypes.byref(nchk))

    def plain(mode):
        rc = lib.edc_quorum_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), None, None, vp(d_k), vp(d_power),
                                          vp(d_flag), thr, mode, zseed, *tail(), None)
        assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))

    def plain_cached(mode):
        rc = lib.edc_cached_quorum_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), None, None, vp(d_k),
                                                 vp(d_power), vp(d_flag), thr, mode, zseed, *tail(), ctypes.byref(nmiss), None)
        assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))

    def tmpl(mode):
        rc = lib.edc_tmpl_quorum_verify_device(eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl, 1, None, vp(d_vk),
                                               vp(d_sig), vp(d_var), vp(d_voff), var_bytes, vp(d_power), vp(d_flag), thr, mode,
                                               zseed, *tail(), None)
        assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))

    def tmpl_cached(mode):
        rc = lib.edc_cached_tmpl_quorum_verify_device(eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl, 1, None,
                                                      vp(d_vk), vp(d_sig), vp(d_var), vp(d_voff), var_bytes, vp(d_power),
                                                      vp(d_flag), thr, mode, zseed, *tail(), ctypes.byref(nmiss), None)
        assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))

    rng = np.random.RandomState(7)
    rows = []
    for mode, label in ((1, "light"), (0, "full")):
        checked, _, m = eng.quorum_plan(off_np.tolist(), power_np.tolist(), flag_np.tolist(), thr_np.tolist(), light=mode == 1)
        order = rng.permutation(np.flatnonzero(np.array(checked, dtype=np.uint8)))
        for ratio in ratios:
            pick = torch.from_numpy(np.sort(order[: int(round(ratio * m))]).astype(np.int64)).to(dev)
            w_vk = d_vk.view(n, 32).index_select(0, pick).contiguous().view(-1)
            w_sig = d_sig.view(n, 64).index_select(0, pick).contiguous().view(-1)
            w_k = d_k.view(n, 32).index_select(0, pick).contiguous().view(-1)
            torch.cuda.synchronize()
            nw = int(pick.numel())

            def plant():
                eng.sigcache_clear()
                if nw:
                    rc = lib.edc_sigcache_batch_verify_device(eng.ctx, nw, vp(w_vk), vp(w_sig), None, None, vp(w_k),
                                                              bytes([0x55]) * 32, None, None)
                    assert rc == 0, (rc, lib.edc_last_error(eng.ctx))

            for kind, base, cached in (("plain", plain, plain_cached), ("templated", tmpl, tmpl_cached)):
                for _ in range(args.warmup):
                    base(mode)
                    plant()
                    cached(mode)
                assert nchk.value == m and nmiss.value == m - nw, (nchk.value, nmiss.value, m, nw)
                last = list(eng.cached_quorum_last())
                tb, tc = [], []
                for _ in range(args.reps):               # alternate, so drift hits both alike
                    t0 = time.perf_counter()
                    base(mode)
                    tb.append((time.perf_counter() - t0) * 1e3)
                    plant()                              # outside the timed region
                    t0 = time.perf_counter()
                    cached(mode)
                    tc.append((time.perf_counter() - t0) * 1e3)
                mb, mc = statistics.median(tb), statistics.median(tc)
                row = {"form": kind, "mode": label, "hit_ratio": ratio, "n_checked": m, "n_miss": m - nw,
                       "uncached_ms": round(mb, 3), "cached_ms": round(mc, 3), "cached_over_uncached": round(mc / mb, 4),
                       "uncached_min_max": [round(min(tb), 3), round(max(tb), 3)],
                       "cached_min_max": [round(min(tc), 3), round(max(tc), 3)], "last": last}
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"n": n, "validators": keys, "commits": nc, "items_per_commit": per, "msg_bytes": MSG, "hole_bytes": HOLE,
           "templates": NTPL, "table_records": 4 * n, "reps": args.reps, "stats": eng.sigcache_stats(), "rows": rows}
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
