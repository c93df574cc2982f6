"""Commit sets against the existing entries, in one run (include/edc.h, edc_commits_*).

BASELINE configs[2]-like votes (2^20 votes from 150 validators, 120-byte messages, 4 templates with a
12-byte hole) cut into commits of 150 items, one template per commit. Entries are alternated inside
one run and the medians of --reps timings are reported:
  device, passing   edc_commits_verify_device  |  edc_batch_verify_device on the same union
                    (the commit set adds no kernel and no synchronization: the ratio must sit inside
                    the run-to-run spread of such medians)
  stream            edc_tmpl_commits_submit with key indices  |  edc_tmpl_batch_submit with key
                    indices on the same items (per-item tpl array), --inflight in flight
  failing           one bad signature: edc_commits_submit_device + edc_commits_wait (union, grouped
                    fallback on the ticket's slot, reduction), the synchronous
                    edc_commits_verify_device  |  edc_batch_verify_device alone
  before            a loop of edc_batch_verify_device per commit over --loop-commits commits, last
                    in every round: 150 items from 150 validators make the context's automatic key
                    grouping give up for the next batches, so 8 untimed union batches follow it
  map               k_tmpl_commit_map alone (edc_debug_tmpl_commit_map, HIP events)
  variants          the same votes with alt_span 4 and the four templates spread over the ITEMS (a
                    hash of the item index), signed as such: edc_tmpl_commits_submit_alt with key
                    indices  |  the stream row's edc_tmpl_commits_submit, and
                    edc_tmpl_batch_submit on the variants workload (what the spread templates
                    alone cost the expansion);
                    edc_tmpl_commits_verify_device  |  the device row's edc_commits_verify_device;
                    k_tmpl_commit_map_alt alone  |  the map row. Every message is 120 bytes in both
                    workloads, so the rows differ by the variant byte and the map kernel only.

  python tools/commits_bench.py [--n 1048576] [--reps 20] [--inflight 4]
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

HEADS, TAILS, HOLE = [70, 71, 70, 108], [38, 37, 38, 0], 12     # every message is 120 bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=150)
    ap.add_argument("--commit", type=int, default=150, help="items per commit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--stream-sets", type=int, default=8, help="commit sets per timed stream run")
    ap.add_argument("--loop-commits", type=int, default=512)
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
    ctpl_np = (np.arange(nc) % 4).astype(np.uint16)
    commit_off = off_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    commit_tpl = ctpl_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))

    # the set and the items; the materialised arena comes from edc_tmpl_expand_device
    rnd = np.random.default_rng(0xC0)
    t = pkg.batch.Templates([rnd.bytes(k) for k in HEADS], [rnd.bytes(k) for k in TAILS])
    ts, _keep = t.struct()
    tpl_h = torch.from_numpy(((np.arange(n) // per) % 4).astype(np.int16))
    var_h = bench.chacha_device(pkg, eng, torch, bytes([0x22]) * 32, 0, (n * HOLE + 63) // 64, dev)[: n * HOLE].cpu()
    voff_h = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * HOLE).astype(np.uint32).view(np.int32))
    d_tpl, d_var, d_voff = tpl_h.to(dev), var_h.to(dev), voff_h.to(dev)
    var_bytes = n * HOLE
    cap = n * (max(HEADS) + max(TAILS)) + var_bytes + 16
    d_msg = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng._check(lib.edc_tmpl_expand_device(eng.ctx, ctypes.byref(ts), n, vp(d_tpl), vp(d_var), vp(d_voff), var_bytes,
                                          vp(d_msg), cap, vp(d_off)))
    assert int(d_off[n]) == 120 * n
    seeds = bench.chacha_device(pkg, eng, torch, bytes([0x11]) * 32, 0, (keys * 32 + 63) // 64, dev)[: keys * 32]
    kidx = (torch.arange(0, n, dtype=torch.int64, device=dev) % keys).to(torch.int32)
    d_vk = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    eng._check(lib.edc_sign_device(eng.ctx, n, vp(seeds), vp(kidx), vp(d_msg), vp(d_off), vp(d_vk), vp(d_sig)))
    # the variants workload: every commit owns templates [0, 4) and item i takes template alt[i]
    alt_np = ((np.arange(n, dtype=np.uint64) * 2654435761 >> 13) % 4).astype(np.uint8)
    alt_h = torch.from_numpy(alt_np)
    ctpl0_np = np.zeros(nc, dtype=np.uint16)
    commit_tpl0 = ctpl0_np.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))
    tpl2_h = torch.from_numpy(alt_np.astype(np.int16))
    d_alt, d_tpl2 = alt_h.to(dev), tpl2_h.to(dev)
    d_sig2 = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    d_msg2 = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng._check(lib.edc_tmpl_expand_device(eng.ctx, ctypes.byref(ts), n, vp(d_tpl2), vp(d_var), vp(d_voff), var_bytes,
                                          vp(d_msg2), cap, vp(d_off2)))
    assert int(d_off2[n]) == 120 * n
    d_vk2 = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    eng._check(lib.edc_sign_device(eng.ctx, n, vp(seeds), vp(kidx), vp(d_msg2), vp(d_off2), vp(d_vk2), vp(d_sig2)))
    torch.cuda.synchronize()
    assert torch.equal(d_vk2, d_vk)
    h_sig2 = d_sig2.cpu()
    del d_msg2, d_off2, d_vk2, d_tpl2
    d_sig_bad = d_sig.clone()
    bad_item = n // 2 + 7
    d_sig_bad[64 * bad_item + 40] = d_sig_bad[64 * bad_item + 40] ^ 1
    torch.cuda.synchronize()

    zseed = bytes([0x33]) * 32
    h_vk, h_sig, h_idx = d_vk.cpu(), d_sig.cpu(), kidx.cpu()
    kb = h_vk[: 32 * keys].numpy().tobytes()
    eng.keycache_load([kb[32 * i:32 * i + 32] for i in range(keys)])
    cp = lambda x: ctypes.cast(ctypes.c_void_p(x.data_ptr()), ctypes.c_char_p)
    u32 = lambda x: ctypes.cast(ctypes.c_void_p(x.data_ptr()), ctypes.POINTER(ctypes.c_uint32))
    eng._check(lib.edc_set_slots(eng.ctx, args.inflight))
    eng._check(lib.edc_reserve(eng.ctx, n))
    cv = ctypes.create_string_buffer(nc)
    iv = ctypes.create_string_buffer(n)
    nbad = ctypes.c_int(0)

    def ok(rc):
        assert rc == 0, f"valid set rejected: {rc} {lib.edc_last_error(eng.ctx)}"

    def failing_commits():
        tk = lib.edc_commits_submit_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig_bad), vp(d_msg), vp(d_off), None,
                                           zseed)
        assert tk >= 0, lib.edc_last_error(eng.ctx)
        rc = lib.edc_commits_wait(eng.ctx, tk, cv, iv, ctypes.byref(nbad))
        assert rc == 1 and nbad.value == 1 and cv.raw[bad_item // per] == 1 and iv.raw[bad_item] == 1, rc

    def failing_sync():
        rc = lib.edc_commits_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig_bad), vp(d_msg), vp(d_off), None,
                                           zseed, cv, iv, ctypes.byref(nbad))
        assert rc == 1 and nbad.value == 1 and cv.raw[bad_item // per] == 1 and iv.raw[bad_item] == 1, rc

    def failing_batch():
        assert lib.edc_batch_verify_device(eng.ctx, n, vp(d_vk), vp(d_sig_bad), vp(d_msg), vp(d_off), zseed, 0, None,
                                           None) == 1

    loop_commits = min(args.loop_commits, n // per)

    def loop_per_commit():
        for c in range(loop_commits):
            a = c * per
            ok(lib.edc_batch_verify_device(eng.ctx, per, ctypes.c_void_p(d_vk.data_ptr() + 32 * a),
                                           ctypes.c_void_p(d_sig.data_ptr() + 64 * a), vp(d_msg),
                                           ctypes.c_void_p(d_off.data_ptr() + 8 * a), zseed, 0, None, None))

    calls = {
        "device_commits": lambda: ok(lib.edc_commits_verify_device(eng.ctx, nc, commit_off, vp(d_vk), vp(d_sig), vp(d_msg),
                                                                   vp(d_off), None, zseed, cv, iv, ctypes.byref(nbad))),
        "device_batch": lambda: ok(lib.edc_batch_verify_device(eng.ctx, n, vp(d_vk), vp(d_sig), vp(d_msg), vp(d_off), zseed,
                                                               0, None, None)),
        "device_tmpl_commits_alt": lambda: ok(lib.edc_tmpl_commits_verify_device(
            eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl0, 4, vp(d_alt), vp(d_vk), vp(d_sig2), vp(d_var), vp(d_voff),
            var_bytes, zseed, cv, iv, ctypes.byref(nbad))),
        "failing_commits_wait": failing_commits,
        "failing_commits_sync": failing_sync,
        "failing_batch_alone": failing_batch,
    }
    u16 = ctypes.cast(ctypes.c_void_p(tpl_h.data_ptr()), ctypes.POINTER(ctypes.c_uint16))
    submit = {
        "stream_tmpl_commits_key_idx": (
            lambda: lib.edc_tmpl_commits_submit(eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl, None, u32(h_idx),
                                                cp(h_sig), cp(var_h), u32(voff_h), zseed),
            lambda tk: lib.edc_commits_wait(eng.ctx, tk, cv, iv, ctypes.byref(nbad))),
        "stream_tmpl_commits_alt_key_idx": (
            lambda: lib.edc_tmpl_commits_submit_alt(eng.ctx, ctypes.byref(ts), nc, commit_off, commit_tpl0, 4, vp(alt_h), None,
                                                    u32(h_idx), cp(h_sig2), cp(var_h), u32(voff_h), zseed),
            lambda tk: lib.edc_commits_wait(eng.ctx, tk, cv, iv, ctypes.byref(nbad))),
        # the variants workload through the existing per-item entry: what the spread templates alone cost
        "stream_tmpl_batch_spread_key_idx": (
            lambda: lib.edc_tmpl_batch_submit(eng.ctx, ctypes.byref(ts), n, None, u32(h_idx), cp(h_sig2),
                                              ctypes.cast(ctypes.c_void_p(tpl2_h.data_ptr()), ctypes.POINTER(ctypes.c_uint16)),
                                              cp(var_h), u32(voff_h), zseed, 0, 0),
            lambda tk: lib.edc_batch_wait(eng.ctx, tk, None, None, None)),
        "stream_tmpl_batch_key_idx": (
            lambda: lib.edc_tmpl_batch_submit(eng.ctx, ctypes.byref(ts), n, None, u32(h_idx), cp(h_sig), u16, cp(var_h),
                                              u32(voff_h), zseed, 0, 0),
            lambda tk: lib.edc_batch_wait(eng.ctx, tk, None, None, None)),
    }

    def stream(fw, k):
        f, wait = fw
        pending = []
        for _ in range(k):
            if len(pending) >= args.inflight:
                ok(wait(pending.pop(0)))
            tk = f()
            assert tk >= 0, lib.edc_last_error(eng.ctx)
            pending.append(tk)
        while pending:
            ok(wait(pending.pop(0)))

    def settle():                                    # untimed: automatic key grouping groups again
        for _ in range(8):
            calls["device_batch"]()

    for f in calls.values():
        for _ in range(args.warmup):
            f()
    for fw in submit.values():
        stream(fw, max(args.warmup, args.inflight))
    loop_per_commit()
    settle()
    ms = {k: [] for k in list(calls) + list(submit) + ["loop_per_commit"]}
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
        for name, fw in submit.items():
            t0 = time.perf_counter()
            stream(fw, args.stream_sets)
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.stream_sets)
        t0 = time.perf_counter()
        loop_per_commit()
        ms["loop_per_commit"].append((time.perf_counter() - t0) * 1e3)
        settle()
    # the map kernel alone: device events around 50 launches
    tpl_out = np.zeros(n, dtype=np.uint16)
    map_ms = ctypes.c_float(0)
    eng._check(lib.edc_debug_tmpl_commit_map(eng.ctx, nc, commit_off, commit_tpl,
                                             tpl_out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), 50,
                                             ctypes.byref(map_ms)))
    assert (tpl_out == tpl_h.numpy().view(np.uint16)).all()
    map_alt_ms, flagged = ctypes.c_float(0), ctypes.c_int(-1)
    eng._check(lib.edc_debug_tmpl_commit_map_alt(eng.ctx, nc, commit_off, commit_tpl0, 4, vp(alt_h),
                                                 ctypes.c_void_p(tpl_out.ctypes.data), ctypes.byref(flagged), 50,
                                                 ctypes.byref(map_alt_ms)))
    assert flagged.value == 0 and (tpl_out == alt_np).all()
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    out = {
        "n": n, "validators": keys, "commits": nc, "items_per_commit": per, "msg_bytes": 120, "templates": t.count,
        "reps": args.reps, "inflight": args.inflight, "median_ms": med,
        "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "device_commits_over_batch": round(med["device_commits"] / med["device_batch"], 4),
        "sigs_per_s": {
            "device_commits": round(n / med["device_commits"] * 1e3, 1),
            "device_batch": round(n / med["device_batch"] * 1e3, 1),
            "loop_per_commit": round(loop_commits * per / med["loop_per_commit"] * 1e3, 1),
            "stream_tmpl_commits_key_idx": round(n / med["stream_tmpl_commits_key_idx"] * 1e3, 1),
            "stream_tmpl_batch_key_idx": round(n / med["stream_tmpl_batch_key_idx"] * 1e3, 1),
            "failing_commits_wait": round(n / med["failing_commits_wait"] * 1e3, 1),
            "stream_tmpl_commits_alt_key_idx": round(n / med["stream_tmpl_commits_alt_key_idx"] * 1e3, 1),
            "device_tmpl_commits_alt": round(n / med["device_tmpl_commits_alt"] * 1e3, 1),
        },
        "loop_commits": loop_commits,
        "failing_over_batch_alone": round(med["failing_commits_wait"] / med["failing_batch_alone"], 3),
        "failing_sync_over_batch_alone": round(med["failing_commits_sync"] / med["failing_batch_alone"], 3),
        "stream_commits_over_batch": round(med["stream_tmpl_commits_key_idx"] / med["stream_tmpl_batch_key_idx"], 3),
        "map_kernel_us": round(map_ms.value * 1e3, 2),
        "map_kernel_bytes": int(2 * n + 4 * (nc + 1) + 2 * nc),
        "alt_span": 4,
        "stream_alt_over_tmpl_commits": round(med["stream_tmpl_commits_alt_key_idx"] / med["stream_tmpl_commits_key_idx"], 4),
        "stream_alt_over_tmpl_batch_spread": round(med["stream_tmpl_commits_alt_key_idx"] /
                                                   med["stream_tmpl_batch_spread_key_idx"], 4),
        "device_tmpl_alt_over_device_commits": round(med["device_tmpl_commits_alt"] / med["device_commits"], 4),
        "map_alt_kernel_us": round(map_alt_ms.value * 1e3, 2),
        "map_alt_kernel_bytes": int(3 * n + 4 * (nc + 1) + 2 * nc),
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
