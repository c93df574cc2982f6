"""Templated messages against the message entries, in one run (include/edc.h, edc_tmpl_*).

BASELINE configs[2] (2^20 votes from 150 validators, 120-byte messages) re-expressed as 4 templates
with a 12-byte hole: message i = head[tpl[i]] + hole_i + tail[tpl[i]]. The same signed items go
through the new and the existing entries alternately, and the medians of --reps timings are
reported:
  host call    edc_tmpl_batch_verify (key_idx)  |  edc_batch_verify  |  edc_batch_verify_prehashed
  stream       edc_tmpl_batch_submit (key_idx)  |  edc_batch_submit_indexed      (--inflight in flight)
  device       edc_tmpl_batch_verify_device     |  edc_batch_verify_device       (difference = expansion)

  python tools/template_bench.py [--n 1048576] [--reps 20] [--inflight 4]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--stream-batches", type=int, default=8, help="batches per timed stream run")
    args = ap.parse_args()
    n, keys = args.n, args.keys
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    lib = eng.lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    # the set and the items; the materialised arena comes from edc_tmpl_expand_device
    rnd = np.random.default_rng(0x7E)
    t = pkg.batch.Templates([rnd.bytes(k) for k in HEADS], [rnd.bytes(k) for k in TAILS])
    ts, _keep = t.struct()
    tpl_h = torch.from_numpy(np.where(np.arange(n) % 8 == 0, 1 + (np.arange(n) // 8) % 3, 0).astype(np.int16))
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
    torch.cuda.synchronize()

    zseed = bytes([0x33]) * 32
    h_vk, h_sig, h_msg, h_off, h_idx = d_vk.cpu(), d_sig.cpu(), d_msg[: 120 * n].cpu(), d_off.cpu(), kidx.cpu()
    kb = h_vk[: 32 * keys].numpy().tobytes()
    eng.keycache_load([kb[32 * i:32 * i + 32] for i in range(keys)])
    h_k = torch.empty(32 * n, dtype=torch.uint8)
    cp = lambda x: ctypes.cast(ctypes.c_void_p(x.data_ptr()), ctypes.c_char_p)
    u16 = ctypes.cast(ctypes.c_void_p(tpl_h.data_ptr()), ctypes.POINTER(ctypes.c_uint16))
    u32 = lambda x: ctypes.cast(ctypes.c_void_p(x.data_ptr()), ctypes.POINTER(ctypes.c_uint32))
    u64 = ctypes.cast(ctypes.c_void_p(h_off.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
    eng._check(lib.edc_challenge(eng.ctx, n, cp(h_vk), cp(h_sig), cp(h_msg), u64, ctypes.c_void_p(h_k.data_ptr())))
    eng._check(lib.edc_set_slots(eng.ctx, args.inflight))
    eng._check(lib.edc_reserve(eng.ctx, n))

    def ok(rc):
        assert rc == 0, f"valid batch rejected: {rc} {lib.edc_last_error(eng.ctx)}"

    calls = {
        "host_tmpl_key_idx": lambda: ok(lib.edc_tmpl_batch_verify(eng.ctx, ctypes.byref(ts), n, None, u32(h_idx), cp(h_sig),
                                                                  u16, cp(var_h), u32(voff_h), zseed, None)),
        "host_msg": lambda: ok(lib.edc_batch_verify(eng.ctx, n, cp(h_vk), cp(h_sig), cp(h_msg), u64, zseed, None)),
        "host_prehashed": lambda: ok(lib.edc_batch_verify_prehashed(eng.ctx, n, cp(h_vk), cp(h_sig), cp(h_k), zseed, None,
                                                                    None)),
        "device_tmpl": lambda: ok(lib.edc_tmpl_batch_verify_device(eng.ctx, ctypes.byref(ts), n, vp(d_vk), vp(d_sig),
                                                                   vp(d_tpl), vp(d_var), vp(d_voff), var_bytes, zseed, 0,
                                                                   None, None)),
        "device_msg": lambda: ok(lib.edc_batch_verify_device(eng.ctx, n, vp(d_vk), vp(d_sig), vp(d_msg), vp(d_off), zseed,
                                                             0, None, None)),
    }
    submit = {
        "stream_tmpl_key_idx": lambda: lib.edc_tmpl_batch_submit(eng.ctx, ctypes.byref(ts), n, None, u32(h_idx), cp(h_sig),
                                                                 u16, cp(var_h), u32(voff_h), zseed, 0, 0),
        "stream_msg_key_idx": lambda: lib.edc_batch_submit_indexed(eng.ctx, n, u32(h_idx), cp(h_sig), cp(h_msg), u64, zseed,
                                                                   0, 0),
    }

    def stream(f, k):
        pending = []
        for _ in range(k):
            if len(pending) >= args.inflight:
                ok(lib.edc_batch_wait(eng.ctx, pending.pop(0), None, None, None))
            tk = f()
            assert tk >= 0, lib.edc_last_error(eng.ctx)
            pending.append(tk)
        while pending:
            ok(lib.edc_batch_wait(eng.ctx, pending.pop(0), None, None, None))

    for f in calls.values():
        for _ in range(args.warmup):
            f()
    for f in submit.values():
        stream(f, max(args.warmup, args.inflight))
    ms = {k: [] for k in list(calls) + list(submit)}
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
        for name, f in submit.items():
            t0 = time.perf_counter()
            stream(f, args.stream_batches)
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.stream_batches)
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    out = {
        "n": n, "validators": keys, "msg_bytes": 120, "templates": t.count, "hole_bytes": HOLE, "reps": args.reps,
        "inflight": args.inflight, "median_ms": med,
        "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "bytes_per_vote": {"tmpl_key_idx": 4 + 64 + 2 + 4 + HOLE, "msg": 32 + 64 + 120 + 8, "msg_key_idx": 4 + 64 + 120 + 8,
                           "prehashed": 128},
        "host_tmpl_over_msg": round(med["host_tmpl_key_idx"] / med["host_msg"], 3),
        "host_tmpl_over_prehashed": round(med["host_tmpl_key_idx"] / med["host_prehashed"], 3),
        "stream_tmpl_over_msg_key_idx": round(med["stream_tmpl_key_idx"] / med["stream_msg_key_idx"], 3),
        "stream_sigs_per_s": {k: round(n / med[k] * 1e3, 1) for k in submit},
        "expansion_ms": round(med["device_tmpl"] - med["device_msg"], 3),
    }
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
