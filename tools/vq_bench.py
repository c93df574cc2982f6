"""Validator-set requests (include/edc.h, edc_vq_verify) against the entries they replace, in one run.

The votes of tools/vhist_quorum_bench.py (2^20 votes from 150 validators, 120-byte messages, 6,991
commits of 150, power 1 each, every vote a commit vote, threshold floor(2T/3), every commit at its own
version), here as 4 templates (54-byte head, 12-byte hole, 54-byte tail; variant i % 4). Everything is
host memory by key index, light mode, alternated inside one run, medians of --reps timings:
  tmpl        the templated request  |  edc_vhist_quorum_verify on the materialised messages (what
              the caller ships today)  |  edc_tmpl_quorum_verify fed a power array joined beforehand
  k           the prehashed request  |  edc_vhist_quorum_verify prehashed, the entry it replaces
              (the same stages; a build whose gathers took the kept keys by position was measured
              with this pair, profiles/vq_bypos_bench.log)
  cached      the templated and the prehashed request through the table, at hit ratio 0 (table
              cleared before the call) and 1.0 (the same call again)
Hit ratios 0.5 and 0.9 are not measured here.

  python tools/vq_bench.py [--n 1048576] [--reps 20]
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

HEAD, HOLE, TAIL, NT = 54, 12, 54, 4
MSG = HEAD + HOLE + TAIL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=int, default=150)
    ap.add_argument("--updates", type=int, default=4, help="power updates per version")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n, per = args.n, args.keys
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    pkg = bench.load_pkg()
    eng = pkg.Engine(0)
    lib = eng.lib
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    cp = lambda a, t=ctypes.c_char_p: a.ctypes.data_as(t)
    addr = lambda a: a.ctypes.data
    u32p, u64p, u16p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint16)

    nc = (n + per - 1) // per
    off_np = np.minimum(np.arange(nc + 1, dtype=np.int64) * per, n).astype(np.uint32)
    thr_np = (2 * np.diff(off_np.astype(np.int64)) // 3).astype(np.uint64)
    flag_np = np.ones(n, dtype=np.uint8)
    ver_np = np.arange(nc, dtype=np.uint32)
    ctpl_np = np.zeros(nc, dtype=np.uint16)
    alt_np = (np.arange(n, dtype=np.int64) % NT).astype(np.uint8)

    rng = np.random.default_rng(0x5151)
    heads = rng.integers(0, 256, (NT, HEAD), dtype=np.uint8)
    tails = rng.integers(0, 256, (NT, TAIL), dtype=np.uint8)
    var_np = rng.integers(0, 256, (n, HOLE), dtype=np.uint8)
    msg_np = np.ascontiguousarray(np.concatenate([heads[alt_np], var_np, tails[alt_np]], axis=1)).reshape(-1)
    voff_np = (np.arange(n + 1, dtype=np.int64) * HOLE).astype(np.uint32)
    moff_np = (np.arange(n + 1, dtype=np.int64) * MSG).astype(np.uint64)
    T = pkg.batch.Templates([h.tobytes() for h in heads], [t.tobytes() for t in tails])
    ts, ts_keep = T.struct()

    d_msg = torch.from_numpy(msg_np).to(dev)
    d_off = torch.from_numpy(moff_np.astype(np.int64)).to(dev)
    seeds = bench.chacha_device(pkg, eng, torch, bytes([0x11]) * 32, 0, (per * 32 + 63) // 64, dev)[: per * 32]
    kidx = (torch.arange(0, n, dtype=torch.int64, device=dev) % per).to(torch.int32)
    d_vk = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_sig = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    eng._check(lib.edc_sign_device(eng.ctx, n, vp(seeds), vp(kidx), vp(d_msg), vp(d_off), vp(d_vk), vp(d_sig)))
    torch.cuda.synchronize()
    h_vk, h_sig = d_vk.cpu().numpy(), d_sig.cpu().numpy()
    k_np = np.zeros(n * 32, dtype=np.uint8)
    eng._check(lib.edc_challenge(eng.ctx, n, cp(h_vk), cp(h_sig), cp(msg_np), cp(moff_np, u64p), cp(k_np)))
    idx_np = kidx.cpu().numpy().astype(np.uint32)
    pw_np = np.ones(n, dtype=np.uint64)                          # the join a caller of edc_tmpl_quorum_verify does itself

    eng.keycache_load([h_vk[32 * p: 32 * p + 32].tobytes() for p in range(per)])
    nv = nc - 1
    upd_off = (np.arange(nv + 1, dtype=np.int64) * args.updates).astype(np.uint32)
    upd_pos = (np.arange(nv * args.updates, dtype=np.int64) % per).astype(np.uint32)
    upd_pw = np.ones(max(nv * args.updates, 1), dtype=np.uint64)
    eng._check(lib.edc_vhist_set(eng.ctx, per, cp(np.ones(per, dtype=np.uint64), u64p), nv, cp(upd_off, u32p), cp(upd_pos, u32p),
                                 cp(upd_pw, u64p)))
    eng.sigcache_create(4 * n)
    eng._check(lib.edc_reserve(eng.ctx, n))

    zseed = bytes([0x33]) * 32
    nbad, nchk, nmiss = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    tally = (ctypes.c_uint64 * nc)()
    cv = ctypes.create_string_buffer(nc)
    c8 = {}

    def request(tmpl, cached):
        rq = pkg.EdcVqRequest(size=ctypes.sizeof(pkg.EdcVqRequest), device=0, mode=1, cached=int(cached), nc=nc,
                              commit_off=addr(off_np), commit_ver=addr(ver_np), threshold=addr(thr_np),
                              z_seed=ctypes.cast(zseed, ctypes.c_void_p).value, key_idx=addr(idx_np), sig=addr(h_sig),
                              flag=addr(flag_np))
        if tmpl:
            rq.ts, rq.commit_tpl, rq.alt_span = ctypes.addressof(ts), addr(ctpl_np), NT
            rq.item_alt, rq.var, rq.var_off = addr(alt_np), addr(var_np), addr(voff_np)
        else:
            rq.k = addr(k_np)
        out8 = ctypes.create_string_buffer(32)
        rs = pkg.EdcVqResult(size=ctypes.sizeof(pkg.EdcVqResult), commit_verdicts=ctypes.addressof(cv),
                             tally=ctypes.addressof(tally), n_bad_commits=ctypes.addressof(nbad),
                             n_checked=ctypes.addressof(nchk), n_miss=ctypes.addressof(nmiss), check8=ctypes.addressof(out8))

        def f():
            rc = lib.edc_vq_verify(eng.ctx, ctypes.byref(rq), ctypes.byref(rs))
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            c8[("vq", tmpl, cached)] = out8.raw
        return f

    def vhist(prehashed):
        out8 = ctypes.create_string_buffer(32)

        def f():
            rc = lib.edc_vhist_quorum_verify(eng.ctx, nc, cp(off_np, u32p), cp(ver_np, u32p), None, cp(idx_np, u32p), cp(h_sig),
                                             None if prehashed else cp(msg_np), None if prehashed else cp(moff_np, u64p),
                                             cp(k_np) if prehashed else None, cp(flag_np), cp(thr_np, u64p), 1, zseed, cv, None,
                                             tally, ctypes.byref(nbad), ctypes.byref(nchk), out8)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            c8[("vhist", prehashed)] = out8.raw
        return f

    def tmpl_joined():
        out8 = ctypes.create_string_buffer(32)

        def f():
            rc = lib.edc_tmpl_quorum_verify(eng.ctx, ctypes.byref(ts), nc, cp(off_np, u32p), cp(ctpl_np, u16p), NT, cp(alt_np),
                                            None, cp(idx_np, u32p), cp(h_sig), cp(var_np), cp(voff_np, u32p), cp(pw_np, u64p),
                                            cp(flag_np), cp(thr_np, u64p), 1, zseed, cv, None, tally, ctypes.byref(nbad),
                                            ctypes.byref(nchk), out8)
            assert rc == 0 and nbad.value == 0, (rc, lib.edc_last_error(eng.ctx))
            c8["tmpl"] = out8.raw
        return f

    def cold(f):
        def g():
            eng.sigcache_clear()
            f()
            assert nmiss.value == nchk.value
        return g

    def warm(f):
        def g():
            f()
            assert nmiss.value == 0
        return g

    calls = {
        "tmpl_request": request(True, False), "tmpl_vhist_messages": vhist(False), "tmpl_quorum_host_joined": tmpl_joined(),
        "k_request": request(False, False), "k_vhist": vhist(True),
        # each cold call is followed by its warm twin, which finds what the cold one inserted
        "tmpl_cached_hit0": cold(request(True, True)), "tmpl_cached_hit1": warm(request(True, True)),
        "k_cached_hit0": cold(request(False, True)), "k_cached_hit1": warm(request(False, True)),
    }
    ms = {k: [] for k in calls}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    # the same list was verified by the request and by what it replaces
    assert c8[("vq", True, False)] == c8[("vhist", False)] == c8["tmpl"] and c8[("vq", False, False)] == c8[("vhist", True)]
    last = eng.vq_last()
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    out = {
        "n": n, "validators": per, "commits": nc, "templates": NT, "hole_bytes": HOLE, "msg_bytes": MSG, "reps": args.reps,
        "versions": nc, "checked": nchk.value, "last_request": list(last),
        "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "max_ms": {k: round(max(v), 3) for k, v in ms.items()},
        "tmpl_request_over_vhist_messages": round(med["tmpl_request"] / med["tmpl_vhist_messages"], 4),
        "tmpl_request_minus_host_joined_ms": round(med["tmpl_request"] - med["tmpl_quorum_host_joined"], 3),
        "k_request_over_vhist": round(med["k_request"] / med["k_vhist"], 4),
    }
    print(json.dumps(out), flush=True)
    del ts_keep
    eng.close()


if __name__ == "__main__":
    main()
