"""Trusting pairs (include/edc.h, trust_ver / trust_threshold of edc_vq_verify) against the same commits
listed twice in one request of the form without them, in one run.

The votes of tools/vq_bench.py (2^20 votes from 150 validators, 6,991 commits of 150, power 1 each,
every vote a commit vote, every commit at its own version; 4 templates with a 12-byte hole). Side A:
threshold floor(2T/3) at the commit's own version. Side B: floor(T'/3) at the version --back versions
earlier (the first commits at version 0). Light mode. A pair is timed against ONE request that lists
every commit twice, once per side (2n votes, 2nc commits): how the same question is asked without the
pair. Alternated inside one run, medians of --reps timings with min-max:
  tmpl    templated host request by key index
  k       prehashed host request by key index
  dev     device-resident prehashed request (key bytes)
Then, through the reps hooks, the paired join / selection / double-vote scans
(edc_debug_vq_trust_select) against edc_debug_vhist_select, which times one side's join and scan.

  python tools/vq_trust_bench.py [--n 1048576] [--reps 20]
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
    ap.add_argument("--back", type=int, default=3, help="how many versions back the trusted set lies")
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
    u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

    nc = (n + per - 1) // per
    off_np = np.minimum(np.arange(nc + 1, dtype=np.int64) * per, n).astype(np.uint32)
    sizes = np.diff(off_np.astype(np.int64))
    thr_np = (2 * sizes // 3).astype(np.uint64)
    tthr_np = (sizes // 3).astype(np.uint64)
    flag_np = np.ones(n, dtype=np.uint8)
    ver_np = np.arange(nc, dtype=np.uint32)
    tver_np = np.maximum(np.arange(nc, dtype=np.int64) - args.back, 0).astype(np.uint32)
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

    eng.keycache_load([h_vk[32 * p: 32 * p + 32].tobytes() for p in range(per)])
    nv = nc - 1
    upd_off = (np.arange(nv + 1, dtype=np.int64) * args.updates).astype(np.uint32)
    upd_pos = (np.arange(nv * args.updates, dtype=np.int64) % per).astype(np.uint32)
    upd_pw = np.ones(max(nv * args.updates, 1), dtype=np.uint64)
    eng._check(lib.edc_vhist_set(eng.ctx, per, cp(np.ones(per, dtype=np.uint64), u64p), nv, cp(upd_off, u32p), cp(upd_pos, u32p),
                                 cp(upd_pw, u64p)))
    eng._check(lib.edc_reserve(eng.ctx, 2 * n))

    # every commit listed twice: side A's nc commits, then side B's
    twice = lambda a: np.ascontiguousarray(np.concatenate([a, a]))
    off2 = np.concatenate([off_np.astype(np.int64), n + off_np[1:].astype(np.int64)]).astype(np.uint32)
    ver2, thr2 = np.concatenate([ver_np, tver_np]), np.concatenate([thr_np, tthr_np])
    idx2, sig2, flag2, k2, alt2, var2 = (twice(a) for a in (idx_np, h_sig, flag_np, k_np, alt_np, var_np))
    voff2 = (np.arange(2 * n + 1, dtype=np.int64) * HOLE).astype(np.uint32)
    ctpl2 = twice(ctpl_np)
    d_k = torch.from_numpy(k_np).to(dev)
    d_flag = torch.from_numpy(flag_np).to(dev)
    d_vk2, d_sig2, d_k2, d_flag2 = (torch.cat([t, t]) for t in (d_vk, d_sig, d_k, d_flag))
    torch.cuda.synchronize()

    zseed = bytes([0x33]) * 32
    nbad, nbt, nchk = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    tally, ttally = (ctypes.c_uint64 * (2 * nc))(), (ctypes.c_uint64 * nc)()
    cv, tv = ctypes.create_string_buffer(2 * nc), ctypes.create_string_buffer(nc)
    checked = {}

    def request(form, pair):
        a = (off_np, ver_np, thr_np, idx_np, h_sig, flag_np, k_np, alt_np, var_np, voff_np, ctpl_np, d_vk, d_sig, d_k, d_flag)
        b = (off2, ver2, thr2, idx2, sig2, flag2, k2, alt2, var2, voff2, ctpl2, d_vk2, d_sig2, d_k2, d_flag2)
        off, ver, thr, idx, sig, flag, k, alt, var, voff, ctpl, dvk, dsig, dk, dflag = a if pair else b
        rq = pkg.EdcVqRequest(size=ctypes.sizeof(pkg.EdcVqRequest), device=int(form == "dev"), mode=1, nc=len(off) - 1,
                              commit_off=addr(off), commit_ver=addr(ver), threshold=addr(thr),
                              z_seed=ctypes.cast(zseed, ctypes.c_void_p).value)
        if form == "dev":
            rq.vk, rq.sig, rq.flag, rq.k = dvk.data_ptr(), dsig.data_ptr(), dflag.data_ptr(), dk.data_ptr()
        else:
            rq.key_idx, rq.sig, rq.flag = addr(idx), addr(sig), addr(flag)
            if form == "tmpl":
                rq.ts, rq.commit_tpl, rq.alt_span = ctypes.addressof(ts), addr(ctpl), NT
                rq.item_alt, rq.var, rq.var_off = addr(alt), addr(var), addr(voff)
            else:
                rq.k = addr(k)
        if pair:
            rq.trust_ver, rq.trust_threshold = addr(tver_np), addr(tthr_np)
        rs = pkg.EdcVqResult(size=ctypes.sizeof(pkg.EdcVqResult), commit_verdicts=ctypes.addressof(cv),
                             tally=ctypes.addressof(tally), n_bad_commits=ctypes.addressof(nbad),
                             n_checked=ctypes.addressof(nchk), trust_verdicts=ctypes.addressof(tv),
                             trust_tally=ctypes.addressof(ttally), n_bad_trust=ctypes.addressof(nbt))

        def f():
            rc = lib.edc_vq_verify(eng.ctx, ctypes.byref(rq), ctypes.byref(rs))
            assert rc == 0 and nbad.value == 0 and (not pair or nbt.value == 0), (rc, lib.edc_last_error(eng.ctx))
            checked[(form, pair)] = nchk.value
        return f

    calls = {"%s_%s" % (form, "pair" if pair else "twice"): request(form, pair)
             for form in ("tmpl", "k", "dev") for pair in (True, False)}
    ms = {k: [] for k in calls}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    for _ in range(args.reps):                       # alternate, so drift hits every entry alike
        for name, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    calls["k_pair"]()
    last = eng.vq_trust_last()
    # the kernels alone: the paired stages against one side's join and scan, which a listing twice runs twice
    hook = dict(light=True, key_idx=idx_np.tolist(), reps=args.reps)
    sel = eng.vq_trust_select_ms(off_np.tolist(), ver_np.tolist(), tver_np.tolist(), flag_np.tolist(), thr_np.tolist(),
                                 tthr_np.tolist(), **hook)
    one_a = eng.vhist_select_ms(off_np.tolist(), ver_np.tolist(), flag_np.tolist(), thr_np.tolist(), **hook)
    one_b = eng.vhist_select_ms(off_np.tolist(), tver_np.tolist(), flag_np.tolist(), tthr_np.tolist(), **hook)
    one_sel = eng.quorum_select_ms(off_np.tolist(), [1] * n, flag_np.tolist(), thr_np.tolist(), light=True, reps=args.reps)
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    out = {
        "n": n, "validators": per, "commits": nc, "versions": nc, "back": args.back, "reps": args.reps,
        "checked": {"%s_%s" % (f, "pair" if p else "twice"): v for (f, p), v in checked.items()},
        "pair_counts_a_b_both_union": list(last),
        "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
        "max_ms": {k: round(max(v), 3) for k, v in ms.items()},
        "pair_over_twice": {f: round(med[f + "_pair"] / med[f + "_twice"], 4) for f in ("tmpl", "k", "dev")},
        "kernels_us": {"paired_join": round(sel[0] * 1e3, 1), "paired_selection_union_scan": round(sel[1] * 1e3, 1),
                       "paired_double_vote_scans": round(sel[2] * 1e3, 1),
                       "one_side_join_a_b": [round(one_a[0] * 1e3, 1), round(one_b[0] * 1e3, 1)],
                       "one_side_double_vote_scan_a_b": [round(one_a[1] * 1e3, 1), round(one_b[1] * 1e3, 1)],
                       "one_side_selection": round(one_sel * 1e3, 1)},
    }
    print(json.dumps(out), flush=True)
    del ts_keep
    eng.close()


if __name__ == "__main__":
    main()
