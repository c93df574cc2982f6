"""GPU: commit sets (include/edc.h, edc_commits_* / edc_tmpl_commits_*): many variable-size batches
in one launch, each commit its own batch::Verifier (reference src/batch.rs:110-217) with its own
verdict, and Item::verify_single's code (src/batch.rs:104-107) per item when the launch fails.

Every expectation is the oracle's (tests/golden/commits.json, made by gen_commits.py) or an existing
entry run on one commit alone (edc_batch_verify_device); never another commit-set call. The items
are laid down by gen_commits.py's rules and signed here on the GPU; Ed25519 signing is
deterministic, and the file holds the SHA-256 of the oracle's signatures, so the bytes that are
verified here are the bytes the oracle judged."""
import ctypes
import hashlib
import importlib.util
import os
import random

import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

L_ORDER = 2**252 + 27742317777372353535851937790883648493


def _gen():
    spec = importlib.util.spec_from_file_location("gen_commits", os.path.join(GOLDEN, "gen_commits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class CommitSet:
    def __init__(self, name, engine, oracle, gen, fx):
        b, s = gen.build(name), fx["sets"][name]
        self.name, self.off, self.commit_tpl = name, b["commit_off"], b["commit_tpl"]
        self.tpl, self.holes, self.msgs = b["tpl"], b["holes"], b["msgs"]
        self.nc, self.n = len(self.off) - 1, len(self.msgs)
        vks, sigs = engine.sign(gen.key_seeds(), self.msgs, seed_index=[j or 0 for j in b["validator"]])
        vks, sigs = list(vks), list(sigs)
        if b["corpus_commit"] is not None:
            for d, (vk, sig) in enumerate(gen.corpus()):
                vks[self.off[b["corpus_commit"]] + d], sigs[self.off[b["corpus_commit"]] + d] = vk, sig
        assert hashlib.sha256(b"".join(sigs)).hexdigest() == s["sig_sha256"], "not the signatures the oracle judged"
        for o in s["overrides"]:
            vks[o["item"]], sigs[o["item"]] = bytes.fromhex(o["vk"]), bytes.fromhex(o["sig"])
        self.vks, self.sigs = vks, sigs
        self.ks = [oracle.challenge(sg[:32], vk, m).to_bytes(32, "little") for vk, sg, m in zip(vks, sigs, self.msgs)]
        assert hashlib.sha256(b"".join(self.ks)).hexdigest() == s["k_sha256"]
        self.codes = [0] * self.n
        for i, c in s["item_codes"].items():
            self.codes[int(i)] = c
        self.verdicts, self.n_bad = s["commit_verdicts"], s["n_bad_commits"]
        self.expect = (1 if self.n_bad else 0, self.verdicts, self.codes, self.n_bad)
        self._dev = None
        self._alone = None

    def dev(self):
        """(d_vk, d_sig, d_msg, d_off, d_k) torch tensors, made once."""
        if self._dev is None:
            import torch
            d = torch.device("cuda:0")

            def up(b):
                return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(d)
            offs = [0]
            for m in self.msgs:
                offs.append(offs[-1] + len(m))
            self._dev = (up(b"".join(self.vks)), up(b"".join(self.sigs)), up(b"".join(self.msgs)),
                         torch.tensor(offs, dtype=torch.int64, device=d), up(b"".join(self.ks)))
            torch.cuda.synchronize()
        return self._dev

    def alone(self, engine):
        """edc_batch_verify_device of every non-empty commit on its own (fresh seed each)."""
        if self._alone is None:
            d_vk, d_sig, d_msg, d_off, _ = self.dev()
            rnd = random.Random(self.name)
            self._alone = []
            for a, e in zip(self.off, self.off[1:]):
                if a == e:
                    self._alone.append(None)
                    continue
                rc = engine.lib.edc_batch_verify_device(engine.ctx, e - a, d_vk.data_ptr() + 32 * a,
                                                        d_sig.data_ptr() + 64 * a, d_msg.data_ptr(),
                                                        d_off.data_ptr() + 8 * a, rnd.randbytes(32), 0, None, None)
                assert rc in (0, 1), engine.lib.edc_last_error(engine.ctx)
                self._alone.append(rc)
        return self._alone


@pytest.fixture(scope="module")
def sets(engine, oracle):
    pytest.importorskip("torch")
    gen, fx = _gen(), golden("commits.json")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CommitSet(name, engine, oracle, gen, fx)
        return cache[name]
    get.templates = lambda edc: edc.batch.Templates(*gen.templates())
    return get


def _device(engine, S, seed, prehashed=False):
    d_vk, d_sig, d_msg, d_off, d_k = S.dev()
    if prehashed:
        return engine.commits_verify_device(S.off, d_vk.data_ptr(), d_sig.data_ptr(), None, None, seed, d_k=d_k.data_ptr())
    return engine.commits_verify_device(S.off, d_vk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(), seed)


def _agrees_alone(engine, S):
    for c, rc in enumerate(S.alone(engine)):
        if rc is None:
            assert S.verdicts[c] == 0, c            # an empty Verifier verifies
        else:
            assert rc == S.verdicts[c], (S.name, c)


def test_all_valid(engine, sets):
    S = sets("valid")
    assert [e - a for a, e in zip(S.off, S.off[1:])] == [0, 1, 150, 7, 2049, 0]
    rc, verdicts, codes, n_bad = _device(engine, S, random.Random(1).randbytes(32))
    assert (rc, verdicts, n_bad) == (0, [0] * 6, 0) and codes == [0] * S.n
    assert S.expect == (0, [0] * 6, [0] * S.n, 0)
    assert _device(engine, S, random.Random(2).randbytes(32), prehashed=True) == S.expect
    _agrees_alone(engine, S)


@pytest.mark.parametrize("name", ["mixed_a", "mixed_b"])
def test_mixed(engine, sets, name):
    S = sets(name)
    assert 4096 < S.n < 4400                        # the fallback cuts at items 2048 and 4096
    got = _device(engine, S, random.Random(name).randbytes(32))
    assert got[0] == 1 and got[3] == S.n_bad == 5
    assert got[1] == S.verdicts
    assert [(i, c) for i, c in enumerate(got[2]) if c] == [(i, c) for i, c in enumerate(S.codes) if c]
    assert got == S.expect
    c20 = S.off.index(2040)                         # the 20-item commit across item 2048 and its neighbours
    assert got[1][c20 - 1:c20 + 2] == [0, 1, 0]
    _agrees_alone(engine, S)


@pytest.mark.parametrize("name", ["mixed_a", "mixed_b"])
def test_forms_agree_with_the_device_form(engine, edc, sets, name):
    S = sets(name)
    rnd = random.Random("forms" + name)
    dev = _device(engine, S, rnd.randbytes(32))
    assert dev == S.expect
    assert _device(engine, S, rnd.randbytes(32), prehashed=True) == dev
    assert engine.commits_verify(S.off, S.sigs, rnd.randbytes(32), vks=S.vks, msgs=S.msgs) == dev
    assert engine.commits_verify(S.off, S.sigs, rnd.randbytes(32), vks=S.vks, ks=S.ks) == dev
    t = sets.templates(edc)
    assert t.count == 4 and t.materialize(S.tpl, S.holes) == S.msgs and {len(h) for h in S.holes} == {12}
    assert engine.commits_verify_templated(t, S.off, S.commit_tpl, S.sigs, S.holes, rnd.randbytes(32), vks=S.vks) == dev
    # asynchronous forms, one at a time
    d_vk, d_sig, d_msg, d_off, d_k = S.dev()
    tk = engine.commits_submit(S.off, S.sigs, rnd.randbytes(32), vks=S.vks, msgs=S.msgs)
    assert engine.commits_wait(tk) == dev
    tk = engine.commits_submit(S.off, S.sigs, rnd.randbytes(32), vks=S.vks, ks=S.ks)
    assert engine.commits_wait(tk) == dev
    tk = engine.commits_submit_templated(t, S.off, S.commit_tpl, S.sigs, S.holes, rnd.randbytes(32), vks=S.vks)
    assert engine.commits_wait(tk) == dev
    tk = engine.commits_submit_device(S.off, d_vk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(),
                                      rnd.randbytes(32))
    assert engine.commits_wait(tk) == dev
    tk = engine.commits_submit_device(S.off, d_vk.data_ptr(), d_sig.data_ptr(), None, None, rnd.randbytes(32),
                                      d_k=d_k.data_ptr())
    assert engine.commits_wait(tk) == dev
    # keys as positions in the registered list (an undecodable registered key stays malformed)
    keys = list(dict.fromkeys(S.vks))
    pos = {k: i for i, k in enumerate(keys)}
    idx = [pos[k] for k in S.vks]
    engine.keycache_load(keys)
    try:
        assert engine.commits_verify(S.off, S.sigs, rnd.randbytes(32), key_idx=idx, msgs=S.msgs) == dev
        assert engine.commits_verify(S.off, S.sigs, rnd.randbytes(32), key_idx=idx, ks=S.ks) == dev
        assert engine.commits_verify_templated(t, S.off, S.commit_tpl, S.sigs, S.holes, rnd.randbytes(32),
                                               key_idx=idx) == dev
        tk = engine.commits_submit(S.off, S.sigs, rnd.randbytes(32), key_idx=idx, msgs=S.msgs)
        assert engine.commits_wait(tk) == dev
        tk = engine.commits_submit_templated(t, S.off, S.commit_tpl, S.sigs, S.holes, rnd.randbytes(32), key_idx=idx)
        assert engine.commits_wait(tk) == dev
        assert _device(engine, S, rnd.randbytes(32)) == dev       # the device form with the cache loaded
    finally:
        engine.keycache_clear()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_independent_of_the_key_grouping(engine, sets, mode):
    A, V = sets("mixed_a"), sets("valid")
    engine.set_key_grouping(mode)
    try:
        assert _device(engine, A, random.Random(mode).randbytes(32)) == A.expect
        assert _device(engine, V, random.Random(mode + 10).randbytes(32)) == V.expect
        tk = engine.commits_submit(A.off, A.sigs, random.Random(mode + 20).randbytes(32), vks=A.vks, msgs=A.msgs)
        assert engine.commits_wait(tk) == A.expect
    finally:
        engine.set_key_grouping(0)


def test_streaming_tickets_keep_their_results(engine, edc, sets):
    V, A, M = sets("valid"), sets("mixed_a"), sets("tmap_small")
    lib, ctx = engine.lib, engine.ctx
    rnd = random.Random("stream")
    t = sets.templates(edc)
    good = slice(V.off[2], V.off[3])                # a valid commit of 150
    bad = slice(A.off[4], A.off[5])                 # the commit whose first signature is corrupted
    assert A.verdicts[4] == 1 and V.verdicts[2] == 0
    d_vk, d_sig, d_msg, d_off, _ = A.dev()
    t0 = engine.commits_submit(V.off, V.sigs, rnd.randbytes(32), vks=V.vks, msgs=V.msgs)               # passes
    t1 = engine.batch_submit(V.vks[good], V.sigs[good], V.msgs[good], rnd.randbytes(32))
    t2 = engine.commits_submit_device(A.off, d_vk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(), d_off.data_ptr(),
                                      rnd.randbytes(32))                                               # fails
    t3 = engine.batch_submit(A.vks[bad], A.sigs[bad], A.msgs[bad], rnd.randbytes(32))
    t4 = engine.commits_submit_templated(t, M.off, M.commit_tpl, M.sigs, M.holes, rnd.randbytes(32), vks=M.vks)  # passes
    assert [t1 - t0, t2 - t0, t3 - t0, t4 - t0] == [1, 2, 3, 4]
    # cross-waiting is refused and leaves the ticket pending
    cv, iv, nb = ctypes.create_string_buffer(V.nc), ctypes.create_string_buffer(V.n), ctypes.c_int(-1)
    vd = (ctypes.c_int * 1)()
    assert lib.edc_batch_wait(ctx, t0, None, None, None) == -2
    assert lib.edc_batch_wait_multi(ctx, t0, 1, vd, None, None, None) == -2
    assert lib.edc_commits_wait(ctx, t1, cv, iv, ctypes.byref(nb)) == -2
    assert engine.commits_wait(t0) == V.expect
    assert engine.batch_wait(t1)[0] == 0
    assert engine.commits_wait(t2) == A.expect      # the fallback runs on slot 2 with t3 and t4 in flight
    assert engine.batch_wait(t3)[0] == 1
    assert engine.commits_wait(t4) == M.expect
    assert lib.edc_commits_wait(ctx, t4, cv, iv, ctypes.byref(nb)) == -2      # already waited
    t5 = engine.commits_submit(V.off, V.sigs, rnd.randbytes(32), vks=V.vks, ks=V.ks)
    assert engine.commits_wait(t5) == V.expect
    assert _device(engine, V, rnd.randbytes(32)) == V.expect                   # slot 0 is free again


def test_one_commit_is_the_streamed_fallback(engine, sets):
    """nc = 1: a streamed batch that fails gets its per-item codes at the wait."""
    A = sets("mixed_a")
    a, e = A.off[4], A.off[6]                       # two bad commits as one
    tk = engine.commits_submit([0, e - a], A.sigs[a:e], random.Random(5).randbytes(32), vks=A.vks[a:e], msgs=A.msgs[a:e])
    assert engine.commits_wait(tk) == (1, [1], A.codes[a:e], 1)
    assert sum(1 for c in A.codes[a:e] if c) == 2


def test_argument_checks_leave_the_context_usable(engine, edc, sets):
    V = sets("valid")
    lib, ctx = engine.lib, engine.ctx
    engine.keycache_clear()                         # "no registered list" below means none
    n = 8
    vk, sig = b"".join(V.vks[:n]), b"".join(V.sigs[:n])
    msgs, ks, holes = V.msgs[:n], b"".join(V.ks[:n]), V.holes[:n]
    arena, moff = b"".join(msgs), (ctypes.c_uint64 * (n + 1))(*[sum(len(m) for m in msgs[:i]) for i in range(n + 1)])
    var, voff = b"".join(holes), (ctypes.c_uint32 * (n + 1))(*[12 * i for i in range(n + 1)])
    sizes = [1, 7]                                  # items 0..7 of the set: commit 1 and the head of commit 2
    assert V.tpl[:n] == [1] + [2] * 7
    good_off = (ctypes.c_uint32 * 3)(0, 1, 8)
    good_tpl = (ctypes.c_uint16 * 2)(1, 2)
    ts, _keep = sets.templates(edc).struct()
    seed = bytes(range(32))
    idx = (ctypes.c_uint32 * n)(*range(n))
    cv, iv, nb = ctypes.create_string_buffer(2), ctypes.create_string_buffer(n), ctypes.c_int(-1)
    out = (cv, iv, ctypes.byref(nb))

    def u32(*v):
        return (ctypes.c_uint32 * len(v))(*v)

    def usable():
        nb.value = -1
        assert lib.edc_commits_verify(ctx, 2, good_off, vk, None, sig, arena, moff, None, seed, *out) == 0
        assert (cv.raw, iv.raw, nb.value) == (bytes(2), bytes(n), 0)
        assert lib.edc_tmpl_commits_verify(ctx, ctypes.byref(ts), 2, good_off, good_tpl, vk, None, sig, var, voff, seed,
                                           *out) == 0

    usable()
    assert sum(sizes) == n
    bad_k = ks[:32 * 3] + L_ORDER.to_bytes(32, "little") + ks[32 * 4:]
    bad_voff = (ctypes.c_uint32 * (n + 1))(*[0, 12, 11] + [12 * i for i in range(3, n + 1)])
    voff1 = (ctypes.c_uint32 * (n + 1))(*[1] + [12 * i for i in range(1, n + 1)])
    none_ts = edc.EdcTemplates(0, ts.head, ts.head_off, ts.tail, ts.tail_off)
    host = lambda off, *a: lib.edc_commits_verify(ctx, len(off) - 1, off, *a, seed, *out)          # noqa: E731
    tmpl = lambda tsx, off, ctpl, *a: lib.edc_tmpl_commits_verify(ctx, ctypes.byref(tsx), len(off) - 1, off, ctpl, *a,
                                                                  seed, *out)                        # noqa: E731
    refusals = [
        lambda: host(u32(1, 1, 8), vk, None, sig, arena, moff, None),                 # commit_off[0] != 0
        lambda: host(u32(0, 9, 8), vk, None, sig, arena, moff, None),                 # a decreasing offset
        lambda: host(u32(0, 1, 1 << 28), vk, None, sig, arena, moff, None),           # n >= 2^28
        lambda: host(good_off, vk, idx, sig, arena, moff, None),                      # both vk and key_idx
        lambda: host(good_off, None, None, sig, arena, moff, None),                   # neither
        lambda: host(good_off, vk, None, sig, arena, moff, ks),                       # both messages and k
        lambda: host(good_off, vk, None, sig, None, None, None),                      # neither
        lambda: host(good_off, None, idx, sig, arena, moff, None),                    # no registered key list
        lambda: host(good_off, vk, None, sig, None, None, bad_k),                     # a prehashed k = l
        lambda: lib.edc_commits_verify(ctx, 2, good_off, vk, None, sig, arena, moff, None, None, *out),   # no seed
        lambda: tmpl(ts, good_off, (ctypes.c_uint16 * 2)(1, 4), vk, None, sig, var, voff),    # commit_tpl[c] = count
        lambda: tmpl(none_ts, good_off, good_tpl, vk, None, sig, var, voff),                  # a refused template set
        lambda: tmpl(ts, good_off, good_tpl, vk, None, sig, var, bad_voff),                   # decreasing hole offsets
        lambda: tmpl(ts, good_off, good_tpl, vk, None, sig, var, voff1),                      # var_off[0] != 0
        lambda: tmpl(ts, good_off, good_tpl, vk, idx, sig, var, voff),                        # both vk and key_idx
        lambda: tmpl(ts, u32(0, 1, 1 << 28), good_tpl, vk, None, sig, var, voff),
        lambda: lib.edc_commits_verify_device(ctx, 2, u32(0, 5, 4), None, None, None, None, None, seed, *out),
        lambda: lib.edc_commits_verify_device(ctx, 1, u32(0, 1 << 28), None, None, None, None, None, seed, *out),
        lambda: lib.edc_commits_submit(ctx, 2, u32(0, 9, 8), vk, None, sig, arena, moff, None, seed),
        lambda: lib.edc_commits_submit(ctx, 2, good_off, vk, None, sig, None, None, bad_k, seed),
        lambda: lib.edc_tmpl_commits_submit(ctx, ctypes.byref(ts), 2, good_off, (ctypes.c_uint16 * 2)(4, 0), vk, None,
                                            sig, var, voff, seed),
        lambda: lib.edc_commits_submit_device(ctx, 2, u32(2, 5, 8), None, None, None, None, None, seed),
    ]
    for i, refuse in enumerate(refusals):
        assert refuse() == -2, i
        usable()
    # a key index outside a registered list
    engine.keycache_load(V.vks[:n])
    try:
        assert host(good_off, None, u32(0, 1, 2, 3, 4, 5, 6, 8), sig, arena, moff, None) == -2
        usable()
        assert host(good_off, None, idx, sig, arena, moff, None) == 0
    finally:
        engine.keycache_clear()
    # nc = 0 is not an error: nothing to verify
    nb.value = -1
    assert lib.edc_commits_verify(ctx, 0, None, None, None, None, None, None, None, seed, None, None, ctypes.byref(nb)) == 0
    assert nb.value == 0
    assert lib.edc_commits_verify_device(ctx, 0, None, None, None, None, None, None, seed, None, None, None) == 0
    assert engine.commits_verify([0, 0, 0], [], seed, vks=[], msgs=[]) == (0, [0, 0], [], 0)      # only empty commits
    tk = engine.commits_submit([0], [], seed, vks=[], msgs=[])
    assert engine.commits_wait(tk) == (0, [], [], 0)
    usable()


@pytest.mark.parametrize("name", ["tmap_small", "tmap_big"])
def test_template_map(engine, edc, oracle, sets, name):
    """The commit-to-item template map: commits far smaller than a workgroup's items (sizes 0..5,
    empty first and last commit) and one commit over many workgroups."""
    S = sets(name)
    t = sets.templates(edc)
    sizes = [e - a for a, e in zip(S.off, S.off[1:])]
    if name == "tmap_small":
        assert S.nc == 600 and set(sizes) == set(range(6)) and sizes[0] == sizes[-1] == 0
    else:
        assert sizes == [3000]
    assert engine.commits_verify_templated(t, S.off, S.commit_tpl, S.sigs, S.holes, random.Random(name).randbytes(32),
                                           vks=S.vks) == S.expect == (0, [0] * S.nc, [0] * S.n, 0)
    # the messages the map must lead to: k of the materialised messages is the oracle's
    msgs = t.materialize(S.tpl, S.holes)
    assert msgs == S.msgs
    assert engine.tmpl_challenge(t, S.vks, S.sigs, S.tpl, S.holes) == S.ks
    # the kernel alone
    off = (ctypes.c_uint32 * (S.nc + 1))(*S.off)
    ctpl = (ctypes.c_uint16 * S.nc)(*S.commit_tpl)
    got = (ctypes.c_uint16 * S.n)()
    assert engine.lib.edc_debug_tmpl_commit_map(engine.ctx, S.nc, off, ctpl, got, 1, None) == 0
    assert list(got) == S.tpl
    # a commit given another template fails, alone: the oracle on the messages that template gives
    c = max(range(S.nc), key=lambda j: (min(sizes[j], 3), j))
    wrong = list(S.commit_tpl)
    wrong[c] = (wrong[c] + 1) % 4
    a, e = S.off[c], min(S.off[c + 1], S.off[c] + 3)       # the oracle judges the commit's first items
    assert e - a == 3
    wmsgs = t.materialize([wrong[c]] * (e - a), S.holes[a:e])
    wcodes = [oracle.verify(vk, sg, m) for vk, sg, m in zip(S.vks[a:e], S.sigs[a:e], wmsgs)]
    assert wcodes == [1] * (e - a)
    rc, verdicts, codes, n_bad = engine.commits_verify_templated(t, S.off, wrong, S.sigs, S.holes,
                                                                 random.Random(name + "w").randbytes(32), vks=S.vks)
    assert (rc, n_bad) == (1, 1) and verdicts == [1 if j == c else 0 for j in range(S.nc)]
    assert codes[a:e] == wcodes and not any(codes[:S.off[c]]) and not any(codes[S.off[c + 1]:])


def test_verify_many(engine, edc, sets):
    A = sets("mixed_a")
    vs = []
    for c in range(3, 8):                           # empty, first bad, last bad, bad key, s = l
        v = edc.batch.Verifier(engine)
        for i in range(A.off[c], A.off[c + 1]):
            v.queue((A.vks[i], A.sigs[i], A.msgs[i]))
        vs.append(v)
    pre = edc.batch.Verifier(engine)                # prehashed items
    for i in range(A.off[1], A.off[2]):
        pre.queue(edc.batch.Item.prehashed(A.vks[i], A.sigs[i], A.ks[i]))
    expect = [v == 0 for v in A.verdicts[3:8]]
    assert expect == [True, False, False, False, False]
    assert edc.batch.verify_many(vs, engine=engine) == expect
    assert edc.batch.verify_many(vs + [pre], z_seed=bytes(32)) == expect + [A.verdicts[1] == 0]
    assert edc.batch.verify_many([pre, vs[0]]) == [True, True]
