"""GPU: templated commit sets with per-item template variants (include/edc.h,
edc_tmpl_commits_*_alt), their device-resident forms (edc_tmpl_commits_*_device) and the map kernel
behind them (edc_debug_tmpl_commit_map_alt).

Every expectation is the oracle's (tests/golden/commits_alt.json, made by gen_commits_alt.py), a
map computed here in Python, or an existing entry (edc_commits_verify on the materialised messages,
edc_tmpl_commits_verify, edc_debug_tmpl_commit_map) run with the same seed. The items are laid down
by the generator's rules and signed here on the GPU; Ed25519 signing is deterministic and the file
holds the SHA-256 of the oracle's signatures, so the bytes verified here are the bytes the oracle
judged."""
import ctypes
import hashlib
import importlib.util
import os
import random
import struct

import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

COUNT = 8                                           # templates in the fixture's set


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class AltSet:
    """A signed set of the fixture: host lists, the oracle's expectation, device tensors."""

    def __init__(self, name, engine, gen, fx):
        b, s = gen.build(name), fx["sets"][name]
        self.name, self.off, self.commit_tpl, self.alt = name, b["commit_off"], b["commit_tpl"], b["alt"]
        self.tpl, self.holes, self.msgs = b["tpl"], b["holes"], b["msgs"]
        self.nc, self.n = len(self.off) - 1, len(self.msgs)
        assert hashlib.sha256(b"".join(self.msgs)).hexdigest() == s["msg_sha256"]
        vks, sigs = engine.sign(gen.key_seeds(), self.msgs, seed_index=b["validator"])
        vks, sigs = list(vks), list(sigs)
        assert hashlib.sha256(b"".join(sigs)).hexdigest() == s["sig_sha256"], "not the signatures the oracle judged"
        for o in s["overrides"]:
            vks[o["item"]], sigs[o["item"]] = bytes.fromhex(o["vk"]), bytes.fromhex(o["sig"])
        self.vks, self.sigs = vks, sigs
        self.codes = [0] * self.n
        for i, c in s["item_codes"].items():
            self.codes[int(i)] = c
        self.verdicts, self.n_bad = s["commit_verdicts"], s["n_bad_commits"]
        self.expect = (1 if self.n_bad else 0, self.verdicts, self.codes, self.n_bad)
        self._dev = None

    def dev(self):
        """(d_alt, d_vk, d_sig, d_var, d_var_off, var_bytes): torch tensors, made once."""
        if self._dev is None:
            import torch
            d = torch.device("cuda:0")

            def up(b):
                return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(d)
            voff = [0]
            for h in self.holes:
                voff.append(voff[-1] + len(h))
            self._dev = (up(bytes(self.alt)), up(b"".join(self.vks)), up(b"".join(self.sigs)), up(b"".join(self.holes)),
                         torch.tensor(voff, dtype=torch.int32, device=d), voff[-1])
            torch.cuda.synchronize()
        return self._dev


@pytest.fixture(scope="module")
def alt(engine, edc):
    pytest.importorskip("torch")
    gen, fx = _load("gen_commits_alt"), golden("commits_alt.json")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = AltSet(name, engine, gen, fx)
        return cache[name]
    get.gen, get.fx = gen, fx
    get.templates = edc.batch.Templates(*gen.templates())
    assert get.templates.count == COUNT and fx["alt_span"] == gen.ALT_SPAN == 4
    return get


# ---- 1. the map kernel alone ----

def _placed(nbytes, off):
    """A host buffer and an address in it `off` bytes past a 16-byte boundary (the hook places its
    device copies at the same offsets)."""
    raw = ctypes.create_string_buffer(nbytes + 48)
    return raw, ((ctypes.addressof(raw) + 15) & ~15) + off


def _map_alt(engine, off, ctpl, span, alt_bytes, alt_at=0, out_at=0):
    """(rc, tpl_out as a list, flagged) of edc_debug_tmpl_commit_map_alt."""
    nc, n = len(off) - 1, off[-1]
    c_off = (ctypes.c_uint32 * (nc + 1))(*off)
    c_tpl = (ctypes.c_uint16 * nc)(*ctpl)
    a_raw, a_ptr = _placed(n, alt_at)
    if alt_bytes is not None:
        ctypes.memmove(a_ptr, bytes(alt_bytes), n)
    o_raw, o_ptr = _placed(2 * n, out_at)
    ctypes.memset(o_ptr, 0xEE, 2 * n)
    flagged = ctypes.c_int(-1)
    rc = engine.lib.edc_debug_tmpl_commit_map_alt(engine.ctx, nc, c_off, c_tpl, span, a_ptr if alt_bytes is not None else None,
                                                  o_ptr, ctypes.byref(flagged), 1, None)
    got = list(struct.unpack("<%dH" % n, ctypes.string_at(o_ptr, 2 * n)))
    return rc, got, flagged.value


def _map_sets(gen):
    return ["small"] + ["edge%d" % n for n in gen.EDGE]


@pytest.mark.parametrize("where", [(0, 0), (3, 6), (8, 0), (0, 2), (5, 14)])
def test_map_equals_the_python_map(engine, alt, where):
    """Aligned arrays (the 8-byte load, the 16-byte store) and deliberately odd ones (byte loads,
    2-byte stores), each path alone and together, on every shape of the fixture."""
    gen = alt.gen
    for name in _map_sets(gen):
        b = gen.build(name, messages=False)
        want = [b["commit_tpl"][c] + b["alt"][i] for c, (a, e) in enumerate(zip(b["commit_off"], b["commit_off"][1:]))
                for i in range(a, e)]
        assert want == b["tpl"] and hashlib.sha256(struct.pack("<%dH" % len(want), *want)).hexdigest() == \
            alt.fx["sets"][name]["tpl_sha256"]
        rc, got, flagged = _map_alt(engine, b["commit_off"], b["commit_tpl"], gen.ALT_SPAN, b["alt"], *where)
        assert (rc, flagged) == (0, 0), name
        assert got == want, name


@pytest.mark.parametrize("sizes", [[3000], [5, 3000, 0, 2100], [0, 2047, 4100, 1], [2049, 0, 0, 2047, 6]])
@pytest.mark.parametrize("where", [(0, 0), (3, 6)])
def test_map_with_commits_across_workgroups(engine, sizes, where):
    """Commits that span a 2,048-item workgroup boundary, so that a workgroup's first and last item
    lie in one commit (and the next workgroup starts inside it), against the map computed here."""
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    n = off[-1]
    assert any(a < g < e for a, e in zip(off, off[1:]) for g in range(2048, n, 2048))
    ctpl = [(3 * c) % 5 for c in range(len(sizes))]
    a = [(i * 2654435761 >> 13) % 4 for i in range(n)]
    want = [ctpl[c] + a[i] for c, (lo, hi) in enumerate(zip(off, off[1:])) for i in range(lo, hi)]
    assert _map_alt(engine, off, ctpl, 4, a, *where) == (0, want, 0)
    a[2048] = 4                                     # the first item of the second workgroup, outside the window
    c = max(j for j in range(len(sizes)) if off[j] <= 2048)
    want[2048] = ctpl[c]
    assert _map_alt(engine, off, ctpl, 4, a, *where) == (0, want, 1)


def test_map_shapes_cover_the_lane_and_workgroup_edges(alt):
    gen = alt.gen
    assert gen.MAP_ITEMS == 2048 and sorted(gen.EDGE) == [1, 7, 8, 9, 2047, 2048, 2049, 4100]
    for n, sizes in gen.EDGE.items():
        assert sum(sizes) == n
    offs = {n: gen.build("edge%d" % n, messages=False)["commit_off"] for n in gen.EDGE}
    assert any(o % 8 for o in offs[7]) and any(o % 8 for o in offs[2048]) and 2045 in offs[4100]   # inside a lane
    assert 2048 in offs[2049] and {2048, 4096} <= set(offs[4100])                                   # on a workgroup boundary


@pytest.mark.parametrize("name,item", [("edge8", 7), ("edge2049", 2047), ("edge2049", 2048), ("edge4100", 4095),
                                       ("edge4100", 4099), ("edge7", 6), ("small", 7)])
@pytest.mark.parametrize("alt_at", [0, 3])
def test_map_flags_a_variant_outside_the_window(engine, alt, name, item, alt_at):
    """One byte >= alt_span as the last item of a full lane (item % 8 == 7) and as the tail item of
    the last lane: the flag is up, every written value is below the set's count, the bad item got
    its commit's base and every other item its template."""
    gen = alt.gen
    b = gen.build(name, messages=False)
    n = b["commit_off"][-1]
    assert item % 8 == 7 or (item == n - 1 and n % 8)
    for bad in (gen.ALT_SPAN, 255):
        a = list(b["alt"])
        a[item] = bad
        rc, got, flagged = _map_alt(engine, b["commit_off"], b["commit_tpl"], gen.ALT_SPAN, a, alt_at)
        assert (rc, flagged) == (0, 1)
        assert max(got) < COUNT
        c = max(j for j in range(len(b["sizes"])) if b["commit_off"][j] <= item)
        want = list(b["tpl"])
        want[item] = b["commit_tpl"][c]
        assert got == want
    # the same array with the window as wide as the byte: no flag
    a = list(b["alt"])
    a[item] = gen.ALT_SPAN
    rc, got, flagged = _map_alt(engine, b["commit_off"], [0] * len(b["sizes"]), gen.ALT_SPAN + 1, a, alt_at)
    assert (rc, flagged) == (0, 0) and got == a


def test_map_without_variants_is_the_existing_map(engine, alt):
    gen = alt.gen
    for name in _map_sets(gen):
        b = gen.build(name, messages=False)
        nc, n = len(b["sizes"]), b["commit_off"][-1]
        ctpl = [(5 * c) % COUNT for c in range(nc)]
        old = (ctypes.c_uint16 * n)()
        assert engine.lib.edc_debug_tmpl_commit_map(engine.ctx, nc, (ctypes.c_uint32 * (nc + 1))(*b["commit_off"]),
                                                    (ctypes.c_uint16 * nc)(*ctpl), old, 1, None) == 0
        for at in (0, 6):
            assert _map_alt(engine, b["commit_off"], ctpl, 1, None, 0, at) == (0, list(old), 0), name
        assert _map_alt(engine, b["commit_off"], ctpl, 1, [0] * n) == (0, list(old), 0), name


# ---- 2. alt_span = 1, item_alt = NULL is the one-template call ----

@pytest.mark.parametrize("name", ["valid", "mixed_a", "mixed_b", "tmap_small", "tmap_big"])
def test_span_one_is_the_one_template_call(engine, edc, oracle, name):
    """Every templated set of commits.json; tmap_big is one commit across two workgroups of the map
    and mixed_b has its bad item as the first item of the second workgroup."""
    from test_gpu_commits import CommitSet
    gen = _load("gen_commits")
    S = CommitSet(name, engine, oracle, gen, golden("commits.json"))
    t = edc.batch.Templates(*gen.templates())
    seed = random.Random("compat" + name).randbytes(32)
    old = engine.commits_verify_templated(t, S.off, S.commit_tpl, S.sigs, S.holes, seed, vks=S.vks)
    assert old == S.expect
    assert engine.commits_verify_templated_alt(t, S.off, S.commit_tpl, 1, None, S.sigs, S.holes, seed, vks=S.vks) == old
    assert engine.commits_verify_templated_alt(t, S.off, S.commit_tpl, 1, [0] * S.n, S.sigs, S.holes, seed, vks=S.vks) == old
    tk = engine.commits_submit_templated_alt(t, S.off, S.commit_tpl, 1, None, S.sigs, S.holes, seed, vks=S.vks)
    assert engine.commits_wait(tk) == old


# ---- 3. parity of every form with the fixture and with the materialised messages ----

def _host(engine, alt, S, seed, **keys):
    return engine.commits_verify_templated_alt(alt.templates, S.off, S.commit_tpl, alt.gen.ALT_SPAN, S.alt, S.sigs, S.holes,
                                               seed, **(keys or {"vks": S.vks}))


def _dev_args(alt, S, d_alt=None):
    d = S.dev()
    return (alt.templates, S.off, S.commit_tpl, alt.gen.ALT_SPAN, d[0] if d_alt is None else d_alt) + d[1:]


@pytest.mark.parametrize("name", ["mixed", "edge4100"])
def test_forms_agree_with_the_fixture_and_the_materialised_messages(engine, alt, name):
    S = alt(name)
    T, span = alt.templates, alt.gen.ALT_SPAN
    assert T.materialize(S.tpl, S.holes) == S.msgs and set(S.alt) == {0, 1, 2, 3}
    assert {len(h) for h in S.holes} == {0, 11, 12, 13}
    rnd = random.Random("parity" + name)
    for _ in range(2):
        seed = rnd.randbytes(32)
        plain = engine.commits_verify(S.off, S.sigs, seed, vks=S.vks, msgs=S.msgs)       # the materialised messages
        assert plain == S.expect
        assert _host(engine, alt, S, seed) == plain
        tk = engine.commits_submit_templated_alt(T, S.off, S.commit_tpl, span, S.alt, S.sigs, S.holes, seed, vks=S.vks)
        assert engine.commits_wait(tk) == plain
        assert engine.commits_verify_templated_device(*_dev_args(alt, S), seed) == plain
        tk = engine.commits_submit_templated_device(*_dev_args(alt, S), seed)
        assert engine.commits_wait(tk) == plain
    if name == "edge4100":
        assert S.expect == (0, [0] * S.nc, [0] * S.n, 0)                                 # a passing set: all zeros
    else:
        assert S.expect[0] == 1 and S.n_bad == 4 and sorted(c for c in S.codes if c) == [1, 1, 1, 2]
    # keys as positions in the registered list
    keys = list(dict.fromkeys(S.vks))
    pos = {k: i for i, k in enumerate(keys)}
    idx = [pos[k] for k in S.vks]
    engine.keycache_load(keys)
    try:
        seed = rnd.randbytes(32)
        assert _host(engine, alt, S, seed, key_idx=idx) == S.expect
        tk = engine.commits_submit_templated_alt(T, S.off, S.commit_tpl, span, S.alt, S.sigs, S.holes, seed, key_idx=idx)
        assert engine.commits_wait(tk) == S.expect
        assert engine.commits_verify_templated_device(*_dev_args(alt, S), seed) == S.expect    # with the cache loaded
    finally:
        engine.keycache_clear()


def test_device_arrays_need_no_alignment_for_the_variants(engine, alt):
    """d_item_alt at an odd address, and NULL with every item on variant 0."""
    import torch
    S = alt("mixed")
    d_alt = torch.zeros(S.n + 16, dtype=torch.uint8, device="cuda:0")
    d_alt[3:3 + S.n] = S.dev()[0]
    torch.cuda.synchronize()
    seed = random.Random("odd").randbytes(32)
    assert (d_alt.data_ptr() + 3) % 8 == 3
    assert engine.commits_verify_templated_device(*_dev_args(alt, S, d_alt.data_ptr() + 3), seed) == S.expect
    # NULL: the messages of variant 0 everywhere; only the items signed on variant 0 still verify
    got = engine.commits_verify_templated_device(*_dev_args(alt, S)[:4], None, *S.dev()[1:], seed)
    zero = [i for i, a in enumerate(S.alt) if a == 0]
    assert got[0] == 1 and [got[2][i] for i in zero] == [S.codes[i] for i in zero]
    assert all(got[2][i] for i, a in enumerate(S.alt) if a)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_independent_of_the_key_grouping(engine, alt, mode):
    M, E = alt("mixed"), alt("edge4100")
    engine.set_key_grouping(mode)
    try:
        rnd = random.Random(mode)
        assert _host(engine, alt, M, rnd.randbytes(32)) == M.expect
        assert _host(engine, alt, E, rnd.randbytes(32)) == E.expect
        assert engine.commits_verify_templated_device(*_dev_args(alt, M), rnd.randbytes(32)) == M.expect
        tk = engine.commits_submit_templated_device(*_dev_args(alt, E), rnd.randbytes(32))
        assert engine.commits_wait(tk) == E.expect
    finally:
        engine.set_key_grouping(0)


# ---- 4. streaming ----

def test_streaming_tickets_keep_their_results(engine, alt):
    """Three host _alt tickets (each with its own variant bytes staged in its own slot), one plain
    commit ticket and two device tickets in flight on one context."""
    M, E = alt("mixed"), alt("edge4100")
    T, span = alt.templates, alt.gen.ALT_SPAN
    lib, ctx = engine.lib, engine.ctx
    rnd = random.Random("stream-alt")
    # the mixed set with other variant bytes: item j of a commit that is Ok moves to another variant,
    # so its signature is over another message. The expectation is edc_commits_verify's on the
    # messages those bytes give.
    j = next(a for c, (a, e) in enumerate(zip(M.off, M.off[1:])) if e > a and M.verdicts[c] == 0)
    alt2 = list(M.alt)
    alt2[j] = (alt2[j] + 1) % span
    c2 = max(c for c in range(M.nc) if M.off[c] <= j)
    tpl2 = list(M.tpl)
    tpl2[j] = M.commit_tpl[c2] + alt2[j]
    expect2 = engine.commits_verify(M.off, M.sigs, rnd.randbytes(32), vks=M.vks, msgs=T.materialize(tpl2, M.holes))
    assert expect2[2][j] == 1 and expect2[3] == M.n_bad + 1 and expect2 != M.expect

    def host(S, a):
        return engine.commits_submit_templated_alt(T, S.off, S.commit_tpl, span, a, S.sigs, S.holes, rnd.randbytes(32),
                                                   vks=S.vks)
    t0 = host(M, M.alt)                                                                      # fails
    t1 = host(E, E.alt)                                                                      # passes
    t2 = engine.commits_submit(M.off, M.sigs, rnd.randbytes(32), vks=M.vks, msgs=M.msgs)      # plain, fails
    t3 = host(M, alt2)                                                                       # fails, one item more
    t4 = engine.commits_submit_templated_device(*_dev_args(alt, E), rnd.randbytes(32))      # passes
    t5 = engine.commits_submit_templated_device(*_dev_args(alt, M), rnd.randbytes(32))      # fails
    assert [t - t0 for t in (t1, t2, t3, t4, t5)] == [1, 2, 3, 4, 5]
    vd = (ctypes.c_int * 1)()
    for t in (t0, t1, t3, t4, t5):                  # an _alt ticket is a commit-set ticket: refused, stays pending
        assert lib.edc_batch_wait(ctx, t, None, None, None) == -2
        assert lib.edc_batch_wait_multi(ctx, t, 1, vd, None, None, None) == -2
    assert engine.commits_wait(t0) == M.expect      # the fallback on its own slot with five tickets in flight behind it
    assert engine.commits_wait(t1) == E.expect
    assert engine.commits_wait(t2) == M.expect
    assert engine.commits_wait(t3) == expect2       # its own variant bytes, not t0's
    assert engine.commits_wait(t4) == E.expect
    assert engine.commits_wait(t5) == M.expect      # the fallback from the caller's device arrays
    cv, iv, nb = ctypes.create_string_buffer(M.nc), ctypes.create_string_buffer(M.n), ctypes.c_int(-1)
    assert lib.edc_commits_wait(ctx, t5, cv, iv, ctypes.byref(nb)) == -2                      # already waited
    assert _host(engine, alt, M, rnd.randbytes(32)) == M.expect                               # slot 0 is free again


# ---- 5. argument and flag paths ----

def test_argument_and_flag_paths_leave_the_context_usable(engine, edc, alt):
    import torch
    M = alt("mixed")
    gen, lib, ctx = alt.gen, engine.lib, engine.ctx
    engine.keycache_clear()
    ts, _keep = alt.templates.struct()
    p = ctypes.byref(ts)
    nc, n = M.nc, M.n
    seed = bytes(range(32))
    off = (ctypes.c_uint32 * (nc + 1))(*M.off)
    ctpl = (ctypes.c_uint16 * nc)(*M.commit_tpl)
    vk, sig, var = b"".join(M.vks), b"".join(M.sigs), b"".join(M.holes)
    voff = (ctypes.c_uint32 * (n + 1))(*([0] + [sum(len(h) for h in M.holes[:i + 1]) for i in range(n)]))
    ab = bytes(M.alt)
    cv, iv, nb = ctypes.create_string_buffer(nc), ctypes.create_string_buffer(n), ctypes.c_int(-1)
    out = (cv, iv, ctypes.byref(nb))
    d_alt, d_vk, d_sig, d_var, d_voff, var_bytes = M.dev()
    dev = (d_vk.data_ptr(), d_sig.data_ptr(), d_var.data_ptr(), d_voff.data_ptr(), var_bytes)

    def usable():
        nb.value = -1
        assert lib.edc_tmpl_commits_verify_alt(ctx, p, nc, off, ctpl, 4, ab, vk, None, sig, var, voff, seed, *out) == 1
        assert (list(cv.raw), list(iv.raw), nb.value) == (M.verdicts, M.codes, M.n_bad)
        assert lib.edc_tmpl_commits_verify_device(ctx, p, nc, off, ctpl, 4, d_alt.data_ptr(), *dev, seed, *out) == 1
        assert (list(cv.raw), list(iv.raw), nb.value) == (M.verdicts, M.codes, M.n_bad)

    def u16(v):
        return (ctypes.c_uint16 * len(v))(*v)

    usable()
    assert M.off[0] == M.off[1] and M.off[-2] == M.off[-1] and M.commit_tpl[-1] == 4     # empty first and last commits
    high = u16([5 if c == 1 else t for c, t in enumerate(M.commit_tpl)])                 # [5, 9) leaves the set of 8
    empty_first = u16([6] + M.commit_tpl[1:])                                            # an empty commit's window counts
    empty_last = u16(M.commit_tpl[:-1] + [5])
    over = bytes(M.alt[:n - 1]) + bytes([4])                                             # item_alt[n - 1] = alt_span
    over0 = bytes([4]) + bytes(M.alt[1:])
    bad_voff = (ctypes.c_uint32 * (n + 1))(*([0, 5, 4] + list(voff)[3:]))
    host = lambda tp, span, a, *r: lib.edc_tmpl_commits_verify_alt(ctx, p, nc, off, tp, span, a, *r, seed, *out)   # noqa: E731
    sub = lambda tp, span, a: lib.edc_tmpl_commits_submit_alt(ctx, p, nc, off, tp, span, a, vk, None, sig, var, voff, seed)  # noqa: E731
    devf = lambda tp, span: lib.edc_tmpl_commits_verify_device(ctx, p, nc, off, tp, span, d_alt.data_ptr(), *dev, seed, *out)  # noqa: E731
    dsub = lambda tp, span: lib.edc_tmpl_commits_submit_device(ctx, p, nc, off, tp, span, d_alt.data_ptr(), *dev, seed)     # noqa: E731
    H = (vk, None, sig, var, voff)
    refusals = [
        lambda: host(ctpl, 0, ab, *H), lambda: host(ctpl, 257, ab, *H),                  # alt_span outside 1..256
        lambda: host(ctpl, 5, ab, *H),                                                   # base 4 + 5 > 8
        lambda: host(high, 4, ab, *H), lambda: host(empty_first, 4, ab, *H), lambda: host(empty_last, 4, ab, *H),
        lambda: host(ctpl, 4, over, *H), lambda: host(ctpl, 4, over0, *H),               # item_alt[i] = alt_span
        lambda: host(ctpl, 3, ab, *H),                                                   # some item_alt[i] = 3 = alt_span
        lambda: host(ctpl, 4, ab, vk, None, sig, var, bad_voff),                         # the existing checks still apply
        lambda: host(ctpl, 4, ab, None, None, sig, var, voff),
        lambda: host(u16([8] + M.commit_tpl[1:]), 1, None, *H),                          # commit_tpl[c] = count
        lambda: lib.edc_tmpl_commits_verify_alt(ctx, p, nc, off, ctpl, 4, ab, *H, None, *out),   # no seed
        lambda: sub(ctpl, 0, ab), lambda: sub(ctpl, 257, ab), lambda: sub(high, 4, ab), lambda: sub(ctpl, 4, over),
        lambda: devf(ctpl, 0), lambda: devf(ctpl, 257), lambda: devf(ctpl, 5), lambda: devf(empty_last, 4),
        lambda: dsub(ctpl, 0), lambda: dsub(high, 4),
        lambda: lib.edc_tmpl_commits_verify_device(ctx, p, nc, off, ctpl, 4, d_alt.data_ptr(), dev[0] + 8, *dev[1:], seed, *out),
        lambda: lib.edc_debug_tmpl_commit_map_alt(ctx, nc, off, ctpl, 0, ab, (ctypes.c_uint16 * n)(), None, 1, None),
        lambda: lib.edc_debug_tmpl_commit_map_alt(ctx, nc, off, ctpl, 257, ab, (ctypes.c_uint16 * n)(), None, 1, None),
    ]
    for i, refuse in enumerate(refusals):
        assert refuse() == -2, i
        usable()
    # the device's own check: one byte >= alt_span is EDC_ERR_ARG from the call and from the wait, never a verdict
    for item in (n - 1, 7, 0):
        bad = d_alt.clone()
        bad[item] = 4
        torch.cuda.synchronize()
        nb.value = -1
        assert lib.edc_tmpl_commits_verify_device(ctx, p, nc, off, ctpl, 4, bad.data_ptr(), *dev, seed, *out) == -2
        assert b"templated items" in lib.edc_last_error(ctx)
        usable()
        tk = lib.edc_tmpl_commits_submit_device(ctx, p, nc, off, ctpl, 4, bad.data_ptr(), *dev, seed)
        assert tk >= 0
        assert lib.edc_commits_wait(ctx, tk, *out) == -2
        assert lib.edc_commits_wait(ctx, tk, *out) == -2                                 # and the ticket is spent
        usable()
    # a hole offset past var_bytes on the device takes the same path
    assert lib.edc_tmpl_commits_verify_device(ctx, p, nc, off, ctpl, 4, d_alt.data_ptr(), *dev[:4], var_bytes - 1, seed,
                                              *out) == -2
    usable()
    # nc = 0: nothing to verify
    nb.value = -1
    assert lib.edc_tmpl_commits_verify_alt(ctx, p, 0, None, None, 4, None, None, None, None, None, None, seed, None, None,
                                           ctypes.byref(nb)) == 0 and nb.value == 0
    assert lib.edc_tmpl_commits_verify_device(ctx, p, 0, None, None, 4, None, None, None, None, None, 0, seed, None, None,
                                              None) == 0
    tk = engine.commits_submit_templated_device(alt.templates, [0], [], 4, None, None, None, None, None, 0, seed)
    assert engine.commits_wait(tk) == (0, [], [], 0)
    assert engine.commits_verify_templated_alt(alt.templates, [0, 0, 0], [0, 4], 4, [], [], [], seed, vks=[]) == (0, [0, 0], [], 0)
    usable()


def test_live_allocations_return_to_their_start(edc, alt):
    M = alt("mixed")
    base = edc.debug_live_allocs()
    eng = edc.Engine(0)
    try:
        seed = bytes(32)
        assert _host(eng, alt, M, seed) == M.expect
        assert eng.commits_verify_templated_device(*_dev_args(alt, M), seed) == M.expect
        tk = eng.commits_submit_templated_device(*_dev_args(alt, M), seed)
        assert eng.commits_wait(tk) == M.expect
        b = alt.gen.build("edge9", messages=False)
        assert _map_alt(eng, b["commit_off"], b["commit_tpl"], 4, b["alt"])[1:] == (b["tpl"], 0)
        assert edc.debug_live_allocs()[0] > base[0]
    finally:
        eng.close()
    assert edc.debug_live_allocs() == base
