"""GPU: templated messages (include/edc.h, edc_tmpl_* and edc_vfy_queue_templated). The device
assembles message i = heads[tpl[i]] + hole_i + tails[tpl[i]]; everything here is compared with
Templates.materialize() on the host, with the existing message entries run on the materialised
messages, and with tests/golden/templates.json (the oracle's k, verdict and [8]*check) -- never
with another templated call."""
import ctypes
import random

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

G = golden("templates.json")
Z_SEED = bytes.fromhex(G["z_seed"])
IDENTITY = bytes([1]) + bytes(31)
EDC_ERR_ARG = -2


def _torch():
    import torch
    return torch, torch.device("cuda:0")


def _dev(data):
    torch, dev = _torch()
    t = torch.frombuffer(bytearray(bytes(data) or b"\0"), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    return t


class Case:
    def __init__(self, edc, c):
        self.t = edc.batch.Templates([bytes.fromhex(h) for h in c["heads"]], [bytes.fromhex(x) for x in c["tails"]])
        self.tpl = c["tpl"]
        self.holes = [bytes.fromhex(h) for h in c["holes"]]
        self.keys = [bytes.fromhex(k) for k in c["keys"]]
        self.key_idx = c["key_idx"]
        self.vks = [self.keys[j] for j in self.key_idx]
        self.sigs = [bytes.fromhex(s) for s in c["sigs"]]
        self.msgs = self.t.materialize(self.tpl, self.holes)
        self.k = [bytes.fromhex(k) for k in c["k"]]
        self.code = c["batch_code"]
        self.check8 = bytes.fromhex(c["check8"])
        self.n = len(self.tpl)


@pytest.fixture(scope="module")
def cases(edc):
    return {c["name"]: Case(edc, c) for c in G["cases"]}


def _dev_items(tpl, holes, slack=0):
    """(d_tpl, d_var, d_var_off, var_bytes): the items as device arrays; d_var has `slack` more bytes."""
    var = b"".join(holes)
    off = [0]
    for h in holes:
        off.append(off[-1] + len(h))
    d_tpl = _dev(b"".join(t.to_bytes(2, "little") for t in tpl))
    d_off = _dev(b"".join(o.to_bytes(4, "little") for o in off))
    return d_tpl, _dev(var + bytes(slack)), d_off, len(var)


def _expand(engine, t, tpl, holes):
    """(arena bytes, offsets) through edc_tmpl_expand_device, into buffers of exactly the bound."""
    torch, dev = _torch()
    n = len(tpl)
    d_tpl, d_var, d_off, vb = _dev_items(tpl, holes)
    cap = n * (max(map(len, t.heads)) + max(map(len, t.tails))) + vb + 16
    d_msg = torch.full((cap,), 0xEE, dtype=torch.uint8, device=dev)
    d_moff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    engine.tmpl_expand_device(t, n, d_tpl.data_ptr(), d_var.data_ptr(), d_off.data_ptr(), vb, d_msg.data_ptr(), cap,
                              d_moff.data_ptr())
    return bytes(d_msg.cpu().numpy().tobytes()), [int(x) for x in d_moff.cpu().tolist()], cap


def _check_expansion(engine, t, tpl, holes):
    msgs = t.materialize(tpl, holes)
    arena, off, cap = _expand(engine, t, tpl, holes)
    want = b"".join(msgs)
    exp_off = [0]
    for m in msgs:
        exp_off.append(exp_off[-1] + len(m))
    assert off == exp_off
    assert arena[:len(want)] == want
    assert arena[len(want):] == b"\xEE" * (cap - len(want))      # nothing written behind the last message


def _random_items(edc, rnd, n, count, big=False):
    lens = [0, 1, 15, 16, 17, 33, 70]
    heads = [rnd.randbytes(rnd.choice(lens) + (900 if big else 0)) for _ in range(count)]
    tails = [rnd.randbytes(rnd.choice(lens)) for _ in range(count)]
    tpl = [rnd.randrange(count) for _ in range(n)]
    holes = [rnd.randbytes(rnd.choice([0, 0, 1, 12, 12, 12, 16, 40])) for _ in range(n)]
    return edc.batch.Templates(heads, tails), tpl, holes


@pytest.mark.parametrize("n", [1, 3, 300, 4099])
def test_expansion_bytes_and_offsets(edc, engine, n):
    """300 crosses a 256-item workgroup, 4099 the scan's block level; odd sizes and mixed lengths put
    message starts at every 16-byte phase."""
    t, tpl, holes = _random_items(edc, random.Random(1000 + n), n, 5)
    _check_expansion(engine, t, tpl, holes)


def test_expansion_of_a_set_too_large_for_lds(edc, engine):
    t, tpl, holes = _random_items(edc, random.Random(7), 300, 40, big=True)   # > 16 KiB: read from HBM
    assert sum(map(len, t.heads)) + sum(map(len, t.tails)) > 16384
    _check_expansion(engine, t, tpl, holes)


def test_expansion_all_empty_and_one_template(edc, engine):
    t = edc.batch.Templates([b""], [b""])
    _check_expansion(engine, t, [0] * 300, [b""] * 300)
    _check_expansion(engine, t, [0] * 5, [b"", b"abc", b"", b"", b"z"])


def test_expansion_at_sha512_and_staging_boundaries(engine, cases):
    c = cases["lengths"]
    assert {len(m) for m in c.msgs} == {0, 1, 15, 16, 17, 47, 48, 111, 112, 175, 176, 300}
    _check_expansion(engine, c.t, c.tpl, c.holes)


@pytest.mark.parametrize("name", ["votes", "lengths"])
def test_challenge(engine, cases, name):
    c = cases[name]
    k = engine.tmpl_challenge(c.t, c.vks, c.sigs, c.tpl, c.holes)
    assert k == engine.challenge(c.vks, c.sigs, c.msgs)
    assert k == c.k
    assert engine.tmpl_challenge(c.t, [], [], [], []) == []


def _device_verify(engine, c, z_base):
    lib = engine.lib
    ts, _keep = c.t.struct()
    d_vk, d_sig = _dev(b"".join(c.vks)), _dev(b"".join(c.sigs))
    d_tpl, d_var, d_off, vb = _dev_items(c.tpl, c.holes)
    c8 = ctypes.create_string_buffer(32)
    rc = lib.edc_tmpl_batch_verify_device(engine.ctx, ctypes.byref(ts), c.n, d_vk.data_ptr(), d_sig.data_ptr(),
                                          d_tpl.data_ptr(), d_var.data_ptr(), d_off.data_ptr(), vb, Z_SEED, z_base, None,
                                          c8)
    # the message entry on the materialised arena, same z
    arena = b"".join(c.msgs)
    offs = [0]
    for m in c.msgs:
        offs.append(offs[-1] + len(m))
    d_msg = _dev(arena + bytes(16))
    d_moff = _dev(b"".join(o.to_bytes(8, "little") for o in offs))
    r8 = ctypes.create_string_buffer(32)
    ref = lib.edc_batch_verify_device(engine.ctx, c.n, d_vk.data_ptr(), d_sig.data_ptr(), d_msg.data_ptr(),
                                      d_moff.data_ptr(), Z_SEED, z_base, None, r8)
    return (rc, c8.raw), (ref, r8.raw)


@pytest.mark.parametrize("name", ["votes", "votes_flipped", "lengths"])
def test_batch_verify_forms(engine, cases, name):
    """Host (vk and key_idx), device (z_base 0 and not) and submit forms against edc_batch_verify on
    the materialised messages and the golden verdict. votes_flipped: one hole byte of item 10 of 32
    differs from what was signed."""
    c = cases[name]
    ref = engine.batch_verify(c.vks, c.sigs, c.msgs, z_seed=Z_SEED, want_check8=True)
    assert ref == (c.code, c.check8)
    if name == "votes_flipped":
        assert ref[0] == 1 and ref[1] not in (IDENTITY, bytes(32))
    assert engine.batch_verify_templated(c.t, c.sigs, c.tpl, c.holes, Z_SEED, vks=c.vks, want_check8=True) == ref
    got, dref = _device_verify(engine, c, 0)
    assert got == dref == ref
    got, dref = _device_verify(engine, c, 1000003)
    assert got == dref and got[0] == c.code and (got[1] != ref[1] or c.code == 0)
    tk = engine.batch_submit_templated(c.t, c.sigs, c.tpl, c.holes, Z_SEED, vks=c.vks, want_check8=True)
    assert engine.batch_wait(tk, want_check8=True) == ref
    try:
        engine.keycache_load(c.keys)
        assert engine.batch_verify_templated(c.t, c.sigs, c.tpl, c.holes, Z_SEED, key_idx=c.key_idx,
                                             want_check8=True) == ref
        tk = engine.batch_submit_templated(c.t, c.sigs, c.tpl, c.holes, Z_SEED, key_idx=c.key_idx, want_check8=True)
        tk2 = engine.batch_submit_indexed(c.key_idx, c.sigs, c.msgs, Z_SEED, want_check8=True)
        assert engine.batch_wait(tk, want_check8=True) == ref
        assert engine.batch_wait(tk2, want_check8=True) == ref
    finally:
        engine.keycache_clear()


def test_empty_batch_is_what_the_message_entry_returns(edc, engine):
    t = edc.batch.Templates([b"h"], [b"t"])
    ref = engine.batch_verify([], [], [], z_seed=Z_SEED, want_check8=True)
    assert engine.batch_verify_templated(t, [], [], [], Z_SEED, vks=[], want_check8=True) == ref
    tk = engine.batch_submit_templated(t, [], [], [], Z_SEED, vks=[], want_check8=True)
    assert engine.batch_wait(tk, want_check8=True) == engine.batch_wait(
        engine.batch_submit([], [], [], Z_SEED, want_check8=True), want_check8=True)


def _queue_mixed(sv, c, cuts, plain):
    """Pieces of c in order: piece `plain` through edc_verifier_queue, the others templated."""
    for p, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if p == plain:
            sv.queue_many(c.vks[a:b], c.sigs[a:b], msgs=c.msgs[a:b])
        else:
            sv.queue_templated(c.t, c.sigs[a:b], c.tpl[a:b], c.holes[a:b], vks=c.vks[a:b])


@pytest.mark.parametrize("name", ["votes", "votes_flipped", "lengths"])
def test_verifier_three_templated_pieces_and_a_plain_one(edc, engine, cases, name):
    c = cases[name]
    ref = engine.batch_verify(c.vks, c.sigs, c.msgs, z_seed=Z_SEED, want_check8=True)
    cuts = [0, 7, 8, c.n - 5, c.n]
    for eager in (False, True):
        sv = edc.batch.StreamVerifier(engine)
        try:
            if eager:
                sv.begin_eager(Z_SEED)
            _queue_mixed(sv, c, cuts, plain=2 if eager else 1)
            assert sv.batch_size == c.n
            assert sv.verify_detailed(None if eager else Z_SEED) == ref
        finally:
            sv.close()


def test_verifier_key_indices_and_cached_second_pass(edc, engine, cases):
    c = cases["votes"]
    ref = engine.batch_verify(c.vks, c.sigs, c.msgs, z_seed=Z_SEED, want_check8=True)
    sv = edc.batch.StreamVerifier(engine)
    try:
        try:                                     # no registered list yet
            sv.queue_templated(c.t, c.sigs, c.tpl, c.holes, key_idx=c.key_idx)
            raise AssertionError("expected an argument error")
        except edc.EngineError as e:
            assert "edc error -2" in str(e)
        assert sv.batch_size == 0
        engine.keycache_load(c.keys)
        engine.sigcache_create(1024)
        sv.queue_templated(c.t, c.sigs[:20], c.tpl[:20], c.holes[:20], key_idx=c.key_idx[:20])
        sv.queue_templated(c.t, c.sigs[20:], c.tpl[20:], c.holes[20:], vks=c.vks[20:])
        assert sv.verify_detailed(Z_SEED) == ref
        sv.reset()
        sv.set_cached(True)
        _queue_mixed(sv, c, [0, 7, 8, 27, 32], plain=1)
        assert sv.batch_size == 32 and sv.cache_counts == (32, 0)
        assert sv.verify_detailed(Z_SEED) == ref == (0, IDENTITY)
        sv.reset()
        _queue_mixed(sv, c, [0, 7, 8, 27, 32], plain=1)      # the same items again: every one is a record
        assert sv.batch_size == 0 and sv.cache_counts == (32, 32)
        assert sv.verify_detailed(Z_SEED)[0] == 0
    finally:
        sv.close()
        engine.sigcache_create(0)
        engine.keycache_clear()


def _refused(edc, f):
    try:
        f()
    except edc.EngineError as e:
        assert "edc error -2" in str(e), str(e)
        return True
    return False


def test_host_forms_refuse_malformed_items(edc, engine, cases):
    c = cases["votes"]
    n = c.n
    bad_tpl = list(c.tpl)
    bad_tpl[9] = c.t.count                       # index == count
    off = [12 * i for i in range(n + 1)]
    dec = list(off)
    dec[5] = dec[4] - 1                          # a decreasing var_off
    nz = [1] + off[1:]                           # var_off[0] != 0
    sv = edc.batch.StreamVerifier(engine)
    try:
        sv.queue_templated(c.t, c.sigs[:4], c.tpl[:4], c.holes[:4], vks=c.vks[:4])
        calls = []
        for kw in ({"tpl": bad_tpl}, {"var_off": dec}, {"var_off": nz}, {"vks": None}, {"key_idx": c.key_idx}):
            a = {"tpl": c.tpl, "var_off": None, "vks": c.vks, "key_idx": None}
            a.update(kw)
            calls += [
                lambda a=a: engine.batch_verify_templated(c.t, c.sigs, a["tpl"], c.holes, Z_SEED, vks=a["vks"],
                                                          key_idx=a["key_idx"], var_off=a["var_off"]),
                lambda a=a: engine.batch_submit_templated(c.t, c.sigs, a["tpl"], c.holes, Z_SEED, vks=a["vks"],
                                                          key_idx=a["key_idx"], var_off=a["var_off"]),
                lambda a=a: sv.queue_templated(c.t, c.sigs, a["tpl"], c.holes, vks=a["vks"], key_idx=a["key_idx"],
                                               var_off=a["var_off"]),
            ]
        calls.append(lambda: engine.tmpl_challenge(c.t, c.vks, c.sigs, bad_tpl, c.holes))
        calls.append(lambda: engine.tmpl_challenge(c.t, c.vks, c.sigs, c.tpl, c.holes, var_off=dec))
        for f in calls:
            assert _refused(edc, f)
            assert sv.batch_size == 4
        # nothing was submitted either: the next ticket is waited normally, and the context still verifies
        tk = engine.batch_submit_templated(c.t, c.sigs, c.tpl, c.holes, Z_SEED, vks=c.vks, want_check8=True)
        assert engine.batch_wait(tk, want_check8=True) == (c.code, c.check8)
        sv.queue_templated(c.t, c.sigs[4:], c.tpl[4:], c.holes[4:], vks=c.vks[4:])
        assert sv.verify_detailed(Z_SEED) == (c.code, c.check8)
    finally:
        sv.close()


def test_device_forms_refuse_an_offset_past_var_bytes(engine, cases):
    """var_off[n] = var_bytes + 1 with the var tensor 64 bytes larger than declared: inside allocated
    memory whatever the implementation does, and outside the declared arena."""
    torch, dev = _torch()
    c = cases["votes"]
    lib = engine.lib
    ts, _keep = c.t.struct()
    d_vk, d_sig = _dev(b"".join(c.vks)), _dev(b"".join(c.sigs))
    d_tpl, d_var, d_off, vb = _dev_items(c.tpl, c.holes, slack=64)
    bad_off = d_off.clone()
    bad_off[4 * c.n:4 * c.n + 4] = torch.tensor(list((vb + 1).to_bytes(4, "little")), dtype=torch.uint8, device=dev)
    cap = c.n * (108 + 38) + vb + 64             # above the bound: longest head 108, longest tail 38
    d_msg = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_moff = torch.zeros(c.n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    c8 = ctypes.create_string_buffer(32)
    for off, want in ((bad_off, EDC_ERR_ARG), (d_off, c.code)):
        rc = lib.edc_tmpl_expand_device(engine.ctx, ctypes.byref(ts), c.n, d_tpl.data_ptr(), d_var.data_ptr(),
                                        off.data_ptr(), vb, d_msg.data_ptr(), cap, d_moff.data_ptr())
        assert rc == (EDC_ERR_ARG if off is bad_off else 0)
        rc = lib.edc_tmpl_batch_verify_device(engine.ctx, ctypes.byref(ts), c.n, d_vk.data_ptr(), d_sig.data_ptr(),
                                              d_tpl.data_ptr(), d_var.data_ptr(), off.data_ptr(), vb, Z_SEED, 0, None, c8)
        assert rc == want
    assert c8.raw == c.check8
    # msg_cap below the bound is refused before anything runs
    assert lib.edc_tmpl_expand_device(engine.ctx, ctypes.byref(ts), c.n, d_tpl.data_ptr(), d_var.data_ptr(),
                                      d_off.data_ptr(), vb, d_msg.data_ptr(), c.n * (108 + 38) + vb + 15,
                                      d_moff.data_ptr()) == EDC_ERR_ARG
    # and the context still serves the message entries
    assert engine.batch_verify(c.vks, c.sigs, c.msgs, z_seed=Z_SEED, want_check8=True) == (c.code, c.check8)
