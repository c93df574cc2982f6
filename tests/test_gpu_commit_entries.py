"""GPU: the host paths of the commit-set entries (include/edc.h, edc_commits_* / edc_tmpl_commits_*)
that no verdict shows: the slot claims and their two messages, tickets that refusals and failed
enqueues must not consume, the order of argument errors and a busy slot, nc = 0 in every form, and
the Python wrappers' in-flight bookkeeping.

Inputs: the first 8 items of the `valid` set of tests/golden/commits.json cut as [0, 1, 8] with
templates (1, 2), and for the forms with variants the leading commits of the `mixed` set of
tests/golden/commits_alt.json up to the first offset >= 8. The expectations are the fixtures'
(the oracle's). The module has its own Engine, so edc_set_slots disturbs no other test. All
comparisons are exact."""
import ctypes
import types

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SLOT0 = b"slot 0 busy: wait for submitted batches first"
ALL_SLOTS = b"all slots in flight: wait for the oldest ticket first"
FORMS = ["host", "device", "tmpl", "alt", "tmpl_device"]
TEMPLATED = ["tmpl", "alt", "tmpl_device"]
VARIANTS = ["alt", "tmpl_device"]
SEED = bytes(range(32))
N = 8


def _u32(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def _u16(*v):
    return (ctypes.c_uint16 * len(v))(*v)


@pytest.fixture(scope="module")
def env(edc, oracle):
    """The module's Engine and the two small inputs, host and device."""
    torch = pytest.importorskip("torch")
    from test_gpu_commits import CommitSet, _gen
    from test_gpu_commits_alt import AltSet, _load
    eng = edc.Engine(0)
    d = torch.device("cuda:0")

    def up(b):
        return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).to(d)

    def offsets(parts, ctype):
        return (ctype * (len(parts) + 1))(*[sum(len(p) for p in parts[:i]) for i in range(len(parts) + 1)])

    gen = _gen()
    V = CommitSet("valid", eng, oracle, gen, golden("commits.json"))
    assert V.tpl[:N] == [1] + [2] * 7 and V.codes[:N] == [0] * N
    P = types.SimpleNamespace(nc=2, n=N, off=[0, 1, N], ctpl=[1, 2], vks=V.vks[:N], sigs=V.sigs[:N], msgs=V.msgs[:N],
                              ks=V.ks[:N], holes=V.holes[:N], tpl=V.tpl[:N], expect=(0, [0, 0], [0] * N, 0),
                              templates=edc.batch.Templates(*gen.templates()))
    galt = _load("gen_commits_alt")
    M = AltSet("mixed", eng, galt, golden("commits_alt.json"))
    nc = next(c for c in range(1, M.nc + 1) if M.off[c] >= N)
    n = M.off[nc]
    assert N <= n <= 20
    bad = sum(M.verdicts[:nc])
    assert bad == sum(1 for a, e in zip(M.off[:nc], M.off[1:nc + 1]) if any(M.codes[a:e]))
    A = types.SimpleNamespace(nc=nc, n=n, off=M.off[:nc + 1], ctpl=M.commit_tpl[:nc], span=galt.ALT_SPAN, alt=M.alt[:n],
                              vks=M.vks[:n], sigs=M.sigs[:n], holes=M.holes[:n], tpl=M.tpl[:n],
                              expect=(1 if bad else 0, M.verdicts[:nc], M.codes[:n], bad),
                              templates=edc.batch.Templates(*galt.templates()))
    for S in (P, A):
        S.c_off, S.c_tpl = _u32(*S.off), _u16(*S.ctpl)
        S.vk, S.sig, S.var = b"".join(S.vks), b"".join(S.sigs), b"".join(S.holes) or b"\0"
        S.voff = offsets(S.holes, ctypes.c_uint32)
        S.item_tpl = _u16(*S.tpl)
        S.ts, S.keep = S.templates.struct()
        S.p_ts = ctypes.byref(S.ts)
    P.arena, P.moff, P.k = b"".join(P.msgs), offsets(P.msgs, ctypes.c_uint64), b"".join(P.ks)
    P.idx = _u32(*range(N))
    P.d_vk, P.d_sig, P.d_msg, P.d_k = up(P.vk), up(P.sig), up(P.arena), up(P.k)
    P.d_off = torch.tensor(list(P.moff), dtype=torch.int64, device=d)
    A.ab = bytes(A.alt)
    A.d_alt, A.d_vk, A.d_sig, A.d_var = up(A.ab), up(A.vk), up(A.sig), up(A.var)
    A.d_voff = torch.tensor(list(A.voff), dtype=torch.int32, device=d)
    A.d_tpl = torch.tensor(A.tpl, dtype=torch.int16, device=d)
    A.var_bytes = A.voff[A.n]
    torch.cuda.synchronize()
    yield types.SimpleNamespace(eng=eng, lib=eng.lib, ctx=eng.ctx, P=P, A=A, edc=edc)
    eng.close()


def _args(env, form, off=None, ts=None, span=None):
    """(the set, the arguments of `form`'s two entries between ctx and z_seed)."""
    P, A = env.P, env.A
    S = A if form in VARIANTS else P
    off = S.c_off if off is None else off
    ts = S.p_ts if ts is None else ts
    span = A.span if span is None else span
    nc = len(off) - 1
    if form == "host":
        return S, (nc, off, S.vk, None, S.sig, S.arena, S.moff, None)
    if form == "device":
        return S, (nc, off, S.d_vk.data_ptr(), S.d_sig.data_ptr(), S.d_msg.data_ptr(), S.d_off.data_ptr(), None)
    if form == "tmpl":
        return S, (ts, nc, off, S.c_tpl, S.vk, None, S.sig, S.var, S.voff)
    if form == "alt":
        return S, (ts, nc, off, S.c_tpl, span, S.ab, S.vk, None, S.sig, S.var, S.voff)
    return S, (ts, nc, off, S.c_tpl, span, S.d_alt.data_ptr(), S.d_vk.data_ptr(), S.d_sig.data_ptr(), S.d_var.data_ptr(),
               S.d_voff.data_ptr(), S.var_bytes)


NAMES = {"host": "edc_commits_%s", "device": "edc_commits_%s_device", "tmpl": "edc_tmpl_commits_%s",
         "alt": "edc_tmpl_commits_%s_alt", "tmpl_device": "edc_tmpl_commits_%s_device"}


def _result(rc, S, cv, iv, nb, nc=None, n=None):
    nc, n = (S.nc, S.n) if nc is None else (nc, n)
    return rc, list(cv.raw[:nc]), list(iv.raw[:n]), nb.value


def _verify(env, form, **kw):
    """(rc, commit verdicts, item codes, n_bad) of the form's verify entry on its set."""
    S, args = _args(env, form, **kw)
    cv, iv, nb = ctypes.create_string_buffer(S.nc), ctypes.create_string_buffer(S.n), ctypes.c_int(-1)
    rc = getattr(env.lib, NAMES[form] % "verify")(env.ctx, *args, SEED, cv, iv, ctypes.byref(nb))
    return _result(rc, S, cv, iv, nb)


def _submit(env, form, **kw):
    S, args = _args(env, form, **kw)
    return getattr(env.lib, NAMES[form] % "submit")(env.ctx, *args, SEED)


def _wait(env, form, ticket, nc=None, n=None):
    S = env.A if form in VARIANTS else env.P
    cv, iv, nb = ctypes.create_string_buffer(S.nc), ctypes.create_string_buffer(S.n), ctypes.c_int(-1)
    rc = env.lib.edc_commits_wait(env.ctx, ticket, cv, iv, ctypes.byref(nb))
    return _result(rc, S, cv, iv, nb, nc, n)


def _expect(env, form):
    return (env.A if form in VARIANTS else env.P).expect


def _err(env):
    return env.lib.edc_last_error(env.ctx)


def _two_slots(env):
    assert env.lib.edc_set_slots(env.ctx, 2) == 0       # also restarts the tickets at 0


def test_the_forms_verify_the_small_inputs(env):
    """The inputs themselves, through every entry, on an idle context."""
    _two_slots(env)
    for form in FORMS:
        assert _verify(env, form) == _expect(env, form), form
        t = _submit(env, form)
        assert t >= 0, _err(env)
        assert _wait(env, form, t) == _expect(env, form), form


def test_slot0_busy(env):
    lib, ctx, P, A = env.lib, env.ctx, env.P, env.A
    _two_slots(env)
    t = _submit(env, "host")
    assert t == 0                                   # ticket 0 of 2 slots: slot 0
    for form in FORMS:
        assert _verify(env, form)[0] == -2 and _err(env) == SLOT0, form
    check8, verdicts, nbad = ctypes.create_string_buffer(32), ctypes.create_string_buffer(N), ctypes.c_int(-1)
    out16, flagged = (ctypes.c_uint16 * A.n)(), ctypes.c_int(-1)
    others = {
        "edc_tmpl_batch_verify": lambda: lib.edc_tmpl_batch_verify(ctx, P.p_ts, N, P.vk, None, P.sig, P.item_tpl, P.var,
                                                                   P.voff, SEED, check8),
        "edc_tmpl_batch_verify_device": lambda: lib.edc_tmpl_batch_verify_device(
            ctx, A.p_ts, A.n, A.d_vk.data_ptr(), A.d_sig.data_ptr(), A.d_tpl.data_ptr(), A.d_var.data_ptr(),
            A.d_voff.data_ptr(), A.var_bytes, SEED, 0, None, check8),
        "edc_batch_verify_prehashed_fallback": lambda: lib.edc_batch_verify_prehashed_fallback(
            ctx, N, P.vk, P.sig, P.k, SEED, verdicts, ctypes.byref(nbad), check8),
        "edc_debug_tmpl_commit_map": lambda: lib.edc_debug_tmpl_commit_map(ctx, P.nc, P.c_off, P.c_tpl, out16, 1, None),
        "edc_debug_tmpl_commit_map_alt": lambda: lib.edc_debug_tmpl_commit_map_alt(
            ctx, A.nc, A.c_off, A.c_tpl, A.span, A.ab, out16, ctypes.byref(flagged), 1, None),
    }
    for name, call in others.items():
        assert call() == -2 and _err(env) == SLOT0, name
    assert _wait(env, "host", t) == P.expect
    assert _verify(env, "host") == P.expect and P.expect[0] == 0
    for name, call in others.items():               # and with slot 0 idle again each of them runs
        assert call() in (0, 1), (name, _err(env))
    assert list(out16) == A.tpl and flagged.value == 0


def test_all_slots_in_flight(env):
    lib, ctx, P, A = env.lib, env.ctx, env.P, env.A
    env.eng.keycache_load(P.vks)                      # the indexed entries check their indices before the claim
    try:
        _two_slots(env)
        t0, t1 = _submit(env, "host"), _submit(env, "alt")
        assert (t0, t1) == (0, 1)
        for form in FORMS:
            assert _submit(env, form) == -2 and _err(env) == ALL_SLOTS, form
        dv, ds, dm, do, dk = (x.data_ptr() for x in (P.d_vk, P.d_sig, P.d_msg, P.d_off, P.d_k))
        others = {
            "edc_batch_submit": lambda: lib.edc_batch_submit(ctx, N, P.vk, P.sig, P.arena, P.moff, SEED, 0, 0),
            "edc_batch_submit_indexed": lambda: lib.edc_batch_submit_indexed(ctx, N, P.idx, P.sig, P.arena, P.moff, SEED, 0, 0),
            "edc_batch_submit_device": lambda: lib.edc_batch_submit_device(ctx, N, dv, ds, dm, do, SEED, 0, None, 0),
            "edc_batch_submit_prehashed": lambda: lib.edc_batch_submit_prehashed(ctx, N, P.vk, P.sig, P.k, SEED, 0, 0),
            "edc_batch_submit_prehashed_indexed": lambda: lib.edc_batch_submit_prehashed_indexed(ctx, N, P.idx, P.sig, P.k,
                                                                                                 SEED, 0, 0),
            "edc_batch_submit_prehashed_device": lambda: lib.edc_batch_submit_prehashed_device(ctx, N, dv, ds, dk, SEED, 0,
                                                                                               None, 0),
            "edc_tmpl_batch_submit": lambda: lib.edc_tmpl_batch_submit(ctx, P.p_ts, N, P.vk, None, P.sig, P.item_tpl, P.var,
                                                                       P.voff, SEED, 0, 0),
            "edc_batch_submit_multi_device": lambda: lib.edc_batch_submit_multi_device(ctx, 1, 2048, dv, ds, dm, do, None,
                                                                                       SEED, 0, 0),
        }
        for name, call in others.items():
            assert call() == -2 and _err(env) == ALL_SLOTS, name
        assert _wait(env, "host", t0) == P.expect
        assert _wait(env, "alt", t1) == A.expect
        t2 = _submit(env, "tmpl")
        assert t2 == t1 + 1                         # the refusals consumed nothing
        assert _wait(env, "tmpl", t2) == P.expect
    finally:
        env.eng.keycache_clear()


def test_a_failed_enqueue_takes_no_ticket(env):
    """The check that comes after the claim: enqueue_prefix refuses device key / signature arrays
    that are not 16-byte aligned, after edc_commits_submit_device has claimed its slot and before
    anything is launched."""
    lib, ctx, P = env.lib, env.ctx, env.P
    _two_slots(env)
    t0 = _submit(env, "device")
    assert t0 == 0 and _wait(env, "device", t0) == P.expect
    assert P.d_vk.data_ptr() % 16 == 0
    rc = lib.edc_commits_submit_device(ctx, P.nc, P.c_off, P.d_vk.data_ptr() + 8, P.d_sig.data_ptr(), P.d_msg.data_ptr(),
                                       P.d_off.data_ptr(), None, SEED)
    assert rc == -2 and b"16-byte aligned" in _err(env)
    t1 = _submit(env, "device")
    assert t1 == t0 + 1
    assert _wait(env, "device", t1) == P.expect


def test_argument_errors_come_before_a_busy_slot(env):
    P = env.P
    _two_slots(env)
    t = _submit(env, "host")
    assert t == 0
    assert _verify(env, "host", off=_u32(1, 1, N))[0] == -2
    assert _err(env).startswith(b"commit offsets:")
    none_ts = env.edc.EdcTemplates(0, P.ts.head, P.ts.head_off, P.ts.tail, P.ts.tail_off)
    assert _verify(env, "tmpl", ts=ctypes.byref(none_ts))[0] == -2
    assert _err(env).startswith(b"template set:")
    assert _verify(env, "tmpl")[0] == -2 and _err(env) == SLOT0
    assert _wait(env, "host", t) == P.expect


def test_no_commits(env):
    """nc = 0. A verify is EDC_OK with n_bad = 0 before anything else is looked at; a submit still
    checks the template set and, with variants, that alt_span is in 1..256, then takes a ticket
    whose wait gives no verdicts."""
    lib, ctx, P, A = env.lib, env.ctx, env.P, env.A
    _two_slots(env)
    nulls = {"host": (0,) + (None,) * 7, "device": (0,) + (None,) * 6, "tmpl": (None, 0) + (None,) * 7,
             "alt": (None, 0, None, None, 0) + (None,) * 6, "tmpl_device": (None, 0, None, None, 0) + (None,) * 5 + (0,)}
    for form in FORMS:
        nb = ctypes.c_int(-1)
        assert getattr(lib, NAMES[form] % "verify")(ctx, *nulls[form], SEED, None, None, ctypes.byref(nb)) == 0, form
        assert nb.value == 0, form
        assert getattr(lib, NAMES[form] % "verify")(ctx, *nulls[form], SEED, None, None, None) == 0, form

    def submit(form, ts=None, span=None):
        a = list(nulls[form])
        if form in TEMPLATED:
            a[0] = ts
        if form in VARIANTS:
            a[4] = span
        return getattr(lib, NAMES[form] % "submit")(ctx, *a, SEED)

    none_ts = env.edc.EdcTemplates(0, P.ts.head, P.ts.head_off, P.ts.tail, P.ts.tail_off)
    nxt = 0
    for form in FORMS:
        t = submit(form, A.p_ts, A.span)
        assert t == nxt, (form, _err(env))
        assert _wait(env, form, t, 0, 0) == (0, [], [], 0), form
        nxt += 1
    for form in TEMPLATED:
        assert submit(form, None, A.span) == -2 and _err(env).startswith(b"template set:"), form
        assert submit(form, ctypes.byref(none_ts), A.span) == -2 and _err(env).startswith(b"template set:"), form
    for form in VARIANTS:
        for span in (0, 257):
            assert submit(form, A.p_ts, span) == -2 and _err(env) == b"template variants: alt_span in 1..256", (form, span)
        assert _submit(env, form, span=0) == -2 and _err(env).startswith(b"template variants: alt_span in 1..256 and"), form
        assert _verify(env, form, span=0)[0] == -2, form          # never read as the one-template call
    t = _submit(env, "host")
    assert t == nxt                                 # none of the refusals took a ticket
    assert _wait(env, "host", t) == P.expect


def test_python_bookkeeping(env):
    eng, P, A = env.eng, env.P, env.A
    _two_slots(env)
    pd = (P.d_vk.data_ptr(), P.d_sig.data_ptr(), P.d_msg.data_ptr(), P.d_off.data_ptr())
    ad = (A.d_alt, A.d_vk, A.d_sig, A.d_var, A.d_voff, A.var_bytes)
    pairs = [
        (eng.commits_verify, eng.commits_submit, (P.off, P.sigs, SEED), dict(vks=P.vks, msgs=P.msgs), P),
        (eng.commits_verify_templated, eng.commits_submit_templated, (P.templates, P.off, P.ctpl, P.sigs, P.holes, SEED),
         dict(vks=P.vks), P),
        (eng.commits_verify_templated_alt, eng.commits_submit_templated_alt,
         (A.templates, A.off, A.ctpl, A.span, A.alt, A.sigs, A.holes, SEED), dict(vks=A.vks), A),
        (eng.commits_verify_templated_device, eng.commits_submit_templated_device,
         (A.templates, A.off, A.ctpl, A.span) + ad + (SEED,), {}, A),
        (eng.commits_verify_device, eng.commits_submit_device, (P.off,) + pd + (SEED,), {}, P),
    ]
    assert eng._commits_inflight == {}
    for verify, submit, args, kw, S in pairs:
        t = submit(*args, **kw)
        assert list(eng._commits_inflight) == [t]
        got = eng.commits_wait(t)
        assert got == verify(*args, **kw) == S.expect, submit.__name__
        assert eng._commits_inflight == {}
    with pytest.raises(env.edc.EngineError):
        eng.commits_submit([1, 1, N], P.sigs, SEED, vks=P.vks, msgs=P.msgs)       # commit_off[0] != 0
    assert eng._commits_inflight == {}
    with pytest.raises(env.edc.EngineError):
        eng.commits_wait(12345)
    t = eng.commits_submit(P.off, P.sigs, SEED, vks=P.vks, ks=P.ks)
    assert eng.commits_wait(t) == P.expect
    with pytest.raises(env.edc.EngineError):
        eng.commits_wait(t)                         # already waited
