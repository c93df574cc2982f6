"""GPU: cached templated quorum commit sets (include/edc.h, edc_cached_tmpl_quorum_*): select, gather
and hash the checked votes, look those up, verify the misses.

Expected values: the pure-Python model (tests/golden/gen_quorum.py) on the oracle's item codes;
edc_tmpl_quorum_verify_device for the cold table; and the PLAIN cached form
(edc_cached_quorum_verify_device, held to the model, the lookup and its own miss list by
test_gpu_cached_quorum.py) on the materialised messages at the same table state, which is built by
clearing the table and feeding it the same votes through edc_sigcache_verify_each. W is the tile."""
import random

import pytest

from test_gpu_quorum import QuorumSet, _offsets, _same
from test_gpu_tmpl_quorum import Items, _i32, _tq, _up, boundary, g, qsets  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

W = 256
BAD = [346, 645, 700, 800, 2047]
KEYS = ("code", "commit_verdicts", "item_verdicts", "tally", "n_bad_commits", "n_checked", "check8")


@pytest.fixture(scope="module")
def ceng(edc):
    pytest.importorskip("torch")
    eng = edc.Engine(0)
    eng.sigcache_create(1 << 14)
    yield eng
    eng.close()


def _ctq(eng, T, off, ctpl, D, thr, seed, light, span=1, **kw):
    a = dict(d_vk=D.vk, d_sig=D.sig, d_var=D.var, d_var_off=D.voff, var_bytes=D.var_bytes, d_power=D.power, d_flag=D.flag,
             d_item_alt=D.alt)
    a.update(kw)
    return eng.quorum_verify_templated_cached_device(T, off, ctpl, a["d_vk"], a["d_sig"], a["d_var"], a["d_var_off"],
                                                     a["var_bytes"], a["d_power"], a["d_flag"], thr, seed, light=light,
                                                     alt_span=span, d_item_alt=a["d_item_alt"])


def _plain(eng, off, D, msgs, thr, seed, light):
    """edc_cached_quorum_verify_device on the materialised messages (keys, signatures and votes of D)."""
    import torch
    d_msg = _up(b"".join(msgs))
    d_off = torch.tensor(_offsets([len(m) for m in msgs]), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return eng.quorum_verify_cached_device(off, D.vk, D.sig, d_msg, d_off, D.power, D.flag, thr, seed, light=light)


def _warm(eng, vks, sigs, msgs, items):
    eng.sigcache_clear()
    if items:
        eng.verify_each_cached([vks[i] for i in items], [sigs[i] for i in items], msgs=[msgs[i] for i in items])
    st = eng.sigcache_stats()
    return st


def _delta(a, b):
    return [b[k] - a[k] for k in ("hits", "misses", "inserted", "dropped")]


@pytest.mark.parametrize("light", [False, True], ids=["full", "light"])
@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_cold_warm_and_partly_warm(ceng, g, qsets, name, light):
    Q, T = qsets(name), qsets.templates
    S = Q.S
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT if light else g.FULL, Q.codes)
    m = j["n_checked"]
    bad = [i for i in range(Q.n) if j["checked"][i] and Q.codes[i]]
    assert name == "valid" or bad == [i for i in BAD if j["checked"][i]]
    rnd = random.Random("ctq%s%d" % (name, light))
    seed = rnd.randbytes(32)
    D = Items(Q.vks, Q.sigs, S.holes, Q.power, Q.flag)
    # cold: every output is edc_tmpl_quorum_verify_device's, and SHA-512 ran over the checked votes only
    ceng.sigcache_clear()
    want = _tq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, seed, light)
    _same(want, j)
    st0 = ceng.sigcache_stats()
    cold = _ctq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, seed, light)
    for key in KEYS:
        assert cold[key] == want[key], key
    assert cold["n_miss"] == m
    assert ceng.cached_quorum_last() == (Q.n, m, 0, m, m, m - len(bad))
    assert ceng.tmpl_quorum_last()[:3] == (Q.n, m, m)
    assert _delta(st0, ceng.sigcache_stats()) == [0, m, m - len(bad), 0]
    if light:
        assert m < Q.n                                          # SHA-512 ran over the checked votes, not all n
    # the same call again: only the bad checked votes miss
    st0 = ceng.sigcache_stats()
    warm = _ctq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, seed, light)
    for key in KEYS[:-1]:
        assert warm[key] == cold[key], key
    assert warm["n_miss"] == len(bad)
    assert ceng.cached_quorum_last() == (Q.n, m, m - len(bad), len(bad), m, 0)
    assert _delta(st0, ceng.sigcache_stats()) == [m - len(bad), len(bad), 0, 0]
    # partly warm, both forms against the plain cached form at the same table state
    sub = sorted(set(rnd.sample(range(Q.n), Q.n // 2)) | set(BAD[:2]))
    feed = [i for i in sub if Q.flag[i] != 0]                       # an absent vote's bytes are not a vote
    hits = sum(1 for i in feed if j["checked"][i] and Q.codes[i] == 0)
    seed = rnd.randbytes(32)
    st0 = _warm(ceng, Q.vks, Q.sigs, Q.msgs, feed)
    plain = _plain(ceng, Q.off, D, Q.msgs, Q.thr, seed, light)
    d_plain = _delta(st0, ceng.sigcache_stats())
    _same(plain, j)
    assert plain["n_miss"] == m - hits and 0 < hits < m and d_plain[:2] == [hits, m - hits]
    for host in (False, True):
        st0 = _warm(ceng, Q.vks, Q.sigs, Q.msgs, feed)
        if host:
            got = ceng.quorum_verify_templated_cached(T, Q.off, S.commit_tpl, Q.sigs, S.holes, Q.power, Q.flag, Q.thr, seed,
                                                      light=light, vks=Q.vks)
        else:
            got = _ctq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, seed, light)
        for key in KEYS + ("n_miss",):
            assert got[key] == plain[key], (host, key)
        assert _delta(st0, ceng.sigcache_stats()) == d_plain
        assert ceng.cached_quorum_last() == (Q.n, m, hits, m - hits, m, d_plain[2])


@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 513, 5 * W + 37])
def test_gather_and_lookup_boundaries(ceng, boundary, m):
    """The sets of test_gpu_tmpl_quorum's gather boundaries (m checked votes of 5 W + 37, full mode), with
    hit patterns laid over the m-item list the lookup runs on: its tiles are not the queue's."""
    B = boundary
    flag = B.flags(m)
    checked = [i for i, f in enumerate(flag) if f]
    thr = [sum(B.power[a:e]) // 3 for a, e in zip(B.off, B.off[1:])]
    sigs = list(B.sigs)
    bad = None
    if m == 257:                                                    # a bad checked vote in the list's second tile
        bad = checked[256]
        sigs[bad] = sigs[bad][:5] + bytes([sigs[bad][5] ^ 1]) + sigs[bad][6:]
    D = Items(B.vks, sigs, B.holes, B.power, flag)
    rnd = random.Random("cb%d" % m)
    patterns = {"cold": [], "all": checked, "first tile of the list": checked[:W], "all but the list's last": checked[:-1],
                "all but the first of the list's second tile": checked[:W] + checked[W + 1:]}
    for what, warm in patterns.items():
        warm = [i for i in warm if i != bad]
        seed = rnd.randbytes(32)
        _warm(ceng, B.vks, sigs, B.msgs, warm)
        plain = _plain(ceng, B.off, D, B.msgs, thr, seed, False)
        assert plain["n_checked"] == m and (plain["code"] == 1) == (bad is not None), what
        if bad is not None:
            assert [i for i, v in enumerate(plain["item_verdicts"]) if v not in (0, 255)] == [bad]
        _warm(ceng, B.vks, sigs, B.msgs, warm)
        got = _ctq(ceng, B.T, B.off, B.ctpl, D, thr, seed, False)
        for key in KEYS + ("n_miss",):
            assert got[key] == plain[key], (what, key)
        # votes with equal key, hole and template are byte-identical items: one record serves them all, and
        # two lanes of one insert launch may still write a copy each (csrc/sigcache.h, Concurrency)
        key = lambda i: (B.vks[i], sigs[i], B.msgs[i])              # noqa: E731
        records = {key(i) for i in warm}
        hits = sum(1 for i in checked if key(i) in records)
        missed = {key(i) for i in checked if key(i) not in records and i != bad}
        last = ceng.cached_quorum_last()
        assert last[:5] == (B.n, m, hits, m - hits, m) and plain["n_miss"] == m - hits, what
        assert len(missed) <= last[5] <= m - hits - (bad is not None), what
        if what == "cold":
            want = _tq(ceng, B.T, B.off, B.ctpl, D, thr, seed, False)
            for key in KEYS:
                assert got[key] == want[key], key


def test_argument_errors_cover_all_items(ceng, edc, g, qsets):
    import torch
    Q, T = qsets("valid"), qsets.templates
    S = Q.S
    j = g.judge(Q.off, Q.power, Q.flag, Q.thr, g.LIGHT, Q.codes)
    rnd = random.Random("ctqargs")
    D = Items(Q.vks, Q.sigs, S.holes, Q.power, Q.flag)
    voff = _offsets([len(h) for h in S.holes])
    absent = next(i for i, f in enumerate(Q.flag) if f == 0 and i > W)
    unchecked = next(i for i, c in enumerate(j["checked"]) if not c and Q.flag[i] == 1)
    alt1 = [0] * Q.n
    alt1[absent] = 1                                                # >= alt_span = 1, at an absent item
    down = list(voff)
    down[unchecked + 1] = down[unchecked] - 1                       # decreasing at an item light mode leaves out
    flag3, big = list(Q.flag), list(Q.power)
    flag3[absent] = 3
    big[unchecked] = 2**63
    cases = [("alt", dict(d_item_alt=_up(bytes(alt1)))), ("down", dict(d_var_off=_i32(down))),
             ("past", dict(var_bytes=D.var_bytes - 1)), ("flag", dict(d_flag=_up(bytes(flag3)))),
             ("power", dict(d_power=QuorumSet.dev_power(big)))]
    torch.cuda.synchronize()
    ceng.sigcache_clear()
    st0 = ceng.sigcache_stats()
    for what, kw in cases:
        for light in (True, False):
            with pytest.raises(edc.EngineError, match="edc error -2"):
                _ctq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, rnd.randbytes(32), light, **kw)
        assert ceng.sigcache_stats() == st0, what
    for kw in (dict(item_alt=alt1), dict(var_off=down)):            # the host form refuses them on the host
        with pytest.raises(edc.EngineError, match="edc error -2"):
            ceng.quorum_verify_templated_cached(T, Q.off, S.commit_tpl, Q.sigs, S.holes, Q.power, Q.flag, Q.thr,
                                                rnd.randbytes(32), vks=Q.vks, **kw)
    assert ceng.sigcache_stats() == st0
    seed = rnd.randbytes(32)
    got = _ctq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, seed, True)  # the next valid call: the cold-table result
    want = _tq(ceng, T, Q.off, S.commit_tpl, D, Q.thr, seed, True)
    for key in KEYS:
        assert got[key] == want[key], key
    assert got["n_miss"] == got["n_checked"] == j["n_checked"]
    # no table, nc = 0
    eng = edc.Engine(0)
    try:
        with pytest.raises(edc.EngineError, match="edc error -2"):
            _ctq(eng, T, Q.off, S.commit_tpl, D, Q.thr, seed, True)
        eng.sigcache_create(1 << 10)
        got = eng.quorum_verify_templated_cached_device(T, [0], [], None, None, None, None, 0, None, None, [], seed)
        assert (got["code"], got["n_checked"], got["n_miss"]) == (0, 0, 0)
    finally:
        eng.close()


def test_host_form_with_key_idx(ceng, qsets):
    """quorum_verify_templated_cached(key_idx=...) after keycache_load, cold and then warm: all eight
    fields are those of the same call with vks= at the same table state, and everything but n_miss
    is quorum_verify_templated(key_idx=...)'s. check8 belongs to the list that was verified, so the
    warm call's, whose list is empty, is held to the vks= call's alone."""
    Q, T = qsets("valid"), qsets.templates
    S = Q.S
    keys = list(dict.fromkeys(Q.vks))
    pos = {k: i for i, k in enumerate(keys)}
    idx = [pos[k] for k in Q.vks]
    seed = random.Random("tmplhostidx").randbytes(32)
    ceng.keycache_load(keys)
    try:
        want = ceng.quorum_verify_templated(T, Q.off, S.commit_tpl, Q.sigs, S.holes, Q.power, Q.flag, Q.thr, seed, key_idx=idx)
        runs = {}
        for how, kw in (("vks", dict(vks=Q.vks)), ("key_idx", dict(key_idx=idx))):
            ceng.sigcache_clear()
            runs[how] = [ceng.quorum_verify_templated_cached(T, Q.off, S.commit_tpl, Q.sigs, S.holes, Q.power, Q.flag, Q.thr,
                                                             seed, **kw) for _ in ("cold", "warm")]
    finally:
        ceng.keycache_clear()
    for got, same in zip(runs["key_idx"], runs["vks"]):
        assert sorted(got) == sorted(KEYS + ("n_miss",))
        assert got == same
    cold, warm = runs["key_idx"]
    for key in KEYS:
        assert cold[key] == want[key], key
    for key in KEYS[:-1]:
        assert warm[key] == want[key], key
    assert cold["n_miss"] == cold["n_checked"] > 0 and warm["n_miss"] == 0      # every vote of this set is valid
