"""GPU: one context growing every tier of the quorum workspace (csrc/edc_api.hip, QuorumWs) and each
side of a pair in turn. STEPS runs in order on ONE engine, and every result must equal, byte for
byte, the same call on a fresh engine; steps 4 and 9 must also equal the Python model of the
selection that tests/test_gpu_vq_trust.py checks its pairs against.

The floors are the growth policies' own: item_cap and off_cap (csrc/devbuf.h) start at 1024, so the
per-vote shape V is 1,200 votes in 30 commits and the per-commit shape C is 1,030 commits of 2 votes,
both over a 40-key registered list with a two-version history.

Version 0, the trusted set: all 40 keys, 10 each (total 400). Version 1: key 0 has left (total 390).
Every commit is judged at version 1 and trusted at version 0, in light mode, and lists its signers in
ascending key order. In V a commit holds all 40: side A skips key 0 (no member) and checks keys 1..27
(270 > 260), side B checks keys 0..13 (140 > 133); the union is keys 0..27, key 0 is B-only."""
import pytest

from test_gpu_vq_trust import _model_select, _offsets

pytestmark = pytest.mark.gpu

SEED = bytes(range(60, 92))
M = 40
POWER = {0: [10] * M, 1: [0] + [10] * (M - 1)}          # 0: no member of that version
THR, TTHR = 2 * 390 // 3, 400 // 3
BAD = 3 * M                                             # V's item of commit 3, key 0: checked by side B alone


class Shape:
    def __init__(self, eng, edc, name, commits, templates):
        """commits: one list of key positions per commit"""
        self.off = _offsets([len(c) for c in commits])
        self.n, self.nc = self.off[-1], len(commits)
        self.who = [p for c in commits for p in c]
        self.flag = [edc.VOTE_COMMIT] * self.n
        self.holes = [b"%s-%d" % (name, i) for i in range(self.n)]
        self.T = templates
        self.msgs = templates.materialize([0] * self.n, self.holes)
        _, self.sigs = eng.sign([SEEDS[p] for p in self.who], self.msgs)
        self.ver, self.tver = [1] * self.nc, [0] * self.nc
        self.thr, self.tthr = [THR] * self.nc, [TTHR] * self.nc
        self.power = [POWER[1][p] for p in self.who]    # the host form's powers: side A's

    def pair(self):
        return dict(versions=self.ver, trust_versions=self.tver, trust_thresholds=self.tthr)

    def model(self, v, thr):
        """(power, flag, checked, planned) of the side that judges at version v"""
        power = [POWER[v][p] for p in self.who]
        flag = [f if pw else 0 for f, pw in zip(self.flag, power)]
        return (power, flag) + _model_select(self.off, power, flag, thr, True)


SEEDS = [bytes([7, p]) * 16 for p in range(M)]


def _register(eng, D):
    eng.sigcache_create(1 << 12)
    eng.keycache_load(D["keys"])
    eng.valset_set_powers(POWER[0])
    eng.vhist_set(POWER[0], [[(0, D["edc"].VHIST_NOT_MEMBER)]])
    return eng


def build_data(edc):
    eng = edc.Engine(0)
    keys, _ = eng.sign(SEEDS, [b""] * M)
    T = edc.batch.Templates([b"regrow head "], [b" tail"])
    D = dict(edc=edc, keys=list(keys),
             S=Shape(eng, edc, b"s", [list(range(8))] * 3, T),
             V=Shape(eng, edc, b"v", [list(range(M))] * 30, T),
             C=Shape(eng, edc, b"c", [[0, 1 + c % (M - 1)] for c in range(1030)], T))
    eng.close()
    D["V_bad"] = list(D["V"].sigs)
    D["V_bad"][BAD] = D["V_bad"][BAD][:40] + bytes([D["V_bad"][BAD][40] ^ 4]) + D["V_bad"][BAD][41:]
    assert D["V"].n == 1200 and D["C"].nc == 1030 and D["S"].n == 24
    return D


@pytest.fixture(scope="module")
def data(edc):
    pytest.importorskip("torch")
    return build_data(edc)


def _plain(eng, X):
    return eng.quorum_verify(X.off, X.sigs, X.power, X.flag, X.thr, SEED, light=True, key_idx=X.who, msgs=X.msgs)


def _vq(eng, X, sigs=None, **kw):
    return eng.vq_verify(X.off, X.flag, X.thr, SEED, light=True, key_idx=X.who, sigs=sigs or X.sigs, msgs=X.msgs, **kw)


def _tmpl_pair(eng, X):
    return eng.vq_verify(X.off, X.flag, X.thr, SEED, light=True, key_idx=X.who, sigs=X.sigs, cached=True, templates=X.T,
                         commit_tpl=[0] * X.nc, alt_span=1, item_alt=[0] * X.n, holes=X.holes, **X.pair())


def _pair_records(eng, X, **kw):
    r = _vq(eng, X, **kw)
    return r, eng.vq_trust_last(), eng.vq_last()


STEPS = [
    ("1 plain, small", lambda e, D: _plain(e, D["S"])),
    ("2 valset request, small", lambda e, D: _vq(e, D["S"])),
    ("3 pair, small", lambda e, D: _pair_records(e, D["S"], **D["S"].pair())),
    ("4 pair, V, one bad signature on side B", lambda e, D: _pair_records(e, D["V"], sigs=D["V_bad"], **D["V"].pair())),
    ("5 pair, C", lambda e, D: _pair_records(e, D["C"], **D["C"].pair())),
    ("6 cached templated pair, V", lambda e, D: (_tmpl_pair(e, D["V"]), e.vq_trust_last(), e.vq_last())),
    ("7 pair, small, again", lambda e, D: _pair_records(e, D["S"], **D["S"].pair())),
    ("8 plain, V", lambda e, D: _plain(e, D["V"])),
    ("9 trust resolve, V", lambda e, D: e.vq_trust_resolve(D["V"].off, D["V"].ver, D["V"].tver, D["V"].flag, D["V"].thr,
                                                           D["V"].tthr, light=True, key_idx=D["V"].who)),
]


def test_one_context_grows_every_tier(data):
    D, edc = data, data["edc"]
    V = D["V"]
    one = _register(edc.Engine(0), D)
    got = []
    for name, step in STEPS:
        got.append(step(one, D))
        fresh = _register(edc.Engine(0), D)
        want = step(fresh, D)
        fresh.close()
        assert got[-1] == want, name
    one.close()
    # the model of both selections of V
    pa, fa, ca, pla = V.model(1, V.thr)
    pb, fb, cb, plb = V.model(0, V.tthr)
    side = [a | 2 * b for a, b in zip(ca, cb)]
    assert side[:M] == [2] + [3] * 13 + [1] * 14 + [0] * 12
    # step 4: the failed union's tally, after the growth
    r, trust_last, vq_last = got[3]
    union = [i for i in range(V.n) if side[i]]
    assert trust_last == (sum(ca), sum(cb), sum(1 for s in side if s == 3), len(union)) and vq_last[:2] == (V.n, len(union))
    assert r["code"] == 1 and r["n_checked"] == len(union) == 840
    assert r["item_verdicts"] == [edc.NOT_CHECKED if not s else int(i == BAD) for i, s in enumerate(side)]
    assert r["tally"] == pla and r["commit_verdicts"] == [0] * V.nc and r["n_bad_commits"] == 0
    assert r["trust_tally"] == [p - (10 if c == 3 else 0) for c, p in enumerate(plb)]
    assert r["trust_verdicts"] == [edc.EDC_INVALID_SIGNATURE if c == 3 else 0 for c in range(V.nc)] and r["n_bad_trust"] == 1
    # step 6 hashed the union alone and found none of it in the fresh table
    assert got[5][0]["n_miss"] == got[5][0]["n_checked"] == 840 and got[5][0]["code"] == 0
    # step 9: both sides' arrays
    r = got[8]
    for s, (power, flag, checked, planned) in (("a", (pa, fa, ca, pla)), ("b", (pb, fb, cb, plb))):
        assert (r[s]["power"], r[s]["flag"], r[s]["checked"], r[s]["planned"]) == (power, flag, checked, planned), s
        assert r[s]["dv"] == [0] * V.nc, s
    assert r["a"]["pos"] == [0xFFFFFFFF if p == 0 else p for p in V.who] and r["b"]["pos"] == V.who
    assert r["side"] == side and r["n_checked"] == 840
