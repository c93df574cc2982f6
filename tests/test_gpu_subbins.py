"""GPU parity of the MSM's sub-bin plans at small sizes (edc_api.hip batch_plan / fold_plan: the
slices of the densest windows cut into nsub[w] sub-bins by term index, edc_msm.hip term_digits and
window_combine) against the C oracle: verdict and compressed [8]*check, bit-exact. Everything is
integer arithmetic, so no tolerance applies.

edc_set_msm_bin_entries(256) brings the split that the 2^17..2^20 batches run by default down to
4-5 thousand items. Every case runs a valid batch and a batch with one bad item (a check point that
is not the identity), each twice (the second run plans from the first run's key-count hint),
restores the knobs it set, and asserts through Engine.last_plan() (edc_debug_last_plan) the
property of the plan it exists for, so that a case cannot pass while running nsub = 1.

The expected shapes follow from batch_plan: with 9-bit windows (n < 2^13) every window is one
256-bucket slice, and nsub[w] = the largest power of two <= entries expected in the slice / target
(at most 64). Short windows expect n + nf entries, high windows nf, where nf = 1 + the key terms the
hint of the previous grouped batch predicts (n per signature)."""
import random

import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

ENTRIES = 256


@pytest.fixture(scope="module")
def oracle_c():
    import os
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c as oc
    return oc


class Case:
    """One signed batch, its copy with one bad item, and the oracle's result for both."""

    def __init__(self, oc, vks, sigs, msgs, zseed, bad):
        self.vks, self.sigs, self.msgs, self.zseed, self.n = list(vks), list(sigs), list(msgs), zseed, len(vks)
        self.bad_msgs = list(msgs)
        self.bad_msgs[bad] = msgs[bad][:-1] + bytes([msgs[bad][-1] ^ 1])
        self.keys = list(dict.fromkeys(self.vks))
        self.exp_ok = oc.batch_verify(list(zip(self.vks, self.sigs, self.msgs)), zseed)
        self.exp_bad = oc.batch_verify(list(zip(self.vks, self.sigs, self.bad_msgs)), zseed)
        assert self.exp_ok[0] == 0 and self.exp_bad[0] == 1 and self.exp_bad[1] not in (None, self.exp_ok[1])

    def variants(self):
        return (self.msgs, self.exp_ok), (self.bad_msgs, self.exp_bad)


def _sign(engine, n, m, seed=0, msg_len=48):
    rnd = random.Random(n * 1000 + m + seed)
    seeds = [rnd.randbytes(32) for _ in range(m)]
    msgs = [rnd.randbytes(msg_len) for _ in range(n)]
    vks, sigs = engine.sign(seeds, msgs, seed_index=[i % m for i in range(n)])
    return vks, sigs, msgs, rnd.randbytes(32)


@pytest.fixture(scope="module")
def cases(engine, oracle_c):
    """(n, keys) -> Case, signed and judged by the oracle once for all the tests that use it."""
    memo = {}

    def get(n, m):
        if (n, m) not in memo:
            vks, sigs, msgs, zseed = _sign(engine, n, m)
            memo[n, m] = Case(oracle_c, vks, sigs, msgs, zseed, (3 * n) // 4 + 1)
        return memo[n, m]
    return get


@pytest.fixture()
def knobs(engine):
    """The engine with every knob these tests touch put back afterwards."""
    try:
        yield engine
    finally:
        engine.set_msm_bin_entries(0)
        engine.set_msm_shape(0, 0)
        engine.set_key_grouping(0)
        engine.set_key_split(0)
        engine.keycache_clear()
        engine.lib.edc_debug_set_scatter_stage(16384)


def _verify(engine, c, msgs):
    return engine.batch_verify(c.vks, c.sigs, msgs, z_seed=c.zseed, want_check8=True)


def _prime(engine, c, grouping=0):
    """A batch that leaves its key count as the context's hint (and must itself be right). Grouping
    is forced on for it: in auto mode a context whose last hint was "every key distinct" would run
    it with one key term per signature, which leaves no hint. `grouping` is the mode set afterwards."""
    engine.set_key_grouping(1)
    try:
        assert _verify(engine, c, c.msgs) == c.exp_ok
    finally:
        engine.set_key_grouping(grouping)


def _run(engine, c, check_plan, prime=None, runs=2):
    """Valid and bad variant, `runs` times each; check_plan(plan, run) sees the plan of every run."""
    for msgs, exp in c.variants():
        if prime is not None:
            prime()
        for run in range(runs):
            got = _verify(engine, c, msgs)
            check_plan(engine.last_plan(), run)
            assert got == exp, (c.n, run, engine.last_plan())


def _few_keys_plan(n):
    """What batch_plan gives for n < 2^13 items of 150 keys with the few-keys hint and 256 entries
    per bin: 15 short windows of one slice with n + 151 expected entries, 16 eight-bit high windows
    with 151."""
    def check(plan, run):
        nsub_short = 16 if (n + 151) // ENTRIES < 32 else 32
        assert plan["few"] and not plan["per_sig"] and not plan["split"] and not plan["fold"]
        assert plan["target"] == ENTRIES and plan["nranges"] == 1 and plan["sum_ranges"] == 0
        assert (plan["nwin"], plan["nwin_short"]) == (31, 15)
        assert plan["bits"] == [9] * 8 + [8] * 7 + [8] * 13 + [7] * 3 and plan["nslice"] == [1] * 31
        assert plan["nsub"] == [nsub_short] * 15 + [1] * 16
        assert max(plan["nsub"]) >= 16 and len(set(plan["nsub"])) > 1
        assert plan["bins_per_range"] == 15 * nsub_short + 16
    return check


# 1. argument checks
def test_bin_entries_argument_checks(knobs, cases):
    lib, ctx = knobs.lib, knobs.ctx
    assert lib.edc_set_msm_bin_entries(ctx, -1) == -2
    assert lib.edc_set_msm_bin_entries(ctx, 255) == -2
    assert lib.edc_set_msm_bin_entries(None, 256) == -2
    assert lib.edc_set_msm_bin_entries(ctx, 0) == 0
    assert lib.edc_set_msm_bin_entries(ctx, 256) == 0
    c = cases(4096, 150)
    for msgs, exp in c.variants():
        assert _verify(knobs, c, msgs) == exp
        assert knobs.last_plan()["target"] == 256


# 2. uneven sub-bins, few keys
@pytest.mark.parametrize("n", [4096, 4099, 5001])
def test_uneven_subbins_few_keys(knobs, cases, n):
    """nsub = 16 on the short windows and 1 on the eight-bit high windows (256 bins); 4099 and 5001
    terms are no multiple of nsub, so the sub-bins of a slice hold different numbers of terms."""
    c = cases(n, 150)
    _prime(knobs, c)
    knobs.set_msm_bin_entries(ENTRIES)
    _run(knobs, c, _few_keys_plan(n))
    assert knobs.last_plan()["bins_per_range"] == 256


# 3. dense high windows
@pytest.mark.parametrize("m,grouping", [(256, 2), (256, 3), (4096, 1)], ids=["per_sig", "overflow", "distinct_grouped"])
def test_dense_high_windows(knobs, cases, m, grouping):
    """n key terms: one per signature by the host's choice (grouping 2), by the on-device overflow
    path (grouping 3, planned from the hint of an all-distinct batch and then from its own, which an
    overflow leaves at n keys), or n distinct keys grouped. 8193 expected entries in a short window
    and 4097 in a high one: nsub = 32 and 16, 15 * 32 + 14 * 16 = 704 bins."""
    n = 4096
    c = cases(n, m)
    _prime(knobs, cases(n, n), grouping)
    knobs.set_msm_bin_entries(ENTRIES)

    def check(plan, run):
        assert not plan["few"] and plan["per_sig"] == (grouping == 2) and plan["target"] == ENTRIES
        assert (plan["nwin"], plan["nwin_short"]) == (29, 15) and plan["nslice"] == [1] * 29
        assert plan["nsub"] == [32] * 15 + [16] * 14 and plan["bins_per_range"] == 704
    _run(knobs, c, check)


# 4. sweep of the knob
def test_knob_sweep_same_result(knobs, cases):
    """5000 items of 150 keys with the few-keys hint: 5151 expected entries per short window, so
    max(nsub) = 16, 8, 4, 1 at 256, 512, 1024, 4096 entries per bin and 1 at the default (4096 at
    this size)."""
    c = cases(5000, 150)
    for msgs, exp in c.variants():
        maxes, results = [], []
        for entries in (256, 512, 1024, 4096, 0):
            knobs.set_msm_bin_entries(0)
            _prime(knobs, c)
            knobs.set_msm_bin_entries(entries)
            for run in range(2):
                results.append(_verify(knobs, c, msgs))
                plan = knobs.last_plan()
                assert plan["few"] and plan["target"] == (entries or 4096)
            maxes.append(max(plan["nsub"]))
        assert maxes == [16, 8, 4, 1, 1]
        assert results == [exp] * 10


# 5. stale hints, both directions
def test_stale_hint_dense_plan_few_terms(knobs, cases):
    """Hint of an all-distinct batch (grouping forced on, so that the next batch is grouped), then
    4096 items of ONE key: the high windows are planned for 4097 full terms (nsub = 16) and get two
    (B and the key), so at least 14 of the 16 sub-bins of each are empty. The second run plans from
    its own hint: few keys, one bin per high window."""
    n = 4096
    c, distinct = cases(n, 1), cases(n, n)
    knobs.set_key_grouping(1)
    knobs.set_msm_bin_entries(ENTRIES)

    def check(plan, run):
        assert not plan["per_sig"]
        if run == 0:
            assert not plan["few"] and plan["nwin"] == 29
            assert all(s >= 8 for s in plan["nsub"][15:]) and plan["nsub"][15] == 16
        else:
            assert plan["few"] and plan["nsub"][15:] == [1] * 16
    _run(knobs, c, check, prime=lambda: _prime(knobs, distinct, 1))


def test_stale_hint_few_keys_plan_dense_terms(knobs, cases):
    """Hint of a 150-key batch, then 4096 distinct keys: each eight-bit high window is ONE bin that
    takes the digits of all n + 1 full-width terms. The second run plans from its own hint (every
    key distinct: one key term per signature, dense windows)."""
    n = 4096
    c, votes = cases(n, n), cases(n, 150)
    knobs.set_msm_bin_entries(ENTRIES)

    def check(plan, run):
        if run == 0:
            assert plan["few"] and not plan["per_sig"] and plan["nwin"] == 31
            assert plan["nsub"] == [16] * 15 + [1] * 16 and plan["nslice"][15:] == [1] * 16
        else:
            assert plan["per_sig"] and not plan["few"] and plan["nsub"] == [32] * 15 + [16] * 14
    _run(knobs, c, check, prime=lambda: _prime(knobs, votes))


# 6. explicit parts win over the knob
def test_explicit_parts_win_over_the_knob(knobs, cases):
    c = cases(4099, 150)
    knobs.set_msm_shape(12, 3)
    knobs.set_msm_bin_entries(ENTRIES)

    def check(plan, run):
        assert plan["sum_ranges"] == 1 and plan["nranges"] == 3 and plan["target"] == 0
        assert plan["nsub"] == [1] * plan["nwin"] and max(plan["bits"]) == 12
    _run(knobs, c, check)


# 7. the bin cap
def test_bin_cap_doubles_the_target(knobs, oracle_c):
    """Shape: one key term per signature (grouping 2), 13-bit windows, 256 entries asked for.
    n = 87,380 is the largest batch that fits as asked: 7,936 bins (8 windows of 16 slices x 32, one
    of 8 x 64, the top short one 16 x 32, then 5 x 16 x 16, 4 x 8 x 32 and 16 x 32 over the high bits).
    n = 87,381 = ceil(2^18 / 3) is the smallest n, at any width 9..16, where the plan as asked
    passes 8,192 bins (the top short window's 3 n / 16 expected entries per slice reach 64 x 256:
    8,448 bins), so batch_plan doubles the target to 512: 4,224 bins. The oracle runs both sizes on
    the host's threads in well under a second."""
    n1 = 87381
    vks, sigs, msgs, zseed = _sign(knobs, n1, 150, msg_len=32)
    knobs.set_key_grouping(2)
    knobs.set_msm_shape(13, 0)
    knobs.set_msm_bin_entries(ENTRIES)
    for n, target, bins in ((n1 - 1, 256, 7936), (n1, 512, 4224)):
        for bad in (None, n // 2 + 3):
            m = list(msgs[:n])
            if bad is not None:
                m[bad] = m[bad][:-1] + bytes([m[bad][-1] ^ 1])
            offs, at = [0], 0
            for x in m:
                at += len(x)
                offs.append(at)
            code, c8, _ = oracle_c.batch_verify_parallel(b"".join(vks[:n]), b"".join(sigs[:n]), b"".join(m), offs, zseed)
            assert code == (0 if bad is None else 1) and c8 is not None
            for run in range(2):
                got = knobs.batch_verify(vks[:n], sigs[:n], m, z_seed=zseed, want_check8=True)
                plan = knobs.last_plan()
                assert plan["per_sig"] and plan["target"] == target and plan["bins_per_range"] == bins <= 8192
                assert max(plan["bits"]) == 13 and max(plan["nsub"]) == (64 if target == 256 else 32)
                assert got == (code, c8), (n, bad, run)


# 8. scatter direct path with sub-bins
@pytest.mark.parametrize("stage", [0, 512])
def test_scatter_direct_path_with_subbins(knobs, cases, stage):
    c = cases(4099, 150)
    _prime(knobs, c)
    knobs.lib.edc_debug_set_scatter_stage(stage)
    knobs.set_msm_bin_entries(ENTRIES)
    _run(knobs, c, _few_keys_plan(c.n))


# 9. small-order and torsion points across sub-bins
def test_torsion_points_across_subbins(knobs, cases, oracle_c):
    """The 196 ZIP215 corpus items (small-order and non-canonical A and R) at random positions of
    the 4096-item batch: a sub-bin's sum can be the identity or a torsion point when window_combine
    adds it. The corpus is valid under ZIP215, so the batch passes; with one bad item it must give
    the oracle's check point."""
    base = cases(4096, 150)
    fx = golden("zip215_small_order.json")
    msg = bytes.fromhex(fx["msg"])
    rnd = random.Random(215)
    vks, sigs, msgs = list(base.vks), list(base.sigs), list(base.msgs)
    pos = rnd.sample(range(base.n), len(fx["cases"]))
    assert len(pos) == 196
    for p, case in zip(pos, fx["cases"]):
        vks[p], sigs[p], msgs[p] = bytes.fromhex(case["vk"]), bytes.fromhex(case["sig"]), msg
    bad = next(i for i in range(3000, base.n) if i not in pos)
    c = Case(oracle_c, vks, sigs, msgs, base.zseed, bad)
    assert len(c.keys) * 16 <= c.n          # still "few keys" for the plan
    _prime(knobs, c)
    knobs.set_msm_bin_entries(ENTRIES)
    _run(knobs, c, _few_keys_plan(c.n))


# 10. split plan
def test_split_plan_with_subbins(knobs, cases):
    """Keys in the key cache: every term is short, 15 windows, 4096 + 2 * 151 expected entries in
    each: nsub = 16. Same result as the oracle and as the unsplit plan."""
    c = cases(4096, 150)
    _prime(knobs, c)
    u, ok = knobs.keycache_load(c.keys)
    assert u == 150 and all(ok)
    knobs.set_msm_bin_entries(ENTRIES)

    def split(plan, run):
        assert plan["split"] and plan["nwin"] == plan["nwin_short"] == 15
        assert plan["nsub"] == [16] * 15 and max(plan["nsub"]) > 1
    _run(knobs, c, split)
    knobs.set_key_split(1)
    _run(knobs, c, _few_keys_plan(c.n))


# 11. incremental verifier
@pytest.mark.parametrize("keycache", [False, True], ids=["plain", "keycache"])
def test_incremental_verifier_with_subbins(knobs, edc, cases, keycache):
    c = cases(4099, 150)
    _prime(knobs, c)
    if keycache:
        knobs.keycache_load(c.keys)
    knobs.set_msm_bin_entries(ENTRIES)
    for msgs, exp in c.variants():
        sv = edc.batch.StreamVerifier(knobs)
        try:
            at = 0
            for size in (7, 1500, c.n - 1507):
                sv.queue_many(c.vks[at:at + size], c.sigs[at:at + size], msgs=msgs[at:at + size])
                at += size
            assert sv.batch_size == c.n
            for run in range(2):
                got = sv.verify_detailed(c.zseed)
                plan = sv.last_plan
                assert plan["split"] == keycache == bool(sv.last_split) and not plan["fold"]
                assert plan["target"] == ENTRIES and plan["nsub"][:15] == [16] * 15
                assert got == exp
        finally:
            sv.close()
        assert _verify(knobs, c, msgs) == exp                 # edc_batch_verify on the same seed
        assert knobs.last_plan()["nsub"][:15] == [16] * 15


# 12. eager folds
def test_eager_folds_with_subbins(knobs, edc, cases):
    """Folds at >= 2000 pending items: pieces of 2100 and 2200 items fold as they are queued (2100
    and 2200 expected entries in each of the 15 one-slice windows: nsub = 8), the second with its
    terms starting at skip = 2100, which is what t & (nsub - 1) sees; 701 items stay for verify."""
    c = cases(5001, 150)
    _prime(knobs, c)
    knobs.set_msm_bin_entries(ENTRIES)
    for msgs, exp in c.variants():
        sv = edc.batch.StreamVerifier(knobs)
        try:
            sv.set_fold(2000)
            for run in range(2):
                sv.begin_eager(c.zseed)
                at = 0
                for size, folded in ((2100, (2100, 1)), (2200, (4300, 2)), (701, (4300, 2))):
                    sv.queue_many(c.vks[at:at + size], c.sigs[at:at + size], msgs=msgs[at:at + size])
                    at += size
                    assert sv.folded == folded
                    plan = sv.last_plan
                    assert plan["fold"] and plan["nwin"] == plan["nwin_short"] == 15 and plan["target"] == ENTRIES
                    assert plan["nsub"] == [8] * 15 and plan["bins_per_range"] == 120
                got = sv.verify_detailed()
                assert not sv.last_plan["fold"] and sv.last_plan["target"] == ENTRIES
                assert got == exp
                sv.reset()
        finally:
            sv.close()
        assert _verify(knobs, c, msgs) == exp                 # edc_batch_verify with the committed seed


# 13. quorum, light mode
@pytest.mark.parametrize("name", ["valid", "mixed_a"])
def test_quorum_light_with_subbins(knobs, oracle, name):
    from test_gpu_commits import CommitSet, _gen as gen_commits
    from test_gpu_quorum import QuorumSet, _same
    from test_quorum_abi import gen_quorum
    g = gen_quorum()
    Q = QuorumSet(name, CommitSet(name, knobs, oracle, gen_commits(), golden("commits.json")), g, golden("quorum.json"))
    j = Q.expect(g, g.LIGHT)
    seed = random.Random("subbins" + name).randbytes(32)
    got = {}
    for entries in (0, ENTRIES):
        knobs.set_msm_bin_entries(entries)
        for run in range(2):
            got[entries, run] = Q.device(knobs, seed, True)
            plan = knobs.last_plan()
            _same(got[entries, run], j)
        assert plan["target"] == (entries or 4096)
        assert (max(plan["nsub"]) > 1) == (entries == ENTRIES), plan
    for key in ("tally", "commit_verdicts", "item_verdicts", "check8", "code", "n_checked", "n_bad_commits"):
        assert got[0, 0][key] == got[0, 1][key] == got[ENTRIES, 0][key] == got[ENTRIES, 1][key], key
