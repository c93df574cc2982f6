"""GPU: the eager incremental verifier (edc_vfy_begin_eager, batch.StreamVerifier(eager=True)). The
block's z seed is committed before the items arrive, queue calls fold sum [z_i]R_i into a running
point and verify() runs the MSM over B, the keys and the unfolded tail. Verdicts and [8]*check are
bit-exact against tests/golden/batches.json or against engine.batch_verify of the same items and
seed, never against the verifier itself; `folded` proves that the folds ran."""
import ctypes
import hashlib
import random

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

BATCHES = golden("batches.json")["batches"]
BY_NAME = {b["name"]: b for b in BATCHES}
IDENTITY = bytes([1]) + bytes(31)
EDC_ERR_ARG = -2
SEED = bytes(range(32))
SEED2 = bytes(range(100, 132))


def _items(b):
    return [(bytes.fromhex(v), bytes.fromhex(s), bytes.fromhex(m)) for v, s, m in b["items"]]


def _expect(b):
    return b["expect_code"], (bytes.fromhex(b["expect_check8"]) if b["expect_check8"] is not None else bytes(32))


def _cols(items):
    return [v for v, _, _ in items], [s for _, s, _ in items], [m for _, _, m in items]


def _queue(sv, items):
    if items:
        vks, sigs, msgs = _cols(items)
        sv.queue_many(vks, sigs, msgs=msgs)


def _piece_sizes(n, pattern):
    sizes = {"whole": [n], "1_2_5_rest": [1, 2, 5, n]}.get(pattern, [1] * n)
    out, at = [], 0
    for s in sizes:
        if at >= n:
            break
        out.append(min(s, n - at))
        at += out[-1]
    return out


def _queue_pieces(sv, items, sizes):
    at = 0
    for s in sizes:
        _queue(sv, items[at:at + s])
        at += s
    assert at >= len(items)


def _expect_folded(sizes, fold):
    """(items, folds) by the rule of include/edc.h: a queue call folds everything pending once at
    least `fold` items are pending."""
    n = items = folds = 0
    for s in sizes:
        n += s
        if s and n - items >= fold:
            items, folds = n, folds + 1
    return items, folds


def _reference(engine, items, seed):
    vks, sigs, msgs = _cols(items)
    return engine.batch_verify(vks, sigs, msgs, z_seed=seed, want_check8=True)


@pytest.fixture()
def sv_factory(edc, engine):
    made = []

    def make(capacity=0, seed=SEED, fold=None):
        sv = edc.batch.StreamVerifier(engine, capacity)
        made.append(sv)
        if fold is not None:
            sv.set_fold(fold)
        if seed is not None:
            sv.begin_eager(seed)
        return sv

    yield make
    for sv in made:
        sv.close()


@pytest.fixture()
def restore(engine):
    yield engine
    engine.keycache_clear()
    engine.set_key_split(0)
    engine.set_key_grouping(0)


# 1. every golden batch x fold granularity x piece pattern
GOLDEN_CASES = [(b, f, p) for b in BATCHES for f in (1, 3, 64) for p in ("whole", "1_2_5_rest", "one_by_one")
                if p != "one_by_one" or len(b["items"]) <= 64]


@pytest.mark.parametrize("b,fold,pattern", GOLDEN_CASES, ids=[f"{b['name']}-fold{f}-{p}" for b, f, p in GOLDEN_CASES])
def test_golden_batches_bit_exact(sv_factory, b, fold, pattern):
    it = _items(b)
    sizes = _piece_sizes(len(it), pattern)
    sv = sv_factory(seed=bytes.fromhex(b["z_seed"]), fold=fold)
    assert sv.eager
    _queue_pieces(sv, it, sizes)
    assert sv.batch_size == len(it)
    items, folds = sv.folded
    assert (items, folds) == _expect_folded(sizes, fold)
    if fold in (1, 3) and len(it) >= 3:      # the case must not pass without ever folding
        assert items > 0 and folds > 0
    assert sv.verify_detailed() == _expect(b)


def _break(items, i):
    v, s, m = items[i]
    items[i] = (v, s[:40] + bytes([s[40] ^ 4]) + s[41:], m)


@pytest.fixture(scope="module")
def votes_ok(engine):
    """4,100 signatures from 150 keys."""
    rnd = random.Random(4100)
    n, nkeys = 4100, 150
    seeds = [hashlib.sha256(b"v" + i.to_bytes(4, "little")).digest() for i in range(nkeys)]
    msgs = [rnd.randbytes(40) for _ in range(n)]
    vks, sigs = engine.sign(seeds, msgs, seed_index=[(7 * i) % nkeys for i in range(n)])
    return list(zip(vks, sigs, msgs))


@pytest.fixture(scope="module")
def votes_4100(votes_ok):
    """The same with signature 3000 wrong."""
    it = list(votes_ok)
    _break(it, 3000)
    return it


@pytest.fixture(scope="module")
def ref_4100(engine, votes_4100):
    exp = _reference(engine, votes_4100, SEED)
    assert exp[0] == 1 and exp[1] not in (IDENTITY, bytes(32))
    return exp


# 2. fold ranges that start and end off the multiples of 4 (ChaCha block) and 2048 (k_coef chunk)
BOUNDARY_CASES = [([2047, 1, 2052], 1), ([3, 2046, 2051], 1), ([4100], 2048)]


@pytest.mark.parametrize("sizes,fold", BOUNDARY_CASES, ids=["2047_1_2052", "3_2046_2051", "whole_fold2048"])
def test_fold_boundaries(sv_factory, votes_4100, votes_ok, ref_4100, sizes, fold):
    sv = sv_factory(4100, fold=fold)
    _queue_pieces(sv, votes_4100, sizes)
    assert sv.folded == _expect_folded(sizes, fold)
    assert sv.verify_detailed() == ref_4100
    sv.reset()
    assert not sv.eager and sv.folded == (0, 0)
    sv.begin_eager(SEED)
    _queue_pieces(sv, votes_ok, sizes)
    assert sv.folded[0] > 0
    assert sv.verify_detailed() == (0, IDENTITY)


# 3. a tail that is never folded
@pytest.mark.parametrize("lo", [0, 2101], ids=["valid", "one_bad"])
def test_unfolded_tail(engine, sv_factory, votes_4100, lo):
    it = votes_4100[lo:lo + 1999]
    sv = sv_factory(fold=1000)
    _queue_pieces(sv, it, [1000, 999])
    assert sv.folded == (1000, 1)
    exp = _reference(engine, it, SEED)
    assert exp[0] == (1 if lo else 0)
    assert sv.verify_detailed() == exp


# 4. growth keeps the running point and the folded count
def test_growth_keeps_the_running_point(engine, sv_factory):
    b = BY_NAME["two_bad_of_300"]
    it = _items(b)
    sv = sv_factory(1, seed=bytes.fromhex(b["z_seed"]), fold=10)
    for p in range(30):
        _queue(sv, it[10 * p:10 * p + 10])
        assert sv.folded == (10 * p + 10, p + 1)
    exp = _reference(engine, it, bytes.fromhex(b["z_seed"]))
    assert exp == _expect(b)
    assert sv.verify_detailed() == exp


# 5. every plan the verify can take; pieces [1500, 2500, 100] at fold 1000: 4,000 folded, a tail of 100
PLAN_SIZES = [1500, 2500, 100]


def _check_plan(sv, ref):
    assert sv.folded == (4000, 2)
    assert sv.verify_detailed() == ref


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_plans_key_grouping_modes(restore, sv_factory, votes_4100, ref_4100, mode):
    restore.set_key_grouping(mode)
    sv = sv_factory(fold=1000)
    _queue_pieces(sv, votes_4100, PLAN_SIZES)
    _check_plan(sv, ref_4100)


@pytest.mark.parametrize("split", [0, 1], ids=["split", "set_key_split_1"])
def test_plans_key_cache(restore, sv_factory, votes_4100, ref_4100, split):
    restore.keycache_load(list(dict.fromkeys(v for v, _, _ in votes_4100)))
    restore.set_key_split(split)
    sv = sv_factory(fold=1000)
    _queue_pieces(sv, votes_4100, PLAN_SIZES)
    _check_plan(sv, ref_4100)
    assert sv.last_split == (0 if split else 1)


def test_plans_queue_indexed(restore, sv_factory, votes_4100, ref_4100):
    keys = list(dict.fromkeys(v for v, _, _ in votes_4100))
    pos = {k: i for i, k in enumerate(keys)}
    restore.keycache_load(keys)
    sv = sv_factory(fold=1000)
    at = 0
    for s in PLAN_SIZES:
        vks, sigs, msgs = _cols(votes_4100[at:at + s])
        sv.queue_indexed([pos[v] for v in vks], sigs, msgs=msgs)
        at += s
    _check_plan(sv, ref_4100)
    assert sv.last_split == 1


@pytest.fixture(scope="module")
def ks_4100(engine, votes_4100):
    return engine.challenge(*_cols(votes_4100))


def test_plans_prehashed(sv_factory, votes_4100, ks_4100, ref_4100):
    sv = sv_factory(fold=1000)
    at = 0
    for s in PLAN_SIZES:
        vks, sigs, _ = _cols(votes_4100[at:at + s])
        sv.queue_many(vks, sigs, ks=ks_4100[at:at + s])
        at += s
    _check_plan(sv, ref_4100)


def test_plans_queue_device(sv_factory, votes_4100, ks_4100, ref_4100):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")

    def to_dev(buf):
        return torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)

    sv = sv_factory(fold=1000)
    at, keep = 0, []
    for j, s in enumerate(PLAN_SIZES):
        vks, sigs, msgs = _cols(votes_4100[at:at + s])
        vk, sg = to_dev(b"".join(vks)), to_dev(b"".join(sigs))
        if j == 1:                       # one piece prehashed, the others with their messages
            k = to_dev(b"".join(ks_4100[at:at + s]))
            keep += [vk, sg, k]
            torch.cuda.synchronize()
            sv.queue_device(s, vk.data_ptr(), sg.data_ptr(), d_k=k.data_ptr())
        else:
            mg = to_dev(b"".join(msgs))
            offs = [0]
            for m in msgs:
                offs.append(offs[-1] + len(m))
            off = torch.tensor(offs, dtype=torch.int64, device=dev)
            keep += [vk, sg, mg, off]
            torch.cuda.synchronize()
            sv.queue_device(s, vk.data_ptr(), sg.data_ptr(), mg.data_ptr(), off.data_ptr())
        at += s
    _check_plan(sv, ref_4100)


# 6. protocol
def test_begin_eager_needs_an_empty_queue(edc, sv_factory):
    sv = sv_factory(seed=None)
    assert not sv.eager
    _queue(sv, _items(BY_NAME["one_valid"]))
    with pytest.raises(edc.EngineError):
        sv.begin_eager(SEED)
    assert not sv.eager
    b = BY_NAME["one_valid"]
    assert sv.verify_detailed(bytes.fromhex(b["z_seed"])) == _expect(b)


def test_eager_verify_takes_no_z(edc, engine, sv_factory):
    b = BY_NAME["batch_verify_32"]
    sv = sv_factory(seed=bytes.fromhex(b["z_seed"]), fold=8)
    _queue(sv, _items(b))
    with pytest.raises(ValueError):
        sv.verify_detailed(SEED)
    with pytest.raises(ValueError):
        sv.verify(random.Random(1))
    check8 = ctypes.create_string_buffer(32)
    assert engine.lib.edc_verifier_verify(sv._handle(), SEED, None, check8) == EDC_ERR_ARG
    assert engine.lib.edc_verifier_verify(sv._handle(), None, bytes(16 * 32), check8) == EDC_ERR_ARG
    assert sv.verify_detailed() == _expect(b)


def test_non_eager_null_null_is_still_an_argument_error(engine, sv_factory):
    sv = sv_factory(seed=None)
    _queue(sv, _items(BY_NAME["one_valid"]))
    check8 = ctypes.create_string_buffer(32)
    assert engine.lib.edc_verifier_verify(sv._handle(), None, None, check8) == EDC_ERR_ARG


def test_verify_ok_queue_more_verify_again(engine, sv_factory, votes_ok, votes_4100):
    first, more = votes_ok[:600], votes_4100[2980:3030]          # the 50 more hold the wrong signature
    sv = sv_factory(fold=256)
    _queue_pieces(sv, first, [300, 300])
    assert sv.folded == (600, 2)
    assert sv.verify_detailed() == (0, IDENTITY)
    _queue(sv, more)
    assert sv.folded == (600, 2)
    exp = _reference(engine, first + more, SEED)
    assert exp[0] == 1 and exp[1] not in (IDENTITY, bytes(32))
    assert sv.verify_detailed() == exp


def test_failed_verify_spends_the_seed(edc, engine, sv_factory):
    b = BY_NAME["batch_verify_one_bad"]
    it = _items(b)
    sv = sv_factory(seed=bytes.fromhex(b["z_seed"]), fold=8)
    _queue(sv, it)
    assert sv.verify_detailed() == _expect(b)
    with pytest.raises(edc.EngineError):
        _queue(sv, it[:1])
    with pytest.raises(edc.EngineError):
        sv.verify_detailed()
    assert sv.batch_size == len(it)
    sv.reset()
    sv.begin_eager(SEED2)
    _queue(sv, it)
    exp = _reference(engine, it, SEED2)
    assert exp[0] == 1 and exp[1] != _expect(b)[1]
    assert sv.verify_detailed() == exp


def test_library_drawn_seed(edc, engine, sv_factory):
    it = _items(BY_NAME["repeated_keys_3"])
    sv = sv_factory(seed=None, fold=16)
    for _ in range(2):
        sv.begin_eager(None)
        _queue_pieces(sv, it, [40, 24])
        assert sv.folded == (64, 2)
        assert sv.verify_detailed() == (0, IDENTITY)
        sv.reset()
    always = edc.batch.StreamVerifier(engine, 0, eager=True)
    try:
        always.set_fold(16)
        for _ in range(2):
            assert always.eager
            _queue(always, it)
            assert always.folded == (64, 1)
            always.verify()
            always.reset()
    finally:
        always.close()


# 7. fallback: the eager verify, then the grouped fallback with the caller's seed
def test_verify_with_fallback(edc, engine, sv_factory, votes_ok):
    bad = [5, 2050, 3999]                                 # all inside folded ranges
    it = list(votes_ok)
    for i in bad:
        _break(it, i)
    plain = sv_factory(4100, seed=None)
    _queue_pieces(plain, it, PLAN_SIZES)
    exp_code, exp_verdicts, _ = plain.verify_with_fallback(SEED2)
    assert exp_code == 1 and [i for i, c in enumerate(exp_verdicts) if c] == bad
    sv = sv_factory(4100, fold=1000)
    _queue_pieces(sv, it, PLAN_SIZES)
    assert sv.folded == (4000, 2)
    code, verdicts, check8 = sv.verify_with_fallback(SEED2)
    assert (code, check8) == _reference(engine, it, SEED)
    assert verdicts == exp_verdicts
    # the seed is spent, the fallback still answers (with its own z)
    with pytest.raises(edc.EngineError):
        sv.verify_detailed()
    assert sv.verify_with_fallback(SEED2)[:2] == (1, exp_verdicts)
