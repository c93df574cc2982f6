"""CPU: the helper behind tests/test_gpu_bucket_shapes.py (tests/bucket_shapes.py). The defect formula
check = [-sum z_i delta_i]B is compared with the big-integer oracle's batch equation on signed
batches, and for every case of the GPU test the census shows, from the plan alone, that the chosen z
put the bins into the shape the case is named for: these assertions are what "the input reaches the
edge" means, so a later change of a size that loses an edge fails here, without a GPU."""
import pytest

import bucket_shapes as bs
import scalar_edges as se

o = se.o


@pytest.fixture(scope="module")
def signed():
    """The base list, signed on the CPU, with its messages."""
    vks, sigs, msgs = bs.sign_reference()
    return bs.prehash(vks, sigs, msgs), msgs


@pytest.fixture(scope="module")
def base(signed):
    return signed[0]


# ---------------------------------------------------------------- the expected value
def test_reference_signer_is_the_oracles(signed):
    base, msgs = signed
    seeds, _, idx = bs.signing_inputs(16)
    for i in (0, 1, 7, 15):
        assert base[i][1] == o.sign(seeds[idx[i]], msgs[i]) and base[i][0] == o.public_key(seeds[idx[i]])
    assert sorted({len(m) for m in msgs}) == list(range(91)) and len({vk for vk, _, _ in base}) == bs.NKEYS


def _oracle(items, msgs_of, z):
    return o.batch_verify([(vk, sig, msgs_of[vk, sig[:32]]) for vk, sig, _ in items], z)


@pytest.mark.parametrize("family", ["zipf", "one_max"])
def test_defect_formula_matches_the_oracle(signed, family):
    """Clean, one defect, three defects, with a repeat inside; code and [8]*check."""
    base, msgs = signed
    n = 24
    items = bs.tile(base[:20], n)                       # items 20..23 repeat 0..3
    msgs_of = {(vk, sig[:32]): m for (vk, sig, _), m in zip(base, msgs)}
    wins = bs.short_wins(9)
    z = bs.zipf(n, wins) if family == "zipf" else bs.one_bucket(n, bs.d_max, wins)
    for defects in ({}, {5: 7}, {0: 1, 11: se.L - 2, 23: 1 << 200}):
        bad = bs.with_defects(items, defects)
        code, c8, xy = bs.expected(z, defects)
        assert (code, c8) == _oracle(bad, msgs_of, z), (family, defects)
        assert code == (1 if defects else 0)
        pt = se.batch_check(bad, z)                     # the prehashed equation, before the cofactor
        assert tuple(se.sc(v) for v in se.affine(pt)) == xy, (family, defects)


@pytest.mark.parametrize("family", ["zipf", "one_mid"])
def test_negated_twin_and_torsion_keep_the_formula(base, family):
    """Twins carry -k, which no message hashes to: the prehashed equation is the reference."""
    items = []
    for it in base[:8]:
        tw = bs.negated_twin(it)
        assert tw is not None and o.verify_prehashed(tw[0], tw[1], int.from_bytes(tw[2], "little")) == o.OK
        items += [it, tw]
    tors = bs.torsion_item()
    assert o.verify_prehashed(tors[0], tors[1], 1) == o.OK
    wins = bs.short_wins(13)
    if family == "zipf":
        items, z = items + [tors], bs.zipf(17, wins)    # z of the torsion item may leave a torsion part
        z[16] &= ~7
    else:
        items, z = items + [tors] * 8, bs.one_bucket(24, bs.d_mid, wins)
    for defects in ({}, {3: 9}):
        bad = bs.with_defects(items, defects)
        code, c8, xy = bs.expected(z, defects)
        pt = se.batch_check(bad, z)
        assert tuple(se.sc(v) for v in se.affine(pt)) == xy and o.compress(o.mul_by_cofactor(pt)) == c8
        assert code == (0 if o.is_identity(o.mul_by_cofactor(pt)) else 1)


# ---------------------------------------------------------------- the census
def test_bin_stats_on_hand_made_bins():
    c = [0] * 256
    c[7] = 256
    s = bs.bin_stats(c)
    assert (s["E"], s["occupied"], s["max_lanes"], s["empty_inside"], s["crossed"]) == (256, 1, 256, 0, 0)
    c = [0] * 256
    c[200] = 100                                        # 100 lanes of one entry among 256
    s = bs.bin_stats(c)
    assert (s["max_lanes"], s["empty_inside"], s["ends"]) == (100, 156, set())
    c = [0] * 256
    c[0], c[255] = 512, 512                             # lanes of 4: the boundary is lane 128's start
    s = bs.bin_stats(c)
    assert s["ends"] == {(0, 4)} and s["crossed"] == 0 and s["max_lanes"] == 128
    c[0], c[255] = 513, 511
    s = bs.bin_stats(c)
    assert s["ends"] == {(1, 3)} and s["crossed"] == 254
    c[0], c[255] = 511, 513
    assert bs.bin_stats(c)["ends"] == {(3, 1)}


def test_census_matches_a_direct_count():
    """census() against a second, direct reading of the rule on a small plan with parts."""
    plan = bs.plan_dict(11, 11, 16)
    assert (plan["nranges"], plan["sum_ranges"], plan["bins_per_range"]) == (16, 1, 78)
    z = bs.zipf(40, bs.short_wins(11), "direct")
    tl = [(se.L - 5, False)] + [(v, True) for v in z] + [((1 << 252) + 3, False)]
    bins = bs.census(plan, tl)
    assert sum(sum(v) for v in bins.values()) == sum(1 for s, sh in tl for d in
                                                     se.plan_digits(s, bs.plan_wins(plan)[:12] if sh else bs.plan_wins(plan))[0] if d)
    assert {k[0] for k in bins} == set(range(16)) and all(k[3] == 0 for k in bins)


@pytest.mark.parametrize("name", [c.name for c in bs.CASES])
def test_case_reaches_its_shape(base, name):
    case = bs.BY_NAME[name]
    items, z, long_pos = bs.build(case, base)
    assert all(0 <= zi <= se.M128 for zi in z) and (z[long_pos] or not any(z))
    for plan in case.cpu_plans():
        assert bs.census_exact(plan, case.per_sig)
        case.prop(case, plan, bs.census(plan, case.terms(items, z)))


def test_the_case_list_covers_every_edge():
    """The sizes, plans and reduction regimes the GPU test is meant to run, as a list one can read."""
    names = set(bs.BY_NAME)
    assert {"one_mid_c16_n%d" % n for n in (1, 2, 3, 100, 255, 256, 257)} <= names
    assert {"two_c16_on", "two_c16_after", "two_c16_before", "all_zero_c9_n64", "comb_auto_n4096", "big_c16_one",
            "big_c16_zipf", "cancel_c9_n128", "repeat_c9_n64", "torsion_c9_n64"} <= names
    assert {c.shape for c in bs.CASES} == {(8, 1), (9, 1), (13, 1), (16, 1), (11, 16), None}
    assert sum(c.n > 10240 for c in bs.CASES) == 2 and sum(c.grouping == 2 for c in bs.CASES) == 3
    assert sum(c.split for c in bs.CASES) == 1 and sum(c.msgs for c in bs.CASES) == 1
    regimes = {}
    for c in bs.CASES:
        p = c.cpu_plans()[0]
        regimes.setdefault(bs.reduce_regime(p["bins_per_range"] * p["nranges"]), []).append(c.name)
    assert set(regimes) == {"quad", "lanes64", "lanes32"}, regimes
