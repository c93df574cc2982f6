"""GPU: the MSM's counting sort and segmented accumulation (edc_msm.hip k_msm_sort, sorted_slot /
acc_lane_of, k_msm_accum_dma: head0, the flush at a bucket end, the walk over empty buckets,
owns_open / continues, the head merge after the barrier) on bins whose occupancy the test chooses
through caller-drawn z (tests/bucket_shapes.py; the same cases are asserted without a GPU by
tests/test_bucket_shape_census.py). Every other GPU test draws near-uniform digits.

Each case sets a plan, asserts it from Engine.last_plan() after the call, recomputes the census from
that reported plan and asserts the shape the case exists for, then compares three entry points
exactly with [-sum z_i delta_i]B from big-integer arithmetic: the host call, the device call with
d_z, and submit + wait with the affine check point before the cofactor. Three variants per case: the
valid batch (identity), one defect inside the longest bucket, one defect in the last item. The base
items are signed by the engine and accepted one by one by the C oracle before use. Everything is
integer arithmetic: all comparisons are for equality."""
import ctypes

import pytest

from conftest import ROOT

import bucket_shapes as bs

pytestmark = pytest.mark.gpu

P = 2**255 - 19


@pytest.fixture(scope="module")
def oracle_c():
    import os
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c as oc
    return oc


@pytest.fixture(scope="module")
def signed(engine, oracle_c):
    """(base items [(vk, sig, k)], their messages): at most 512 items over 8 keys, messages of 0..90
    bytes, each accepted by the C oracle."""
    seeds, msgs, idx = bs.signing_inputs()
    vks, sigs = engine.sign(seeds, msgs, seed_index=idx)
    assert len(vks) == bs.NBASE <= 512 and len(set(vks)) == bs.NKEYS
    for vk, sig, m in zip(vks, sigs, msgs):
        assert oracle_c.verify(vk, sig, m) == 0
    return bs.prehash(vks, sigs, msgs), msgs


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


def _cols(items):
    return [v for v, _, _ in items], [s for _, s, _ in items], [k for _, _, k in items]


def _zbytes(z):
    return b"".join(zi.to_bytes(16, "little") for zi in z)


def _affine(partial):
    X, Y, Z = (int.from_bytes(partial[32 * i:32 * i + 32], "little") for i in range(3))
    zi = pow(Z, P - 2, P)
    return (X * zi % P).to_bytes(32, "little"), (Y * zi % P).to_bytes(32, "little")


def _device(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda:0"))


def _checked(engine, case, items, z, shape_too):
    """The plan of the call just made is the case's, and (once per case) the bins have its shape."""
    plan = engine.last_plan()
    case.check_plan(plan)
    if shape_too:
        case.prop(case, plan, bs.census(plan, case.terms(items, z)))
    return plan


@pytest.mark.parametrize("name", [c.name for c in bs.CASES])
def test_bucket_shape(knobs, signed, name):
    torch = pytest.importorskip("torch")
    base, base_msgs = signed
    case = bs.BY_NAME[name]
    lib = knobs.lib
    knobs.set_key_grouping(case.grouping)
    if case.shape:
        knobs.set_msm_shape(*case.shape)
    else:
        knobs.set_msm_bin_entries(case.entries)
    for tag, items, z, defects in bs.variants(case, base):
        code, c8, xy = bs.expected(z, defects)
        exp = (code, c8)
        assert code == (1 if defects and z[next(iter(defects))] else 0)
        vks, sigs, ks = _cols(items)
        zb = _zbytes(z)
        if case.split and tag == "clean":
            # registered once; the one-call path plans its split from the previous batch
            u, ok = knobs.keycache_load(list(dict.fromkeys(vks)))
            assert u == bs.NKEYS and all(ok)
            assert knobs.batch_verify_prehashed(vks, sigs, ks, z=zb, want_check8=True) == exp, (name, tag)
        # the host call
        got = knobs.batch_verify_prehashed(vks, sigs, ks, z=zb, want_check8=True)
        plan = _checked(knobs, case, items, z, tag == "clean")
        assert got == exp, (name, tag, plan)
        if case.msgs:                                   # the message entry feeds the same MSM
            msgs = bs.tile(base_msgs, case.n)
            assert knobs.batch_verify(vks, sigs, msgs, z=zb, want_check8=True) == exp, (name, tag)
            _checked(knobs, case, items, z, False)
        # the device call with d_z
        d = [_device(torch, b"".join(x)) for x in (vks, sigs, ks)]
        d_z = _device(torch, zb)
        torch.cuda.synchronize()
        ptr = [t.data_ptr() for t in d]
        out = ctypes.create_string_buffer(32)
        rc = lib.edc_batch_verify_prehashed_device(knobs.ctx, case.n, *ptr, None, 0, d_z.data_ptr(), out)
        _checked(knobs, case, items, z, False)
        assert (rc, out.raw) == exp, (name, tag)
        # submit + wait: the check point before the cofactor
        t = lib.edc_batch_submit_prehashed_device(knobs.ctx, case.n, *ptr, None, 0, d_z.data_ptr(), 1)
        assert t >= 0, (name, tag)
        out, part, bad = ctypes.create_string_buffer(32), ctypes.create_string_buffer(128), ctypes.c_int(-1)
        rc = lib.edc_batch_wait(knobs.ctx, t, out, part, ctypes.byref(bad))
        plan = _checked(knobs, case, items, z, False)
        assert (rc, out.raw) == exp and bad.value == 0, (name, tag)
        assert _affine(part.raw) == xy, (name, tag)

