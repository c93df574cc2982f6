"""bench.py's plain run, --full and --dump-outputs.

A plain run prints the headline line and nothing that needs runs of its own; --full adds the
instrumented batches, the host-buffer calls and the CPU baseline; --dump-outputs writes what the
timed path returned, in a form that is the same from run to run.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

P = 2 ** 255 - 19
# the Ed25519 base point (RFC 8032, 5.1)
BX = 15112221349535400772501151409588531511454012693041857206046113283949847762202
BY = 46316835694926478169428394003475163141307993866256225615783033603165251855960
FULL_ONLY = ("roofline", "roofline_sha512", "roofline_msm_accum", "hbm_view", "phases_ms", "batch_latency_ms",
             "host_api", "cpu_baseline")
# scaling_other_shape is in every line (tools/*_ab.sh read it from both kinds of run): None unless measured
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup",
            "scaling_other_shape")


def _last(part=None, bad=0, verdicts=None, rank_partial=None):
    buf = ctypes.create_string_buffer(128)
    if part is not None:
        buf.raw = part
    return {"partial": buf, "bad": None, "bad_int": ctypes.c_int(bad), "verdicts": verdicts,
            "rank_partial": rank_partial}


def _projective(x, y, z):
    return b"".join((v % P).to_bytes(32, "little") for v in (x * z, y * z, z, x * y * z))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_is_independent_of_the_projective_representative(tmp_path):
    outs = []
    for i, z in enumerate((1, 2, P - 5, 0x1234567890abcdef ** 3)):
        d = str(tmp_path / f"z{i}")
        bench.dump_outputs(d, [0, 0, 1], _last(_projective(BX, BY, z), bad=0))
        outs.append(_load(d))
    for o in outs:
        assert sorted(o) == ["bad", "check_point", "verdicts"]
        assert all(a.dtype == np.float64 for a in o.values())
        assert o["verdicts"].tolist() == [0, 0, 1] and o["bad"].tolist() == [0]
        assert bytes(int(v) for v in o["check_point"]) == BX.to_bytes(32, "little") + BY.to_bytes(32, "little")


def test_dump_outputs_multi_rank_and_multi_batch(tmp_path):
    d = str(tmp_path / "rank")
    bench.dump_outputs(d, [0], _last(rank_partial=(_projective(0, 1, 77), 1)))
    o = _load(d)
    # rank 0's own shard partial, not the combined record: named so
    assert sorted(o) == ["shard0_bad", "shard0_check_point", "verdicts"]
    assert o["shard0_bad"].tolist() == [1]
    assert bytes(int(v) for v in o["shard0_check_point"]) == bytes(32) + (1).to_bytes(32, "little")
    d = str(tmp_path / "multi")
    bench.dump_outputs(d, [0, 0], _last(verdicts=[0, 0, 1, 0]))
    o = _load(d)
    assert sorted(o) == ["launch_verdicts", "verdicts"]
    assert o["launch_verdicts"].tolist() == [0, 0, 1, 0]


def test_dump_outputs_skips_a_record_that_is_no_point(tmp_path):
    """Z = 0 (a probe build loaded with --lib may return it): the run goes on to its result line."""
    d = str(tmp_path / "z0")
    bench.dump_outputs(d, [1], _last(bytes(128), bad=0))
    assert sorted(_load(d)) == ["bad", "verdicts"]


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "4096", "--steps", "3",
                        "--warmup", "1", *argv], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_the_same_outputs_twice(tmp_path):
    lines = [_bench("--dump-outputs", str(tmp_path / name)) for name in ("a", "b")]
    for line in lines:
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
        # ms_per_step (3 decimals) is the time of one timed step: value = signatures per step / that time
        assert abs(line["ms_per_step"] - 4096 / line["value"] * 1e3) <= 1e-3
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) == ["bad", "check_point", "verdicts"]
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    # a valid batch: every timed step's verdict is Ok, the check point is the identity (0, 1)
    assert a["verdicts"].tolist() == [0, 0, 0] and a["bad"].tolist() == [0]
    assert bytes(int(v) for v in a["check_point"]) == bytes(32) + (1).to_bytes(32, "little")


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    line = _bench("--full", "--cpu-sample", "4096")
    assert all(k in line for k in HEADLINE + FULL_ONLY)
    assert line["full"] is True
    assert set(line["phases_ms"]) >= {"challenge_sha512", "decompress_R", "msm_bucket"}
    assert line["host_api"]["prehashed"]["sigs_per_s"] > 0
    assert line["cpu_baseline"]["ok"] is True and "openssl_anchor" in line["cpu_baseline"]
