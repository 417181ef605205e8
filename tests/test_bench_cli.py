"""CPU: bench.py's command line and its output dump (no GPU: nothing here reaches main())."""
import sys

import numpy as np
import pytest

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        parse(monkeypatch, *argv)


def test_dump_outputs_types(tmp_path):
    pooled = np.random.default_rng(0).standard_normal((4, 8), dtype=np.float32)
    ids = np.array([[3, 1], [2**40, 0]], np.int64)
    bench.dump_outputs(str(tmp_path / "d"), {"embed_pooled": pooled, "topk_ids": ids})
    a, b = np.load(tmp_path / "d" / "embed_pooled.npy"), np.load(tmp_path / "d" / "topk_ids.npy")
    assert a.dtype == np.float32 and np.array_equal(a, pooled)
    assert b.dtype == np.float64 and np.array_equal(b.astype(np.int64), ids)


def test_dump_outputs_stays_under_the_limit_with_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1 << 16)
    x = np.arange(4000 * 16, dtype=np.float32).reshape(4000, 16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "ids": np.arange(4000 * 2).reshape(4000, 2)})
    xa, ia = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "ids.npy")
    assert xa.nbytes + ia.nbytes <= 1 << 16
    assert np.array_equal(xa, np.load(tmp_path / "b" / "x.npy"))  # the same rows on every run
    rows = xa[:, 0].astype(np.int64) // 16
    assert np.all(np.diff(rows) > 0) and np.array_equal(xa, x[rows])  # whole rows, in order
