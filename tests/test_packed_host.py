"""CPU: the host side of packed variable-length batches that needs no device.

The plan of a packed call -- the rules of its offsets, the row count, every array it uploads -- is host arithmetic of plain values
(semcode_amd/csrc/sc_encoder_plan.cpp) and is checked through diag_encoder_plan in tests/test_encoder_plan_host.py; sc_encoder_packed_rows
itself takes an encoder handle, which needs a device (tests/test_packed_gpu.py).  Here: the cutter the provider sizes its packed calls with,
the flattening of a padded batch, the ABI entries and the setting."""
import numpy as np
import pytest

from semcode_amd.embeddings.providers import cut_packed, flatten_ids


def rows_of(lens):
    """Stand-in for Encoder.packed_rows in the cutter tests -- the library's rule (include/semcode_hip.h): ceil32 per text, the total
    rounded up to 256.  test_rows_of_is_the_librarys_count holds it against the library's plan."""
    used = int(((np.asarray(lens, np.int64) + 31) // 32 * 32).sum())
    return (used + 255) // 256 * 256


def test_rows_of_is_the_librarys_count():
    from semcode_amd._native import diag_encoder_plan

    rng = np.random.default_rng(0)  # the lens of test_cutter_groups_are_consecutive_and_within_budget, seed 0
    lens = np.concatenate([rng.integers(1, 300, size=200), [2048, 1, 2048, 2048, 31, 33], rng.integers(1, 2049, size=50)])
    rng.shuffle(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)])
    plan = diag_encoder_plan(np.zeros(int(offsets[-1]), np.int32), offsets)
    assert int(plan["M"][0]) == rows_of(lens)


@pytest.mark.parametrize("budget", [256, 1024, 4096, 65536])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cutter_groups_are_consecutive_and_within_budget(seed, budget):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(1, 300, size=200), [2048, 1, 2048, 2048, 31, 33], rng.integers(1, 2049, size=50)])
    rng.shuffle(lens)
    groups = cut_packed(lens, budget, rows_of)
    assert groups[0][0] == 0 and groups[-1][1] == len(lens)
    for (a, b), (a2, _) in zip(groups, groups[1:] + [(len(lens), None)]):
        assert a < b and b == a2  # consecutive, none empty, nothing skipped
        assert rows_of(lens[a:b]) <= budget or b == a + 1  # over budget only when a single text alone is
        if b < len(lens):
            assert rows_of(lens[a:b + 1]) > budget  # greedy: the next text did not fit


def test_cutter_edges():
    assert cut_packed([], 1024, rows_of) == []
    assert cut_packed([5], 1024, rows_of) == [(0, 1)]
    assert cut_packed([2048, 2048], 1024, rows_of) == [(0, 1), (1, 2)]  # each alone exceeds the budget
    assert cut_packed([32] * 64, 1024, rows_of) == [(0, 32), (32, 64)]  # exactly at the budget
    calls = []
    cut_packed([100] * 1000, 65536, lambda l: calls.append(len(l)) or rows_of(l))
    assert len(calls) <= 40  # bisection, not one planner call per text


def test_flatten_ids_drops_the_padding():
    ids = np.array([[5, 6, 7, 0], [8, 0, 0, 0], [1, 2, 3, 4]], np.int32)
    flat, offsets = flatten_ids(ids, np.array([3, 1, 4], np.int32))
    assert flat.dtype == np.int32 and flat.tolist() == [5, 6, 7, 8, 1, 2, 3, 4]
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 3, 4, 8]


def test_abi_has_the_packed_entries():
    import ctypes

    from semcode_amd import _native
    from semcode_amd.csrc import build

    names = ["sc_encoder_packed_rows", "sc_encoder_embed_packed", "sc_encoder_embed_packed_into", "sc_encoder_embed_packed_into_async",
             "sc_diag_attention_run"]
    handle = ctypes.CDLL(str(build.build(verbose=False)))
    for n in names:
        assert n in _native.SIGNATURES and hasattr(handle, n), n
    # NULL handles are argument errors with a message, also without a device
    lib = _native.lib()
    rows = ctypes.c_int64(-7)
    off = np.array([0, 4], np.int64)
    assert lib.sc_encoder_packed_rows(None, off.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(rows)) == -1 and rows.value == -7
    buf = ctypes.create_string_buffer(512)
    lib.sc_last_error(buf, 512)
    assert b"sc_encoder_packed_rows" in buf.value
    assert lib.sc_encoder_embed_packed(None, None, None, 1, None) == -1


def test_setting_defaults_to_padded(monkeypatch):
    from semcode_amd.settings import Settings

    assert Settings().mi355x_packed is False
    monkeypatch.setenv("SEMCODE_MI355X_PACKED", "1")
    assert Settings().mi355x_packed is True
