"""CPU: sc_diag_attention_run's descriptor rules and geometry, which run before the runtime is looked at (rt = NULL, no device).

A descriptor the harness serves fails with the NULL-runtime message alone; a bad one fails with its own status and message first."""
import ctypes as C

import numpy as np
import pytest

from semcode_amd import _native
from semcode_amd._native import ATTN_CAUSAL, ATTN_CLS, ATTN_FULL, ATTN_WINDOW

INVALID, UNSUPPORTED = -1, -4
LENS = np.array([32, 9], np.int32)
P_STARTS, P_LENS = np.array([0, 32], np.int32), np.array([1, 33], np.int32)  # the second sequence ends at row 96
SLOPES, REL = np.array([0.25, 0.0625, 0.5, 0.125], np.float32), np.zeros((32, 4), np.float32)
RECT = dict(B=2, S=32, lens=LENS)
PACKED = dict(B=2, starts=P_STARTS, lens=P_LENS)
REL_BIAS = dict(rel_bias=REL, rel_buckets=32, rel_max_distance=128)


def run(mask=ATTN_FULL, heads=2, head_dim=64, **fields):
    """(status, message) of one call with rt = NULL; qkv and out are never touched before the runtime is."""
    desc = _native.DiagAttn(mask=mask, heads=heads, head_dim=head_dim)
    for name, value in fields.items():
        setattr(desc, name, value.ctypes.data if isinstance(value, np.ndarray) else value)
    dummy = np.zeros(4, np.float32)
    st = _native.lib().sc_diag_attention_run(None, C.addressof(desc), _native._ptr(dummy), _native._ptr(dummy))
    buf = C.create_string_buffer(1024)
    _native.lib().sc_last_error(buf, 1024)
    return st, buf.value.decode()


VALID = {
    "rect": dict(RECT),
    "rect blocked": dict(RECT, blocked_rows=256),
    "rect head_dim 32": dict(RECT, heads=4, head_dim=32),
    "rect slopes": dict(RECT, slopes=SLOPES),
    "rect rel_bias": dict(RECT, **REL_BIAS),
    "packed": dict(PACKED),
    "packed blocked": dict(PACKED, blocked_rows=256),
    "packed head_dim 32": dict(PACKED, heads=4, head_dim=32),
    "packed rel_bias": dict(PACKED, **REL_BIAS),
    "window rect": dict(RECT, mask=ATTN_WINDOW, local_window=6),
    "window packed": dict(PACKED, mask=ATTN_WINDOW, local_window=128),
    "causal rect 2/1": dict(RECT, mask=ATTN_CAUSAL, kv_heads=1),
    "causal packed 1/1 of 128": dict(PACKED, mask=ATTN_CAUSAL, heads=1, kv_heads=1, head_dim=128),
    "cls": dict(RECT, mask=ATTN_CLS),
    "cls head_dim 32 slopes": dict(RECT, mask=ATTN_CLS, heads=4, head_dim=32, slopes=SLOPES, S=7),
}


@pytest.mark.parametrize("form", sorted(VALID))
def test_a_valid_descriptor_fails_on_the_null_runtime_alone(form):
    st, msg = run(**VALID[form])
    assert st == INVALID and "runtime is NULL" in msg, (st, msg)


BAD = [
    # what exists today: status and words as before
    (dict(RECT, mask=ATTN_CAUSAL, kv_heads=0), UNSUPPORTED, ("kv_heads",)),
    (dict(RECT, mask=ATTN_CAUSAL, heads=2, kv_heads=3), UNSUPPORTED, ("kv_heads",)),
    (dict(RECT, mask=ATTN_CAUSAL, heads=3, kv_heads=2), UNSUPPORTED, ("kv_heads",)),
    (dict(RECT, mask=ATTN_WINDOW, local_window=0), UNSUPPORTED, ("local_window",)),
    (dict(RECT, mask=ATTN_WINDOW, local_window=3), UNSUPPORTED, ("local_window",)),
    (dict(PACKED, mask=ATTN_WINDOW, local_window=130), UNSUPPORTED, ("local_window",)),
    (dict(RECT, head_dim=48), UNSUPPORTED, ("head_dim",)),
    (dict(PACKED, heads=3, head_dim=32), UNSUPPORTED, ("head_dim", "even")),
    (dict(RECT, heads=4, head_dim=32, slopes=SLOPES), UNSUPPORTED, ("head_dim 32", "slopes")),
    (dict(PACKED, heads=4, head_dim=32, slopes=SLOPES), UNSUPPORTED, ("head_dim 32", "slopes")),
    (dict(RECT, S=48), UNSUPPORTED, ("S must be",)),
    (dict(RECT, blocked_rows=32), INVALID, ("blocked_rows",)),
    (dict(RECT, heads=0), INVALID, ("heads",)),
    (dict(PACKED, heads=33), INVALID, ("2048",)),
    (dict(RECT, mask=ATTN_CLS, S=2049), INVALID, ("CLS", "S must be")),
    (dict(RECT, rel_bias=REL, rel_buckets=33, rel_max_distance=128), INVALID, ("rel_buckets",)),
    (dict(RECT, mask=4), INVALID, ("mask",)),
    (dict(RECT, lens=None), INVALID, ("lens",)),
    # what the descriptor can say and no launcher serves: the two fields are named
    (dict(RECT, mask=ATTN_WINDOW, local_window=6, slopes=SLOPES), UNSUPPORTED, ("mask 1", "slopes")),
    (dict(RECT, mask=ATTN_CAUSAL, kv_heads=1, slopes=SLOPES), UNSUPPORTED, ("mask 2", "slopes")),
    (dict(RECT, mask=ATTN_WINDOW, local_window=6, heads=4, head_dim=32), UNSUPPORTED, ("window", "head_dim")),
    (dict(RECT, heads=4, head_dim=32, **REL_BIAS), UNSUPPORTED, ("rel_bias", "head_dim")),
    (dict(RECT, slopes=SLOPES, **REL_BIAS), UNSUPPORTED, ("rel_bias", "slopes")),
    (dict(RECT, mask=ATTN_WINDOW, local_window=6, **REL_BIAS), UNSUPPORTED, ("rel_bias", "mask")),
    (dict(RECT, mask=ATTN_CAUSAL, kv_heads=1, **REL_BIAS), UNSUPPORTED, ("rel_bias", "mask")),
    (dict(RECT, mask=ATTN_CLS, **REL_BIAS), UNSUPPORTED, ("rel_bias", "mask")),
    (dict(PACKED, mask=ATTN_CLS, S=32), UNSUPPORTED, ("CLS", "starts")),
    (dict(RECT, mask=ATTN_CLS, blocked_rows=256), UNSUPPORTED, ("CLS", "blocked_rows")),
    (dict(RECT, mask=ATTN_CAUSAL, heads=4, kv_heads=2, head_dim=32), UNSUPPORTED, ("causal", "head_dim")),
    (dict(RECT, kv_heads=1), UNSUPPORTED, ("kv_heads", "mask")),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_a_bad_descriptor_fails_with_its_own_status_and_message(i):
    fields, status, words = BAD[i]
    st, msg = run(**fields)
    assert st == status and all(w in msg for w in words) and "runtime" not in msg, (fields, st, msg)


@pytest.mark.parametrize("change, word", [
    (dict(starts=np.array([0, 16], np.int32)), "start 16"),
    (dict(lens=np.array([1, 0], np.int32)), "length 0"),
    (dict(lens=np.array([1, 2049], np.int32)), "length 2049"),
    (dict(blocked_rows=64), "blocked_rows 64 < the last sequence's end 96"),
    (dict(B=0), "B 1 .. 65536"),
])
@pytest.mark.parametrize("mask", [dict(), dict(mask=ATTN_WINDOW, local_window=6), dict(mask=ATTN_CAUSAL, kv_heads=2)])
def test_packed_geometry_is_refused(mask, change, word):
    st, msg = run(**dict(PACKED, **mask, **change))
    assert st == INVALID and word in msg and "runtime" not in msg, (st, msg)


def test_python_helper_rows_and_shapes():
    assert _native._diag_attention_rows(P_STARTS, P_LENS) == 256
    assert _native._diag_attention_rows(P_STARTS, P_LENS, blocked_rows=512) == 512
    assert _native._diag_attention_rows(None, LENS, S=32) == 64
    for call in (lambda q: _native.diag_attention_packed(None, q, P_STARTS, P_LENS, 2),
                 lambda q: _native.diag_attention_window(None, q, P_LENS, 2, 6, starts=P_STARTS),
                 lambda q: _native.diag_attention_bias_packed(None, q, P_STARTS, P_LENS, 2, REL[:, :2], 128)):
        with pytest.raises(ValueError, match=r"\[256, 384\]"):
            call(np.zeros((128, 384), np.float32))
        with pytest.raises(_native.ScError, match="runtime is NULL"):  # the right shape reaches the library
            call(np.zeros((256, 384), np.float32))
    with pytest.raises(ValueError):
        _native.diag_attention_causal(None, np.zeros((64, 384), np.float32), LENS, 2, 1, S=32)  # (2 + 2 * 1) * 64 = 256 columns
    with pytest.raises(_native.ScError, match="runtime is NULL"):  # a rectangle's B * S rows are padded to blocked_rows here
        _native.diag_attention_ex(None, np.zeros((64, 384), np.float32), LENS, 2, 32, 2, blocked_rows=256)
