"""GPU: every form of the attention harness (sc_diag_attention_run behind the diag_attention* wrappers) at the smallest shapes that go
through its shared staging, hidden 128.  No reference and no tolerance: the parity tests of each family hold the values.  Here the NaN
contract of include/semcode_hip.h -- outputs are pre-filled with NaN, every row of a sequence comes back finite, packed rows outside
every sequence stay NaN -- and the two layouts of qkv, row-major and 64-column blocks, agreeing bit for bit."""
import numpy as np
import pytest

from semcode_amd import _native as nv

pytestmark = pytest.mark.gpu

B, S, LENS = 2, 32, np.array([32, 9], np.int32)
P_STARTS, P_LENS, P_ROWS, P_END = np.array([0, 32], np.int32), np.array([1, 33], np.int32), 256, 96  # rows 0 .. 31 and 32 .. 95 are owned
SLOPES2, SLOPES4 = np.array([0.25, 0.0625], np.float32), np.array([0.25, 0.0625, 0.5, 0.125], np.float32)
REL = (0.1 * np.random.default_rng(1).standard_normal((32, 2))).astype(np.float32)  # T5: 32 buckets, max_distance 128

# form -> (qkv columns, out columns, rectangle call, packed call); each call takes (rt, qkv, blocked_rows)
FORMS = {
    "plain": (384, 128, lambda rt, q, bl: nv.diag_attention(rt, q, LENS, B, S, 2, blocked_rows=bl),
              lambda rt, q, bl: nv.diag_attention_packed(rt, q, P_STARTS, P_LENS, 2, blocked_rows=bl)),
    "alibi": (384, 128, lambda rt, q, bl: nv.diag_attention_ex(rt, q, LENS, B, S, 2, blocked_rows=bl, slopes=SLOPES2),
              lambda rt, q, bl: nv.diag_attention_packed(rt, q, P_STARTS, P_LENS, 2, blocked_rows=bl, slopes=SLOPES2)),
    "head_dim 32": (384, 128, lambda rt, q, bl: nv.diag_attention_ex(rt, q, LENS, B, S, 4, blocked_rows=bl, head_dim=32),
                    lambda rt, q, bl: nv.diag_attention_packed(rt, q, P_STARTS, P_LENS, 4, blocked_rows=bl, head_dim=32)),
    "rel_bias": (384, 128, lambda rt, q, bl: nv.diag_attention_bias(rt, q, LENS, B, S, 2, REL, 128, blocked_rows=bl),
                 lambda rt, q, bl: nv.diag_attention_bias_packed(rt, q, P_STARTS, P_LENS, 2, REL, 128, blocked_rows=bl)),
    "window 6": (384, 128, lambda rt, q, bl: nv.diag_attention_window(rt, q, LENS, 2, 6, S=S, blocked_rows=bl),
                 lambda rt, q, bl: nv.diag_attention_window(rt, q, P_LENS, 2, 6, starts=P_STARTS, blocked_rows=bl)),
    "causal 2/1 of 64": (256, 128, lambda rt, q, bl: nv.diag_attention_causal(rt, q, LENS, 2, 1, S=S, blocked_rows=bl),
                         lambda rt, q, bl: nv.diag_attention_causal(rt, q, P_LENS, 2, 1, starts=P_STARTS, blocked_rows=bl)),
    "causal 1/1 of 128": (384, 128, lambda rt, q, bl: nv.diag_attention_causal(rt, q, LENS, 1, 1, S=S, blocked_rows=bl, head_dim=128),
                          lambda rt, q, bl: nv.diag_attention_causal(rt, q, P_LENS, 1, 1, starts=P_STARTS, blocked_rows=bl, head_dim=128)),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_nan_contract_and_layouts(rt, form):
    cols, H, rect, packed = FORMS[form]
    rng = np.random.default_rng(len(form))
    q = rng.standard_normal((B * S, cols)).astype(np.float32)
    row = rect(rt, q, 0)
    assert row.shape == (B * S, H) and np.isfinite(row).all()  # rows at or beyond a text's length are queries too (window: zero)
    blocked = rect(rt, np.concatenate([q, np.zeros((256 - B * S, cols), np.float32)]), 256)
    assert blocked.shape == row.shape and np.array_equal(bits(blocked), bits(row))

    q = rng.standard_normal((P_ROWS, cols)).astype(np.float32)
    row = packed(rt, q, 0)
    assert row.shape == (P_ROWS, H)
    assert np.isfinite(row[:P_END]).all() and np.isnan(row[P_END:]).all()
    assert np.array_equal(bits(packed(rt, q, P_ROWS)), bits(row))


@pytest.mark.parametrize("heads, head_dim, slopes", [(2, 64, None), (2, 64, SLOPES2), (4, 32, None), (4, 32, SLOPES4)])
def test_cls_rows(rt, heads, head_dim, slopes):
    """The CLS form: one row per text (the harness lays the 64 rows out in blocks of 256 itself)."""
    q = np.random.default_rng(heads).standard_normal((B * S, 384)).astype(np.float32)
    out = nv.diag_attention_cls(rt, q, LENS, B, S, heads, head_dim=head_dim, slopes=slopes)
    assert out.shape == (B, 128) and np.isfinite(out).all()
