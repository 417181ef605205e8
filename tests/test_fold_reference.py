"""CPU: the float64 stage references of tests/fold_ref.py, which tests/test_fold_kernels_gpu.py holds every kernel against.

Pins them without a GPU: the folded algebra the kernels use equals the plain LayerNorm form; the stages chained in the order of
forward_folded_locked (embed-raw -> LNA QKV -> attention -> RESLN -> LNA GELU -> RESLN -> pool-LN) reproduce
oracle.bert_oracle.forward, itself pinned against transformers' BertModel; the layout helpers round-trip.
"""
import numpy as np
import pytest

import fold_ref as fr
from oracle import bert_oracle as bo
from semcode_amd import _native


def test_folded_identity_equals_the_plain_layernorm_form():
    """rs (A W'^T - mu c1) + c2 with W' = W diag(gamma), c1 = W' 1, c2 = b + W beta is LayerNorm(A; gamma, beta) W^T + b."""
    rng = np.random.default_rng(0)
    M, N, K, eps = 40, 24, 512, 1e-12
    A = rng.standard_normal((M, K)) + rng.uniform(-8, 8, (M, 1))
    W = rng.standard_normal((N, K)) / np.sqrt(K)
    g, be, b = rng.standard_normal(K), rng.standard_normal(K), rng.standard_normal(N)
    plain = fr.lna_plain(A, W, g, be, b, eps)
    Wf, c1, c2 = W * g, (W * g).sum(1), b + W @ be
    fin = fr.finalise(fr.slot_stats(A), K, eps)
    folded = fin[:, 1:2] * (A @ Wf.T - fin[:, 0:1] * c1) + c2
    assert np.abs(folded - plain).max() <= 1e-9 * max(1.0, np.abs(plain).max())
    assert np.abs(fr.lna_with_folded_weight(A, Wf, c2, eps) - plain).max() <= 1e-9 * max(1.0, np.abs(plain).max())
    assert np.abs(fr.lna_with_folded_weight(A, Wf, c2, eps, "gelu") - fr.gelu(plain)).max() <= 1e-9


@pytest.mark.parametrize("switches", [dict(), dict(alibi=True)])
def test_staged_references_chained_reproduce_the_oracle_forward(switches):
    cfg = dict(bo.BERT_BASE, vocab=97, hidden=256, layers=3, heads=4, ffn=512, max_pos=32, **switches)
    H, eps = cfg["hidden"], cfg["ln_eps"]
    blob = bo.make_blob(cfg, 3, "test")
    W = {k: v.astype(np.float64) for k, v in bo.unpack(cfg, blob).items()}
    rng = np.random.default_rng(1)
    B, S = 5, 32
    ids = rng.integers(0, 97, (B, S))
    lens = np.array([32, 1, 17, 31, 8])
    want = bo.forward(cfg, blob, ids, lens, out_dtype=np.float64)

    slopes = bo.alibi_slopes(cfg["heads"]) if switches.get("alibi") else None
    x = fr.embed_sum(ids, W["word_emb"], W.get("pos_emb"), W["type_emb"], cfg["max_pos"])  # raw rows
    gp, bp = W["emb_ln_g"], W["emb_ln_b"]                                                    # the LayerNorm in front of the layer
    for l in range(cfg["layers"]):
        p = f"l{l}."
        wqkv = np.concatenate([W[p + "wq"], W[p + "wk"], W[p + "wv"]])
        bqkv = np.concatenate([W[p + "bq"], W[p + "bk"], W[p + "bv"]])
        qkv = fr.lna_plain(x, wqkv, gp, bp, bqkv, eps)
        ctx = fr.attention(qkv, lens, B, S, cfg["heads"], slopes)
        y = fr.resln(ctx, W[p + "wo"], W[p + "bo"] + bp, gp, x, eps)
        hm = fr.lna_plain(y, W[p + "w1"], W[p + "ln1_g"], W[p + "ln1_b"], W[p + "b1"], eps, "gelu")
        x = fr.resln(hm, W[p + "w2"], W[p + "b2"] + W[p + "ln1_b"], W[p + "ln1_g"], y, eps)
        gp, bp = W[p + "ln2_g"], W[p + "ln2_b"]
    got = fr.mean_pool_ln(x, gp, bp, eps, lens, S)
    assert np.abs(got - want).max() <= 1e-9, np.abs(got - want).max()
    # the small pipeline's stages: LayerNorm kernels + plain pooling give the same thing
    assert np.abs(fr.mean_pool(fr.layernorm(x, gp, bp, eps), lens, S) - want).max() <= 1e-9
    n = fr.mean_pool(fr.layernorm(x, gp, bp, eps), lens, S, normalize=True)
    assert np.abs(n - bo.forward(cfg, blob, ids, lens, normalize=True, out_dtype=np.float64)).max() <= 1e-9


def test_rope_reference_is_a_rotation_by_position():
    rng = np.random.default_rng(2)
    y = rng.standard_normal((64, 192))
    r = fr.rope_rotate(y, 32, 10000.0, 128)
    assert np.array_equal(r[:, 128:], y[:, 128:])                      # V columns untouched
    assert np.array_equal(r[0], y[0]) and np.array_equal(r[32], y[32])  # position 0 = row & 31 == 0
    for h0 in (0, 64):  # norms of the (j, j + 32) pairs are kept; pair 0 turns by exactly `position` radians
        n0 = y[:, h0:h0 + 32] ** 2 + y[:, h0 + 32:h0 + 64] ** 2
        n1 = r[:, h0:h0 + 32] ** 2 + r[:, h0 + 32:h0 + 64] ** 2
        assert np.abs(n0 - n1).max() <= 1e-12
        ang = np.arctan2(r[:, h0 + 32], r[:, h0]) - np.arctan2(y[:, h0 + 32], y[:, h0])
        assert np.abs(np.angle(np.exp(1j * (ang - (np.arange(64) & 31))))).max() <= 1e-9


def test_layout_helpers_round_trip():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((12, 192)).astype(np.float32)
    for mod in (fr, _native):
        b = mod.block64(a)
        assert b.shape == (3, 12, 64) and np.array_equal(b[2, 5], a[5, 128:192])  # block j, row m = columns 64 j .. 64 j + 63 of row m
        assert np.array_equal(mod.unblock64(b, 12, 192), a)
    x = rng.standard_normal((7, 768))
    st = fr.slot_stats(x)
    assert st.shape == (3, 7, 2)
    assert np.allclose(st[1, 4], [x[4, 256:512].sum(), (x[4, 256:512] ** 2).sum()], rtol=1e-13, atol=1e-13)
    assert np.allclose(st.sum(0), fr.embed_slot_stats(x, 3).sum(0), rtol=1e-12, atol=1e-12) and not fr.embed_slot_stats(x, 3)[1:].any()
    fin = fr.finalise(st, 768, 1e-12)
    mu, var = fr.row_moments(x)
    assert np.allclose(fin[:, 0], mu[:, 0], atol=1e-13) and np.allclose(fin[:, 1], 1 / np.sqrt(var[:, 0] + 1e-12), rtol=1e-12)


def test_row_populations_are_what_they_claim():
    A, kind = fr.make_rows(np.random.default_rng(4), 512, 1024)
    assert np.array_equal(fr.bf16_round(A), A)
    mu, var = fr.row_moments(A)
    r = np.abs(mu[:, 0]) / np.sqrt(np.maximum(var[:, 0], 1e-300))
    assert not A[kind == fr.ZERO].any() and (kind == fr.ZERO).sum() >= 37 + 20
    assert r[kind == fr.ORDINARY].max() < 0.2 and 0.9 < r[kind == fr.LARGE_MEAN].min() and r[kind == fr.LARGE_MEAN].max() < 9
    assert r[kind == fr.TINY_VAR].min() > 100 and var[kind == fr.TINY_VAR].max() < 1e-3
    e = (fr.slot_stats(A)[:, kind == fr.UNEVEN, 1])
    assert (e.max(0) / e.min(0)).min() > 1e3
