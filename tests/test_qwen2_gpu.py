"""GPU: the causal decoder family (Qwen2: sc_encoder_cfg.arch 2) through the C ABI -- the causal grouped-query attention kernels and the
RMSNorm kernel of encoder_causal.hip on their own, the whole forward against transformers, its properties and its refusals.

Bounds.
  Attention against float64 numpy over bf16-rounded q, k, v (q times 2: a sharp softmax): max <= 3e-2, median <= 3e-3, the project's
  bounds for P and O rounded to bf16 (tests/test_encoder_gpu.py::test_attention_kernel, the window test).  The same numpy without a
  mask, with the mask one key wider, or with interleaved K/V heads must exceed them on every sequence of at least 33 tokens.
  RMSNorm against float64: half a bf16 ulp of the reference plus twice the kernel's f32 term, the bound
  tests/test_fold_kernels_gpu.py::check_one_bf16_rounding puts on sc_diag_layernorm (the term restated for a norm without a mean).
  Whole path: T_last / T_mean of tests/golden/qwen2_golden.json -- twice what transformers' own bf16 forward of that model misses its
  fp32 forward by (scripts/gen_qwen2_fixtures.py) -- and the project's cos >= 0.999.  The generator has checked that eight mix-ups each
  miss the last-token vector of every text longer than 32 tokens by more than that (tests/test_qwen2.py repeats the check).
"""
import json

import numpy as np
import pytest

import fold_ref as fr
import qwen2_ref as qr
from semcode_amd import _native

pytestmark = pytest.mark.gpu

HEAD_FORMS = [(2, 1), (4, 2), (2, 2), (14, 2)]  # (heads, kv_heads)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def make_qkv(rows, heads, kvh, seed):
    rng = np.random.default_rng(seed)
    scale = np.r_[np.full(heads * 64, 2.0), np.ones(2 * kvh * 64)].astype(np.float32)
    return bf16_round(rng.standard_normal((rows, (heads + 2 * kvh) * 64)).astype(np.float32) * scale)


class SeqRef:
    """float64 attention of one sequence's real rows: out(mask_extra, no_mask, interleaved)."""

    def __init__(self, qkv_rows, n, heads, kvh):
        x = qkv_rows[:n].astype(np.float64)
        H, KV = heads * 64, kvh * 64
        self.n, self.heads, self.kvh = n, heads, kvh
        self.q = x[:, :H].reshape(n, heads, 64).transpose(1, 0, 2)
        self.k = x[:, H:H + KV].reshape(n, kvh, 64).transpose(1, 0, 2)
        self.v = x[:, H + KV:].reshape(n, kvh, 64).transpose(1, 0, 2)

    def out(self, extra=0, no_mask=False, interleaved=False):
        n, heads, kvh = self.n, self.heads, self.kvh
        of = [(h % kvh) if interleaved else h // (heads // kvh) for h in range(heads)]
        s = self.q @ self.k[of].transpose(0, 2, 1) / 8.0
        if not no_mask:
            s = np.where((np.arange(n)[None, :] <= np.arange(n)[:, None] + extra)[None], s, -np.inf)
        e = np.exp(s - s.max(-1, keepdims=True))
        return ((e / e.sum(-1, keepdims=True)) @ self.v[of]).transpose(1, 0, 2).reshape(n, heads * 64)


def check_causal(got, ref: SeqRef, what):
    """got: the kernel's rows of the sequence's real tokens"""
    err = np.abs(got - ref.out())
    print(f"{what} heads {ref.heads}/{ref.kvh} len {ref.n}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2, (what, ref.n, err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 3e-3, (what, ref.n)
    if ref.n >= 33:  # the inputs can tell: numpy with another mask or another head mapping must not pass
        wrong = [("no mask", ref.out(no_mask=True)), ("mask one key wider", ref.out(extra=1))]
        if ref.kvh not in (1, ref.heads):
            wrong.append(("interleaved K/V heads", ref.out(interleaved=True)))
        for name, w in wrong:
            e2 = np.abs(got - w)
            assert e2.max() > 3e-2, (what, name, ref.n, e2.max())


RECT_LENS = {32: [32, 1, 31], 64: [64, 33, 1], 256: [256, 129, 65, 33], 1024: [1024, 513, 257, 1], 2048: [2048, 1100, 513]}
RECT_FORMS = {32: [(2, 1), (2, 2)], 64: [(2, 1), (4, 2)], 256: [(2, 1), (4, 2), (14, 2)], 1024: [(2, 1), (4, 2)], 2048: [(2, 1)]}


# ------------------------------------------------------------------ 1. single-kernel parity
@pytest.mark.parametrize("S", sorted(RECT_LENS))
def test_attention_causal_kernel(rt, S):
    lens = np.array(RECT_LENS[S], np.int32)
    B = len(lens)
    for heads, kvh in RECT_FORMS[S]:
        H = heads * 64
        qkv = make_qkv(B * S, heads, kvh, 7400 + S + heads)
        row = _native.diag_attention_causal(rt, qkv, lens, heads, kvh, S=S)
        assert row.shape == (B * S, H) and np.isfinite(row).all()  # padding rows are queries too: they see key 0 at least
        if (heads, kvh) == RECT_FORMS[S][-1]:
            pad = np.zeros((B * S + 256, qkv.shape[1]), np.float32)
            pad[:B * S] = qkv
            blk = _native.diag_attention_causal(rt, pad, lens, heads, kvh, S=S, blocked_rows=B * S + 256)
            assert np.array_equal(bits(blk), bits(row)), int((bits(blk) != bits(row)).sum())  # the layouts hold the same numbers
        for b, n in enumerate(np.minimum(lens, S)):
            check_causal(row[b * S:b * S + n], SeqRef(qkv[b * S:(b + 1) * S], int(n), heads, kvh), f"rect S={S}")


PACKED_LENS = np.array([1, 31, 32, 33, 65, 129, 257, 513, 1100, 2048, 128, 256], np.int32)  # every launch class, both sides of each threshold


def packed_layout(lens):
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    end = int(span.sum())
    return span, starts, end, (end + 255) // 256 * 256


@pytest.mark.parametrize("heads,kvh", HEAD_FORMS)
def test_attention_causal_packed_kernel(rt, heads, kvh):
    lens = PACKED_LENS if heads <= 4 else PACKED_LENS[[0, 3, 5, 6, 7]]  # 14 heads: one text of every class
    span, starts, end, R = packed_layout(lens)
    assert R > end  # rows beyond the last sequence exist
    qkv = make_qkv(R, heads, kvh, 7500 + heads + kvh)
    row = _native.diag_attention_causal(rt, qkv, lens, heads, kvh, starts=starts)
    assert row.shape == (R, heads * 64)
    assert np.isnan(row[end:]).all()    # rows of no sequence: untouched
    assert np.isfinite(row[:end]).all()  # alignment rows included
    if (heads, kvh) == (4, 2):
        pad = np.zeros((R + 256, qkv.shape[1]), np.float32)
        pad[:R] = qkv
        blk = _native.diag_attention_causal(rt, pad, lens, heads, kvh, starts=starts, blocked_rows=R + 256)
        assert np.array_equal(bits(blk[:R]), bits(row)) and np.isnan(blk[end:]).all()
    for s, n in zip(starts, lens):
        check_causal(row[s:s + n], SeqRef(qkv[s:s + n], int(n), heads, kvh), "packed")


@pytest.mark.parametrize("heads,kvh", [(2, 1), (4, 2)])
def test_causal_kernel_packed_and_rectangle_agree_bit_for_bit(rt, heads, kvh):
    """Keys are folded in groups of four tiles from key 0 whatever the segment size, and a query block's tiles depend on its own position
    and the text's length only: a text's rows are the same bits in a rectangle of any S and in packed rows of any class."""
    lens = np.array([1100, 257, 129, 33, 1], np.int32)
    S = 2048
    qkv = make_qkv(len(lens) * S, heads, kvh, 7600 + heads)
    rect = _native.diag_attention_causal(rt, qkv, lens, heads, kvh, S=S)
    span, starts, end, R = packed_layout(lens)
    pk = np.zeros((R, qkv.shape[1]), np.float32)
    for b, (s, sp) in enumerate(zip(starts, span)):
        pk[s:s + sp] = qkv[b * S:b * S + sp]
    got = _native.diag_attention_causal(rt, pk, lens, heads, kvh, starts=starts)
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert np.array_equal(bits(got[s:s + n]), bits(rect[b * S:b * S + n])), b
    small = _native.diag_attention_causal(rt, qkv[2 * S:2 * S + 256], lens[2:3], heads, kvh, S=256)  # the 129-token text in a rectangle of its own class
    assert np.array_equal(bits(small[:129]), bits(rect[2 * S:2 * S + 129]))


def test_causal_kernel_refusals(rt):
    for heads, kvh in ((3, 2), (2, 3), (2, 0)):
        with pytest.raises(_native.ScError) as err:
            _native.diag_attention_causal(rt, np.zeros((32, (heads + 2 * kvh) * 64), np.float32), np.array([32], np.int32), heads, kvh, S=32)
        assert "kv_heads" in str(err.value)


# ------------------------------------------------------------------ 2. RMSNorm
U = 2.0 ** -24
EPS = 1e-6


@pytest.mark.parametrize("H,tokens", [(H, t) for H in (128, 896, 2048) for t in (1, 7, 9, 4095)] + [(896, 16385)])
def test_rmsnorm_kernel(rt, H, tokens):
    """rmsnorm_kernel<3> (H = 128 with the k0 < H guards), <4> (896: the last chunk guarded), <8> (2048); token counts around the 8 rows of
    a workgroup sweep, odd ones, and beyond one grid sweep (16385).  Rows of unit scale, rows 100 times larger, all-zero rows.  The sum of
    squares is a chain of at most 64 fused multiply-adds per lane and 5 shuffle levels (depth 69, all terms positive); rsqrt, the division
    and eps are 4 more roundings and enter by half; x * rs * gamma rounds twice."""
    rng = np.random.default_rng(H * 5 + tokens)
    x = rng.standard_normal((tokens, H))
    r = np.arange(tokens)
    x[r % 5 == 2] *= 100.0
    x[r % 11 == 3] = 0.0
    x = bf16_round(x.astype(np.float32))
    g = rng.standard_normal(H).astype(np.float32)
    got = _native.diag_rmsnorm(rt, x, g, EPS)
    x64 = x.astype(np.float64)
    rs = 1.0 / np.sqrt((x64 * x64).mean(-1, keepdims=True) + EPS)
    ref = x64 * rs * g.astype(np.float64)
    assert not got[~x.any(1)].any()  # zero rows stay zero
    f32term = ((69 + 4) * U / 2 + 2 * U) * np.abs(ref) + U * np.abs(ref)
    err = np.abs(got - ref)
    bar = 0.5 * fr.bf16_ulp(ref) + 2 * f32term
    print(f"rmsnorm H={H} tokens={tokens}: err/bar max {float((err / np.maximum(bar, 1e-300)).max()):.4f}")
    assert np.isfinite(got).all()
    assert np.all(err <= bar), (float((err / np.maximum(bar, 1e-300)).max()), np.unravel_index((err - bar).argmax(), err.shape))


# ------------------------------------------------------------------ 3. whole path against transformers
@pytest.fixture(scope="module")
def q2_golden(golden):
    return np.load(golden / "qwen2_golden.npz"), json.loads((golden / "qwen2_golden.json").read_text())


def weights_of(m):
    return qr.make_weights(m["cfg"], m["seed"], m["qk_scale"], m["bias_sigma"], m["vo_scale"], m["mlp_scale"], m["emb_scale"], m["norm_sigma"], m["bias_first"])


def packed_of(ids, lens):
    flat = np.concatenate([ids[i, :n] for i, n in enumerate(lens)]).astype(np.int32)
    return flat, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


CASES = ["g2_s64", "mha_s128", "g2_s256", "mqa_s128", "g2_s1024", "g2_s2048", "half_b"]


@pytest.mark.parametrize("name", CASES)
def test_embeddings_against_transformers(rt, q2_golden, name):
    data, meta = q2_golden
    m = meta[name]
    cfg = m["cfg"]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    flat, offsets = packed_of(ids, lens)
    enc = _native.Encoder(rt, cfg, weights=weights_of(m))
    try:
        assert enc.pooling == "mean"  # the default stays
        vec = {}
        for pooling, T, want in (("last", m["T_last"], data[f"{name}_last"]), ("mean", m["T_mean"], data[f"{name}_mean"])):
            enc.pooling = pooling
            for form, got in (("rectangle", enc.embed_ids(ids, lens)), ("packed", enc.embed_packed(flat, offsets))):
                d, cos = miss(got, want)
                print(f"{name} / {pooling} / {form}: max|d| {d.max():.4f} (T {T:.4f}), cos min {cos.min():.6f}")
                assert np.isfinite(got).all() and got.shape == want.shape
                assert d.max() <= T, (pooling, form, d)
                assert cos.min() >= 0.999, (pooling, form, cos)
                vec[pooling, form] = got
            d, _ = miss(vec[pooling, "packed"], vec[pooling, "rectangle"])  # packed and padded vectors agree within T
            assert d.max() <= T, (pooling, d)
    finally:
        enc.close()


# ------------------------------------------------------------------ 4. properties
def test_a_text_does_not_depend_on_its_batch_mates(rt, q2_golden):
    data, meta = q2_golden
    m = meta["g2_s256"]
    cfg = m["cfg"]
    ids, lens = data["g2_s256_ids"].astype(np.int32), data["g2_s256_lens"].astype(np.int32)
    enc = _native.Encoder(rt, cfg, weights=weights_of(m))
    try:
        for pooling in ("last", "mean"):
            enc.pooling = pooling
            both = enc.embed_ids(ids, lens)
            assert np.array_equal(bits(enc.embed_ids(ids, lens)), bits(both))  # run to run
            flat, offsets = packed_of(ids, lens)
            pboth = enc.embed_packed(flat, offsets)
            assert np.array_equal(bits(enc.embed_packed(flat, offsets)), bits(pboth))
            for i in (0, 2):  # 256 and 65 tokens: alone, and (packed) behind another text
                alone = enc.embed_ids(ids[i:i + 1], lens[i:i + 1])
                assert np.array_equal(bits(alone[0]), bits(both[i])), (pooling, i)
                f1, o1 = packed_of(ids[i:i + 1], lens[i:i + 1])
                assert np.array_equal(bits(enc.embed_packed(f1, o1)[0]), bits(pboth[i])), (pooling, i)
                j = (i + 1) % len(lens)
                f2, o2 = packed_of(ids[[j, i]], lens[[j, i]])
                assert np.array_equal(bits(enc.embed_packed(f2, o2)[1]), bits(pboth[i])), (pooling, i)
    finally:
        enc.close()


# ------------------------------------------------------------------ 5. refusals and the ABI's new fields
def test_create_rules_pooling_and_info(rt, q2_golden):
    _, meta = q2_golden
    base = dict(meta["g2_s256"]["cfg"], vocab=64, layers=2)
    for change, words in ((dict(rotary=False), ("arch 2", "pos_type")), (dict(swiglu=False), ("arch 2", "ffn_type")), (dict(swiglu=False, geglu=True), ("arch 2", "ffn_type")),
                          (dict(heads=8), ("head dimension",)), (dict(kv_heads=3), ("kv_heads", "3")), (dict(kv_heads=8), ("kv_heads",)),
                          (dict(local_window=32), ("local_window",)), (dict(global_every=3), ("global_every",))):
        with pytest.raises(_native.ScError) as err:
            _native.Encoder(rt, dict(base, **change), synth_seed=1)
        assert all(w in str(err.value) for w in words), (change, str(err.value))
    with pytest.raises(_native.ScError) as err:  # grouped-query heads without the causal pipeline
        _native.Encoder(rt, dict(_native.BERT_BASE, vocab=64, layers=1, kv_heads=4), synth_seed=1)
    assert "kv_heads" in str(err.value) and "arch 2" in str(err.value)
    enc = _native.Encoder(rt, dict(base, kv_heads=0), synth_seed=1)  # 0 means heads
    try:
        info = _native.EncoderCfg()
        assert _native.lib().sc_encoder_info(enc.handle, _native.C.byref(info)) == 0
        assert (info.arch, info.kv_heads, info.heads) == (2, 4, 4)
    finally:
        enc.close()
    enc = _native.Encoder(rt, base, synth_seed=1)
    bert = _native.Encoder(rt, dict(_native.BERT_BASE, vocab=64, layers=1, hidden=128, heads=2, ffn=256), synth_seed=1)
    try:
        info = _native.EncoderCfg()
        assert _native.lib().sc_encoder_info(enc.handle, _native.C.byref(info)) == 0
        assert (info.arch, info.kv_heads, info.rope_theta, info.pos_type, info.ffn_type) == (2, 2, 1000000.0, 2, 2)
        lib = _native.lib()
        assert lib.sc_encoder_set_pooling(enc.handle, 1) != 0 and enc.pooling == "mean"  # [CLS] is refused on arch 2 and changes nothing
        with pytest.raises(ValueError):
            enc.pooling = "cls"
        assert lib.sc_encoder_set_pooling(enc.handle, 2) == 0 and enc.pooling == "last"
        assert lib.sc_encoder_set_pooling(enc.handle, 3) != 0 and enc.pooling == "last"
        assert lib.sc_encoder_set_pooling(bert.handle, 2) != 0 and bert.pooling == "mean"  # still refused on a BERT encoder
        with pytest.raises(ValueError):
            bert.pooling = "last"
        ids = np.random.default_rng(0).integers(1, 64, size=(3, 64)).astype(np.int32)
        out = enc.embed_ids(ids, np.array([64, 9, 1], np.int32))
        assert out.shape == (3, 256) and np.isfinite(out).all() and np.abs(out).max() > 0
        with pytest.raises(_native.ScError) as err:
            enc.score_pairs(np.arange(1, 9, dtype=np.int32), np.array([0, 8], np.int64), np.array([4], np.int32))
        assert "arch 2" in str(err.value) and "pairs" in str(err.value)
    finally:
        enc.close()
        bert.close()


# ------------------------------------------------------------------ 6. a model directory through the provider
def test_model_directory_through_mi355x_embeddings(rt, q2_golden, tmp_path):
    """model.safetensors + config.json + tokenizer.json + 1_Pooling/config.json, nothing else configured: the provider reads all four.
    Bound: T_last of the golden case whose model this is (texts of the same length range), cos >= 0.999, against the numpy restatement on
    the provider's own ids."""
    tk = pytest.importorskip("tokenizers")
    from safetensors.numpy import save_file
    from tokenizers import models, pre_tokenizers, trainers

    from semcode_amd.embeddings.providers import MI355XEmbeddings

    _, meta = q2_golden
    m = meta["mqa_s128"]
    cfg = m["cfg"]
    blob = weights_of(m)
    save_file(qr.to_hf_state_dict(cfg, blob, "model."), str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(qr.hf_config(cfg)))
    (tmp_path / "1_Pooling").mkdir()
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({"word_embedding_dimension": cfg["hidden"], "pooling_mode_cls_token": False,
                                                                    "pooling_mode_mean_tokens": False, "pooling_mode_lasttoken": True}))
    tok = tk.Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    texts = ["def forward(self, hidden_states):\n    return self.norm(hidden_states)", "for i in range(len(xs)): total += xs[i] * ws[i]  # dot",
             "while queue:\n    node = queue.popleft()\n    for nxt in graph[node]:\n        if nxt not in seen:\n            seen.add(nxt); queue.append(nxt)", "class Causal:\n    def __init__(self, heads=14, kv_heads=2):\n        self.heads, self.kv_heads = heads, kv_heads\n" * 3]
    tok.train_from_iterator(texts * 3, trainers.BpeTrainer(vocab_size=cfg["vocab"], special_tokens=["<|endoftext|>"], initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    tok.save(str(tmp_path / "tokenizer.json"))  # (no post-processor: the family adds no special tokens)
    for packed in (False, True):
        emb = MI355XEmbeddings(weights=tmp_path / "model.safetensors", runtime=rt, max_tokens=128, packed=packed)
        try:
            assert emb._cfg["qwen2"] and emb._cfg["kv_heads"] == 1 and emb.pooling == "last" and emb._fast_tokenizer is None
            ids, lens = emb.tokenize(texts)
            assert ids.shape[1] == 128 and lens.max() > 64 and lens.min() >= 15 and ids.max() < cfg["vocab"]
            got = emb.embed_documents_array(texts)
            want = qr.forward(cfg, blob, ids, lens, "last")
            d, cos = miss(got, want)
            print(f"provider (packed={packed}): max|d| {d.max():.4f} (T {m['T_last']:.4f}), cos min {cos.min():.6f}")
            assert d.max() <= m["T_last"] and cos.min() >= 0.999, (d, cos)
        finally:
            emb.close()
