"""GPU: the pre-norm encoder family (ModernBERT: sc_encoder_cfg.arch 1) through the C ABI -- the windowed attention kernels of
encoder_window.hip on their own, the whole forward against transformers, its properties and its refusals.

Bounds.
  Single kernel against float64 numpy over bf16-rounded q, k, v (q times 2: a sharp softmax): max <= 3e-2, median <= 3e-3, the
  project's bounds for P and O rounded to bf16 (tests/test_encoder_gpu.py::test_attention_kernel).  The same numpy with the window one
  key wider or narrower on each side must exceed them: the inputs can tell.
  Whole path: T (mean) / T_cls ([CLS]) of tests/golden/modernbert_golden.json -- twice what transformers' own bf16 forward of that model
  misses its fp32 forward by (scripts/gen_modernbert_fixtures.py) -- and the project's cos >= 0.999.  The generator has checked that no
  window, a window off by one, either rotary base everywhere, post-norm, attn_norm in layer 0 and swapped gate halves each miss every
  text longer than the window by more than that (tests/test_modernbert.py repeats the check).
"""
import json

import numpy as np
import pytest

import modernbert_ref as mr
from semcode_amd import _native

pytestmark = pytest.mark.gpu

HEADS, H = 2, 128
WINDOWS = (2, 16, 32, 128)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def make_qkv(rows, seed):
    rng = np.random.default_rng(seed)
    return bf16_round(rng.standard_normal((rows, 3 * H)).astype(np.float32) * np.r_[np.full(H, 2.0), np.ones(2 * H)].astype(np.float32))


class SeqRef:
    """float64 scores of one sequence's real rows, computed once; out(half) = softmax over |i - j| <= half, times V."""

    def __init__(self, qkv_rows, n):
        x = qkv_rows[:n].astype(np.float64)
        sp = lambda t: t.reshape(n, HEADS, 64).transpose(1, 0, 2)
        self.n, self.v = n, sp(x[:, 2 * H:])
        self.s = sp(x[:, :H]) @ sp(x[:, H:2 * H]).transpose(0, 2, 1) / 8.0
        self.dist = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])

    def out(self, half):
        s = np.where(self.dist[None] <= half, self.s, -np.inf)
        e = np.exp(s - s.max(-1, keepdims=True))
        return ((e / e.sum(-1, keepdims=True)) @ self.v).transpose(1, 0, 2).reshape(self.n, H)


def check_window(got, ref: SeqRef, w, what):
    """got: the kernel's rows of the sequence's real tokens"""
    err = np.abs(got - ref.out(w // 2))
    print(f"{what} window {w} len {ref.n}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2, (what, w, ref.n, err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 3e-3, (what, w, ref.n)
    if ref.n >= 33 and ref.n > w // 2 + 1:  # keys exist on either side of the band's edge: numpy with the wrong window must not pass
        for wrong in (w // 2 - 1, w // 2 + 1):
            e2 = np.abs(got - ref.out(wrong))
            assert e2.max() > 3e-2, (what, w, wrong, ref.n, e2.max())


RECT_LENS = {32: [32, 1, 17], 64: [64, 33, 1], 256: [256, 129, 65, 33], 1024: [1024, 513, 129, 1], 2048: [2048, 1100, 513]}


# ------------------------------------------------------------------ 1. single-kernel parity
@pytest.mark.parametrize("S", sorted(RECT_LENS))
def test_attention_window_kernel(rt, S):
    lens = np.array(RECT_LENS[S], np.int32)
    B = len(lens)
    qkv = make_qkv(B * S, 6400 + S)
    refs = [SeqRef(qkv[b * S:(b + 1) * S], int(n)) for b, n in enumerate(lens)]
    for w in WINDOWS:
        row = _native.diag_attention_window(rt, qkv, lens, HEADS, w, S=S)
        assert row.shape == (B * S, H) and np.isfinite(row).all()  # padding rows are queries too: finite, zero where they see no key
        if w == 32:
            pad = np.zeros((B * S + 256, 3 * H), np.float32)
            pad[:B * S] = qkv
            blk = _native.diag_attention_window(rt, pad, lens, HEADS, w, S=S, blocked_rows=B * S + 256)
            assert np.array_equal(bits(blk), bits(row)), int((bits(blk) != bits(row)).sum())  # the layouts hold the same numbers
        for b, ref in enumerate(refs):
            check_window(row[b * S:b * S + ref.n], ref, w, f"rect S={S}")
            beyond = row[b * S + (ref.n + 31) // 32 * 32 + 32 * ((w // 2 + 31) // 32):(b + 1) * S]
            assert not beyond.any()  # query blocks wholly beyond len + w/2 see no key


def test_attention_window_packed_kernel(rt):
    lens = np.array([1, 33, 65, 129, 257, 513, 1100, 17], np.int32)  # every launch class, both sides of each threshold
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    end = int(span.sum())
    R = (end + 255) // 256 * 256
    assert R > end  # rows beyond the last sequence exist
    qkv = make_qkv(R, 6401)
    refs = [SeqRef(qkv[s:s + n], int(n)) for s, n in zip(starts, lens)]
    for w in WINDOWS:
        row = _native.diag_attention_window(rt, qkv, lens, HEADS, w, starts=starts)
        assert row.shape == (R, H)
        assert np.isnan(row[end:]).all()    # rows of no sequence: untouched
        assert np.isfinite(row[:end]).all()  # alignment rows included
        if w == 128:
            pad = np.zeros((R + 256, 3 * H), np.float32)
            pad[:R] = qkv
            blk = _native.diag_attention_window(rt, pad, lens, HEADS, w, starts=starts, blocked_rows=R + 256)
            assert np.array_equal(bits(blk[:R]), bits(row)) and np.isnan(blk[end:]).all()
        for s, ref in zip(starts, refs):
            check_window(row[s:s + ref.n], ref, w, "packed")


def test_window_kernel_packed_and_rectangle_agree_bit_for_bit(rt):
    """The two forms share the body and pick the instantiation by the text's own length: same bits."""
    lens = np.array([1100, 129, 33], np.int32)
    S = 2048
    qkv = make_qkv(3 * S, 6402)
    rect = _native.diag_attention_window(rt, qkv, lens, HEADS, 128, S=S)
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    R = (int(span.sum()) + 255) // 256 * 256
    pk = np.zeros((R, 3 * H), np.float32)
    for b, (s, sp) in enumerate(zip(starts, span)):
        pk[s:s + sp] = qkv[b * S:b * S + sp]
    got = _native.diag_attention_window(rt, pk, lens, HEADS, 128, starts=starts)
    # (the rectangle at S = 2048 runs the 12-tile instantiation for every text, the packed rows the one of the text's class: the
    # arithmetic per query block is the same single pass over the same tiles)
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert np.array_equal(bits(got[s:s + n]), bits(rect[b * S:b * S + n])), b


def test_window_kernel_refusals(rt):
    qkv = make_qkv(32, 1)
    for w in (0, 3, 130):
        with pytest.raises(_native.ScError) as err:
            _native.diag_attention_window(rt, qkv, np.array([32], np.int32), HEADS, w, S=32)
        assert "local_window" in str(err.value)


# ------------------------------------------------------------------ 2. whole path against transformers
@pytest.fixture(scope="module")
def mb_golden(golden):
    return np.load(golden / "modernbert_golden.npz"), json.loads((golden / "modernbert_golden.json").read_text())


def packed_of(ids, lens):
    flat = np.concatenate([ids[i, :n] for i, n in enumerate(lens)]).astype(np.int32)
    return flat, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


CASES = ["w128", "w128_short", "w32", "w32_s128", "w16_s64", "w32_l7", "w128_ge2", "base_w128", "w32_s32"]


@pytest.mark.parametrize("name", CASES)
def test_embeddings_against_transformers(rt, mb_golden, name):
    data, meta = mb_golden
    m = meta[name]
    cfg = m["cfg"]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    flat, offsets = packed_of(ids, lens)
    enc = _native.Encoder(rt, cfg, weights=mr.make_weights(cfg, m["seed"], m["qk_scale"], m["vo_scale"], m["mlp_scale"], m["global_qk"]))
    try:
        vec = {}
        for pooling, T, want in (("mean", m["T"], data[f"{name}_mean"]), ("cls", m["T_cls"], data[f"{name}_cls"])):
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


# ------------------------------------------------------------------ 3. properties
def test_a_text_does_not_depend_on_its_batch_mates(rt, mb_golden):
    data, meta = mb_golden
    m = meta["w32"]
    cfg = m["cfg"]
    ids, lens = data["w32_ids"].astype(np.int32), data["w32_lens"].astype(np.int32)
    enc = _native.Encoder(rt, cfg, weights=mr.make_weights(cfg, m["seed"], m["qk_scale"], m["vo_scale"], m["mlp_scale"], m["global_qk"]))
    try:
        for pooling in ("mean", "cls"):
            enc.pooling = pooling
            both = enc.embed_ids(ids, lens)
            assert np.array_equal(bits(enc.embed_ids(ids, lens)), bits(both))  # run to run
            flat, offsets = packed_of(ids, lens)
            pboth = enc.embed_packed(flat, offsets)
            assert np.array_equal(bits(enc.embed_packed(flat, offsets)), bits(pboth))
            for i in (0, 2):  # 600 and 300 tokens: alone, and (packed) behind another text
                alone = enc.embed_ids(ids[i:i + 1], lens[i:i + 1])
                assert np.array_equal(bits(alone[0]), bits(both[i])), (pooling, i)
                f1, o1 = packed_of(ids[i:i + 1], lens[i:i + 1])
                assert np.array_equal(bits(enc.embed_packed(f1, o1)[0]), bits(pboth[i])), (pooling, i)
                j = (i + 1) % len(lens)
                f2, o2 = packed_of(ids[[j, i]], lens[[j, i]])
                assert np.array_equal(bits(enc.embed_packed(f2, o2)[1]), bits(pboth[i])), (pooling, i)
    finally:
        enc.close()


def test_global_every_one_does_not_window(rt, mb_golden):
    data, meta = mb_golden
    m = meta["w32"]
    cfg = dict(m["cfg"], global_every=1)
    ids, lens = data["w32_ids"].astype(np.int32), data["w32_lens"].astype(np.int32)
    long_ = lens > cfg["local_window"]
    # the windowed model's weights (make_weights softens the layers that are global in ITS cfg), run with every layer global
    enc = _native.Encoder(rt, cfg, weights=mr.make_weights(m["cfg"], m["seed"], m["qk_scale"], m["vo_scale"], m["mlp_scale"], m["global_qk"]))
    try:
        flat, offsets = packed_of(ids, lens)
        for form, got in (("rectangle", enc.embed_ids(ids, lens)), ("packed", enc.embed_packed(flat, offsets))):
            d, cos = miss(got, data["w32_ge1_mean"])
            print(f"every layer global / {form}: max|d| {d.max():.4f} (T {m['T']:.4f})")
            assert d.max() <= m["T"] and cos.min() >= 0.999, (form, d)
            d, cos = miss(got, data["w32_mean"])  # ... and not the windowed model's vectors
            assert ((d > m["T"]) | (cos < 0.999))[long_].all(), (form, d)
    finally:
        enc.close()


# ------------------------------------------------------------------ 4. refusals and the ABI's new fields
def test_create_rules_and_info(rt, mb_golden):
    _, meta = mb_golden
    base = dict(meta["w32"]["cfg"], vocab=64, layers=3)
    for change, words in ((dict(rotary=False), ("arch 1", "pos_type")), (dict(rotary=False, alibi=True), ("arch 1", "pos_type")),
                          (dict(geglu=False), ("arch 1", "ffn_type")), (dict(geglu=False, swiglu=True), ("arch 1", "ffn_type")),
                          (dict(heads=4), ("head dimension",)), (dict(local_window=31), ("local_window", "31")),
                          (dict(local_window=130), ("local_window",)), (dict(local_window=0), ("local_window",)), (dict(global_every=0), ("global_every",))):
        with pytest.raises(_native.ScError) as err:
            _native.Encoder(rt, dict(base, **change), synth_seed=1)
        assert all(w in str(err.value) for w in words), (change, str(err.value))
    with pytest.raises(_native.ScError) as err:  # local attention without the pre-norm pipeline
        _native.Encoder(rt, dict(base, modernbert=False), synth_seed=1)
    assert "arch 1" in str(err.value)
    enc = _native.Encoder(rt, base, synth_seed=1)
    try:
        info = _native.EncoderCfg()
        assert _native.lib().sc_encoder_info(enc.handle, _native.C.byref(info)) == 0
        assert (info.arch, info.local_window, info.global_every, info.rope_theta, info.rope_theta_local) == (1, 32, 3, 160000.0, 10000.0)
        ids = np.random.default_rng(0).integers(1, 64, size=(3, 64)).astype(np.int32)
        out = enc.embed_ids(ids, np.array([64, 9, 1], np.int32))
        assert out.shape == (3, 128) and np.isfinite(out).all() and np.abs(out).max() > 0
        with pytest.raises(_native.ScError) as err:
            enc.score_pairs(np.arange(1, 9, dtype=np.int32), np.array([0, 8], np.int64), np.array([4], np.int32))
        assert "arch 1" in str(err.value) and "pair head" in str(err.value)
    finally:
        enc.close()


# ------------------------------------------------------------------ 5. a model directory through the provider
def test_model_directory_through_mi355x_embeddings(rt, mb_golden, tmp_path):
    """model.safetensors + config.json + tokenizer.json, nothing else configured: the provider reads all three.  Bound: T of the golden
    case whose model this is (texts of the same length range), cos >= 0.999, against the numpy restatement on the provider's own ids."""
    tk = pytest.importorskip("tokenizers")
    from safetensors.numpy import save_file
    from tokenizers import models, pre_tokenizers, processors, trainers

    from semcode_amd.embeddings.providers import MI355XEmbeddings

    _, meta = mb_golden
    m = meta["w32_s128"]
    cfg = m["cfg"]
    blob = mr.make_weights(cfg, m["seed"], m["qk_scale"], m["vo_scale"], m["mlp_scale"], m["global_qk"])
    save_file(mr.to_hf_state_dict(cfg, blob), str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(mr.hf_config(cfg)))
    tok = tk.Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    texts = ["def forward(self, hidden_states):\n    return self.final_norm(hidden_states)", "for i in range(len(xs)): total += xs[i] * ws[i]  # dot",
             "while queue:\n    node = queue.popleft()\n    for nxt in graph[node]:\n        if nxt not in seen:\n            seen.add(nxt); queue.append(nxt)", "class Window:\n    def __init__(self, size=128, every=3):\n        self.size, self.every = size, every\n" * 3]
    tok.train_from_iterator(texts * 3, trainers.BpeTrainer(vocab_size=cfg["vocab"], special_tokens=["[PAD]", "[CLS]", "[SEP]"],
                                                           initial_alphabet=pre_tokenizers.ByteLevel.alphabet()))
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    tok.save(str(tmp_path / "tokenizer.json"))
    for packed in (False, True):
        emb = MI355XEmbeddings(weights=tmp_path / "model.safetensors", runtime=rt, max_tokens=128, packed=packed)
        try:
            assert emb._cfg["modernbert"] and emb._cfg["local_window"] == 32 and emb.pooling == "mean" and emb._fast_tokenizer is None
            ids, lens = emb.tokenize(texts)
            assert ids.shape[1] == 128 and lens.max() > 64 and lens.min() >= 20 and ids.max() < cfg["vocab"]
            got = emb.embed_documents_array(texts)
            want = mr.forward(cfg, blob, ids, lens)
            d, cos = miss(got, want)
            print(f"provider (packed={packed}): max|d| {d.max():.4f} (T {m['T']:.4f}), cos min {cos.min():.6f}")
            assert d.max() <= m["T"] and cos.min() >= 0.999, (d, cos)
        finally:
            emb.close()
