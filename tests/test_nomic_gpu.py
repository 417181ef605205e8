"""GPU: nomic-bert on the HIP encoder (rotary positions pos_type 2, SwiGLU ffn_type 2), through the C ABI.

Tolerances are the project's (tests/test_encoder_gpu.py header): single kernels vs float64 on the same bf16-rounded inputs
|err| <= 2^-8 of the output scale; whole encoder vs transformers' fp32 NomicBertModel golden vectors (tests/golden/nomic_golden.npz,
weights with Wq / Wk x 4 so that positions matter: scripts/gen_nomic_fixtures.py) cos >= 0.999 and max|d| <= 2e-2."""
import ctypes as C
import json

import numpy as np
import pytest

import nomic_ref as nr
from oracle import bert_oracle as bo
from semcode_amd import _native

pytestmark = pytest.mark.gpu

CASES = ["tiny", "mid", "long", "mid_theta10000", "base", "base_long"]


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def check_pooled(got, want):  # copied from tests/test_encoder_gpu.py
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    print(f"cos min {cos.min():.6f}  max|d| {np.abs(got - want).max():.5f}")
    assert cos.min() >= 0.999, cos
    assert np.abs(got - want).max() <= 2e-2, np.abs(got - want).max()


def ulps(err, ref):
    return err / 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)


@pytest.fixture(scope="module")
def nomic_golden(golden):
    return np.load(golden / "nomic_golden.npz"), json.loads((golden / "nomic_golden.json").read_text())


@pytest.fixture()
def rope_option():
    yield lambda v: _native.diag_set_option("rope_fused", v)
    _native.diag_set_option("rope_fused", -1)


def nomic_cfg(m):
    return dict(m["cfg"], rope_theta=m["theta"])


@pytest.mark.parametrize("theta", [1000.0, 10000.0])
@pytest.mark.parametrize("S", [32, 512, 2048])
def test_rope_kernel(rt, S, theta):
    heads, rows = 4, 2 * S + 5  # positions wrap (row % S); the row count is not a multiple of anything
    rng = np.random.default_rng(S + int(theta))
    x = bf16_round(rng.standard_normal((rows, heads * 64)).astype(np.float32))
    got = _native.diag_rope(rt, x, S, heads, theta).astype(np.float64)
    cos, sin = nr.rope_tables(S, theta)
    pos = np.arange(rows) % S
    ref = nr.rotate_half(x.astype(np.float64).reshape(rows, heads, 64), cos[pos][:, None, :], sin[pos][:, None, :]).reshape(rows, heads * 64)
    err = np.abs(got - ref)
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"rope S={S} theta={theta}: max err {err.max():.3e} (scale {scale:.2f}), worst {ulps(err, ref).max():.3f} bf16 ulp")
    assert np.isfinite(got).all()
    assert err.max() <= scale * 2.0 ** -8, (err.max(), scale, np.unravel_index(err.argmax(), err.shape))


def test_swiglu_kernel(rt):
    rows, F = 64, 512
    rng = np.random.default_rng(13)
    n = rows * F
    g = np.concatenate([np.linspace(-16.0, 16.0, n // 2), rng.standard_normal(n - n // 2) * 2.0]).astype(np.float32).reshape(rows, F)
    u = rng.standard_normal((rows, F)).astype(np.float32)
    h = bf16_round(np.concatenate([g, u], axis=1))
    got = _native.diag_swiglu(rt, h).astype(np.float64)
    gd, ud = h[:, :F].astype(np.float64), h[:, F:].astype(np.float64)
    ref = gd / (1.0 + np.exp(-gd)) * ud
    err = np.abs(got - ref)
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"swiglu: max err {err.max():.3e} (scale {scale:.2f}), worst {ulps(err, ref)[np.abs(ref) > 1e-3].max():.3f} bf16 ulp where |ref| > 1e-3")
    assert np.isfinite(got).all()
    assert err.max() <= scale * 2.0 ** -8, (err.max(), scale)
    # far tails: exp(-g) overflows f32 for g < -88.7 -> the output is a signed zero / tiny, never NaN; large g passes through
    gt = np.array([-3.0e38, -1.0e4, -200.0, -100.0, -89.0, -88.0, -30.0, 30.0, 100.0, 1.0e4, 3.0e38, 0.0] + [0.0] * 4, np.float32)
    ht = bf16_round(np.concatenate([np.tile(gt, (2, 1)), np.stack([np.full(16, 1.5, np.float32), np.full(16, -2.0, np.float32)])], axis=1))
    out = _native.diag_swiglu(rt, ht)
    assert not np.isnan(out).any(), out
    assert np.all(np.abs(out[:, :7]) < 1e-8), out[:, :7]
    assert np.isfinite(out[:, :10]).all() and np.allclose(out[:, 7:10], bf16_round(ht[:, 7:10] * ht[:, 16 + 7:16 + 10]), rtol=2.0 ** -7)


@pytest.mark.parametrize("mode", ["small", "batch-rope0", "batch-rope1"])
@pytest.mark.parametrize("case", CASES)
def test_nomic_encoder_matches_transformers_golden(rt, nomic_golden, rope_option, case, mode):
    """Every case x pipeline x rotation form, against NomicBertModel's fp32 vectors.  Observed on an MI355X with the fixtures'
    factor Wq / Wk x 4 (max|d|, bar 2e-2; cos >= 0.99999 everywhere): tiny 0.0128 in all three modes (128 hidden is not foldable: the
    stand-alone rotation kernel in every mode); mid 0.0124 / 0.0093 / 0.0092 (small / stand-alone / fused); long 0.0111; mid_theta10000 0.0091 / 0.0091 / 0.0090;
    base 0.0041 / 0.0052 / 0.0042; base_long 0.0034 / 0.0032 / 0.0033.  The factor did not have to be lowered.  check_pooled prints
    the figures (pytest -s)."""
    data, meta = nomic_golden
    m = meta[case]
    blob = nr.make_weights(m["cfg"], m["seed"], m["qk_scale"])
    enc = _native.Encoder(rt, nomic_cfg(m), weights=blob)
    try:
        if mode == "small":
            enc.set_path("small")
        else:
            enc.set_path("batch")
            rope_option(int(mode[-1]))
        got = enc.embed_ids(data[f"{case}_ids"].astype(np.int32), data[f"{case}_lens"])
        print(case, mode, end=": ")
        check_pooled(got, data[f"{case}_pooled"])
    finally:
        enc.close()


def test_fused_and_standalone_rope_agree_and_repeat(rt, rope_option):
    cfg = dict(vocab=400, hidden=768, layers=2, heads=12, ffn=3072, max_pos=2048, type_vocab=2, ln_eps=1e-12, rotary=True, swiglu=True, rope_theta=1000.0)
    blob = nr.make_weights(cfg, 21)
    rng = np.random.default_rng(8)
    ids = rng.integers(1, 400, size=(9, 128)).astype(np.int32)  # 1 152 token rows -> 1 280 padded
    lens = np.array([128, 3, 77, 128, 33, 100, 5, 128, 64], np.int32)
    want = nr.forward(cfg, blob, ids, lens, 1000.0)
    enc = _native.Encoder(rt, cfg, weights=blob)
    enc.set_path("batch")
    out = {}
    for form in (0, 1):
        rope_option(form)
        out[form] = enc.embed_ids(ids, lens)
        assert np.array_equal(out[form], enc.embed_ids(ids, lens)), form  # bit-reproducible run to run
        print("rope_fused", form, end=": ")
        check_pooled(out[form], want)
    print("fused vs standalone", end=": ")
    check_pooled(out[1], out[0])
    assert not np.array_equal(out[0], out[1])  # two roundings against one: the option really switches the code path
    enc.close()


@pytest.mark.parametrize("path", ["small", "batch"])
def test_rotary_batch_and_padding_invariance(rt, rope_option, path):
    """Positions come from row % S: a chunk's vector must not depend on its neighbours, its place in the batch or the bucket."""
    cfg = dict(vocab=400, hidden=256, layers=2, heads=4, ffn=512, max_pos=2048, type_vocab=2, ln_eps=1e-12, rotary=True, swiglu=True, rope_theta=1000.0)
    blob = nr.make_weights(cfg, 31)
    enc = _native.Encoder(rt, cfg, weights=blob)
    enc.set_path(path)
    rng = np.random.default_rng(2)
    B = 21
    ids = rng.integers(1, 400, size=(B, 64)).astype(np.int32)
    lens = rng.integers(3, 65, size=B).astype(np.int32)
    want = nr.forward(cfg, blob, ids, lens, 1000.0)
    for form in ((0, 1) if path == "batch" else (-1,)):
        rope_option(form)
        a = enc.embed_ids(ids, lens)
        check_pooled(a, want)
        alone = np.concatenate([enc.embed_ids(ids[i:i + 1], lens[i:i + 1]) for i in (0, 7, 20)])
        check_pooled(alone, want[[0, 7, 20]])
        assert np.abs(alone - a[[0, 7, 20]]).max() <= 1e-2
        perm = rng.permutation(B)
        check_pooled(enc.embed_ids(ids[perm], lens[perm]), want[perm])
        ids128 = np.zeros((B, 128), np.int32)
        ids128[:, :64] = ids
        c = enc.embed_ids(ids128, lens)  # the longer bucket
        check_pooled(c, want)
        assert np.abs(a - c).max() <= 1e-2
    enc.close()


def test_nomic_bad_arguments(rt):
    cfg = dict(vocab=50, hidden=128, layers=1, heads=2, ffn=256, max_pos=64, type_vocab=2, ln_eps=1e-12)
    with pytest.raises(ValueError):
        _native.Encoder(rt, dict(cfg, rotary=True, alibi=True))
    with pytest.raises(ValueError):
        _native.Encoder(rt, dict(cfg, swiglu=True, geglu=True))
    enc = _native.Encoder(rt, dict(cfg, rotary=True, swiglu=True))
    assert np.isfinite(enc.embed_ids(np.ones((1, 64), np.int32), np.array([64], np.int32))).all()
    with pytest.raises(_native.ScError):
        enc.embed_ids(np.zeros((1, 128), np.int32), np.ones(1, np.int32))  # S > max_pos: the rotary table has max_pos rows
    enc.close()
    for bad in (dict(pos_type=3), dict(ffn_type=3), dict(pos_type=2, rope_theta=-1.0)):
        c = _native.EncoderCfg(vocab=50, hidden=128, layers=1, heads=2, ffn=256, max_pos=64, type_vocab=2, ln_eps=1e-12, **bad)
        h = C.c_void_p()
        assert _native.lib().sc_encoder_create(rt.handle, C.byref(c), None, 0, C.byref(h)) != 0 and not h.value
    with pytest.raises(_native.ScError):
        _native.diag_rope(rt, np.zeros((4, 64), np.float32), 48, 1, 1000.0)  # S not a power of two


def test_rope_option_does_not_leak_into_other_families(rt, rope_option):
    rng = np.random.default_rng(5)
    for switches in (dict(), dict(alibi=True, geglu=True)):
        cfg = dict(bo.BERT_BASE, vocab=400, hidden=256, layers=2, heads=4, ffn=512, max_pos=64, **switches)
        blob = bo.make_blob(cfg, 11, "test")
        enc = _native.Encoder(rt, cfg, weights=blob)
        ids = rng.integers(1, 400, size=(40, 64)).astype(np.int32)  # 2 560 rows: the batch pipeline
        lens = rng.integers(1, 65, size=40).astype(np.int32)
        base = enc.embed_ids(ids, lens)
        for v in (1, 0, -1):
            rope_option(v)
            assert np.array_equal(enc.embed_ids(ids, lens).view(np.uint32), base.view(np.uint32)), (switches, v)
        check_pooled(base, bo.forward(cfg, blob, ids, lens))
        enc.close()


def test_nomic_gguf_through_the_provider_at_2048_tokens(tmp_path, rt):
    """A nomic-bert GGUF (as test_nomic_weights writes it) configures the provider by itself -- rotary, SwiGLU, theta, context
    length, vocabulary -- and embeds chunks of up to 2 048 tokens; same bits as the encoder built from the blob."""
    from semcode_amd.embeddings import gguf
    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from test_nomic_weights import TINY, nomic_gguf_meta, nomic_gguf_tensors

    cfg = dict(TINY)
    blob = nr.make_weights(cfg, 17)
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(200)] + [f"##s{i}" for i in range(95)]
    stored = [t if t.startswith("[") else (t[2:] if t.startswith("##") else "▁" + t) for t in words]
    path = tmp_path / "nomic.gguf"
    gguf.write_gguf(path, nomic_gguf_meta(cfg, freq_base=1000.0, tokens=stored), nomic_gguf_tensors(cfg, blob))
    emb = MI355XEmbeddings(weights=path, runtime=rt, max_tokens=2048)
    assert emb._cfg["rotary"] and emb._cfg["swiglu"] and emb._cfg["rope_theta"] == 1000.0 and emb._cfg["max_pos"] == 2048 and emb.max_tokens == 2048
    ref = _native.Encoder(rt, dict(cfg, rope_theta=1000.0), weights=blob)
    rng = np.random.default_rng(1)
    texts = [" ".join(f"w{i}" for i in rng.integers(0, 200, size=n)) for n in (1900, 700, 12)]
    ids, lens = emb.tokenize(texts)
    assert ids.shape == (3, 2048) and list(lens) == [1902, 702, 14] and emb.truncated_texts == 0
    got = emb.embed_documents_array(texts)
    assert np.array_equal(got.view(np.uint32), ref.embed_ids(ids, lens).view(np.uint32))
    check_pooled(got, nr.forward(cfg, blob, ids, lens, 1000.0))
    emb.close()
    ref.close()
