"""GPU: parity of the HIP transformer-encoder forward (through the C ABI).

Floating point, bf16 matrix cores with f32 accumulation.  Tolerances (stated by BASELINE.json's
north_star as "within stated fp tolerance"):
  * single kernels vs a float64 reference on the same bf16-rounded inputs: |err| <= 2^-8 relative
    to the output scale (one bf16 output rounding + f32 accumulation noise);
  * whole encoder vs transformers' fp32 BertModel golden vectors: cosine >= 0.999 per chunk and
    max |err| <= 2e-2 on the (unit-scale, LayerNorm'd, mean-pooled) outputs.
"""
import json

import numpy as np
import pytest

from oracle import bert_oracle as bo
from semcode_amd import _native

pytestmark = pytest.mark.gpu


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def test_gelu_epilogue_accuracy(rt):
    """The 256-tile GEMM's GELU epilogue on its own: W = identity passes bf16 inputs through the accumulator unchanged, so
    out = bf16(gelu(x)) for x over [-16, 16] including both tails.  Bar: within one bf16 rounding of the erf definition
    (half an ulp) plus the approximation error of gemm_tile.h gelu_erf_fast2 -- 0.015 ulp wherever |gelu| > 1e-3, 0.14 ulp
    down to |gelu| > 1e-5 -- and 1e-6 absolute below that."""
    M = N = K = 256
    rng = np.random.default_rng(11)
    x = np.concatenate([np.linspace(-16.0, 16.0, M * K // 2), rng.standard_normal(M * K // 2) * 2.0]).astype(np.float32)
    A = bf16_round(x.reshape(M, K))
    W = np.eye(N, K, dtype=np.float32)
    got = _native.diag_gemm_bf16(rt, A, W, np.zeros(N, np.float32), None, epi=1).astype(np.float64)
    ref = gelu(A.astype(np.float64))
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 1e-300))) - 7)
    err = np.abs(got - ref)
    big, mid = np.abs(ref) > 1e-5, np.abs(ref) > 1e-3
    assert (err[mid] / ulp[mid]).max() <= 0.515, (err[mid] / ulp[mid]).max()
    assert (err[big] / ulp[big]).max() <= 0.64, (err[big] / ulp[big]).max()
    assert err[~big].max() <= 1e-6, err[~big].max()
    assert np.all(got[A > 12] == A[A > 12]) and np.all(np.abs(got[A < -12]) < 1e-30)  # saturated tails, no NaN


@pytest.mark.parametrize("splitk", [False, True])  # True: the tile x K-slice path small batches (a query) take
@pytest.mark.parametrize("epi", [0, 1, 2])
@pytest.mark.parametrize("shape", [(128, 128, 64), (256, 384, 768), (384, 768, 3072),  # 128x128 tiles
                                   (256, 256, 64), (256, 256, 128), (512, 768, 768), (256, 768, 3072), (1024, 2304, 192)])  # 256x256 tiles
def test_gemm_kernel(rt, epi, shape, splitk):
    M, N, K = shape
    rng = np.random.default_rng(M + N + K + epi)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = rng.standard_normal((M, N)).astype(np.float32)
    if splitk and shape not in ((512, 768, 768), (256, 768, 3072), (256, 256, 64)):
        pytest.skip("split-K only differs from the plain path on the shapes it applies to (+ one it must leave alone)")
    got = _native.diag_gemm_bf16(rt, A, W, bias, R if epi == 2 else None, epi=epi + (16 if splitk else 0))
    ref = bf16_round(A).astype(np.float64) @ bf16_round(W).astype(np.float64).T + bias
    if epi == 1:
        ref = gelu(ref)
    if epi == 2:
        ref = ref + bf16_round(R)
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(got - ref)
    # asymmetric operands: a transposed or permuted tile cannot pass this
    assert err.max() <= scale * 2.0 ** -8 + 1e-3, (err.max(), scale, np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("S", [32, 64, 128, 256, 512, 1024, 2048])  # 1024 / 2048: keys streamed through the LDS in segments of 512
def test_attention_kernel(rt, S):
    B, heads = 3 if S <= 512 else 4, 2
    H = heads * 64
    rng = np.random.default_rng(S)
    qkv = rng.standard_normal((B * S, 3 * H)).astype(np.float32)
    qkv[:, :H] *= 2.0  # sharper softmax
    lens = np.array([S, max(1, S // 2 + 3), 1] + ([S - 517] if S > 512 else []), np.int32)  # (S - 517: a ragged last segment)
    got = _native.diag_attention(rt, qkv, lens, B, S, heads)
    x = bf16_round(qkv).astype(np.float64).reshape(B, S, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) / 8.0
    s = np.where(np.arange(S)[None, None, None, :] < lens[:, None, None, None], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    ref = (p @ v).transpose(0, 2, 1, 3).reshape(B * S, H)
    err = np.abs(got - ref)
    assert err.max() <= 3e-2, (err.max(), np.unravel_index(err.argmax(), err.shape))  # P and O are rounded to bf16
    assert np.median(err) <= 3e-3


def test_long_attention_equals_the_resident_kernel_on_short_sequences(rt):
    """A sequence of <= 512 real tokens padded to 1 024 goes through the segmented kernel with ONE segment: same arithmetic per
    (query, key), so the real rows carry the bits the S = 512 kernel writes."""
    B, heads = 2, 2
    H = heads * 64
    rng = np.random.default_rng(5)
    qkv = rng.standard_normal((B * 512, 3 * H)).astype(np.float32)
    lens = np.array([512, 301], np.int32)
    short = _native.diag_attention(rt, qkv, lens, B, 512, heads).reshape(B, 512, H)
    pad = np.zeros((B, 1024, 3 * H), np.float32)
    pad[:, :512] = qkv.reshape(B, 512, 3 * H)
    long = _native.diag_attention(rt, pad.reshape(B * 1024, 3 * H), lens, B, 1024, heads).reshape(B, 1024, H)
    for b in range(B):
        assert np.array_equal(long[b, : lens[b]].view(np.uint32), short[b, : lens[b]].view(np.uint32))


@pytest.fixture(scope="module")
def enc_golden(golden):
    return np.load(golden / "encoder_golden.npz"), json.loads((golden / "encoder_golden.json").read_text())


def check_pooled(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    assert cos.min() >= 0.999, cos
    assert np.abs(got - want).max() <= 2e-2, np.abs(got - want).max()


@pytest.mark.parametrize("path", ["small", "batch"])  # split-K + LayerNorm kernels | 256-tile GEMMs with every LayerNorm folded in
@pytest.mark.parametrize("case", ["tiny", "base1", "base12"])
def test_encoder_matches_transformers_golden(rt, enc_golden, case, path):
    data, meta = enc_golden
    m = meta[case]
    blob = bo.make_blob(m["cfg"], m["seed"], m["style"])  # style "test": LayerNorm gamma / beta and all biases are non-trivial
    enc = _native.Encoder(rt, m["cfg"], weights=blob)
    enc.set_path(path)
    got = enc.embed_ids(data[f"{case}_ids"], data[f"{case}_lens"])
    check_pooled(got, data[f"{case}_pooled"])
    enc.close()


@pytest.mark.parametrize("path", ["small", "batch"])
def test_encoder_device_synthetic_weights_match_oracle_rule(rt, enc_golden, path):
    # no blob: the library builds the benchmark weights on device; the golden output was produced by
    # transformers with the same rule restated in oracle.bert_oracle.make_blob(style="bench")
    data, meta = enc_golden
    m = meta["base12_bench_weights"]
    enc = _native.Encoder(rt, m["cfg"], weights=None, synth_seed=m["seed"])
    enc.set_path(path)
    got = enc.embed_ids(data["base12_bench_weights_ids"], data["base12_bench_weights_lens"])
    check_pooled(got, data["base12_bench_weights_pooled"])
    enc.close()


def test_layernorm_folded_pipeline_equals_the_layernorm_kernels(rt):
    """The two pipelines on the same ragged batch, BERT-base shape with non-trivial LayerNorm parameters and biases (make_blob
    style "test"), 3 layers: the folded one (statistics from the producing epilogue, normalisation inside the consuming GEMM)
    must agree with the stand-alone LayerNorm kernels to bf16 noise, and with the float64 restatement to the usual bar; a
    normalised-output encoder takes the folded pipeline's other pooling branch."""
    cfg = dict(bo.BERT_BASE, layers=3, vocab=2000, max_pos=128)
    blob = bo.make_blob(cfg, 5, "test")
    rng = np.random.default_rng(6)
    ids = rng.integers(1, 2000, size=(9, 128)).astype(np.int32)  # 1 152 token rows -> 1 280 padded
    lens = np.array([128, 1, 77, 128, 33, 100, 2, 128, 64], np.int32)
    want = bo.forward(cfg, blob, ids, lens)
    for normalize in (False, True):
        enc = _native.Encoder(rt, cfg, weights=blob, normalize=normalize)
        ref = want / np.linalg.norm(want, axis=1, keepdims=True) if normalize else want
        out = {}
        for path in ("small", "batch"):
            enc.set_path(path)
            out[path] = enc.embed_ids(ids, lens)
            cos = (out[path] * ref).sum(1) / (np.linalg.norm(out[path], axis=1) * np.linalg.norm(ref, axis=1))
            assert cos.min() >= 0.999, (path, normalize, cos)
        scale = float(np.abs(ref).max())
        assert np.abs(out["small"] - out["batch"]).max() <= 3e-2 * scale, np.abs(out["small"] - out["batch"]).max()
        enc.set_path("batch")
        perm = rng.permutation(9)
        assert np.array_equal(enc.embed_ids(ids[perm], lens[perm]), out["batch"][perm])  # fixed reduction orders: bit-reproducible
        enc.close()


def test_encoder_batch_and_padding_invariance(rt):
    cfg = dict(bo.BERT_BASE, vocab=300, hidden=128, layers=2, heads=2, ffn=256, max_pos=128)
    blob = bo.make_blob(cfg, 7, "test")
    enc = _native.Encoder(rt, cfg, weights=blob)
    rng = np.random.default_rng(1)
    B = 37  # ragged: B*S not a multiple of the 128-row GEMM tile
    ids = rng.integers(1, 300, size=(B, 32)).astype(np.int32)
    lens = rng.integers(1, 33, size=B).astype(np.int32)
    a = enc.embed_ids(ids, lens)
    want = bo.forward(cfg, blob, ids, lens)
    check_pooled(a, want)
    # one chunk at a time gives the same vectors (rows are independent)
    b = np.concatenate([enc.embed_ids(ids[i:i + 1], lens[i:i + 1]) for i in range(0, B, 9)])
    assert np.array_equal(a[::9], b)
    # a longer padded bucket does not change the result beyond rounding noise
    ids64 = np.zeros((B, 64), np.int32)
    ids64[:, :32] = ids
    c = enc.embed_ids(ids64, lens)
    assert np.abs(a - c).max() <= 1e-2
    # normalised variant
    encn = _native.Encoder(rt, cfg, weights=blob, normalize=True)
    n = encn.embed_ids(ids, lens)
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-3)
    enc.close()
    encn.close()


def test_encoder_full_size_properties(rt):
    """BASELINE configs[1] at full size (256 chunks x 256 tokens, BERT-base shape, the benchmark's device-generated weights),
    checked through properties that do not need a full-size reference: chunks are independent, so permuting the batch permutes
    the output bit for bit (256x256-tile GEMMs, attention, LayerNorm, pooling all at their benchmark shapes); a sample of the
    rows matches the CPU restatement; and the small-batch path (split-K GEMMs) agrees with the large-batch path."""
    cfg = dict(bo.BERT_BASE)
    enc = _native.Encoder(rt, cfg, weights=None, synth_seed=0)
    rng = np.random.default_rng(3)
    ids = rng.integers(1000, 30000, size=(256, 256)).astype(np.int32)
    lens = np.full(256, 256, np.int32)
    lens[[5, 77, 200]] = [1, 100, 255]  # a few ragged chunks among the full ones
    a = enc.embed_ids(ids, lens)
    assert np.isfinite(a).all()
    perm = rng.permutation(256)
    assert np.array_equal(enc.embed_ids(ids[perm], lens[perm]), a[perm])
    sample = [0, 5, 77, 200]
    want = bo.forward(cfg, bo.make_blob(cfg, 0, "bench"), ids[sample], lens[sample])
    check_pooled(a[[0, 77, 200]], want[[0, 2, 3]])
    # the 1-token chunk is not averaged over tokens, so it carries the full per-token bf16 noise of 12 layers: looser absolute bar
    one, ref1 = a[5], want[1]
    assert one @ ref1 / (np.linalg.norm(one) * np.linalg.norm(ref1)) >= 0.999 and np.abs(one - ref1).max() <= 0.1
    # 768 tokens: split-K GEMMs and stand-alone LayerNorm kernels, against the batch pipeline's LayerNorm-folded GEMMs (the same
    # function, rounded to bf16 at different points); the 1-token chunk again gets the per-token bar
    small = enc.embed_ids(ids[sample[:3]], lens[sample[:3]])
    assert np.abs(small[[0, 2]] - a[[0, 77]]).max() <= 2e-2
    assert small[1] @ a[5] / (np.linalg.norm(small[1]) * np.linalg.norm(a[5])) >= 0.999 and np.abs(small[1] - a[5]).max() <= 0.1
    enc.close()


def test_batch_pipeline_is_reproducible_run_to_run(rt):
    """Six forwards of the same 256 x 256-token batch through the LayerNorm-folded pipeline, 2 layers of BERT-base shape with
    non-trivial biases and LayerNorm parameters: every buffer of the last layer (out-projection output, its row statistics, FFN
    output) and the pooled vectors repeat bit for bit.  This is the regression test of the packed-f32 op_sel hazard (DESIGN.md
    section 9): it showed as ~500 differing elements of the out-projection output per forward."""
    import ctypes as C

    cfg = dict(bo.BERT_BASE, layers=2, vocab=4000)
    enc = _native.Encoder(rt, cfg, weights=bo.make_blob(cfg, 11, "test"))
    enc.set_path("batch")
    rng = np.random.default_rng(4)
    ids = rng.integers(1, 4000, size=(256, 256)).astype(np.int32)
    lens = np.full(256, 256, np.int32)
    M = 256 * 256

    def snapshot():
        out = [enc.embed_ids(ids, lens).copy()]
        for which, nbytes in ((0, M * 768 * 2), (1, M * 768 * 2), (5, 3 * M * 8), (7, M * 8)):
            buf = np.empty(nbytes, np.uint8)
            _native._check(_native.lib().sc_diag_encoder_read(enc.handle, which, buf.ctypes.data_as(C.c_void_p), nbytes))
            out.append(buf)
        return out

    first = snapshot()
    for _ in range(5):
        again = snapshot()
        for k, (x, y) in enumerate(zip(first, again)):
            assert np.array_equal(x, y), (k, int((x != y).sum()))
    enc.close()


def test_encoder_bad_arguments(rt):
    with pytest.raises(_native.ScError):
        _native.Encoder(rt, dict(bo.BERT_BASE, hidden=96, heads=2))  # head dim != 64
    cfg = dict(bo.BERT_BASE, vocab=50, hidden=128, layers=1, heads=2, ffn=256, max_pos=64)
    with pytest.raises(_native.ScError):
        _native.Encoder(rt, cfg, weights=np.zeros(10, np.float32))  # wrong blob size
    enc = _native.Encoder(rt, cfg)
    with pytest.raises(_native.ScError):
        enc.embed_ids(np.zeros((1, 48), np.int32), np.ones(1, np.int32))  # S not a bucket
    with pytest.raises(_native.ScError):
        enc.embed_ids(np.zeros((1, 128), np.int32), np.ones(1, np.int32))  # S > max_pos
    enc.close()


@pytest.mark.parametrize("switches", [dict(alibi=True), dict(geglu=True), dict(alibi=True, geglu=True)])
def test_jina_v2_switches_match_restatement(rt, switches):
    """ALiBi attention bias and GEGLU feed-forward (jina-embeddings-v2 family).  No independent implementation exists
    offline for these switches: parity is against this repo's own numpy restatement only."""
    cfg = dict(bo.BERT_BASE, vocab=400, hidden=256, layers=2, heads=4, ffn=512, max_pos=64, **switches)
    blob = bo.make_blob(cfg, 11, "test")
    enc = _native.Encoder(rt, cfg, weights=blob)
    rng = np.random.default_rng(3)
    for S in (32, 256) if switches.get("alibi") else (32, 64):
        ids = rng.integers(1, 400, size=(5, S)).astype(np.int32)
        lens = np.array([S, S // 2 + 1, 3, S - 1, 17], np.int32)
        check_pooled(enc.embed_ids(ids, lens), bo.forward(cfg, blob, ids, lens))
    enc.close()


def test_long_chunks_alibi_encoder_matches_restatement(rt):
    """Chunks of 1 024 / 2 048 tokens (the reference's default chunker emits up to 200 lines / 6 000 characters,
    tree_sitter_chunker.py:64-65; jina-embeddings-v2 is an 8k-context ALiBi model): the whole forward at S = 1024 and 2048 --
    segmented attention with the ALiBi bias across segments -- against the numpy restatement (parity unpinned beyond it)."""
    cfg = dict(bo.BERT_BASE, vocab=400, hidden=128, layers=2, heads=2, ffn=256, max_pos=64, alibi=True, geglu=True)
    blob = bo.make_blob(cfg, 21, "test")
    enc = _native.Encoder(rt, cfg, weights=blob)
    rng = np.random.default_rng(9)
    for S, lens in ((1024, [1024, 700, 513, 40]), (2048, [2048, 1500, 3])):
        ids = rng.integers(1, 400, size=(len(lens), S)).astype(np.int32)
        check_pooled(enc.embed_ids(ids, np.array(lens, np.int32)), bo.forward(cfg, blob, ids, np.array(lens, np.int32)))
    enc.close()


def test_jina_v2_base_shape(rt):
    cfg = dict(bo.BERT_BASE, layers=2, alibi=True, geglu=True)  # 12 heads: non-power-of-two slope ladder
    blob = bo.make_blob(cfg, 12, "test")
    enc = _native.Encoder(rt, cfg, weights=blob)
    rng = np.random.default_rng(4)
    ids = rng.integers(1, 30000, size=(3, 128)).astype(np.int32)
    lens = np.array([128, 77, 40], np.int32)
    check_pooled(enc.embed_ids(ids, lens), bo.forward(cfg, blob, ids, lens))
    enc.close()


def test_embed_entry_points_agree(rt):
    """The four embed entry points side by side on one ragged batch, per pipeline: embed_ids, embed_ids_dev, embed_ids_into and its
    asynchronous form return / store the same bytes; three asynchronous batches before one wait() (the third re-uses the first pinned
    slot, so it has to wait for the first batch) store their own rows; an index of another dimension is refused by name."""
    import torch

    cfg = dict(bo.BERT_BASE, vocab=1000, hidden=256, heads=4, ffn=512, layers=2, max_pos=64)  # smallest shape the folded pipeline takes
    enc = _native.Encoder(rt, cfg, weights=None, synth_seed=3)
    rng = np.random.default_rng(8)
    B, S = 3, 32
    batches = [rng.integers(1, 1000, size=(B, S)).astype(np.int32) for _ in range(3)]
    ids, lens = batches[0], np.array([32, 7, 1], np.int32)
    rows = np.arange(B, dtype=np.int64)
    for path in ("small", "batch"):
        enc.set_path(path)
        want = enc.embed_ids(ids, lens)
        assert np.isfinite(want).all()
        ids_d, lens_d = torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(lens).to("cuda:0")
        out_d = torch.full((B, 256), float("nan"), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        enc.embed_ids_dev(ids_d.data_ptr(), lens_d.data_ptr(), B, S, out_d.data_ptr())
        rt.synchronize()
        assert out_d.cpu().numpy().tobytes() == want.tobytes(), path
        ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
        got = enc.embed_ids_into(ids, lens, ix, rows, want_host=True)
        assert got.tobytes() == want.tobytes(), path
        assert len(ix) == B and ix.get_rows(0, B).tobytes() == want.tobytes(), path
        ix.close()
        ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
        assert enc.embed_ids_into(ids, lens, ix, rows, wait=False) is None
        enc.wait()
        assert len(ix) == B and ix.get_rows(0, B).tobytes() == want.tobytes(), path
        ix.close()
        each = [enc.embed_ids(b, lens) for b in batches]
        assert not np.array_equal(each[0], each[2])
        ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
        for i, b in enumerate(batches):
            enc.embed_ids_into(b, lens, ix, rows + i * B, wait=False)
        enc.wait()
        assert len(ix) == 3 * B and ix.get_rows(0, 3 * B).tobytes() == np.concatenate(each).tobytes(), path
        ix.close()
    other = _native.Index(rt, 128, metric="IP", kind="FLAT")
    for wait, name in ((True, "sc_encoder_embed_ids_into:"), (False, "sc_encoder_embed_ids_into_async:")):
        with pytest.raises(_native.ScError) as err:
            enc.embed_ids_into(ids, lens, other, rows, wait=wait)
        assert err.value.status == -1 and name in str(err.value), str(err.value)  # SC_ERR_INVALID
    assert len(other) == 0
    other.close()
    enc.close()
