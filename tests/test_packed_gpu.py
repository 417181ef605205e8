"""GPU: packed variable-length batches (sc_encoder_embed_packed*, sc_diag_attention_run) through the C ABI.

References: oracle/bert_oracle.py (learned positions; ALiBi + GEGLU) and tests/nomic_ref.py (rotary + SwiGLU), each text given ALONE and
unpadded, so that nothing a neighbour or a padding row could leak is in them.  Bar: the project's whole-encoder bar of
tests/test_encoder_gpu.py / test_encoder_fuzz_gpu.py -- cosine >= 0.999, |err| <= 2e-2 (5e-2 for texts of fewer than 8 tokens), relative to
the element where it exceeds 1.  Attention alone: test_fold_kernels_gpu.py's check_attention bar (max 3e-2, median 3e-3) against
tests/fold_ref.py's float64 attention per sequence.  Model shape: hidden 256, 4 heads, ffn 512, 2 layers, vocab 400 -- the smallest the
LayerNorm-folded pipeline takes."""
import numpy as np
import pytest

import fold_ref as fr
import nomic_ref as nr
from oracle import bert_oracle as bo
from semcode_amd import _native

pytestmark = pytest.mark.gpu

LENS = [1, 31, 32, 33, 64, 65, 255, 256, 257, 511, 512]  # every side of the 32-row alignment and of the attention classes (128, 256)
LONG_LENS = [513, 40, 1024, 1500, 200]                   # cross the 512-key attention segments
SMALL = dict(vocab=400, hidden=256, heads=4, ffn=512, layers=2, type_vocab=2, ln_eps=1e-12)
KINDS = {
    "bert": dict(SMALL, max_pos=512),
    "alibi": dict(SMALL, max_pos=2048, alibi=True, geglu=True),
    "nomic": dict(SMALL, max_pos=2048, rotary=True, swiglu=True, rope_theta=1000.0),
}


def make_weights(kind):
    cfg = KINDS[kind]
    return nr.make_weights(cfg, 21) if kind == "nomic" else bo.make_blob(cfg, 21, "test")


def reference(kind, blob, texts):
    """Every text alone, unpadded, in float64."""
    cfg = KINDS[kind]
    out = []
    for t in texts:
        ids, lens = np.asarray(t)[None, :], np.array([len(t)])
        out.append(nr.forward(cfg, blob, ids, lens, cfg["rope_theta"])[0] if kind == "nomic" else bo.forward(cfg, blob, ids, lens)[0])
    return np.stack(out)


def make_texts(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, SMALL["vocab"], size=n).astype(np.int32) for n in lens]


def flat(texts):
    return np.concatenate(texts), np.concatenate(([0], np.cumsum([len(t) for t in texts]))).astype(np.int64)


_cache = {}


def case(kind, which):
    """(blob, texts, float64 reference) of one model kind and one set of lengths: computed once, shared by every test, never modified."""
    key = (kind, which)
    if key not in _cache:
        blob = _cache.setdefault(("blob", kind), make_weights(kind))
        texts = make_texts(LENS if which == "short" else LONG_LENS, 5 if which == "short" else 6)
        ref = reference(kind, blob, texts)
        ref.setflags(write=False)
        _cache[key] = (blob, texts, ref)
    return _cache[key]


def check_pooled(got, want, lens, tag):
    lens = np.asarray(lens)
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    err = np.abs(got - want)
    bound = np.where(lens[:, None] < 8, 5e-2, 2e-2) * np.maximum(1.0, np.abs(want))
    print(f"{tag}: cos min {cos.min():.6f}, max |err| {err.max():.5f}, max err / bound {(err / bound).max():.3f}")
    assert np.isfinite(got).all(), tag
    assert cos.min() >= 0.999, (tag, float(cos.min()), int(lens[cos.argmin()]))
    at = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), (tag, float(err[at]), float(want[at]), int(lens[at[0]]))


def l2(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)


def test_packed_rows(rt):
    enc = _native.Encoder(rt, KINDS["bert"], weights=None)
    try:
        assert enc.packed_rows(np.concatenate(([0], np.cumsum(LENS)))) == 2304  # ceil32 sums to 2144
        assert enc.packed_rows([0, 1]) == 256
    finally:
        enc.close()


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("path", ["batch", "small"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_packed_forward(rt, kind, path, normalize):
    blob, texts, ref = case(kind, "short")
    enc = _native.Encoder(rt, KINDS[kind], weights=blob, normalize=bool(normalize))
    try:
        enc.set_path(path)
        got = enc.embed_packed(*flat(texts))
        check_pooled(got, l2(ref) if normalize else ref, LENS, f"packed {kind} {path} normalize={normalize}")
    finally:
        enc.close()


@pytest.mark.parametrize("path", ["batch", "small"])
@pytest.mark.parametrize("kind", ["alibi", "nomic"])
def test_packed_forward_long(rt, kind, path):
    blob, texts, ref = case(kind, "long")
    enc = _native.Encoder(rt, KINDS[kind], weights=blob)
    try:
        enc.set_path(path)
        check_pooled(enc.embed_packed(*flat(texts)), ref, LONG_LENS, f"packed long {kind} {path}")
    finally:
        enc.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_cross_talk(rt, kind):
    """A text's vector does not depend on where it lies or on what lies next to it: bit-identical in the batch pipeline."""
    blob = case(kind, "short")[0]
    enc = _native.Encoder(rt, KINDS[kind], weights=blob)
    try:
        enc.set_path("batch")
        text = make_texts([100], 9)[0]
        a = enc.embed_packed(*flat(make_texts([257], 10) + [text]))[-1]
        b = enc.embed_packed(*flat(make_texts([5, 31, 33], 11) + [text]))[-1]
        c = enc.embed_packed(*flat([text] + make_texts([300], 12)))[0]
        assert np.isfinite(a).all()
        assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes()
    finally:
        enc.close()


def test_provider_order_and_batching(rt, tmp_path):
    from semcode_amd.embeddings.providers import MI355XEmbeddings

    words = [a + b for a in "abcdefghijklmnopqrst" for b in "abcdefghijklmnopqrst"][:396]
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + words) + "\n")
    rng = np.random.default_rng(3)
    counts = [1, 2, 29, 30, 31, 62, 63, 300, 254, 255] + list(rng.integers(1, 200, size=30))
    texts = [" ".join(words[i] for i in rng.integers(0, len(words), size=n)) for n in counts]
    assert len(texts) == 40
    kw = dict(cfg=KINDS["bert"], vocab=vocab, runtime=rt, allow_synthetic=True, synth_seed=4)
    packed = MI355XEmbeddings(packed=True, packed_rows_budget=1024, **kw)
    padded = MI355XEmbeddings(packed=False, **kw)
    try:
        # the batch pipeline computes every row independently of the others (the split-K factor of the small-batch one depends on the
        # row count), so under it "what each text alone returns" is a statement about bits
        packed._encoder.set_path("batch")
        ids, lens = packed.tokenize(texts)
        assert sorted(set(lens.tolist())) != [int(lens[0])] and int(lens.max()) > 256
        groups = packed._packed_groups(lens)
        assert len(groups) > 3 and groups[0][0] == 0 and groups[-1][1] == 40
        got = packed.embed_documents_array(texts)
        alone = np.stack([packed._encoder.embed_packed(ids[i, : lens[i]], [0, int(lens[i])])[0] for i in range(40)])
        assert got.tobytes() == alone.tobytes()
        assert np.array_equal(np.asarray(packed.embed_query(texts[7]), np.float32), alone[7])
        check_pooled(got, padded.embed_documents_array(texts), lens, "provider packed vs padded")
    finally:
        packed.close()
        padded.close()


def test_into_and_async(rt):
    blob, texts, _ = case("bert", "short")
    enc = _native.Encoder(rt, KINDS["bert"], weights=blob)
    try:
        for path in ("small", "batch"):
            enc.set_path(path)
            batches = [texts[:4], texts[4:8], texts[8:]]
            each = [enc.embed_packed(*flat(b)) for b in batches]
            B = 4
            rows = np.arange(B, dtype=np.int64)
            ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
            got = enc.embed_packed_into(*flat(batches[0]), ix, rows, want_host=True)
            assert got.tobytes() == each[0].tobytes(), path
            assert len(ix) == B and ix.get_rows(0, B).tobytes() == each[0].tobytes(), path
            ix.close()
            ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
            first = 0
            for b in batches:  # two in flight; the third waits for the first
                assert enc.embed_packed_into(*flat(b), ix, np.arange(first, first + len(b), dtype=np.int64), wait=False) is None
                first += len(b)
            enc.wait()
            assert len(ix) == len(texts) and ix.get_rows(0, len(texts)).tobytes() == np.concatenate(each).tobytes(), path
            ix.close()
            # a padded asynchronous batch and a packed one share the two slots and one wait()
            ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
            ids = np.zeros((2, 32), np.int32)
            ids[0, :31], ids[1] = texts[1], texts[2]
            want_padded = enc.embed_ids(ids, np.array([31, 32], np.int32))
            enc.embed_ids_into(ids, np.array([31, 32], np.int32), ix, np.arange(2, dtype=np.int64), wait=False)
            enc.embed_packed_into(*flat(batches[1]), ix, np.arange(2, 6, dtype=np.int64), wait=False)
            enc.wait()
            assert ix.get_rows(0, 6).tobytes() == np.concatenate([want_padded, each[1]]).tobytes(), path
            ix.close()
        other = _native.Index(rt, 128, metric="IP", kind="FLAT")
        for wait, name in ((True, "sc_encoder_embed_packed_into:"), (False, "sc_encoder_embed_packed_into_async:")):
            with pytest.raises(_native.ScError) as err:
                enc.embed_packed_into(*flat(texts[:2]), other, np.arange(2, dtype=np.int64), wait=wait)
            assert err.value.status == -1 and name in str(err.value), str(err.value)
        assert len(other) == 0
        other.close()
    finally:
        enc.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


ATT_LENS = [1, 32, 33, 255, 256, 257, 512, 513, 1500]


@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("heads", [2, 12])
def test_attention_packed_kernel(rt, heads, alibi):
    H = heads * 64
    lens = np.array(ATT_LENS, np.int32)
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    end = int(span.sum())
    R = (end + 255) // 256 * 256
    assert R > end  # rows beyond the last sequence exist
    rng = np.random.default_rng(heads + 100 * alibi)
    qkv = fr.bf16_round(rng.standard_normal((R, 3 * H)).astype(np.float32) * np.r_[np.full(H, 2.0), np.ones(2 * H)].astype(np.float32))
    slopes = bo.alibi_slopes(heads).astype(np.float32) if alibi else None
    row = _native.diag_attention_packed(rt, qkv, starts, lens, heads, slopes=slopes)
    Rb = R + 256
    pad = np.zeros((Rb, 3 * H), np.float32)
    pad[:R] = qkv
    blk = _native.diag_attention_packed(rt, pad, starts, lens, heads, blocked_rows=Rb, slopes=slopes)
    assert np.array_equal(bits(blk[:R]), bits(row)), int((bits(blk[:R]) != bits(row)).sum())
    assert np.isnan(row[end:]).all() and np.isnan(blk[end:]).all()  # rows of no sequence: untouched
    assert np.isfinite(row[:end]).all()                             # alignment rows included
    for s, n, sp in zip(starts, lens, span):
        ref = fr.attention(qkv[s:s + sp], [n], 1, int(sp), heads, slopes)
        err = np.abs(row[s:s + n] - ref[:n])
        print(f"packed attention heads={heads} alibi={alibi} len={n}: max err {err.max():.3e}, median {np.median(err):.3e}")
        assert err.max() <= 3e-2, (n, err.max(), np.unravel_index(err.argmax(), err.shape))
        assert np.median(err) <= 3e-3, n


def test_argument_errors_leave_the_encoder_alone(rt):
    blob, texts, _ = case("bert", "short")
    enc = _native.Encoder(rt, KINDS["bert"], weights=blob)
    ali = _native.Encoder(rt, KINDS["alibi"], weights=None)
    try:
        ids, offsets = flat(texts)
        want = enc.embed_packed(ids, offsets)
        lib = _native.lib()
        out = np.empty((len(texts), 256), np.float32)
        p = lambda a: a.ctypes.data_as(_native.C.c_void_p)

        def last_error():
            buf = _native.C.create_string_buffer(512)
            lib.sc_last_error(buf, 512)
            return buf.value
        bad = {
            "offsets[0] != 0": np.array([1, 5, 9], np.int64),
            "length 0": np.array([0, 4, 4], np.int64),
            "negative length": np.array([0, 6, 3], np.int64),
            "longer than max_pos": np.array([0, 513, 520], np.int64),
        }
        big = np.zeros(3000, np.int32)
        for tag, off in bad.items():
            assert lib.sc_encoder_embed_packed(enc.handle, p(big), p(off), 2, p(out)) == -1, tag
            assert b"sc_encoder_embed_packed" in last_error(), tag
            rows = _native.C.c_int64(-7)
            assert lib.sc_encoder_packed_rows(enc.handle, p(off), 2, _native.C.byref(rows)) == -1 and rows.value == -7, tag
        assert lib.sc_encoder_embed_packed(ali.handle, p(big), p(np.array([0, 2049], np.int64)), 1, p(out)) == -1  # no table: 2048 still bounds
        assert ali.packed_rows([0, 2048]) == 2048
        for B in (0, -1, 65537):
            assert lib.sc_encoder_embed_packed(enc.handle, p(big), p(bad["length 0"]), B, p(out)) == -1, B
        assert lib.sc_encoder_embed_packed(enc.handle, None, p(offsets), len(texts), p(out)) == -1
        assert lib.sc_encoder_embed_packed(enc.handle, p(ids), None, len(texts), p(out)) == -1
        assert lib.sc_encoder_embed_packed(enc.handle, p(ids), p(offsets), len(texts), None) == -1
        assert lib.sc_encoder_embed_packed(None, p(ids), p(offsets), len(texts), p(out)) == -1
        # more rows than SC_ENCODER_PACKED_MAX_ROWS = 524288: unsupported, by the planner alone
        with pytest.raises(_native.ScError) as err:
            ali.packed_rows(np.arange(258, dtype=np.int64) * 2048)
        assert err.value.status == -4, str(err.value)
        assert enc.embed_packed(ids, offsets).tobytes() == want.tobytes()
    finally:
        enc.close()
        ali.close()
