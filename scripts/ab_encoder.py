"""Same-box A/B of the encoder between two builds of the library (written for the split of sc_encoder.cpp:
profiles/encoder_split_ab.log; scripts/ab_encoder.sh drives it).  One process per build:

    python scripts/ab_encoder.py dump LIB.so OUT.txt        pooled vectors of synthetic-weight encoders and the diag_* results on
                                                            seeded inputs, one line per array: name, shape, sha256 of its bytes
    python scripts/ab_encoder.py compare A.txt B.txt        the two dumps line by line; VERDICT: pass only if every line is equal
    python scripts/ab_encoder.py bench LIB.so ARGS...       bench.py ARGS... on that build (the library path is set, nothing is copied)
    python scripts/ab_encoder.py speed DIR                  DIR/run_<i>_{new,base}.log + DIR/out_<i>_*/embed_pooled.npy of the bench runs:
                                                            outputs bit for bit, medians; the new build passes if its median is not
                                                            below the parent's by more than the parent's spread (max - min)
    python scripts/ab_encoder.py attn LIB.so OUT.json [ONLY]  time per launch of the attention kernels on the MiniLM, ModernBERT and causal
                                                            shapes (ONLY: the workloads whose name starts with it, e.g. causal)
    python scripts/ab_encoder.py attnspeed DIR              DIR/attn_<i>_{new,base}.json of such runs: the same rule per workload

Encoders: BERT, jina (ALiBi + GEGLU), nomic (rotary + SwiGLU, rope_fused 0 and 1) x {hidden 256 / ffn 512 (foldable), hidden 128 /
ffn 384 (128-tile path)} x normalize {0, 1} x (B, S) {(2, 32), (5, 256)} (256 and 1 280 token rows: either side of the 1 024-row
pipeline switch) x set_path {auto, batch, small}.  Then every instantiation of the attention kernels on its own (attention_section,
causal_section), and the three architectures through every kind of packed call with seeded heads (forward_section).
"""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def use_library(lib_path):
    """Points semcode_amd._native at that build.  A build of the parent commit does not export entry points added since: the binding
    drops those (named on stderr) instead of refusing the whole library; nothing this script calls may be among them."""
    import ctypes

    from semcode_amd import _native as nv

    try:
        import torch  # noqa: F401  (before the library, as _native.lib() loads it)
    except Exception:
        pass
    nv.LIB_PATH = Path(lib_path).resolve()
    handle = ctypes.CDLL(str(nv.LIB_PATH))
    missing = [name for name in nv.SIGNATURES if not hasattr(handle, name)]
    for name in missing:
        del nv.SIGNATURES[name]
    if missing:
        print(f"{nv.LIB_PATH.name} lacks {missing}: not bound", file=sys.stderr)
    return nv


def line(name, a):
    a = np.ascontiguousarray(a)
    return f"{name} {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}"


def attention_section(nv, rt, rng):
    """Every instantiation of the attention kernels on its own (written for the head width as a policy of the kernels:
    profiles/attention_shell_ab.log), hidden 128 = 2 heads of 64 or 4 heads of 32.  Rectangles: every S the launcher knows, lens
    {S, S - 23, 1} (full, masked tail, one key; 1 024 and 2 048: one, two, up to four segments of 512), plain / ALiBi / head_dim 32,
    row-major and blocked.  Packed: lens on both sides of the three launch classes, with live and dead waves.  Window: local_window
    128 and 6 on rectangles and on the packed lens."""
    out = []
    H = 128
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    forms = {"plain": dict(heads=2), "alibi": dict(heads=2, slopes=np.array([0.25, 0.0625], np.float32)), "hd32": dict(heads=4, head_dim=32)}
    ceil256 = lambda n: (n + 255) // 256 * 256
    rects = [(S, [S, S - 23, 1]) for S in (32, 64, 128, 256, 512)] + [(1024, [1024, 513, 40]), (2048, [2048, 1025])]
    for S, lens in rects:
        B = len(lens)
        qkv, lens = f(B * S, 3 * H), np.array(lens, np.int32)
        for blocked in (0, ceil256(B * S)):
            for form, kw in forms.items():
                out.append(line(f"attn rect S={S} {form} blocked={blocked}", nv.diag_attention_ex(rt, qkv, lens, B, S, blocked_rows=blocked, **kw)))
            if S in (128, 256, 1024):
                padded = np.concatenate([qkv, np.zeros((blocked - B * S, 3 * H), np.float32)]) if blocked else qkv  # diag_attention_ex pads by itself
                for lw in (128, 6):
                    out.append(line(f"attn window rect S={S} lw={lw} blocked={blocked}", nv.diag_attention_window(rt, padded, lens, 2, lw, S=S, blocked_rows=blocked)))
    lens = np.array([1, 32, 33, 255, 256, 257, 512, 513, 1500], np.int32)
    rows = (lens + 31) // 32 * 32
    starts = (np.cumsum(rows) - rows).astype(np.int32)
    R = ceil256(int(rows.sum()))
    qkv = f(R, 3 * H)
    for blocked in (0, R):
        for form, kw in forms.items():
            out.append(line(f"attn packed {form} blocked={blocked}", nv.diag_attention_packed(rt, qkv, starts, lens, blocked_rows=blocked, **kw)))
        for lw in (128, 6):
            out.append(line(f"attn window packed lw={lw} blocked={blocked}", nv.diag_attention_window(rt, qkv, lens, 2, lw, starts=starts, blocked_rows=blocked)))
    return out


def causal_section(nv, rt, rng):
    """Every instantiation of the causal attention kernels on its own (written for the head width as a template parameter of those
    kernels: profiles/causal_width_ab.log), head_dim 64 and 128, heads / kv_heads (2, 1) and (4, 2).  Rectangles: lens {S, S - 23, 1}
    (2 048: 1 100 and 33 tokens, segments carried along); packed: lens on both sides of the launch classes; row-major and blocked."""
    out = []
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    ceil256 = lambda n: (n + 255) // 256 * 256
    rects = [(S, [S, S - 23, 1]) for S in (32, 64, 128, 256, 512)] + [(2048, [1100, 33])]
    plens = np.array([1, 32, 33, 127, 128, 129, 255, 256, 257, 513, 1100], np.int32)
    prows = (plens + 31) // 32 * 32
    pstarts = (np.cumsum(prows) - prows).astype(np.int32)
    R = ceil256(int(prows.sum()))
    for hd in (64, 128):
        for heads, kvh in ((2, 1), (4, 2)):
            QN, tag = (heads + 2 * kvh) * hd, f"hd={hd} heads={heads}/{kvh}"
            for S, lens in rects:
                B, lens = len(lens), np.array(lens, np.int32)
                qkv = f(B * S, QN)
                for blocked in (0, ceil256(B * S)):
                    padded = np.concatenate([qkv, np.zeros((blocked - B * S, QN), np.float32)]) if blocked else qkv
                    out.append(line(f"causal rect S={S} {tag} blocked={blocked}", nv.diag_attention_causal(rt, padded, lens, heads, kvh, S=S, blocked_rows=blocked, head_dim=hd)))
            qkv = f(R, QN)
            for blocked in (0, R):
                out.append(line(f"causal packed {tag} blocked={blocked}", nv.diag_attention_causal(rt, qkv, plens, heads, kvh, starts=pstarts, blocked_rows=blocked, head_dim=hd)))
    return out


def forward_section(nv, rt, rng):
    """The host paths of the second split of the encoder host code (profiles/encoder_split2_ab.log) that the pooled lines above do not
    reach: 2-layer synthetic models of the three architectures through every kind of packed call, with seeded heads.  Packed lens
    [1, 33, 129, 257, 300] (1 024 token rows) and the same twice plus [512] (2 304): either side of the 1 024-row switch, each under
    set_path auto / batch / small.  arch 1: global_every 1 and 3, mean and [CLS]; arch 2: head_dim 64 with and without qk_norm and 128,
    kv_heads < heads, mean and last token; arch 0: [CLS] with cls_prune 0 and 1, rectangle and packed; score_pairs (arch 0, with and
    without pooler), score_seqs (arch 1 pooling 0 and 1, arch 2), embed_tokens (documents, expanded queries) and score_late (with and
    without d_keep) on arch 0 (foldable and not) and arch 1."""
    out = []
    f = lambda *s: (0.05 * rng.standard_normal(s)).astype(np.float32)
    small = [1, 33, 129, 257, 300]
    packs = {}
    for name, lens in (("1024", small), ("2304", small + small + [512])):
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        packs[name] = (rng.integers(1, 1000, size=int(offsets[-1])).astype(np.int32), offsets, np.array(lens))
    rect = (rng.integers(1, 1000, size=(5, 256)).astype(np.int32), np.array([256, 1, 33, 129, 200], np.int32))
    q_lens = [1, 33, 100, 128]
    q_off = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int64)
    q_ids = rng.integers(1, 1000, size=int(q_off[-1])).astype(np.int32)

    def each_path(enc, tag, call):
        for path in ("auto", "batch", "small"):
            enc.set_path(path)
            for name, a in call().items():
                out.append(line(f"{tag} path={path} {name}", a))
        enc.set_path("auto")

    def embeds(enc, tag):
        each_path(enc, f"{tag} rect", lambda: {"pooled": enc.embed_ids(*rect)})
        for pname, (ids, offsets, _) in packs.items():
            each_path(enc, f"{tag} packed {pname}", lambda: {"pooled": enc.embed_packed(ids, offsets)})

    def tokens(enc, tag):
        enc.set_token_head(f(64, enc.hidden))
        for pname, (ids, offsets, lens) in packs.items():
            keep = (rng.integers(0, 4, size=ids.size) > 0).astype(np.uint8)
            keep[offsets[:-1]] = 1  # every document keeps a token
            pq, pd = np.array([0, 1, 2, 3, 3], np.int32), np.array([0, len(lens) - 1, 2, 1, 4], np.int32)
            each_path(enc, f"{tag} tokens {pname}", lambda: {
                "docs": enc.embed_tokens(ids, offsets)[0], "queries": enc.embed_tokens(q_ids, q_off, expand_id=103)[0],
                "late": enc.score_late(q_ids, q_off, ids, offsets, pq, pd, expand_id=103),
                "late keep": enc.score_late(q_ids, q_off, ids, offsets, pq, pd, expand_id=103, d_keep=keep),
                "late plain": enc.score_late(q_ids, q_off, ids, offsets, pq, pd)})

    arch0 = {"h256": dict(hidden=256, heads=4, ffn=512), "h128": dict(hidden=128, heads=2, ffn=384)}
    for shape, dims in arch0.items():
        cfg = dict(nv.BERT_BASE, vocab=1000, layers=2, max_pos=512, **dims)
        for normalize in (0, 1):
            enc = nv.Encoder(rt, cfg, weights=None, normalize=bool(normalize), synth_seed=5)
            embeds(enc, f"fwd arch0 {shape} norm={normalize} mean")
            enc.pooling = "cls"
            for prune in (0, 1):
                nv.diag_set_option("cls_prune", prune)
                embeds(enc, f"fwd arch0 {shape} norm={normalize} cls prune={prune}")
            nv.diag_set_option("cls_prune", -1)
            enc.pooling = "mean"
            if normalize:
                H = enc.hidden
                for pooler in (False, True):
                    enc.set_pair_head(f(2, H), f(2), *((f(H, H), f(H)) if pooler else ()))
                    for pname, (ids, offsets, lens) in packs.items():
                        first = np.maximum(1, lens // 3).astype(np.int32)
                        pairs = lens >= 2  # (a pair has at least two tokens: the text of one token is left out)
                        p_off = np.concatenate([[0], np.cumsum(lens[pairs])]).astype(np.int64)
                        p_ids = np.concatenate([ids[a:b] for a, b, k in zip(offsets[:-1], offsets[1:], pairs) if k])
                        each_path(enc, f"fwd arch0 {shape} pairs pooler={pooler} {pname}",
                                  lambda: dict(zip(("logits", "cls"), enc.score_pairs(p_ids, p_off, first[pairs], want_cls=True))))
                tokens(enc, f"fwd arch0 {shape}")
            enc.close()

    modern = dict(vocab=1000, hidden=256, layers=2, heads=4, ffn=512, max_pos=512, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True,
                  local_window=128, rope_theta=160000.0, rope_theta_local=10000.0)
    for ge in (1, 3):
        enc = nv.Encoder(rt, dict(modern, global_every=ge), weights=None, normalize=True, synth_seed=6)
        H = enc.hidden
        for pooling in ("mean", "cls"):
            enc.pooling = pooling
            embeds(enc, f"fwd arch1 ge={ge} {pooling}")
            enc.set_score_head(dict(kind=1, pooling=pooling, dense_w=f(H, H), dense_b=f(H), norm_g=1 + f(H), norm_b=f(H), norm_eps=1e-5, cls_w=f(1, H), cls_b=f(1)))
            for pname, (ids, offsets, _) in packs.items():
                each_path(enc, f"fwd arch1 ge={ge} seqs head={pooling} {pname}", lambda: dict(zip(("logits", "rows"), enc.score_seqs(ids, offsets, want_rows=True))))
        enc.pooling = "mean"
        tokens(enc, f"fwd arch1 ge={ge}")
        enc.close()

    causal = dict(vocab=1000, hidden=256, layers=2, ffn=512, max_pos=512, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0)
    widths = {"hd64": dict(heads=4, kv_heads=2), "hd64 qk_norm": dict(heads=4, kv_heads=2, qk_norm=True), "hd128": dict(heads=4, kv_heads=2, head_dim=128, qk_norm=True)}
    for wname, dims in widths.items():
        enc = nv.Encoder(rt, dict(causal, **dims), weights=None, normalize=True, synth_seed=7)
        for pooling in ("mean", "last"):
            enc.pooling = pooling
            embeds(enc, f"fwd arch2 {wname} {pooling}")
        enc.set_score_head(dict(kind=2, cls_w=f(2, enc.hidden), cls_b=f(2)))
        for pname, (ids, offsets, _) in packs.items():
            each_path(enc, f"fwd arch2 {wname} seqs {pname}", lambda: dict(zip(("logits", "rows"), enc.score_seqs(ids, offsets, want_rows=True))))
        enc.close()
    return out


def dump(lib_path, out_path):
    nv = use_library(lib_path)
    rt = nv.Runtime()
    out = []
    rng = np.random.default_rng(2024)
    families = {"bert": {}, "jina": dict(alibi=True, geglu=True), "nomic": dict(rotary=True, swiglu=True)}
    shapes = {"h256": dict(hidden=256, heads=4, ffn=512), "h128": dict(hidden=128, heads=2, ffn=384)}
    batches = {}
    for B, S in ((2, 32), (5, 256)):
        batches[(B, S)] = (rng.integers(1, 1000, size=(B, S)).astype(np.int32), rng.integers(1, S + 1, size=B).astype(np.int32))
    for fam, switches in families.items():
        for shape, dims in shapes.items():
            for normalize in (0, 1):
                cfg = dict(nv.BERT_BASE, vocab=1000, layers=2, max_pos=256, **dims, **switches)
                enc = nv.Encoder(rt, cfg, weights=None, normalize=bool(normalize), synth_seed=5)
                for fused in ((0, 1) if fam == "nomic" else (-1,)):
                    nv.diag_set_option("rope_fused", fused)
                    for (B, S), (ids, lens) in batches.items():
                        for path in ("auto", "batch", "small"):
                            enc.set_path(path)
                            out.append(line(f"pooled {fam} {shape} norm={normalize} rope_fused={fused} B={B} S={S} path={path}", enc.embed_ids(ids, lens)))
                nv.diag_set_option("rope_fused", -1)
                enc.close()

    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    M, N, K = 256, 256, 256
    A, W, bias, R = f(M, K), 0.05 * f(N, K), f(N), f(M, N)
    for epi in (0, 1, 2):
        for sk in (0, 16):
            out.append(line(f"gemm_bf16 epi={epi} splitk={sk}", nv.diag_gemm_bf16(rt, A, W, bias, R if epi == 2 else None, epi=epi | sk)))
    out.append(line("gemm_bf16 128-tile", nv.diag_gemm_bf16(rt, f(128, 64), f(384, 64), f(384))))
    out.append(line("gemm_i8", nv.diag_gemm_i8(rt, rng.integers(-127, 128, (256, 128)), rng.integers(-127, 128, (256, 128)))))
    B, S, heads = 3, 64, 2
    H = heads * 64
    qkv, lens = f(B * S, 3 * H), np.array([64, 9, 1], np.int32)
    out.append(line("attention", nv.diag_attention(rt, qkv, lens, B, S, heads)))
    out.append(line("attention_ex blocked", nv.diag_attention_ex(rt, qkv, lens, B, S, heads, blocked_rows=256)))
    out.append(line("attention_ex slopes", nv.diag_attention_ex(rt, qkv, lens, B, S, heads, slopes=np.array([0.25, 0.0625], np.float32))))
    out.append(line("rope", nv.diag_rope(rt, f(200, 3 * 64), 64, 3, 10000.0)))
    out.append(line("rope theta=1000", nv.diag_rope(rt, f(128, 64), 32, 1, 1000.0)))
    h = f(70, 2 * 136)
    out.append(line("swiglu", nv.diag_swiglu(rt, h)))
    out.append(line("geglu", nv.diag_geglu(rt, h)))
    gamma, beta = 1 + 0.1 * f(K), 0.1 * f(K)
    Wf, c1, c2 = nv.diag_fold_ln(rt, W, gamma, beta, bias)
    for name, a in (("Wf", Wf), ("c1", c1), ("c2", c2)):
        out.append(line(f"fold_ln {name}", a))
    stats = np.stack([A.sum(1), (A * A).sum(1)], axis=1).reshape(1, M, 2).astype(np.float32)
    for epi, kw in ((3, {}), (4, dict(blocked=True)), (6, dict(blocked=True, rope_S=64, rope_theta=0.0, rope_ncols=128))):
        Cc, fin = nv.diag_gemm_lna(rt, epi, A, Wf, c1, c2, stats, 1e-12, **kw)
        out.append(line(f"gemm_lna epi={epi} C", Cc))
        out.append(line(f"gemm_lna epi={epi} fin", fin))
    for blocked in (False, True):
        Cc, st = nv.diag_gemm_resln(rt, A, W, bias, gamma, R, fin, 1e-12, a_blocked=blocked)
        out.append(line(f"gemm_resln blocked={blocked} C", Cc))
        out.append(line(f"gemm_resln blocked={blocked} stats", st))
    x = f(B * S, 256)
    out.append(line("layernorm", nv.diag_layernorm(rt, x, gamma, beta, 1e-12)))
    for normalize in (False, True):
        out.append(line(f"mean_pool normalize={normalize}", nv.diag_mean_pool(rt, x, lens, S, normalize)))
    y = f(256, 256)
    ystats = np.stack([y.sum(1), (y * y).sum(1)], axis=1).reshape(1, 256, 2).astype(np.float32)
    out.append(line("mean_pool_ln", nv.diag_mean_pool_ln(rt, y, ystats, gamma, beta, 1e-12, lens, S)))
    ids = rng.integers(0, 50, size=(B, S)).astype(np.int32)
    wemb, pemb, temb = f(50, 256), f(64, 256), f(2, 256)
    rows, st = nv.diag_embed(rt, ids, wemb, pemb, temb, 64, tokens_pad=256, slots=1)
    out.append(line("embed raw rows", rows))
    out.append(line("embed raw stats", st))
    out.append(line("embed ln", nv.diag_embed(rt, ids, wemb, None, temb, 64, ln=(gamma, beta, 1e-12))))
    out += attention_section(nv, rt, np.random.default_rng(7))
    out += causal_section(nv, rt, np.random.default_rng(8))
    out += forward_section(nv, rt, np.random.default_rng(9))
    rt.close()
    Path(out_path).write_text("\n".join(out) + "\n")
    print(f"{len(out)} arrays -> {out_path}")


def compare(a_path, b_path):
    a, b = Path(a_path).read_text().splitlines(), Path(b_path).read_text().splitlines()
    ok = len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        same = x == y
        ok &= same
        print(f"{x.rsplit(' ', 1)[0]}: {'equal' if same else 'DIFFERENT'}")
    print(f"{len(a)} / {len(b)} arrays")
    print("VERDICT:", "pass" if ok else "FAIL")
    return 0 if ok else 1


def bench(lib_path, argv):
    import runpy

    use_library(lib_path)
    root = Path(__file__).resolve().parent.parent
    sys.argv = [str(root / "bench.py"), *argv]
    runpy.run_path(sys.argv[0], run_name="__main__")


def speed(dirname):
    import json

    d = Path(dirname)
    val, pooled = {"new": [], "base": []}, []
    for log in sorted(d.glob("run_*.log")):
        i, which = log.stem.split("_")[1:]
        res = [json.loads(l) for l in log.read_text().splitlines() if l.startswith("{")][-1]
        val[which].append(res["value"])
        pooled.append(np.load(d / f"out_{i}_{which}" / "embed_pooled.npy"))
        print(f"run {i} {which:4s} {res['value']:10.1f} chunks/s  {res['ms_per_step']:.3f} ms/step")
    same = all(p.tobytes() == pooled[0].tobytes() for p in pooled)
    print(f"embed_pooled.npy of the {len(pooled)} runs: {'byte-identical' if same else 'DIFFERENT'}")
    nm, bm = float(np.median(val["new"])), float(np.median(val["base"]))
    spread = max(val["base"]) - min(val["base"])
    ok = same and len(val["new"]) == len(val["base"]) == 3 and nm >= bm - spread
    print(f"median new {nm:.1f}  parent {bm:.1f}  new/parent {nm / bm:.4f}  parent spread {spread:.1f} ({100 * spread / bm:.2f} %)")
    print("VERDICT:", "pass" if ok else "FAIL")
    return 0 if ok else 1


def attn(lib_path, out_path, only=""):
    """Time per launch of the attention profiling class (3), as scripts/bench_modernbert.py brackets it, on the shapes of
    scripts/bench_minilm.py (384 hidden, 256 texts of 256 tokens, heads of 32 and of 64) and of scripts/bench_modernbert.py (32k tokens
    as texts of 256 / 1 024 / 2 048, the windowed and the all-global model), padded and packed, on rectangles of every other
    length with heads of 32 (64k tokens), and on the causal shapes of scripts/bench_qwen3.py (W64: 32 / 16 heads of 64, W128: 16 / 8
    heads of 128; 2 layers, only the attention class is timed; 32k tokens as texts of 128 / 256 / 1 024 / 2 048 -- every causal
    instantiation of both widths): one JSON line per workload.  only: the workloads whose model name starts with it."""
    import json

    nv = use_library(lib_path)
    rt = nv.Runtime()
    rng = np.random.default_rng(11)
    mini = dict(nv.BERT_BASE, hidden=384, layers=6, ffn=1536, max_pos=512)
    modern = dict(vocab=50368, hidden=768, layers=22, heads=12, ffn=1152, max_pos=8192, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True,
                  local_window=128, global_every=3, rope_theta=160000.0, rope_theta_local=10000.0)
    models = {"minilm d32": (dict(mini, heads=12), (256,)), "minilm d64": (dict(mini, heads=6), (256,)),
              "modernbert windowed": (modern, (256, 1024, 2048)), "modernbert global": (dict(modern, global_every=1), (256, 1024, 2048)),
              # the other rectangle kernels of the 32-wide heads (S = 256 is above): 64 rows of tokens per text length
              "minilm d32 rect": (dict(mini, heads=12, max_pos=2048), (32, 64, 128, 512, 1024, 2048))}
    causal = dict(vocab=1024, layers=2, ffn=3072, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0)
    models["causal d64"] = (dict(causal, hidden=2048, heads=32, kv_heads=16), (128, 256, 1024, 2048))
    models["causal d128"] = (dict(causal, hidden=1024, heads=16, kv_heads=8, head_dim=128, qk_norm=True), (128, 256, 1024, 2048))
    out = []
    for name, (cfg, lengths) in models.items():
        if not name.startswith(only):
            continue
        enc = nv.Encoder(rt, cfg, weights=None, synth_seed=1, **(dict(pooling="last") if name.startswith("causal") else {}))
        for S in lengths:
            B = 65536 // S if name.endswith("rect") else (256 if name.startswith("minilm") else 32768 // S)
            ids, lens = rng.integers(1, min(30000, cfg["vocab"]), size=(B, S)).astype(np.int32), np.full(B, S, np.int32)
            flat, offsets = ids.reshape(-1), (np.arange(B + 1) * S).astype(np.int64)
            for form, call in (("padded", lambda: enc.embed_ids(ids, lens)), ("packed", lambda: enc.embed_packed(flat, offsets)))[: 1 if name.endswith("rect") else 2]:
                call()  # warm-up: workspace, first touch
                rt.set_profiling(1)
                rt.profile_reset()
                call()
                call()
                ms, n = rt.profile_read(3)
                rt.set_profiling(0)
                out.append(json.dumps({"name": f"{name} S={S} {form}", "us_per_launch": 1e3 * ms / max(n, 1), "launches": n}))
        enc.close()
    rt.close()
    Path(out_path).write_text("\n".join(out) + "\n")
    print(f"{len(out)} workloads -> {out_path}")


def attnspeed(dirname):
    """DIR/attn_<i>_{new,base}.json of the alternating `attn` runs: per workload the medians; the new build passes a workload if its
    median time per launch is not above the parent's by more than the parent's spread (max - min)."""
    import json

    t = {"new": {}, "base": {}}
    for f in sorted(Path(dirname).glob("attn_*.json")):
        which = f.stem.split("_")[2]
        for l in f.read_text().splitlines():
            r = json.loads(l)
            t[which].setdefault(r["name"], []).append(r["us_per_launch"])
    ok = bool(t["base"]) and t["base"].keys() == t["new"].keys()
    print("# attention class, us per launch | parent runs | new runs | median parent -> new | parent spread | verdict")
    for name, base in t["base"].items():
        new = t["new"].get(name, [])
        bm, nm, spread = float(np.median(base)), float(np.median(new or [np.inf])), max(base) - min(base)
        good = len(base) == len(new) >= 3 and nm <= bm + spread
        ok &= good
        print(f"{name} | {' '.join(f'{v:.1f}' for v in base)} | {' '.join(f'{v:.1f}' for v in new)} | {bm:.1f} -> {nm:.1f} ({nm / bm:.4f}) | {spread:.1f} | "
              f"{'pass' if good else 'FAIL'}")
    print("VERDICT:", "pass" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) in (4, 5) and sys.argv[1] == "attn":
        attn(*sys.argv[2:])
    elif len(sys.argv) == 3 and sys.argv[1] == "attnspeed":
        sys.exit(attnspeed(sys.argv[2]))
    elif len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "bench":
        bench(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 3 and sys.argv[1] == "speed":
        sys.exit(speed(sys.argv[2]))
    else:
        sys.exit(__doc__)
