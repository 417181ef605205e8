"""The shared recipe of the late-interaction (ColBERT) tests: seeded models on the BERT and the ModernBERT backbones, their questions and
passages, and a numpy restatement of what sc_encoder_embed_tokens / sc_encoder_score_late compute.  TEST INFRASTRUCTURE ONLY
(tests/test_late_*.py, scripts/gen_late_fixtures.py).

  token vectors: the last hidden state after the model's last norm, times proj [W, H] (no bias), L2-normalised per token.
  question:      [CLS] [Q] words [SEP], then [MASK] rows up to 32 in all; the [MASK] rows are attended as queries and masked as keys.
  passage:       [CLS] [D] words [SEP]; tokens of the skiplist (punctuation) take no part in a maximum.
  score:         sum over the question's rows of the maximum over the passage's kept tokens of the dot product (MaxSim).

The backbone is restated here in float64 for every row of a text with the keys beyond `n_real` masked -- the references the other tests use
run the real rows only.  maxsim_rule is the bit-exact rule of semcode_amd/csrc/maxsim_rule.h in float32, its dot from the oracle's canonical
chain.  tests/golden/late_golden.{npz,json} stores what transformers (fp32, CPU) computes -- not the weights: make_weights / make_proj
rebuild those from the case and its seed.

DEVIATIONS: one deliberate mix-up each, so that the generator can show that the fixtures tell it apart.
"""
from __future__ import annotations

import ctypes as C
import json
from pathlib import Path

import numpy as np

import modernbert_ref as mb
from oracle import bert_oracle as bo
from oracle import sc_oracle as orc

BERT_COMMON = dict(vocab=400, max_pos=512, type_vocab=2, ln_eps=1e-12)
MB_COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True, rope_theta=160000.0, rope_theta_local=10000.0)
# name: backbone cfg, W.  "fold": the shapes take the LayerNorm-folded pipeline (every GEMM dimension % 256)
CASES = {
    "bert128": dict(cfg=dict(BERT_COMMON, hidden=128, heads=2, ffn=512, layers=2), W=32, fold=False),
    "bert384": dict(cfg=dict(BERT_COMMON, hidden=384, heads=12, ffn=1536, layers=2), W=96, fold=False),
    "bert768": dict(cfg=dict(BERT_COMMON, hidden=768, heads=12, ffn=3072, layers=1), W=128, fold=True),
    "mb256": dict(cfg=dict(MB_COMMON, hidden=256, heads=4, ffn=512, layers=4, local_window=16, global_every=3), W=128, fold=False),
}
PAD_ID, CLS_ID, SEP_ID, MASK_ID, Q_ID, D_ID = 0, 1, 2, 3, 4, 5
SKIP_IDS = (6, 7, 8, 9)  # the punctuation of the skiplist
FIRST_WORD = 12
QUERY_LEN = 32
N_QUESTIONS, N_PASSAGES = 4, 6
# Question lengths.  One has exactly 32 tokens (no expansion row).  On the pre-norm case a question keeps 24 tokens or more: an expansion row
# at position j sees the real keys within local_window / 2 = 8 positions in the local layers, and a row that sees no key at all has no
# defined attention output (transformers gives it the mean of every value row, masked ones included; the library refuses such a call).
Q_LENS = {0: (3, 11, 20, 32), 1: (24, 27, 30, 32)}
P_LENS = {0: (2, 17, 33, 64, 130, 300), 1: (2, 17, 33, 130, 300, 1100)}
DEVIATIONS = ("unnormalised", "no_expansion", "expansion_attended", "expansion_token0", "skiplist_ignored", "sum_max_swapped", "markers_swapped",
              "pre_norm_rows")


def arch_of(case: dict) -> int:
    return 1 if case["cfg"].get("modernbert") else 0


def make_weights(case: dict, seed: int, scale: float) -> np.ndarray:
    """arch 0: bert_oracle's "test" blob with Wq, Wk, Wv, Wo times `scale`; arch 1: modernbert_ref.make_weights with its scales times scale / 4."""
    cfg = case["cfg"]
    if arch_of(case) == 1:
        blob = mb.make_weights(cfg, seed, 8.0 * scale / 4.0, 3.0 * scale / 4.0, 3.0, 0.6)
        g = mb.unpack(cfg, blob)["final_g"]
        g[:] = 1.0 + 6.0 * (g - 1.0)  # the last norm bends the rows: a projection of the rows in front of it shows
        return blob
    blob = bo.make_blob(cfg, seed, "test").copy()
    W = bo.unpack(cfg, blob)
    for l in range(cfg["layers"]):
        for n in ("wq", "wk", "wv", "wo"):
            W[f"l{l}.{n}"] *= np.float32(scale)
    last = f"l{cfg['layers'] - 1}."
    W[last + "ln2_g"][:] = 1.0 + 6.0 * (W[last + "ln2_g"] - 1.0)  # (as above)
    W[last + "ln2_b"][:] *= 6.0
    return blob


def make_proj(case: dict, seed: int) -> np.ndarray:
    """linear.weight [W, H] ~ N(0, 1 / H)."""
    H = case["cfg"]["hidden"]
    rng = np.random.default_rng(55000 + seed)
    return (rng.standard_normal((case["W"], H)) / np.sqrt(H)).astype(np.float32)


def make_texts(case: dict, seed: int):
    """(questions, passages): lists of int32 id arrays, unexpanded.  Passage p shares words with question p % N_QUESTIONS; every passage
    longer than 2 tokens holds skiplist tokens."""
    cfg, a = case["cfg"], arch_of(case)
    rng = np.random.default_rng(88000 + seed)
    words = lambda n: rng.integers(FIRST_WORD, cfg["vocab"], max(0, n)).tolist()  # noqa: E731
    qs = [[CLS_ID, Q_ID] + words(n - 3) + [SEP_ID] for n in Q_LENS[a]]
    ps = []
    for p, n in enumerate(P_LENS[a]):
        if n == 2:
            ps.append([CLS_ID, D_ID])
            continue
        body = words(n - 3)
        own = qs[p % N_QUESTIONS][2:-1]
        for i, wd in enumerate(own):  # the question's words, spread over the passage
            if body:
                body[(7 * i + 3) % len(body)] = wd
        for i in range(1, len(body), 5):
            body[i] = SKIP_IDS[(i // 5) % len(SKIP_IDS)]
        ps.append([CLS_ID, D_ID] + body + [SEP_ID])
    return [np.asarray(q, np.int32) for q in qs], [np.asarray(p, np.int32) for p in ps]


def expand(q: np.ndarray, fill: int = MASK_ID) -> np.ndarray:
    n = (len(q) + QUERY_LEN - 1) // QUERY_LEN * QUERY_LEN
    return np.concatenate([q, np.full(n - len(q), fill, np.int32)])


def keep_flags(p: np.ndarray) -> np.ndarray:
    return (~np.isin(p, SKIP_IDS)).astype(np.uint8)


def pack(texts) -> "tuple[np.ndarray, np.ndarray]":
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return np.concatenate(texts).astype(np.int32), off


# ---------------------------------------------------------------- the backbone, every row, keys beyond n_real masked
def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps) * g + b


def _gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def hidden_rows(case: dict, Wt: dict, ids: np.ndarray, n_real: int):
    """ids [n] (expansion rows included) -> (rows before the model's last norm, rows after it), float64 [n, H]."""
    cfg = case["cfg"]
    n, H, nh, eps = len(ids), cfg["hidden"], cfg["heads"], cfg["ln_eps"]
    dh = H // nh
    sp = lambda t: t.reshape(n, nh, dh).transpose(1, 0, 2)  # noqa: E731
    keymask = np.where(np.arange(n) < n_real, 0.0, -np.inf)[None, None, :]

    def attend(q, k, v, extra=0.0):
        s = q @ k.transpose(0, 2, 1) / np.sqrt(dh) + keymask + extra
        e = np.exp(s - s.max(-1, keepdims=True))
        return ((e / e.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(n, H)

    if arch_of(case) == 0:
        x = _ln(Wt["word_emb"][ids] + Wt["pos_emb"][np.arange(n)] + Wt["type_emb"][0], Wt["emb_ln_g"], Wt["emb_ln_b"], eps)
        pre = x
        for l in range(cfg["layers"]):
            p = f"l{l}."
            q, k, v = (sp(x @ Wt[p + "w" + c].T + Wt[p + "b" + c]) for c in "qkv")
            x = _ln(attend(q, k, v) @ Wt[p + "wo"].T + Wt[p + "bo"] + x, Wt[p + "ln1_g"], Wt[p + "ln1_b"], eps)
            pre = _gelu(x @ Wt[p + "w1"].T + Wt[p + "b1"]) @ Wt[p + "w2"].T + Wt[p + "b2"] + x
            x = _ln(pre, Wt[p + "ln2_g"], Wt[p + "ln2_b"], eps)
        return pre, x
    F, half = cfg["ffn"], int(cfg["local_window"]) // 2
    tabs = {True: mb.rope_tables(n, cfg["rope_theta"], dh), False: mb.rope_tables(n, cfg["rope_theta_local"], dh)}
    band = np.where(np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) <= half, 0.0, -np.inf)[None]
    h = _ln(Wt["word_emb"][ids], Wt["emb_ln_g"], Wt["emb_ln_b"], eps)
    for l in range(cfg["layers"]):
        p, glob = f"l{l}.", mb.is_global(cfg, l)
        a = h if l == 0 else _ln(h, Wt[p + "ln1_g"], Wt[p + "ln1_b"], eps)
        q, k, v = (sp(a @ Wt[p + "w" + c].T + Wt[p + "b" + c]) for c in "qkv")
        cos, sin = tabs[glob]
        h = attend(mb.rotate_half(q, cos, sin), mb.rotate_half(k, cos, sin), v, 0.0 if glob else band) @ Wt[p + "wo"].T + Wt[p + "bo"] + h
        u = _ln(h, Wt[p + "ln2_g"], Wt[p + "ln2_b"], eps) @ Wt[p + "w1"].T + Wt[p + "b1"]
        h = (_gelu(u[:, :F]) * u[:, F:]) @ Wt[p + "w2"].T + Wt[p + "b2"] + h
    return h, _ln(h, Wt["final_g"], Wt["final_b"], eps)


def unpack64(case: dict, blob: np.ndarray) -> dict:
    mod = mb if arch_of(case) == 1 else bo
    return {k: v.astype(np.float64) for k, v in mod.unpack(case["cfg"], blob).items()}


def token_vectors(case: dict, Wt: dict, proj: np.ndarray, ids: np.ndarray, n_real: int, deviate: "str | None" = None) -> np.ndarray:
    pre, post = hidden_rows(case, Wt, ids, n_real)
    v = (pre if deviate == "pre_norm_rows" else post) @ proj.astype(np.float64).T
    return v if deviate == "unnormalised" else v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)


def question_vectors(case, Wt, proj, q, deviate=None):
    if deviate == "markers_swapped":
        q = np.where(q == Q_ID, D_ID, q)
    if deviate == "no_expansion":
        return token_vectors(case, Wt, proj, q, len(q), deviate)
    ids = expand(q, PAD_ID if deviate == "expansion_token0" else MASK_ID)
    return token_vectors(case, Wt, proj, ids, len(ids) if deviate == "expansion_attended" else len(q), deviate)


def passage_vectors(case, Wt, proj, p, deviate=None):
    if deviate == "markers_swapped":
        p = np.where(p == D_ID, Q_ID, p)
    return token_vectors(case, Wt, proj, p, len(p), deviate)


def maxsim64(Qv, Dv, keep, deviate=None) -> float:
    s = Qv @ Dv[np.ones(len(Dv), bool) if deviate == "skiplist_ignored" else keep.astype(bool)].T
    return float(s.sum(1).max() if deviate == "sum_max_swapped" else s.max(1).sum())


def applicable(dev: str, q: np.ndarray, p: np.ndarray) -> bool:
    """Whether a mix-up differs from the model at all for this pair."""
    if dev in ("no_expansion", "expansion_attended", "expansion_token0"):
        return len(q) % QUERY_LEN != 0
    if dev == "skiplist_ignored":
        return bool(np.isin(p, SKIP_IDS).any())
    if dev == "sum_max_swapped":
        return int(keep_flags(p).sum()) > 1
    return True


def forward(case: dict, blob: np.ndarray, proj: np.ndarray, questions, passages, deviate: "str | None" = None):
    """-> (question vectors list, passage vectors list, scores [nq, np]) float64."""
    Wt = unpack64(case, blob)
    qv = [question_vectors(case, Wt, proj, q, deviate) for q in questions]
    dv = [passage_vectors(case, Wt, proj, p, deviate) for p in passages]
    sc = np.array([[maxsim64(a, b, keep_flags(p), deviate) for b, p in zip(dv, passages)] for a in qv])
    return qv, dv, sc


def ordered_pairs(score_row: np.ndarray, gap: float) -> "list[tuple[int, int]]":
    n = len(score_row)
    return [(i, j) for i in range(n) for j in range(n) if score_row[i] - score_row[j] > gap]


def stored_rows(n: int) -> np.ndarray:
    """Rows of a passage of n tokens whose vectors the golden file keeps (the file has a size limit): all up to 130 tokens, beyond that every
    4th (every 8th beyond 512 tokens) and the last 8."""
    if n <= 130:
        return np.arange(n)
    step = 8 if n > 512 else 4
    return np.unique(np.concatenate([np.arange(0, n, step), np.arange(n - 8, n)]))


# ---------------------------------------------------------------- the bit-exact rule (semcode_amd/csrc/maxsim_rule.h) in float32
def _key(v: np.ndarray) -> np.ndarray:
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _unkey(u) -> np.float32:
    u = np.uint32(u)
    u = (u & np.uint32(0x7FFFFFFF)) if (u & np.uint32(0x80000000)) else ~u
    return np.array([u], np.uint32).view(np.float32)[0]


def oracle_dots(Q: np.ndarray, D: np.ndarray) -> np.ndarray:
    """[nq, nd] float32: every dot by the oracle's canonical fmaf chain."""
    Q, D = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(D, np.float32)
    f, W = orc.lib().sc_oracle_dot, Q.shape[1]
    qp, dp = Q.ctypes.data, D.ctypes.data
    out = np.empty((len(Q), len(D)), np.float32)
    for t in range(len(Q)):
        for j in range(len(D)):
            out[t, j] = f(C.c_void_p(dp + 4 * W * j), C.c_void_p(qp + 4 * W * t), W)
    return out


def maxsim_rule(Q: np.ndarray, D: np.ndarray, keep: "np.ndarray | None" = None) -> np.float32:
    dots = oracle_dots(Q, D)
    if keep is not None:
        dots = dots[:, np.asarray(keep).astype(bool)]
    acc = np.float32(0.0)
    for t in range(len(Q)):
        m = _unkey(_key(dots[t]).max()) if dots.shape[1] else np.float32(-np.inf)
        acc = np.float32(acc + m)
    return acc


# ---------------------------------------------------------------- transformers names and the two directory layouts
def hf_model_config(case: dict) -> dict:
    cfg = case["cfg"]
    if arch_of(case) == 1:
        return mb.hf_config(cfg)
    return {"model_type": "bert", "vocab_size": cfg["vocab"], "hidden_size": cfg["hidden"], "num_hidden_layers": cfg["layers"], "num_attention_heads": cfg["heads"],
            "intermediate_size": cfg["ffn"], "max_position_embeddings": cfg["max_pos"], "type_vocab_size": cfg["type_vocab"], "layer_norm_eps": cfg["ln_eps"],
            "hidden_act": "gelu", "pad_token_id": 0}


def hf_state_dict(case: dict, blob: np.ndarray) -> dict:
    """Backbone tensors under transformers' BertModel / ModernBertModel names (numpy arrays)."""
    if arch_of(case) == 1:
        return mb.to_hf_state_dict(case["cfg"], blob)
    return {k: np.ascontiguousarray(v.numpy()) for k, v in bo.to_hf_state_dict(case["cfg"], blob).items()}


def vocab_lines(cfg: dict) -> "list[str]":
    names = {PAD_ID: "[PAD]", CLS_ID: "[CLS]", SEP_ID: "[SEP]", MASK_ID: "[MASK]", Q_ID: "[unused0]", D_ID: "[unused1]", 6: ".", 7: ",", 8: "!", 9: "?", 10: "[UNK]",
             11: "[unused2]"}
    return [names.get(i, f"w{i}") for i in range(cfg["vocab"])]


def text_of(ids: np.ndarray, cfg: dict) -> str:
    """The words of a question or passage (markers, [CLS] and [SEP] left out) as text the WordPiece tokenizer maps back to the ids."""
    v = vocab_lines(cfg)
    return " ".join(v[i] for i in ids if i not in (CLS_ID, SEP_ID, Q_ID, D_ID))


def write_pylate_dir(path: Path, case: dict, blob: np.ndarray, proj: np.ndarray, **overrides) -> Path:
    from safetensors.numpy import save_file

    path = Path(path)
    (path / "1_Dense").mkdir(parents=True, exist_ok=True)
    (path / "config.json").write_text(json.dumps(hf_model_config(case)))
    save_file(hf_state_dict(case, blob), str(path / "model.safetensors"))
    dense = {"linear.weight": np.ascontiguousarray(proj)}
    if overrides.pop("bias", False):
        dense["linear.bias"] = np.zeros(len(proj), np.float32)
    save_file(dense, str(path / "1_Dense" / "model.safetensors"))
    (path / "vocab.txt").write_text("\n".join(vocab_lines(case["cfg"])) + "\n")
    st = dict(query_prefix="[unused0]", document_prefix="[unused1]", query_length=QUERY_LEN, document_length=300, attend_to_expansion_tokens=False,
              skiplist_words=[".", ",", "!", "?"])
    st.update(overrides)
    (path / "config_sentence_transformers.json").write_text(json.dumps(st))
    return path


def write_stanford_dir(path: Path, case: dict, blob: np.ndarray, proj: np.ndarray, **overrides) -> Path:
    from safetensors.numpy import save_file

    assert arch_of(case) == 0
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    (path / "config.json").write_text(json.dumps(hf_model_config(case)))
    sd = {"bert." + k: v for k, v in hf_state_dict(case, blob).items()}
    sd["linear.weight"] = np.ascontiguousarray(proj)
    if overrides.pop("bias", False):
        sd["linear.bias"] = np.zeros(len(proj), np.float32)
    save_file(sd, str(path / "model.safetensors"))
    (path / "vocab.txt").write_text("\n".join(vocab_lines(case["cfg"])) + "\n")
    meta = dict(query_maxlen=QUERY_LEN, doc_maxlen=300, dim=case["W"], mask_punctuation=True, attend_to_mask_tokens=False)
    meta.update(overrides)
    (path / "artifact.metadata").write_text(json.dumps(meta))
    return path
