"""CPU: the plan of a packed encoder call (semcode_amd/csrc/sc_encoder_plan.cpp) through sc_diag_encoder_plan -- no device, no encoder.

The plan is what embed_packed_locked uploads: padded ids, a position per row, starts, lens, the attention work items and, by the kind of
call, segment ids and unit lengths (pairs) or the output row of every row (token calls).  It is checked against a NumPy restatement of the
rules of include/semcode_hip.h written here, and the refusals against the message texts of the entry points."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
LENS = [1, 31, 32, 33, 128, 129, 256, 257, 2048]
MAX_ROWS = 524288  # SC_ENCODER_PACKED_MAX_ROWS
MAX_NQ = 128       # MAXSIM_MAX_NQ


@pytest.fixture(scope="module")
def nv():
    from semcode_amd.csrc import build

    build.build(verbose=False)
    from semcode_amd import _native

    return _native


def batch(lens, seed=0):
    lens = np.asarray(lens, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.random.default_rng(seed).integers(1, 30000, size=int(offsets[-1])).astype(np.int32)
    return ids, offsets


def ref_plan(ids, offsets, first_lens=None, expand_id=None):
    """The rules restated: text i owns ceil32(len_i) rows from starts[i]; M = the total rounded up to 256."""
    lens = np.diff(offsets)
    span = (lens + 31) // 32 * 32
    starts = np.concatenate([[0], np.cumsum(span)[:-1]])
    rows = int(span.sum())
    M = (rows + 255) // 256 * 256
    r = {"ids": np.zeros(M, np.int32), "pos": np.zeros(M, np.int32), "starts": starts.astype(np.int32), "lens": lens.astype(np.int32), "rows": rows, "M": M}
    for i, (s, n, sp) in enumerate(zip(starts, lens, span)):
        r["ids"][s:s + n] = ids[offsets[i]:offsets[i + 1]]
        r["pos"][s:s + sp] = np.arange(sp)
    items = []
    for cls in range(3):  # 0: longer than 256 tokens, one item per 8 query blocks of 32 rows; 1: up to 256; 2: up to 128, one item each
        mine = [i for i, n in enumerate(lens) if (0 if n > 256 else 1 if n > 128 else 2) == cls]
        items.append([[starts[i], lens[i], qb, 0] for i in mine for qb in (range(0, span[i] // 32, 8) if cls == 0 else [0])])
    r["nitems"] = [len(x) for x in items]
    r["items"] = np.array([it for x in items for it in x], np.int32).reshape(-1)
    if first_lens is not None:
        r["types"] = np.zeros(M, np.int32)
        for s, n, f in zip(starts, lens, first_lens):
            r["types"][s + f:s + n] = 1
        r["ones"] = np.ones(len(lens), np.int32)
    if expand_id is not None:
        r["dst"] = np.full(M, -1, np.int32)
        at = 0
        for s, n, sp in zip(starts, lens, span):
            take = sp if expand_id >= 0 else n
            r["ids"][s + n:s + take] = expand_id
            r["dst"][s:s + take] = np.arange(at, at + take)
            at += take
        r["nrows"] = at
    return r


def same(plan, ref):
    for name, want in ref.items():
        got = plan[name]
        assert np.array_equal(got.reshape(-1), np.asarray(want).reshape(-1)), name


@pytest.mark.parametrize("lens", [LENS, [1]])
def test_texts(nv, lens):
    ids, offsets = batch(lens)
    plan = nv.diag_encoder_plan(ids, offsets)
    ref = ref_plan(ids, offsets)
    same(plan, ref)
    span = (np.asarray(lens) + 31) // 32 * 32
    assert plan["starts"].tolist() == np.concatenate([[0], np.cumsum(span)[:-1]]).tolist()  # the running sum of ceil32
    for s, n, sp in zip(plan["starts"], lens, span):
        assert plan["pos"][s:s + sp].tolist() == list(range(sp))  # restarts per text, over the whole 32-row span
        assert not plan["ids"][s + n:s + sp].any()  # alignment rows
    assert not plan["ids"][span.sum():].any() and not plan["pos"][span.sum():].any() and plan["ids"].size == int(plan["M"][0]) == ref["M"]
    assert "types" not in plan and "dst" not in plan


def test_items(nv):
    ids, offsets = batch(LENS)
    plan = nv.diag_encoder_plan(ids, offsets)
    items, nitems = plan["items"].reshape(-1, 4), plan["nitems"].tolist()
    assert sum(nitems) == len(items) <= int(plan["items_cap"][0]) == len(LENS) + int(plan["M"][0]) // 256
    cls_of = {}
    at = 0
    for cls, n in enumerate(nitems):  # the three classes in order
        for start, length, qb, zero in items[at:at + n]:
            cls_of.setdefault(int(length), set()).add(cls)
            assert zero == 0 and start == plan["starts"][LENS.index(length)]
        at += n
    assert [cls_of[n] for n in (128, 129, 256, 257)] == [{2}, {1}, {1}, {0}]
    for n in (257, 2048):  # class 0: one item per 8 query blocks
        qbs = [int(qb) for _, length, qb, _ in items[:nitems[0]] if length == n]
        assert qbs == list(range(0, (n + 31) // 32, 8))
    assert all(qb == 0 for _, _, qb, _ in items[nitems[0]:])


def test_pairs(nv):
    lens = [2, 33, 64, 129, 300]
    first = [1, 33, 10, 128, 1]  # (33: no second segment)
    ids, offsets = batch(lens)
    plan = nv.diag_encoder_plan(ids, offsets, "pairs", first_lens=first)
    same(plan, ref_plan(ids, offsets, first_lens=first))
    for s, n, f in zip(plan["starts"], lens, first):
        sp = (n + 31) // 32 * 32
        assert not plan["types"][s:s + f].any() and plan["types"][s + f:s + n].all() and not plan["types"][s + n:s + sp].any()
    assert (plan["ones"] == 1).all() and plan["ones"].size == len(lens)
    texts = nv.diag_encoder_plan(ids, offsets)
    nb = int(texts["common_bytes"][0])
    assert nb == int(plan["common_bytes"][0]) == int(texts["plan_bytes"][0]) < int(plan["plan_bytes"][0])
    assert np.array_equal(plan["common"], texts["common"])  # a plan without pairs lies as before


def test_token_calls(nv):
    lens = [1, 31, 32, 33, 100, 128]
    ids, offsets = batch(lens)
    docs = nv.diag_encoder_plan(ids, offsets, "tokens", expand_id=-1)
    same(docs, ref_plan(ids, offsets, expand_id=-1))
    real = np.concatenate([np.arange(s, s + n) for s, n in zip(docs["starts"], lens)])
    assert docs["dst"][real].tolist() == list(range(sum(lens))) and int(docs["nrows"][0]) == sum(lens)
    assert (np.delete(docs["dst"], real) == -1).all()
    qs = nv.diag_encoder_plan(ids, offsets, "tokens", expand_id=103, query=True)
    same(qs, ref_plan(ids, offsets, expand_id=103))
    rows = int(qs["rows"][0])
    assert qs["dst"][:rows].tolist() == list(range(rows)) and (qs["dst"][rows:] == -1).all() and int(qs["nrows"][0]) == rows
    for s, n in zip(qs["starts"], lens):
        assert (qs["ids"][s + n:s + (n + 31) // 32 * 32] == 103).all()
    assert not qs["ids"][rows:].any()


def refused(nv, text, ids, offsets, *args, **kw):
    with pytest.raises(nv.ScError, match=re.escape("sc_diag_encoder_plan: " + text)):
        nv.diag_encoder_plan(ids, offsets, *args, **kw)


def test_refusals_of_every_packed_call(nv):
    z = np.zeros(MAX_ROWS + 4096, np.int32)
    refused(nv, "offsets[0] must be 0 (got 3)", z, [3, 8])
    refused(nv, "text 1 has length 0 (every text needs at least one token)", z, [0, 4, 4, 9])
    refused(nv, "text 0 has 513 tokens, more than 512 (the smaller of 2048 and the model's max_pos)", z, [0, 513], max_pos=512)
    refused(nv, "text 1 has 2049 tokens, more than 2048 (the smaller of 2048 and the model's max_pos)", z, [0, 4, 2053], max_pos=8192)
    nv.diag_encoder_plan(z, [0, 2048], max_pos=512, pos_type=1)  # ALiBi: only the 2048 bound
    refused(nv, "text 0 has 2049 tokens, more than 2048 (the smaller of 2048 and the model's max_pos)", z, [0, 2049], max_pos=512, pos_type=1)
    nv.diag_encoder_plan(z, np.arange(257) * 2048)
    refused(nv, "%d token rows, more than SC_ENCODER_PACKED_MAX_ROWS = %d (split the batch)" % (MAX_ROWS + 2048, MAX_ROWS), z, np.arange(258) * 2048)
    refused(nv, "batch 0 out of range", z, [0])
    refused(nv, "batch 65537 out of range", z, np.arange(65538))


def test_refusals_of_pairs(nv):
    z = np.zeros(64, np.int32)
    refused(nv, "pair 1 has 1 token(s) (a pair needs at least 2)", z, [0, 5, 6], "pairs", first_lens=[2, 1])
    refused(nv, "first_lens[0] = 0 outside 1 .. 5 (the pair's length)", z, [0, 5], "pairs", first_lens=[0])
    refused(nv, "first_lens[1] = 7 outside 1 .. 6 (the pair's length)", z, [0, 5, 11], "pairs", first_lens=[5, 7])
    refused(nv, "pair 0 has a second segment, the model's type_vocab is 1 (needs 2)", z, [0, 5], "pairs", first_lens=[3], type_vocab=1)
    nv.diag_encoder_plan(z, [0, 5], "pairs", first_lens=[5], type_vocab=1)  # one segment needs no second type


def test_refusals_of_token_calls(nv):
    z = np.zeros(512, np.int32)
    long_q = [0, 4, 4 + MAX_NQ + 1]
    refused(nv, "query 1 has %d tokens, more than %d" % (MAX_NQ + 1, MAX_NQ), z, long_q, "tokens", expand_id=103, query=True)
    refused(nv, "query 1 has %d tokens, more than %d" % (MAX_NQ + 1, MAX_NQ), z, long_q, "tokens", expand_id=-1, query=True)
    nv.diag_encoder_plan(z, long_q, "tokens", expand_id=-1)  # documents may be longer
    nv.diag_encoder_plan(z, [0, MAX_NQ], "tokens", expand_id=103, query=True)
    refused(nv, "expand_id 30522 outside the vocabulary (30522 tokens)", z, [0, 4], "tokens", expand_id=30522, query=True, vocab=30522)
    local = dict(arch=1, global_every=3, local_window=6)
    refused(nv, "query 0 has 33 tokens: its last expansion row would see no key within local_window 6", z, [0, 33], "tokens", expand_id=103, query=True, **local)
    nv.diag_encoder_plan(z, [0, 61], "tokens", expand_id=103, query=True, **local)  # 3 expansion rows: the last still reaches the last token
    nv.diag_encoder_plan(z, [0, 33], "tokens", expand_id=-1, query=True, **local)  # no expansion rows
    nv.diag_encoder_plan(z, [0, 33], "tokens", expand_id=103, query=True, arch=1, global_every=1, local_window=6)  # every layer global
