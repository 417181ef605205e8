"""CPU: the host planners of batched IVF probing (semcode_amd/csrc/sc_ivf_plan.cpp) through sc_diag_ivf_plan -- no device.

Every valid plan gives bit-identical search results, so the GPU suite cannot see a plan that merely costs speed (a list streamed
twice, the wrong class, the longest-part-first order lost).  Here the plans are checked against their invariants and against
tests/golden/ivf_plan_golden.json, recorded from the planners as they were cut out of the searches, before any simplification:

    python tests/test_ivf_plan_host.py --record
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
GOLDEN = ROOT / "tests" / "golden" / "ivf_plan_golden.json"
CUS = 256
PREFIX = 4096  # rows of a list that phase A of the coarse stage takes
SPECIAL_LENS = [0, 1, 15, 16, 17, 255, 256, 257, 4096, 4097, 30000]
# (queries that probe the list, length of that list): every chunk size at which the list-major planner changes class
TARGETS = {40: [(130, 30000), (65, 4097), (64, 257), (33, 4096), (32, 256), (17, 17), (16, 16), (1, 1)], 8: [(65, 30000), (33, 4097), (17, 256), (1, 1)]}


@pytest.fixture(scope="module")
def nv():
    from semcode_amd.csrc import build

    build.build(verbose=False)
    from semcode_amd import _native

    return _native


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("SC_IVF_WIDE", raising=False)
    monkeypatch.delenv("SC_SCAN_QSTREAM", raising=False)


def make_inputs(nlist: int, nprobe: int):
    """-> probes [Q, nprobe] int64 (with -1 and nlist entries), list_off [nlist + 1] int64"""
    rng = np.random.default_rng(1000 * nlist + nprobe)
    if nlist == 40:
        lens = np.array(SPECIAL_LENS + list(rng.integers(1, 3000, size=nlist - len(SPECIAL_LENS))), np.int64)
    else:
        lens = np.array([30000, 0, 1, 17, 4097, 256, 15, 4096], np.int64)
    lens = lens[rng.permutation(nlist)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if nprobe == nlist - 1:  # every query probes all lists but one, in random order: counts of Q minus a few
        Q = 66 if nlist == 8 else 131
        probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(Q)]).astype(np.int64)
        free = np.argwhere(probes >= 0)
    else:
        # the targets laid out column by column: a list's entries are consecutive cells of at most Q queries, so no query gets a list twice
        targets = TARGETS[nlist]
        by_len = {int(n): i for i, n in enumerate(lens)}
        special = [by_len[n] for _, n in targets]
        others = [l for l in range(nlist) if l not in special]
        seq = np.concatenate([np.full(c, l, np.int64) for (c, _), l in zip(targets, special)])
        Q = max(c for c, _ in targets) if nprobe > 1 else len(seq) + 7
        cells = np.array([others[(q * (nprobe + 1) + j) % len(others)] for j in range(nprobe) for q in range(Q)], np.int64)  # column-major filler
        cells[: len(seq)] = seq
        probes = np.ascontiguousarray(cells.reshape(nprobe, Q).T)
        free = np.argwhere(np.isin(probes, others))  # (the targets keep their counts)
    # some entries are not lists
    pick = free[rng.choice(len(free), size=min(6, len(free)), replace=False)]
    for n, (q, j) in enumerate(pick):
        probes[q, j] = -1 if n % 2 == 0 else nlist
    return probes, off


CASES = [(nlist, nprobe, k, ld, wide) for nlist in (8, 40) for nprobe in (1, 4, nlist - 1) for k in (10, 64) for ld in (64, 3072) for wide in (True, False)]


def case_id(c):
    return "nlist%d-nprobe%d-k%d-ld%d-%s" % (c[0], c[1], c[2], c[3], "wide" if c[4] else "narrow")


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + b"|" + a.tobytes()).hexdigest()


def plans(nv, case):
    nlist, nprobe, k, ld, wide = case
    probes, off = make_inputs(nlist, nprobe)
    return probes, off, {path: nv.diag_ivf_plan(path, probes, off, k, ld, CUS, wide=wide) for path in ("listmajor", "coarse")}


def digest(probes, off, both):
    return {"inputs": sha(np.concatenate([probes.ravel(), off])), **{path: {name: sha(a) for name, a in sorted(p.items())} for path, p in both.items()}}


def test_inputs_reach_every_chunk_size():
    want = {40: {1, 16, 17, 32, 33, 64, 65, 130}, 8: {1, 17, 33, 65}}
    for nlist in (8, 40):
        for nprobe in (1, 4):
            probes, off = make_inputs(nlist, nprobe)
            counts = np.bincount(probes[(probes >= 0) & (probes < nlist)], minlength=nlist)
            assert want[nlist] <= set(counts.tolist()), (nlist, nprobe, counts)
            assert (probes == -1).any() and (probes == nlist).any()
            lens = np.diff(off)
            assert counts[lens == 0].sum() > 0 or nprobe == 1  # an empty list is probed
        probes, off = make_inputs(nlist, nlist - 1)
        assert probes.shape[1] == nlist - 1 and all(len(set(r[(r >= 0) & (r < nlist)])) == ((r >= 0) & (r < nlist)).sum() for r in probes)
    assert set(SPECIAL_LENS) <= set(np.diff(make_inputs(40, 4)[1]).tolist())


def test_long_rows_take_the_streamed_query_plan(nv):
    probes, off = make_inputs(8, 4)
    assert int(nv.diag_ivf_plan("listmajor", probes, off, 10, 3072, CUS)["qstream"][0]) == 1
    assert int(nv.diag_ivf_plan("listmajor", probes, off, 10, 64, CUS)["qstream"][0]) == 0


def scalar(p, name):
    assert p[name].shape == (1,)
    return int(p[name][0])


def check_listmajor(p, probes, off, k, wide):
    Q, nprobe = probes.shape
    nlist = len(off) - 1
    lens = np.diff(off)
    qt, qt_res, mp, L = (scalar(p, n) for n in ("qt", "qt_res", "maxparts", "L"))
    Gw, Gw2, G, G_big = (scalar(p, n) for n in ("Gw", "Gw2", "G", "G_big"))
    assert L == nprobe * mp and p["src"].size == Q * L and 0 <= G_big <= G
    assert mp == 1 or (L >= 1 and k >= 1 and 2 * L * k * 8 <= 128 * 1024)  # sc_topk_gather_merge_supported(L, k)
    if not wide:
        assert Gw == 0 and Gw2 == 0 and scalar(p, "wide_ok") == 0
    # slot tables in the order of `partial`: wide 64, wide 32, narrow (streamed queries first, then resident)
    qs, p0, p1, cls, grp = [], [], [], [], []
    for ci, (qn, sn, stride, g) in enumerate((("qmap_w", "sr_w", 64, Gw), ("qmap_w2", "sr_w2", 32, Gw2), ("qmap", "sr", qt, G))):
        qm, sr = p[qn].reshape(-1, stride), p[sn].reshape(-1, 2)
        assert len(qm) == g and len(sr) == g
        occ = (qm >= 0).sum(1)
        assert ((qm >= 0) == (np.arange(stride)[None, :] < occ[:, None])).all()  # the valid slots are a prefix
        glen = sr[:, 1] - sr[:, 0]
        assert (glen > 0).all()
        if ci == 0:
            assert ((occ >= 33) & (occ <= 64)).all()
        elif ci == 1:
            assert ((occ >= 17) & (occ <= 32)).all()
        else:
            assert ((occ >= 1) & (occ <= qt)).all()
            assert (occ[:G_big] > qt_res).all() and (occ[G_big:] <= qt_res).all()
            assert np.array_equal(p["sb"].reshape(-1, 2), np.stack([np.zeros(g, np.int64), (glen + 15) // 16], 1))
        for part in ((glen,) if ci < 2 else (glen[:G_big], glen[G_big:])):
            assert (np.diff(part) <= 0).all()  # longest parts first inside a class
        qs.append(qm.ravel())
        p0.append(np.repeat(sr[:, 0], stride))
        p1.append(np.repeat(sr[:, 1], stride))
        cls.append(np.full(g * stride, ci))
        grp.append(np.repeat(np.arange(g), stride))
    qs, p0, p1, cls = (np.concatenate(a) for a in (qs, p0, p1, cls))
    assert scalar(p, "lists_w") == Gw * 64 + Gw2 * 32 and scalar(p, "groups") == Gw + Gw2 + G
    src = p["src"].reshape(Q, L)
    used = src[src >= 0]
    assert len(np.unique(used)) == len(used) and np.array_equal(np.sort(used), np.flatnonzero(qs >= 0))  # every used slot named exactly once
    for q in range(Q):
        for j in range(nprobe):
            l, ent = probes[q, j], src[q, j * mp:(j + 1) * mp]
            if l < 0 or l >= nlist or lens[l] == 0:
                assert (ent == -1).all()
                continue
            n = int((ent >= 0).sum())
            sl = ent[:n]
            assert n >= 1 and (ent[n:] == -1).all() and (qs[sl] == q).all() and len(set(cls[sl])) == 1
            assert p0[sl[0]] == off[l] and p1[sl[-1]] == off[l + 1] and np.array_equal(p0[sl[1:]], p1[sl[:-1]])  # the parts tile the list, in part order
    for l in range(nlist):  # the queries of a list ascend across its groups (first parts; a non-empty list's first row is its own)
        if lens[l] > 0:
            want = np.flatnonzero(((probes == l).any(1)))
            assert np.array_equal(qs[(p0 == off[l]) & (qs >= 0)], want)
    streamed = sum(int((p[n].reshape(-1, 2)[:, 1] - p[n].reshape(-1, 2)[:, 0]).sum()) for n in ("sr_w", "sr_w2", "sr"))
    probed = np.unique(probes[(probes >= 0) & (probes < nlist)])
    assert scalar(p, "streamed_rows") == streamed and scalar(p, "unique_rows") == int(lens[probed].sum())


def check_coarse(p, probes, off):
    Q, nprobe = probes.shape
    nlist = len(off) - 1
    lens = np.diff(off)
    KP = scalar(p, "KP")
    sq, sl, sd = p["slot_q"], p["slot_l"], p["slot_dst"]
    assert len(sq) % 64 == 0 and len(sq) == len(sl) == len(sd) and np.array_equal(sq == -1, sl == -1) and scalar(p, "groups") == len(sq) // 64
    valid = (probes >= 0) & (probes < nlist)
    cum = np.cumsum(np.where(valid, np.minimum(lens[np.clip(probes, 0, nlist - 1)], PREFIX), 0), axis=1)
    ja = np.where((cum >= 2 * KP).any(1), (cum >= 2 * KP).argmax(1) + 1, nprobe)
    assert np.array_equal(p["ja"], ja)
    # per group of 64 slots: its items tile one row range in tiles of at most 256 rows
    cover, rows_kind, streamed = {}, [0, 0, 0], 0
    for kind, name in enumerate(("items_a", "items_tail", "items_b")):
        it = p[name]
        assert (it["slot_base"] % 64 == 0).all()
        for base in np.unique(it["slot_base"]):
            g = np.sort(it[it["slot_base"] == base], order="row0")
            assert ((g["rows"] >= 1) & (g["rows"] <= 256)).all() and np.array_equal(g["row0"][1:], g["row0"][:-1] + g["rows"][:-1])
            lo, hi = int(g["row0"][0]), int(g["row0"][-1] + g["rows"][-1])
            gq, gl = sq[base:base + 64], sl[base:base + 64]
            nq = int((gq >= 0).sum())
            assert nq >= 1 and (gq[:nq] >= 0).all() and len(set(gl[:nq])) == 1
            streamed += hi - lo
            rows_kind[kind] += (hi - lo) * nq
            for q in gq[:nq]:
                key = (kind, int(q), int(gl[0]))
                assert key not in cover
                cover[key] = (lo, hi, int(base))
    assert len(np.unique(np.concatenate([p[n]["slot_base"] for n in ("items_a", "items_tail", "items_b")]))) == len(sq) // 64  # every group has items
    expect = {}
    for q in range(Q):
        for j in range(nprobe):
            l = int(probes[q, j])
            if not valid[q, j] or lens[l] == 0:
                continue
            first, end = int(off[l]), int(off[l + 1])
            if j < ja[q]:
                expect[(0, q, l)] = (first, min(end, first + PREFIX))
                if end - first > PREFIX:
                    expect[(1, q, l)] = (first + PREFIX, end)
            else:
                expect[(2, q, l)] = (first, end)
    assert {k_: v[:2] for k_, v in cover.items()} == expect
    # phase A is dense: the rows of a query's phase-A ranges land at (uint32)(row + slot_dst), side by side from 0
    assert p["cntA"].dtype == np.uint32
    spans = [[] for _ in range(Q)]
    for (kind, q, l), (lo, hi, base) in cover.items():
        if kind == 0:
            s = base + int(np.flatnonzero(sq[base:base + 64] == q)[0])
            spans[q].append(((lo + int(sd[s])) % (1 << 32), hi - lo))
    for q in range(Q):
        at = 0
        for start, n in sorted(spans[q]):
            assert start == at
            at += n
        assert at == int(p["cntA"][q])
    assert scalar(p, "two_level") == int(len(p["items_tail"]) > 0 and rows_kind[1] * 4 >= rows_kind[0])
    probed = np.unique(probes[valid])
    assert scalar(p, "streamed_rows") == streamed and scalar(p, "unique_rows") == int(lens[probed].sum())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_plan_invariants_and_golden(nv, case):
    probes, off, both = plans(nv, case)
    check_listmajor(both["listmajor"], probes, off, case[2], case[4])
    check_coarse(both["coarse"], probes, off)
    again = plans(nv, case)[2]
    for path in both:  # two calls give identical bytes
        assert both[path].keys() == again[path].keys() and all(both[path][n].tobytes() == again[path][n].tobytes() for n in both[path])
    golden = json.loads(GOLDEN.read_text())
    assert digest(probes, off, both) == golden[case_id(case)]


def test_cases_differ_where_they_should(nv):
    """The golden would pin nothing if the knobs did not reach the planner: wide on / off and the two row lengths give different plans."""
    a = plans(nv, (40, 4, 10, 64, True))[2]["listmajor"]
    b = plans(nv, (40, 4, 10, 64, False))[2]["listmajor"]
    c = plans(nv, (40, 4, 10, 3072, False))[2]["listmajor"]
    assert scalar(a, "Gw") > 0 and scalar(a, "Gw2") > 0 and scalar(b, "Gw") == 0
    assert scalar(b, "G_big") == 0 and 0 < scalar(c, "G_big") < scalar(c, "G")


@pytest.mark.parametrize("ld", [64, 768, 3072])
@pytest.mark.parametrize("R", [1, 2, 300])
def test_exact_path_of_a_sub_batch(nv, ld, R):
    """The queries the coarse stage cannot certify are probed again exactly: list-major from two queries on while the gather merge
    holds a query's nprobe k-lists (2 * nprobe * k keys of 8 bytes in 128 KiB: nprobe * k <= 8192), per-query probing otherwise --
    which plans one query at a time and whose segment table (20 bytes per probe) and candidate lists (k + 16 rounded up to 64 keys
    per wave) stay far below the scan's 160 KiB at k <= 256, nprobe <= 512, so over the coarse stage's whole range some exact probe
    serves and no batch is refused for its uncertified queries.  The rule and the list-major planner itself agree on where that
    planner has a plan."""
    off = np.array([0, 100], np.int64)  # one list of 100 rows, which every query probes
    for k in (1, 64, 128, 129, 256):
        for nprobe in (2, 32, 64, 512):
            want = "ivf_listmajor" if R >= 2 and nprobe * k <= 8192 else "ivf"
            assert nv.diag_ivf_exact_path(ld, R, k, nprobe, CUS) == want, (ld, R, k, nprobe)
            pr = np.zeros((max(R, 2), nprobe), np.int64)
            if nprobe * k <= 8192:
                nv.diag_ivf_plan("listmajor", pr, off, k, ld, CUS)
            else:
                with pytest.raises(nv.ScError) as e:
                    nv.diag_ivf_plan("listmajor", pr, off, k, ld, CUS)
                assert e.value.status == -4  # SC_ERR_UNSUPPORTED
    # outside what any probe accepts: no path, so the coarse stage must not take the request either
    assert nv.diag_ivf_exact_path(ld, R, 10, 513, CUS) == "none" and nv.diag_ivf_exact_path(ld, R, 1025, 8, CUS) == "none"
    assert nv.diag_ivf_exact_path(ld, 0, 10, 8, CUS) == "none"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    from semcode_amd import _native

    out = {}
    for c in CASES:
        probes, off, both = plans(_native, c)
        out[case_id(c)] = digest(probes, off, both)
    GOLDEN.write_text(json.dumps(out, indent=0, sort_keys=True) + "\n")
    print(f"{len(out)} cases -> {GOLDEN}")
