"""GPU: every dense-search path on degenerate VALUES (tests/degenerate_data.py) against the CPU oracle, through the public C ABI.

Bar, for every search below: rows == the oracle's rows and the uint32 view of the distances == the oracle's, ties to the lower row.
Per (family, metric) case one fresh FLAT index (and one fresh IVF_FLAT index for the probes), the oracle's answers computed once:

  exact mode      Q = 1, 16, 40; k = 10 (copies100: also k = 128)
  batched mode    coarse stage 0 / 8 / 16 x Q = 40 (narrow kernel) / 200 (256-query tiles), k = 10; stage 0 is set again before each
                  auto-stage search (the int8 stage's self-switch-off is per index); copies*, ternary, scaled+0 also k = 100 at stages
                  0 and 8; once more at stage 8 with wide_candidates = 1 and at stage 0 with collect_pass = 0.  path == "batched" and
                  coarse_bits as pinned are asserted, so a silent detour through another path shows; uncertified / handed_to_bf16 /
                  collect_tried / collect_resolved are printed per search ("COUNTERS" lines) and NOT capped: on these inputs a sound
                  certificate is expected to refuse often.  The one guard against vacuity: scaled+0 and scaled+12 at stages 8 and 16
                  answer something by themselves (uncertified < Q; holds at dim 64).
  search_masked   all ones with mask_gather forced to 1; a seeded random half (reference: the oracle over the allowed rows, mapped back)
  IVF_FLAT        nlist 64, train(niter=4, seed=0); modes ivf / ivf_listmajor / ivf_coarse at nprobe = 64 each equal the flat oracle,
                  at nprobe = 8 each other bit for bit; Q = 40 and 200.  train() refusing a family with an ScError would skip only
                  this leg of that case; no family does.
  scaled(s != 0)  additionally the device's own results on every path above equal its results on scaled(0) under the scaling law of
                  tests/test_degenerate_values_host.py (same rows; IP / L2 distances times 2^(2 s) bit for bit, COSINE unchanged).

What the planner does with two of the requested combinations at this size (140 000 rows), so that the assertions say what runs:
k = 100 with the bf16 stage pinned is not a batched search (only the int8 stage keeps the 512 candidates top_k > 64 needs; the planner
answers it with the exact scan), so k = 100 runs at stages 0 and 8; and the wide candidate set needs more than 2^18 rows, so here
k = 100 and wide_candidates = 1 are answered by the plain form (512 candidates re-scored for the cut) -- `wide` is printed, not asserted;
test_wide_form_on_tied_rows runs the same paths over 280 000 rows of copies(100), where the wide form does run, and asserts it.

Observed (MI355X): no path returned a wrong row or bit on any family; the stages refuse rather than err -- see the table in DESIGN.md
section 4 ("Degenerate values").  train() refused no family.
"""
import time

import numpy as np
import pytest

import degenerate_data as dd
from oracle import sc_oracle as orc
from semcode_amd import _native

pytestmark = pytest.mark.gpu

METRICS = ["IP", "L2", "COSINE"]
K100 = ("copies1500", "copies100", "copies12", "ternary", "scaled+0")
bits = dd.bits


class Answers:
    """The oracle's answers of one (family, metric) case, each computed once (every query subset is a prefix of the 200)."""

    def __init__(self, X, Q, metric):
        self.X, self.Q, self.metric, self._top = X, Q, metric, {}

    def top(self, nq, k):
        key = (k, 40 if (k > 100 and nq <= 40) else len(self.Q))
        if key not in self._top:
            self._top[key] = orc.search(self.X, self.Q[:key[1]], k, self.metric)
        d, r = self._top[key]
        return d[:nq], r[:nq]

    def masked(self, allowed, nq, k):
        idx = np.flatnonzero(allowed)
        d, r = orc.search(self.X[idx], self.Q[:nq], k, self.metric)
        return d, np.where(r >= 0, idx[np.clip(r, 0, None)], -1)


def same(got, want, what):
    (d, r), (od, orow) = got, want
    assert np.array_equal(r, orow), f"{what}: rows / order differ from the reference in {int((r != orow).any(axis=1).sum())} of {len(r)} queries"
    assert np.array_equal(bits(d), bits(od)), f"{what}: distances not bit-exact"


def flat_paths(rt, X, Q, metric, name, tag, expect_wide=False):
    """label -> (nq, k, dist, rows) of every flat path on a fresh index over X."""
    out = {}
    ix = _native.Index(rt, X.shape[1], metric=metric)
    ix.add(X)
    try:
        ix.set_search_mode("exact")
        for nq, k in [(1, 10), (16, 10), (40, 10)] + ([(40, 128)] if name == "copies100" else []):
            out[f"exact Q={nq} k={k}"] = (nq, k) + ix.search(Q[:nq], k=k)
            assert ix.last_search_stats()["path"] == "exact"
        ix.set_search_mode("batched")

        def batched(label, stage, nq, k):
            ix.set_coarse_stage(stage)  # (0: also clears the int8 stage's switch-off)
            d, r = ix.search(Q[:nq], k=k)
            st = ix.last_search_stats()
            assert st["path"] == "batched" and st["coarse_bits"] == (16 if stage == 16 else 8), (label, st)
            print(f"COUNTERS {tag} | {label} | Q={nq} uncertified={st['uncertified']} handed_to_bf16={st['handed_to_bf16']} "
                  f"collect_tried={st['collect_tried']} collect_resolved={st['collect_resolved']} wide={int(st['wide'])}")
            out[label] = (nq, k, d, r)
            if expect_wide and (k > 64 or "wide_candidates" in label):
                assert st["wide"], (label, st)
            return st

        for stage in (0, 8, 16):
            for nq in (40, 200):
                st = batched(f"batched stage={stage} Q={nq} k=10", stage, nq, 10)
                if name in ("scaled+0", "scaled+12") and stage in (8, 16):
                    assert st["uncertified"] < nq, (stage, st)  # the stage answers something by itself
        if name in K100:
            for stage in (0, 8):
                for nq in (40, 200):
                    batched(f"batched stage={stage} Q={nq} k=100", stage, nq, 100)
        try:
            _native.diag_set_option("wide_candidates", 1)
            batched("batched stage=8 Q=200 k=10 wide_candidates=1", 8, 200, 10)
        finally:
            _native.diag_set_option("wide_candidates", 0)
        try:
            _native.diag_set_option("collect_pass", 0)
            st = batched("batched stage=0 Q=200 k=10 collect_pass=0", 0, 200, 10)
            assert st["collect_tried"] == 0, st
        finally:
            _native.diag_set_option("collect_pass", 1)
        ix.set_coarse_stage(0)
        ix.set_search_mode("auto")
        # masked
        n = len(X)
        try:
            _native.diag_set_option("mask_gather", 1)
            out["masked all ones, gathered"] = (40, 10) + ix.search_masked(Q[:40], np.ones(n, bool), k=10)
            assert ix.last_search_stats()["path"] == "masked" and ix.last_mask_stats() == {"allowed_rows": n, "scanned_rows": n, "gathered": True}
        finally:
            _native.diag_set_option("mask_gather", 0)
        half = half_mask(n)
        out["masked half"] = (40, 10) + ix.search_masked(Q[:40], half, k=10)
        assert ix.last_mask_stats()["allowed_rows"] == int(half.sum())
    finally:
        ix.close()
    return out


def half_mask(n):
    return np.random.default_rng(77).random(n) < 0.5


def ivf_paths(rt, X, Q, metric, tag):
    """The trained IVF_FLAT legs: label -> (nq, k, dist, rows); the nprobe = 8 entries are compared with each other here."""
    out = {}
    ix = _native.Index(rt, X.shape[1], metric=metric, kind="IVF_FLAT", nlist=64)
    ix.add(X)
    try:
        try:
            ix.train(niter=4, seed=0)
        except _native.ScError as e:  # (a refusal skips this leg only; anything else fails the case)
            print(f"IVF {tag}: train refused: {e}")
            return None
        for nq in (40, 200):
            res8 = {}
            for mode in ("ivf", "ivf_listmajor", "ivf_coarse"):
                ix.set_search_mode(mode)
                out[f"{mode} nprobe=64 Q={nq}"] = (nq, 10) + ix.search(Q[:nq], k=10, nprobe=64)
                res8[mode] = ix.search(Q[:nq], k=10, nprobe=8)
                st = ix.last_search_stats()
                print(f"IVF {tag} | {mode} nprobe=8 Q={nq} | path={st['path']} uncertified={st['uncertified']}")
            for mode in ("ivf_listmajor", "ivf_coarse"):
                same(res8[mode], res8["ivf"], f"{tag} {mode} against ivf at nprobe=8 Q={nq}")
            out[f"probes nprobe=8 Q={nq}"] = (nq, 10) + res8["ivf"]
    finally:
        ix.close()
    return out


def check_against_oracle(out, ans, tag):
    n = len(ans.X)
    for label, (nq, k, d, r) in out.items():
        if label.startswith("probes nprobe=8"):
            continue  # a partial probe: compared between the modes, not with the flat oracle
        if label == "masked half":
            want = ans.masked(half_mask(n), nq, k)
        else:
            want = ans.top(nq, k)
        same((d, r), want, f"{tag} {label}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", list(dd.FAMILIES))
def test_every_path_equals_the_oracle(rt, name, metric):
    t0 = time.perf_counter()
    tag = f"{name} {metric}"
    X, Q = dd.family(name)
    ans = Answers(X, Q, metric)
    flat = flat_paths(rt, X, Q, metric, name, tag)
    check_against_oracle(flat, ans, tag)
    ivf = ivf_paths(rt, X, Q, metric, tag)
    assert ivf is not None, "train() refused this family: record it in the module docstring and skip this leg for it"
    check_against_oracle(ivf, ans, tag)
    if name.startswith("scaled") and name != "scaled+0":
        # the device's own results under the scaling law, path by path, against a twin index over scaled(0)
        s = int(name[len("scaled"):])
        X0, Q0 = dd.scaled(0)
        twin = dict(flat_paths(rt, X0, Q0, metric, name, f"scaled+0 (twin of {name}) {metric}"))
        twin.update(ivf_paths(rt, X0, Q0, metric, f"scaled+0 (twin of {name}) {metric}"))
        assert set(twin) == set(flat) | set(ivf)
        for label, (nq, k, d0, r0) in twin.items():
            d, r = ({**flat, **ivf})[label][2:]
            same((d, r), (d0 if metric == "COSINE" else np.ldexp(d0, 2 * s), r0), f"{tag} {label} against the device's own scaled(0)")
    if name == "zero_norm":
        check_zero_norm_properties(flat, X, Q, metric)
    print(f"TIME {tag}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("metric", METRICS)
def test_wide_form_on_tied_rows(rt, metric):
    """The wide candidate set of the int8 stage exists from 2^18 rows on, beyond the 140 000 of the families: copies(100) at 280 000
    rows (2 800 rows tie with the 10th score: above the 512 candidates, below the 4096-entry survivor cap) takes it for k = 100 and
    under wide_candidates = 1 -- asserted -- and every flat path still equals the oracle."""
    X, Q = dd.copies(100, n=280_000)
    tag = f"copies100 n=280000 {metric}"
    flat = flat_paths(rt, X, Q, metric, "copies100", tag, expect_wide=True)
    check_against_oracle(flat, Answers(X, Q, metric), tag)


def check_zero_norm_properties(flat, X, Q, metric):
    """What the rule means for the results themselves, on the device's answers (batched, stage 0, all 200 queries)."""
    nq, k, d, r = flat["batched stage=0 Q=200 k=10"]
    zrows = np.sort(dd.ZERO_ROWS)
    assert not np.isnan(d).any()
    for q in dd.ZERO_QUERIES:
        if metric == "L2":  # the smallest-norm rows: the zero rows at distance 0, in row order
            assert np.array_equal(r[q], zrows[:k]) and (d[q] == 0).all()
        else:  # every score is 0: rows 0 .. k-1
            assert np.array_equal(r[q], np.arange(k)) and (d[q] == 0).all()
    hit = np.isin(r, zrows)
    if metric != "L2":
        assert (d[hit] == 0).all()  # zero rows score 0 (IP; COSINE: the zero-norm rule)
    else:
        qn = np.array([orc.sqnorm(orc.padded(Q[i:i + 1])[0]) for i in range(nq)], np.float32)
        assert np.array_equal(bits(d[hit]), bits(np.broadcast_to(qn[:, None], d.shape)[hit]))  # ... and |q|^2 under L2


def test_fewer_nonzero_rows_than_k(rt):
    """300 rows, 295 of them zero, COSINE, k = 10, batched mode: fewer candidates than a stage keeps and fewer non-zero rows than k.
    The result is the oracle's: ten real rows, never padding -- the rows with a positive cosine, then zero-norm rows at score 0 in
    row order."""
    X, Q = dd.zero_norm_small()
    od, orow = orc.search(X, Q, 10, "COSINE")
    assert (orow >= 0).all() and np.isin(orow, np.flatnonzero(~X.any(axis=1))).sum(axis=1).min() >= 5
    ix = _native.Index(rt, X.shape[1], metric="COSINE")
    ix.add(X)
    try:
        ix.set_search_mode("batched")
        for stage in (0, 8, 16):
            for nq in (1, 40):
                ix.set_coarse_stage(stage)
                d, r = ix.search(Q[:nq], k=10)
                st = ix.last_search_stats()
                assert st["path"] == "batched" and st["coarse_bits"] == (16 if stage == 16 else 8), st
                same((d, r), (od[:nq], orow[:nq]), f"stage {stage} Q={nq}")
        ix.set_search_mode("exact")
        same(ix.search(Q, k=10), (od, orow), "exact")
    finally:
        ix.close()
