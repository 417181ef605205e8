"""CPU: the numpy restatement of nomic-bert (tests/nomic_ref.py) reproduces transformers' NomicBertModel.

tests/golden/nomic_golden.npz holds the pooled vectors NomicBertModel (fp32, eager attention) gives for seeded weights
(scripts/gen_nomic_fixtures.py); the restatement must land within 1e-5 of every one.  That pins rotate-half pairing, the rotary
base, gate-first SwiGLU, bias-free Linear layers, the type-0 embedding and masked mean pooling to an implementation outside this
repository; the GPU tests (tests/test_nomic_gpu.py) then compare the kernels with the same vectors."""
import json

import numpy as np
import pytest

import nomic_ref as nr


@pytest.fixture(scope="module")
def nomic_golden(golden):
    return np.load(golden / "nomic_golden.npz"), json.loads((golden / "nomic_golden.json").read_text())


CASES = ["tiny", "mid", "long", "mid_theta10000", "base", "base_long"]


def test_golden_file_holds_the_cases_and_no_weights(nomic_golden, golden):
    data, meta = nomic_golden
    assert sorted(meta) == sorted(CASES)
    assert sorted(data.files) == sorted(f"{c}_{k}" for c in CASES for k in ("ids", "lens", "pooled"))
    assert (golden / "nomic_golden.npz").stat().st_size < 100_000
    assert meta["base"]["cfg"]["hidden"] == 768 and meta["base_long"]["S"] == 2048 and meta["mid_theta10000"]["theta"] == 10000.0


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_transformers_golden(nomic_golden, case):
    data, meta = nomic_golden
    m = meta[case]
    blob = nr.make_weights(m["cfg"], m["seed"], m["qk_scale"])
    got = nr.forward(m["cfg"], blob, data[f"{case}_ids"].astype(np.int32), data[f"{case}_lens"], m["theta"])
    d = float(np.abs(got - data[f"{case}_pooled"]).max())
    print(f"{case}: max|d| = {d:.2e}")
    assert d <= 1e-5, d
