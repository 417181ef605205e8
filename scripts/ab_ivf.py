"""Same-box A/B of the batched IVF probes between two builds of the library (written for the split of sc_ivf.cpp, where host
planning time is the only thing that can move; scripts/ab_ivf.sh drives it).  One process per run:

    python scripts/ab_ivf.py run LIB.so OUT.json     1M x 768 clustered rows, nlist 1024, nprobe 16, k 10: ms per batch (median of 30
                                                     after 5 warm-up searches) for Q in {1024, 32} x {ivf_listmajor, ivf_coarse}, the
                                                     probe statistics and a sha256 of the results
    python scripts/ab_ivf.py trace LIB.so            the same searches, three each, with SC_IVF_TRACE set by the caller: the library's
                                                     own phase times ("host plan ... ms" of the list-major probe) on stderr
    python scripts/ab_ivf.py benchivf LIB.so         the IVF_FLAT block of bench.py --full (bench_ivf, its default 10M x 3072 config) alone
    python scripts/ab_ivf.py report DIR              DIR/run_<i>_{new,base}.json: results bit for bit, medians per point; a point passes
                                                     if the new median is not above the parent's by more than the parent's max - min
"""
import hashlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
ROWS, DIM, NLIST, NPROBE, K = 1_000_000, 768, 1024, 16, 10
POINTS = [(mode, Q) for mode in ("ivf_listmajor", "ivf_coarse") for Q in (1024, 32)]


def use_lib(lib_path):
    """Point the binding at one build; entry points that build lacks (the parent's: added since) are not part of the comparison."""
    import ctypes

    import torch  # noqa: F401  (first: the binding's own loading order)

    from semcode_amd import _native as nv

    nv.LIB_PATH = Path(lib_path).resolve()
    handle = ctypes.CDLL(str(nv.LIB_PATH))
    for name in [n for n in nv.SIGNATURES if not hasattr(handle, n)]:
        print(f"{lib_path} lacks {name}", file=sys.stderr)
        del nv.SIGNATURES[name]
    return nv


def setup(lib_path):
    import torch

    nv = use_lib(lib_path)
    stream = torch.cuda.Stream()
    rt = nv.Runtime(device=0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)
    ix = nv.Index(rt, DIM, metric="L2", kind="IVF_FLAT", nlist=NLIST)
    ix.fill_synthetic_clustered(ROWS, seed=0, nclusters=NLIST, spread=0.5)
    qsrc = nv.Index(rt, DIM, metric="L2")
    qsrc.fill_synthetic_clustered(1024, seed=0, nclusters=NLIST, spread=0.5, first_row=ROWS + 12345)
    q = torch.from_numpy(qsrc.get_rows(0, 1024)).to(dev)
    qsrc.close()
    ix.train(niter=5)
    od = torch.empty((1024, K), dtype=torch.float32, device=dev)
    orow = torch.empty((1024, K), dtype=torch.int64, device=dev)

    def search(Q):
        ix.search_dev(q.data_ptr(), Q, K, od.data_ptr(), orow.data_ptr(), nprobe=NPROBE)
        rt.synchronize()

    return rt, ix, search, od, orow, stream


def run(lib_path, out_path):
    rt, ix, search, od, orow, _ = setup(lib_path)
    res = {}
    for mode, Q in POINTS:
        ix.set_search_mode(mode)
        for _ in range(5):
            search(Q)
        ms = []
        for _ in range(30):
            t0 = time.perf_counter()
            search(Q)
            ms.append(1e3 * (time.perf_counter() - t0))
        st = ix.last_search_stats()
        h = hashlib.sha256(orow[:Q].cpu().numpy().tobytes() + od[:Q].cpu().numpy().tobytes()).hexdigest()
        res[f"{mode} Q={Q}"] = {"ms_per_batch": float(np.median(ms)), "min": min(ms), "path": st["path"], "uncertified": st["uncertified"], "probe_stats": ix.last_probe_stats(),
                                "results_sha256": h}
        print(f"{mode} Q={Q}: {res[f'{mode} Q={Q}']}", flush=True)
    Path(out_path).write_text(json.dumps(res) + "\n")
    ix.close()
    rt.close()


def trace(lib_path):
    rt, ix, search, *_ = setup(lib_path)
    for mode, Q in POINTS:
        ix.set_search_mode(mode)
        for _ in range(3):
            print(f"--- {mode} Q={Q}", file=sys.stderr, flush=True)
            search(Q)
    ix.close()
    rt.close()


def benchivf(lib_path):
    import importlib.util

    import torch

    nv = use_lib(lib_path)
    spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sys.argv = ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2", "--full"]
    args = bench.parse()
    ctx = bench.Ctx()
    ctx.world, ctx.rank, ctx.dev = 1, 0, torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=ctx.dev)
    ctx.rt = nv.Runtime(device=0, stream=stream.cuda_stream)
    with torch.cuda.stream(stream):
        res = bench.bench_ivf(ctx, args)
    res.pop("outputs")
    print(json.dumps(res), flush=True)


def report(dirname):
    runs = {"new": [], "base": []}
    for f in sorted(Path(dirname).glob("run_*.json")):
        runs[f.stem.split("_")[2]].append(json.loads(f.read_text()))
    ok = len(runs["new"]) >= 3 and len(runs["base"]) >= 3
    for point in (f"{mode} Q={Q}" for mode, Q in POINTS):
        new, base = ([r[point]["ms_per_batch"] for r in runs[w]] for w in ("new", "base"))
        same = len({json.dumps({k: r[point][k] for k in ("results_sha256", "probe_stats", "path", "uncertified")}, sort_keys=True) for w in runs for r in runs[w]}) == 1
        nm, bm, spread = float(np.median(new)), float(np.median(base)), max(base) - min(base)
        good = same and nm <= bm + spread
        ok &= good
        print(f"{point}: parent {' '.join(f'{v:.3f}' for v in base)} | new {' '.join(f'{v:.3f}' for v in new)} ms per batch; median parent {bm:.3f} new {nm:.3f} "
              f"(parent spread {spread:.3f}); results, path and probe statistics {'identical' if same else 'DIFFERENT'}: {'pass' if good else 'FAIL'}")
    print("VERDICT:", "pass" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "run" and len(sys.argv) == 4:
        run(sys.argv[2], sys.argv[3])
    elif cmd in ("trace", "benchivf") and len(sys.argv) == 3:
        {"trace": trace, "benchivf": benchivf}[cmd](sys.argv[2])
    elif cmd == "report" and len(sys.argv) == 3:
        sys.exit(report(sys.argv[2]))
    else:
        sys.exit(__doc__)
