"""Report of scripts/ab_scan_bench.sh: outputs of new vs parent runs (np.array_equal), QPS per workload against the parent-run noise."""
import json, sys
from pathlib import Path
import numpy as np

d = Path(sys.argv[1])
runs = {}
for log in sorted(d.glob("run_*.log")):
    for l in log.read_text().splitlines():
        if l.startswith("{"):
            runs[log.stem[4:]] = json.loads(l)
names = sorted(runs)  # 1_new 2_base 3_new 4_base
new = [n for n in names if n.endswith("new")]; base = [n for n in names if n.endswith("base")]
ok = True
# outputs
for a, b in zip(new, base):
    fa = sorted((d / f"out_{a}").glob("*.npy")); fb = sorted((d / f"out_{b}").glob("*.npy"))
    assert [f.name for f in fa] == [f.name for f in fb] and fa, (fa, fb)
    for x, y in zip(fa, fb):
        eq = np.array_equal(np.load(x), np.load(y))
        ok &= eq
        print(f"outputs {a} vs {b}: {x.name} {'equal' if eq else 'DIFFERENT'}")
def points(r):
    p = {"Q=1024 headline": r["value"]}
    for s in r.get("sweep", []):
        p[f"sweep Q={s['queries']} {s['mode']}"] = s["qps"]
    return p
P = {n: points(runs[n]) for n in names}
for k in P[names[0]]:
    n1, n2 = (P[n][k] for n in new); b1, b2 = (P[n][k] for n in base)
    noise = abs(b1 - b2); nm = (n1 + n2) / 2; bm = (b1 + b2) / 2
    good = nm >= bm - noise
    ok &= good
    print(f"{k}: new {n1:.1f} {n2:.1f} (mean {nm:.1f}) parent {b1:.1f} {b2:.1f} (mean {bm:.1f}) noise {noise:.1f} ({100 * noise / bm:.2f} %) new/parent {nm / bm:.4f} -> {'ok' if good else 'BELOW'}")
print("uncertified:", {n: runs[n].get("uncertified", runs[n].get("roofline", {}).get("uncertified")) for n in names})
print("VERDICT:", "pass" if ok else "FAIL")
