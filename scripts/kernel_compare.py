"""Kernels of the scan files in two builds of the library, one line per kernel: registers, scratch, LDS, occupancy, instruction count,
and whether the instruction text is identical (labels renumbered, comments dropped).  Written for the split of scan_batched.hip
by stage (profiles/scan_split_kernels.log); `canon` maps the parent's spelling of an instantiation to the new one: the template argument
order of scan_coarse256_kernel, the attention kernels on a head-width policy (profiles/attention_shell_kernels.log).

    python -m semcode_amd.csrc.build --force --save-temps 2> BUILD.log     (in a checkout of each commit; keep csrc/_obj/*gfx950.s)
    python scripts/kernel_compare.py PARENT_S_DIR PARENT_BUILD.log NEW_S_DIR NEW_BUILD.log [STEM,STEM...]

With a list of stems (e.g. gemm_bf16,encoder_ops: profiles/encoder_split_kernels.log) the same files are compared in both builds; a stem
one build lacks (a file removed or added) contributes that build's kernels only.
"""
import hashlib
import re
import subprocess
import sys
from pathlib import Path

CXXFILT = "c++filt"


def remarks(log):
    out, cur = {}, None
    for line in Path(log).read_text().splitlines():
        m = re.match(r"remark: (\S+?):\d+:0: +(.*?) \[-Rpass", line)
        if not m:
            continue
        src, body = m.groups()
        if body.startswith("Function Name: "):
            cur = body[len("Function Name: "):]
            out[cur] = {"src": src}
        elif cur and ": " in body:
            k, v = body.rsplit(": ", 1)
            out[cur][k.strip()] = v
    return out


def bodies(sdir, stems):
    out = {}
    for s in sorted(Path(sdir).glob("*gfx950.s")):
        if not any(s.name.startswith(st + "-hip-") for st in stems):
            continue
        name, lines = None, []
        for line in s.read_text().splitlines():
            m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
            if m and not line.startswith(".") and not line.startswith("\t"):
                name, lines = m.group(1), []
                continue
            if name is None:
                continue
            st = line.strip()
            if st.startswith(".Lfunc_end"):
                out[name] = lines
                name = None
                continue
            if not st or st.startswith(";") or st.startswith("."):
                if re.match(r"^\.LBB\d+_\d+:", st):
                    lines.append(re.sub(r"\.LBB\d+_", ".LBB_", st.split(":")[0] + ":"))
                continue
            st = re.sub(r"\s*;.*$", "", st)
            st = re.sub(r"\.LBB\d+_", ".LBB_", st)
            lines.append(st)
    return out


def demangle(names):
    r = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def canon(d):
    """parent -> new spelling of an instantiation (scan_coarse256_kernel<METRIC, DBG, I8, PP, DENSE>, the attention kernels); None =
    instantiation removed on purpose"""
    d = re.sub(r"\(.*$", "", d).replace("void ", "")
    m = re.match(r"scan_coarse256_kernel<(\d+), (\d+), (true|false), (\d+), (true|false)>", d)
    if m:
        metric, dbg, i8, pp, dense = m.groups()
        if dbg not in ("0", "2"):
            return None
        return f"scan_coarse256_kernel<{metric}, {i8}, {pp}, {dense}, {'true' if dbg == '2' else 'false'}>"
    # attention kernels on a head-width policy (profiles/attention_shell_kernels.log): <KT, ALIBI, NW> -> <Head64<ALIBI>, KT, NW>,
    # attention32_* -> <Head32, ...>; the 4-wave instantiations at KT 8 and 16 went with the experiment switch that chose them
    m = re.match(r"attention_kernel<(\d+), (true|false), (\d+)>", d)
    if m:
        kt, alibi, nw = m.groups()
        return None if (int(kt) >= 8 and nw == "4") else f"attention_kernel<Head64<{alibi}>, {kt}, {nw}>"
    d = re.sub(r"^attention_long_kernel<(true|false)>", r"attention_long_kernel<Head64<\1>>", d)
    d = re.sub(r"^attention_packed_kernel<(\d+), (\d+), (true|false)>", r"attention_packed_kernel<Head64<\3>, \1, \2>", d)
    d = re.sub(r"^attention32_long_kernel$", "attention_long_kernel<Head32>", d)
    d = re.sub(r"^attention32_(packed_)?kernel<", r"attention_\1kernel<Head32, ", d)
    # causal attention on the head width (profiles/causal_width_kernels.log): <NB, KTS, NW[, LONG]>, NB 64-column blocks a head
    d = re.sub(r"^attention_causal_kernel<(\d+), (\d+)>", r"attention_causal_kernel<1, \1, \2>", d)
    d = re.sub(r"^attention_causal128_kernel<(\d+), (\d+)>", r"attention_causal_kernel<2, \1, \2>", d)
    m = re.match(r"attention_causal_packed_kernel<(\d+), (\d+)>", d)
    if m:
        d = f"attention_causal_packed_kernel<1, {m.group(1)}, {m.group(2)}, {'true' if m.group(1) == '16' else 'false'}>"
    d = re.sub(r"^attention_causal128_packed_kernel<(\d+), (\d+), (true|false)>", r"attention_causal_packed_kernel<2, \1, \2, \3>", d)
    return d.replace("> >", ">>")


def main(pdir, plog, ndir, nlog, stems=None):
    new_stems = stems.split(",") if stems else ["scan_shadow", "scan_coarse", "scan_coarse64", "scan_select", "scan_rerank", "scan_exact"]
    old_stems = new_stems if stems else ["scan_batched", "scan_exact"]
    pr, nr = remarks(plog), remarks(nlog)
    pb, nb = bodies(pdir, old_stems), bodies(ndir, new_stems)
    pr = {k: v for k, v in pr.items() if v["src"].split(".")[0] in old_stems}
    nr = {k: v for k, v in nr.items() if v["src"].split(".")[0] in new_stems}
    dm = demangle(list(pr) + list(nr))
    pk = {}
    removed = []
    for k in pr:
        c = canon(dm[k])
        if c is None:
            removed.append(dm[k].split("(")[0])
        else:
            pk[c] = k
    nk = {re.sub(r"\(.*$", "", dm[k]).replace("void ", "").replace("> >", ">>"): k for k in nr}
    keys = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    print("# kernel | file | VGPR AGPR scratch LDS occupancy (parent -> new when they differ) | instructions parent -> new | text")
    bad = 0
    for c in sorted(set(pk) | set(nk)):
        if c not in nk:
            print(f"{c} | MISSING in the new build"); bad += 1; continue
        if c not in pk:
            print(f"{c} | {nr[nk[c]]['src']} | new instantiation | {len(nb[nk[c]])} instructions"); continue
        a, b = pr[pk[c]], nr[nk[c]]
        res = " ".join(a[k] if a[k] == b[k] else f"{a[k]}->{b[k]}" for k in keys)
        la, lb = pb[pk[c]], nb[nk[c]]
        ia = sum(1 for l in la if not l.endswith(":")); ib = sum(1 for l in lb if not l.endswith(":"))
        same = hashlib.sha1("\n".join(la).encode()).digest() == hashlib.sha1("\n".join(lb).encode()).digest()
        flag = "identical" if same else ("differs" if ib <= ia else f"differs, GREW +{ib - ia}")
        if any(a[k] != b[k] for k in keys) or ib > ia:
            bad += 1
        print(f"{c} | {b['src']} | {res} | {ia} -> {ib} | {flag}")
    for r in sorted(removed):
        print(f"{r} | removed (experiment instantiation)")
    print(f"# kernels whose resources changed or whose instruction count grew: {bad}")


if __name__ == "__main__":
    main(*sys.argv[1:6])
