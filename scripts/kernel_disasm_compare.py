"""Every kernel of two builds of libsemcode_hip.so, disassembled and compared: one line per kernel with its instruction count in each
build and whether the instruction text is identical.  Needs no GPU and no -save-temps build: the gfx950 code objects are taken out
of the libraries themselves.

    python scripts/kernel_disasm_compare.py PARENT_LIB.so NEW_LIB.so > profiles/NAME_kernels.log

How: `llvm-objdump --offloading` unbundles the code object of every translation unit, `llvm-objdump -d` disassembles it; per function
symbol the instruction text is kept without addresses, encodings and the address comments behind branch targets (a branch's own
operand is a relative offset and stays).  Kernels are named by their demangled symbol, so a kernel that moved to another file is still
the same kernel.  (scripts/kernel_compare.py compares the compiler's assembly and resource remarks of -save-temps builds instead.)
"""
import hashlib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")


def tool(name):
    exe = shutil.which(name) or str(LLVM / name)
    if not Path(exe).exists():
        raise SystemExit(f"{name} not found")
    return exe


def kernels(lib):
    """demangled kernel name -> list of instruction lines"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = Path(tmp) / "lib.so"
        shutil.copy(lib, copy)
        subprocess.run([tool("llvm-objdump"), "--offloading", str(copy)], cwd=tmp, check=True, capture_output=True)
        for co in sorted(Path(tmp).glob("lib.so.*gfx950*")):
            text = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True, text=True).stdout
            name, lines = None, []
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    if name is not None:
                        out[name] = lines
                    name, lines = m.group(1), []
                    continue
                if name is None or not line.startswith("\t") and not line.startswith(" "):
                    continue
                ins = re.sub(r"\s*//.*$", "", line).strip()
                if ins and ins != "...":  # "...": zero padding objdump skips behind a function, no instruction
                    lines.append(re.sub(r"\s+", " ", ins))
            if name is not None:
                out[name] = lines
    names = list(out)
    dm = subprocess.run([tool("c++filt") if shutil.which("c++filt") else tool("llvm-cxxfilt")], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    res = {}
    for n, d in zip(names, dm):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\((?:[^()]|\([^()]*\))*\)(?: \[clone .*\])?$", "", d) if d != n else d
        res[d if d not in res else d + " #" + n] = out[n]
    return res


def main(parent, new):
    a, b = kernels(parent), kernels(new)
    print("# scripts/kernel_disasm_compare.py: llvm-objdump -d of the gfx950 code objects inside the two libraries: parent commit -> this change")
    print("# kernel | instructions parent -> new | text")
    differs = missing = 0
    for k in sorted(set(a) | set(b)):
        if k not in b:
            print(f"{k} | {len(a[k])} -> MISSING in the new build")
            missing += 1
        elif k not in a:
            print(f"{k} | new kernel | {len(b[k])} instructions")
        else:
            same = hashlib.sha1("\n".join(a[k]).encode()).digest() == hashlib.sha1("\n".join(b[k]).encode()).digest()
            differs += not same
            print(f"{k} | {len(a[k])} -> {len(b[k])} | {'identical' if same else 'DIFFERS'}")
    print(f"# kernels of the parent build: {len(a)}; identical in the new build: {len(set(a) & set(b)) - differs}; differing: {differs}; missing: {missing}; "
          f"new: {len(set(b) - set(a))}")
    return 1 if differs or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
