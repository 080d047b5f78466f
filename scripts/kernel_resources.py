"""Resource usage of the kernels of csrc/*.hip sources, from the compiler's own report: no GPU needed.

    python scripts/kernel_resources.py [--csrc DIR] [--filter SUBSTR] rollout.hip eval.hip act.hip

Each source is compiled for the device only with the build's flags (ops/_build.py device_flags) plus
``-Rpass-analysis=kernel-resource-usage``; the code size of a kernel is its symbol's size in the code object.
Prints one markdown row per kernel: VGPRs, AGPRs, SGPRs, spilled SGPRs / VGPRs, scratch bytes per lane, static LDS
bytes, occupancy (waves per SIMD) and code bytes.  ``--csrc`` compiles another tree's sources (e.g. the parent
commit's, checked out elsewhere) for a before / after table (profiles/categorical_fused/README.md).
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_dppo_amd.ops import _build   # noqa: E402

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("SGPRs Spill", "SGPR spill"),
          ("VGPRs Spill", "VGPR spill"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
          ("Occupancy [waves/SIMD]", "occ")]


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if tool is None:   # (the mangled names then)
        return list(names)
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return [re.sub(r"^void \(anonymous namespace\)::|\(.*\)$", "", x) for x in r.stdout.splitlines()]


def kernels_of(src: str, csrc: str):
    """[(demangled name, {column: int})] of one source, in the report's order"""
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "k.o")
        cmd = [_build.HIPCC] + _build.device_flags() + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only",
                                                         "--no-gpu-bundle-output", "-c", os.path.join(csrc, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-4000:])
        readelf = os.path.join(os.path.dirname(_build.HIPCC), "..", "llvm", "bin", "llvm-readelf")
        syms = subprocess.run([readelf, "--symbols", "--wide", obj], capture_output=True, text=True, check=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    out, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = {"code": size.get(v, -1)}
            out.append((v, cur))
        elif cur is not None:
            for field, col in FIELDS:
                if k == field:
                    cur[col] = int(v)
    names = demangle([n for n, _ in out])
    return [(n, d) for n, (_, d) in zip(names, out)]


def main(argv):
    csrc, filt, srcs = _build.CSRC, "", []
    it = iter(argv)
    for a in it:
        if a == "--csrc":
            csrc = next(it)
        elif a == "--filter":
            filt = next(it)
        else:
            srcs.append(a)
    cols = [c for _, c in FIELDS] + ["code"]
    print("| kernel | " + " | ".join(cols) + " |")
    print("|---|" + "---:|" * len(cols))
    for src in srcs:
        for name, d in kernels_of(src, csrc):
            if filt in name:
                print(f"| `{name}` | " + " | ".join(str(d.get(c, "")) for c in cols) + " |")


if __name__ == "__main__":
    main(sys.argv[1:])
