#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy / code-size table of a HIP source, from a device-only compile with the
Makefile's flags (hipcc -Rpass-analysis=kernel-resource-usage for the resources, the code object's symbol table for
the code size), e.g.  python3 tools/kres.py realtimeraytracing_gradproject_amd/csrc/rt_trace.hip [-DX=1]
rt_trace.hip gets the Makefile's TRACEFLAGS as well, so the table is the product's. --mangled prints the mangled
names (one table row per code-object symbol, for diffing two commits), --all the non-kernel functions too."""
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM", "/opt/rocm")
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics"]
TRACEFLAGS = ["-fno-slp-vectorize", "-mllvm", "-structurizecfg-skip-uniform-regions=1"]  # Makefile: rt_trace.o only

src = sys.argv[1]
opts = [a for a in sys.argv[2:] if a in ("--all", "--mangled")]
extra = [a for a in sys.argv[2:] if a not in opts]
flags = HIPFLAGS + (TRACEFLAGS if os.path.basename(src) == "rt_trace.hip" else [])
with tempfile.TemporaryDirectory() as tmp:
    co = os.path.join(tmp, "kres.co")
    cmd = [f"{ROCM}/bin/hipcc"] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", co,
                                           "-Rpass-analysis=kernel-resource-usage"] + extra
    run = subprocess.run(cmd, capture_output=True, text=True)
    if run.returncode != 0:
        sys.exit(run.stderr)
    syms = subprocess.run([f"{ROCM}/llvm/bin/llvm-readelf", "-sW", co], capture_output=True, text=True, check=True).stdout
size = {}
for ln in syms.splitlines():
    f = ln.split()
    if len(f) == 8 and f[3] == "FUNC":
        size[f[7]] = f[2]
rows, cur = [], None
for ln in run.stderr.splitlines():
    m = re.search(r"remark: (.*?) \[-Rpass", ln)
    if not m:
        continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        name = t.split(":", 1)[1].strip()
        dm = name
        if "--mangled" not in opts:
            dm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            dm = re.sub(r"rt::\(anonymous namespace\)::", "", dm)
            dm = dm.split("(")[0][:60]
        cur = {"name": dm, "Code [bytes]": size.get(name, "-")}
        rows.append(cur)
    elif cur is not None and ":" in t:
        k, v = t.split(":", 1)
        cur[k.strip()] = v.strip()
keys = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]", "Code [bytes]"]
heads = ["VGPRs", "AGPRs", "SGPRs", "Scratch", "Occup", "SSpill", "VSpill", "LDS", "Code"]
w = max([60] + [len(r["name"]) for r in rows])
print(f"{'kernel':{w}s} " + " ".join(f"{h:>8s}" for h in heads))
for r in rows:
    if "--all" not in opts and "k_" not in r["name"]:
        continue
    print(f"{r['name']:{w}s} " + " ".join(f"{r.get(k, '-'):>8s}" for k in keys))
