#!/usr/bin/env python3
"""Per-kernel register / spill / occupancy summary of one HIP source (hipcc -Rpass-analysis=
kernel-resource-usage, device pass only), demangled names shortened: the quick check for spills after a
kernel edit.  tests/test_cpu_host.py holds the Fcomb kernels to their spill counts through table().
usage: tools/regs.py csrc/<file>.hip [name-substring]"""
import re
import subprocess
import sys

HIPCC = "/opt/rocm/bin/hipcc"


def table(src):
    """{demangled kernel name: {"VGPRs": n, "AGPRs": n, "VGPRs Spill": n, "Occupancy [waves/SIMD]": n, ...}}"""
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wno-unused-function", "-munsafe-fp-atomics",
           "--cuda-device-only", "-c", src, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    if any(k in src for k in ("wino",)):
        cmd[1:1] = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    cur = None
    rows = {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark: +([A-Za-z /\[\]]+?): (\d+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.splitlines()
    return {dn.replace("(anonymous namespace)::", ""): v for v, dn in zip(rows.values(), names)}


if __name__ == "__main__":
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    for dn, v in table(sys.argv[1]).items():
        if flt and flt not in dn:
            continue
        print(f"{dn[:90]:90s} vgpr {v.get('VGPRs', '?'):>3} agpr {v.get('AGPRs', '?'):>3} "
              f"spill {v.get('VGPRs Spill', '?')} occ {v.get('Occupancy [waves/SIMD]', '?')} lds {v.get('LDS Size [bytes/block]', '?')}")
