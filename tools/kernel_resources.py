#!/usr/bin/env python3
"""Reduce hipcc's -Rpass-analysis=kernel-resource-usage remarks to one line per kernel:
  demangled name | SGPRs | VGPRs | scratch bytes/lane | SGPR spills | VGPR spills | waves/SIMD | LDS bytes
usage: hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c csrc/ntt.hip -o /dev/null 2> remarks
       tools/kernel_resources.py remarks > table      (sorted by name, so two tables diff line by line)
"""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill",
          "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def reduce(path):
    kernels, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = kernels.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    names = list(kernels)
    plain = subprocess.run(["c++filt", "-p"], input="\n".join(names),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    rows = []
    for mangled, name in zip(names, plain):
        name = name.replace("fhe::(anonymous namespace)::", "")
        rows.append(" | ".join([name] + [kernels[mangled][f] for f in FIELDS]))
    return sorted(rows)


if __name__ == "__main__":
    print("\n".join(reduce(sys.argv[1])))
