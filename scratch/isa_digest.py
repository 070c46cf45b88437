#!/usr/bin/env python3
"""Per-kernel digest of a device assembly file (`hipcc ... --cuda-device-only -S`).

    python scratch/isa_digest.py gemm.s

One line per kernel symbol: symbol, instruction count, sha256 (first 16 hex digits) of its instruction stream, VGPRs, SGPRs,
accum_offset, scratch bytes, LDS bytes, and a digest of all its `.amdhsa_*` lines.  The stream is the function's body with
comments stripped and the function ordinal taken out of local labels (`.LBB<n>_<m>` -> `.LBB_<m>`: the ordinal moves when
definitions move).  Two builds compute the same kernels exactly when their outputs are equal (`diff`).
"""
import hashlib
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main(path):
    body, hsa, cur = {}, {}, None
    for raw in open(path):
        line = re.sub(r"\.LBB\d+_", ".LBB_", raw.split(";")[0]).strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = hsa.setdefault(m.group(1), [])
        elif line == ".end_amdhsa_kernel" or line.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"[A-Za-z_][\w$.]*:$", line):          # a function's entry label
            cur = body.setdefault(line[:-1], [])
        elif cur is not None and line and (not line.startswith(".") or line.startswith((".LBB", ".amdhsa_"))):
            cur.append(" ".join(line.split()))
    for sym in sorted(hsa):
        res = dict(l[len(".amdhsa_"):].split() for l in hsa[sym])
        count = sum(1 for l in body[sym] if not l.endswith(":"))
        print(sym, count, digest(body[sym]), *(f"{k}={res[k]}" for k in RES), "hsa=" + digest(hsa[sym]))


if __name__ == "__main__":
    main(sys.argv[1])
