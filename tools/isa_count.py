#!/usr/bin/env python3
"""Instruction counts along one path through a kernel's assembly listing.

  hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/rp_kernel.hip -o kernel.s
  tools/isa_count.py kernel.s 74801:74836 74838:74883 ...

The ranges are 1-based, inclusive line ranges of the listing: the basic blocks one wave execution runs through, picked
by reading the listing (a path, not a region: blocks the path skips are left out).  Prints one JSON object: VALU
(v_*), of them register moves (v_mov_*), SALU (s_* but loads, waits, nops and branches), branches, vector-memory loads,
scalar loads, waits (s_waitcnt) and nops.
"""
import json
import sys


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith(("global_load", "flat_load", "buffer_load", "scratch_load")):
        return "vmem_load"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem_other"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem_load"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    lines = open(sys.argv[1]).read().split("\n")
    out = {k: 0 for k in ("valu", "valu_mov", "salu", "branch", "vmem_load", "vmem_other", "lds", "smem_load", "wait",
                          "nop", "other")}
    for rng in sys.argv[2:]:
        a, b = (int(x) for x in rng.split(":"))
        for ln in lines[a - 1:b]:
            t = ln.strip()
            if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
                continue
            op = t.split()[0]
            k = classify(op)
            out[k] += 1
            if op.startswith("v_mov_"):
                out["valu_mov"] += 1
    out["ranges"] = sys.argv[2:]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
