#!/usr/bin/env python3
"""Static figures of every cone_kernel instance from an assembly listing of
riptide_amd/csrc/ffa_kernels.hip (the Makefile's HIPFLAGS with
`-S --cuda-device-only -o listing.s`): registers, spills and scratch from the
kernel descriptors' metadata, code size, and counts of VALU instructions,
lane reads / writes (the SGPR-spill traffic) and s_nop in the body.

usage: python tools/cone_static.py listing.s [out.json]
With --spills INSTANCE (e.g. "4,0,2": SMAX,WIDE,SNR) prints, for that
instance, every basic block of the listing that holds lane reads / writes,
with their counts and the block's instruction count.
"""
import json
import re
import sys


def instance(sym):
    """Template arguments of a mangled cone_kernel instance: 'SMAX,WIDE,SNR'
    (integral arguments only: L<type><value>E)."""
    return ",".join(re.findall(r"L[a-z](\d+)E", sym.split("cone_kernel", 1)[1]))


def parse(path):
    text = open(path, errors="replace").read()
    # bodies: "sym:" ... ".Lfunc_endN:"
    bodies = {}
    for m in re.finditer(r"^(_ZN2rt11cone_kernel\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        bodies[m.group(1)] = m.group(2)
    meta = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target|\Z)", text, re.S | re.M):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if name not in bodies:
            continue
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        meta[name] = {"vgprs": g("vgpr_count"), "sgprs": g("sgpr_count"), "sgpr_spill_count": g("sgpr_spill_count"),
                      "vgpr_spill_count": g("vgpr_spill_count"), "scratch_bytes": g("private_segment_fixed_size"),
                      "lds_bytes": g("group_segment_fixed_size")}
    rows = []
    for name in sorted(bodies, key=lambda n: [int(x) for x in instance(n).split(",")]):
        body = bodies[name]
        ins = [l.split(";")[0].strip() for l in body.split("\n")]
        ins = [l for l in ins if l and not l.startswith((".", ";")) and not l.endswith(":")]
        size = re.search(r"^%s:[^\n]*\n.*?; codeLenInByte = (\d+)" % re.escape(name), text, re.S | re.M)
        rows.append({"instance": instance(name), **meta.get(name, {}),
                     "code_bytes": int(size.group(1)) if size else None,
                     "valu": sum(1 for l in ins if l.startswith("v_")),
                     "v_readlane": sum(1 for l in ins if l.startswith("v_readlane")),
                     "v_writelane": sum(1 for l in ins if l.startswith("v_writelane")),
                     "s_nop": sum(1 for l in ins if l.startswith("s_nop")), "symbol": name})
    return rows, bodies


def lane_blocks(body):
    """(label, lane reads, lane writes, instructions) of every basic block of a body."""
    out, label, r, w, n = [], "entry", 0, 0, 0
    for line in body.split("\n"):
        l = line.split(";")[0].strip()
        if not l or l.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", l):
                out.append((label, r, w, n))
                label, r, w, n = l[:-1], 0, 0, 0
            continue
        n += 1
        r += l.startswith("v_readlane")
        w += l.startswith("v_writelane")
    out.append((label, r, w, n))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows, bodies = parse(args[0])
    if "--spills" in sys.argv:
        want = sys.argv[sys.argv.index("--spills") + 1]
        for r in rows:
            if r["instance"].startswith(want):
                for label, rd, wr, n in lane_blocks(bodies[r["symbol"]]):
                    if rd or wr:
                        print(f"{label:14s} insts {n:5d} v_readlane {rd:4d} v_writelane {wr:4d}")
        return
    hdr = ("instance", "vgprs", "sgprs", "sgpr_spill_count", "vgpr_spill_count", "scratch_bytes", "code_bytes", "valu",
           "v_readlane", "v_writelane", "s_nop")
    print(" ".join(f"{h:>16s}" for h in hdr))
    for r in rows:
        print(" ".join(f"{str(r.get(h)):>16s}" for h in hdr))
    if len(args) > 1:
        json.dump([{k: v for k, v in r.items() if k != "symbol"} for r in rows], open(args[1], "w"), indent=1)


if __name__ == "__main__":
    main()
