#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly listings of one translation unit (hipcc --offload-arch=gfx950 --cuda-device-only -S):
which kernels are the same instruction for instruction, which are the same instructions in another order or with other register numbers
(`reordered`: the same multiset of mnemonics and the same resource figures), which differ, which exist on one side only.  No GPU needed.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/vstab_corners.hip -o branch.s     (and parent.s)
    cat branch_corners.s branch_corners_fused.s > branch.s                                    (a unit the branch split in two)
    python tools/asm_kernel_diff.py parent.s branch.s

A kernel's text is what stands between its label and its .Lfunc_end; basic-block labels are renumbered per function (adding a kernel to
the unit shifts the function index inside every .LBB<function>_<block>), comments and blank lines are dropped.  The resource figures
(VGPRs, SGPRs, LDS, private segment) come from the .amdhsa metadata of each listing.  Exit status 1 if a kernel present in both is DIFFERENT."""
import collections
import re
import sys


def mnemonics(body):
    """the multiset of instruction mnemonics of a kernel's text: labels and directives left out"""
    return collections.Counter(line.split()[0] for line in body if not line.rstrip().endswith(":") and not line.lstrip().startswith("."))


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = []
        for line in m.group(2).splitlines():
            line = line.split(";")[0].rstrip()
            if not line.strip():
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        out[m.group(1)] = body
    res = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\w+).*?\.private_segment_fixed_size:\s*(\d+).*?\.sgpr_count:\s*(\d+).*?"
                         r"\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)", text, re.S):
        res[m.group(2)] = dict(lds=int(m.group(1)), private=int(m.group(3)), sgpr=int(m.group(4)), vgpr=int(m.group(5)), spill=int(m.group(6)))
    return out, res


def main():
    (a, ra), (b, rb) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        r = rb.get(name) or ra.get(name)
        fig = "vgpr %(vgpr)d sgpr %(sgpr)d lds %(lds)d private %(private)d spills %(spill)d" % r if r else ""
        if name not in a:
            print(f"new        {name}: {len(b[name])} lines; {fig}")
        elif name not in b:
            print(f"gone       {name}")
        elif a[name] == b[name] and ra.get(name) == rb.get(name):
            print(f"identical  {name}: {len(a[name])} lines; {fig}")
        elif mnemonics(a[name]) == mnemonics(b[name]) and ra.get(name) == rb.get(name):
            n = sum(x != y for x, y in zip(a[name], b[name])) + abs(len(a[name]) - len(b[name]))
            print(f"reordered  {name}: {len(a[name])} lines, {n} of them differ in place (order or register numbers only); {fig}")
        else:
            bad += 1
            print(f"DIFFERENT  {name}: {len(a[name])} -> {len(b[name])} lines; {ra.get(name)} -> {rb.get(name)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
