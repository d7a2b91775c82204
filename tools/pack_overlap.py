#!/usr/bin/env python3
"""What pack_k costs inside a step, from a tools/rocpd_lanes.py timeline: every pack_k launch, their sum, and for each conv
kernel that runs next to one for at least half of its own duration, that duration against the other launches of the same
instantiation with the same grid that do not touch a pack_k.   usage: pack_overlap.py lanes.txt [out.txt]"""
import re
import sys


def main(path, out):
    rows = []
    for line in open(path).read().splitlines()[2:]:
        m = re.match(r"\s*([\d.]+)\s+([\d.]+) q(\d+)\s+x(\d+) (\S+)\s+wg (\d+)", line)
        if m:
            rows.append((float(m.group(1)), float(m.group(2)), int(m.group(3)), m.group(5), int(m.group(6))))
    packs = [r for r in rows if r[3].startswith("pack_k")]

    def shared(r):
        return sum(max(0.0, min(r[0] + r[1], p[0] + p[1]) - max(r[0], p[0])) for p in packs)
    w = out.write
    w("pack_k: %d launches, %.1f us per step\n" % (len(packs), sum(p[1] for p in packs)))
    for p in packs:
        w("  start %9.1f  %7.1f us  q%d  %5d workgroups\n" % (p[0], p[1], p[2], p[4]))
    w("conv launches at least half inside a pack_k launch, against the same instantiation and grid clear of pack_k:\n")
    for r in rows:
        if r[3].startswith("conv_") and shared(r) >= 0.5 * r[1]:
            alone = sorted(x[1] for x in rows if x[3] == r[3] and x[4] == r[4] and shared(x) == 0.0)
            w("  start %9.1f  %7.1f us  q%d  %-44s wg %5d   clear of pack_k: %s\n" % (
                r[0], r[1], r[2], r[3], r[4],
                ("%d launches, %.1f - %.1f us, median %.1f" % (len(alone), alone[0], alone[-1], alone[len(alone) // 2]))
                if alone else "none in this step"))


if __name__ == "__main__":
    f = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
    main(sys.argv[1], f)
