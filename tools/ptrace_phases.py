#!/usr/bin/env python3
"""Per-phase time of training runs from GBPE_DEBUG=ptrace=1 lines (tools/ab_libs.py
with AB_STDERR=1): merges, host wall ms and us/merge per k_body form.

The multi-tile steps (zone1 0) and the segment steps of zones above 1M symbols are split
by the zone's length at the step's start (the line's `zone0`): <= 1M, 1M-2M, 2M-4M,
above.  A library from before `zone0` was printed takes it from the lines of
another library in the same files that start at the same merge (the zone's
length at a merge does not depend on the form that runs it)."""
import re
import sys

M = 1 << 20
BUCKETS = ((M, "<=1M"), (2 * M, "1M-2M"), (4 * M, "2M-4M"), (1 << 62, ">4M"))


def bucket(z):
    return next(i for i, (hi, _) in enumerate(BUCKETS) if z <= hi)


for path in sys.argv[1:]:
    runs, cur, lib = [], [], None
    z0 = {}   # zone0 by (merge, done, mc, zone at the end): the same step of the same corpus in any library
    for line in open(path):
        if "[ptrace]" not in line:
            continue
        head, _, tail = line.partition("[ptrace]")
        d = {k: float(v) for k, v in re.findall(r"(\w+) ([\d.]+)", tail)}
        if cur and (d["merge"] < cur[-1]["merge"] or head != lib):
            runs.append((lib, cur))
            cur = []
        lib = head
        cur.append(d)
        if "zone0" in d:
            z0[(d["merge"], d["done"], d["mc"], d["zone"])] = d["zone0"]
    if cur:
        runs.append((lib, cur))
    for lib, run in runs:
        print("%s total %.1f ms, %d merges" % (lib.strip(), sum(r["us"] for r in run) / 1e3, sum(r["done"] for r in run)))
        ph = {}
        for r in run:
            zs = r.get("zone0", z0.get((r["merge"], r["done"], r["mc"], r["zone"])))
            z1 = int(r["zone1"])
            split = zs is not None and (z1 == 0 or zs > M)
            key = (min(z1, 3), int(r["bt"]), bucket(zs) if split else -1)
            p = ph.setdefault(key, [0.0, 0, 0, 1e18, 0])
            p[0] += r["us"]
            p[1] += r["done"]
            p[2] += r["paired"]
            p[3] = min(p[3], r["merge"])
            p[4] = max(p[4], r["merge"] + r["done"])
        for k, p in sorted(ph.items(), key=lambda kv: kv[1][3]):
            print("  zone1 %d bt %4d%s: merges %6d-%6d %7.1f ms %7.2f us/merge, paired %d" %
                  (k[0], k[1], " zone " + BUCKETS[k[2]][1] if k[2] >= 0 else "", p[3], p[4], p[0] / 1e3,
                   p[0] / max(p[1], 1), p[2]))
