"""The per-dispatch sequence (kernel name, grid size, workgroup size) of a rocprofv3 --kernel-trace csv, in dispatch order, and the comparison
of two such sequences: a host-side refactor must leave it unchanged.
  python scripts/dispatch_sequence.py dump <run_kernel_trace.csv> <out.tsv>
  python scripts/dispatch_sequence.py compare <a.tsv> <b.tsv>        (exit status 1 when they differ)"""
import collections
import csv
import re
import sys


def load(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, p: "x".join(r[f"{p}_{a}"] for a in "XYZ") if f"{p}_X" in r else r[p]
    return [(re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]), dims(r, "Grid_Size"), dims(r, "Workgroup_Size")) for r in rows]


def main():
    if sys.argv[1] == "dump":
        with open(sys.argv[3], "w") as f:
            for d in load(sys.argv[2]):
                f.write("\t".join(d) + "\n")
        return 0
    a, b = ([tuple(l.rstrip("\n").split("\t")) for l in open(p)] for p in sys.argv[2:4])
    ours = lambda s: [d for d in s if "wseg" in d[0] or "conv_" in d[0]]
    same_all, same_conv = a == b, ours(a) == ours(b)
    print(f"dispatches: {len(a)} vs {len(b)}; whole sequence equal: {same_all}; conv / wgrad sequence equal ({len(ours(a))} launches): {same_conv}")
    if not same_all:
        n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"first difference at dispatch {n}:\n  {a[n] if n < len(a) else None}\n  {b[n] if n < len(b) else None}")
        ca, cb = collections.Counter(a), collections.Counter(b)
        for k in sorted(set(ca) | set(cb)):
            if ca[k] != cb[k]:
                print(f"  {ca[k]:6d} vs {cb[k]:6d}  {k}")
    print("kernels (launches, distinct grids):")
    agg = collections.defaultdict(lambda: [0, set()])
    for name, grid, wg in ours(a):
        agg[name][0] += 1
        agg[name][1].add(grid)
    for name, (n, grids) in sorted(agg.items()):
        print(f"  {n:6d} {len(grids):4d}  {name[:150]}")
    return 0 if same_all else 1


if __name__ == "__main__":
    sys.exit(main())
