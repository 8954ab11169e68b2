"""Pair-mode sampling in a kernel trace of scripts/sample_only.py (rocprofv3 --kernel-trace --output-format csv):
  python scripts/pair_trace.py <parent kernel_trace.csv> <new kernel_trace.csv (sample_only.py pair)> [out.json]
Per tree what scripts/lanes_trace.py gives (mean us per kernel and grid size, the step from head end to head end), the
hardware queues the kernels ran on, and the share of steps in which a pass that is no big GEMM (BatchNorm finalize /
apply, the head, the running-statistics update) runs inside a big GEMM -- which, on one tree, can only be another call's.
Then how much each of the three big GEMMs lengthens from parent to new."""
import csv
import json
import sys

from lanes_trace import GEMM, HEAD, load, summary

PASSES = ("bn_finalize_kernel", "bn_apply_kernel", HEAD, "bn_running_kernel")


def queues(path):
    out = {}
    for r in csv.DictReader(open(path)):
        q = r.get("Queue_Id")
        if q is not None:
            name = r["Kernel_Name"].split("(")[0]
            out.setdefault(name, {}).setdefault(q, 0)
            out[name][q] += 1
    return out


def inside(rows):
    """Share of steps (head launches, the first 10 % dropped) with a non-GEMM pass that overlaps a big GEMM in time."""
    g0 = min(g for _, _, name, g in rows if GEMM in name)
    big = [(s, e) for s, e, name, g in rows if GEMM in name and g != g0]
    heads = [e for _, e, name, _ in rows if HEAD in name]
    skip = len(heads) // 10
    hit, j = 0, 0
    passes = [(s, e) for s, e, name, _ in rows if any(p in name for p in PASSES)]
    for k in range(skip + 1, len(heads)):
        lo, hi = heads[k - 1], heads[k]
        step_passes = [(s, e) for s, e in passes if lo < e <= hi]
        step_big = [(s, e) for s, e in big if e > lo and s < hi]
        hit += any(ps < be and bs < pe for ps, pe in step_passes for bs, be in step_big)
    return round(hit / max(1, len(heads) - skip - 1), 3)


def main():
    out = {}
    for tree, path in (("parent", sys.argv[1]), ("new", sys.argv[2])):
        rows = load(path)
        out[tree] = summary(rows)
        out[tree]["steps_with_a_pass_inside_a_big_gemm"] = inside(rows)
        out[tree]["queues"] = queues(path)
    big = sorted((k for k in out["parent"]["kernels"] if GEMM in k), key=lambda k: -out["parent"]["kernels"][k]["us"])[:3]
    out["big_gemms_lengthen_us"] = {k: round(out["new"]["kernels"][k]["us"] - out["parent"]["kernels"][k]["us"], 2)
                                    for k in big if k in out["new"]["kernels"]}
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
