"""Two-lane sampling in a kernel trace of scripts/sample_only.py (rocprofv3 --kernel-trace --output-format csv):
  python scripts/lanes_trace.py <parent kernel_trace.csv> <new kernel_trace.csv> [out.json]
Per tree: mean us per kernel and grid size after dropping each kernel's first 10 % (as profiles/border_order_trace.json),
the mean step (head end to head end), and the share of steps in which the next call's latent solve / layer-0 GEMM begin
before this call's head ends.  Then how much each of the three big GEMMs lengthens from parent to new."""
import csv
import json
import sys

SOLVE, HEAD, GEMM = "ode_fwd_valu_kernel", "conv_pointwise1_kernel", "igemm_fast_kernel"


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        grid = int(r.get("Grid_Size") or int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"]))
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0], grid))
    rows.sort()
    return rows


def summary(rows):
    by = {}
    for s, e, name, grid in rows:
        by.setdefault(f"{name} grid {grid}", []).append((e - s) / 1e3)
    steps = sum(HEAD in name for _, _, name, _ in rows)
    kernels = {}
    for k, v in by.items():
        kept = v[len(v) // 10:]
        kernels[k] = {"launches": len(kept), "us": round(sum(kept) / len(kept), 2), "per_step": round(len(v) / steps, 2)}
    heads = [(s, e) for s, e, name, _ in rows if HEAD in name]
    solves = [s for s, _, name, _ in rows if SOLVE in name]
    gemm0_grid = min(g for _, _, name, g in rows if GEMM in name)
    gemm0 = [s for s, _, name, g in rows if GEMM in name and g == gemm0_grid]
    skip = len(heads) // 10
    span = (heads[-1][1] - heads[skip][1]) / 1e3 / (len(heads) - 1 - skip)
    # call k + 1's front against call k's head: the j-th solve / layer-0 GEMM belongs to the j-th call
    n = min(len(heads), len(solves), len(gemm0)) - 1
    ks = range(skip, n)
    under = lambda starts: round(sum(starts[k + 1] < heads[k][1] for k in ks) / len(ks), 3)      # noqa: E731
    return {"kernels": kernels, "step_us": round(span, 2), "steps": len(ks), "solve_begins_before_head_ends": under(solves),
            "gemm0_begins_before_head_ends": under(gemm0)}


def main():
    out = {"parent": summary(load(sys.argv[1])), "new": summary(load(sys.argv[2]))}
    big = sorted((k for k in out["parent"]["kernels"] if GEMM in k), key=lambda k: -out["parent"]["kernels"][k]["us"])[:3]
    out["big_gemms_lengthen_us"] = {k: round(out["new"]["kernels"][k]["us"] - out["parent"]["kernels"][k]["us"], 2)
                                    for k in big if k in out["new"]["kernels"]}
    out["big_gemms_lengthen_us"]["sum"] = round(sum(out["big_gemms_lengthen_us"].values()), 2)
    text = json.dumps(out, indent=1)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
