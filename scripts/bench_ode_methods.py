"""Latent forward / adjoint launch times of the fixed-grid methods (rk4, euler, midpoint) at N = 32 and N = 1024, T = 16,
pre-net on: device-event time per launch, all methods in ONE process with the blocks alternating (method after method
inside a block, block after block), median and range over the blocks.  A library without methods 2 and 3 (no
_lib.ODE_METHODS) is timed with rk4 alone, so the same script gives the parent's rk4 rows.
    python scripts/bench_ode_methods.py [--blocks 8] [--reps 400] [--out profiles/FILE.jsonl]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_ode_amd._lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=8)
ap.add_argument("--reps", type=int, default=400)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_ode_methods.py times device launches: it needs the GPU"

def st(): return torch.cuda.current_stream().cuda_stream
codes = getattr(L, "ODE_METHODS", {"rk4": 0})
methods = [m for m in ("rk4", "euler", "midpoint") if m in codes]
torch.manual_seed(0)
P = [torch.randn(s, device="cuda") * 0.3 for s in ((64, 16), (64,), (16, 64), (16,), (16, 16), (16,), (16, 16), (16,))]
op = L.OdeParams(*[p.data_ptr() for p in P])
T = 16
tt = torch.linspace(0, 1, T)
dt = (tt[1:] - tt[:-1]).cuda()
ops, keep = {}, []
for N in (32, 1024):
    x, c = torch.randn(N, 16, device="cuda"), torch.randn(N, 50, device="cuda")
    z, traj = torch.empty(N * T, 96, device="cuda"), torch.empty(N, T, 16, device="cuda")
    gz = torch.randn(N * T, 96, device="cuda")
    grads = torch.empty(L.ODE_NPARAM, device="cuda")
    work = torch.empty(L.lib().gode_ode_bwd_work_size(N), device="cuda")
    keep += [x, c, z, traj, gz, grads, work]
    for m in methods:
        f = L.OdeFwdOp(p=op, x=x.data_ptr(), content=c.data_ptr(), dt=dt.data_ptr(), sel_t=None, z=z.data_ptr(), traj=traj.data_ptr(),
                       N=N, T=T, substeps=1, prenet=1, zcols=96, method=codes[m])
        b = L.OdeBwdOp(p=op, x=x.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), sel_t=None, gz=gz.data_ptr(), work=work.data_ptr(),
                       grads=grads.data_ptr(), N=N, T=T, substeps=1, prenet=1, accumulate=0, zcols=96, method=codes[m])
        ops[(m, N, "fwd")], ops[(m, N, "bwd")] = f, b

def timed(o, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): L.run_one(o, st())
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch

for key in ops:                                       # warm-up: every op (the adjoint reads the trajectory its forward left)
    if key[2] == "fwd":
        for _ in range(20): L.run_one(ops[key], st())
        for _ in range(20): L.run_one(ops[key[:2] + ("bwd",)], st())
torch.cuda.synchronize()
lines, samples = [], {k: [] for k in ops}
for blk in range(args.blocks):
    for N in (32, 1024):
        for m in methods:
            L.run_one(ops[(m, N, "fwd")], st())      # the trajectory of THIS method for its adjoint
            for p in ("fwd", "bwd"):
                us = timed(ops[(m, N, p)], args.reps)
                samples[(m, N, p)].append(us)
                lines.append(dict(block=blk, method=m, N=N, T=T, launch=p, us=round(us, 3), reps=args.reps))
for (m, N, p), v in samples.items():
    lines.append(dict(summary=True, method=m, N=N, T=T, launch=p, median_us=round(statistics.median(v), 3), min_us=round(min(v), 3),
                      max_us=round(max(v), 3), blocks=len(v)))
text = "\n".join(json.dumps(l) for l in lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
