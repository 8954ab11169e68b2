"""Latent forward / adjoint launch times of both right-hand sides (rhs 0: W2 tanh(W1 y + b1) + b2; rhs 1: tanh(W1 y + b1)) under
the fixed-grid methods at N = 32 and N = 1024, T = 16, pre-net and content on: device-event time per launch, every
(method, rhs) in ONE process with the blocks alternating, median and range over the blocks -- scripts/bench_ode_methods.py
with the second axis.  A library without the `rhs` field (no _lib.ODE_RHS) is timed with the two-layer function alone, so
the same script gives the parent's rows.
    python scripts/bench_ode_rhs.py [--blocks 8] [--reps 400] [--tag NAME] [--out profiles/FILE.jsonl (appended)]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gan_ode_amd._lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=8)
ap.add_argument("--reps", type=int, default=400)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_ode_rhs.py times device launches: it needs the GPU"

def st(): return torch.cuda.current_stream().cuda_stream
codes = getattr(L, "ODE_METHODS", {"rk4": 0})
methods = [m for m in ("rk4", "euler", "midpoint") if m in codes]
rhs_codes = getattr(L, "ODE_RHS", {"mlp": 0})
torch.manual_seed(0)
P = [torch.randn(s, device="cuda") * 0.3 for s in ((64, 16), (64,), (16, 64), (16,), (16, 16), (16,), (16, 16), (16,))]
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
        for r, rc in rhs_codes.items():
            op = L.OdeParams(*[p.data_ptr() for p in (P if rc == 0 else P[:6])])       # rhs 1: W2 / b2 NULL
            extra = {"rhs": rc} if rc else {}
            f = L.OdeFwdOp(p=op, x=x.data_ptr(), content=c.data_ptr(), dt=dt.data_ptr(), sel_t=None, z=z.data_ptr(), traj=traj.data_ptr(),
                           N=N, T=T, substeps=1, prenet=1, zcols=96, method=codes[m], **extra)
            b = L.OdeBwdOp(p=op, x=x.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), sel_t=None, gz=gz.data_ptr(), work=work.data_ptr(),
                           grads=grads.data_ptr(), N=N, T=T, substeps=1, prenet=1, accumulate=0, zcols=96, method=codes[m], **extra)
            ops[(m, r, N, "fwd")], ops[(m, r, N, "bwd")] = f, b

def timed(o, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): L.run_one(o, st())
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us per launch

for key in ops:                                       # warm-up: every op (the adjoint reads the trajectory its forward left)
    if key[3] == "fwd":
        for _ in range(20): L.run_one(ops[key], st())
        for _ in range(20): L.run_one(ops[key[:3] + ("bwd",)], st())
torch.cuda.synchronize()
lines, samples = [], {k: [] for k in ops}
for blk in range(args.blocks):
    for N in (32, 1024):
        for m in methods:
            for r in rhs_codes:
                L.run_one(ops[(m, r, N, "fwd")], st())      # the trajectory of THIS solve for its adjoint
                for p in ("fwd", "bwd"):
                    us = timed(ops[(m, r, N, p)], args.reps)
                    samples[(m, r, N, p)].append(us)
                    lines.append(dict(tag=args.tag, block=blk, method=m, rhs=r, N=N, T=T, launch=p, us=round(us, 3), reps=args.reps))
for (m, r, N, p), v in samples.items():
    lines.append(dict(tag=args.tag, summary=True, method=m, rhs=r, N=N, T=T, launch=p, median_us=round(statistics.median(v), 3),
                      min_us=round(min(v), 3), max_us=round(max(v), 3), blocks=len(v)))
text = "\n".join(json.dumps(l) for l in lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(text + "\n")
