"""gode_ode_bwd: discrete backprop (backprop = 1) against the continuous adjoint (backprop = 0), rk4 / two-layer, T = 16,
the reference's grid, at N = 32 and N = 1024, and the discrete launch with substeps = 4 (the forward re-run through ysteps).
HIP events around `--reps` back-to-back calls, `--rounds` rounds with the variants alternating; the median round is printed.

    python scripts/bench_ode_discrete.py [--baseline-lib PATH/libgode.so]

--baseline-lib: another build of the library (the parent commit's) whose adjoint launch is timed in the same rounds; the
extended op struct starts with that build's struct, so the same ops serve both."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import gan_ode_amd._lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--baseline-lib", default=None)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None, help="also append the result lines to this file")
args = ap.parse_args()

lib = L.lib()
base = None
if args.baseline_lib:
    base = C.CDLL(os.path.abspath(args.baseline_lib))
    base.gode_ode_bwd.argtypes, base.gode_ode_bwd.restype = [C.c_void_p, C.c_void_p], C.c_int


def st():
    return torch.cuda.current_stream().cuda_stream


torch.manual_seed(0)
P = [torch.randn(s, device="cuda") * 0.3 for s in ((64, 16), (64,), (16, 64), (16,), (16, 16), (16,), (16, 16), (16,))]
params = L.OdeParams(*[p.data_ptr() for p in P])
T = 16
tt = torch.linspace(0, 1, T)
dt = (tt[1:] - tt[:-1]).cuda()
lines = []
for N in (32, 1024):
    x = torch.randn(N, 16, device="cuda")
    z = torch.empty(N * T, 72, device="cuda")
    traj = torch.empty(N, T, 16, device="cuda")
    gz = torch.randn(N * T, 72, device="cuda")
    grads = torch.empty(L.ODE_NPARAM, device="cuda")
    work = torch.empty(lib.gode_ode_bwd_work_size(N), device="cuda")
    ysteps = torch.empty(lib.gode_ode_bwd_steps_size(N, T, 4, 0), device="cuda")

    def bwd(backprop, substeps):
        return L.OdeBwdOp(p=params, x=x.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), sel_t=None, gz=gz.data_ptr(),
                          work=work.data_ptr(), grads=grads.data_ptr(), N=N, T=T, substeps=substeps, prenet=1, accumulate=0,
                          zcols=72, backprop=backprop, ysteps=ysteps.data_ptr() if substeps > 1 and backprop else None)

    results = {}
    for substeps in (1, 4):
        fwd = L.OdeFwdOp(p=params, x=x.data_ptr(), content=None, dt=dt.data_ptr(), sel_t=None, z=z.data_ptr(),
                         traj=traj.data_ptr(), N=N, T=T, substeps=substeps, prenet=1, zcols=72)
        L.run_one(fwd, st())
        variants = [("adjoint", lib, bwd(0, substeps)), ("discrete", lib, bwd(1, substeps))]
        if base is not None:
            variants.insert(0, ("adjoint (baseline lib)", base, bwd(0, substeps)))
        times = {name: [] for name, _, _ in variants}
        for rnd in range(args.rounds + 1):          # (round 0 warms every variant up)
            for name, lb, op in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    rc = lb.gode_ode_bwd(C.byref(op), st())
                    assert rc == 0, (name, rc)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(e0.elapsed_time(e1) / args.reps * 1e3)
        for name, _, _ in variants:
            t = times[name]
            results[(name, substeps)] = statistics.median(t)
            lines.append(f"N={N:5d} T={T} rk4 two-layer substeps={substeps} {name:24s} median {statistics.median(t):8.2f} us"
                         f"  (min {min(t):.2f}, max {max(t):.2f}; {args.rounds} rounds x {args.reps} calls)")
    ref = results.get(("adjoint (baseline lib)", 1), results[("adjoint", 1)])
    lines.append(f"N={N:5d} ratio discrete / adjoint{' (baseline lib)' if base is not None else ''}, substeps=1: "
                 f"{results[('discrete', 1)] / ref:.3f}   (target <= 1.25)")
for ln in lines:
    print(ln)
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
