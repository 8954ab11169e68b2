"""sha256 of the rk4 (method 0) vector-ALU forward / adjoint results (latent rows, trajectory, gradient vector) on seeded
inputs, one line per case: run from the root of two trees and compare the outputs (profiles/ode_methods_rk4_hashes.txt).
    python scripts/ode_rk4_hashes.py"""
import hashlib, os, sys
sys.path.insert(0, os.getcwd())
import torch
import gan_ode_amd._lib as L
from gan_ode_amd.modules import solver_grid_arrays

def st(): return torch.cuda.current_stream().cuda_stream
def h(t): return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]
torch.manual_seed(0)
P = [torch.randn(s, device="cuda") * 0.3 for s in ((64, 16), (64,), (16, 64), (16,), (16, 16), (16,), (16, 16), (16,))]
for N, T, prenet, sub, step in ((32, 16, 1, 1, None), (33, 5, 0, 1, None), (1024, 16, 1, 1, None), (20, 4, 1, 3, None), (20, 6, 1, 1, 0.15),
                                (2049, 3, 0, 1, 0.3), (8192, 4, 1, 1, None)):
    op = L.OdeParams(*[(p.data_ptr() if (prenet or k >= 4) else None) for k, p in enumerate(P)])
    tt = torch.linspace(0, 1, T); dt = (tt[1:] - tt[:-1]).cuda()
    g = torch.Generator().manual_seed(N + T)
    x, c = torch.randn(N, 16, generator=g).cuda(), torch.randn(N, 50, generator=g).cuda()
    gz = torch.randn(N * T, 96, generator=g).cuda()
    z, traj = torch.zeros(N * T, 96, device="cuda"), torch.zeros(N, T, 16, device="cuda")
    grads = torch.zeros(L.ODE_NPARAM, device="cuda")
    work = torch.empty(L.lib().gode_ode_bwd_work_size(N), device="cuda")
    f = L.OdeFwdOp(p=op, x=x.data_ptr(), content=c.data_ptr(), dt=dt.data_ptr(), sel_t=None, z=z.data_ptr(), traj=traj.data_ptr(),
                   N=N, T=T, substeps=sub, prenet=prenet, zcols=96)
    b = L.OdeBwdOp(p=op, x=x.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), sel_t=None, gz=gz.data_ptr(), work=work.data_ptr(),
                   grads=grads.data_ptr(), N=N, T=T, substeps=sub, prenet=prenet, accumulate=0, zcols=96)
    if step is not None:
        gd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in solver_grid_arrays(T, step).items()}
        f.G = gd["G"]
        f.grid_dt, f.emit_at, f.emit_w = gd["grid_dt"].data_ptr(), gd["emit_at"].data_ptr(), gd["emit_w"].data_ptr()
        b.bstep_off, b.bstep_dt = gd["bstep_off"].data_ptr(), gd["bstep_dt"].data_ptr()
    L.run_one(f, st()); L.run_one(b, st()); torch.cuda.synchronize()
    print(N, T, prenet, sub, step, h(z), h(traj), h(grads[0 if prenet else 2128:]))
