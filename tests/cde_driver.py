"""The kernel-level driver of the CDE tests: the seeded parameters, guarded buffers and one gode_cde_fwd / gode_cde_bwd call
(Solve) with every output inside NaN / sentinel guards.  Shared by tests/test_gpu_cde.py and
tests/test_gpu_latent_schedules.py; params64() runs without a GPU (tests/test_host_latent_schedules.py)."""
import numpy as np
import torch

import cde_ref as R
from conftest import seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L

GUARD = 64
KINK = 2e-6
NAN = float("nan")
NAMES = "Wa ba Wb bb W1 b1 W2 b2".split()


def stream():
    return torch.cuda.current_stream().cuda_stream


def params64(seed=3):
    """f and CDEFunc weights of a seeded VideoGeneratorCDE (the default init) as float64 leaves (CPU)."""
    seed_all(seed)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8)
    return R.params_of(gen)


def _params(seed=3):
    """f and CDEFunc weights of a seeded VideoGeneratorCDE (the default init), fp32 on the GPU + float64 leaves."""
    P64 = params64(seed)
    P32 = [p.detach().float().cuda().contiguous() for p in P64]
    return P32, P64


def _guarded(n, dtype=torch.float32, fill=NAN):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, fill=NAN):
    b = buf.cpu()
    for part in (b[:GUARD], b[-GUARD:]):
        if np.isnan(fill):
            assert torch.isnan(part).all()
        else:
            assert (part == fill).all()


class Solve:
    """One gode_cde_fwd call with every output inside NaN / sentinel guards.  content ([N, 50] or None) and zcols: the
    row of z is [16 motion | 50 content | zeros up to zcols] with a content code, 16 motion columns in a row of zcols
    floats (the rest untouched) without one."""

    def __init__(self, P32, x, T, S_cap=512, sel=None, rtol=1e-4, atol=1e-6, content=None, zcols=16):
        N = x.shape[0]
        self.P32, self.N, self.T, self.S_cap, self.sel, self.zcols = P32, N, T, S_cap, sel, zcols
        self.x = x.float().cuda().contiguous()
        self.tslope = R.time_slopes(T).float().cuda()
        self.rows = rows = N if sel is not None else N * T
        self.zb, self.z = _guarded(rows * zcols)
        self.sb, self.states = _guarded(int(L.lib().gode_cde_state_size(N, S_cap)))
        self.hb, self.sched = _guarded(2 * S_cap, torch.float64)
        self.cb, self.counts = _guarded(2, torch.int32, -7)
        ns = int(L.lib().gode_cde_sync_size(N))
        self.sync = torch.zeros(max(ns, 1), dtype=torch.int32, device="cuda")
        self.sel_d = sel.to(torch.int32).cuda() if sel is not None else None
        self.content_d = content.float().cuda().contiguous() if content is not None else None
        self.op = L.CdeFwdOp(p=L.CdeParams(*[p.data_ptr() for p in P32]), x=self.x.data_ptr(),
                             tslope=self.tslope.data_ptr(),
                             content=self.content_d.data_ptr() if content is not None else None,
                             sel_t=self.sel_d.data_ptr() if sel is not None else None, z=self.z.data_ptr(),
                             states=self.states.data_ptr(), sched=self.sched.data_ptr(), counts=self.counts.data_ptr(),
                             sync=self.sync.data_ptr() if ns else None, N=N, T=T, S_cap=S_cap, zcols=zcols,
                             rtol=rtol, atol=atol)
        L.run_one(self.op, stream())
        torch.cuda.synchronize()
        self.acc, self.trials = [int(v) for v in self.counts.cpu()]

    def schedule(self):
        s = self.sched.cpu()
        return s[:self.acc], s[self.S_cap:self.S_cap + self.acc]

    def backward(self, gz, accumulate=0, init=None):
        """gz [rows, 16] -> (grads [7536] block, its guarded buffer).  With zcols > 16 the upstream rows are zcols wide
        and hold NaN outside the 16 motion columns: the kernel must not read there."""
        gzd = gz.float().cuda().contiguous()
        if self.zcols != 16:
            wide = torch.full((self.rows, self.zcols), NAN, device="cuda")
            wide[:, :16] = gzd.view(self.rows, 16)
            gzd = wide
        gb, grads = _guarded(L.CDE_NPARAM)
        if init is not None:
            grads.copy_(init.cuda())
        work = torch.full((int(L.lib().gode_cde_bwd_work_size(self.N)),), NAN, device="cuda")
        op = L.CdeBwdOp(p=self.op.p, x=self.op.x, tslope=self.op.tslope, sel_t=self.op.sel_t, states=self.op.states,
                        sched=self.op.sched, counts=self.op.counts, gz=gzd.data_ptr(), work=work.data_ptr(),
                        grads=grads.data_ptr(), N=self.N, T=self.T, S_cap=self.S_cap, accumulate=accumulate,
                        zcols=self.zcols)
        L.run_one(op, stream())
        torch.cuda.synchronize()
        return grads.cpu(), gb


def _split(g):
    return [g[o:o + k].view(shp) for o, k, shp in G.modules._CDE_GRAD_OFFS]
