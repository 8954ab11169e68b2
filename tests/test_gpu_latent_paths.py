"""GPU: every dispatch path of the plain Neural-ODE motion latent (gode_ode_fwd / gode_ode_bwd and their _multi forms)
against a float64 oracle: oracle.ode_ref on float64 copies of the fp32 parameters and inputs.

The library picks the kernels from N, the method, whether a `sync` buffer is given and how many solves share a launch;
the test ids name the path:
  rk4-valu       N <= 8192: ode_valu.hip
  rk4-mfma       N > 8192: ode_fwd_kernel / ode_bwd_kernel (ode.hip; 256 threads with a content code, 64 without)
  reduce2        an rk4 / dopri5-fallback adjoint with more than 128 partial rows (N > 2048): latent_reduce_chunks_kernel
  dopri5-valu    N <= 32 (one workgroup, grads written directly) or N <= 4096 with `sync` (the cap: 128 workgroups
                 exchanging the whole-batch error norm)
  dopri5-mfma    N > 4096, N > 32 without `sync`, or the jobs of one _multi call spinning > 128 workgroups together:
                 ode_dopri5_fwd_kernel / ode_dopri5_bwd_kernel, one error norm per 64-trajectory workgroup
  dopri5-multi   several solves in one gode_ode_fwd_multi / gode_ode_bwd_multi launch (+ latent_rows_kernel)
A dopri5 reference uses the device's norm grouping: one oracle solve over the batch for the whole-batch norm, one per
consecutive 64-trajectory chunk for the fallback (reference gradient = the sum of the chunks').  Without a pre-net the
first 2128 floats of `grads` belong to the caller's neighbours (GradArena hands the adjoint a pointer that far in front
of the ODEFunc block): every adjoint here writes into a NaN-filled buffer the test owns, and those floats must stay NaN.
Latent rows and columns a kernel must not write carry NaN sentinels too.  Tolerances are those of the existing kernel
tests: states 1e-4 (rk4) / 2e-5 (dopri5), gradients 2e-4 / 1e-4."""
import copy

import pytest
import torch

from conftest import rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import solver_grid_arrays
from oracle import mocogan_ref as M
from oracle import ode_ref

pytestmark = pytest.mark.gpu

NP = L.ODE_NPARAM
OFF_W1 = 2128                   # start of the ODEFunc block of the gradient vector
BLOCKS = (("Wa", 0, 1024), ("ba", 1024, 64), ("Wb", 1088, 1024), ("bb", 2112, 16),
          ("W1", 2128, 256), ("b1", 2384, 16), ("W2", 2400, 256), ("b2", 2656, 16))
RTOL, ATOL = 1e-7, 1e-9
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


def identical(a, b):
    """Identical results: equal values (torch.equal) with the NaN sentinels in the same places."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


class Latent:
    """One latent solve: fp32 parameters and inputs (CPU), their device copies, the two op structs and NaN-filled output
    buffers with spare rows behind the ones the kernels own."""

    def __init__(self, N, T, seed, prenet, *, method, sel=False, content=True, zcols=72, sync=False, step_size=None):
        self.N, self.T, self.method, self.step_size = N, T, method, step_size
        self.prenet, self.zcols = prenet, zcols
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        self.f = M.OdeRhs(16, 16)
        self.pre = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.LeakyReLU(0.2), torch.nn.Linear(64, 16),
                                       torch.nn.LeakyReLU(0.2)) if prenet else None
        self.x = torch.randn(N, 16, generator=gen)
        self.tt = torch.linspace(0, 1, T).float()
        self.gup = torch.randn(N, T, 16, generator=gen)
        self.sel = torch.randint(0, T, (N,), generator=gen, dtype=torch.int32) if sel else None
        self.content = torch.randn(N, 50, generator=gen) if content else None
        params = (list(self.pre.parameters()) if prenet else []) + list(self.f.parameters())
        self.P = [p.detach().cuda() for p in params]
        ptrs = [p.data_ptr() for p in self.P]
        self.params = L.OdeParams(*(ptrs if prenet else [None] * 4 + ptrs))
        self.rows = N if sel else N * T
        self.xd = self.x.cuda()
        self.cd = self.content.cuda() if content else None
        self.seld = self.sel.cuda() if sel else None
        gz = torch.full((self.rows, zcols), NAN)          # only the 16 motion columns may be read
        gz[:, :16] = self.gup[torch.arange(N), self.sel.long()] if sel else self.gup.reshape(N * T, 16)
        self.gz = gz.cuda()
        self.nwg = (N + 63) // 64                          # 64-trajectory workgroups of the dopri5 fallback
        nsync = L.lib().gode_odernn_sync_size(N)
        self.sync_f = torch.zeros(max(nsync, 1), dtype=torch.int32, device="cuda") if sync else None
        self.sync_b = torch.zeros(max(nsync, 1), dtype=torch.int32, device="cuda") if sync else None
        self.work = torch.full((L.lib().gode_ode_bwd_work_size(N),), NAN, device="cuda")
        self.reset()
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        common = dict(p=self.params, x=self.xd.data_ptr(), sel_t=ptr(self.seld), N=N, T=T, prenet=int(prenet), zcols=zcols)
        if method == 0:
            self.dt = (self.tt[1:] - self.tt[:-1]).cuda()
            self.fop = L.OdeFwdOp(content=ptr(self.cd), dt=self.dt.data_ptr(), z=self.z.data_ptr(),
                                  traj=self.traj.data_ptr(), substeps=1, **common)
            self.bop = L.OdeBwdOp(traj=self.traj.data_ptr(), dt=self.dt.data_ptr(), gz=self.gz.data_ptr(),
                                  work=self.work.data_ptr(), grads=self.grads.data_ptr(), substeps=1, accumulate=0, **common)
            if step_size is not None:
                self.grid = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in solver_grid_arrays(T, step_size).items()}
                self.fop.G = self.grid["G"]
                self.fop.grid_dt, self.fop.emit_at = self.grid["grid_dt"].data_ptr(), self.grid["emit_at"].data_ptr()
                self.fop.emit_w = self.grid["emit_w"].data_ptr()
                self.bop.bstep_off, self.bop.bstep_dt = self.grid["bstep_off"].data_ptr(), self.grid["bstep_dt"].data_ptr()
        else:
            self.tout = self.tt.cuda()
            self.fop = L.OdeFwdOp(content=ptr(self.cd), dt=None, z=self.z.data_ptr(), traj=self.traj.data_ptr(), substeps=1,
                                  method=1, rtol=RTOL, atol=ATOL, tout=self.tout.data_ptr(), nsteps=self.nst.data_ptr(),
                                  sync=ptr(self.sync_f), **common)
            self.bop = L.OdeBwdOp(traj=self.traj.data_ptr(), dt=None, gz=self.gz.data_ptr(), work=self.work.data_ptr(),
                                  grads=self.grads.data_ptr(), substeps=0, accumulate=0, method=1, rtol=RTOL, atol=ATOL,
                                  tout=self.tout.data_ptr(), nsteps=self.nstb.data_ptr(), sync=ptr(self.sync_b), **common)

    def reset(self):
        """(Re)fill every output with its sentinel, in place (the op structs keep their pointers)."""
        N, T = self.N, self.T
        if not hasattr(self, "z"):
            self.z = torch.empty(self.rows + 2, self.zcols, device="cuda")
            self.traj = torch.empty(N + 1, T, 16, device="cuda")
            self.grads = torch.empty(NP + 16, device="cuda")
            self.nst = torch.empty(self.nwg + 1, dtype=torch.int32, device="cuda")
            self.nstb = torch.empty(self.nwg + 1, dtype=torch.int32, device="cuda")
        for t in (self.z, self.traj, self.grads):
            t.fill_(NAN)
        self.nst.fill_(-7)
        self.nstb.fill_(-7)

    def fwd(self):
        L.run_one(self.fop, stream())
        torch.cuda.synchronize()

    def bwd(self, accumulate):
        self.bop.accumulate = accumulate
        L.run_one(self.bop, stream())
        torch.cuda.synchronize()

    def outputs(self):
        return [t.clone() for t in (self.z, self.traj, self.nst)]

    # ---- float64 oracle -------------------------------------------------------------------------------------------
    def oracle(self, chunk=None):
        """-> states [N, T, 16], gradient vector [2672] (pre-net block zero without a pre-net), forward dopri5 trial
        steps per solve (counted in fp32, _trials_fp32).  chunk: one solve per consecutive `chunk` trajectories (the fallback's per-workgroup norm); the
        gradient is then the sum of the chunks'."""
        step = chunk or self.N
        zs, trials = [], []
        g = torch.zeros(NP, dtype=torch.float64)
        for n0 in range(0, self.N, step):
            z, gc, tr = self._oracle(slice(n0, min(self.N, n0 + step)))
            zs.append(z)
            g += gc
            trials.append(tr)
        return torch.cat(zs), g, trials

    def _oracle(self, sl):
        f = copy.deepcopy(self.f).double()
        pre = copy.deepcopy(self.pre).double() if self.prenet else None
        x = self.x[sl].double()
        y0 = pre(x) if pre is not None else x.requires_grad_(True)
        tt = self.tt.double()
        if self.method == 0:
            opts = None if self.step_size is None else {"step_size": self.step_size}
            sol = ode_ref.odeint_adjoint(f, y0, tt, method="rk4", options=opts)
        else:
            sol = ode_ref.odeint_adjoint(f, y0, tt, method="dopri5", rtol=RTOL, atol=ATOL)
        trials = self._trials_fp32(sl) if self.method == 1 else None
        z = sol.transpose(0, 1)                                   # [n, T, 16]
        w = self.gup[sl].double()
        if self.sel is not None:
            w = w * (torch.arange(self.T)[None, :] == self.sel[sl].long()[:, None]).double()[:, :, None]
        (z * w).sum().backward()
        params = (list(pre.parameters()) if pre is not None else []) + list(f.parameters())
        g = torch.zeros(NP, dtype=torch.float64)
        for (_, o, n), p in zip(BLOCKS if pre is not None else BLOCKS[4:], params):
            g[o:o + n] = p.grad.reshape(-1)
        return z.detach(), g, trials

    def _trials_fp32(self, sl):
        """Trial steps of the same dopri5 solve in fp32 (torchdiffeq's arithmetic at the reference's dtype).  At rtol 1e-7
        the fp32 round-off in the error estimate is about half the tolerance, so an fp32 controller rejects steps a
        float64 one accepts (~2 more trials here): the device's counts are compared with this solve, not the float64 one."""
        f = copy.deepcopy(self.f)
        calls = [0]          # a dopri5 solve makes 2 evaluations for its initial step + 6 per trial step
        f.register_forward_pre_hook(lambda *_: calls.__setitem__(0, calls[0] + 1))
        with torch.no_grad():
            y0 = self.pre(self.x[sl]) if self.prenet else self.x[sl]
            ode_ref.odeint(f, y0, self.tt, method="dopri5", rtol=RTOL, atol=ATOL)
        return (calls[0] - 2) // 6

    # ---- checks ---------------------------------------------------------------------------------------------------
    def check_fwd(self, zref, tol):
        N, T, rows = self.N, self.T, self.rows
        z, traj = self.z.cpu(), self.traj.cpu()
        assert rel_err(traj[:N], zref) < tol, rel_err(traj[:N], zref)
        want = zref[torch.arange(N), self.sel.long()] if self.sel is not None else zref.reshape(N * T, 16)
        assert rel_err(z[:rows, :16], want) < tol, rel_err(z[:rows, :16], want)
        if self.content is not None:
            c = self.content if self.sel is not None else self.content.repeat_interleave(T, 0)
            assert torch.equal(z[:rows, 16:66], c)
            assert bool((z[:rows, 66:] == 0).all())                # pad columns
        else:
            assert bool(z[:rows, 16:].isnan().all())               # content NULL: the kernels leave those columns alone
        assert bool(z[rows:].isnan().all()) and bool(traj[N:].isnan().all())

    def check_grads(self, gref, tol):
        g = self.grads.cpu()
        assert bool(g[NP:].isnan().all())
        if not self.prenet:
            assert bool(g[:OFF_W1].isnan().all()), f"pre-net block written: {int((~g[:OFF_W1].isnan()).sum())} of 2128 floats"
        for name, o, n in BLOCKS if self.prenet else BLOCKS[4:]:
            assert rel_err(g[o:o + n], gref[o:o + n]) < tol, (name, rel_err(g[o:o + n], gref[o:o + n]))

    def check_accumulated(self, base):
        """grads after a second adjoint with accumulate = 1 on top of `base` (the first one's result)."""
        lo = 0 if self.prenet else OFF_W1
        g = self.grads.cpu()
        assert rel_err(g[lo:NP], 2 * base[lo:NP].cpu()) < 1e-6
        assert bool(g[NP:].isnan().all()) and bool(g[:lo].isnan().all())

    def check_nsteps(self, nst, trials, T_min=None):
        """dopri5 trial-step counts: nsteps[0] for one whole-batch norm (trials: one count), ceil(N/64) entries for the
        per-workgroup fallback (trials: one per chunk); the entries behind them keep their sentinel.  Forward counts
        equal the fp32 oracle's up to one borderline accept/reject decision; adjoint counts (T_min) are only bounded below."""
        v = nst.cpu()
        k = len(trials)
        if T_min is None:
            assert all(abs(int(v[w]) - trials[w]) <= 1 for w in range(k)), (v[:k].tolist(), trials)
        else:
            assert int(v[:k].min()) >= T_min, v[:k].tolist()
        assert bool((v[k:] == -7).all()), v.tolist()


def _adjoint_checks(lat, gref, tol, run):
    """accumulate = 0 against the oracle, a second identical call bitwise, accumulate = 1 doubles the result."""
    run(0)
    lat.check_grads(gref, tol)
    g1 = lat.grads.clone()
    run(0)
    assert identical(lat.grads, g1), "adjoint not deterministic"
    run(1)
    lat.check_accumulated(g1)
    return g1


# ---------------------------------------------------------------------------------------------------------------------
# 1. rk4 across the VALU / MFMA switch (N > 8192) and the one- / two-level gradient reduce (> 128 partial rows of 16)
# (N, T, prenet, content, sel_t, zcols, step_size)
RK4_CASES = [
    pytest.param(2048, 5, True, True, False, 96, None, id="rk4-valu-N2048-reduce1-prenet-content"),
    pytest.param(2049, 5, False, False, True, 68, None, id="rk4-valu-N2049-reduce2-lastchunk1-noprenet-sel"),
    pytest.param(8192, 4, True, True, True, 68, None, id="rk4-valu-N8192-limit-reduce2-prenet-sel"),
    pytest.param(8193, 4, False, True, False, 96, None, id="rk4-mfma-N8193-lastblock1-reduce2-noprenet-content"),
    pytest.param(9001, 6, True, False, True, 96, 0.15, id="rk4-mfma-N9001-stepsize-prenet-nocontent-sel"),
    pytest.param(9001, 4, False, True, False, 68, 0.3, id="rk4-mfma-N9001-stepsize-noprenet-content"),
]


@pytest.mark.parametrize("N,T,prenet,content,sel,zcols,step_size", RK4_CASES)
def test_rk4_latent_paths_against_float64_oracle(N, T, prenet, content, sel, zcols, step_size):
    lat = Latent(N, T, 1000 + N + T, prenet, method=0, sel=sel, content=content, zcols=zcols, step_size=step_size)
    zref, gref, _ = lat.oracle()
    lat.fwd()
    lat.check_fwd(zref, 1e-4)
    out = lat.outputs()
    lat.fwd()
    assert all(identical(a, b) for a, b in zip(out, lat.outputs())), "forward not deterministic"
    _adjoint_checks(lat, gref, 2e-4, lat.bwd)


# ---------------------------------------------------------------------------------------------------------------------
# 2. dopri5, one op (gode_ode_fwd / gode_ode_bwd, method 1, substeps 0)
# (N, T, prenet, sync, sel_t, chunk): chunk None = one whole-batch norm, 64 = the per-workgroup fallback
D5_CASES = [
    pytest.param(20, 4, False, False, True, None, id="dopri5-valu-direct-N20-noprenet-sel"),
    pytest.param(4096, 2, True, True, False, None, id="dopri5-valu-cap-N4096-prenet"),
    pytest.param(4096, 3, False, True, True, None, id="dopri5-valu-cap-N4096-noprenet-sel"),
    pytest.param(4128, 2, False, True, False, 64, id="dopri5-mfma-N4128-over-cap-reduce2-noprenet"),
    pytest.param(4128, 2, True, True, True, 64, id="dopri5-mfma-N4128-over-cap-reduce2-prenet-sel"),
    pytest.param(33, 4, True, False, True, 64, id="dopri5-mfma-nosync-N33-prenet-sel"),
    pytest.param(100, 4, False, False, False, 64, id="dopri5-mfma-nosync-N100-noprenet"),
]


@pytest.mark.parametrize("N,T,prenet,sync,sel,chunk", D5_CASES)
def test_dopri5_latent_paths_against_float64_oracle(N, T, prenet, sync, sel, chunk):
    lat = Latent(N, T, 2000 + N + T, prenet, method=1, sel=sel, sync=sync)
    zref, gref, trials = lat.oracle(chunk)
    lat.fwd()
    lat.check_fwd(zref, 2e-5)
    lat.check_nsteps(lat.nst, trials)
    out = lat.outputs()
    lat.fwd()
    assert all(identical(a, b) for a, b in zip(out, lat.outputs())), "forward not deterministic"
    _adjoint_checks(lat, gref, 1e-4, lat.bwd)
    lat.check_nsteps(lat.nstb, trials, T_min=T - 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3. dopri5, several ops per launch
def _fwd_multi(lats):
    arr = (L.OdeFwdOp * len(lats))(*[a.fop for a in lats])
    L.check(L.lib().gode_ode_fwd_multi(arr, len(lats), stream()), "gode_ode_fwd_multi")
    torch.cuda.synchronize()


def _bwd_multi(lats, accumulate):
    for a, acc in zip(lats, accumulate):
        a.bop.accumulate = acc
    arr = (L.OdeBwdOp * len(lats))(*[a.bop for a in lats])
    L.check(L.lib().gode_ode_bwd_multi(arr, len(lats), stream()), "gode_ode_bwd_multi")
    torch.cuda.synchronize()


def _singles(lats):
    """Every op alone (gode_ode_fwd / gode_ode_bwd, accumulate 0): forward outputs and gradient vectors."""
    fwd, grads = [], []
    for a in lats:
        a.reset()
        a.fwd()
        fwd.append(a.outputs())
        a.bwd(0)
        grads.append(a.grads.clone())
    return fwd, grads


def _check_multi_fwd_bitwise(lats, fwd):
    for a in lats:
        a.reset()
    _fwd_multi(lats)
    for k, a in enumerate(lats):
        assert all(identical(u, v) for u, v in zip(fwd[k], a.outputs())), f"fused forward of op {k} != its single-op call"
    out = [a.outputs() for a in lats]
    _fwd_multi(lats)
    assert all(identical(u, v) for o, a in zip(out, lats) for u, v in zip(o, a.outputs())), "forward not deterministic"


def _shared_oracle(lats):
    g = torch.zeros(NP, dtype=torch.float64)
    for a in lats:
        g += a.oracle()[1]
    return g


@pytest.mark.parametrize("fallback,pair_flags", [(False, (0, 1)), (True, (0, 1)), (True, (0, 0))],
                         ids=["dopri5-multi-fused", "dopri5-multi-nosync-op-falls-back", "dopri5-multi-nosync-op-falls-back-flags00"])
def test_dopri5_multi_matches_single_ops_and_shared_grads_the_oracle_sum(fallback, pair_flags):
    """Ops of mixed shape in one launch: one workgroup (own grads), four workgroups with `sync` and a pre-net, and a
    two-workgroup + one-workgroup pair without pre-net sharing one grads vector (the video and the image path of one
    generator: the first stores, the second adds).  fallback: one more op without `sync` (N = 70), which falls back to
    the per-workgroup kernels alone in the forward and sends every adjoint of the call down the one-op-at-a-time path.
    Forward outputs and own-grads adjoints are bitwise their single-op calls; the shared vector is the oracle's sum.
    pair_flags: the shared pair's accumulate flags.  (0, 0) on the one-op-at-a-time path pins the group rule of gode.h from this
    user of the shared launcher template (tests/test_gpu_odernn_paths.py: multi-sequential-flags00 is the other): the later op
    of a group adds, whatever its flag."""
    a = Latent(20, 4, 31, False, method=1)
    b = Latent(100, 3, 32, True, method=1, sync=True)
    d = Latent(40, 4, 33, False, method=1, sync=True, sel=True)
    e = Latent(24, 4, 34, False, method=1, sel=True)
    lats = [a, b, d, e]
    if fallback:
        lats.insert(2, Latent(70, 3, 35, True, method=1))
    fwd, grads = _singles(lats)
    _check_multi_fwd_bitwise(lats, fwd)
    own = [x for x in lats if x not in (d, e)]
    e.bop.grads = d.grads.data_ptr()
    gshared = _shared_oracle([d, e])
    acc0 = [pair_flags[1] if x is e else 0 for x in lats]
    for x in lats:
        x.grads.fill_(NAN)

    def run(acc):
        _bwd_multi(lats, acc0 if acc == 0 else [1] * len(lats))

    run(0)
    for x in own:
        assert identical(x.grads, grads[lats.index(x)]), f"op N={x.N}: fused adjoint != its single-op call"
    d.check_grads(gshared, 1e-4)
    assert bool(e.grads.isnan().all())
    saved = [x.grads.clone() for x in lats]
    run(0)
    assert all(identical(x.grads, s) for x, s in zip(lats, saved)), "adjoint not deterministic"
    run(1)
    for x, s in zip(lats, saved):
        if x is not e:
            x.check_accumulated(s)


def test_dopri5_multi_jobs_over_the_cap_together_fall_back():
    """Two ops of N = 2080 with `sync` (65 workgroups each: each fits the co-residency limit of 128, together they do not)
    and a one-workgroup op: both multi-workgroup jobs fall back to one norm per 64 trajectories -- nsteps then holds one
    count per such workgroup, and results match the per-64 oracle, not the whole-batch single-op results.  The
    one-workgroup op still matches its single-op call bitwise."""
    p = Latent(2080, 2, 41, True, method=1, sync=True)
    q = Latent(2080, 2, 42, False, method=1, sync=True, sel=True)
    s = Latent(20, 3, 43, False, method=1)
    lats = [p, q, s]
    fwd, grads = _singles(lats)
    for a in lats:
        a.reset()
    _fwd_multi(lats)
    assert all(identical(u, v) for u, v in zip(fwd[2], s.outputs()))
    refs = [a.oracle(64) for a in (p, q)]
    for a, (zref, _, trials) in zip((p, q), refs):
        assert len(trials) == 33
        a.check_fwd(zref, 2e-5)
        a.check_nsteps(a.nst, trials)
    out = [a.outputs() for a in lats]
    _fwd_multi(lats)
    assert all(identical(u, v) for o, a in zip(out, lats) for u, v in zip(o, a.outputs())), "forward not deterministic"

    def run(acc):
        _bwd_multi(lats, [acc] * 3)

    for a in lats:
        a.grads.fill_(NAN)
    run(0)
    assert identical(s.grads, grads[2])
    for a, (_, gref, trials) in zip((p, q), refs):
        a.check_grads(gref, 1e-4)
        a.check_nsteps(a.nstb, trials, T_min=1)
    saved = [a.grads.clone() for a in lats]
    run(0)
    assert all(identical(a.grads, g) for a, g in zip(lats, saved)), "adjoint not deterministic"
    run(1)
    for a, g in zip(lats, saved):
        a.check_accumulated(g)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the user-visible form of the no-pre-net contract
def test_trainer_dopri5_without_prenet_direct_grads_is_bitwise_the_stock_path():
    """ode_method = "dopri5", linear=False: GanTrainer's G step flushes the video and the image adjoint as one
    gode_ode_bwd_multi call into the gradient arena, whose ODEFunc block is preceded by decoder tensors.  One step with
    direct_grads=True must give bitwise the losses, parameters and .grad tensors of direct_grads=False."""
    runs = []
    for direct in (True, False):
        seed_all(91)
        gen = G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8, linear=False)
        gen.ode_method = "dopri5"
        dv, di = G.VideoDiscriminator(1, ksize=2, ndf=8), G.PatchImageDiscriminator(1, ndf=8)
        for m in (gen, dv, di):
            m.cuda()
        tr = G.GanTrainer(gen, dv, di, direct_grads=direct)
        rng = torch.Generator().manual_seed(5)
        imgs = [torch.rand(4, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        vids = [torch.rand(4, 16, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        seed_all(92)
        losses = [float(v) for v in tr.step(imgs, vids)]
        if direct:
            arena = tr.arenas[id(gen)]
            assert arena.params[-4] is gen.ode_fn.fn[0].weight and arena.params[-1] is gen.ode_fn.fn[2].bias
        runs.append((losses, [p.detach().clone() for m in (gen, dv, di) for p in m.parameters()],
                     [None if p.grad is None else p.grad.clone() for p in gen.parameters()]))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][2], runs[1][2]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
