"""GPU: torchdiffeq's euler and midpoint on the plain Neural-ODE motion latent (gode_ode_fwd / gode_ode_bwd methods 2 and
3; gen.ode_method = "euler" / "midpoint"), forward and continuous adjoint.

Op level: as tests/test_gpu_latent_paths.py (whose Latent this file extends) -- fp32 parameters and inputs, a float64
oracle.ode_ref.odeint_adjoint(method=name) reference, NaN sentinels behind every buffer and in columns a kernel must not
write, tolerances of the fixed-grid kernels: states 1e-4, gradients 2e-4.  At T = 16 the float64 midpoint and rk4
solutions differ by 2e-5..3e-5, INSIDE that tolerance, so the tableau is checked at T = 2 and T = 3, where each case
first asserts that the oracle's solutions of the other two fixed-grid methods lie >= 10 x the tolerance away from the
expected one (states and ODEFunc gradient); the larger-T cases check the grids, not the tableau.  `substeps` is the
build's own extension: its reference takes the oracle's steps on the refined grid (_substep_oracle).

Module level: the public classes against oracle.mocogan_ref.Generator(ode_method=name) / tests/categ_ref.py at the same
seeds with the tolerances of the rk4 tests of tests/test_gpu_modules.py (frames 1e-4; generator gradients median-based
5e-3, max-norm 5e-2: one flipped BatchNorm/ReLU kink of a tiny net, see there)."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_err, seed_all

import categ_ref as R
import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd import modules as Mod
from oracle import mocogan_ref as M
from oracle import ode_ref
from test_gpu_latent_paths import BLOCKS, NP, OFF_W1, Latent, _adjoint_checks, identical

pytestmark = pytest.mark.gpu

STOL, GTOL = 1e-4, 2e-4                 # op level: states, gradients
TOL = 1e-4                              # module level: frames
METHODS = [pytest.param("euler", id="euler"), pytest.param("midpoint", id="midpoint")]
FIXED = ("rk4", "euler", "midpoint")


def robust_rel(a, b):
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64).flatten()
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64).flatten()
    return float((a - b).abs().median() / (b.norm() / b.numel() ** 0.5).clamp_min(1e-300))


class FixedLatent(Latent):
    """A fixed-grid latent solve (Latent with method 0) whose ops carry `name`'s code."""

    def __init__(self, N, T, seed, prenet, name, *, substeps=1, **kw):
        super().__init__(N, T, seed, prenet, method=0, **kw)
        self.name, self.substeps = name, substeps
        if T == 1:                       # no interval: the ops still want a dt pointer
            self.dt = torch.zeros(1, device="cuda")
            self.fop.dt = self.bop.dt = self.dt.data_ptr()
        self.set_method(name)
        self.fop.substeps = self.bop.substeps = substeps

    def set_method(self, name):
        self.name = name
        self.fop.method = self.bop.method = L.ODE_METHODS[name]

    def oracle(self, name=None):
        """-> states [N, T, 16], gradient vector [2672] of `name` (default: the ops' method) in float64."""
        name = name or self.name
        f = copy.deepcopy(self.f).double()
        pre = copy.deepcopy(self.pre).double() if self.prenet else None
        x = self.x.double()
        y0 = pre(x) if pre is not None else x.requires_grad_(True)
        tt = self.tt.double()
        w = self.gup.double()
        if self.sel is not None:
            w = w * (torch.arange(self.T)[None, :] == self.sel.long()[:, None]).double()[:, :, None]
        if self.substeps == 1:
            opts = None if self.step_size is None else {"step_size": self.step_size}
            z = ode_ref.odeint_adjoint(f, y0, tt, method=name, options=opts).transpose(0, 1)
            (z * w).sum().backward()
        else:
            z, a0, gth = _substep_oracle(f, y0.detach(), tt, self.substeps, name, w.transpose(0, 1))
            for p, g in zip(f.parameters(), gth):
                p.grad = g
            y0.backward(a0)
            z = z.transpose(0, 1)
        params = (list(pre.parameters()) if pre is not None else []) + list(f.parameters())
        g = torch.zeros(NP, dtype=torch.float64)
        for (_, o, n), p in zip(BLOCKS if pre is not None else BLOCKS[4:], params):
            g[o:o + n] = p.grad.reshape(-1)
        return z.detach(), g, None

    def run_all(self):
        """Forward (against the oracle, twice: bitwise) and the three adjoint checks."""
        zref, gref, _ = self.oracle()
        self.fwd()
        self.check_fwd(zref, STOL)
        out = self.outputs()
        self.fwd()
        assert all(identical(a, b) for a, b in zip(out, self.outputs())), "forward not deterministic"
        _adjoint_checks(self, gref, GTOL, self.bwd)
        return zref, gref


def _substep_oracle(f, y0, tt, k, name, grad_sol):
    """`substeps` = k in float64 with the oracle's own steppers: the forward solve on the grid that splits every output
    interval into k equal steps, and oracle.ode_ref's adjoint loop (per output interval in reverse time, y reset to the
    stored solution, a += grad_out) with each interval's augmented solve on the same k steps.
    -> solution [T, N, 16], dL/dy0, [dL/dtheta]."""
    T = len(tt)
    theta = tuple(f.parameters())

    def refined(a, b):
        return torch.cat([a + (b - a) / k * torch.arange(k, dtype=tt.dtype), b.reshape(1)])

    with torch.no_grad():
        sol = [y0]
        for j in range(T - 1):
            sol.append(ode_ref.odeint(f, sol[-1], refined(tt[j], tt[j + 1]), method=name)[-1])
        sol = torch.stack(sol)
        state = [torch.zeros((), dtype=sol.dtype), sol[-1], grad_sol[-1]] + [torch.zeros_like(p) for p in theta]

        def aug(tau, s):
            y, a = s[1], s[2]
            with torch.enable_grad():
                y_req = y.detach().requires_grad_(True)
                val = f(tau.detach(), y_req)
                grads = torch.autograd.grad(val, (y_req,) + theta, -a)
            return (torch.zeros_like(s[0]), val.detach(), *grads)

        for i in range(T - 1, 0, -1):
            seg = ode_ref.odeint(aug, tuple(state), refined(tt[i], tt[i - 1]), method=name)
            state = [c[-1] for c in seg]
            state[1] = sol[i - 1]
            state[2] = state[2] + grad_sol[i - 1]
    return sol, state[2], state[3:]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the tableau: T = 2 and T = 3, where the three fixed-grid methods are far apart
@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("T,prenet,sel", [pytest.param(2, True, False, id="T2-prenet-content"),
                                          pytest.param(3, False, True, id="T3-noprenet-sel")])
def test_tableau_is_told_apart_from_the_other_fixed_grid_methods(name, T, prenet, sel):
    """Seed 12, chosen on the float64 oracle alone: at T = 3 the midpoint / rk4 gap of default-initialised nets straddles
    10 x the state tolerance (3.4e-4 .. 1.5e-3 over seeds 10-39; this seed: 1.5e-3 states, 4.4e-3 gradient).  T = 2 with
    the same seed: 7.1e-3 / 1.8e-2; euler is >= 2.7e-2 / 1.2e-1 from either at both lengths."""
    lat = FixedLatent(33, T, 12, prenet, name, sel=sel, content=True)
    zref, gref, _ = lat.oracle()
    for other in FIXED:
        if other != name:
            zo, go, _ = lat.oracle(other)
            ds, dg = rel_err(zo, zref), rel_err(go[OFF_W1:], gref[OFF_W1:])
            print(f"{name} vs {other}: states {ds:.3g} gradient {dg:.3g}")
            assert ds >= 10 * STOL and dg >= 10 * GTOL, (other, ds, dg)
    lat.run_all()                   # (check_grads: without a pre-net the first 2128 floats of grads stay NaN)


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes and grids
# (N, T, prenet, content, sel_t, zcols, substeps, step_size)
GRID_CASES = [
    pytest.param(1, 5, True, True, False, 72, 1, None, id="N1-single-trajectory"),
    pytest.param(17, 5, True, True, False, 68, 1, None, id="N17-second-workgroup-of-one"),
    pytest.param(9, 1, True, True, False, 72, 1, None, id="T1-no-steps"),
    pytest.param(20, 4, True, True, False, 72, 3, None, id="N20-substeps3"),
    pytest.param(20, 4, False, False, True, 72, 3, None, id="N20-substeps3-noprenet-sel"),
    pytest.param(20, 6, True, True, False, 68, 1, 0.15, id="N20-stepsize0.15-interpolated"),
    pytest.param(20, 6, False, True, True, 96, 1, 0.15, id="N20-stepsize0.15-sel"),
    pytest.param(20, 6, True, False, False, 96, 1, 0.3, id="N20-stepsize0.3-steps-span-outputs"),
    pytest.param(20, 6, True, True, True, 68, 1, 0.3, id="N20-stepsize0.3-sel"),
    pytest.param(2049, 3, True, True, False, 72, 1, None, id="N2049-two-level-reduce"),
]


@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("N,T,prenet,content,sel,zcols,substeps,step_size", GRID_CASES)
def test_method_against_float64_oracle(name, N, T, prenet, content, sel, zcols, substeps, step_size):
    lat = FixedLatent(N, T, 3000 + N + T, prenet, name, sel=sel, content=content, zcols=zcols, substeps=substeps,
                      step_size=step_size)
    zref, gref = lat.run_all()
    if T == 1:
        # no steps: the output is the pre-net's, and the adjoint is the upstream gradient through the pre-net alone
        pre = copy.deepcopy(lat.pre).double()
        y0 = pre(lat.x.double())
        assert rel_err(zref[:, 0], y0.detach()) < 1e-12
        (y0 * lat.gup[:, 0].double()).sum().backward()
        assert rel_err(gref[:OFF_W1], torch.cat([p.grad.reshape(-1) for p in pre.parameters()])) < 1e-12
        assert float(gref[OFF_W1:].abs().max()) == 0.0 and float(lat.grads[OFF_W1:NP].abs().max()) == 0.0


@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("content", [True, False], ids=["content", "content-null"])
def test_methods_stay_on_the_valu_kernels_above_the_mfma_switch(name, content):
    """N = 8193 > 8192: rk4 leaves for the MFMA-chain kernels there, which step with Kutta 3/8 only; methods 2 and 3 must
    give their own solutions within the same tolerances.  (The rk4 oracle lies more than 2 x the tolerance away -- asserted;
    midpoint: 8.9e-4 states, 2.7e-3 gradient -- so a Kutta-3/8 result would miss the tolerance by at least its width.)
    The same object with method 0 still passes against the rk4 oracle."""
    lat = FixedLatent(8193, 3, 77, True, name, content=content, zcols=96)
    zref, gref = lat.run_all()
    lat.set_method("rk4")
    z4, g4, _ = lat.oracle()
    assert rel_err(z4, zref) >= 2 * STOL and rel_err(g4[OFF_W1:], gref[OFF_W1:]) >= 2 * GTOL
    lat.reset()
    lat.run_all()


def test_method_codes_above_3_are_refused():
    lat = FixedLatent(5, 3, 5, True, "euler")
    for op in (lat.fop, lat.bop):
        for bad in (4, 7, -1):
            op.method = bad
            with pytest.raises(RuntimeError):
                L.run_one(op, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(lat.z.isnan().all()) and bool(lat.grads.isnan().all())
    # methods 2 and 3 validate like method 0: dt and substeps >= 1 are required
    for code in (2, 3):
        lat.fop.method = lat.bop.method = code
        for op in (lat.fop, lat.bop):
            op.substeps = 0
            with pytest.raises(RuntimeError):
                L.run_one(op, torch.cuda.current_stream().cuda_stream)
            op.substeps = 1
            dt, op.dt = op.dt, None
            with pytest.raises(RuntimeError):
                L.run_one(op, torch.cuda.current_stream().cuda_stream)
            op.dt = dt
    lat.fop.grid_dt = lat.dt.data_ptr()          # a grid without its emit arrays
    with pytest.raises(RuntimeError):
        L.run_one(lat.fop, torch.cuda.current_stream().cuda_stream)
    lat.bop.bstep_dt = lat.dt.data_ptr()         # step sizes without their offsets
    with pytest.raises(RuntimeError):
        L.run_one(lat.bop, torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the public classes
def _gen_pair(mnist, name, *, linear=True, step_size=None, seed=0):
    seed_all(seed)
    if mnist:
        gen = G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8, linear=linear)
        ref = M.Generator(1, 50, 0, 16, 16, ngf=8, mnist=True, ode_method=name)
    else:
        gen = G.VideoGenerator(3, 50, 0, 16, 16, dim_hidden=16, ngf=8, linear=linear)
        ref = M.Generator(3, 50, 0, 16, 16, dim_hidden=16, ngf=8, mnist=False, ode_method=name)
    if not linear:
        ref.linear = torch.nn.Identity()
    gen.ode_method = name
    if step_size is not None:
        gen.ode_step_size = step_size
        ref.ode_options = {"step_size": step_size}
    ref.load_state_dict({k: v.detach().clone() for k, v in gen.state_dict().items()})
    return gen.cuda(), ref


def _check_samples_and_gradients(gen, ref, nv=4, ni=4):
    """sample_videos(nv) and sample_images(ni) at the same seeds: frames, then every generator gradient."""
    seed_all(101)
    vid, _ = gen.sample_videos(nv)
    seed_all(102)
    img, _ = gen.sample_images(ni)
    seed_all(101)
    rvid, _ = ref.sample_videos(nv)
    seed_all(102)
    rimg, _ = ref.sample_images(ni)
    ev, ei = rel_err(vid.detach().cpu(), rvid.detach()), rel_err(img.detach().cpu(), rimg.detach())
    print("frames", ev, ei)
    assert vid.shape == rvid.shape and img.shape == rimg.shape and ev < TOL and ei < TOL
    rng = torch.Generator().manual_seed(3)
    wv, wi = torch.randn(vid.shape, generator=rng), torch.randn(img.shape, generator=rng)
    ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum()).backward()
    ((rvid * wv).sum() + (rimg * wi).sum()).backward()
    rp = dict(ref.named_parameters())
    for k, p in gen.named_parameters():
        if rp[k].grad is None:
            assert p.grad is None, k
            continue
        med, mx = robust_rel(p.grad.cpu(), rp[k].grad), rel_err(p.grad.cpu(), rp[k].grad)
        print(k, med, mx)
        assert med < 5e-3 and mx < 5e-2, (k, med, mx)
    return vid.detach()


@pytest.mark.parametrize("name", METHODS)
@pytest.mark.parametrize("mnist", [True, False], ids=["mnist-ode", "ucf64"])
def test_generators_against_the_oracle_generator(mnist, name):
    gen, ref = _gen_pair(mnist, name, seed=40)
    _check_samples_and_gradients(gen, ref)


@pytest.mark.parametrize("name", METHODS)
def test_generator_without_prenet(name):
    gen, ref = _gen_pair(True, name, linear=False, seed=41)
    assert not any(k.startswith("linear") for k in gen.state_dict())
    _check_samples_and_gradients(gen, ref)


@pytest.mark.parametrize("name", METHODS)
def test_generator_step_size_grid(name):
    gen, ref = _gen_pair(True, name, step_size=0.15, seed=42)
    vid = _check_samples_and_gradients(gen, ref)
    gen.ode_step_size = None                    # and it is a different solve from the default grid
    seed_all(101)
    with torch.no_grad():
        assert rel_err(gen.sample_videos(4)[0].cpu(), vid.cpu()) > 1e-6


@pytest.mark.parametrize("name", METHODS)
def test_categorical_generator(name):
    seed_all(43)
    gen = G.VideoGeneratorMNISTODE(1, 50, 3, 16, 16, ngf=8)
    gen.ode_method = name
    ref = R.Generator(1, 50, 3, 16, 16, dim_hidden=16, ngf=8, mnist=True, ode_method=name)
    ref.load_state_dict({k: v.detach().clone() for k, v in gen.state_dict().items()})
    gen.cuda()
    seed_all(31)
    vid, labels = gen.sample_videos(4)
    seed_all(32)
    img, _ = gen.sample_images(4)
    seed_all(31)
    rvid, rlabels = ref.sample_videos(4)
    seed_all(32)
    rimg, _ = ref.sample_images(4)
    assert labels.dtype == torch.int64 and torch.equal(labels.cpu(), rlabels)
    assert rel_err(vid.detach().cpu(), rvid.detach()) < TOL and rel_err(img.detach().cpu(), rimg.detach()) < TOL


@pytest.mark.parametrize("name", METHODS)
def test_sample_z_m_substeps_and_prefetched_latents(name):
    """sample_z_m against the oracle generator's; gen.ode_substeps = 2 against the refined-grid reference; and frames
    decoded from prefetch_latents bitwise those of the plain call."""
    gen, ref = _gen_pair(True, name, seed=44)
    seed_all(7)
    zm = gen.sample_z_m(5)
    seed_all(7)
    rzm = ref.sample_z_m(5)
    assert zm.shape == rzm.shape == (5 * 16, 16) and rel_err(zm.detach().cpu(), rzm.detach()) < STOL
    gen.ode_substeps = 2
    seed_all(7)
    zm2 = gen.sample_z_m(5)
    seed_all(7)
    x = ref.linear(torch.randn(5, 16)).double().detach()
    want, _, _ = _substep_oracle(copy.deepcopy(ref.ode_fn).double(), x, torch.linspace(0, 1, 16).float().double(), 2, name,
                                 torch.zeros(16, 5, 16, dtype=torch.float64))
    assert rel_err(zm2.detach().cpu(), want.transpose(0, 1).reshape(-1, 16)) < STOL
    assert rel_err(zm2.detach().cpu(), zm.detach().cpu()) > 1e-6
    gen.ode_substeps = 1
    with torch.no_grad():
        seed_all(8)
        v0, _ = gen.sample_videos(4)
        i0, _ = gen.sample_images(4)
        v0, i0 = v0.clone(), i0.clone()
        seed_all(8)
        gen.prefetch_latents([("videos", 4), ("images", 4)])
        v1, _ = gen.sample_videos(4)
        i1, _ = gen.sample_images(4)
    assert torch.equal(v0, v1) and torch.equal(i0, i1)


def test_switching_the_method_between_calls_gives_each_methods_own_result():
    gen, _ = _gen_pair(True, "rk4", seed=45)
    out = {}
    with torch.no_grad():
        for name in ("euler", "midpoint", "rk4", "euler", "midpoint"):
            gen.ode_method = name
            seed_all(9)
            v = gen.sample_videos(4, video_len=2)[0].clone()
            if name in out:
                assert torch.equal(out[name], v), name
            out[name] = v
    for name in ("euler", "midpoint"):
        ref = M.Generator(1, 50, 0, 16, 16, ngf=8, mnist=True, ode_method=name)
        ref.load_state_dict({k: v.detach().cpu().clone() for k, v in gen.state_dict().items()})
        seed_all(9)
        with torch.no_grad():
            want = ref.sample_videos(4, video_len=2)[0]
        assert rel_err(out[name].cpu(), want) < TOL, name
    d = rel_err(out["euler"].cpu(), out["midpoint"].cpu())
    print("euler vs midpoint frames at video_len=2:", d)
    assert d > 10 * TOL
    gen.ode_method = "bosh3"
    with pytest.raises(NotImplementedError, match="midpoint"):
        gen.sample_videos(4, video_len=2)


def _nets(name, seed, joint_ref=False):
    seed_all(seed)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    gen.ode_method = name
    refs = None
    if joint_ref:
        refs = M.build_mnist(ngf=8, ndf=8)
        refs[0].ode_method = name
        for m, o in zip((gen, dv, di), refs):
            o.load_state_dict(m.state_dict())
    for m in (gen, dv, di):
        m.cuda()
    return (gen, dv, di), refs


def _batches(n, B=4, seed=6):
    g = torch.Generator().manual_seed(seed)
    return [([torch.rand(B, 1, 28, 28, generator=g) for _ in range(2)], [torch.rand(B, 16, 1, 28, 28, generator=g) for _ in range(2)])
            for _ in range(n)]


@pytest.mark.parametrize("name", METHODS)
def test_trainer_step_against_the_oracle_train_step(name):
    """One GanTrainer.step at batch 4 (joint generator plan, adjoint into the gradient arena) against the oracle's
    train_step with the same method: losses at 1e-4, BatchNorm running statistics at 1e-4 (the acceptance of
    tests/test_gpu_modules.py::test_smallest_and_odd_batches_against_oracle)."""
    (gen, dv, di), (ogen, odv, odi) = _nets(name, 50, joint_ref=True)
    tr = G.GanTrainer(gen, dv, di)
    opts = M.make_optimizers(ogen, odv, odi)
    (imgs, vids), = _batches(1)
    seed_all(71)
    got = [float(v) for v in G.train_step(tr, [t.cuda() for t in imgs], [t.cuda() for t in vids])]
    seed_all(71)
    want = [float(v) for v in M.train_step(ogen, odv, odi, opts, imgs, vids)]
    assert np.allclose(got, want, rtol=1e-4, atol=0), (got, want)
    for (k, v), (_, w) in zip(gen.state_dict().items(), ogen.state_dict().items()):
        if "running_" in k:
            assert rel_err(v.cpu(), w) < 1e-4, k
        elif v.dtype == torch.int64:
            assert int(v) == int(w), k


@pytest.mark.parametrize("name", METHODS)
def test_graph_replayed_step_is_bitwise_the_eager_step(name):
    runs = []
    for graph in (True, False):
        (gen, dv, di), _ = _nets(name, 51)
        tr = G.GanTrainer(gen, dv, di, graph=graph)
        losses = []
        for it, (imgs, vids) in enumerate(_batches(4, seed=12)):
            seed_all(300 + it)
            losses.append([float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])])
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        runs.append((losses, [v.detach().clone() for m in (gen, dv, di) for v in m.state_dict().values()]))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_rk4_is_bitwise_itself_with_the_new_methods_unreachable(monkeypatch):
    """gen.ode_method = "rk4": frames and gradients of sample_videos / sample_images equal those of the same process with
    codes 2 and 3 refused by ode_method_code (so nothing of the rk4 path goes through the new ones)."""
    def run():
        gen, _ = _gen_pair(True, "rk4", seed=46)
        seed_all(11)
        vid, _ = gen.sample_videos(4)
        seed_all(12)
        img, _ = gen.sample_images(4)
        rng = torch.Generator().manual_seed(3)
        wv, wi = torch.randn(vid.shape, generator=rng), torch.randn(img.shape, generator=rng)
        ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum()).backward()
        return [vid.detach().clone(), img.detach().clone()] + [p.grad.clone() for p in gen.parameters() if p.grad is not None]

    base = run()
    code = L.ode_method_code

    def only_old(name):
        c = code(name)
        if c in (2, 3):
            raise AssertionError(f"new method code {c} reached on the rk4 path")
        return c

    monkeypatch.setattr(L, "ode_method_code", only_old)
    with pytest.raises(AssertionError):
        Mod.ode_method_code("euler")
    got = run()
    assert len(got) == len(base) and all(torch.equal(a, b) for a, b in zip(got, base))
