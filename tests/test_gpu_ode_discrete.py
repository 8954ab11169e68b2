"""GPU: discrete backprop through the fixed-grid motion-latent solve (gode_ode_bwd with backprop = 1;
gen.ode_backprop = "discrete").

The reference of every test is float64 autograd THROUGH oracle.ode_ref.odeint (tests/ode_discrete_ref.solve; substeps = k:
the same call per output interval on the k-fold refined grid), the pre-net in front, loss (z * w).sum() with a random w.
Tolerances are those of the fixed-grid kernels (tests/test_gpu_ode_methods.py): gradients GTOL = 2e-4 per tensor block with
conftest.rel_err.  The op-level objects are that file's FixedLatent and tests/test_gpu_ode_rhs.py's TanhLatent with the
backward op switched to backprop = 1: NaN-filled grads (the pre-net block without a pre-net and floats [2400, 2672) with
rhs = 1 must stay NaN), and NaN sentinels behind grads, work and ysteps."""
import copy

import pytest
import torch

from conftest import rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
import ode_discrete_ref as D
from oracle import mocogan_ref as M
from oracle import ode_ref
from test_gpu_latent_paths import BLOCKS, NAN, NP, OFF_W1, identical, stream
from test_gpu_ode_methods import FIXED, GTOL, STOL, FixedLatent, _gen_pair
from test_gpu_ode_rhs import TanhLatent, _one_layer_pair

pytestmark = pytest.mark.gpu

ALL = [pytest.param(n, id=n) for n in FIXED]
RHS = [pytest.param(0, id="two-layer"), pytest.param(1, id="one-layer")]


class _Discrete:
    """Mixin over FixedLatent / TanhLatent: the backward op asks for discrete backprop on the forward op's grid, and the
    oracle is autograd through odeint (adjoint=True: odeint_adjoint, what backprop = 0 is tested against)."""

    def make_discrete(self):
        lib = L.lib()
        self.bop.backprop = 1
        if self.step_size is not None:
            self.bop.G = self.fop.G
            self.bop.grid_dt, self.bop.emit_at, self.bop.emit_w = self.fop.grid_dt, self.fop.emit_at, self.fop.emit_w
        self.ny = lib.gode_ode_bwd_steps_size(self.N, self.T, self.substeps, self.bop.G)
        self.ysteps = torch.full((self.ny + 16,), NAN, device="cuda")
        self.bop.ysteps = self.ysteps.data_ptr() if self.ny else None
        self.nwork = lib.gode_ode_bwd_work_size(self.N)
        self.work = torch.full((self.nwork + 16,), NAN, device="cuda")
        self.bop.work = self.work.data_ptr()
        return self

    def scale_function(self, s):
        """ODEFunc parameters x s, on the host copy and on the device copy (the same fp32 product on both)."""
        with torch.no_grad():
            for p in self.f.parameters():
                p.mul_(s)
            for p in (self.P1 if getattr(self, "rhs", 0) else self.P[-4:]):
                p.mul_(s)
        return self

    def force_sel(self, picks):
        """Trajectory n selects time picks[n] (sel_t, its device copy and the rows of gz, in place)."""
        for n, t in picks.items():
            self.sel[n] = t
        self.seld.copy_(self.sel)
        self.gz[:, :16] = self.gup[torch.arange(self.N), self.sel.long()].cuda()
        return self

    def _pieces(self):
        f = copy.deepcopy(self.f).double()
        pre = copy.deepcopy(self.pre).double() if self.prenet else None
        w = self.gup.double()
        if self.sel is not None:
            w = w * (torch.arange(self.T)[None, :] == self.sel.long()[:, None]).double()[:, :, None]
        return f, pre, w, self.tt.double()

    def oracle(self, name=None, adjoint=False):
        name = name or self.name
        f, pre, w, tt = self._pieces()
        x = self.x.double()
        y0 = pre(x) if pre is not None else x.requires_grad_(True)
        z = D.solve(f, y0, tt, name, self.step_size, self.substeps, adjoint).transpose(0, 1)
        (z * w).sum().backward()
        params = (list(pre.parameters()) if pre is not None else []) + list(f.parameters())
        g = torch.zeros(NP, dtype=torch.float64)
        for (_, o, n), p in zip(BLOCKS if pre is not None else BLOCKS[4:], params):
            if p.grad is not None:                # (T = 1: the function is never called)
                g[o:o + n] = p.grad.reshape(-1)
        return z.detach(), g, None

    def adjoint_gap(self, name):
        """On the float64 oracle alone: how far odeint_adjoint's gradient lies from autograd through odeint -- y0's gradient
        and the ODEFunc gradients concatenated, conftest.rel_err."""
        f, pre, w, tt = self._pieces()
        x = self.x.double()
        y0 = (pre(x) if pre is not None else x).detach()
        got = []
        for adjoint in (True, False):
            _, gy, gth = D.autograd_reference(f, y0, tt, name, w.transpose(0, 1), self.step_size, self.substeps, adjoint)
            got.append(torch.cat([gy.reshape(-1)] + [g.reshape(-1) for g in gth]))
        return rel_err(got[0], got[1])

    def check_sentinels(self):
        assert bool(self.work[self.nwork:].isnan().all()), "written behind work"
        assert bool(self.ysteps[self.ny:].isnan().all()), "written behind ysteps"
        assert bool(self.grads[NP:].isnan().all()), "written behind grads"
        if self.ny:
            assert not bool(self.ysteps[:self.ny].isnan().any()), "a step-start state was not stored"

    def run_discrete(self):
        out = self.run_all()             # forward against the oracle; backward: oracle, bitwise repeat, accumulate doubles
        self.check_sentinels()
        return out


class DiscreteLatent(_Discrete, FixedLatent):
    pass


class DiscreteTanhLatent(_Discrete, TanhLatent):
    pass


def make(rhs, N, T, seed, prenet, name, **kw):
    return (DiscreteTanhLatent if rhs else DiscreteLatent)(N, T, seed, prenet, name, **kw).make_discrete()


# ---------------------------------------------------------------------------------------------------------------------
# 1. told apart from the adjoint
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("T,prenet", [pytest.param(2, True, id="T2-prenet"), pytest.param(3, False, id="T3-noprenet")])
def test_discrete_gradient_is_told_apart_from_the_adjoint(name, rhs, T, prenet):
    """N = 5, seed 12, ODEFunc parameters x 3: the continuous adjoint's gradient lies >= 10 x GTOL from the gradient of the
    computed solve (asserted on the float64 oracle alone; DESIGN section 29's table: 5.8e-3 .. 7.3e-1 at T = 3, more at
    T = 2), so a kernel that ran the adjoint would miss GTOL by at least its ninefold."""
    lat = make(rhs, 5, T, 12, prenet, name, content=True).scale_function(3.0)
    gap = lat.adjoint_gap(name)
    print(f"{name} rhs {rhs} T {T}: adjoint vs discrete on the oracle {gap:.3g}")
    assert gap >= 10 * GTOL, gap
    _, ga, _ = lat.oracle(adjoint=True)
    zref, gref, _ = lat.oracle()
    print("   ODEFunc block, adjoint oracle vs discrete oracle:", rel_err(ga[OFF_W1:], gref[OFF_W1:]))
    lat.run_discrete()


# ---------------------------------------------------------------------------------------------------------------------
# 2. launch shapes
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("N", [1, 5, 16, 17, 33])
def test_launch_shapes(name, N, T):
    """N: a partial row and wave, exactly one workgroup, one trajectory spilling into a second, three workgroups through
    the reduce; T = 1 has no interval, only the pre-net gradient.  Default-initialised nets; the right-hand side, the
    pre-net and sel_t alternate over the cases."""
    rhs, prenet, sel = (N + T) % 2, T == 1 or N % 3 != 2, N in (16, 33)
    lat = make(rhs, N, T, 5000 + N + T, prenet, name, sel=sel, content=bool(N % 2), zcols=68 if N % 2 else 96)
    zref, gref = lat.run_discrete()
    assert lat.ny == 0
    if T == 1:
        end = 2400 if rhs else NP
        assert float(gref[OFF_W1:].abs().max()) == 0.0 and float(lat.grads[OFF_W1:end].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. grid modes
GRIDS = [pytest.param(4, 3, None, id="T4-substeps3"),
         pytest.param(4, 1, 0.13, id="T4-stepsize0.13-interpolated-last-step-clamped"),
         pytest.param(5, 1, 0.125, id="T5-stepsize0.125-outputs-on-grid-points")]


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("rhs", RHS)
@pytest.mark.parametrize("T,substeps,step_size", GRIDS)
def test_grid_modes(name, rhs, T, substeps, step_size):
    lat = make(rhs, 20, T, 6000 + T, bool(rhs), name, sel=not rhs, substeps=substeps, step_size=step_size)
    if step_size is not None:
        w = lat.grid["emit_w"].cpu()[1:]
        if step_size == 0.13:       # 8 steps, the last one clamped to t = 1; every output but the last interpolated
            assert lat.grid["G"] == 8 and bool(((w[:-1] > 0) & (w[:-1] < 1)).all()) and float(w[-1]) == 1.0
            assert float(lat.grid["grid_dt"][-1]) < 0.1
        else:
            assert lat.grid["G"] == 8 and bool(((w == 0) | (w == 1)).all())
        assert lat.ny == 20 * lat.grid["G"] * 16
    else:
        assert lat.ny == 20 * (T - 1) * substeps * 16
    lat.run_discrete()


# ---------------------------------------------------------------------------------------------------------------------
# 4. contracts
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("T,substeps,step_size", [pytest.param(6, 1, None, id="output-grid")] + GRIDS)
def test_selected_times_including_the_first_and_the_last(name, T, substeps, step_size):
    """sel_t: a trajectory sees only its selected time -- among them time 0 (no step carries a gradient: the pre-net alone)
    and time T-1."""
    lat = make(0, 17, T, 7000 + T, True, name, sel=True, substeps=substeps, step_size=step_size)
    lat.force_sel({0: 0, 1: T - 1, 16: 0, 15: T - 1, 2: 1})
    lat.run_discrete()


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("rhs", RHS)
def test_accumulate_adds_onto_a_known_vector_and_untouched_floats_stay(name, rhs):
    """prenet = 0: the first 2128 floats of grads are neither read nor written; rhs = 1: floats [2400, 2672) neither;
    accumulate = 1 adds the gradient onto what grads held; two runs are bit-identical (run_discrete's checks too)."""
    lat = make(rhs, 17, 3, 8000, False, name, substeps=2)
    zref, gref = lat.run_discrete()
    end = 2400 if rhs else NP
    lat.bwd(0)
    g1 = lat.grads.clone()
    assert bool(g1[:OFF_W1].isnan().all()) and bool(g1[end:].isnan().all()) and not bool(g1[OFF_W1:end].isnan().any())
    known = torch.linspace(-3, 5, NP + 16, device="cuda")
    known[:OFF_W1] = NAN
    known[end:] = NAN
    lat.grads.copy_(known)
    lat.bwd(1)
    got = lat.grads.clone()
    assert bool(got[:OFF_W1].isnan().all()) and bool(got[end:].isnan().all())
    assert torch.equal(got[OFF_W1:end], known[OFF_W1:end] + g1[OFF_W1:end])
    lat.grads.copy_(known)
    lat.bwd(1)
    assert identical(lat.grads, got)
    lat.check_sentinels()


def test_discrete_stays_on_the_valu_kernel_and_the_adjoint_is_what_it_was():
    """The same object with backprop = 0 still passes against odeint_adjoint (its own grid arguments: bstep_off / bstep_dt),
    and its result differs from the discrete one."""
    lat = make(0, 20, 4, 9000, True, "euler", step_size=0.13)
    zref, gd = lat.run_discrete()
    g_discrete = lat.grads.clone()
    lat.bop.backprop = 0
    lat.reset()
    lat.ysteps.fill_(NAN)
    lat.fwd()
    _, ga, _ = lat.oracle(adjoint=True)
    lat.bwd(0)
    lat.check_grads(ga, GTOL)
    assert rel_err(lat.grads[OFF_W1:NP].cpu(), g_discrete[OFF_W1:NP].cpu()) > 10 * GTOL
    assert bool(lat.ysteps.isnan().all())          # the adjoint does not touch the scratch


# ---------------------------------------------------------------------------------------------------------------------
# 5. modules
def _odeint_for_adjoint(monkeypatch):
    """oracle.ode_ref.odeint_adjoint -> odeint (autograd through the steps), for the reference generator of one test."""
    monkeypatch.setattr(ode_ref, "odeint_adjoint",
                        lambda func, y0, t, *, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint_params=None:
                        ode_ref.odeint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options))


def _pair(one_layer, seed):
    gen, ref = (_one_layer_pair if one_layer else _gen_pair)(True, "euler", seed=seed)
    return gen, ref.double()


def _kink_margin(ref, n):
    """On the float64 reference alone: how close sample_videos(n)'s forward (seed 101) comes to a ReLU / LeakyReLU kink --
    the smallest |pre-activation| over its layer's largest, of every rectifier of the generator (pre-net and decoder)."""
    seen = []
    hooks = [m.register_forward_pre_hook(lambda m, i: seen.append(float((i[0].detach().abs() / i[0].detach().abs().max()).min())))
             for m in ref.modules() if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU))]
    seed_all(101)
    with torch.no_grad():
        ref.sample_videos(n)
    for h in hooks:
        h.remove()
    return min(seen)


# The weights' seed of the generator test, per variant: of seeds 60-71 the one whose float64 reference forward stays farthest
# from a rectifier kink (_kink_margin: 1.05e-6 and 8.4e-7; the others 3e-9 .. 8.7e-7), chosen on the oracle alone.
KINK_FREE_SEED = {False: 67, True: 61}


def _latent_grads(net):
    return {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()
            if k.startswith(("linear.", "ode_fn.")) and p.grad is not None}


@pytest.mark.parametrize("one_layer", [False, True], ids=["mnist-ode", "mnist-ode-tanh"])
def test_generator_frames_are_bitwise_and_latent_gradients_are_the_discrete_ones(one_layer, monkeypatch):
    """VideoGeneratorMNISTODE[Tanh](1, 50, 0, 16, 16, ngf=8), euler, batch 3: frames bit-identical under both settings of
    ode_backprop; with "discrete" the latent-parameter gradients against the float64 copy of the oracle generator whose
    odeint_adjoint is odeint (same weights, same draws); and the two settings' gradients differ.

    The gradients reach the latent through the train-mode decoder: 737,520 rectified activations at this size, and a
    pre-activation that fp32 rounding carries across zero changes every latent gradient by a discrete amount that is no
    property of the latent kernel.  Measured with "discrete" over weight seeds 60-63 of both variants: 4e-7 .. 1.2e-6 on
    seven of the eight, and 5.5e-4 .. 1.0e-3 on the two-layer seed 60 -- against the float64 AND against the fp32 reference,
    3.6e-7 on the same seed in eval mode -- where the float64 forward has two pre-activations 7.7e-8 and 9.6e-8 of their
    layer's maximum from zero, below fp32's resolution of such a sum.  So the weights' seed is the one of 60-71 whose
    reference forward stays farthest from every kink (KINK_FREE_SEED), and the margin is asserted before any kernel runs."""
    gen, ref = _pair(one_layer, KINK_FREE_SEED[one_layer])
    margin = _kink_margin(ref, 3)
    print("nearest rectifier kink of the reference forward:", margin)
    assert margin >= 8e-7, margin          # >= 13 x fp32's epsilon of the layer's largest pre-activation
    rng = torch.Generator().manual_seed(3)
    out = {}
    for mode in ("adjoint", "discrete", "adjoint", "discrete"):       # (switching back and forth takes effect: _ode_ptrs key)
        gen.ode_backprop = mode
        gen.zero_grad()
        seed_all(101)
        vid, _ = gen.sample_videos(3)
        if "w" not in out:
            out["w"] = torch.randn(vid.shape, generator=rng)
        (vid * out["w"].cuda()).sum().backward()
        got = (vid.detach().clone(), _latent_grads(gen))
        if mode in out:
            assert torch.equal(out[mode][0], got[0]) and all(torch.equal(got[1][k], v) for k, v in out[mode][1].items()), mode
        out[mode] = got
    assert torch.equal(out["adjoint"][0], out["discrete"][0])
    _odeint_for_adjoint(monkeypatch)
    seed_all(101)
    rvid, _ = ref.sample_videos(3)
    assert rel_err(out["discrete"][0].cpu(), rvid.detach()) < 1e-4
    (rvid * out["w"].double()).sum().backward()
    want = _latent_grads(ref)
    assert set(want) == set(out["discrete"][1]) and len(want) == (6 if one_layer else 8)
    for k, w in want.items():
        e, ea = rel_err(out["discrete"][1][k], w), rel_err(out["adjoint"][1][k], w)
        print(k, "discrete", e, "adjoint", ea)
    for k, w in want.items():
        assert rel_err(out["discrete"][1][k], w) < GTOL, (k, rel_err(out["discrete"][1][k], w))
    far = max(rel_err(out["adjoint"][1][k], w) for k, w in want.items() if k.startswith("ode_fn."))
    assert far > GTOL, far              # (euler at T = 16: the adjoint is percents away)


@pytest.mark.parametrize("one_layer", [False, True], ids=["mnist-ode", "mnist-ode-tanh"])
def test_sample_z_m_under_autograd(one_layer, monkeypatch):
    """sample_z_m's _LatentFn picks the mode up through the plan's bwd_op."""
    gen, ref = _pair(one_layer, 61)
    gen.ode_backprop = "discrete"
    seed_all(7)
    zm = gen.sample_z_m(3)
    w = torch.randn(zm.shape, generator=torch.Generator().manual_seed(4))
    (zm * w.cuda()).sum().backward()
    _odeint_for_adjoint(monkeypatch)
    seed_all(7)
    rzm = ref.sample_z_m(3)
    assert rel_err(zm.detach().cpu(), rzm.detach()) < STOL
    (rzm * w.double()).sum().backward()
    got, want = _latent_grads(gen), _latent_grads(ref)
    assert set(got) == set(want)
    for k, v in want.items():
        print(k, rel_err(got[k], v))
        assert rel_err(got[k], v) < GTOL, (k, rel_err(got[k], v))
    gen.ode_substeps = 2                          # a forward re-run through ysteps, sized for this setting
    gen.zero_grad()
    seed_all(7)
    zm2 = gen.sample_z_m(3)
    (zm2 * w.cuda()).sum().backward()
    f = copy.deepcopy(ref.ode_fn)
    seed_all(7)
    x = torch.randn(3, 16).double()
    pre = copy.deepcopy(ref.linear)
    sol = D.solve(f, pre(x), torch.linspace(0, 1, 16).float().double(), "euler", substeps=2)
    (sol.transpose(0, 1).reshape(-1, 16) * w.double()).sum().backward()
    assert rel_err(zm2.detach().cpu(), sol.detach().transpose(0, 1).reshape(-1, 16)) < STOL
    got = _latent_grads(gen)
    for prefix, net in (("linear.", pre), ("ode_fn.", f)):
        for k, p in net.named_parameters():
            assert rel_err(got[prefix + k], p.grad) < GTOL, (prefix + k, rel_err(got[prefix + k], p.grad))


def _trainer_run(direct, graph=False, steps=1):
    seed_all(91)
    gen = G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8)
    gen.ode_method, gen.ode_backprop = "euler", "discrete"
    dv, di = G.VideoDiscriminator(1, ksize=2, ndf=8), G.PatchImageDiscriminator(1, ndf=8)
    for m in (gen, dv, di):
        m.cuda()
    tr = G.GanTrainer(gen, dv, di, direct_grads=direct, graph=graph)
    rng = torch.Generator().manual_seed(5)
    losses = []
    for it in range(steps):
        imgs = [torch.rand(4, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        vids = [torch.rand(4, 16, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
        seed_all(92 + it)
        losses.append([float(v) for v in tr.step(imgs, vids)])
    torch.cuda.synchronize()
    subs = [sub for plans in gen._pool.plans.values() for plan in plans
            for sub in (plan.subplans() if hasattr(plan, "subplans") else (plan,))]
    assert subs and all(sub.bwd_op.backprop == 1 for sub in subs)
    return (losses, [p.detach().clone() for m in (gen, dv, di) for p in m.parameters()],
            [None if p.grad is None else p.grad.clone() for p in gen.parameters()])


def _same_runs(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    assert all((x is None) == (y is None) and (x is None or torch.equal(x, y)) for x, y in zip(a[2], b[2]))


def test_trainer_step_direct_grads_is_bitwise_the_stock_path():
    """One GanTrainer step with the discrete latent backward writing into the gradient arena against direct_grads=False."""
    _same_runs(_trainer_run(True), _trainer_run(False))


def test_graph_replayed_steps_are_bitwise_the_eager_steps():
    _same_runs(_trainer_run(True, graph=True, steps=3), _trainer_run(True, graph=False, steps=3))
