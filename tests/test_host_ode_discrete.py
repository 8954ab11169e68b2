"""Host side of gen.ode_backprop = "discrete" (gode_ode_bwd_op.backprop = 1): the extended op struct,
gode_ode_bwd_steps_size, every argument refusal before any launch, the Python refusals, and the three reverse steps of
include/gode.h restated in float64 (tests/ode_discrete_ref.py) against autograd through oracle.ode_ref.odeint.  No GPU."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

import gan_ode_amd as G
import gan_ode_amd._lib as L
import ode_discrete_ref as D
from gan_ode_amd import modules as Mod
from oracle import mocogan_ref as M

E_ARG, RUN_E_ARG = -1, -1000          # GODE_E_ARG from an entry point, and as gode_run reports it for op 0


def test_extended_op_has_the_compiled_size_and_a_zeroed_op_is_the_adjoint():
    lib = L.lib()
    assert C.sizeof(L.OdeBwdOp) == lib.gode_sizeof(L.OP_ODE_BWD) == 240
    names = [n for n, _ in L.OdeBwdOp._fields_]
    assert names[-6:] == ["backprop", "G", "grid_dt", "emit_at", "emit_w", "ysteps"] and names[-7] == "sync"
    op = L.OdeBwdOp()
    assert op.backprop == 0 and op.G == 0 and not op.grid_dt and not op.emit_at and not op.emit_w and not op.ysteps
    assert Mod.ODE_BACKPROPS == {"adjoint": 0, "discrete": 1}


@pytest.mark.parametrize("N,T,substeps,G,want", [
    (32, 16, 1, 0, 0), (1, 1, 1, 0, 0), (5, 2, 0, 0, 0),                 # the grid is the output times: traj serves
    (32, 16, 4, 0, 32 * 60 * 16), (5, 2, 3, 0, 5 * 3 * 16), (7, 1, 3, 0, 0),
    (20, 4, 1, 9, 20 * 9 * 16), (33, 5, 3, 8, 33 * 8 * 16),              # a grid_dt grid: G steps, whatever substeps says
    (1 << 20, 16, 8, 0, (1 << 20) * 120 * 16),                            # past 2^31 floats
])
def test_steps_size(N, T, substeps, G, want):
    assert L.lib().gode_ode_bwd_steps_size(N, T, substeps, G) == want


def _complete_op(keep, **kw):
    """An op that passes every check of gode_ode_bwd (host memory stands in: a refused op launches nothing)."""
    buf = torch.zeros(4096)
    keep.append(buf)
    p = buf.data_ptr()
    op = L.OdeBwdOp(p=L.OdeParams(*[p] * 8), x=p, traj=p, dt=p, gz=p, work=p, grads=p, N=5, T=3, substeps=1, prenet=1,
                    accumulate=0, zcols=72)
    for k, v in kw.items():
        setattr(op, k, v)
    return op


def _refused_everywhere(op, multi=True):
    lib = L.lib()
    assert lib.gode_ode_bwd(C.byref(op), None) == E_ARG
    assert lib.gode_run((L.i32 * 1)(L.OP_ODE_BWD), (L.ptr * 1)(C.addressof(op)), 1, None) == RUN_E_ARG
    if multi:
        assert lib.gode_ode_bwd_multi(C.byref(op), 1, None) == E_ARG


def test_argument_refusals_come_before_any_launch():
    keep = []
    p = _complete_op(keep).traj
    for bad in (2, -1, 7):                                          # a backprop code other than 0 or 1
        _refused_everywhere(_complete_op(keep, backprop=bad))
    # discrete backprop through the adaptive solver's steps, with the adaptive adjoint's arguments or the fixed ones
    _refused_everywhere(_complete_op(keep, backprop=1, method=1, substeps=0, rtol=1e-7, atol=1e-9, tout=p))
    _refused_everywhere(_complete_op(keep, backprop=1, method=1, substeps=2))
    for method in (0, 2, 3):
        for rhs in (0, 1):
            # ysteps needed and NULL: substeps > 1, and a grid_dt grid
            _refused_everywhere(_complete_op(keep, backprop=1, method=method, rhs=rhs, substeps=3))
            _refused_everywhere(_complete_op(keep, backprop=1, method=method, rhs=rhs, G=4, grid_dt=p, emit_at=p, emit_w=p))
            # a grid without its emit arrays or its length
            _refused_everywhere(_complete_op(keep, backprop=1, method=method, rhs=rhs, G=4, grid_dt=p, ysteps=p))
            _refused_everywhere(_complete_op(keep, backprop=1, method=method, rhs=rhs, G=0, grid_dt=p, emit_at=p, emit_w=p,
                                             ysteps=p))
            # any discrete op inside gode_ode_bwd_multi, complete or not
            for kw in (dict(), dict(substeps=3, ysteps=p)):
                assert L.lib().gode_ode_bwd_multi(C.byref(_complete_op(keep, backprop=1, method=method, rhs=rhs, **kw)), 1,
                                                  None) == E_ARG
    # (an otherwise complete adaptive adjoint with backprop = 1 in a _multi call of two)
    ops = (L.OdeBwdOp * 2)(_complete_op(keep, method=1, substeps=0, rtol=1e-7, atol=1e-9, tout=p),
                           _complete_op(keep, backprop=1, method=1, substeps=0, rtol=1e-7, atol=1e-9, tout=p))
    assert L.lib().gode_ode_bwd_multi(ops, 2, None) == E_ARG


def _bare_plan(gen):
    plan = object.__new__(Mod._GenPlan)
    plan.gen, plan._ode_ptrs = gen, None
    return plan


def test_python_refusals():
    gen = G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8)
    assert gen.ode_backprop == "adjoint" and G.VideoGenerator.ode_backprop == "adjoint"
    assert Mod.ode_backprop_code(gen) == 0
    gen.ode_backprop = "discrete"
    for name in ("rk4", "euler", "midpoint"):
        gen.ode_method = name
        assert Mod.ode_backprop_code(gen) == 1
    gen.ode_method = "dopri5"
    for call in (lambda: gen.sample_videos(2), lambda: gen.sample_images(2), lambda: gen.sample_z_m(2),
                 lambda: gen.sample_pair(2, 2), lambda: gen.prefetch_latents([("videos", 2)]),
                 lambda: _bare_plan(gen)._programs()):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert all(repr(k) in str(e.value) for k in ("rk4", "euler", "midpoint"))
    gen.ode_method = "rk4"
    for bad in ("Discrete", "exact", "", None, 1):
        gen.ode_backprop = bad
        for call in (lambda: gen.sample_videos(2), lambda: gen.sample_z_m(2), lambda: _bare_plan(gen)._programs()):
            with pytest.raises(ValueError, match="discrete"):
                call()
    plan = _bare_plan(gen)
    with pytest.raises(ValueError):
        plan._programs()
    assert plan._ode_ptrs is None and not hasattr(plan, "bwd_op")


@pytest.mark.parametrize("cls,args", [
    (G.VideoGeneratorMNISTODERNN, dict()), (G.VideoGeneratorGRU, dict()), (G.VideoGeneratorSDE, dict()),
    (G.VideoGeneratorCDE, dict())], ids=["ode-rnn", "gru", "sde", "cde"])
def test_the_other_motion_latents_refuse_discrete(cls, args):
    try:
        gen = cls(1, 50, 0, 16, 16, ngf=8, **args)
    except TypeError:
        gen = cls(1, 50, 0, 16, 16, dim_hidden=16, ngf=8, **args)
    assert Mod.ode_backprop_code(gen) == 0                       # the default passes
    gen.ode_backprop = "discrete"
    for call in (lambda: gen.sample_videos(2), lambda: gen.sample_images(2), lambda: gen.sample_z_m(2)):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            call()
    gen.ode_backprop = "nonsense"
    with pytest.raises(ValueError):
        gen.sample_videos(2)


class OneLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fn = torch.nn.Sequential(torch.nn.Linear(16, 16), torch.nn.Tanh())

    def forward(self, t, x):
        return self.fn(x)


def _function(rhs, seed, scale):
    torch.manual_seed(seed)
    f = (OneLayer() if rhs else M.OdeRhs(16, 16)).double()
    with torch.no_grad():
        for p in f.parameters():
            p.mul_(scale)
    return f


GRIDS = [pytest.param(4, None, 1, id="T4"), pytest.param(2, None, 1, id="T2"), pytest.param(1, None, 1, id="T1-no-steps"),
         pytest.param(3, None, 3, id="T3-substeps3"),
         pytest.param(4, 0.13, 1, id="T4-stepsize0.13-interpolated-clamped"),
         pytest.param(5, 0.125, 1, id="T5-stepsize0.125-on-grid-points"),
         pytest.param(6, 0.3, 1, id="T6-stepsize0.3-steps-span-outputs")]


@pytest.mark.parametrize("T,step_size,substeps", GRIDS)
@pytest.mark.parametrize("rhs", [0, 1], ids=["two-layer", "one-layer"])
@pytest.mark.parametrize("method", D.METHODS)
def test_reverse_steps_equal_autograd_through_odeint(method, rhs, T, step_size, substeps):
    f = _function(rhs, 12, 3.0)
    gen = torch.Generator().manual_seed(5)
    y0 = torch.randn(5, 16, generator=gen, dtype=torch.float64)
    gout = torch.randn(T, 5, 16, generator=gen, dtype=torch.float64)
    tt = torch.linspace(0, 1, T).float().double()
    sol, gy, gth = D.autograd_reference(f, y0, tt, method, gout, step_size, substeps)
    my, mth = D.discrete_backprop(list(f.parameters()), method, y0, tt, gout, step_size, substeps)
    assert rel_err(my, gy) < 1e-12, rel_err(my, gy)
    for a, b in zip(mth, gth):
        if T == 1:
            assert float(a.abs().max()) == 0.0 == float(b.abs().max())
        else:
            assert rel_err(a, b) < 1e-12, rel_err(a, b)
    if step_size is not None:
        ws = [w for e in D.solver_grid(tt, step_size)[1] for _, w in e]
        assert len(ws) == T - 1
        if step_size == 0.13:
            assert all(0.0 < w < 1.0 for w in ws[:-1]) and ws[-1] == 1.0      # every output interpolated; last step clamped
        if step_size == 0.125:
            assert all(w in (0.0, 1.0) for w in ws)
