"""Host side of the one-layer right-hand side f(y) = tanh(W y + b) of models/mocogan_mnist.py: the ops' `rhs` field (no
size change, no new op kind, ABI version 105), its refusals before any launch, the ODEFuncTanh class and the drop-in
module (constructor rules, state-dict keys, same-seed initial weights in the reference's construction order) and the
plan's six-tensor, 2400-float gradient block.  No GPU."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd import modules as Mod

E_ARG = -1


def test_rhs_travels_in_the_former_pad_fields_and_no_struct_changes_size():
    lib = L.lib()
    assert lib.gode_version() == 105
    assert L.OdeFwdOp(rhs=1).rhs == 1 and L.OdeBwdOp(rhs=1).rhs == 1
    assert L.OdeFwdOp().rhs == 0 and L.OdeBwdOp().rhs == 0
    assert C.sizeof(L.OdeFwdOp) == lib.gode_sizeof(L.OP_ODE_FWD) and C.sizeof(L.OdeBwdOp) == lib.gode_sizeof(L.OP_ODE_BWD)
    assert (L.OP_ODE_FWD, L.OP_ODE_BWD) == (5, 6)
    # the field sits directly behind `method`, where the padding word was
    assert L.OdeFwdOp.rhs.offset == L.OdeFwdOp.method.offset + 4 and L.OdeFwdOp.rtol.offset == L.OdeFwdOp.rhs.offset + 4
    assert L.OdeBwdOp.rhs.offset == L.OdeBwdOp.method.offset + 4 and L.OdeBwdOp.rtol.offset == L.OdeBwdOp.rhs.offset + 4
    assert lib.gode_ode_bwd_work_size(33) == 3 * L.ODE_NPARAM          # rows keep their stride


def test_rhs_table():
    assert L.ODE_RHS == {"mlp": 0, "tanh": 1}
    assert L.ode_rhs_code("mlp") == 0 and L.ode_rhs_code("tanh") == 1
    assert L.ODE_RHS_TANH_NPARAM == 2400 and L.ODE_NPARAM == 2672


def _valid_ops(method=0):
    """ops that pass every argument check (pointers: non-null dummies, never dereferenced -- each call below is refused
    before any launch)"""
    fake = 0x1000
    p = L.OdeParams(*([fake] * 8))
    kw = dict(p=p, x=fake, sel_t=None, N=4, T=3, prenet=1, zcols=72, method=method)
    if method == 1:
        kw.update(rtol=1e-7, atol=1e-9, tout=fake)
    fop = L.OdeFwdOp(content=None, dt=fake, z=fake, traj=fake, substeps=1, **kw)
    bop = L.OdeBwdOp(traj=fake, dt=fake, gz=fake, work=fake, grads=fake, substeps=0 if method == 1 else 1, accumulate=0, **kw)
    return fop, bop


@pytest.mark.parametrize("method,rhs", [(0, 2), (0, -1), (2, 2), (3, -1), (1, 2), (1, -1), (1, 1)])
def test_single_entries_refuse_a_bad_rhs_before_any_launch(method, rhs):
    lib = L.lib()
    fop, bop = _valid_ops(method)
    fop.rhs = bop.rhs = rhs
    assert lib.gode_ode_fwd(C.byref(fop), None) == E_ARG
    assert lib.gode_ode_bwd(C.byref(bop), None) == E_ARG
    if method == 1:
        bop.substeps = 2          # a dopri5 forward with the fixed Kutta-3/8 adjoint: still method 1
        assert lib.gode_ode_bwd(C.byref(bop), None) == E_ARG


@pytest.mark.parametrize("rhs", [1, 2, -1])
def test_multi_entries_refuse_a_bad_rhs_before_any_launch(rhs):
    lib = L.lib()
    fop, bop = _valid_ops(1)
    fop.rhs = bop.rhs = rhs
    assert lib.gode_ode_fwd_multi(C.byref(fop), 1, None) == E_ARG
    assert lib.gode_ode_bwd_multi(C.byref(bop), 1, None) == E_ARG
    ok_f, ok_b = _valid_ops(1)                  # ... and as any op of an array
    farr, barr = (L.OdeFwdOp * 2)(ok_f, fop), (L.OdeBwdOp * 2)(ok_b, bop)
    assert lib.gode_ode_fwd_multi(farr, 2, None) == E_ARG
    assert lib.gode_ode_bwd_multi(barr, 2, None) == E_ARG


def test_rhs_1_requires_w1_and_b1():
    lib = L.lib()
    assert "rhs" in dict(L.OdeFwdOp._fields_) and "rhs" in dict(L.OdeBwdOp._fields_)     # (else `op.rhs = 1` sets nothing)
    for field in ("W1", "b1"):
        fop, bop = _valid_ops(0)
        fop.rhs = bop.rhs = 1
        fop.p.W2 = fop.p.b2 = bop.p.W2 = bop.p.b2 = None        # may be NULL ...
        setattr(fop.p, field, None)                             # ... these may not
        setattr(bop.p, field, None)
        assert lib.gode_ode_fwd(C.byref(fop), None) == E_ARG and lib.gode_ode_bwd(C.byref(bop), None) == E_ARG
    fop, bop = _valid_ops(0)                                    # rhs 0 still wants all four
    fop.p.W2 = bop.p.b2 = None
    assert lib.gode_ode_fwd(C.byref(fop), None) == E_ARG and lib.gode_ode_bwd(C.byref(bop), None) == E_ARG


# ---------------------------------------------------------------------------------------------------------------------
# classes
def test_one_layer_function_class():
    f = G.ODEFuncTanh(16)
    assert Mod.ODEFuncTanh is G.ODEFuncTanh
    assert [type(m) for m in f.fn] == [nn.Linear, nn.Tanh]
    assert list(f.state_dict()) == ["fn.0.weight", "fn.0.bias"]
    assert tuple(f.fn[0].weight.shape) == (16, 16) and tuple(f.fn[0].bias.shape) == (16,)
    assert list(f.forward.__code__.co_varnames[:3]) == ["self", "t", "x"]


def test_drop_in_module_gives_the_four_names():
    import models.mocogan_mnist as MM
    assert MM.ODEFunc is G.ODEFuncTanh
    assert issubclass(MM.VideoGenerator, G.VideoGenerator)
    assert issubclass(MM.VideoGeneratorMNIST, G.VideoGeneratorMNIST)
    assert issubclass(MM.VideoGeneratorMNISTODE, G.VideoGeneratorMNISTODE)      # (isinstance checks of the trainer keep working)
    assert (MM.VideoGenerator, MM.VideoGeneratorMNIST, MM.VideoGeneratorMNISTODE) == \
        (G.VideoGeneratorTanh, G.VideoGeneratorMNISTTanh, G.VideoGeneratorMNISTODETanh)


def _classes():
    import models.mocogan_mnist as MM
    return [(MM.VideoGenerator, 3), (MM.VideoGeneratorMNIST, 1), (MM.VideoGeneratorMNISTODE, 1)]


def test_one_layer_function_with_falsy_dim_hidden_is_served_on_all_three_classes():
    for cls, nc in _classes():
        for kw in ({}, {"dim_hidden": None}, {"dim_hidden": 0}):
            gen = cls(nc, 50, 0, 16, 16, ngf=8, **kw)
            assert isinstance(gen.ode_fn, G.ODEFuncTanh), (cls, kw)


def test_the_ucf_drivers_literal_call_constructs():
    import models.mocogan_mnist as MM
    gen = MM.VideoGenerator(3, 50, 0, 16, 16)
    assert isinstance(gen.ode_fn, G.ODEFuncTanh) and isinstance(gen, G.VideoGenerator) and not gen.mnist


def test_base_classes_serve_the_one_layer_function_when_it_is_passed():
    for cls, nc in ((G.VideoGenerator, 3), (G.VideoGeneratorMNIST, 1), (G.VideoGeneratorMNISTODE, 1)):
        gen = cls(nc, 50, 0, 16, 16, ode_fn=G.ODEFuncTanh, ngf=8)
        assert isinstance(gen.ode_fn, G.ODEFuncTanh)


def test_one_layer_function_with_a_truthy_dim_hidden_is_a_type_error():
    for cls, nc in _classes():
        with pytest.raises(TypeError, match="dim_hidden"):
            cls(nc, 50, 0, 16, 16, dim_hidden=16, ngf=8)
    with pytest.raises(TypeError, match="dim_hidden"):
        G.VideoGenerator(3, 50, 0, 16, 16, ode_fn=G.ODEFuncTanh, dim_hidden=16, ngf=8)


def test_two_layer_rules_stay():
    with pytest.raises(TypeError, match="dim_hidden"):
        G.VideoGenerator(3, 50, 0, 16, 16, ngf=8)                       # models/mocogan_ode.py's failure, mirrored
    gen = G.VideoGenerator(3, 50, 0, 16, 16, dim_hidden=16, ngf=8)
    assert isinstance(gen.ode_fn, G.ODEFunc) and len(list(gen.ode_fn.parameters())) == 4
    assert isinstance(G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8).ode_fn, G.ODEFunc)
    with pytest.raises(NotImplementedError):
        G.VideoGenerator(3, 50, 0, 16, 16, dim_hidden=32, ngf=8)
    import models.mocogan_mnist as MM                                   # the drop-in takes the two-layer class as the reference would
    gen = MM.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ode_fn=G.ODEFunc, dim_hidden=16, ngf=8)
    assert isinstance(gen.ode_fn, G.ODEFunc)


def test_latent_sizes_stay_refused():
    for cls, nc in _classes():
        with pytest.raises(NotImplementedError):
            cls(nc, 50, 0, 8, 16, ngf=8)
        with pytest.raises(NotImplementedError):
            cls(nc, 10, 0, 16, 16, ngf=8)


@pytest.mark.parametrize("cls", [G.VideoGeneratorMNISTODERNN, G.VideoGeneratorSDE, G.VideoGeneratorCDE, G.VideoGeneratorGRU],
                         ids=lambda c: c.__name__)
def test_other_motion_latents_refuse_the_one_layer_function(cls):
    with pytest.raises(NotImplementedError):
        cls(1, 50, 0, 16, 16, ode_fn=G.ODEFuncTanh, ngf=8)


def test_state_dict_keys_of_the_three_drop_in_classes():
    for cls, nc in _classes():
        keys = list(cls(nc, 50, 0, 16, 16, ngf=8).state_dict())
        assert [k for k in keys if k.startswith("ode_fn")] == ["ode_fn.fn.0.weight", "ode_fn.fn.0.bias"], cls
        assert [k for k in keys if k.startswith("linear")] == ["linear.0.weight", "linear.0.bias", "linear.2.weight", "linear.2.bias"]
        assert keys[:4] == ["recurrent.weight_ih", "recurrent.weight_hh", "recurrent.bias_ih", "recurrent.bias_hh"]
        assert not any(k.startswith("linear") for k in cls(nc, 50, 0, 16, 16, ngf=8, linear=False).state_dict())


# ---- the reference's constructor order (models/mocogan.py:185-215, models/mocogan_mnist.py:19-36, 56-93, 113-130) in plain torch
def _main(dim_z, ngf, nc, mnist):
    w = [dim_z, ngf * 8, ngf * 4, ngf * 2, ngf]
    seq = []
    for i in range(4):
        st, pd = (1, 0) if i == 0 else (2, 1)
        seq += [nn.ConvTranspose2d(w[i], w[i + 1], 4, st, pd, bias=False), nn.BatchNorm2d(w[i + 1]), nn.ReLU(True)]
    seq += [nn.ConvTranspose2d(ngf, nc, kernel_size=1, stride=1, padding=2, bias=False) if mnist
            else nn.ConvTranspose2d(ngf, nc, 4, 2, 1, bias=False), nn.Tanh()]
    return nn.Sequential(*seq)


def _one_layer(dim):
    m = nn.Module()
    m.fn = nn.Sequential(nn.Linear(dim, dim), nn.Tanh())
    return m


def _prenet(linear):
    return nn.Sequential(nn.Linear(16, 64), nn.LeakyReLU(0.2), nn.Linear(64, 16), nn.LeakyReLU(0.2)) if linear else nn.Identity()


def _reference_construction(kind, nc, ngf, linear):
    m = nn.Module()
    m.recurrent = nn.GRUCell(16, 16)                    # mocogan.VideoGenerator.__init__
    m.main = _main(66, ngf, nc, mnist=False)
    if kind == "ucf":
        m.ode_fn = _one_layer(16)
        m.linear = _prenet(linear)
        return m
    # VideoGeneratorMNIST.__init__ -- which VideoGeneratorMNISTODE calls with its defaults (one-layer function, linear=True)
    m.ode_fn = _one_layer(16)
    m.main = _main(66, ngf, nc, mnist=True)
    m.linear = _prenet(True if kind == "mnistode" else linear)
    if kind == "mnistode":
        m.ode_fn = _one_layer(16)
        m.linear = _prenet(linear)
    return m


@pytest.mark.parametrize("linear", [True, False], ids=["prenet", "noprenet"])
@pytest.mark.parametrize("kind", ["ucf", "mnist", "mnistode"])
def test_same_seed_gives_the_reference_constructions_initial_weights(kind, linear):
    import models.mocogan_mnist as MM
    cls, nc = {"ucf": (MM.VideoGenerator, 3), "mnist": (MM.VideoGeneratorMNIST, 1), "mnistode": (MM.VideoGeneratorMNISTODE, 1)}[kind]
    for seed in (0, 7):
        torch.manual_seed(seed)
        gen = cls(nc, 50, 0, 16, 16, ngf=8, linear=linear)
        torch.manual_seed(seed)
        want = _reference_construction(kind, nc, 8, linear).state_dict()
        got = gen.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (kind, seed, k)


# ---------------------------------------------------------------------------------------------------------------------
# the plan
def _bare_plan(gen):
    plan = object.__new__(Mod._GenPlan)
    plan.gen, plan._ode_ptrs = gen, None
    return plan


def test_plan_of_a_one_layer_generator_has_six_tensors_and_2400_floats():
    gen = G.VideoGeneratorMNISTODETanh(1, 50, 0, 16, 16, ngf=8)
    plan = _bare_plan(gen)
    ps = plan._params()
    want = [gen.linear[0].weight, gen.linear[0].bias, gen.linear[2].weight, gen.linear[2].bias,
            gen.ode_fn.fn[0].weight, gen.ode_fn.fn[0].bias]
    assert len(ps) == 6 and all(a is b for a, b in zip(ps, want))
    assert plan.rhs == 1 and plan.nparam == 2400
    assert list(plan.grad_offs) == [(0, 1024, (64, 16)), (1024, 64, (64,)), (1088, 1024, (16, 64)), (2112, 16, (16,)),
                                    (2128, 256, (16, 16)), (2384, 16, (16,))]
    assert sum(n for _, n, _ in plan.grad_offs) == 2400 == sum(p.numel() for p in ps)
    assert [p is q for p, q in zip(gen._arena_tail(), want)] == [True] * 6 and len(gen._arena_tail()) == 6
    nopre = G.VideoGeneratorMNISTODETanh(1, 50, 0, 16, 16, ngf=8, linear=False)
    ps = _bare_plan(nopre)._params()
    assert ps[:4] == (None,) * 4 and len(ps) == 6 and len(nopre._arena_tail()) == 2
    two = _bare_plan(G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8))          # the two-layer plan is what it was
    assert two.rhs == 0 and two.nparam == 2672 and len(two.grad_offs) == 8 and len(two._params()) == 8


def test_dopri5_on_a_one_layer_generator_is_refused_before_any_op_exists():
    gen = G.VideoGeneratorMNISTODETanh(1, 50, 0, 16, 16, ngf=8)
    gen.ode_method = "dopri5"
    plan = _bare_plan(gen)
    for _ in range(2):
        with pytest.raises(NotImplementedError) as e:
            plan._programs()
        assert all(repr(k) in str(e.value) for k in ("rk4", "euler", "midpoint"))
        assert plan._ode_ptrs is None and not hasattr(plan, "fwd_op") and not hasattr(plan, "bwd_op")
    gen.ode_method = "bosh3"                    # an unknown name is refused first, as on every generator
    with pytest.raises(NotImplementedError, match="bosh3"):
        plan._programs()
    assert plan._ode_ptrs is None and not hasattr(plan, "fwd_op")

