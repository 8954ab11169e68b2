"""Host side of gen.ode_method = "euler" / "midpoint": the method table, the refusal of anything else, the op structs (no
size changes, no new op kind, ABI version 105) and the method-independent solver grid.  No GPU."""
import ctypes as C
import types

import pytest
import torch

import gan_ode_amd._lib as L
from gan_ode_amd import modules as Mod


def test_method_table_and_codes():
    assert L.ODE_METHODS == {"rk4": 0, "dopri5": 1, "euler": 2, "midpoint": 3}
    assert Mod.ODE_METHODS == L.ODE_METHODS
    for name, code in L.ODE_METHODS.items():
        assert L.ode_method_code(name) == code and Mod.ode_method_code(name) == code


@pytest.mark.parametrize("name", ["bosh3", "adaptive_heun", "dopri8", "RK4", "", None, 2])
def test_unknown_method_is_refused_naming_the_served_ones(name):
    for fn in (L.ode_method_code, Mod.ode_method_code):
        with pytest.raises(NotImplementedError) as e:
            fn(name)
        assert all(repr(k) in str(e.value) for k in ("rk4", "dopri5", "euler", "midpoint"))


def test_plan_refuses_an_unknown_method_before_it_builds_any_op():
    """_GenPlan._programs asks ode_method_code first: nothing of the plan is touched, and asking again refuses again."""
    gen = types.SimpleNamespace(ode_method="bosh3", ode_step_size=None, ode_rtol=1e-7, ode_atol=1e-9, ode_substeps=1)
    plan = object.__new__(Mod._GenPlan)
    plan.gen, plan._ode_ptrs = gen, None
    plan._params = lambda: (None,) * 8
    for _ in range(2):
        with pytest.raises(NotImplementedError, match="bosh3"):
            plan._programs()
        assert plan._ode_ptrs is None and not hasattr(plan, "fwd_op")


def test_op_structs_keep_their_size_and_the_abi_its_version():
    lib = L.lib()
    assert lib.gode_version() == 105
    assert C.sizeof(L.OdeFwdOp) == lib.gode_sizeof(L.OP_ODE_FWD)
    assert C.sizeof(L.OdeBwdOp) == lib.gode_sizeof(L.OP_ODE_BWD)
    assert (L.OP_ODE_FWD, L.OP_ODE_BWD) == (5, 6)
    for op in (L.OdeFwdOp(method=3), L.OdeBwdOp(method=2)):       # the codes travel in the existing field
        assert op.method in (2, 3)


@pytest.mark.parametrize("T,step_size", [(6, 0.15), (6, 0.3), (16, 0.05), (3, 0.4)])
def test_solver_grid_does_not_depend_on_the_method(T, step_size):
    """The plan's grid for gen.ode_step_size comes from solver_grid_arrays(T, step_size) alone: the same arrays whichever
    fixed-grid method the generator names."""
    want = Mod.solver_grid_arrays(T, step_size)
    for name in ("rk4", "euler", "midpoint"):
        plan = object.__new__(Mod._GenPlan)
        plan.T, plan.device = T, torch.device("cpu")
        plan.gen = types.SimpleNamespace(ode_method=name, ode_step_size=step_size)
        got = plan._solver_grid(step_size)
        assert set(got) == set(want) == {"G", "grid_dt", "emit_at", "emit_w", "bstep_off", "bstep_dt"}
        for k, v in want.items():
            assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, (name, k)
    assert float(want["grid_dt"].sum()) == pytest.approx(1.0, abs=1e-6) and want["G"] == len(want["grid_dt"])
