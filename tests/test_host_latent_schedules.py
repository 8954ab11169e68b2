"""CPU: the rows of tests/latent_sched_cases.py reach the schedules they are there for -- sde_grid_arrays gives every SDE row
its step count and outputs-per-step count, the float64 controller of tests/cde_ref.py gives every flagged CDE row an accepted
step that covers at least two output times -- and the float64 references the GPU file compares against are sound on them:
restate() finite with finite gradients, replay() on solve()'s own schedule equal to solve(), the ReLU-kink mask keeping more
than half of the trajectories."""
import pytest
import torch

import cde_ref as R
import latent_sched_cases as C
from cde_driver import KINK, params64
from sde_ref import _params, grads_of, restate

from gan_ode_amd.modules import sde_grid_arrays


@pytest.mark.parametrize("name", [r.name for r in C.SDE_ROWS])
def test_sde_row_schedule_is_the_one_stated(name):
    row = C.SDE_BY_NAME[name]
    grid = sde_grid_arrays(row.T, row.dt)
    per = C.sde_per_step(grid)
    assert grid["S"] == row.S and len(per) == row.S
    assert (max(per) if per else 0) == row.per_step
    assert sum(per) == row.T - 1                                   # every output belongs to exactly one step
    near0 = [j for j in range(1, row.T) if abs(float(grid["w1"][j])) < 1e-6]
    assert bool(near0) == row.w1_zero, near0
    if row.S:
        assert abs(float(grid["dt"].double().sum()) - 1.0) < 1e-6 and (grid["dt"] > 0).all()
    if row.name == "clamped-step":                                 # dt is clamped to the interval: one-step's schedule
        other = sde_grid_arrays(16, 1.0)
        for k in ("dt", "sqrt_dt", "emit_at", "w0", "w1"):
            assert torch.equal(grid[k], other[k]), k


def test_sde_rows_reach_every_count():
    assert {r.per_step for r in C.SDE_ROWS} >= {2, 4, 15}
    assert {r.S for r in C.SDE_ROWS} >= {0, 1}
    reached = set()
    for r in C.SDE_ROWS:
        reached |= set(C.sde_per_step(sde_grid_arrays(r.T, r.dt)))
    assert reached >= {1, 2, 4, 15}
    assert {r.N for r in C.SDE_ROWS} >= {1, 16, 17}
    assert any(r.content and r.zcols == 68 for r in C.SDE_ROWS) and any(not r.content and r.zcols == 16 for r in C.SDE_ROWS)
    assert all(r.N <= 33 for r in C.SDE_ROWS + C.CDE_ROWS)


@pytest.mark.parametrize("name,prenet", C.SDE_CASES)
def test_sde_row_float64_restatement_is_finite_with_finite_gradients(name, prenet):
    row = C.SDE_BY_NAME[name]
    grid, x, _, _, g = C.sde_inputs(row)
    P64 = [p.double().requires_grad_() for p in _params(prenet)]
    states, outs = restate(P64, x.double(), grid, prenet)
    assert states.shape == (row.N, row.S + 1, 16) and outs.shape == (row.N, row.T, 16)
    assert torch.isfinite(states).all() and torch.isfinite(outs).all()
    gup = torch.randn(outs.shape, generator=g, dtype=torch.float64)
    grads = grads_of((outs * gup).sum(), P64)
    assert all(torch.isfinite(t).all() for t in grads)
    if row.S == 0:
        assert all(float(t.abs().max()) == 0 for t in grads[-8:])       # no step: drift and diffusion are never evaluated
        if prenet:
            assert all(float(t.abs().max()) > 0 for t in grads[:4])
    else:
        assert all(float(t.abs().max()) > 0 for t in grads)


@pytest.fixture(scope="module")
def cde_params():
    return params64()


@pytest.mark.parametrize("name", [r.name for r in C.CDE_ROWS])
def test_cde_row_float64_controller_schedule_and_replay(name, cde_params):
    row = C.CDE_BY_NAME[name]
    x, _, _ = C.cde_inputs(row)
    sched = []
    with torch.no_grad():
        out, acc, trials = R.solve(cde_params, x, row.T, row.rtol, row.atol, sched=sched)
        st, sh = [t for t, _ in sched], [h for _, h in sched]
        assert len(sched) == acc and trials >= acc
        assert st[0] == 0.0 and st[-1] < row.T - 1 <= st[-1] + sh[-1]
        per = C.cde_per_step(st, sh, row.T)
        assert sum(per) == row.T - 1
        print(f"{name}: {acc} accepted / {trials} trials, outputs per step {per}, ends at {st[-1] + sh[-1]:.3f}")
        if row.multi:
            assert C.cde_covers_two(st, sh) and max(per) >= 2, per
        mg = {}
        # solve() reads the dense output off a float64 clock: the replay with the exact abscissa takes the same path
        outs, states, z0 = R.replay(cde_params, x, row.T, st, sh, margin=mg, round_abscissa=False)
    assert outs.shape == (row.N, row.T, 16) and states.shape == (row.N, acc + 1, 16)
    err = float((outs - out).abs().max() / out.abs().max())
    assert err <= 1e-9, err
    keep = (mg["relu"] > KINK).float().mean()
    assert float(keep) > 0.5, float(keep)


def test_cde_rows_stated_schedules(cde_params):
    """The schedules the case table quotes (float64 controller)."""
    want = {"three-per-step": [0, 2, 2, 3, 2, 2, 3, 1], "five-per-step": [0, 3, 5, 5, 2], "gap-then-two": [0, 1, 1, 0, 2],
            "all-in-one": [0, 2]}
    for name, per in want.items():
        row = C.CDE_BY_NAME[name]
        x, _, _ = C.cde_inputs(row)
        sched = []
        with torch.no_grad():
            R.solve(cde_params, x, row.T, row.rtol, row.atol, sched=sched)
        assert C.cde_per_step([t for t, _ in sched], [h for _, h in sched], row.T) == per, name
        if name == "five-per-step":
            assert sched[-1][0] + sched[-1][1] > row.T                 # stage times past the last knot
