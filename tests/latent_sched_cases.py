"""Step schedules of the SDE and CDE motion latents in which one step carries several outputs, as plain data: one row per
schedule, each at the smallest shapes that reach it, with the property it must reach.  Both forward kernels emit outputs in
a `while` loop inside the step loop (sde_fwd_kernel: `while (jo < T && emit_at[jo] == k)`; cde_fwd_kernel: `while (jo < T &&
jo <= t1)`) and both backward kernels fold them back in with matching loops (sde_bwd_kernel: the `jhi` / `jlo` loops;
cde_bwd_kernel: `while (jhi >= 1 && jhi > t0)`); at the reference's settings (sde_dt = 2.5e-2; rtol 1e-4, atol 1e-6) every
such loop body runs at most once per step.  Shared by tests/test_host_latent_schedules.py (every row's schedule, from
sde_grid_arrays and the float64 controller of tests/cde_ref.py, has the stated property) and
tests/test_gpu_latent_schedules.py (every row runs on the GPU against the float64 restatements, and asserts the property
again on the schedule the kernels ran on).

What each loop would do as an `if`, and the smallest row that then fails:
* sde_fwd_kernel's emit loop: jo advances once per step, so from the first step with two outputs on every output is written
  late or never and keeps its NaN sentinel -- two-per-step (step 2 emits outputs 3 and 4), every row with S > 0.
* sde_bwd_kernel's jhi / jlo loops: only one w1 share and one w0 share per state enter the adjoint, the others are folded in
  at later (wrong) states or dropped -- two-per-step; the jlo loop after the step loop is held by one-step, whose 15 w0 shares
  all belong to state 0.
* cde_fwd_kernel's dense-output loop: one output per accepted step, so the solve goes on past T - 1 until the last output is
  out and reads the outputs off the wrong steps -- all-in-one (2 outputs, 2 steps on the device), three-per-step.
* cde_bwd_kernel's fold loop: only the last output of a step enters gy0 / gy1 / gym / gk1 / gk7, the others are charged to
  earlier steps' interpolants -- all-in-one, three-per-step."""
import collections

import torch

# ---- SDE: gode_sde_fwd / gode_sde_bwd on sde_grid_arrays(T, dt) -------------------------------------------------------
# prenet: the pre-net settings the row runs with.  content: a content code is given (else content NULL: the kernel writes
# the 16 motion columns only).  sel: the row runs once with all rows and once with sel_t.  S, per_step: the step count and
# the largest number of outputs one step produces; w1_zero: some output's w1 is within 1e-6 of 0 (the fp32 time sum stops
# just short of an output time, so the next step starts ~1e-7 before it and the output sits at that step's very start).
SdeRow = collections.namedtuple("SdeRow", "name N T dt prenet content zcols sel S per_step w1_zero reaches")
BOTH = (True, False)

SDE_ROWS = [
    SdeRow("two-per-step", 17, 16, 0.1, BOTH, True, 96, True, 10, 2, True,
           "some step emits 2 outputs; a second workgroup of one trajectory; outputs with w1 ~ 0"),
    SdeRow("four-per-step", 33, 16, 0.2, BOTH, True, 96, True, 5, 4, True, "4 outputs in a step; three workgroups; outputs with w1 ~ 0"),
    SdeRow("one-step", 5, 16, 1.0, BOTH, True, 72, True, 1, 15, False,
           "all 15 outputs in the only step: the backward folds every w0 share in after the step loop, at state 0"),
    SdeRow("clamped-step", 16, 16, 2.0, BOTH, True, 96, True, 1, 15, False,
           "dt larger than the interval, clamped to it: the schedule of one-step; exactly one full workgroup"),
    SdeRow("no-steps", 9, 1, 2.5e-2, BOTH, True, 68, True, 0, 0, False,
           "T = 1, S = 0: no step, no schedule read; the output is the pre-net's"),
    SdeRow("single", 1, 16, 0.2, BOTH, True, 80, True, 5, 4, True, "N = 1: one trajectory, 15 idle rows in the workgroup"),
    SdeRow("min-zcols", 17, 16, 0.1, BOTH, True, 68, True, 10, 2, True, "a content code at zcols = 68, the accepted minimum"),
    SdeRow("no-content", 17, 16, 0.2, BOTH, False, 16, True, 5, 4, True,
           "content NULL, zcols = 16: rows of the 16 motion columns alone, forward and backward"),
]
SDE_BY_NAME = {r.name: r for r in SDE_ROWS}
SDE_CASES = [(r.name, p) for r in SDE_ROWS for p in r.prenet]


def sde_per_step(grid):
    """outputs per step of a sde_grid_arrays schedule: a list of S counts"""
    counts = [0] * grid["S"]
    for k in grid["emit_at"].tolist()[1:]:
        counts[k] += 1
    return counts


def sde_inputs(row):
    """the row's host inputs: x [1 + S, N, 16] (x0, xi), content [N, 50], sel [N] int32, and the generator they came from"""
    from gan_ode_amd.modules import sde_grid_arrays
    grid = sde_grid_arrays(row.T, row.dt)
    g = torch.Generator().manual_seed(row.N * 31 + row.T)
    x = torch.randn(1 + grid["S"], row.N, 16, generator=g)
    content = torch.randn(row.N, 50, generator=g)
    sel = torch.randint(0, row.T, (row.N,), generator=g, dtype=torch.int32)
    return grid, x, content, sel, g


# ---- CDE: gode_cde_fwd / gode_cde_bwd at loosened tolerances ----------------------------------------------------------
# multi: some accepted step must cover at least 2 output times (floor(t0 + h) - floor(t0) >= 2).  Every row runs with all
# rows and with sel_t.  Inputs: x = randn(N, T) from Generator().manual_seed(100 + N + T), the parameters of seed 3.
CdeRow = collections.namedtuple("CdeRow", "name N T rtol atol content zcols multi reaches")

CDE_ROWS = [
    CdeRow("three-per-step", 17, 16, 1e-1, 1e-2, False, 16, True,
           "steps covering 2 and 3 output times (float64 controller: 8 steps with 0,2,2,3,2,2,3,1 outputs); two workgroups"),
    CdeRow("five-per-step", 33, 16, 0.5, 0.1, False, 16, True,
           "three workgroups; 5 steps, up to 5 outputs in one; the last step ends well past T - 1: stage times past the "
           "last knot"),
    CdeRow("gap-then-two", 20, 5, 1e-2, 1e-3, False, 16, True,
           "a step with no output between steps with outputs, then one with 2"),
    CdeRow("all-in-one", 5, 3, 1e-1, 1e-2, False, 16, True, "one step holds every output"),
    CdeRow("t2", 3, 2, 1e-4, 1e-6, False, 16, False, "T = 2, the accepted minimum: one spline interval, one output"),
    CdeRow("content-68", 17, 16, 1e-1, 1e-2, True, 68, True, "a content code at zcols = 68, all rows and sel_t"),
    CdeRow("content-96", 20, 5, 1e-4, 1e-6, True, 96, False, "a content code at zcols = 96, default tolerances"),
]
CDE_BY_NAME = {r.name: r for r in CDE_ROWS}


def cde_inputs(row):
    """the row's host inputs: x [N, T], content [N, 50] (None without a content code), and the generator of x"""
    g = torch.Generator().manual_seed(100 + row.N + row.T)
    x = torch.randn(row.N, row.T, generator=g)
    content = torch.randn(row.N, 50, generator=torch.Generator().manual_seed(7 + row.N)) if row.content else None
    return x, content, g


def cde_per_step(sched_t, sched_h, T):
    """output times 1..T-1 inside (t0, t0 + h] per accepted step"""
    counts = []
    for t0, h in zip(sched_t, sched_h):
        t0, t1 = float(t0), float(t0) + float(h)
        counts.append(sum(1 for j in range(1, T) if t0 < j <= t1))
    return counts


def cde_covers_two(sched_t, sched_h):
    """some accepted step has floor(t0 + h) - floor(t0) >= 2"""
    import math
    return any(math.floor(float(t0) + float(h)) - math.floor(float(t0)) >= 2 for t0, h in zip(sched_t, sched_h))
