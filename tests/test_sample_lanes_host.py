"""CPU: the host logic of two-lane sampling -- which path a call takes (engine.lane_mode), which main-lane op releases the
side lane (engine.release_after) and the argument errors of gode_run_lanes, which come back before any HIP call."""
import ctypes as C

import pytest

from gan_ode_amd import _lib as L
from gan_ode_amd import engine as E

# every condition as it stands when a call overlaps
ALL_GOOD = dict(enabled=True, trace=False, recording=False, categorical=False, grad=False, keep=False, fixed_grid_ode=True,
                splittable=True, prev_lanes=True, launches_between=0, repacked=False, versions_same=True, same_stream=True,
                gpu_behind=True)


def test_overlap_needs_every_condition():
    assert E.lane_mode(**ALL_GOOD) == E.LANE_OVERLAP


@pytest.mark.parametrize("flip", [dict(prev_lanes=False), dict(launches_between=1), dict(launches_between=-1),
                                  dict(repacked=True), dict(versions_same=False), dict(same_stream=False)])
def test_one_broken_overlap_condition_orders_the_call(flip):
    assert E.lane_mode(**{**ALL_GOOD, **flip}) == E.LANE_ORDERED


@pytest.mark.parametrize("flip", [dict(enabled=False), dict(trace=True), dict(recording=True), dict(categorical=True),
                                  dict(grad=True), dict(keep=True), dict(fixed_grid_ode=False), dict(splittable=False),
                                  dict(gpu_behind=False)])
def test_one_single_stream_condition_keeps_the_one_stream_path(flip):
    assert E.lane_mode(**{**ALL_GOOD, **flip}) == E.LANE_SINGLE
    # ... whatever the overlap conditions say
    assert E.lane_mode(**{**ALL_GOOD, **flip, "prev_lanes": False, "versions_same": False}) == E.LANE_SINGLE


def test_gate_starts_a_streak_two_calls_behind_and_keeps_it_one_call_behind():
    # (previous call took the lanes, its staging copy pending, the copy of the call before it pending)
    assert not E.lane_gate(False, False, False)         # idle GPU: a caller that consumes every result first
    assert not E.lane_gate(False, True, False)          # one call behind: not enough to start
    assert E.lane_gate(False, True, True)               # two behind: start
    assert E.lane_gate(True, True, False)               # in a streak one behind is enough to go on
    assert E.lane_gate(True, True, True)
    assert not E.lane_gate(True, False, False)          # the GPU caught up: the streak ends
    assert not E.lane_gate(False, None, None) and not E.lane_gate(True, None, None)     # no such calls yet


def test_ring_back_names_the_slots_of_the_previous_calls():
    filled = []                          # slot order of a ring of 4, as stage_inputs fills it
    i = 0
    for call in range(9):
        if call >= 1:
            assert E.ring_back(i, 4, 1) == filled[-1]
        if call >= 2:
            assert E.ring_back(i, 4, 2) == filled[-2]
        filled.append(i)
        i = (i + 1) % 4


# hand-built op lists over made-up addresses:
# [solve | layer-0 GEMM || finalize(0), apply(0), GEMM 1, finalize(1), apply(1), GEMM 2]
IN, Z, TRAJ, Y0, ST0, A0, Y1, ST1, A1, OUT, WORK, W = (0x1000 * k for k in range(1, 13))


def _decoder(a0):
    solve = L.OdeFwdOp(x=IN, content=IN + 64, z=Z, traj=TRAJ)
    solve.p.W1 = W                       # a parameter pointer the solve only reads
    return [solve,
            L.IgemmOp(src=Z, wpack=W + 8, out=Y0, stats=ST0, work=WORK),
            L.BnFinalizeOp(stats=ST0, scale=W + 16, shift=W + 24),
            L.BnApplyOp(y=Y0, out=a0, scale=W + 16, shift=W + 24),
            L.IgemmOp(src=a0, wpack=W + 32, out=Y1, stats=ST1, work=WORK),
            L.BnFinalizeOp(stats=ST1, scale=W + 40, shift=W + 48),
            L.BnApplyOp(y=Y1, out=A1, scale=W + 40, shift=W + 48),
            L.IgemmOp(src=A1, wpack=W + 56, out=OUT, work=WORK)]


def test_release_after_is_the_layer0_apply_when_its_output_is_a_buffer_of_its_own():
    ops = _decoder(A0)
    written = E.front_writes(ops[:2], uses_work=lambda op: False)
    assert written == {Z, TRAJ, Y0, ST0}
    assert E.release_after(ops, 2, written) == 3


def test_release_after_is_the_layer1_gemm_when_the_apply_runs_in_place():
    ops = _decoder(Y0)                   # a[0] aliases y[0]: the layer-1 GEMM reads the buffer the front writes
    assert E.release_after(ops, 2, E.front_writes(ops[:2], uses_work=lambda op: False)) == 4


def test_a_front_gemm_that_uses_the_shared_workspace_holds_the_lane_to_the_last_gemm():
    ops = _decoder(A0)
    assert WORK in E.front_writes(ops[:2])         # (the default answer: it does)
    assert E.release_after(ops, 2) == 7


def test_release_after_with_no_reader_is_the_first_main_op_and_bad_splits_are_refused():
    ops = _decoder(A0)
    assert E.release_after(ops, 2, set()) == 2
    for n_front in (0, len(ops), len(ops) + 1):
        with pytest.raises(ValueError):
            E.release_after(ops, n_front, set())
    with pytest.raises(ValueError):              # an op kind with no write set cannot sit in a front
        E.front_writes([L.BnApplyOp(y=Y0, out=A0)])


def test_a_reader_through_an_interior_pointer_is_seen_when_the_buffer_has_an_extent():
    ops = _decoder(A0)
    ops[5].stats1 = ST0 + 256            # finalize(1) made to read the inside of the layer-0 statistics
    written = E.front_writes(ops[:2], uses_work=lambda op: False)
    assert E.release_after(ops, 2, written) == 3                       # base addresses alone: not seen
    assert E.release_after(ops, 2, written, {ST0: 1024}) == 5
    assert E.release_after(ops, 2, written, {ST0: 256}) == 3           # one byte past the end is outside


def test_op_pointers_sees_nested_parameter_blocks_and_skips_nulls():
    solve = _decoder(A0)[0]
    assert sorted(E.op_pointers(solve)) == sorted([W, IN, IN + 64, Z, TRAJ])


def test_run_lanes_argument_errors_come_before_any_hip_call():
    lib = L.lib()
    op = L.BnApplyOp()
    kinds, ops = (L.i32 * 2)(L.OP_BN_APPLY, L.OP_BN_APPLY), (L.ptr * 2)(C.addressof(op), C.addressof(op))
    # (the object is not looked into before the arguments are through: any non-null address stands in for one here)
    obj = C.addressof(C.create_string_buffer(256))
    run = lib.gode_run_lanes
    assert run(None, kinds, ops, 2, 1, 1, L.LANES_ORDERED, None) == -1            # null object
    assert run(obj, kinds, ops, 2, 3, 1, L.LANES_ORDERED, None) == -1             # n_front > n
    assert run(obj, kinds, ops, 2, 1, 0, L.LANES_ORDERED, None) == -1             # release_after < n_front
    assert run(obj, kinds, ops, 2, 1, 2, L.LANES_ORDERED, None) == -1             # release_after >= n
    assert run(obj, kinds, ops, 2, 2, 1, L.LANES_OVERLAP, None) == -1             # n_front == n: no main lane
    assert run(obj, kinds, ops, 2, -1, 1, L.LANES_ORDERED, None) == -1
    assert run(obj, kinds, ops, 2, 1, 1, 7, None) == -1                           # unknown mode
    assert run(obj, None, ops, 2, 1, 1, L.LANES_ORDERED, None) == -1
    assert lib.gode_lanes_create(None) == -1
    assert lib.gode_lanes_destroy(None) == -1
    assert lib.gode_lanes_stream(None) is None
