"""CPU: the host-side decisions of pair-mode sampling (two decoder passes in flight on two plans used in turn) as pure
functions -- which plan takes a call, whose entry event its lane waits for, when a streak starts and goes on -- and the
property edge (a) of DESIGN section 24 rests on: whatever a call's lane overwrites was last used at least two calls ago,
and the event it waits for was recorded after that."""
import itertools

from gan_ode_amd.engine import lane_gate, lane_mode, pair_schedule, pair_turn, pair_wait


def test_plans_alternate_and_a_fresh_streak_starts_on_the_first_plan():
    assert pair_turn(None) == 0
    assert pair_turn(0) == 1 and pair_turn(1) == 0
    turns, prev = [], None
    for _ in range(6):
        prev = pair_turn(prev)
        turns.append(prev)
    assert turns == [0, 1, 0, 1, 0, 1]


def test_an_overlapping_call_waits_for_the_peers_entry_event_and_an_ordered_one_for_its_own():
    for turn in (0, 1):
        assert pair_wait(turn, True) == 1 - turn
        assert pair_wait(turn, False) == turn


def test_a_streak_of_pair_calls():
    calls = [(True, False)] + [(False, True)] * 5
    assert pair_schedule(calls) == [(0, 0), (1, 0), (0, 1), (1, 2), (0, 3), (1, 4)]


def test_an_ordered_call_inside_a_streak_keeps_alternating_and_waits_for_its_own_entry():
    """(a weight was written between calls 2 and 3: the previous forward was a pair call, so the plans go on in turn)"""
    calls = [(True, False), (False, True), (False, True), (False, False), (False, True)]
    assert pair_schedule(calls) == [(0, 0), (1, 0), (0, 1), (1, 3), (0, 3)]


def test_a_call_behind_a_forward_that_was_no_pair_call_starts_afresh_and_cannot_overlap():
    calls = [(True, False), (False, True), (True, True), (False, True)]
    assert pair_schedule(calls) == [(0, 0), (1, 0), (0, 2), (1, 2)]


def test_edge_a_every_lane_starts_behind_the_last_use_of_what_it_overwrites():
    """Over every sequence of 7 calls: the lane of call m on plan P waits for an event recorded at the entry of call m - 1
    or later, and P's previous call k (whose result, tail op and buffers call m overwrites) has k <= m - 2 whenever the
    call overlaps -- so everything the caller queued against result k before call k + 1 <= m - 1 entered has run.  An
    ordered call waits for its own entry: for everything queued so far."""
    for flags in itertools.product([(True, False), (False, True), (False, False)], repeat=7):
        flags = ((True, False),) + flags[1:]
        last_on = {}
        for m, ((turn, waited), (fresh, may)) in enumerate(zip(pair_schedule(flags), flags)):
            assert waited in (m, m - 1), (flags, m)
            if waited == m - 1:
                assert may and not fresh
                assert last_on.get(turn, -1) <= m - 2, (flags, m)
                assert last_on.get(1 - turn) == m - 1, (flags, m)
            last_on[turn] = m


def test_the_gate_starts_a_streak_two_calls_behind_and_keeps_it_one_behind():
    assert lane_gate(False, True, True) and not lane_gate(False, True, False) and not lane_gate(False, False, False)
    assert lane_gate(True, True, False) and not lane_gate(True, False, False)


def test_pair_calls_overlap_under_the_conditions_of_the_two_lanes():
    base = dict(enabled=True, trace=False, recording=False, categorical=False, grad=False, keep=False, fixed_grid_ode=True,
                splittable=True, prev_lanes=True, launches_between=0, repacked=False, versions_same=True, same_stream=True)
    assert lane_mode(**base) == "overlap"
    for k, v in (("prev_lanes", False), ("launches_between", 1), ("repacked", True), ("versions_same", False),
                 ("same_stream", False)):
        assert lane_mode(**{**base, k: v}) == "ordered", k
    for k in ("trace", "recording", "categorical", "grad", "keep"):
        assert lane_mode(**{**base, k: True}) == "single", k
    assert lane_mode(**{**base, "gpu_behind": False}) == "single"
