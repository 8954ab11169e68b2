"""GPU: pair-mode sampling (two decoder passes in flight on two plans used in turn, the BatchNorm running statistics
updated by one trailing op on the caller's stream) against the one-stream path in the same process: every scenario runs
once with gen.sample_lanes = "pair" (pair mode whether or not the GPU is behind the host, so that no mode depends on
timing) and once with False from the same seeds; every call's videos and labels, and all running statistics and
num_batches_tracked afterwards, must be torch.equal.  Tiny shapes (2 videos of 4 frames, ngf = 8): the hazards are
orderings, not sizes.  No scenario synchronises between calls.  The first call of EACH plan is ordered: building a plan and
its program queues uploads on the caller's stream, so a fresh generator starts ordered, ordered, overlap, ..."""
import pytest
import torch

from conftest import seed_all

import gan_ode_amd as G

pytestmark = pytest.mark.gpu

N, T = 2, 4


def _sample(gen, modes, n=N):
    """One no-grad call -> [videos, labels]; appends the path it took to modes["calls"]."""
    before = gen.lane_stats()
    with torch.no_grad():
        v, lab = gen.sample_videos(n, video_len=T)
    after = gen.lane_stats()
    took = [k for k in ("pair_overlap", "pair_ordered", "overlap", "ordered", "single") if after[k] != before[k]]
    assert len(took) == 1, (before, after)
    modes.setdefault("calls", []).append(took[0])
    return [v, lab]


def _both(body, with_trainer=False):
    """body(gen, modes[, trainer]) -> list of tensors; run in pair mode and on one stream -> the modes of the pair run;
    asserts the results and the running statistics bitwise equal."""
    runs = []
    for lanes in ("pair", False):
        seed_all(5)
        gen, dv, di = G.build_mnist(ngf=8, ndf=8)
        gen.cuda()
        gen.sample_lanes = lanes
        modes = {}
        if with_trainer:
            dv.cuda(); di.cuda()
            outs = body(gen, modes, G.GanTrainer(gen, dv, di))
        else:
            outs = body(gen, modes)
        stats = [b.clone() for k, b in gen.state_dict().items() if "running" in k or "num_batches" in k]
        torch.cuda.synchronize()
        runs.append((outs, stats, modes["calls"]))
    (o1, s1, m1), (o0, s0, m0) = runs
    assert set(m0) - {"grad"} == {"single"}, m0          # ("grad": the marker of a gradient-mode call, in both runs)
    assert len(o1) == len(o0) and len(s1) == len(s0) == 12
    for k, (a, b) in enumerate(zip(o1 + s1, o0 + s0)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), k
    return m1


def _flat(pairs):
    return [t for p in pairs for t in p]


def test_twelve_calls_back_to_back():
    modes = _both(lambda gen, m: _flat(_sample(gen, m) for _ in range(12)))
    assert modes == ["pair_ordered"] * 2 + ["pair_overlap"] * 10, modes


def test_a_state_dict_clone_queued_between_calls_3_and_4_sees_what_it_sees_on_one_stream():
    def body(gen, m):
        outs = _flat(_sample(gen, m) for _ in range(3))
        clone = [v.clone() for k, v in gen.state_dict().items() if "running" in k or "num_batches" in k]
        outs += _flat(_sample(gen, m) for _ in range(3))
        return outs + clone

    modes = _both(body)
    assert modes == ["pair_ordered"] * 2 + ["pair_overlap"] * 4, modes


def test_a_reader_of_result_n_queued_before_call_n_plus_1_sees_result_n():
    """A long consumer (a big matmul) sits on the caller's stream in front of the reader, so the reader runs while later
    calls' lanes are already at work; the reader's copy must equal the result as it is at the end."""
    def body(gen, m):
        big = torch.randn(3072, 3072, device="cuda")
        outs, kept = [], []
        for _ in range(8):
            v, lab = _sample(gen, m)
            big @ big                                     # noqa: B018 -- queued in front of the reader
            outs += [v.clone(), v.double().sum(dim=(1, 2, 3, 4)), lab]
            kept.append(v)
        return outs + kept

    modes = _both(body)
    assert modes == ["pair_ordered"] * 2 + ["pair_overlap"] * 6, modes


def test_weight_writes_between_calls_order_the_next_call():
    def body(gen, m, tr):
        outs = _flat(_sample(gen, m) for _ in range(3))
        gen.main[3].weight.data.mul_(1.25)                # a layer-1 weight, behind autograd's back ...
        gen.main[4].weight.data.add_(0.5)                 # ... and a BatchNorm gamma
        gen.invalidate_packs()
        outs += _flat(_sample(gen, m) for _ in range(3))
        tr.g_step(2)                                      # an optimiser step: libgode's backward passes and Adam
        outs += _flat(_sample(gen, m) for _ in range(3))
        sd = {k: (v * 0.5 if v.is_floating_point() else v.clone()) for k, v in gen.state_dict().items()}
        gen.load_state_dict(sd)
        outs += _flat(_sample(gen, m) for _ in range(3))
        with torch.no_grad():
            gen.main[10].bias.mul_(1.5)                   # an in-place write torch's version counter sees
        return outs + _flat(_sample(gen, m) for _ in range(3))

    modes = _both(body, with_trainer=True)
    assert modes == ["pair_ordered"] * 2 + ["pair_overlap"] + ["pair_ordered", "pair_overlap", "pair_overlap"] * 4, modes


def test_sample_images():
    def body(gen, m):
        outs = []
        for _ in range(5):
            before = gen.lane_stats()
            with torch.no_grad():
                outs.append(gen.sample_images(3)[0])
            after = gen.lane_stats()
            m.setdefault("calls", []).extend(k for k in after if k in ("pair_overlap", "pair_ordered", "single")
                                             and after[k] != before[k])
        return outs

    assert _both(body) == ["pair_ordered"] * 2 + ["pair_overlap"] * 3


def test_a_call_in_gradient_mode_between_pair_calls():
    def body(gen, m):
        outs = _flat(_sample(gen, m) for _ in range(3))
        v, lab = gen.sample_videos(N, video_len=T)        # gradient mode: the one-stream path, on the first plan
        assert v.requires_grad
        outs += [v.detach(), lab]
        m["calls"].append("grad")
        return outs + _flat(_sample(gen, m) for _ in range(3))

    modes = _both(body)
    # (the gradient-mode call keeps its plan checked out for a backward pass while `v` lives, so the pool hands the calls
    # behind it a fresh first plan, which builds a second one of its own: two more first calls)
    assert modes == ["pair_ordered", "pair_ordered", "pair_overlap", "grad", "pair_ordered", "pair_ordered", "pair_overlap"]


def test_eval_mode_calls_between_pair_calls_hand_the_streak_to_the_two_lane_front_and_back():
    """An eval-mode pass has no pair form, so under the same knob its calls take the two-lane front: a call of one kind
    ends the streak of the other and starts its own ordered (the first eval call also builds its program)."""
    def body(gen, m):
        outs = _flat(_sample(gen, m) for _ in range(3))
        gen.eval()
        outs += _flat(_sample(gen, m) for _ in range(3))
        gen.train()
        return outs + _flat(_sample(gen, m) for _ in range(3))

    modes = _both(body)
    assert modes == (["pair_ordered", "pair_ordered", "pair_overlap", "ordered", "overlap", "overlap",
                      "pair_ordered", "pair_overlap", "pair_overlap"]), modes


def test_the_second_plan_is_built_when_a_streak_starts_and_the_default_stays_single_for_a_lone_caller():
    seed_all(5)
    gen, _, _ = G.build_mnist(ngf=8, ndf=8)
    gen.cuda()
    modes = {}
    for _ in range(3):                                    # the default knob: a caller that waits for every result
        _sample(gen, modes)
        torch.cuda.synchronize()
    st = gen.lane_stats()
    assert modes["calls"] == ["single"] * 3 and st["pair_plans"] == 0 and st["lanes_objects"] == 1, (modes, st)
    gen.sample_lanes = "pair"
    _sample(gen, modes)
    assert gen.lane_stats()["pair_plans"] == 0            # the first call of a streak runs on the first plan
    _sample(gen, modes); _sample(gen, modes)
    torch.cuda.synchronize()
    st = gen.lane_stats()
    assert modes["calls"][3:] == ["pair_ordered", "pair_ordered", "pair_overlap"] and st["pair_plans"] == 1, (modes, st)
    assert set(gen._pool.plans) == {(N, T, False)} and len(gen._pool.plans[(N, T, False)]) == 1
