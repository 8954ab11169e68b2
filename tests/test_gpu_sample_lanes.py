"""GPU: two-lane sampling (the next call's H2D copy, latent solve and layer-0 GEMM on a side stream under this call's
decoder) against the one-stream path in the same process: every scenario runs once with gen.sample_lanes = "always" (two
lanes whether or not the GPU is behind the host, so that no mode depends on timing) and once with False from the same
seeds, and every call's videos and the BatchNorm running statistics afterwards must agree bit for bit.  The shapes are
tiny (2 videos of 4 frames, ngf = 8): the hazards are orderings, not sizes.  No scenario synchronises between calls."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from conftest import seed_all

import gan_ode_amd as G
from gan_ode_amd import _lib as L

pytestmark = pytest.mark.gpu

N, T = 2, 4


def _plan(gen, n=N, T_=T):
    return gen._pool.plans[(n, T_, False)][0]


def _sample(gen, modes, n=N):
    """One no-grad call; appends the path it took to `modes`."""
    with torch.no_grad():
        v, _ = gen.sample_videos(n, video_len=T)
    calls = _plan(gen, n).lane_calls
    seen = modes.setdefault("_seen", {}).setdefault(n, dict.fromkeys(calls, 0))
    took = [k for k in calls if calls[k] != seen[k]]
    assert len(took) == 1, (calls, seen)
    seen.update(calls)
    modes.setdefault("calls", []).append(took[0])
    return v


def _both(body, with_trainer=False):
    """body(gen, modes[, trainer]) -> list of tensors; run with lanes on and off -> (modes of the lanes-on run); asserts
    the results and the running statistics bitwise equal."""
    runs = []
    for lanes in ("always", False):
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
    assert set(m0) == {"single"}, m0
    assert len(o1) == len(o0) and len(s1) == len(s0) > 0
    for k, (a, b) in enumerate(zip(o1 + s1, o0 + s0)):
        assert a.shape == b.shape and torch.equal(a, b), k
    return m1


def test_eight_calls_back_to_back_overlap():
    modes = _both(lambda gen, m: [_sample(gen, m) for _ in range(8)])
    assert modes[0] == "ordered" and modes.count("overlap") >= 6, modes


@pytest.mark.parametrize("which", ["layer0_weight", "ode_weight"])
def test_in_place_change_of_a_tensor_the_front_reads_orders_the_next_call(which):
    def body(gen, m):
        outs = [_sample(gen, m) for _ in range(3)]
        w = gen.main[0].weight if which == "layer0_weight" else gen.ode_fn.fn[0].weight
        with torch.no_grad():
            w.mul_(1.25)
        return outs + [_sample(gen, m) for _ in range(3)]

    modes = _both(body)
    assert modes == ["ordered", "overlap", "overlap", "ordered", "overlap", "overlap"], modes


def test_a_generator_step_between_calls_orders_the_next_call():
    def body(gen, m, tr):
        outs = [_sample(gen, m) for _ in range(3)]
        tr.g_step(2)                     # libgode's backward passes and Adam: the weights the front reads change
        return outs + [_sample(gen, m) for _ in range(3)]

    modes = _both(body, with_trainer=True)
    assert modes[:3] == ["ordered", "overlap", "overlap"] and modes[3] == "ordered" and modes[4:] == ["overlap"] * 2, modes


def test_load_state_dict_between_calls_orders_the_next_call():
    def body(gen, m):
        sd = {k: (v * 0.5 if v.is_floating_point() else v.clone()) for k, v in gen.state_dict().items()}
        outs = [_sample(gen, m) for _ in range(3)]
        gen.load_state_dict(sd)
        return outs + [_sample(gen, m) for _ in range(3)]

    modes = _both(body)
    assert modes == ["ordered", "overlap", "overlap", "ordered", "overlap", "overlap"], modes


def test_two_plans_alternating_are_always_ordered():
    modes = _both(lambda gen, m: [_sample(gen, m, n) for n in (2, 3, 2, 3, 2, 3)])
    assert modes == ["ordered"] * 6, modes


def test_calls_under_a_user_stream_with_a_consumer_on_it():
    def body(gen, m):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        outs = []
        with torch.cuda.stream(s):
            for _ in range(4):
                v = _sample(gen, m)
                outs += [v, v.double().sum(dim=(1, 2, 3, 4))]     # a consumer queued right behind the call, on s
        torch.cuda.current_stream().wait_stream(s)
        outs.append(_sample(gen, m))      # ... and a call back on the default stream: another stream, so ordered
        return outs

    modes = _both(body)
    assert modes == ["ordered", "overlap", "overlap", "overlap", "ordered"], modes


def test_a_state_dict_clone_queued_between_two_calls_sees_what_it_sees_on_one_stream():
    def body(gen, m):
        outs = [_sample(gen, m), _sample(gen, m)]
        clone = [v.clone() for v in gen.state_dict().values()]      # queued on the caller's stream, no synchronisation
        outs += [_sample(gen, m), _sample(gen, m)]
        return outs + clone

    modes = _both(body)
    assert modes == ["ordered", "overlap", "overlap", "overlap"], modes


def test_under_trace_the_path_is_single():
    def body(gen, m):
        outs = [_sample(gen, m), _sample(gen, m)]
        L.TRACE = []
        try:
            outs.append(_sample(gen, m))
        finally:
            L.TRACE = None
        return outs + [_sample(gen, m), _sample(gen, m)]

    modes = _both(body)
    assert modes == ["ordered", "overlap", "single", "ordered", "overlap"], modes


def test_a_write_through_data_followed_by_invalidate_packs_orders_the_next_call():
    """p.data.mul_() bumps no version counter: gen.invalidate_packs() is the documented call after it."""
    def body(gen, m):
        outs = [_sample(gen, m) for _ in range(3)]
        gen.ode_fn.fn[0].weight.data.mul_(1.25)
        gen.invalidate_packs()
        return outs + [_sample(gen, m) for _ in range(3)]

    modes = _both(body)
    assert modes == ["ordered", "overlap", "overlap", "ordered", "overlap", "overlap"], modes


def test_a_rebuilt_latent_program_orders_the_next_call():
    """gen.ode_step_size rebuilds the solve's grid tensors, uploaded on the caller's stream."""
    def body(gen, m):
        outs = [_sample(gen, m) for _ in range(3)]
        gen.ode_step_size = 0.125
        return outs + [_sample(gen, m) for _ in range(3)]

    modes = _both(body)
    assert modes == ["ordered", "overlap", "overlap", "ordered", "overlap", "overlap"], modes


def test_sample_images_takes_the_lanes_bitwise():
    def body(gen, m):
        outs = []
        with torch.no_grad():
            for _ in range(4):
                outs.append(gen.sample_images(3)[0])
        calls = gen._pool.plans[(3, gen.video_length, True)][0].lane_calls
        m["calls"] = [k for k in ("ordered", "overlap", "single") for _ in range(calls[k])]
        return outs

    assert _both(body) == ["ordered", "overlap", "overlap", "overlap"]


def test_a_caller_that_synchronises_after_every_call_stays_on_one_stream():
    """The default (sample_lanes = True): a call that finds the previous call's staging copy complete has no decoder to
    put its front under."""
    seed_all(5)
    gen, _, _ = G.build_mnist(ngf=8, ndf=8)
    gen.cuda()
    modes = {}
    for _ in range(4):
        _sample(gen, modes)
        torch.cuda.synchronize()
    assert modes["calls"] == ["single"] * 4


def test_lanes_object_round_trip_and_a_capturing_stream_runs_in_order():
    """gode_lanes_create / _destroy on a real object, and gode_run_lanes on a capturing stream: every op goes to that stream
    in order (no fork inside a capture), so the replayed graph writes what the one-stream program writes."""
    lib = L.lib()
    h = L.ptr()
    assert lib.gode_lanes_create(C.byref(h)) == 0 and h.value and lib.gode_lanes_stream(h)
    x = torch.arange(4096, dtype=torch.float32, device="cuda").view(64, 64) - 2000.0
    mid, out, ref = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    ops = [L.BnApplyOp(y=x.data_ptr(), out=mid.data_ptr(), M=64, C=64, act=L.ACT_RELU),
           L.BnApplyOp(y=mid.data_ptr(), out=out.data_ptr(), M=64, C=64, act=L.ACT_NONE)]
    kinds, ptrs = (L.i32 * 2)(*[o.KIND for o in ops]), (L.ptr * 2)(*[C.addressof(o) for o in ops])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        assert lib.gode_run_lanes(h, kinds, ptrs, 2, 1, 1, L.LANES_ORDERED, st) == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, x.clamp_min(0))
    # ... and outside a capture the same call forks and joins
    out.zero_()
    assert lib.gode_run_lanes(h, kinds, ptrs, 2, 1, 1, L.LANES_ORDERED, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x.clamp_min(0))
    del g
    assert lib.gode_lanes_destroy(h) == 0


def test_environment_knob_keeps_one_stream():
    """GODE_SAMPLE_LANES=0 is read once per process, so this is a process of its own."""
    code = ("import torch, gan_ode_amd as G\n"
            "gen, _, _ = G.build_mnist(ngf=8, ndf=8); gen.cuda(); gen.sample_lanes = 'always'\n"
            "with torch.no_grad():\n"
            "    for _ in range(3): gen.sample_videos(2, video_len=4)\n"
            "torch.cuda.synchronize(); print(gen._pool.plans[(2, 4, False)][0].lane_calls)\n")
    from conftest import REPO
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env={**os.environ, "GODE_SAMPLE_LANES": "0"},
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "{'overlap': 0, 'ordered': 0, 'single': 3}" in r.stdout, r.stdout


def test_switching_the_knob_on_after_the_plan_was_built_makes_the_lanes_object_then():
    """An A/B run that starts with sample_lanes = False: the plan has no lanes object until the first lanes call."""
    seed_all(5)
    gen, _, _ = G.build_mnist(ngf=8, ndf=8)
    gen.cuda()
    gen.sample_lanes = False
    modes = {}
    _sample(gen, modes)
    assert gen.lane_stats()["lanes_objects"] == 0
    gen.sample_lanes = "always"
    _sample(gen, modes); _sample(gen, modes)
    torch.cuda.synchronize()
    st = gen.lane_stats()
    assert modes["calls"] == ["single", "ordered", "overlap"], modes
    assert st["lanes_objects"] == 1 and st["lanes_objects_made_late"] == 1 and st["overlap"] == 1, st
