"""GPU: generator latents drawn on the device (latent_rng = "device"; gode_latent_draw) -- the op against
the restatement of tests/latent_rng_ref.py, exact pruning, and the generators, lanes, trainer and graph replay against
host-mode twins that are fed the stream's values."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_rng_ref as R
from conftest import seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
import gan_ode_amd.modules as Mod

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15          # (above 2^63: the seed travels as a signed field)
PAD = 8
INT_SENTINEL = 0x7FFFFFFF


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_op(n, outer, inner, T, n_all, C_, traj0, call, stream_, seed=SEED, call_dev=0, content=True, cls=True):
    """gode_latent_draw standalone, every sub-block between PAD sentinel words -> (x [outer, n, inner], content [n, 50] or
    None, sel_t or None, cls or None) as host tensors; asserts that the sentinels survive."""
    sizes = [outer * n * inner, n * 50 if content else 0, n if n_all else 0, n if (C_ and cls) else 0]
    fl = torch.full((PAD + sum(s + PAD for s in sizes),), float("nan"), device="cuda")
    bits = fl.view(torch.int32)
    offs, o = [], PAD
    for k, s in enumerate(sizes):
        offs.append(o)
        o += s + PAD
    bits[offs[2] - PAD:] = INT_SENTINEL
    before = bits.clone()
    ptr_of = lambda k: fl.data_ptr() + 4 * offs[k] if sizes[k] else None      # noqa: E731
    cd = torch.tensor([call_dev], dtype=torch.int32, device="cuda") if call_dev else None
    sseed = seed - (1 << 64) if seed >= 1 << 63 else seed
    scall = call - (1 << 32) if call >= 1 << 31 else call
    op = L.LatentDrawOp(x=ptr_of(0), content=ptr_of(1), sel_t=ptr_of(2), cls=ptr_of(3),
                        call_dev=cd.data_ptr() if cd is not None else None, seed=sseed, traj0=traj0, n=n, outer=outer,
                        inner=inner, T=T, n_all=n_all, C=C_, stream=stream_, call=scall)
    L.check(L.lib().gode_latent_draw(C.byref(op), stream()), "gode_latent_draw")
    torch.cuda.synchronize()
    keep = torch.ones_like(bits, dtype=torch.bool)
    for k, s in enumerate(sizes):
        keep[offs[k]:offs[k] + s] = False
    assert torch.equal(bits[keep], before[keep]), "a word outside the four sub-blocks was written"
    cut = lambda k: fl[offs[k]:offs[k] + sizes[k]].clone()                       # noqa: E731
    return (cut(0).view(outer, n, inner).cpu(), cut(1).view(n, 50).cpu() if sizes[1] else None,
            cut(2).view(torch.int32).cpu() if sizes[2] else None, cut(3).view(torch.int32).cpu() if sizes[3] else None)


CASES = [(1, 1, 16, 16, 0, 0, 0, 0, 0), (5, 1, 16, 2, 0, 3, 3, 7, 0), (33, 3, 16, 2, 0, 0, 0, 2 ** 32 - 1, 5),
         (4, 1, 16, 16, 0, 0, 2 ** 33, 1, 2 ** 21 - 1), (32, 1, 16, 16, 1024, 0, 0, 3, 0), (4, 1, 16, 4, 1, 0, 0, 0, 0),
         (1, 1, 16, 1, 2, 0, 0, 0, 0), (8, 1, 16, 16, 64, 30, 0, 9, 1),
         # the selection's two forms meet at 64 rows: one wavefront's registers up to there, block-wide above (300: more
         # rows than threads; 100 of 100: every collision branch of the block-wide form)
         (64, 1, 16, 4, 32, 0, 0, 4, 0), (65, 1, 16, 4, 32, 3, 0, 4, 0), (300, 2, 16, 16, 40, 0, 1, 6, 3),
         (100, 1, 16, 4, 25, 0, 0, 1, 0)]


@pytest.mark.parametrize("case", CASES, ids=[str(k) for k in range(len(CASES))])
def test_op_against_the_restatement(case):
    n, outer, inner, T, n_all, C_, traj0, call, stream_ = case
    call_dev = 1 if call == 2 ** 32 - 1 else 0                    # the wrap: (2^32 - 1) + 1 = call 0
    x, content, sel, cls = run_op(n, outer, inner, T, n_all, C_, traj0, call, stream_, call_dev=call_dev)
    rx, rc, rs, rk = R.draw(SEED, stream_, (call + call_dev) & 0xFFFFFFFF, n, outer, inner, T, n_all, C_, traj0)
    assert (sel is None) == (rs is None) and (cls is None) == (rk is None)
    if rs is not None:
        assert np.array_equal(sel.numpy(), rs)
        if n == n_all * T:                                         # B == R: every row, in order
            assert sel.tolist() == [r % T for r in range(n)]
    if rk is not None:
        assert np.array_equal(cls.numpy(), rk) and 0 <= int(cls.min()) and int(cls.max()) < C_
    ex, ec = np.abs(x.double().numpy() - rx).max(), np.abs(content.double().numpy() - rc).max()
    print(f"case {case}: max |z - z64| motion {ex:.3g} content {ec:.3g}")
    assert ex < 1e-5 and ec < 1e-5
    # the nullable outputs are optional, and the others do not depend on their presence
    x2, c2, s2, k2 = run_op(n, outer, inner, T, n_all, C_, traj0, call, stream_, call_dev=call_dev, content=False, cls=False)
    assert c2 is None and k2 is None and torch.equal(x2, x) and (s2 is None or torch.equal(s2, sel))


def test_pruning_is_exact():
    n, outer, inner, T, n_all = 8, 17, 16, 4, 64
    xs, cs, sel, ks = run_op(n, outer, inner, T, n_all, 5, 0, 11, 2)
    xf, cf, _, kf = run_op(n_all, outer, inner, T, 0, 5, 0, 11, 2)
    rows = R.selection(SEED, 2, 11, n, n_all * T)
    traj = torch.from_numpy(rows // T)
    assert np.array_equal(sel.numpy(), rows % T)
    assert torch.equal(xs, xf[:, traj]) and torch.equal(cs, cf[traj]) and torch.equal(ks, kf[traj])
    # ... and a full draw that starts at another trajectory is the tail of the full draw
    xt, ct, _, kt = run_op(n_all - 3, outer, inner, T, 0, 5, 3, 11, 2)
    assert torch.equal(xt, xf[:, 3:]) and torch.equal(ct, cf[3:]) and torch.equal(kt, kf[3:])


def test_repeatability_and_call_advance():
    a = run_op(32, 1, 16, 16, 1024, 7, 0, 5, 0)
    b = run_op(32, 1, 16, 16, 1024, 7, 0, 5, 0)
    c = run_op(32, 1, 16, 16, 1024, 7, 0, 6, 0)
    d = run_op(32, 1, 16, 16, 1024, 7, 0, 3, 0, call_dev=2)       # the base call from device memory: 2 + 3
    for p, q, r, s in zip(a, b, c, d):
        assert torch.equal(p, q) and torch.equal(p, s) and not torch.equal(p, r)


# ---- module level ----------------------------------------------------------------------------------------------------
GENS = {
    "ode_mnist": lambda: G.VideoGeneratorMNISTODE(1, 50, 0, 16, 4, dim_hidden=16, ngf=8),
    "ode_64_categ": lambda: G.VideoGenerator(3, 50, 3, 16, 4, dim_hidden=16, ngf=8),
    "tanh": lambda: Mod.VideoGeneratorMNISTODETanh(1, 50, 0, 16, 4, ngf=8),
    "odernn": lambda: Mod.VideoGeneratorMNISTODERNN(1, 50, 0, 16, 4, dim_hidden=16, ngf=8),
    "gru": lambda: Mod.VideoGeneratorGRU(3, 50, 0, 16, 4, ngf=8),
    "sde": lambda: Mod.VideoGeneratorSDE(1, 50, 0, 16, 4, ngf=8),
    "cde": lambda: Mod.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8),
}


def _pair_of(name, seed=3):
    """(device-mode generator, host-mode twin with the same weights) on the GPU."""
    out = []
    for mode in ("device", "host"):
        seed_all(seed)
        g = GENS[name]().cuda()
        g.latent_rng, g.latent_seed, g.latent_stream = mode, SEED, 4
        out.append(g)
    return out


def feed_twin(twin, dev_gen, first_call=0):
    """Replaces the host-mode twin's _host_inputs by the latent stream's values, read back from the op run standalone, for
    consecutive calls from `first_call` on: what the device-mode generator's calls draw, in call order."""
    state = dict(call=first_call)
    ncat = int(twin.dim_z_category)

    def host_inputs(select, n, T):
        twin._check_len(T)
        xs = _x_shape_of(dev_gen, select, n, T)
        outer, inner = (xs[0], xs[2]) if len(xs) == 3 else (1, xs[1])
        x, content, sel, cls = run_op(n, outer, inner, T, n * T * 2 if select else 0, ncat, 0, state["call"],
                                      dev_gen.latent_stream, seed=dev_gen.latent_seed)
        state["call"] = (state["call"] + 1) & 0xFFFFFFFF
        x = x.view(xs)
        return (x, content, sel) if not ncat else (x, content, sel, cls.numpy())

    twin._host_inputs = host_inputs
    return state


def _x_shape_of(gen, select, n, T):
    """The noise block's shape [outer, n, inner] or [n, inner] of the plan `gen` ran such a call on."""
    for plans in gen._pool.plans.values():
        for p in plans:
            for sub in (p.subplans() if isinstance(p, Mod._GenJointPlan) else (p,)):
                if (sub.select, sub.n, sub.T) == (select, n, T):
                    return tuple(sub.x.shape)
    raise AssertionError(f"the device-mode generator ran no plan for {(select, n, T)}")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(GENS))
def test_every_generator_against_its_host_twin(name, training):
    dev, twin = _pair_of(name)
    feed_twin(twin, dev)
    for g in (dev, twin):
        g.train(training)
    s_np, s_t = np.random.get_state()[1].copy(), torch.get_rng_state()
    res = {}
    for g in (dev, twin):
        v, lab = g.sample_videos(3)
        i, _ = g.sample_images(2)
        w = torch.linspace(-1, 1, v.numel() + i.numel(), device="cuda")
        loss = (v.reshape(-1) * w[:v.numel()]).sum() + (i.reshape(-1) * w[v.numel():]).sum()
        loss.backward()
        res[g] = (v.detach().clone(), lab.clone(), i.detach().clone(),
                  [(k, p.grad.clone()) for k, p in g.named_parameters() if p.grad is not None])
    assert dev.latent_call == 2 and twin.latent_call == 0
    assert np.array_equal(np.random.get_state()[1], s_np) and torch.equal(torch.get_rng_state(), s_t)
    (v1, l1, i1, g1), (v0, l0, i0, g0) = res[dev], res[twin]
    assert torch.equal(v1, v0) and torch.equal(i1, i0) and l1.dtype == l0.dtype and torch.equal(l1, l0)
    assert float(v1.abs().max()) > 0 and len(g1) == len(g0) > 0
    for (k1, a), (k0, b) in zip(g1, g0):
        assert k1 == k0 and torch.equal(a, b), k1
    # the device-mode plans carry the draw op in front of the latent program
    for key, plans in dev._pool.plans.items():
        assert [op.KIND for op in plans[0].fwd_prog.ops][0] == L.OP_LATENT_DRAW, key


def test_counter_semantics_and_global_rng_state():
    dev, twin = _pair_of("ode_mnist")
    s_np, s_t = np.random.get_state()[1].copy(), torch.get_rng_state()
    with torch.no_grad():
        dev.sample_videos(3)
        assert dev.latent_call == 1
        dev.sample_images(2)
        assert dev.latent_call == 2
        assert dev.can_pair(16, 16)         # (64 video rows: the statistics rows split at the batch boundary)
        dev.sample_pair(16, 16)
        assert dev.latent_call == 4
        dev.latent_call = 2 ** 32 - 1
        dev.sample_pair(16, 16, images_first=True)
        assert dev.latent_call == 1                                # wraps
        with dev.latents_at(7):
            a = [dev.sample_videos(3)[0].clone(), dev.sample_images(2)[0].clone()]
            assert dev.latent_call == 9
        assert dev.latent_call == 1
        with dev.latents_at(7):
            b = [dev.sample_videos(3)[0].clone(), dev.sample_images(2)[0].clone()]
        # (training mode: the batch statistics normalise, so the running statistics that moved in between do not show)
        assert all(torch.equal(p, q) for p, q in zip(a, b))
        # prefetch_latents consumes the indices in announcement order: bitwise the call-by-call results
        calls = [("videos", 3), ("images", 2), ("pair_iv", (16, 16)), ("videos", 3)]
        dev.latent_call = 20
        dev.prefetch_latents(calls)
        assert dev.latent_call == 25
        pre = [dev.sample_videos(3)[0].clone(), dev.sample_images(2)[0].clone()]
        (pv, _), (pi, _) = dev.sample_pair(16, 16, images_first=True)
        pre += [pv.clone(), pi.clone(), dev.sample_videos(3)[0].clone()]
        dev.latent_call = 20
        one = [dev.sample_videos(3)[0].clone(), dev.sample_images(2)[0].clone()]
        (pv, _), (pi, _) = dev.sample_pair(16, 16, images_first=True)
        one += [pv.clone(), pi.clone(), dev.sample_videos(3)[0].clone()]
        assert dev.latent_call == 25 and all(torch.equal(p, q) for p, q in zip(pre, one))
    assert np.array_equal(np.random.get_state()[1], s_np) and torch.equal(torch.get_rng_state(), s_t)
    # sample_pair against the twin fed the stream's values of its two calls, in the order of the calls
    for images_first in (False, True):
        feed_twin(twin, dev, first_call=30)
        dev.latent_call = 30
        with torch.no_grad():
            (v1, _), (i1, _) = dev.sample_pair(16, 16, images_first=images_first)
            (v0, _), (i0, _) = twin.sample_pair(16, 16, images_first=images_first)
        assert dev.latent_call == 32 and torch.equal(v1, v0) and torch.equal(i1, i0)
    # the reference's surface keeps drawing on the host in both modes
    twin = _pair_of("ode_mnist")[1]
    seed_all(9)
    z1 = dev.sample_z_video(2)[0]
    seed_all(9)
    z0 = twin.sample_z_video(2)[0]
    assert torch.equal(z1, z0) and dev.latent_call == 32
    dev.latent_rng = "bogus"
    with pytest.raises(ValueError, match="bogus"):
        dev.sample_pair(16, 16)


@pytest.mark.parametrize("knob", ["always", "pair"])
def test_lanes_and_pair_mode_are_bitwise_one_stream(knob):
    runs = []
    for lanes in (knob, False):
        seed_all(5)
        gen, _, _ = G.build_mnist(ngf=8, ndf=8)
        gen.cuda()
        gen.latent_rng, gen.latent_seed, gen.sample_lanes = "device", SEED, lanes
        with torch.no_grad():
            outs = [gen.sample_videos(2, video_len=4)[0] for _ in range(6)]
        stats = [b.clone() for k, b in gen.state_dict().items() if "running" in k]
        torch.cuda.synchronize()
        runs.append((outs + stats, gen.lane_stats()))
    (o1, st1), (o0, st0) = runs
    assert st0["single"] == 6 and st1["single"] == 0, (st0, st1)
    if knob == "pair":
        assert st1["pair_overlap"] + st1["pair_ordered"] == 6 and st1["pair_overlap"] >= 1, st1
    else:
        assert st1["overlap"] + st1["ordered"] == 6 and st1["overlap"] >= 1, st1
    assert gen.latent_call == 6
    for k, (a, b) in enumerate(zip(o1, o0)):
        assert torch.equal(a, b), k


def test_host_mode_is_unchanged(monkeypatch):
    def frames():
        seed_all(12)
        gen = GENS["ode_mnist"]().cuda()
        seed_all(13)
        with torch.no_grad():
            v, i = gen.sample_videos(3)[0].clone(), gen.sample_images(2)[0].clone()
            (pv, _), (pi, _) = gen.sample_pair(16, 16)
        kinds = [op.KIND for plans in gen._pool.plans.values() for p in plans
                 for op in (p.fwd_prog.ops if hasattr(p, "fwd_prog") else p.vid.fwd_prog.ops + p.img.fwd_prog.ops)]
        return [v, i, pv.clone(), pi.clone()], kinds, gen

    new, kinds, gen = frames()
    assert kinds and L.OP_LATENT_DRAW not in kinds and gen.latent_call == 0
    assert all(p.draw_op is None for plans in gen._pool.plans.values() for p in plans if hasattr(p, "draw_op"))

    # the same calls with the device-mode path made unreachable: the parent's path
    def unreachable(*a, **k):
        raise AssertionError("the device-mode path was entered in host mode")

    class Unreachable:
        __init__ = unreachable

    monkeypatch.setattr(Mod, "_DeviceLatents", Unreachable)
    monkeypatch.setattr(Mod._GenPlan, "_latent_program", lambda self, ops: L.Program(ops))
    monkeypatch.setattr(Mod._GenPlan, "_set_draw", unreachable)
    monkeypatch.setattr(Mod._GenPlan, "_draw_event", unreachable)
    monkeypatch.setattr(Mod.VideoGenerator, "_inputs", lambda self, *a: self._host_inputs(*a))
    old, _, _ = frames()
    assert all(torch.equal(a, b) for a, b in zip(new, old))


# ---- trainer ---------------------------------------------------------------------------------------------------------
def _trainer(mode, graph=False, seed=21):
    seed_all(seed)
    gen, dv, di = G.build_mnist(ngf=8, ndf=8)
    gen.cuda(); dv.cuda(); di.cuda()
    gen.latent_rng, gen.latent_seed = mode, SEED
    return G.GanTrainer(gen, dv, di, graph=graph), gen, dv, di


def _batches(it, B=4):
    rng = torch.Generator().manual_seed(100 + it)
    return ([torch.rand(B, 1, 28, 28, generator=rng).cuda() for _ in range(2)],
            [torch.rand(B, 16, 1, 28, 28, generator=rng).cuda() for _ in range(2)])


def _state(tr, nets):
    torch.cuda.synchronize()
    out = [v.detach().clone() for m in nets for v in m.state_dict().values()]
    for opt in (tr.gen_opt, tr.vid_opt, tr.img_opt):
        for st in opt.state_dict()["state"].values():
            out += [v.detach().clone() for v in st.values() if torch.is_tensor(v)]
    return out


def test_trainer_iteration_eager_against_the_host_twin():
    res = []
    for mode in ("device", "host"):
        tr, gen, dv, di = _trainer(mode)
        if mode == "host":
            feed_twin(gen, res[0][2])
        s_np, s_t = np.random.get_state()[1].copy(), torch.get_rng_state()
        losses = [float(v) for v in tr.step(*_batches(0))]
        if mode == "device":
            assert gen.latent_call == 6                            # 2 x (images, videos) + the generator step's two
            assert np.array_equal(np.random.get_state()[1], s_np) and torch.equal(torch.get_rng_state(), s_t)
        res.append((losses, _state(tr, (gen, dv, di)), gen))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert len(res[0][1]) == len(res[1][1]) > 20
    for k, (a, b) in enumerate(zip(res[0][1], res[1][1])):
        assert torch.equal(a, b), k


def test_trainer_graph_replay_is_bitwise_eager_device_mode():
    runs = []
    for graph in (True, False):
        tr, gen, dv, di = _trainer("device", graph=graph)
        losses = []
        for it in range(4):                                        # graph: the capture and three replays
            losses.append([float(v) for v in tr.step(*_batches(it))])
        assert (tr._graph is not None) == graph and gen.latent_call == 24
        if graph:
            kinds = [e[0] for e in tr._feed.script]
            assert "noise" not in kinds and kinds.count("latent") == 6, kinds
        runs.append((losses, _state(tr, (gen, dv, di))))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for k, (a, b) in enumerate(zip(runs[0][1], runs[1][1])):
        assert torch.equal(a, b), k
