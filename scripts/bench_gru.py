"""The GRU generator (VideoGeneratorGRU, the original MoCoGAN) against the ODE generator (VideoGenerator, rk4) at the UCF
shape in ONE process, alternating round by round so that clock and thermal drift hit both alike; timed with bench.py's
_timed.

  python scripts/bench_gru.py [--steps 30] [--warmup 5] [--rounds 5] [--out FILE]

Prints one JSON object:
  kernels:       the latent kernels alone, HIP events: the GRU forward and BPTT (its reduction included) at N = 16, 32
                 and 4096, and the ODE forward / adjoint at the same N, on seeded initial weights;
  sample_videos: ms per sample_videos(16) call (no_grad, train-mode BatchNorm, 3x64x64, ngf=64) and videos/s, median;
  iteration:     ms per GanTrainer.step at batch 16 (d_iters 2, ndf=64), median of rounds;
  ratios:        GRU / ODE for the last two.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import gan_ode_amd as G  # noqa: E402
import gan_ode_amd._lib as L  # noqa: E402

bench.torch = torch          # bench.py binds its module globals in main(); _timed's synchronisation needs torch
B, T, W = 16, 16, 64


def _gen(kind):
    torch.manual_seed(0)
    np.random.seed(0)
    if kind == "gru":
        return G.VideoGeneratorGRU(3, 50, 0, 16, T, ngf=W)
    return G.VideoGenerator(3, 50, 0, 16, T, dim_hidden=16, ngf=W)


def _nets(kind):
    gen = _gen(kind)
    dv, di = G.VideoDiscriminator(3, ndf=W), G.PatchImageDiscriminator(3, ndf=W)
    return gen.cuda(), dv.cuda(), di.cuda()


def _alternate(fns, steps, warmup, rounds):
    """{name: median ms per step over `rounds` rounds}, the callables taking turns every round"""
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            dt = bench._timed(fn, steps, warmup if r == 0 else 2, False)
            out[k].append(1e3 * dt / steps)
    return {k: statistics.median(v) for k, v in out.items()}, out


def _events(fn, reps=50, warmup=5):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps        # microseconds


def _gru_kernels(gen, N):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(N)
    dev = dict(device="cuda")
    _, prm = gen._param_list()
    noise = torch.randn(T + 1, N, 16, generator=g).cuda()
    content = torch.randn(N, 50, generator=g).cuda()
    z = torch.empty(N * T, 96, **dev)                  # the generator's latent-row layout (Z_COLS)
    hs = torch.empty(N, T + 1, 16, **dev)
    gz = torch.randn(N * T, 96, generator=g).cuda()
    work = torch.empty(int(L.lib().gode_gru_bwd_work_size(N)), **dev)
    grads = torch.empty(L.GRU_NPARAM, **dev)
    p = L.GruParams(*[q.data_ptr() for q in prm])
    fop = L.GruFwdOp(p=p, noise=noise.data_ptr(), content=content.data_ptr(), sel_t=None, z=z.data_ptr(),
                     hs=hs.data_ptr(), N=N, T=T, zcols=96)
    bop = L.GruBwdOp(p=p, noise=noise.data_ptr(), hs=hs.data_ptr(), sel_t=None, gz=gz.data_ptr(), work=work.data_ptr(),
                     grads=grads.data_ptr(), N=N, T=T, accumulate=0, zcols=96)
    return {"gru_fwd_us": _events(lambda: L.run_one(fop, st)), "gru_bwd_us": _events(lambda: L.run_one(bop, st))}


def _ode_kernels(gen, N):
    """the ODE generator's latent kernels through its own plan (fused pre-net + rk4 forward; adjoint)"""
    from gan_ode_amd.modules import _GenPlan
    st = torch.cuda.current_stream().cuda_stream
    plan = _GenPlan(gen, N, T, False, zbuf=torch.empty(N * T, 96, device="cuda"))     # the latent half only
    g = torch.Generator().manual_seed(N)
    plan.stage_inputs(torch.randn(N, 16, generator=g), torch.randn(N, 50, generator=g), None)
    gz = torch.randn(N * T, 96, generator=g).cuda()
    grads = torch.empty(L.ODE_NPARAM, device="cuda")
    plan.bwd_op.gz, plan.bwd_op.grads, plan.bwd_op.accumulate = gz.data_ptr(), grads.data_ptr(), 0
    return {"ode_fwd_us": _events(lambda: L.run_one(plan.fwd_op, st)),
            "ode_bwd_us": _events(lambda: L.run_one(plan.bwd_op, st))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G.limit_host_threads()
    init = {k: _gen(k).cuda() for k in ("gru", "ode")}        # seeded initial weights for the kernel timings
    kernels = {}
    for N in (16, 32, 4096):
        r = _gru_kernels(init["gru"], N)
        r.update(_ode_kernels(init["ode"], N))
        kernels[str(N)] = {k: round(v, 2) for k, v in r.items()}
    gens = {k: _nets(k) for k in ("ode", "gru")}

    def sampler(gen):
        def fn():
            with torch.no_grad():
                gen.sample_videos(B)
        return fn

    sv, sv_rounds = _alternate({k: sampler(v[0]) for k, v in gens.items()}, a.steps, a.warmup, a.rounds)
    rng = torch.Generator().manual_seed(1)
    imgs = [(torch.rand(B, 3, 64, 64, generator=rng) * 2 - 1).cuda() for _ in range(2)]
    vids = [(torch.rand(B, T, 3, 64, 64, generator=rng) * 2 - 1).cuda() for _ in range(2)]
    trainers = {k: G.GanTrainer(*v) for k, v in gens.items()}
    it_steps = max(a.steps // 3, 5)
    it, it_rounds = _alternate({k: (lambda tr=tr: tr.step(imgs, vids)) for k, tr in trainers.items()}, it_steps,
                               max(a.warmup // 3, 3), a.rounds)
    out = dict(device=torch.cuda.get_device_name(0), batch=B, T=T, ngf=W, ndf=W, steps=a.steps, rounds=a.rounds,
               kernels=kernels,
               sample_videos_ms={k: round(v, 4) for k, v in sv.items()},
               videos_per_s={k: round(B * 1e3 / v, 1) for k, v in sv.items()},
               iteration_ms={k: round(v, 3) for k, v in it.items()},
               ratios=dict(sample_videos=round(sv["gru"] / sv["ode"], 4), iteration=round(it["gru"] / it["ode"], 4)),
               rounds_ms=dict(sample_videos=sv_rounds, iteration=it_rounds))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
