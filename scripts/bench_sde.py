"""The Neural-SDE generator (VideoGeneratorSDE) against the ODE generator (VideoGeneratorMNISTODE) in ONE process,
alternating round by round so that clock and thermal drift hit both alike; timed with bench.py's _timed.

  python scripts/bench_sde.py [--steps 30] [--warmup 10] [--rounds 5] [--out FILE]

Prints one JSON object:
  sample_videos: ms per sample_videos(32) call (no_grad, train-mode BatchNorm, ngf=64) and videos/s, median of rounds;
  iteration:     ms per GanTrainer.step at batch 32 (d_iters 2, ndf=64), median of rounds;
  kernels:       the latent kernels alone (forward, and backward incl. its reduction) at N = 32 .. 2^16, HIP events.
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
from gan_ode_amd.modules import sde_grid_arrays  # noqa: E402

bench.torch = torch          # bench.py binds its module globals in main(); _timed's synchronisation needs torch
B, T = 32, 16


def _nets(kind):
    torch.manual_seed(0)
    np.random.seed(0)
    gen = G.VideoGeneratorSDE(1, 50, 0, 16, 16) if kind == "sde" else G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16)
    dv, di = G.VideoDiscriminator(1, ksize=2, ndf=64), G.PatchImageDiscriminator(1, ndf=64)
    return gen.cuda(), dv.cuda(), di.cuda()


def _alternate(fns, steps, warmup, rounds):
    """{name: median ms per step over `rounds` rounds}, the callables taking turns every round"""
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            dt = bench._timed(fn, steps, warmup if r == 0 else 2, False)
            out[k].append(1e3 * dt / steps)
    return {k: statistics.median(v) for k, v in out.items()}, out


def _events(fn, reps=20, warmup=3):
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


def _kernels(N):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(N)
    dev = dict(device="cuda")
    pre = [torch.randn(s, generator=g).cuda() * 0.3 for s in [(64, 16), (64,), (16, 64), (16,)]]
    mlp = lambda: [torch.randn(s, generator=g).cuda() * 0.3 for s in [(16, 16), (16,), (16, 16), (16,)]]  # noqa: E731
    ode_p, drift, diff = mlp(), mlp(), mlp()
    res = {}
    # ODE: rk4 on linspace(0, 1, T), the reference's call
    tt = torch.linspace(0, 1, T).float()
    dt = (tt[1:] - tt[:-1]).cuda()
    x = torch.randn(N, 16, generator=g).cuda()
    z = torch.empty(N * T, 96, **dev)                  # the generator's latent-row layout (Z_COLS)
    traj = torch.empty(N, T, 16, **dev)
    gz = torch.randn(N * T, 96, generator=g).cuda()
    prm = L.OdeParams(*[p.data_ptr() for p in pre + ode_p])
    work = torch.empty(L.lib().gode_ode_bwd_work_size(N), **dev)
    grads = torch.empty(L.ODE_NPARAM, **dev)
    fop = L.OdeFwdOp(p=prm, x=x.data_ptr(), dt=dt.data_ptr(), z=z.data_ptr(), traj=traj.data_ptr(), N=N, T=T,
                     substeps=1, prenet=1, zcols=96)
    bop = L.OdeBwdOp(p=prm, x=x.data_ptr(), traj=traj.data_ptr(), dt=dt.data_ptr(), gz=gz.data_ptr(),
                     work=work.data_ptr(), grads=grads.data_ptr(), N=N, T=T, substeps=1, prenet=1, zcols=96)
    res["ode_fwd_us"] = _events(lambda: L.run_one(fop, st))
    res["ode_bwd_us"] = _events(lambda: L.run_one(bop, st))
    # SDE: Euler-Maruyama, dt = 2.5e-2
    gd = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in sde_grid_arrays(T, 2.5e-2).items()}
    S = gd["S"]
    xs = torch.randn(1 + S, N, 16, generator=g).cuda()
    states = torch.empty(N, S + 1, 16, **dev)
    swork = torch.empty(L.lib().gode_sde_bwd_work_size(N), **dev)
    sgrads = torch.empty(L.SDE_NPARAM, **dev)
    sp = L.SdeParams(*[p.data_ptr() for p in pre + drift + diff])
    common = dict(p=sp, x=xs.data_ptr(), dt=gd["dt"].data_ptr(), sqrt_dt=gd["sqrt_dt"].data_ptr(),
                  emit_at=gd["emit_at"].data_ptr(), emit_w0=gd["w0"].data_ptr(), emit_w1=gd["w1"].data_ptr(), N=N, T=T,
                  S=S, prenet=1, zcols=96)
    sfop = L.SdeFwdOp(z=z.data_ptr(), states=states.data_ptr(), **common)
    sbop = L.SdeBwdOp(states=states.data_ptr(), gz=gz.data_ptr(), work=swork.data_ptr(), grads=sgrads.data_ptr(),
                      **common)
    res["sde_fwd_us"] = _events(lambda: L.run_one(sfop, st))
    res["sde_bwd_us"] = _events(lambda: L.run_one(sbop, st))
    res["sde_steps"] = S
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G.limit_host_threads()
    gens = {k: _nets(k) for k in ("ode", "sde")}

    def sampler(gen):
        def fn():
            with torch.no_grad():
                gen.sample_videos(B)
        return fn

    sv, sv_rounds = _alternate({k: sampler(v[0]) for k, v in gens.items()}, a.steps, a.warmup, a.rounds)
    rng = torch.Generator().manual_seed(1)
    imgs = [torch.rand(B, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
    vids = [torch.rand(B, T, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
    trainers = {k: G.GanTrainer(*v) for k, v in gens.items()}
    it_steps = max(a.steps // 3, 5)
    it, it_rounds = _alternate({k: (lambda tr=tr: tr.step(imgs, vids)) for k, tr in trainers.items()}, it_steps,
                               max(a.warmup // 3, 3), a.rounds)
    kernels = {N: _kernels(N) for N in (32, 128, 512, 2048, 8192, 32768, 65536)}
    out = dict(device=torch.cuda.get_device_name(0), batch=B, T=T, steps=a.steps, rounds=a.rounds,
               sample_videos_ms={k: round(v, 4) for k, v in sv.items()},
               videos_per_s={k: round(B * 1e3 / v, 1) for k, v in sv.items()},
               sample_videos_ratio_sde_over_ode=round(sv["sde"] / sv["ode"], 4),
               iteration_ms={k: round(v, 3) for k, v in it.items()},
               iteration_ratio_sde_over_ode=round(it["sde"] / it["ode"], 4),
               rounds_ms=dict(sample_videos=sv_rounds, iteration=it_rounds),
               kernels_us={str(N): {k: round(v, 2) for k, v in r.items()} for N, r in kernels.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
