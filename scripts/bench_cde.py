"""The Neural-CDE generator (VideoGeneratorCDE) against the ODE generator (VideoGeneratorMNISTODE) in ONE process,
alternating round by round so that clock and thermal drift hit both alike; timed with bench.py's _timed.

  python scripts/bench_cde.py [--steps 20] [--warmup 5] [--rounds 5] [--out FILE]

Prints one JSON object:
  sample_videos: ms per sample_videos(32) call (no_grad, train-mode BatchNorm, ngf=64) and videos/s, median of rounds;
  iteration:     ms per GanTrainer.step at batch 32 (d_iters 2, ndf=64), median of rounds;
  kernels:       the CDE latent kernels alone (forward; backward incl. its reduction) at N = 32 and 2048, HIP events,
                 with the accepted and trial steps of that solve, on the seeded initial weights at the default tolerances.
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
from gan_ode_amd.modules import cde_time_slopes  # noqa: E402

bench.torch = torch          # bench.py binds its module globals in main(); _timed's synchronisation needs torch
B, T = 32, 16


def _nets(kind):
    torch.manual_seed(0)
    np.random.seed(0)
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16) if kind == "cde" else G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16)
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


def _kernels(gen, N, S_cap=512):
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(N)
    dev = dict(device="cuda")
    _, prm = gen._param_list()
    x = torch.randn(N, T, generator=g).cuda()
    tslope = cde_time_slopes(T).cuda()
    z = torch.empty(N * T, 96, **dev)                  # the generator's latent-row layout (Z_COLS)
    gz = torch.randn(N * T, 96, generator=g).cuda()
    states = torch.empty(int(L.lib().gode_cde_state_size(N, S_cap)), **dev)
    sched = torch.empty(2 * S_cap, dtype=torch.float64, **dev)
    counts = torch.zeros(2, dtype=torch.int32, **dev)
    ns = int(L.lib().gode_cde_sync_size(N))
    sync = torch.zeros(max(ns, 1), dtype=torch.int32, **dev)
    work = torch.empty(int(L.lib().gode_cde_bwd_work_size(N)), **dev)
    grads = torch.empty(L.CDE_NPARAM, **dev)
    p = L.CdeParams(*[q.data_ptr() for q in prm])
    common = dict(p=p, x=x.data_ptr(), tslope=tslope.data_ptr(), sel_t=None, states=states.data_ptr(),
                  sched=sched.data_ptr(), counts=counts.data_ptr(), N=N, T=T, S_cap=S_cap, zcols=96)
    fop = L.CdeFwdOp(content=None, z=z.data_ptr(), sync=sync.data_ptr() if ns else None, rtol=gen.cde_rtol,
                     atol=gen.cde_atol, **common)
    bop = L.CdeBwdOp(gz=gz.data_ptr(), work=work.data_ptr(), grads=grads.data_ptr(), accumulate=0, **common)
    res = {"cde_fwd_us": _events(lambda: L.run_one(fop, st))}
    acc, trials = [int(v) for v in counts.cpu()]
    if acc < 0:
        raise RuntimeError(f"N={N}: the solve stopped ({acc}, {trials})")
    res["cde_bwd_us"] = _events(lambda: L.run_one(bop, st))
    res["accepted_steps"], res["trial_steps"] = acc, trials
    res["fwd_us_per_trial"] = res["cde_fwd_us"] / trials
    res["bwd_us_per_accepted"] = res["cde_bwd_us"] / acc
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G.limit_host_threads()
    gens = {k: _nets(k) for k in ("ode", "cde")}

    def sampler(gen):
        def fn():
            with torch.no_grad():
                gen.sample_videos(B)
        return fn

    sv, sv_rounds = _alternate({k: sampler(v[0]) for k, v in gens.items()}, a.steps, a.warmup, a.rounds)
    solves = dict(zip(("accepted", "trials"), gens["cde"][0]._pool.get((B, T, False), None).last_counts))
    rng = torch.Generator().manual_seed(1)
    imgs = [torch.rand(B, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
    vids = [torch.rand(B, T, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
    trainers = {k: G.GanTrainer(*v) for k, v in gens.items()}
    it_steps = max(a.steps // 3, 5)
    it, it_rounds = _alternate({k: (lambda tr=tr: tr.step(imgs, vids)) for k, tr in trainers.items()}, it_steps,
                               max(a.warmup // 3, 3), a.rounds)
    torch.manual_seed(0)
    np.random.seed(0)
    init = G.VideoGeneratorCDE(1, 50, 0, 16, 16).cuda()       # seeded initial weights (the trainer has moved gens')
    kernels = {N: _kernels(init, N) for N in (32, 2048)}
    out = dict(device=torch.cuda.get_device_name(0), batch=B, T=T, steps=a.steps, rounds=a.rounds,
               rtol=init.cde_rtol, atol=init.cde_atol,
               sample_videos_ms={k: round(v, 4) for k, v in sv.items()},
               videos_per_s={k: round(B * 1e3 / v, 1) for k, v in sv.items()},
               sample_videos_solve_steps=solves,
               iteration_ms={k: round(v, 3) for k, v in it.items()},
               rounds_ms=dict(sample_videos=sv_rounds, iteration=it_rounds),
               kernels={str(N): {k: round(v, 3) for k, v in r.items()} for N, r in kernels.items()})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
