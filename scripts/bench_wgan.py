"""The Wasserstein loss and the fused parameter noise against the BCE iteration in ONE process, alternating round by
round so that clock and thermal drift hit every configuration alike; timed with bench.py's _timed.

  python scripts/bench_wgan.py [--steps 30] [--warmup 10] [--rounds 5] [--out FILE]

Configurations (GanTrainer at batch 32, ngf = ndf = 64, d_iters 2, each on networks of its own):
  bce          loss="bce"                                  (mnist_moco_ode.py)
  bce_noise    loss="bce", param_noise=1e-5                (mnist_moco_ode_noise.py)
  wgan_noise   loss="wasserstein", param_noise=1e-4        (mnist_moco_ode_wgan.py)
  stock_noise  loss="bce", and after every optimiser step torch's randn_like / mul / add_ per parameter (eager only:
               what a loop of one's own costs without the fused kernel)
each eager and with graph=True.  Prints one JSON object: ms per iteration (median of rounds) and the ratios; the
optimiser launches alone (adam_multi vs adam_noise_multi over the generator's 44 tensors, HIP events).
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

bench.torch = torch          # bench.py binds its module globals in main(); _timed's synchronisation needs torch
B, T = 32, 16
CONFIGS = {"bce": dict(), "bce_noise": dict(param_noise=1e-5), "wgan_noise": dict(loss="wasserstein", param_noise=1e-4),
           "stock_noise": dict()}


def _nets():
    torch.manual_seed(0)
    np.random.seed(0)
    gen, dv, di = G.build_mnist()
    return gen.cuda(), dv.cuda(), di.cuda()


def _stock_noise(tr, sigma=1e-5):
    """wrap every optimiser's step: FusedAdam, then add_noise as the reference writes it"""
    for opt in (tr.gen_opt, tr.vid_opt, tr.img_opt):
        inner = opt.step

        def step(*a, _inner=inner, _opt=opt, **k):
            _inner(*a, **k)
            with torch.no_grad():
                for p in _opt.param_groups[0]["params"]:
                    p.add_(torch.randn_like(p) * sigma)
        opt.step = step
    return tr


def _alternate(fns, steps, warmup, rounds):
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


def _optimiser_launches():
    """one optimiser step over the generator's parameters (gradients on all but the dead GRU cell), with and without
    noise; back-to-back launches, so the GPU time per launch"""
    gen, _, _ = _nets()
    for p in gen.parameters():
        p.grad = None if any(p is q for q in gen.recurrent.parameters()) else torch.randn_like(p) * 1e-3
    res = {}
    for name, kw in (("adam_multi", {}), ("adam_noise_multi", dict(noise_sigma=1e-5, noise_seed=1))):
        opt = G.FusedAdam(gen.parameters(), **kw)
        res[name + "_us"] = _events(opt.step)
    res["ratio"] = res["adam_noise_multi_us"] / res["adam_multi_us"]
    res["params"] = sum(p.numel() for p in gen.parameters())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G.limit_host_threads()
    rng = torch.Generator().manual_seed(1)
    imgs = [torch.rand(B, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
    vids = [torch.rand(B, T, 1, 28, 28, generator=rng).cuda() for _ in range(2)]
    fns = {}
    for name, kw in CONFIGS.items():
        for graph in (False, True):
            if name == "stock_noise" and graph:
                continue
            tr = G.GanTrainer(*_nets(), graph=graph, **kw)
            if name == "stock_noise":
                _stock_noise(tr)
            fns[f"{name}/{'graph' if graph else 'eager'}"] = (lambda tr=tr: tr.step(imgs, vids))
    it_steps = max(a.steps // 3, 5)
    it, it_rounds = _alternate(fns, it_steps, max(a.warmup // 3, 3), a.rounds)
    opt = _optimiser_launches()
    ratio = lambda x, y: round(it[x] / it[y], 4)  # noqa: E731
    out = dict(device=torch.cuda.get_device_name(0), batch=B, T=T, steps=it_steps, rounds=a.rounds,
               iteration_ms={k: round(v, 3) for k, v in it.items()},
               ratio_wgan_noise_over_bce=dict(eager=ratio("wgan_noise/eager", "bce/eager"),
                                              graph=ratio("wgan_noise/graph", "bce/graph")),
               ratio_bce_noise_over_bce=dict(eager=ratio("bce_noise/eager", "bce/eager"),
                                             graph=ratio("bce_noise/graph", "bce/graph")),
               ratio_stock_noise_over_bce_noise_eager=ratio("stock_noise/eager", "bce_noise/eager"),
               optimiser_step_gen_us={k: round(v, 2) if isinstance(v, float) else v for k, v in opt.items()},
               rounds_ms=it_rounds)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
