"""The discriminators' instance noise (use_noise=True) against the noise-free iteration in ONE process,
alternating round by round so that clock and thermal drift hit every configuration alike; timed with bench.py's _timed.

  python scripts/bench_dnoise.py [--steps 30] [--warmup 10] [--rounds 5] [--out FILE]

Configurations (GanTrainer, ngf = ndf = 64, d_iters 2, each on networks of its own), eager and graph=True:
  mnist   build_mnist, batch 32, sigma 0 (noise-free) and 0.1
  ucf     build_ucf, batch 16, sigma 0 (noise-free) and 0.1
Prints one JSON object: ms per iteration (median of rounds), the noisy / noise-free ratios, and the apply-mode op alone on
the MNIST video discriminator's largest noised tensor (HIP events over back-to-back launches: time and achieved HBM
bandwidth at 8 B per element).
"""
import argparse
import ctypes as C
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
CONFIGS = {"mnist": (G.build_mnist, 32, 1, 28), "ucf": (G.build_ucf, 16, 3, 64)}


def _nets(build, sigma):
    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(use_noise=True, noise_sigma=sigma) if sigma else {}
    return [m.cuda() for m in build(**kw)]


def _alternate(fns, steps, warmup, rounds):
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            dt = bench._timed(fn, steps, warmup if r == 0 else 2, False)
            out[k].append(1e3 * dt / steps)
    return {k: statistics.median(v) for k, v in out.items()}, out


def _op_alone(reps=50):
    """gode_dnoise (apply mode, LeakyReLU, no BatchNorm) over y[0] of the MNIST video discriminator at batch 32 (ndf 64,
    ksize 2): [32*15*14*14, 64] -> the noisy input of layer 1, against gode_bn_apply on the same tensor."""
    M, Cc = 32 * 15 * 14 * 14, 64
    y = torch.randn(M, Cc, device="cuda")
    out = torch.empty_like(y)
    ops = {"dnoise": L.DnoiseOp(x=y.data_ptr(), out=out.data_ptr(), M=M, C=Cc, act=L.ACT_LRELU, seed=1, stream=1, layer=1,
                                sigma=0.1),
           "bn_apply": L.BnApplyOp(y=y.data_ptr(), out=out.data_ptr(), M=M, C=Cc, act=L.ACT_LRELU)}
    res = {}
    for name, op in ops.items():
        fn = getattr(L.lib(), "gode_" + name)
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(5):
            L.check(fn(C.byref(op), st), name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            L.check(fn(C.byref(op), st), name)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        res[name] = dict(us=round(us, 2), GBps=round(8 * M * Cc / us / 1e3, 1))
    res["elements"] = M * Cc
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    G.limit_host_threads()
    fns = {}
    for cfg, (build, B, Cc, H) in CONFIGS.items():
        rng = torch.Generator().manual_seed(1)
        imgs = [torch.rand(B, Cc, H, H, generator=rng).cuda() for _ in range(2)]
        vids = [torch.rand(B, 16, Cc, H, H, generator=rng).cuda() for _ in range(2)]
        for sigma in (0.0, 0.1):
            for graph in (False, True):
                tr = G.GanTrainer(*_nets(build, sigma), graph=graph)
                fns[f"{cfg}/sigma{sigma}/{'graph' if graph else 'eager'}"] = \
                    (lambda tr=tr, imgs=imgs, vids=vids: tr.step(imgs, vids))
    it, it_rounds = _alternate(fns, a.steps, a.warmup, a.rounds)
    ratios = {f"{cfg}/{mode}": round(it[f"{cfg}/sigma0.1/{mode}"] / it[f"{cfg}/sigma0.0/{mode}"], 4)
              for cfg in CONFIGS for mode in ("eager", "graph")}
    out = dict(device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds,
               iteration_ms={k: round(v, 3) for k, v in it.items()}, ratio_noisy_over_noise_free=ratios,
               rounds_ms={k: [round(x, 3) for x in v] for k, v in it_rounds.items()}, op_alone=_op_alone())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
