"""Differentiable augmentation (GanTrainer(diffaug=...)) against the plain iteration in ONE process,
alternating round by round so that clock and thermal drift hit every configuration alike; timed with bench.py's _timed.

  python scripts/bench_diffaug.py [--steps 30] [--warmup 10] [--rounds 5] [--out FILE]

Configurations (GanTrainer, ngf = ndf = 64, d_iters 2, each on networks of its own, eager schedule):
  mnist   build_mnist, batch 32, policy off and 'color,translation,cutout'
  ucf     build_ucf, batch 16, policy off and 'color,translation,cutout'
Prints one JSON object: ms per iteration (median of rounds), the on / off ratios, and gode_diffaug alone on the two
configurations' video batches, forward and backward, with the whole policy (mask 31: sum launch + apply launch, 12 B per
element) and with the data-movement part alone (mask 24: one launch, 8 B per element) -- HIP events over back-to-back
launches: time, achieved bytes/s on the algorithmic bytes, and that rate over the HBM rate a streaming kernel reaches
(6.3 TB/s).
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
POLICY = "color,translation,cutout"
HBM_BYTES_PER_S = 6.3e12


def _nets(build):
    torch.manual_seed(0)
    np.random.seed(0)
    return [m.cuda() for m in build()]


def _alternate(fns, steps, warmup, rounds):
    out = {k: [] for k in fns}
    for r in range(rounds):
        for k, fn in fns.items():
            dt = bench._timed(fn, steps, warmup if r == 0 else 2, False)
            out[k].append(1e3 * dt / steps)
    return {k: statistics.median(v) for k, v in out.items()}, out


def _op_alone(reps=200):
    """gode_diffaug over a video batch [B, 16, H, W, C] read as the generator's channels-last view."""
    res = {}
    st = torch.cuda.current_stream().cuda_stream
    for cfg, (_, B, Cc, H) in CONFIGS.items():
        x = torch.rand(B, 16, H, H, Cc, device="cuda") * 2 - 1
        out = torch.empty_like(x)
        v = x.permute(0, 4, 1, 2, 3)
        for mask in (31, 24):
            nwork = L.lib().gode_diffaug_work_size(B, 16, H, H, mask)
            work = torch.empty(max(1, nwork // 2), dtype=torch.float64, device="cuda")
            for backward in (0, 1):
                op = L.DiffAugOp(x=x.data_ptr(), out=out.data_ptr(), work=work.data_ptr(),
                                 xs=(C.c_int64 * 5)(v.stride(0), v.stride(2), v.stride(3), v.stride(4), v.stride(1)), seed=1, g0=0,
                                 N=B, C=Cc, D=16, H=H, W=H, mask=mask, backward=backward, stream=1, call=0)
                for _ in range(10):
                    L.check(L.lib().gode_diffaug(C.byref(op), st), "gode_diffaug")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    L.check(L.lib().gode_diffaug(C.byref(op), st), "gode_diffaug")
                e1.record()
                torch.cuda.synchronize()
                us = 1e3 * e0.elapsed_time(e1) / reps
                nbytes = 4 * x.numel() * (3 if mask & 4 else 2)
                res[f"{cfg}/mask{mask}/{'bwd' if backward else 'fwd'}"] = dict(
                    us=round(us, 2), launches=2 if nwork else 1, bytes=nbytes, GBps=round(nbytes / us / 1e3, 1),
                    hbm_fraction=round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3))
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
        for policy in (None, POLICY):
            tr = G.GanTrainer(*_nets(build), diffaug=policy, diffaug_seed=1)
            fns[f"{cfg}/{'on' if policy else 'off'}"] = (lambda tr=tr, imgs=imgs, vids=vids: tr.step(imgs, vids))
    it, it_rounds = _alternate(fns, a.steps, a.warmup, a.rounds)
    ratios = {cfg: round(it[f"{cfg}/on"] / it[f"{cfg}/off"], 4) for cfg in CONFIGS}
    out = dict(device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds, policy=POLICY,
               iteration_ms={k: round(v, 3) for k, v in it.items()}, ratio_on_over_off=ratios,
               rounds_ms={k: [round(x, 3) for x in v] for k, v in it_rounds.items()}, op_alone=_op_alone())
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
