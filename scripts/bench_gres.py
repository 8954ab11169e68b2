"""The stage-1 block (GResBlock on libgode) against its plain-torch restatement (tests/gres_ref.py, stock
torch / MIOpen) on the same GPU, alternating round by round so that clock and thermal drift hit both alike.

  python scripts/bench_gres.py [--steps 10] [--warmup 3] [--rounds 3] [--out FILE]

Two shapes: the reference demo's block (3 -> 100 channels, BT = 80, 64x64 -> 128x128, n_class 96) and a 64 -> 64 block at
32x32 (BT = 80).  Per shape: ms per forward (no_grad) and per forward + backward, HIP events, median of rounds, and the
ratio stock / libgode (> 1: libgode is faster).  Prints one JSON object.  No threshold is fixed here.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

import gan_ode_amd as G  # noqa: E402
import gres_ref  # noqa: E402

SHAPES = {"demo_3_100_64": dict(cin=3, cout=100, bt=80, hw=64), "mid_64_64_32": dict(cin=64, cout=64, bt=80, hw=32)}


def _events(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _pair(shape):
    torch.manual_seed(0)
    ref = gres_ref.GResBlock(shape["cin"], shape["cout"])
    hip = G.GResBlock(shape["cin"], shape["cout"], [3, 3])
    hip.load_state_dict(ref.state_dict())
    return hip.cuda(), ref.cuda()


def _fns(blk, x, cond, gy):
    def fwd():
        with torch.no_grad():
            blk(x, cond)

    def fwd_bwd():
        xr = x.detach().requires_grad_(True)
        blk.zero_grad(set_to_none=True)
        blk(xr, cond).backward(gy)
    return fwd, fwd_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    G.limit_host_threads()
    res = {}
    for name, s in SHAPES.items():
        hip, ref = _pair(s)
        g = torch.Generator().manual_seed(1)
        x = torch.rand(s["bt"], s["cin"], s["hw"], s["hw"], generator=g).cuda()
        cond = torch.rand(s["bt"], 96, generator=g).cuda()
        gy = torch.randn(s["bt"], s["cout"], 2 * s["hw"], 2 * s["hw"], generator=g).cuda()
        fns = {"hip": _fns(hip, x, cond, gy), "torch": _fns(ref, x, cond, gy)}
        t = {k: {"fwd": [], "fwd_bwd": []} for k in fns}
        for r in range(a.rounds):
            for k, (f, fb) in fns.items():
                t[k]["fwd"].append(_events(f, a.steps, a.warmup if r == 0 else 1))
                t[k]["fwd_bwd"].append(_events(fb, a.steps, a.warmup if r == 0 else 1))
        med = {k: {m: statistics.median(v) for m, v in d.items()} for k, d in t.items()}
        res[name] = dict(shape=s, ms=med, rounds=t,
                         ratio_torch_over_hip={m: med["torch"][m] / med["hip"][m] for m in ("fwd", "fwd_bwd")})
        del hip, ref, x, cond, gy
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
