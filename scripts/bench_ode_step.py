"""Times the four parameter updates of one RK4 generator step at the MNIST generator's real parameter list: the fused
path (one gode_ode_step launch per stage) against the reference's per-tensor update expressions (ode_training.py:143-199)
run as torch ops on the same GPU tensors.  Gradients are fixed random tensors: only the updates are timed.

  python scripts/bench_ode_step.py [--reps 200]

Prints one JSON line: microseconds per step (4 updates) and launches per step for both paths (the torch path's launches
are counted from the operators of its expressions).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_ode_amd as G  # noqa: E402
from gan_ode_amd.ode_training import _Device, stage_plan  # noqa: E402


def per_tensor_updates(params, g, lr):
    """The reference's four updates, tensor by tensor (None gradients skipped)."""
    g1, g2, g3, g4 = g
    with torch.no_grad():
        for p, a in zip(params, g1):
            if a is not None:
                p.add_(lr / 2 * (-a))
        for p, a, b in zip(params, g1, g2):
            if a is not None:
                p.add_(lr / 2 * (a - b))
        for p, b, c in zip(params, g2, g3):
            if b is not None:
                p.add_(lr * (b / 2 - c))
        for p, a, b, c, d in zip(params, g1, g2, g3, g4):
            if a is not None:
                p.add_(lr * (-a / 6 - b / 3 + 2 * c / 3 - d / 6))


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


# elementwise launches of the four per-tensor expressions above, by their operators: neg mul add_ | sub mul add_ |
# div sub mul add_ | neg div, div, sub, mul div, add, div, sub, mul, add_
PER_TENSOR_LAUNCHES = 3 + 3 + 4 + 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    gen, _, _ = G.build_mnist()
    gen.cuda()
    params = list(gen.parameters())
    lr = 0.02
    gen_ = torch.Generator(device="cuda").manual_seed(0)
    grads = [[None if n.startswith("recurrent.") else torch.randn(p.shape, device="cuda", generator=gen_) * 1e-3
              for n, p in gen.named_parameters()] for _ in range(4)]
    live = [i for i, p in enumerate(params) if p.numel() > 0]
    dev = _Device(params)
    plan = stage_plan("rk4", lr, 0.0, False)
    by_k = {k + 1: [grads[k][i] for i in live] for k in range(4)}

    def fused():
        for s, (coefs, _, _) in enumerate(plan, start=1):
            dev.step("s%d" % s, coefs, {k: by_k[k] for k in coefs})

    out = dict(tensors=len(params), with_gradient=sum(g is not None for g in grads[0]),
               floats=sum(p.numel() for p in params),
               fused_us=timed(fused, a.reps), per_tensor_us=timed(lambda: per_tensor_updates(params, grads, lr), a.reps),
               fused_launches=4, per_tensor_launches=PER_TENSOR_LAUNCHES * sum(g is not None for g in grads[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
