"""Writes tests/golden/gres_tiny_<case>.npz: the reference's own GResBlock (stage1/GResBlock.py) run on the CPU under fixed
seeds.  Per case: the initial state_dict (sd0/), x, condition and the upstream gradient gy; the outputs of two successive
train-mode forwards (y1, y2: the second sees the carried u, v and running statistics); every gradient after the first (g/,
g/x, g/condition); the state_dict after the two (sd2/); an eval-mode forward after them (y_eval).  Data only: no reference
source enters the repository.

  python scripts/make_gres_golden.py /path/to/reference

ReLU kinks are a condition, not a tolerance: every pre-activation of the forward whose gradients are recorded (the first) must
stay at least MARGIN of its tensor's max-abs away from zero, otherwise the next seed is tried; the smallest ratio is recorded
as `margin`.  (The later forwards only contribute outputs, which are continuous across a kink; with their ~50 000 further
values in case B no seed would pass.)  spread/<name> is the
distance of the reference's fp32 result from its own fp64 run, relative to the fp64 max-abs.  conv0's bias sits in front of a
train-mode BatchNorm in the bn cases: its gradient is zero in exact arithmetic and the fp32 reference returns rounding
noise, so scale/g/conv0.module.bias records the natural scale of that sum (max over channels of sum |g| of conv0's output).
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
from gres_cases import CASES  # noqa: E402

MARGIN = 1e-4


def run(mod, case, seed, dtype):
    """One pass of the recipe in `dtype`; returns (arrays, smallest pre-activation ratio)."""
    torch.manual_seed(seed)
    blk = mod.GResBlock(case["cin"], case["cout"], [3, 3], n_class=case["n_class"], bn=case["bn"],
                        upsample_factor=case["up"], downsample_factor=case["down"])
    out = {f"sd0/{k}": v.clone().numpy() for k, v in blk.state_dict().items()}
    x = torch.randn(case["bt"], case["cin"], *case["map"])
    cond = torch.rand(case["bt"], case["n_class"])
    blk = blk.to(dtype)
    pre, gsum = [], {}

    def grab(_m, _i, o):
        pre.append(o.detach())
    hooks = []
    if blk.bn:
        hooks += [blk.CBNorm1.register_forward_hook(grab), blk.CBNorm2.register_forward_hook(grab)]
    else:
        hooks.append(blk.conv0.register_forward_hook(grab))

    def conv0_grad_scale(_m, _i, o):
        if o.requires_grad:
            o.register_hook(lambda g: gsum.update(v=float(g.abs().sum((0, 2, 3)).max())))
    hooks.append(blk.conv0.register_forward_hook(conv0_grad_scale))
    xr, cr = x.to(dtype).clone().requires_grad_(True), cond.to(dtype).clone().requires_grad_(True)
    if not blk.bn:
        pre.append(xr.detach())
    y1 = blk(xr, cr)
    ratio = min(float(t.abs().min() / t.abs().max()) for t in pre)
    if ratio < MARGIN and dtype == torch.float32:
        return None, ratio
    gy = torch.randn(y1.shape).to(dtype)
    y1.backward(gy)
    out.update(x=x.numpy(), condition=cond.numpy(), gy=gy.float().numpy(), y1=y1.detach())
    out["g/x"], out["g/condition"] = xr.grad.clone(), (cr.grad.clone() if cr.grad is not None else None)
    for k, p in blk.named_parameters():
        if p.grad is not None:
            out[f"g/{k}"] = p.grad.clone()
    out["scale/g/conv0.module.bias"] = np.float64(gsum["v"])
    out["y2"] = blk(xr.detach(), cr.detach()).detach()
    for k, v in blk.state_dict().items():
        out[f"sd2/{k}"] = v.clone()
    blk.eval()
    out["y_eval"] = blk(xr.detach(), cr.detach()).detach()
    for h in hooks:
        h.remove()
    return {k: v for k, v in out.items() if v is not None}, ratio


def main(ref):
    warnings.filterwarnings("ignore")
    spec = importlib.util.spec_from_file_location("ref_gresblock", os.path.join(ref, "stage1", "GResBlock.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name, case in CASES.items():
        seed = case["seed"]
        while True:
            a32, ratio = run(mod, case, seed, torch.float32)
            if ratio >= MARGIN:
                break
            seed += 1
        a64, _ = run(mod, case, seed, torch.float64)
        arrays = {"seed": np.int64(seed), "margin": np.float64(ratio)}
        for k, v in a32.items():
            arrays[k] = v.numpy() if isinstance(v, torch.Tensor) else v
            if k[0] in "yg" and k != "gy" and isinstance(v, torch.Tensor):
                w = a64[k]
                arrays[f"spread/{k}"] = np.float64((v.double() - w).abs().max() / w.abs().max().clamp_min(1e-300))
        path = os.path.join(GOLDEN, f"gres_tiny_{name}.npz")
        np.savez_compressed(path, **arrays)
        worst = max((float(v), k) for k, v in arrays.items() if k.startswith("spread/") and k != "spread/g/conv0.module.bias")
        print(f"{name}: seed {seed}, margin {ratio:.2e}, worst spread {worst[0]:.1e} ({worst[1]}), "
              f"conv0 bias grad spread {float(arrays.get('spread/g/conv0.module.bias', 0)):.1e}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
