"""Times stage 2's CIFAR DCGAN at the notebook's size (B = 64, nz = 128, ngf = ndf = 64, 32x32 RGB): one Euler `dis_img` step plus
one `gen` step of GANODETrainer (reg = 0) with the notebook's closures on synthetic images, on the HIP modules
(gan_ode_amd.dcgan) and on the same two networks as stock torch modules with nn.BCEWithLogitsLoss on the same GPU -- the
reference's own implementation, the yardstick.

  python scripts/bench_dcgan.py [--blocks 7] [--reps 20] [--profile-steps N] [--layer-times]

Device events around `reps` step pairs, after a warm-up; blocks of the two paths alternate in one process.  Prints one JSON
line: the per-block times (microseconds per step pair), median and range of both paths, and their ratio.
--profile-steps N: runs N step pairs of the HIP path only after the warm-up and prints nothing else -- for
`rocprofv3 --kernel-trace --stats -- python scripts/bench_dcgan.py --profile-steps 20`.
--layer-times: one step pair of the HIP path with every library op launched on its own between two device events
(_lib.TRACE); prints one JSON line per op, for the products with their geometry and the kernel family the launch plan gives them.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_ode_amd as G  # noqa: E402
from gan_ode_amd import _lib as L  # noqa: E402
from gan_ode_amd import dcgan  # noqa: E402

BS, NZ, NGF, NDF, NC = 64, 128, 64, 64, 3
WARMUP = 10


class StockGenerator(nn.Module):
    def __init__(self, ngpu, nz=NZ, ngf=NGF, nc=NC):
        super().__init__()
        self.ngf = ngf
        self.project = nn.Conv2d(nz, ngf * 8 * 4 * 4, 1, 1, 0, bias=False)
        layers = []
        for c in (ngf * 8, ngf * 4, ngf * 2):
            layers += [nn.ConvTranspose2d(c, c // 2, 4, 2, 1, bias=False), nn.BatchNorm2d(c // 2), nn.ReLU(True)]
        self.main = nn.Sequential(*layers, nn.Conv2d(ngf, nc, 3, 1, 1, bias=False), nn.Tanh())

    def forward(self, input):
        return self.main(self.project(input).view(-1, self.ngf * 8, 4, 4))


class StockDiscriminator(nn.Module):
    def __init__(self, ngpu, ndf=NDF, nc=NC):
        super().__init__()
        ch = (nc, ndf, ndf, ndf * 2, ndf * 2, ndf * 4, ndf * 4, ndf * 8)
        layers = []
        for ci, co, (k, s, p) in zip(ch[:-1], ch[1:], dcgan.Discriminator.LAYERS):
            layers += [nn.Conv2d(ci, co, k, s, p, bias=False), nn.LeakyReLU(0.1, inplace=True)]
        self.main = nn.Sequential(*layers, nn.Conv2d(ndf * 8, 1, 4, 1, 0, bias=False))

    def forward(self, input):
        return self.main(input).view(-1, 1).squeeze(1)


def xavier(m):
    name = type(m).__name__
    if "Conv" in name:
        nn.init.xavier_uniform_(m.weight, gain=1.0)
    elif "BatchNorm" in name:
        nn.init.normal_(m.weight, 1.0, 0.02)
        nn.init.zeros_(m.bias)


def make_path(gen_cls, dis_cls, criterion, data):
    torch.manual_seed(97382)
    gen, dis = gen_cls(1), dis_cls(1)
    gen.apply(xavier), dis.apply(xavier)
    gen, dis = gen.cuda(), dis.cuda()
    device = "cuda"

    def dis_loss(data):
        dis.zero_grad()
        real = data[0].to(device)
        n = real.size(0)
        loss_real = criterion(dis(real), torch.full((n,), 1, dtype=real.dtype, device=device))
        fake = gen(torch.randn(n, NZ, 1, 1, device=device))
        return loss_real + criterion(dis(fake), torch.full((n,), 0, dtype=real.dtype, device=device))

    def gen_loss():
        gen.zero_grad()
        noise = torch.randn(BS, NZ, 1, 1, device=device)
        label = torch.full((BS,), 1, dtype=float, device=device)
        return criterion(dis(gen(noise)), label)

    tr = G.GANODETrainer(gen.parameters(), dis.parameters(), None, gen_loss, dis_loss, None, lr=0.01, reg=0.0, method="euler")

    def pair():
        tr.step(data, model="dis_img")
        tr.step(model="gen")
    return pair


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


FAMILIES = ("tiled GEMM", "LDS-patch FPROP", "pointwise", "tiny-K", "dot")


def layer_times(pair):
    L.TRACE = []
    pair()
    torch.cuda.synchronize()
    trace, L.TRACE = L.TRACE, None
    for op, e0, e1 in trace:
        row = dict(op=op if isinstance(op, str) else type(op).__name__, us=round(e0.elapsed_time(e1) * 1e3, 1))
        if isinstance(op, (L.IgemmOp, L.WgradOp, L.PackOp)):
            g = op.g
            row["geom"] = "N%d %dx%dx%d->%dx%dx%d k%d s%d p%d" % (g.N, g.Ci, g.Hi, g.Wi, g.Co, g.Ho, g.Wo, g.kh, g.sh, g.ph)
        if isinstance(op, L.IgemmOp):
            row["dir"] = "FPROP" if op.dir == L.FPROP else "DGRAD"
            row["family"] = FAMILIES[L.lib().gode_igemm_family(ctypes.byref(op))]
        elif hasattr(op, "M") and hasattr(op, "C"):
            row["geom"] = "M%d C%d" % (op.M, op.C)
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--layer-times", action="store_true")
    a = ap.parse_args()
    G.limit_host_threads()
    torch.backends.cudnn.benchmark = True           # as the notebook sets it: the stock path picks its convolution kernels by trial
    # a loader step's `data`: images on the host (the closure moves them, as the notebook does) and their labels
    data = [torch.rand(BS, NC, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1, torch.zeros(BS, dtype=torch.int64)]
    hip = make_path(dcgan.Generator, dcgan.Discriminator, dcgan.BCEWithLogitsLoss(), data)
    for _ in range(WARMUP):
        hip()
    torch.cuda.synchronize()
    if a.layer_times:
        return layer_times(hip)
    if a.profile_steps:
        for _ in range(a.profile_steps):
            hip()
        torch.cuda.synchronize()
        return
    stock = make_path(StockGenerator, StockDiscriminator, nn.BCEWithLogitsLoss(), data)
    for _ in range(WARMUP):
        stock()
    t = {"hip": [], "stock": []}
    for _ in range(a.blocks):
        t["hip"].append(timed(hip, a.reps))
        t["stock"].append(timed(stock, a.reps))
    out = dict(batch=BS, reps=a.reps, blocks=a.blocks, unit="us per dis_img + gen Euler step pair")
    for k, v in t.items():
        out[k] = dict(blocks=[round(u, 1) for u in v], median=round(statistics.median(v), 1),
                      range=[round(min(v), 1), round(max(v), 1)])
    out["hip_over_stock"] = round(out["hip"]["median"] / out["stock"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
