"""Times stage 2's MNIST GAN at the notebook's size (B = 100, 100-256-512-1024-784 / 784-1024-512-256-1): one Euler `dis_img`
step plus one `gen` step of GANODETrainer (reg = 0) with the closures of notebook cell 6, on the HIP modules
(gan_ode_amd.fcgan) and on the same two networks as stock torch modules with nn.BCELoss on the same GPU -- the reference's
own implementation, the yardstick.

  python scripts/bench_fcgan.py [--blocks 7] [--reps 50] [--profile-steps N]

Device events around `reps` step pairs, after a warm-up; blocks of the two paths alternate in one process.  Prints one JSON
line: the per-block times (microseconds per step pair), median and range of both paths, and their ratio.
--profile-steps N: runs N step pairs of the HIP path only after the warm-up and prints nothing else -- for
`rocprofv3 --kernel-trace --stats -- python scripts/bench_fcgan.py --profile-steps 20`.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_ode_amd as G  # noqa: E402
from gan_ode_amd import fcgan  # noqa: E402

BS, Z_DIM, MNIST_DIM = 100, 100, 784


class StockGenerator(nn.Module):
    def __init__(self, g_input_dim, g_output_dim):
        super().__init__()
        self.fc1 = nn.Linear(g_input_dim, 256)
        self.fc2 = nn.Linear(self.fc1.out_features, self.fc1.out_features * 2)
        self.fc3 = nn.Linear(self.fc2.out_features, self.fc2.out_features * 2)
        self.fc4 = nn.Linear(self.fc3.out_features, g_output_dim)

    def forward(self, x):
        x = F.leaky_relu(self.fc1(x), 0.2)
        x = F.leaky_relu(self.fc2(x), 0.2)
        x = F.leaky_relu(self.fc3(x), 0.2)
        return torch.tanh(self.fc4(x))


class StockDiscriminator(nn.Module):
    def __init__(self, d_input_dim):
        super().__init__()
        self.fc1 = nn.Linear(d_input_dim, 1024)
        self.fc2 = nn.Linear(self.fc1.out_features, self.fc1.out_features // 2)
        self.fc3 = nn.Linear(self.fc2.out_features, self.fc2.out_features // 2)
        self.fc4 = nn.Linear(self.fc3.out_features, 1)

    def forward(self, x):
        x = F.dropout(F.leaky_relu(self.fc1(x), 0.2), 0.3)
        x = F.dropout(F.leaky_relu(self.fc2(x), 0.2), 0.3)
        x = F.dropout(F.leaky_relu(self.fc3(x), 0.2), 0.3)
        return torch.sigmoid(self.fc4(x))


def make_path(gen_cls, dis_cls, criterion, x):
    torch.manual_seed(97382)
    gen, dis = gen_cls(Z_DIM, MNIST_DIM).cuda(), dis_cls(MNIST_DIM).cuda()
    device = "cuda"

    def d_loss(x):
        dis.zero_grad()
        x_real, y_real = x.view(-1, MNIST_DIM), torch.ones(BS, 1)
        x_real, y_real = x_real.to(device), y_real.to(device)
        real_loss = criterion(dis(x_real), y_real)
        z = torch.randn(BS, Z_DIM).to(device)
        x_fake, y_fake = gen(z), torch.zeros(BS, 1).to(device)
        return real_loss + criterion(dis(x_fake), y_fake)

    def g_loss():
        gen.zero_grad()
        z = torch.randn(BS, Z_DIM).to(device)
        y = torch.ones(BS, 1).to(device)
        return criterion(dis(gen(z)), y)

    tr = G.GANODETrainer(gen.parameters(), dis.parameters(), None, g_loss, d_loss, None, lr=0.02, reg=0.0, method="euler")

    def pair():
        tr.step(x, model="dis_img")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    G.limit_host_threads()
    x = torch.rand(BS, 1, 28, 28, generator=torch.Generator().manual_seed(0)) * 2 - 1
    hip = make_path(fcgan.Generator, fcgan.Discriminator, fcgan.BCELoss(), x)
    for _ in range(20):
        hip()
    torch.cuda.synchronize()
    if a.profile_steps:
        for _ in range(a.profile_steps):
            hip()
        torch.cuda.synchronize()
        return
    stock = make_path(StockGenerator, StockDiscriminator, nn.BCELoss(), x)
    for _ in range(20):
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
