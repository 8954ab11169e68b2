"""MNIST batch-32 iteration: categorical (C = 10) next to unconditional (C == 0), same process, alternating blocks."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gan_ode_amd as G
G.limit_host_threads()
mode = sys.argv[1] if len(sys.argv) > 1 else "time"
B = 32
def make(C):
    torch.manual_seed(0); np.random.seed(0)
    if C:
        nets = (G.VideoGeneratorMNISTODE(1, 50, C, 16, 16), G.CategoricalVideoDiscriminator(1, C, ksize=2), G.PatchImageDiscriminator(1))
    else:
        nets = G.build_mnist()
    for m in nets: m.cuda()
    tr = G.GanTrainer(*nets)
    imgs = [torch.rand(B, 1, 28, 28).cuda() for _ in range(2)]
    vids = [torch.rand(B, 16, 1, 28, 28).cuda() for _ in range(2)]
    labs = [torch.randint(0, C, (B,)).cuda() for _ in range(2)] if C else None
    return lambda: tr.step(imgs, vids, labs)
if mode == "profile":
    step = make(10)
    for _ in range(12): step()
    torch.cuda.synchronize()
    sys.exit(0)
steps = {0: make(0), 10: make(10)}
for s in steps.values():
    for _ in range(10): s()
torch.cuda.synchronize()
res = {0: [], 10: []}
for rep in range(6):
    for C in ((0, 10) if rep % 2 == 0 else (10, 0)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(30): steps[C]()
        e1.record(); torch.cuda.synchronize()
        res[C].append(e0.elapsed_time(e1) / 30)
for C in (0, 10):
    print(f"C={C}: ms/iteration per block {['%.3f' % v for v in res[C]]} median {np.median(res[C]):.3f}")
