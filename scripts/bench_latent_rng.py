"""Latents drawn on the host (latent_rng = "host", the default) next to latents drawn on the device ("device"), same
process, alternating blocks: (a) sample_videos(32) / sample_images(32) in a loop -- MNIST ODE generator and the GRU
generator at the 64x64 config; (b) a GanTrainer iteration, eager, MNIST batch 32, queued back to back and with a
synchronise after every iteration (a loop that reads its losses); (c) the same with graph=True.
Wall time per call on a host clock around work that ends in a device synchronise; one JSON line per block, then a
summary (median and range over the blocks).  `--out FILE` appends the raw lines there; arguments `sample`, `eager`, `graph`
select parts, `diag` adds the eager iteration without the prefetch / without the image discriminator's side stream and the
draw op alone."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import gan_ode_amd as G
from gan_ode_amd.modules import VideoGeneratorGRU
G.limit_host_threads()
only = [a for a in sys.argv[1:] if not a.startswith("--")]
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out:
    only.remove(out)
B, BLOCKS = 32, 6
MODES = ("host", "device")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed(fn, reps, sync_each=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        if sync_each:                      # a loop that reads its losses every iteration
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def blocks(what, fns, reps, warm, sync_each=False):
    """fns: mode -> callable.  Warm both, then BLOCKS blocks per mode, the order alternating."""
    for m in MODES:
        for _ in range(warm):
            fns[m]()
    torch.cuda.synchronize()
    for rep in range(BLOCKS):
        for m in (MODES if rep % 2 == 0 else MODES[::-1]):
            emit(what=what, latent_rng=m, block=rep, reps=reps, ms_per_call=round(timed(fns[m], reps, sync_each), 4))


def sampler(make):
    gens = {}
    for m in MODES:
        torch.manual_seed(0); np.random.seed(0)
        g = make().cuda()
        g.latent_rng = m
        gens[m] = g
    return gens


def videos(g):
    with torch.no_grad():
        g.sample_videos(B)


def images(g):
    with torch.no_grad():
        g.sample_images(B)


def trainer(mode, graph, **kw):
    torch.manual_seed(0); np.random.seed(0)
    nets = G.build_mnist()
    for n in nets:
        n.cuda()
    nets[0].latent_rng = mode
    tr = G.GanTrainer(*nets, graph=graph, **kw)
    imgs = [torch.rand(B, 1, 28, 28).cuda() for _ in range(2)]
    vids = [torch.rand(B, 16, 1, 28, 28).cuda() for _ in range(2)]
    return lambda: tr.step(imgs, vids)


if not only or "sample" in only:
    for name, make in (("mnist_ode", lambda: G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, dim_hidden=16)),
                       ("gru_64", lambda: VideoGeneratorGRU(3, 50, 0, 16, 16))):
        gens = sampler(make)
        blocks(f"{name} sample_videos({B})", {m: (lambda g=gens[m]: videos(g)) for m in MODES}, 200, 30)
        blocks(f"{name} sample_images({B})", {m: (lambda g=gens[m]: images(g)) for m in MODES}, 200, 30)
        del gens
if not only or "eager" in only:
    fns = {m: trainer(m, False) for m in MODES}
    blocks(f"mnist iteration eager B={B}", fns, 40, 12)
    blocks(f"mnist iteration eager B={B}, sync each", fns, 40, 2, sync_each=True)
    del fns
if not only or "graph" in only:
    blocks(f"mnist iteration graph B={B}", {m: trainer(m, True) for m in MODES}, 40, 12)

if "diag" in only:
    # what the back-to-back eager figure depends on: the trainer's side stream and the prefetch; and the draw op alone
    import ctypes as C
    import gan_ode_amd._lib as L
    for label, kw in (("prefetch off", dict(prefetch_latents=False)), ("overlap_image_d off", dict(overlap_image_d=False))):
        blocks(f"mnist iteration eager B={B}, {label}", {m: trainer(m, False, **kw) for m in MODES}, 40, 12)
    for n, outer, inner, T, n_all in ((32, 1, 16, 16, 1024), (512, 1, 16, 16, 0), (32, 17, 16, 16, 1024), (32, 17, 16, 16, 0)):
        buf = torch.zeros(n * (outer * inner + 52), device="cuda")
        nx = outer * n * inner
        op = L.LatentDrawOp(x=buf.data_ptr(), content=buf.data_ptr() + 4 * nx, sel_t=buf.data_ptr() + 4 * (nx + 50 * n),
                            cls=None, call_dev=None, seed=1, traj0=0, n=n, outer=outer, inner=inner, T=T, n_all=n_all, C=0,
                            stream=0, call=0)
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(20):
            L.check(L.lib().gode_latent_draw(C.byref(op), st))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(1000):
            L.lib().gode_latent_draw(C.byref(op), st)
        e1.record(); torch.cuda.synchronize()
        emit(what="gode_latent_draw alone, 1000 launches back to back (device events)", n=n, outer=outer, inner=inner, T=T,
             n_all=n_all, us_per_launch=round(e0.elapsed_time(e1), 3))

print()
for what in dict.fromkeys(l["what"] for l in lines if "ms_per_call" in l):
    for m in MODES:
        v = [l["ms_per_call"] for l in lines if l["what"] == what and l["latent_rng"] == m]
        print(f"{what:42s} {m:6s} median {np.median(v):8.4f} ms  range {min(v):8.4f} .. {max(v):8.4f}")
if out:
    with open(out, "a") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")
