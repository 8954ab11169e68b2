"""Times the drivers' genSamples on the GPU: gan_ode_amd.video_io.gen_samples against the reference's
route restated below.  Needs the MI355X.

  python scripts/bench_gen_samples.py [--out profiles/gen_samples_times.jsonl] [--blocks 7] [--configs mnist ucf] [--n 8]

Both routes run in one process on the same full-width generator, in alternating blocks after a warm-up of each, on a host clock
around work that ends on the host (the file is on disk, so every device copy has completed; a synchronise precedes the first
stamp).  Per config one JSON line: the median and range of the whole call of either route, and its stages timed in blocks of
their own:
  fast       sample (eval-mode sample_videos(n*n), synchronised) | grid (gode_video_grid, idx only, synchronised) | copy
             (T * nH * nW bytes to the host) | encode (write_gif: LZW and file)
  reference  sample | copy (.cpu().numpy() of the fp32 videos) | tile (the float64 grid, transpose, (x + 1) / 2 * 255) |
             vwrite (clip, truncate, gray test or palette index on the host, then the same write_gif) | encode (write_gif alone on
             the indices vwrite computed: the part both routes share)
and the bytes either route copies, counted from shapes.  The two files of a same-seed call are compared byte for byte first.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def reference_gen_samples(g, io, path, n=8, size=64):
    """mnist_moco_ode.py:31-48, with the path as an argument.  -> the stages' seconds"""
    import torch
    t = [time.perf_counter()]
    g.eval()
    with torch.no_grad():
        s = g.sample_videos(n ** 2)[0]
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        s = s.cpu().detach().numpy()
    g.train()
    t.append(time.perf_counter())
    out = np.zeros((3, 16, size * n, size * n))
    for j in range(n):
        for k in range(n):
            out[:, :, size * j:size * (j + 1), size * k:size * (k + 1)] = s[j * n + k, :, :, :, :]
    out = out.transpose((1, 2, 3, 0))
    out = (out + 1) / 2 * 255
    t.append(time.perf_counter())
    io.vwrite(path, out)
    t.append(time.perf_counter())
    return dict(zip(("sample", "copy", "tile", "vwrite"), np.diff(t)))


def fast_stages(g, V, path, n):
    import torch
    t = [time.perf_counter()]
    g.eval()
    with torch.no_grad():
        s = g.sample_videos(n * n)[0]
    g.train()
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    idx = V.video_grid(s, n=n, rgb=False, idx=True)
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    host = idx.cpu().numpy()
    t.append(time.perf_counter())
    V.write_gif(path, host, V.GRAY_PALETTE if s.shape[1] == 1 else V.RGB676_PALETTE)
    t.append(time.perf_counter())
    return dict(zip(("sample", "grid", "copy", "encode"), np.diff(t))), host


def _summary(v):
    ms = [x * 1e3 for x in v]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "blocks_ms": [round(x, 3) for x in ms]}


def bench(config, n, blocks, tmp):
    import torch
    import gan_ode_amd as G
    from gan_ode_amd import video_io as V
    torch.manual_seed(0)
    np.random.seed(0)
    gen = (G.build_mnist if config == "mnist" else G.build_ucf)()[0].cuda()
    size, C = (28, 1) if config == "mnist" else (64, 3)
    fast_path, ref_path = os.path.join(tmp, f"gensamples_id{config}.gif"), os.path.join(tmp, f"ref_{config}.gif")

    def fast():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        V.gen_samples(gen, n=n, e=config, size=size, video_sample_path=tmp)
        return time.perf_counter() - t0

    def ref():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_gen_samples(gen, V, ref_path, n=n, size=size)
        return time.perf_counter() - t0

    # the values timed are the values tested: the same seeds give the same file on either route
    for fn in (fast, ref):
        torch.manual_seed(1)
        np.random.seed(1)
        fn()
    same = open(fast_path, "rb").read() == open(ref_path, "rb").read()
    fast(), ref()                                                  # warm-up of every shape is behind us now
    whole = {"fast": [], "reference": []}
    stages = {"fast": [], "reference": []}
    encode = []
    for _ in range(blocks):
        whole["fast"].append(fast())
        whole["reference"].append(ref())
        torch.cuda.synchronize()
        st, host = fast_stages(gen, V, fast_path, n)
        stages["fast"].append(st)
        torch.cuda.synchronize()
        stages["reference"].append(reference_gen_samples(gen, V, ref_path, n=n, size=size))
        t0 = time.perf_counter()
        V.write_gif(ref_path, host, V.GRAY_PALETTE if C == 1 else V.RGB676_PALETTE)
        encode.append(time.perf_counter() - t0)
    T = 16
    res = {"config": config, "n": n, "frame": size, "channels": C, "blocks": blocks, "files_identical": same,
           "file_bytes": os.path.getsize(fast_path),
           "copy_bytes": {"fast": T * n * size * n * size, "reference": n * n * C * T * size * size * 4},
           "host_float64_bytes": 3 * T * n * size * n * size * 8,
           "whole": {k: _summary(v) for k, v in whole.items()},
           "stages": {k: {name: _summary([b[name] for b in v]) for name in v[0]} for k, v in stages.items()},
           "encode_alone": _summary(encode)}
    res["reference_over_fast"] = round(res["whole"]["reference"]["median_ms"] / res["whole"]["fast"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gen_samples_times.jsonl"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--configs", nargs="+", default=["mnist", "ucf"], choices=["mnist", "ucf"])
    args = ap.parse_args()
    import torch
    import gan_ode_amd as G
    assert torch.cuda.is_available(), "bench_gen_samples.py needs the MI355X"
    G.limit_host_threads()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp, open(args.out, "w") as f:
        for config in args.configs:
            res = bench(config, args.n, args.blocks, tmp)
            f.write(json.dumps(res) + "\n")
            f.flush()
            print(json.dumps({k: res[k] for k in ("config", "files_identical", "copy_bytes", "reference_over_fast")}
                             | {"fast_ms": res["whole"]["fast"]["median_ms"], "reference_ms": res["whole"]["reference"]["median_ms"],
                                "encode_ms": res["encode_alone"]["median_ms"]}), flush=True)


if __name__ == "__main__":
    main()
