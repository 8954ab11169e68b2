"""Measures the Rotated-MNIST clip builder on the GPU; needs the MI355X, there is no CPU path for the op.

  python scripts/bench_rot_mnist.py [--out profiles/rot_mnist.json] [--digits 10000] [--blocks 7] [--workers 16]

The reference's tr_size: 10,000 digits x 16 frames of 28 x 28, mode "rsre".  Three numbers:
  launch   gode_rot_clips as ONE launch (table already on the device), device events around windows of back-to-back launches,
           warmed up first, median of the blocks with their spread ((max - min) / median); and the whole rotate_clips call (table
           built on the host, uploaded, launched) on a host clock that ends in a synchronise;
  hbm      the bytes the launch has to move, counted from shapes (digits + table in, the normalised frames out: 0.5 GB), over the
           launch time, as a share of the HBM peak of 6.29 TB/s;
  scipy    the same work through scipy.ndimage.rotate + the min-max normalisation on the host, over `workers` processes (the
           host's CPU quota), run before the GPU is opened; plus one process alone on a sixteenth of the digits.
"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BYTES_PER_S = 6.29e12
K = 16


def _scipy_chunk(args):
    from scipy import ndimage
    digits, angles = args
    x = (digits.astype(np.float32) - (255 / 2.0)) / 255
    X = np.zeros((len(x), K, 784))
    for d in range(len(x)):
        for k in range(K):
            X[d, k] = ndimage.rotate(x[d], angles[d, k], reshape=False, cval=-0.5).reshape(784)
    X = X / (np.max(X, 2, keepdims=True) - np.min(X, 2, keepdims=True))
    return X - np.min(X, 2, keepdims=True)


def bench_scipy(digits, angles, workers):
    chunks = [(digits[i::workers], angles[i::workers]) for i in range(workers)]
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_scipy_chunk, [(digits[:2], angles[:2])] * workers)          # workers started, scipy imported
        t0 = time.perf_counter()
        pool.map(_scipy_chunk, chunks)
        pooled = time.perf_counter() - t0
    t0 = time.perf_counter()
    _scipy_chunk(chunks[0])
    return {"workers": workers, "seconds": pooled, "one_process_seconds_for_a_share": time.perf_counter() - t0,
            "share_digits": len(chunks[0][0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rot_mnist.json"))
    ap.add_argument("--digits", type=int, default=10000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--workers", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    n = args.digits
    rs = np.random.RandomState(0)
    digits = rs.randint(0, 256, (n, 28, 28)).astype(np.uint8)
    digits[:, :4] = 0                                                        # a black margin, as MNIST has
    from gan_ode_amd import data as D
    angles = D.rot_angles(n, K, "rsre", np.random.RandomState(1))
    res = {"digits": n, "frames": K, "mode": "rsre", "scipy": bench_scipy(digits, angles, args.workers)}

    import torch
    import gan_ode_amd as G
    from gan_ode_amd import _lib as L
    assert torch.cuda.is_available(), "bench_rot_mnist.py needs the MI355X"
    x = torch.from_numpy(digits).cuda()
    cs = D.rot_table(angles).cuda()
    out = torch.empty((n, K, 28, 28), dtype=torch.float32, device="cuda")
    op = L.RotClipsOp(images=x.data_ptr(), cs=cs.data_ptr(), out=out.data_ptr(), raw=None, n=n, K=K, H=28, W=28, in_u8=1,
                      in_scale=1.0, in_shift=0.0, cval=-0.5)
    st = G.engine.stream_ptr()
    for _ in range(3):
        L.run_one(op, st)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            L.run_one(op, st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / args.iters)
    launch_ms = statistics.median(ms)
    n_bytes = x.numel() + cs.numel() * 4 + out.numel() * 4
    res["launch"] = {"ms": launch_ms, "blocks_ms": [round(v, 5) for v in ms], "spread": (max(ms) - min(ms)) / launch_ms,
                     "frames_per_s": n * K / (launch_ms * 1e-3)}
    res["hbm"] = {"bytes": n_bytes, "output_bytes": out.numel() * 4, "bytes_per_s": n_bytes / (launch_ms * 1e-3),
                  "bound_ms": n_bytes / HBM_BYTES_PER_S * 1e3, "share_of_peak": n_bytes / HBM_BYTES_PER_S * 1e3 / launch_ms}
    whole = []
    for _ in range(args.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        D.rotate_clips(x, angles, out=out)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    res["call"] = {"ms": statistics.median(whole), "blocks_ms": [round(v, 3) for v in whole]}
    # the values timed are the values tested: a slice against the host result of the same digits
    want = _scipy_chunk((digits[:32], angles[:32])).reshape(32, K, 28, 28)
    res["max_abs_diff_vs_scipy_first_32"] = float((out[:32].cpu().double() - torch.from_numpy(want)).abs().max())
    res["scipy_over_launch"] = res["scipy"]["seconds"] * 1e3 / launch_ms
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"launch_ms": launch_ms, "spread": res["launch"]["spread"], "hbm_share": res["hbm"]["share_of_peak"],
                      "call_ms": res["call"]["ms"], "scipy_s": res["scipy"]["seconds"], "workers": args.workers,
                      "max_abs_diff_vs_scipy": res["max_abs_diff_vs_scipy_first_32"]}))


if __name__ == "__main__":
    main()
