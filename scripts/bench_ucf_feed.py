"""Measures the device-resident UCF-101 feed on the GPU; needs the MI355X, there is no CPU path.

  python scripts/bench_ucf_feed.py [--out profiles/ucf_feed.json] [--blocks 7]

Protocol: device events around windows of back-to-back calls, every shape warmed up first, the sides of a comparison
alternated block by block in ONE process, and the spread of the baseline's own blocks ((max - min) / median) reported next to
every ratio.  Bytes are counted from shapes.  Three measurements:
  ingest  gode_resize_u8 at 240x320x3 -> 64x85 -> columns 10..73, both modes: frames/s, achieved bytes/s, the HBM bound
          (input + output bytes over 6.29 TB/s), and the same arithmetic as torch ops on the device (F.interpolate + clamp +
          round + slice + cast);
  gather  one gode_clip_gather launch for 16 clips of 16 frames against the torch ops it replaces (index, float, sub, div);
  feed    a UCF iteration (batch 16, ngf = ndf = 64) fed from Ucf101OnDevice against the same iteration on fixed
          device-resident batches in the same channels-last layout, and in bench.py's contiguous [B, T, C, H, W] layout.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import gan_ode_amd as G  # noqa: E402
from gan_ode_amd import data as D  # noqa: E402

HBM_BYTES_PER_S = 6.29e12


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(sides, iters, blocks, warmup=3):
    """sides: name -> callable.  -> name -> {ms (median of the blocks), blocks, spread}."""
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(blocks):
        for k, fn in sides.items():
            ms[k].append(window_ms(fn, iters))
    return {k: {"ms": statistics.median(v), "blocks_ms": [round(x, 5) for x in v],
                "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in ms.items()}


def torch_resize(x, antialias):
    y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=(64, 85), mode="bicubic", align_corners=False, antialias=antialias)
    return y.clamp_(0.0, 255.0).round_()[:, :, :, 10:74].to(torch.uint8)


def bench_ingest(blocks, frames=256):
    x = torch.randint(0, 256, (frames, 240, 320, 3), dtype=torch.uint8, device="cuda")
    n_bytes = x.numel() + frames * 64 * 64 * 3
    out = {"frames": frames, "bytes_per_call": n_bytes, "hbm_bound_ms": n_bytes / HBM_BYTES_PER_S * 1e3}
    for aa in (False, True):
        tables = D.ResizeTables(240, 320, 64, 85, 10, 64, aa, "cuda")
        dst = torch.empty(frames, 64, 64, 3, dtype=torch.uint8, device="cuda")
        r = alternate({"gode_resize_u8": lambda: D.resize_u8(x, tables, dst=dst), "torch_ops": lambda: torch_resize(x, aa)},
                      iters=100, blocks=blocks)
        k = r["gode_resize_u8"]
        k["frames_per_s"] = frames / (k["ms"] * 1e-3)
        k["bytes_per_s"] = n_bytes / (k["ms"] * 1e-3)
        k["share_of_hbm_bound"] = out["hbm_bound_ms"] / k["ms"]
        r["torch_over_gode"] = r["torch_ops"]["ms"] / k["ms"]
        got, ref = dst.permute(0, 3, 1, 2), torch_resize(x, aa)
        r["bytes_differing_from_torch_fp32"] = int((got != ref).sum())
        r["ky_kx"] = [tables.ky, tables.kx]
        out["antialias" if aa else "plain"] = r
    return out


def bench_gather(blocks, n_frames=8192, B=16, T=16):
    store = torch.randint(0, 256, (n_frames, 64, 64, 3), dtype=torch.uint8, device="cuda")
    first = torch.randint(0, n_frames - T, (B,), generator=torch.Generator().manual_seed(0)).cuda()
    steps = torch.arange(T, device="cuda")

    def torch_ops():
        return (store[first[:, None] + steps[None, :]].float() - 128.0) / 128.0

    r = alternate({"gode_clip_gather": lambda: D.clip_gather(store, first, T), "torch_ops": torch_ops}, iters=2000, blocks=blocks)
    assert torch.equal(D.clip_gather(store, first, T), torch_ops())
    n_bytes = B * T * 12288 * 5
    r["bytes_per_call"] = n_bytes
    r["gode_clip_gather"]["bytes_per_s"] = n_bytes / (r["gode_clip_gather"]["ms"] * 1e-3)
    r["torch_over_gode"] = r["torch_ops"]["ms"] / r["gode_clip_gather"]["ms"]
    r["accepted"] = r["gode_clip_gather"]["ms"] <= r["torch_ops"]["ms"]
    return r


def bench_feed(blocks, B=16, videos=64, length=48):
    torch.manual_seed(1234)
    np.random.seed(1234)
    nets = [m.cuda() for m in G.build_ucf()]
    tr = G.GanTrainer(*nets)
    ds = D.Ucf101OnDevice(seed=0)
    for k in range(videos):
        ds.add_video(torch.randint(0, 256, (length, 240, 320, 3), dtype=torch.uint8, device="cuda"), k % 101)
    sv, si = ds.videos(B), ds.images(B)
    fixed_i, fixed_v = [next(si).clone() for _ in range(2)], [next(sv).clone() for _ in range(2)]      # strides kept
    plain_i, plain_v = [t.contiguous() for t in fixed_i], [t.contiguous() for t in fixed_v]          # bench.py's layout
    sides = {"fixed_channels_last": lambda: tr.step(fixed_i, fixed_v),
             "fed": lambda: tr.step([next(si), next(si)], [next(sv), next(sv)]),
             "fixed_contiguous": lambda: tr.step(plain_i, plain_v)}
    r = alternate(sides, iters=20, blocks=blocks)
    base = r["fixed_channels_last"]
    r["feed_ms"] = r["fed"]["ms"] - base["ms"]
    r["fed_over_fixed"] = r["fed"]["ms"] / base["ms"]
    r["baseline_spread"] = base["spread"]
    r["store"] = {"videos": len(ds), "frames": ds.n_frames, "bytes": ds.n_frames * 12288}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ucf_feed.json"))
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ucf_feed.py measures on the GPU; there is none here")
    G.limit_host_threads()
    res = {"device": torch.cuda.get_device_name(0), "ingest": bench_ingest(a.blocks), "gather": bench_gather(a.blocks),
           "feed": bench_feed(a.blocks)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"ingest_plain_ms": res["ingest"]["plain"]["gode_resize_u8"]["ms"],
                      "ingest_antialias_ms": res["ingest"]["antialias"]["gode_resize_u8"]["ms"],
                      "gather_ms": res["gather"]["gode_clip_gather"]["ms"], "gather_torch_ms": res["gather"]["torch_ops"]["ms"],
                      "gather_accepted": res["gather"]["accepted"], "iteration_fed_ms": res["feed"]["fed"]["ms"],
                      "iteration_fixed_ms": res["feed"]["fixed_channels_last"]["ms"],
                      "baseline_spread": res["feed"]["baseline_spread"]}))


if __name__ == "__main__":
    main()
