"""Writes tests/golden/gen_gru_tiny*.npz: the reference's own MoCoGAN VideoGenerator (models/mocogan.py:185-301, the GRU
motion latent) run on the CPU under fixed seeds, by the recipe of oracle/make_goldens.py's golden_generator(): seeded
VideoGenerator(3, 50, 0, 16, 16, ngf=8) weights; sample_videos(1) and sample_images(3) under seeds s+1 and s+2;
fp16-rounded cotangents; every parameter gradient (recurrent.* included); the BatchNorm buffers after the two calls; and
eval-mode videos.  Data only: no reference source enters the repository.  The arrays are split over four files
(PARTS) so that each stays below 1 MiB; tests/test_gpu_gru.py merges them.

  python scripts/make_gru_golden.py /path/to/reference

models/mocogan.py imports only torch and numpy; it is loaded by path (this repository's drop-in `models` package would
otherwise shadow it).  On a machine without a GPU the reference draws h_0 and e_t with torch.FloatTensor(...).normal_(),
the global CPU generator -- the order libgode's VideoGeneratorGRU reproduces.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SEED, NGF, N_VID, N_IMG = 41, 8, 1, 3
# file -> which arrays it holds (by key prefix or name); the first file takes everything not claimed by another
PARTS = {"gen_gru_tiny.npz": None, "gen_gru_tiny_grads.npz": ("g/", "wv"), "gen_gru_tiny_videos.npz": ("videos",),
         "gen_gru_tiny_eval.npz": ("videos_eval",)}


def _part_of(key):
    for name, sel in PARTS.items():
        if sel and any(key == s or (s.endswith("/") and key.startswith(s)) for s in sel):
            return name
    return "gen_gru_tiny.npz"


def seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def h16(x):
    return x.half().float()


def main(ref):
    assert not torch.cuda.is_available(), "run on a CPU-only machine: the reference would draw its noise on the device"
    spec = importlib.util.spec_from_file_location("ref_mocogan", os.path.join(ref, "models", "mocogan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seed(SEED)
    gen = mod.VideoGenerator(3, 50, 0, 16, 16, ngf=NGF)
    arrays = {f"w/{k}": v.detach().cpu().numpy().copy() for k, v in gen.state_dict().items()}
    seed(SEED + 1)
    vid, labels = gen.sample_videos(N_VID)
    seed(SEED + 2)
    img, _ = gen.sample_images(N_IMG)
    seed(SEED + 3)
    wv, wi = h16(torch.randn_like(vid)), h16(torch.randn_like(img))
    ((vid * wv).sum() + (img * wi).sum()).backward()
    for k, p in gen.named_parameters():
        arrays[f"g/{k}"] = p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(0, np.float32)
    for k, v in gen.state_dict().items():
        if "running_" in k or "num_batches" in k:
            arrays[f"w_after/{k}"] = v.detach().cpu().numpy().copy()
    arrays.update(videos=vid.detach().numpy(), labels=labels.numpy(), images=img.detach().numpy(),
                  wv=wv.numpy().astype(np.float16), wi=wi.numpy().astype(np.float16), seed=np.int64(SEED),
                  ngf=np.int64(NGF))
    gen.eval()
    seed(SEED + 4)
    with torch.no_grad():
        ev, _ = gen.sample_videos(N_VID)
    arrays["videos_eval"] = ev.numpy()
    for name in PARTS:
        part = {k: v for k, v in arrays.items() if _part_of(k) == name}
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **part)
        print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(part)} arrays")
        assert os.path.getsize(path) < 1 << 20, path


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(REPO), "reference"))
