"""Bit-identity of the weight gradients (GPU box): runs gode_wgrad on the cells of tests/test_gpu_wgrad_paths.py and on the
convolution layers of the MNIST (generator rows 512, discriminators batch 32) and UCF (rows 256, batch 16) configs, each
plain and with BN+ReLU fused into x, from fixed seeds, and prints one sha256 of dw per case.  Two libraries that launch the
same kernels with the same arguments print the same lines (the slab reduce sums in a fixed order).
    python scripts/wgrad_hashes.py > hashes.txt"""
import ctypes as C
import hashlib
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

import gan_ode_amd._lib as L
from gan_ode_amd.engine import conv_out, make_geom, stream_ptr
from test_gpu_wgrad_paths import CELLS, SHAPES


def layers():
    """(name, (N, Ci, Co, xi, k, s, p)) of the config layers, as tests/hostcheck/corpus.h builds them."""
    out = []

    def generator(cfg, rows, mnist):
        out.append((f"{cfg}.G{rows}.L0", (rows, 512, 96, (1, 4, 4), (1, 4, 4), (1, 1, 1), (0, 0, 0))))
        for l, ci in enumerate((256, 128, 64)):
            out.append((f"{cfg}.G{rows}.L{l + 1}", (rows, ci, 2 * ci, (1, 8 << l, 8 << l), (1, 4, 4), (1, 2, 2), (0, 1, 1))))
        out.append((f"{cfg}.G{rows}.L4", (rows, 1, 64, (1, 28, 28), (1, 1, 1), (1, 1, 1), (0, 2, 2)) if mnist else
                    (rows, 3, 64, (1, 64, 64), (1, 4, 4), (1, 2, 2), (0, 1, 1))))

    def video_d(cfg, B, Cin, D, H, k):
        ch = (Cin, 64, 128, 256, 512)
        for l in range(4):
            out.append((f"{cfg}.V{B}.L{l}", (B, ch[l], ch[l + 1], (D, H, H), (k, k, k), (1, 2, 2), (0, 1, 1))))
            D, H = conv_out(D, k, 1, 0), conv_out(H, k, 2, 1)
        out.append((f"{cfg}.V{B}.L4", (B, 512, 1, (D, H, H), (k, k, k), (1, 1, 1), (0, 0, 0))))

    def image_d(cfg, B, Cin, H):
        ch = (Cin, 64, 128, 256, 1)
        for l in range(4):
            out.append((f"{cfg}.I{B}.L{l}", (B, ch[l], ch[l + 1], (1, H, H), (1, 4, 4), (1, 2, 2), (0, 1, 1))))
            H = conv_out(H, 4, 2, 1)

    generator("mnist", 512, True); video_d("mnist", 32, 1, 16, 28, 2); image_d("mnist", 32, 1, 28)
    generator("ucf", 256, False); video_d("ucf", 16, 3, 16, 64, 4); image_d("ucf", 16, 3, 64)
    return out


def run(name, spec, seed, xo=0, yo=0, wo=0, xform=None):
    N, Ci, Co, xi, k, s, p = spec
    yd = tuple(conv_out(xi[a], k[a], s[a], p[a]) for a in range(3))
    g = make_geom(N, Ci, Co, xi, yd, k, s, p)
    torch.manual_seed(seed)

    def placed(shape, off):
        buf = torch.empty(math.prod(shape) + 4, device="cuda")
        v = buf[off:buf.numel() - 4 + off].view(shape)
        v.normal_()
        return v

    x, y = placed((N, *xi, Ci), xo), placed((N, *yd, Co), yo)
    Cx = Co if xform == "y" else Ci
    sc, sh = torch.rand(Cx, device="cuda") + 0.5, torch.randn(Cx, device="cuda")
    dw = torch.full((Co, Ci, *k), float("nan"), device="cuda")
    op = L.WgradOp(g=g, act=L.ACT_NONE if xform is None else L.ACT_RELU, xform_on_y=int(xform == "y"), splits=0, accumulate=0,
                   x=x.data_ptr(), y=y.data_ptr(), scale=None if xform is None else sc.data_ptr(),
                   shift=None if xform is None else sh.data_ptr(), dw=dw.data_ptr())
    work = torch.empty(L.lib().gode_wgrad_work_size(C.byref(op)) + 4, device="cuda")[wo:]
    op.work = work.data_ptr()
    L.run_one(op, stream_ptr())
    torch.cuda.synchronize()
    print(f"{name} x{xo} y{yo} w{wo} {xform or '-'} {hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest()}", flush=True)


if __name__ == "__main__":
    for i, (shape, xo, yo, wo, xform) in enumerate(CELLS):
        run("paths." + shape, SHAPES[shape][0], 1000 + i, xo, yo, wo, xform)
    for i, (name, spec) in enumerate(layers()):
        run(name, spec, 2000 + i)
        run(name, spec, 3000 + i, xform="x")
