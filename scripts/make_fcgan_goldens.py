"""Writes tests/golden/fcgan_own.npz: for every problem of tests/fc_ref.py (modules at four batch sizes, one dis_img and one gen
step per method, the penalty, the notebook's Adam iteration) the error of the fp32 CPU restatement against the fp64 one, per
tensor -- the figures the 8x allowances of tests/test_gpu_fcgan.py are taken from.  Stock torch on the CPU
with one thread; data only, nothing of the reference is read.

  python scripts/make_fcgan_goldens.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import fc_ref as R  # noqa: E402
from gan_ode_amd.ode_training import FD_H  # noqa: E402


def main():
    torch.set_num_threads(1)
    out = R.measure_own(FD_H)
    np.savez_compressed(R.OWN_FILE, **{k: np.float64(v) for k, v in out.items()})
    print(f"{R.OWN_FILE}: {len(out)} figures, {os.path.getsize(R.OWN_FILE)} bytes")
    for k in sorted(out):
        print(f"  {k}: {out[k]:.3e}")


if __name__ == "__main__":
    main()
