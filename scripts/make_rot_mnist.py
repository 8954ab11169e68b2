"""Builds rot-mnist_rand.mat from MNIST IDX files already on disk: the reference's prepare_MNIST_data (utils/images.py:178-220)
with the rotation on the GPU (gode_rot_clips).  Needs the MI355X; fetches nothing.

  python scripts/make_rot_mnist.py --images train-images-idx3-ubyte.gz --labels train-labels-idx1-ubyte.gz \
      --count 11000 --mode rsre --out rot-mnist_rand.mat [--seed 0] [--valid 1000] [--frames 16]

As the reference: the first `count` digits are read, the leading `valid` of them (default count // 11: its valid_size =
tr_size / 10) are held out, the rest are rotated through `frames` angles of `mode` and every frame is normalised to [0, 1].
The file holds X float64 [n, frames, 784] and Y float64 [n, 1]; dataset.MNISTRotationVideo and the reference drivers load it.
--seed seeds NumPy's global stream, which the "rand-end" / "rsre" angles are drawn from (the reference's np.random.uniform
calls in its order).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gan_ode_amd import data as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", required=True)
    ap.add_argument("--labels", required=True)
    ap.add_argument("--count", type=int, default=11000)
    ap.add_argument("--valid", type=int, default=None)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--mode", default="normal", choices=D.ROT_MODES)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    valid = args.count // 11 if args.valid is None else args.valid
    if not 0 <= valid < args.count:
        ap.error(f"--valid {valid} leaves nothing of --count {args.count}")
    digits = D.read_idx_images(args.images, args.count)[valid:]
    labels = D.read_idx_labels(args.labels, args.count)[valid:]
    if args.seed is not None:
        np.random.seed(args.seed)
    ds = D.RotMnistOnDevice.from_digits(digits, labels, K=args.frames, mode=args.mode)
    ds.save_mat(args.out)
    print(f"wrote {args.out}: X {tuple(ds.X.reshape(ds.N, ds.T, -1).shape)}, Y ({ds.N}, 1), mode {args.mode}")


if __name__ == "__main__":
    main()
