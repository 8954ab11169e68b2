"""Writes tests/golden/rotmnist_ref.npz: what the reference's own rotate_data (utils/images.py:101-173) returns for three small
images in each of its three angle modes, as recorded data for tests/test_host_rotmnist.py and tests/test_gpu_rotmnist.py.

  python scripts/make_rotmnist_golden.py --reference /path/to/reference/checkout

Generation time only (needs scipy; the tests read the .npz alone).  The reference module cannot be imported -- its last lines
download MNIST -- so the `rotate_data` function definition alone is taken out of the parsed file with `ast` and compiled with
`np`, `ndimage`, `os` and a stand-in for PIL's `Image` as its globals (the JPEG previews it saves for the first ten digits are a
side effect, not data).  It runs in a temporary working directory that has the `data/` folder it writes those previews under.

Per mode: np.random.seed(SEED), then rotate_data(images, one-hot labels, K=16, mode).  Stored: the inputs, the seed, and per
mode the returned X (squeezed: float64 [3, 16, 784]) and Y.  Nothing of the reference's text goes into this script or the file.
"""
import argparse
import ast
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "rotmnist_ref.npz")
SEED, K, MODES = 0, 16, ("normal", "rand-end", "rsre")


class _NoImage:
    """Image.fromarray(a).convert('RGB').save(name) without PIL and without a file."""

    @staticmethod
    def fromarray(_):
        return _NoImage()

    def convert(self, _):
        return self

    def save(self, _):
        pass


def load_rotate_data(reference):
    from scipy import ndimage
    path = os.path.join(reference, "utils", "images.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "rotate_data"]
    assert len(fn) == 1, f"{path}: {len(fn)} definitions of rotate_data"
    ns = {"np": np, "ndimage": ndimage, "os": os, "Image": _NoImage, "DATA_DIRECTORY": "data", "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["rotate_data"]


def inputs():
    """Three 28 x 28 fp32 images in [-0.5, 0.5] as rows of 784: two of uniform noise, one blob on the -0.5 background."""
    rs = np.random.RandomState(20251)
    noise = rs.uniform(-0.5, 0.5, (2, 28, 28))
    y, x = np.mgrid[0:28, 0:28]
    blob = -0.5 + np.exp(-((y - 12.0) ** 2 / 30.0 + (x - 15.5) ** 2 / 12.0))
    images = np.concatenate([noise, blob[None]]).reshape(3, 784).astype(np.float32)
    labels = np.zeros((3, 10))
    labels[np.arange(3), [7, 0, 3]] = 1
    return images, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds utils/images.py)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    rotate_data = load_rotate_data(os.path.abspath(args.reference))
    images, labels = inputs()
    store = {"images": images, "labels": labels, "seed": np.int64(SEED), "K": np.int64(K)}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.mkdir(os.path.join(tmp, "data"))
        os.chdir(tmp)
        try:
            for mode in MODES:
                np.random.seed(SEED)
                X, Y = rotate_data(images, labels, K=K, mode=mode)
                X, Y = np.asarray(X, dtype=np.float64).squeeze(), np.asarray(Y, dtype=np.float64).squeeze()
                assert X.shape == (3, K, 784) and Y.shape == (3,), (X.shape, Y.shape)
                store[f"X_{mode}"], store[f"Y_{mode}"] = X, Y
        finally:
            os.chdir(cwd)
    np.savez(args.out, **store)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    sys.exit(main())
