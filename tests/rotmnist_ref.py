"""Shared by tests/test_host_rotmnist.py and tests/test_gpu_rotmnist.py (not collected): the rotation cells of gode_rot_clips,
their seeded inputs and float64 oracle results (computed once per cell, never modified by a test), the tolerances of DESIGN
section 25 and the rule for pixels whose source point lies on the input's edge."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN

from gan_ode_amd import data as D

CVAL = 0.25                 # not a value the noise images favour: a wrong inside / outside decision shows up
RAW_TOL = 1e-4              # |raw - float64 oracle|: ~3e-5 from the fp32 coordinates (1e-5 px, slope of a few units per pixel),
                            # ~1e-6 from the fp32 prefilter and the 16-tap sum
OUT_TOL = 4.0 * RAW_TOL     # |out - oracle| <= OUT_TOL / r per frame, r the frame's oracle range (asserted >= MIN_RANGE)
MIN_RANGE = 0.5
EDGE = 3e-5                 # a source coordinate this close to 0, H - 1 or W - 1 may fall on either side in fp32
MAX_EDGE_SHARE = 0.005
FIXTURE = os.path.join(GOLDEN, "rotmnist_ref.npz")
MODES = ("normal", "rand-end", "rsre")


def _f_many_angles():
    return np.linspace(-350.0, 350.0, 300)[:, None]


# name -> (H, W, n, K, angles float64 [n, K] in degrees)
CELLS = {
    "a_normal": (28, 28, 3, 16, lambda: D.rot_angles(3, 16, "normal")),       # the workload; 784 = 3 * 256 + 16; frame 0 at angle 0
    "b_rsre":   (28, 28, 3, 16, lambda: D.rot_angles(3, 16, "rsre", np.random.RandomState(0))),   # seed 0: negative, > a turn
    "c_oblong": (9, 13, 2, 3, lambda: np.array([[0.0, 33.0, -151.5], [17.25, 200.0, 75.0]])),     # axis order, two centres
    "d_min":    (4, 4, 1, 2, lambda: np.array([[0.0, 37.0]])),                # shortest recursion; stencil mirrored at both ends
    "e_max":    (64, 64, 1, 2, lambda: np.array([[0.0, 123.4]])),             # the LDS size; 16 strided passes
    "f_many":   (28, 28, 300, 1, _f_many_angles),                             # workgroup indexing beyond one wave of groups
}


@functools.lru_cache(maxsize=None)
def cell_angles(name):
    return CELLS[name][4]()


@functools.lru_cache(maxsize=None)
def cell_input(name):
    """Seeded fp32 noise images [n, H, W] in [-0.5, 0.5)."""
    H, W, n, _, _ = CELLS[name]
    g = torch.Generator().manual_seed(sorted(CELLS).index(name))
    return torch.rand((n, H, W), generator=g, dtype=torch.float32) - 0.5


def edge_mask(angles, H, W):
    """bool [n, K, H, W]: pixels left out of a comparison -- the float64 source point lies within EDGE of 0, H - 1 or W - 1 on
    either axis.  At angle exactly 0 the fp32 coordinates are exact (the table holds (1, 0)) and nothing is left out."""
    py, px = D.rot_source_points(angles, H, W)
    near = lambda p, hi: (np.abs(p) <= EDGE) | (np.abs(p - hi) <= EDGE)      # noqa: E731
    m = near(py, H - 1) | near(px, W - 1)
    m &= (np.asarray(angles) != 0.0)[..., None, None]
    return torch.from_numpy(m)


def oracle(images, angles, cval):
    """-> (raw float64 [n, K, H, W], out float64, per-frame range [n, K], edge mask)."""
    raw = D.rotate_reference(images, angles, cval)
    flat = raw.reshape(raw.shape[0], raw.shape[1], -1)
    return raw, D.normalise_reference(raw), flat.max(-1).values - flat.min(-1).values, edge_mask(angles, *raw.shape[2:])


@functools.lru_cache(maxsize=None)
def cell_oracle(name):
    return oracle(cell_input(name), cell_angles(name), CVAL)


def check_frames(got_raw, got_out, want, what):
    """The kernel's raw / out (either may be None) against an oracle() tuple: raw within RAW_TOL, out within OUT_TOL / r per
    frame, edge pixels left out, their share <= MAX_EDGE_SHARE.  Prints the measured maxima; -> (max raw error, max of out
    error * r / OUT_TOL, share left out)."""
    raw, out, r, edge = want
    share = float(edge.double().mean())
    assert float(r.min()) >= MIN_RANGE, float(r.min())
    e_raw = e_out = 0.0
    if got_raw is not None:
        e_raw = float((got_raw.cpu().double() - raw).abs()[~edge].max())
    if got_out is not None:
        rel = (got_out.cpu().double() - out).abs() * r[..., None, None] / OUT_TOL
        assert bool(torch.isfinite(got_out).all())
        e_out = float(rel[~edge].max())
    print(what, "max |raw - oracle|", e_raw, "bound", RAW_TOL, "| max |out - oracle| * r", e_out * OUT_TOL, "bound", OUT_TOL,
          "| edge share", share, "| min range", float(r.min()))
    assert share <= MAX_EDGE_SHARE
    assert e_raw <= RAW_TOL
    assert e_out <= 1.0
    return e_raw, e_out, share


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def fixture_angles(mode):
    """The angles rotate_data drew for the fixture: its seed on a stream of its own (RandomState(s) is what np.random.seed(s)
    makes of the global one)."""
    f = fixture()
    return D.rot_angles(3, int(f["K"]), mode, np.random.RandomState(int(f["seed"])))
