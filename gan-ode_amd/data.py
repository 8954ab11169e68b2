"""The step immediately upstream of the hot path: Rotated-MNIST clips.

Reference: dataset/mnist_rotation.py:7-63 -- `rot-mnist_rand.mat` holds X [n, 16, 784] in [0, 1] and Y; the first
N=500 clips are the training set, viewed as [N, 16, 1, 28, 28]; the image dataset returns one random frame per clip.
The whole training set is 25 MB in fp32, so it lives on the GPU and batches are gathered there (no per-step H2D);
the discriminators read the [B, T, C, H, W] batch in place through strides (no transpose copy).

UCF-101 (dataset/ucf101new.py) gets the same treatment, DESIGN section 21: frames are resized, cropped and quantised ONCE on
the GPU (gode_resize_u8) into one uint8 store, and every step gathers and normalises its windows there (gode_clip_gather).
The arithmetic of the resize is fixed by bicubic_taps / resize_crop_reference below.  Video decoding is the caller's.

The file itself is what utils/images.py:101-173 (rotate_data) makes of raw MNIST digits; DESIGN section 25 builds it on the GPU
(gode_rot_clips: RotMnistOnDevice.from_digits / resample / save_mat, rotate_clips), with rot_angles, rotate_reference and
normalise_reference as the float64 statement of its arithmetic and read_idx_images / read_idx_labels for the IDX files.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L


def load_rot_mnist(path, train=True, N=500, T=16):
    """-> (X float32 [N, T, 1, 28, 28], Y); same slicing as MNISTRotationVideo.__init__."""
    from scipy.io import loadmat
    if not os.path.exists(path):
        raise FileExistsError(f"File {path} does not exists")
    data = loadmat(path)
    X = torch.from_numpy(np.ascontiguousarray(data["X"].squeeze())).float()
    Y = torch.from_numpy(np.ascontiguousarray(data["Y"].squeeze()))
    if train:
        return X[:N].reshape(N, T, 1, 28, 28), Y[:N]
    return X[N:].reshape(-1, T, 1, 28, 28), Y[N:]


class MNISTRotationVideo(torch.utils.data.Dataset):
    """Drop-in for dataset.MNISTRotationVideo (host tensors, for the reference's DataLoader)."""

    def __init__(self, path_to_data, train=True, N=500, T=16, transform=None):
        self.X, self.Y = load_rot_mnist(path_to_data, train, N, T)
        self.transform = transform

    def __len__(self):
        return len(self.Y)

    def __getitem__(self, idx):
        v = self.X[idx]
        if self.transform is not None:
            v = self.transform(v)
        return v.float(), self.Y[idx]


class MNISTRotationImage(MNISTRotationVideo):
    """Drop-in for dataset.MNISTRotationImage: a random frame of clip idx (np.random.randint, as the reference)."""

    def __init__(self, path_to_data, train=True, N=500, T=16, transform=None):
        super().__init__(path_to_data, train, N, T, transform)
        self.T = T

    def __getitem__(self, idx):
        img = self.X[idx, np.random.randint(0, self.T)]
        if self.transform is not None:
            img = self.transform(img)
        return img.float(), self.Y[idx]


def _class_labels(labels, n, what):
    """Class indices int64 [n] from class indices or from the one-hot rows extract_labels builds (utils/images.py:84-94)."""
    y = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if y.ndim == 2 and y.shape[1] > 1:
        y = np.argmax(y == 1, axis=1)              # np.where(y == 1)[0][0] per row (utils/images.py:137)
    y = y.reshape(-1)
    if y.shape[0] != n:
        raise ValueError(f"{what}: {y.shape[0]} labels for {n} clips")
    return torch.from_numpy(np.ascontiguousarray(y.astype(np.int64)))


class RotMnistOnDevice:
    """Device-resident training set with shuffled, drop_last batch streams (what DataLoader(shuffle=True,
    drop_last=True) + dataGen() deliver in mnist_moco_ode.py:56-71), gathered on the GPU.

    The clips come from a `rot-mnist_rand.mat` file or a tensor, or are built on the GPU from raw digits by from_digits
    (gode_rot_clips); such a set can draw fresh angles with resample() and write the file with save_mat().
    Y: int64 classes [N] on the device (None when no labels were given)."""

    def __init__(self, path_or_tensor, device="cuda", N=500, T=16, seed=None, labels=None):
        if torch.is_tensor(path_or_tensor):
            X = path_or_tensor
        else:
            X, Y = load_rot_mnist(path_or_tensor, True, N, T)
            labels = Y if labels is None else labels
        self.X = X.to(device).contiguous()             # [N, T, 1, 28, 28]
        self.N, self.T = self.X.shape[0], self.X.shape[1]
        self.Y = None if labels is None else _class_labels(labels, self.N, "RotMnistOnDevice").to(self.X.device)
        self.digits = self.angles = self.mode = self.angle_rng = None       # set by from_digits
        self.cval = -0.5
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(seed)

    @classmethod
    def from_digits(cls, digits_uint8, labels=None, K=16, mode="normal", device="cuda", seed=None, angle_rng=None):
        """The set rotate_data (utils/images.py:101-173) builds from raw digits, made on the GPU: uint8 [n, H, W] (the bytes of
        the IDX file, read_idx_images; 4 <= H, W <= 64) -> X [n, K, 1, H, W] in one gode_rot_clips launch.  The digits stay on
        the device for resample().  labels: class indices [n] or one-hot rows [n, 10].  mode / angle_rng: rot_angles' (the
        angles of "rand-end" / "rsre" come from NumPy's global stream unless angle_rng is given); seed: the batch streams'."""
        d = torch.as_tensor(digits_uint8)
        if d.dtype != torch.uint8 or d.dim() != 3:
            raise ValueError(f"RotMnistOnDevice.from_digits: uint8 digits [n, H, W] expected, got {d.dtype} {tuple(d.shape)}")
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"RotMnistOnDevice.from_digits(device={device!r}): the rotation runs on the GPU; libgode has no "
                               "CPU or PyTorch fallback")
        d = d.to(device).contiguous()
        angles = rot_angles(d.shape[0], K, mode, angle_rng)
        ds = cls(rotate_clips(d, angles).unsqueeze(2), device=device, seed=seed, labels=labels)
        ds.digits, ds.angles, ds.mode, ds.angle_rng = d, angles, mode, angle_rng
        return ds

    def resample(self, mode=None):
        """Draw new angles (mode: this call's and the later ones'; default the set's) and rebuild X in place: fresh "rand-end" /
        "rsre" clips per epoch, one launch.  "normal" reproduces X bit for bit."""
        if self.digits is None:
            raise RuntimeError("RotMnistOnDevice.resample: the set holds no digits (it was not built by from_digits)")
        angles = rot_angles(self.N, self.T, self.mode if mode is None else mode, self.angle_rng)
        rotate_clips(self.digits, angles, cval=self.cval, out=self.X.view(self.N, self.T, *self.X.shape[3:]))
        self.angles, self.mode = angles, (self.mode if mode is None else mode)
        return self

    def save_mat(self, path):
        """The file the reference drivers load (utils/images.py:220): X float64 [n, K, H * W], Y float64 [n, 1]."""
        from scipy.io import savemat
        if self.Y is None:
            raise ValueError("RotMnistOnDevice.save_mat: the set has no labels")
        savemat(path, {"X": self.X.reshape(self.N, self.T, -1).cpu().double().numpy(),
                       "Y": self.Y.cpu().double().numpy().reshape(-1, 1)})

    def _epochs(self, batch):
        while True:
            perm = torch.randperm(self.N, generator=self.gen)
            for i in range(0, self.N - batch + 1, batch):
                yield perm[i:i + batch]

    def _labelled(self, x, idx, labels):
        if not labels:
            return x
        if self.Y is None:
            raise ValueError("RotMnistOnDevice: labels=True on a set without labels")
        return x, self.Y[idx]

    def videos(self, batch, labels=False):
        """Endless stream of [B, T, 1, 28, 28] batches; labels=True: (batch, int64 [B] classes on the device)."""
        for idx in self._epochs(batch):
            idx = idx.to(self.X.device)
            yield self._labelled(self.X[idx], idx, labels)

    def images(self, batch, labels=False):
        """Endless stream of [B, 1, 28, 28] batches, one uniform frame per drawn clip; labels as in videos()."""
        for idx in self._epochs(batch):
            frame = torch.randint(0, self.T, (batch,), generator=self.gen)
            idx = idx.to(self.X.device)
            yield self._labelled(self.X[idx, frame.to(self.X.device)], idx, labels)


# ======================================================================================================================
# Rotated-MNIST clips from raw digits
# ======================================================================================================================
def _open_idx(path):
    import gzip
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def _read_idx(path, magic, ndim, count, what):
    with _open_idx(path) as f:
        head = f.read(4 + 4 * ndim)
        if len(head) != 4 + 4 * ndim or int.from_bytes(head[:4], "big") != magic:
            raise ValueError(f"{what}: {path} is not an IDX file with magic {magic}")
        dims = [int.from_bytes(head[4 + 4 * i:8 + 4 * i], "big") for i in range(ndim)]
        if count is not None:
            if count < 0 or count > dims[0]:
                raise ValueError(f"{what}: {count} items asked of the {dims[0]} in {path}")
            dims[0] = int(count)
        size = int(np.prod(dims))
        buf = f.read(size)
    if len(buf) != size:
        raise ValueError(f"{what}: {path} ends after {len(buf)} of {size} bytes")
    return np.frombuffer(buf, dtype=np.uint8).reshape(dims).copy()


def read_idx_images(path, count=None):
    """The MNIST image file (train-images-idx3-ubyte, gzipped or not) -> uint8 [n, rows, cols]: the bytes extract_data reads
    (utils/images.py:64-74) before its rescaling, which gode_rot_clips applies on load.  count: only the first `count`.
    Nothing is downloaded."""
    return _read_idx(path, 2051, 3, count, "read_idx_images")


def read_idx_labels(path, count=None):
    """The MNIST label file (train-labels-idx1-ubyte, gzipped or not) -> int64 classes [n] (utils/images.py:84-90; the one-hot
    rows built there only serve to be turned back into these indices at :137)."""
    return _read_idx(path, 2049, 1, count, "read_idx_labels").astype(np.int64)


ROT_MODES = ("normal", "rand-end", "rsre")


def rot_angles(n, K=16, mode="normal", rng=None):
    """float64 [n, K]: the angles in degrees rotate_data (utils/images.py:107-136) gives each of n digits.
      normal    linspace(0, 359.99, K) for every digit
      rand-end  linspace(0, e, K), e = uniform(-269.99, 269.99) pushed 90 degrees away from zero (e < 0: e - 90, else e + 90)
      rsre      linspace(s, e, K), s = uniform(-89.99, 89.99) drawn first, then e = uniform(-269.99, 269.99)
    The draws are the reference's np.random.uniform calls in its order, digit by digit, from NumPy's global stream when rng is
    None (after np.random.seed(s) these are the reference's angles for that seed), else from rng (a RandomState or Generator).
    Not reproduced: the reference's closing `rnd_idx = np.random.shuffle(np.arange(n))` -- shuffle returns None, so X[None, :]
    shuffles nothing and only adds an axis that .squeeze() removes; it draws from the stream AFTER all angles."""
    if mode not in ROT_MODES:
        raise ValueError(f"rot_angles: mode {mode!r}; the reference has " + ", ".join(repr(m) for m in ROT_MODES))
    n, K = int(n), int(K)
    if n < 0 or K < 1:
        raise ValueError(f"rot_angles: n = {n}, K = {K}")
    uniform = np.random.uniform if rng is None else rng.uniform
    out = np.empty((n, K), dtype=np.float64)
    for k in range(n):
        if mode == "normal":
            out[k] = np.linspace(0, 359.99, K)
        elif mode == "rand-end":
            end = uniform(-269.99, 269.99)
            end = end - 90 if end < 0 else end + 90
            out[k] = np.linspace(0, end, K)
        else:
            start = uniform(-89.99, 89.99)
            end = uniform(-269.99, 269.99)
            out[k] = np.linspace(start, end, K)
    return out


_SPLINE_POLE = math.sqrt(3.0) - 2.0


def _spline_prefilter64(c):
    """The cubic B-spline recursive filter along the LAST axis of a float64 array (a copy): gain 6, pole sqrt(3) - 2, mirror
    boundary -- one axis of scipy.ndimage.spline_filter(a, 3, mode='mirror')."""
    z, n = _SPLINE_POLE, c.shape[-1]
    c = c * 6.0
    zn1 = z ** (n - 1)
    c0 = c[..., 0] + zn1 * c[..., n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[..., i] + zn1 * c[..., n - 1 - i])
        zi *= z
    c[..., 0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[..., i] += z * c[..., i - 1]
    c[..., n - 1] = (z * c[..., n - 2] + c[..., n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def _rot_weights64(t):
    return ((1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
            (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0)


def _mirror(i, n):
    i = np.abs(i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def rot_source_points(angles, H, W):
    """float64 (p_y, p_x), each [n, K, H, W]: the input point output pixel (y, x) of every frame reads."""
    a = np.deg2rad(np.asarray(angles, dtype=np.float64))
    c, s = np.cos(a)[..., None, None], np.sin(a)[..., None, None]
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    dy, dx = np.arange(H, dtype=np.float64)[:, None] - cy, np.arange(W, dtype=np.float64)[None, :] - cx
    return cy + c * dy + s * dx, cx - s * dy + c * dx


def _as_images64(images, what):
    x = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    if x.ndim != 3:
        raise ValueError(f"{what}: images must be [n, H, W], got {tuple(x.shape)}")
    if min(x.shape[1:]) < L.ROT_MIN_SIZE:
        raise ValueError(f"{what}: images of {x.shape[1]} x {x.shape[2]}; each side is at least {L.ROT_MIN_SIZE}")
    return x.astype(np.float64)


def _as_angles64(angles, n, what):
    a = np.asarray(angles.detach().cpu().numpy() if torch.is_tensor(angles) else angles, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != n or a.shape[1] < 1:
        raise ValueError(f"{what}: angles must be [n, K] degrees with n = {n} and K >= 1, got {tuple(a.shape)}")
    return a


def rotate_reference(images, angles, cval=-0.5):
    """[n, H, W] values (NumPy or torch, taken to float64) and angles [n, K] in degrees -> float64 tensor [n, K, H, W]:
    scipy.ndimage.rotate(image, angle, reshape=False, cval=cval, order=3) restated in float64 -- the prefilter along both
    axes, the source point of every output pixel, cval outside [0, H - 1] x [0, W - 1], else 4 x 4 cubic B-spline taps with
    mirrored indices.  The oracle of gode_rot_clips (its `raw` output); agrees with scipy to ~1e-14."""
    x = _as_images64(images, "rotate_reference")
    n, H, W = x.shape
    a = _as_angles64(angles, n, "rotate_reference")
    coef = _spline_prefilter64(np.swapaxes(_spline_prefilter64(np.swapaxes(x, 1, 2)), 1, 2))      # axis 0, then axis 1
    py, px = rot_source_points(a, H, W)
    inside = (py >= 0) & (py <= H - 1) & (px >= 0) & (px <= W - 1)
    py, px = np.where(inside, py, 0.0), np.where(inside, px, 0.0)
    fy, fx = np.floor(py), np.floor(px)
    wy, wx = _rot_weights64(py - fy), _rot_weights64(px - fx)
    iy, ix = fy.astype(np.int64) - 1, fx.astype(np.int64) - 1
    digit = np.arange(n)[:, None, None, None]
    out = np.zeros_like(py)
    for j in range(4):
        yj = _mirror(iy + j, H)
        for i in range(4):
            out += wy[j] * wx[i] * coef[digit, yj, _mirror(ix + i, W)]
    return torch.from_numpy(np.where(inside, out, float(cval)))


def normalise_reference(frames):
    """[..., H, W] -> float64 tensor of the same shape: every frame min-max normalised as utils/images.py:166-167 writes it,
    x / (max - min) first, then minus the minimum of that quotient.  A constant frame divides by zero and comes out
    non-finite, as in the reference."""
    x = (frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)).astype(np.float64)
    flat = x.reshape(x.shape[:-2] + (-1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = flat / (flat.max(-1, keepdims=True) - flat.min(-1, keepdims=True))
        q = q - q.min(-1, keepdims=True)
    return torch.from_numpy(q.reshape(x.shape))


def rot_table(angles):
    """float32 tensor [n, K, 2] = (cos, sin) of the angles in degrees: evaluated in float64, rounded once.  Angle 0 gives
    exactly (1, 0)."""
    a = np.deg2rad(np.asarray(angles, dtype=np.float64))
    return torch.from_numpy(np.stack([np.cos(a), np.sin(a)], axis=-1).astype(np.float32))


def rotate_clips(images, angles, cval=-0.5, want_raw=False, want_out=True, out=None, in_scale=1.0, in_shift=0.0):
    """gode_rot_clips: device images [n, H, W] -- uint8 (taken through the reference's (v - 127.5f) / 255.0f on load) or fp32 --
    and host angles [n, K] in degrees -> fp32 [n, K, H, W] min-max normalised frames (`out`: written there when given); with
    want_raw (out, raw), raw the rotated frames before normalisation; want_out=False: raw alone.  4 <= H, W <= 64."""
    from .engine import stream_ptr
    if not torch.is_tensor(images) or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError("rotate_clips: uint8 or float32 images expected, got "
                         f"{images.dtype if torch.is_tensor(images) else type(images).__name__}")
    if images.dim() != 3 or not images.is_contiguous():
        raise ValueError(f"rotate_clips: images must be a contiguous [n, H, W] tensor, got {tuple(images.shape)}")
    n, H, W = images.shape
    if not (L.ROT_MIN_SIZE <= H <= L.ROT_MAX_SIZE and L.ROT_MIN_SIZE <= W <= L.ROT_MAX_SIZE):
        raise ValueError(f"rotate_clips: images of {H} x {W}; gode_rot_clips takes sides of {L.ROT_MIN_SIZE} to "
                         f"{L.ROT_MAX_SIZE}")
    a = _as_angles64(angles, n, "rotate_clips")
    K = a.shape[1]
    if not (want_out or want_raw):
        raise ValueError("rotate_clips: neither the normalised nor the raw frames are wanted")
    _require_cuda(images, "rotate_clips: images")
    shape = (n, K, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=images.device) if want_out else None
    elif (not want_out or tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
          or out.device != images.device):
        raise ValueError(f"rotate_clips: out must be a contiguous float32 {shape} on {images.device}")
    raw = torch.empty(shape, dtype=torch.float32, device=images.device) if want_raw else None
    if n:
        cs = rot_table(a).to(images.device)
        op = L.RotClipsOp(images=images.data_ptr(), cs=cs.data_ptr(), out=out.data_ptr() if want_out else None,
                          raw=raw.data_ptr() if want_raw else None, n=n, K=K, H=H, W=W,
                          in_u8=int(images.dtype == torch.uint8), in_scale=in_scale, in_shift=in_shift, cval=cval)
        L.run_one(op, stream_ptr())
    if want_out and want_raw:
        return out, raw
    return out if want_out else raw


# ======================================================================================================================
# UCF-101
# ======================================================================================================================
def _taps64(n_in, n_out, antialias, first=0, count=None):
    """Per output index i in [first, first + count): (first input index, float64 weights of the contiguous input range).
    The separable weights that torch.nn.functional.interpolate(x.double(), mode="bicubic", align_corners=False,
    antialias=antialias) evaluates along one axis of n_in -> n_out, in double."""
    n_in, n_out = int(n_in), int(n_out)
    count = n_out - first if count is None else int(count)
    if n_in < 1 or n_out < 1 or first < 0 or count < 1 or first + count > n_out:
        raise ValueError(f"bicubic_taps: outputs [{first}, {first + count}) leave the resized axis of {n_out} (input {n_in})")
    s = n_in / n_out
    rows = []
    for i in range(first, first + count):
        if antialias:
            A = -0.5
            support, inv = (2.0 * s, 1.0 / s) if s >= 1.0 else (2.0, 1.0)
            c = s * (i + 0.5)
            lo = max(int(c - support + 0.5), 0)
            n = min(int(c + support + 0.5), n_in) - lo
            w = []
            for j in range(n):
                x = abs((j + lo - c + 0.5) * inv)
                w.append(((A + 2.0) * x - (A + 3.0)) * x * x + 1.0 if x < 1.0 else
                         ((((x - 5.0) * x + 8.0) * x - 4.0) * A if x < 2.0 else 0.0))
            total = math.fsum(w)
            rows.append((lo, [v / total for v in w]))
        else:
            A = -0.75
            src = s * (i + 0.5) - 0.5
            ix = math.floor(src)
            t = src - ix
            cc1 = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0           # noqa: E731
            cc2 = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A     # noqa: E731
            taps = (cc2(t + 1.0), cc1(t), cc1(1.0 - t), cc2(2.0 - t))
            idx = [min(max(ix - 1 + k, 0), n_in - 1) for k in range(4)]
            w = [0.0] * (idx[3] - idx[0] + 1)
            for k in range(4):                      # taps that clamp to one index are merged, added in double
                w[idx[k] - idx[0]] += taps[k]
            rows.append((idx[0], w))
    return rows


def bicubic_taps(n_in, n_out, antialias, first=0, count=None):
    """The tap table of one axis, as gode_resize_u8 reads it: (first int32 [n], count int32 [n], weights float32 [n, k], k)
    for the outputs [first, first + count) of a bicubic n_in -> n_out resize.  Output i reads the inputs
    [first[i], first[i] + count[i]) with weights[i, :count[i]] (zero behind); computed in double, rounded once to fp32."""
    rows = _taps64(n_in, n_out, antialias, first, count)
    k = max(len(w) for _, w in rows)
    w64 = torch.zeros(len(rows), k, dtype=torch.float64)
    for r, (_, w) in enumerate(rows):
        w64[r, :len(w)] = torch.tensor(w, dtype=torch.float64)
    return (torch.tensor([f for f, _ in rows], dtype=torch.int32), torch.tensor([len(w) for _, w in rows], dtype=torch.int32),
            w64.float(), k)


def _dense_taps64(n_in, n_out, antialias, first=0, count=None):
    """The same table as a dense float64 matrix [count, n_in] (weights NOT rounded to fp32)."""
    rows = _taps64(n_in, n_out, antialias, first, count)
    m = torch.zeros(len(rows), int(n_in), dtype=torch.float64)
    for r, (f, w) in enumerate(rows):
        m[r, f:f + len(w)] = torch.tensor(w, dtype=torch.float64)
    return m


def _check_frames(frames, what):
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise ValueError(f"{what}: uint8 frames expected (decoded video), got "
                         f"{frames.dtype if torch.is_tensor(frames) else type(frames).__name__}")
    if frames.dim() != 4:
        raise ValueError(f"{what}: frames must be [F, H, W, C] (or [F, C, H, W] with channels_first=True), got "
                         f"{tuple(frames.shape)}")


def _check_crop(out_w, crop_left, crop_w, what):
    if crop_left < 0 or crop_w < 1 or crop_left + crop_w > out_w:
        raise ValueError(f"{what}: the crop [{crop_left}, {crop_left + crop_w}) leaves the resized width {out_w}")


def resize_crop_reference(frames_uint8, out_h, out_w, crop_left, crop_w, antialias):
    """uint8 [F, H, W, C] -> (v float64 [F, out_h, crop_w, C], bytes uint8 of the same shape): the bicubic resize to
    out_h x out_w with only the columns [crop_left, crop_left + crop_w) kept, evaluated in float64 from the tables of
    bicubic_taps (before their rounding to fp32) as two matrix products, and its quantisation clamp -> round half to even ->
    cast.  The oracle of gode_resize_u8 and the resize of the host drop-ins UCF101Video / UCF101Image."""
    _check_frames(frames_uint8, "resize_crop_reference")
    _check_crop(out_w, crop_left, crop_w, "resize_crop_reference")
    x = frames_uint8.cpu().double()
    wy = _dense_taps64(x.shape[1], out_h, antialias)
    wx = _dense_taps64(x.shape[2], out_w, antialias, crop_left, crop_w)
    v = torch.einsum("yh,fhxc->fyxc", wy, torch.einsum("xw,fhwc->fhxc", wx, x))
    return v, v.clamp(0.0, 255.0).round().to(torch.uint8)


def _check_taps(first, count, k, n_in, axis):
    if k > L.RESIZE_MAX_TAPS:
        raise ValueError(f"gode_resize_u8: {k} taps along {axis} exceed the kernel's maximum of {L.RESIZE_MAX_TAPS} "
                         "(antialiased downscales beyond 8x are not served)")
    if bool((count < 1).any()) or bool((count > k).any()) or bool((first < 0).any()) or bool((first + count > n_in).any()):
        raise ValueError(f"gode_resize_u8: a tap range along {axis} is empty, longer than {k} or leaves the input of {n_in}")


def _require_cuda(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be a GPU tensor: libgode has no CPU or PyTorch fallback")


class ResizeTables:
    """The two tap tables of one source size on the device: H x W -> out_h x out_w, columns [crop_left, crop_left + crop_w)."""

    def __init__(self, H, W, out_h, out_w, crop_left, crop_w, antialias, device):
        _check_crop(out_w, crop_left, crop_w, "ResizeTables")
        yf, yc, yw, self.ky = bicubic_taps(H, out_h, antialias)
        xf, xc, xw, self.kx = bicubic_taps(W, out_w, antialias, crop_left, crop_w)
        _check_taps(yf, yc, self.ky, H, "y")
        _check_taps(xf, xc, self.kx, W, "x")
        self.H, self.W, self.out_h, self.out_w = int(H), int(W), int(out_h), int(crop_w)
        self.sum_abs = (float(yw.double().abs().sum(1).max()), float(xw.double().abs().sum(1).max()))     # Sy, Sx
        if torch.device(device).type != "cuda":
            raise RuntimeError(f"ResizeTables: device {device!r}: libgode has no CPU or PyTorch fallback")
        self.y_first, self.y_count, self.y_w, self.x_first, self.x_count, self.x_w = (
            t.contiguous().to(device) for t in (yf, yc, yw, xf, xc, xw))


def resize_u8(frames, tables, dst=None, want_f32=False):
    """gode_resize_u8 on a uint8 device tensor [F, H, W, C] of ANY strides (a permuted [F, C, H, W] view goes in as it is).
    -> dst (uint8 [F, out_h, out_w, C] contiguous; allocated unless given), or (dst, v fp32) with want_f32."""
    from .engine import stream_ptr
    _check_frames(frames, "resize_u8")
    _require_cuda(frames, "resize_u8: frames")
    F, H, W, Cn = frames.shape
    if Cn not in (1, 3):
        raise ValueError(f"resize_u8: {Cn} channels; frames have 1 or 3")
    if (H, W) != (tables.H, tables.W):
        raise ValueError(f"resize_u8: frames are {H} x {W}, the tables were built for {tables.H} x {tables.W}")
    shape = (F, tables.out_h, tables.out_w, Cn)
    if dst is None:
        dst = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif tuple(dst.shape) != shape or dst.dtype != torch.uint8 or not dst.is_contiguous() or dst.device != frames.device:
        raise ValueError(f"resize_u8: dst must be a contiguous uint8 {shape} on {frames.device}")
    v = torch.empty(shape, dtype=torch.float32, device=frames.device) if want_f32 else None
    if F:
        op = L.ResizeU8Op(src=frames.data_ptr(), dst=dst.data_ptr(), dst_f32=v.data_ptr() if want_f32 else None,
                          y_first=tables.y_first.data_ptr(), y_count=tables.y_count.data_ptr(), y_w=tables.y_w.data_ptr(),
                          x_first=tables.x_first.data_ptr(), x_count=tables.x_count.data_ptr(), x_w=tables.x_w.data_ptr(),
                          ss=(C.c_int64 * 4)(*frames.stride()), F=F, Hin=H, Win=W, C=Cn, out_h=tables.out_h, out_w=tables.out_w,
                          ky=tables.ky, kx=tables.kx)
        L.run_one(op, stream_ptr())
    return (dst, v) if want_f32 else dst


def clip_gather(frames, first_frames, T, sub=128.0, inv=1.0 / 128.0):
    """gode_clip_gather: uint8 store [n_frames, ...] + int64 device indices [B] -> fp32 [B, T, ...] = (x - sub) * inv of the
    frames [first, first + T) of every clip; a clip that leaves the store is NaN."""
    from .engine import stream_ptr
    _require_cuda(frames, "clip_gather: frames")
    if frames.dtype != torch.uint8 or not frames.is_contiguous() or frames.dim() < 2 or frames.shape[0] < 1:
        raise ValueError("clip_gather: frames must be a contiguous, non-empty uint8 store [n_frames, ...]")
    if not (torch.is_tensor(first_frames) and first_frames.dtype == torch.int64 and first_frames.dim() == 1
            and first_frames.device == frames.device and first_frames.is_contiguous() and first_frames.numel() >= 1):
        raise ValueError(f"clip_gather: first_frames must be a contiguous int64 tensor [B] on {frames.device}")
    B, T = first_frames.shape[0], int(T)
    if T < 1:
        raise ValueError(f"clip_gather: T = {T}")
    out = torch.empty((B, T) + tuple(frames.shape[1:]), dtype=torch.float32, device=frames.device)
    op = L.ClipGatherOp(frames=frames.data_ptr(), first=first_frames.data_ptr(), out=out.data_ptr(), n_frames=frames.shape[0],
                        frame_elems=frames[0].numel(), B=B, T=T, sub=sub, inv=inv)
    L.run_one(op, stream_ptr())
    return out


class Ucf101OnDevice:
    """Device-resident UCF-101 training set: every added video is resized (bicubic to image_size x resized_width), cropped
    (columns crop_left .. crop_left + image_size) and quantised ONCE by gode_resize_u8 into one uint8 store
    [n_frames, S, S, C]; videos() / images() are the endless shuffled drop_last batch streams of ucf_moco_ode.py:56-74, each
    batch one gode_clip_gather launch.  Decoding is the caller's: add_video takes decoded uint8 frames.

    Sampling (a torch.Generator of the object's own, seeded by `seed`; the global torch / NumPy streams are not touched): per
    epoch one randperm over the kept videos; a clip starts uniformly on [0, L - n_frame - 1) as ucf101new.py:88 draws it, and
    at 0 for L <= n_frame + 1, where that draw raises in the reference; an image is a uniform frame of [0, L).

    gather: a callable (first_frames int64 [B], T) -> batch that replaces the kernel launch (the index stream can then be
    exercised without a GPU, on frames appended with add_resized); it is the only way to construct the set off a GPU."""

    GEOMETRY = ("n_frame", "image_size", "resized_width", "crop_left", "antialias")

    def __init__(self, device="cuda", n_frame=16, image_size=64, resized_width=85, crop_left=10, antialias=False, seed=None,
                 gather=None):
        self.device = torch.device(device)
        if self.device.type != "cuda" and gather is None:
            raise RuntimeError(f"Ucf101OnDevice(device={device!r}): the set lives on the GPU; libgode has no CPU or PyTorch "
                               "fallback")
        if n_frame < 1 or image_size < 1:
            raise ValueError(f"Ucf101OnDevice: n_frame={n_frame}, image_size={image_size}")
        _check_crop(resized_width, crop_left, image_size, "Ucf101OnDevice")
        self.n_frame, self.image_size, self.resized_width, self.crop_left = int(n_frame), int(image_size), int(resized_width), int(crop_left)
        self.antialias = bool(antialias)
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(seed)
        self._gather = gather
        self._store = None                      # uint8 [capacity, S, S, C]
        self.n_frames = 0
        self._offsets, self._lengths, self._labels = [], [], []
        self._index = None                      # the three lists as int64 host tensors, rebuilt after an append
        self._tables = {}                       # (H, W) -> ResizeTables

    # ---- building ----------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self._lengths)

    @property
    def frames(self):
        """The stored frames, uint8 [n_frames, S, S, C] (a view of the store)."""
        if self._store is None:
            raise RuntimeError("Ucf101OnDevice: no video has been added")
        return self._store[:self.n_frames]

    def _reserve(self, F, Cn):
        """Room for F more frames; the store grows geometrically.  -> the uint8 [F, S, S, C] slot."""
        S = self.image_size
        if self._store is not None and self._store.shape[3] != Cn:
            raise ValueError(f"Ucf101OnDevice: a video with {Cn} channels in a set of {self._store.shape[3]}-channel frames")
        need = self.n_frames + F
        if self._store is None or need > self._store.shape[0]:
            grown = torch.empty((max(need, 2 * (0 if self._store is None else self._store.shape[0]), 1024), S, S, Cn),
                                dtype=torch.uint8, device=self.device)
            if self.n_frames:
                grown[:self.n_frames].copy_(self._store[:self.n_frames])
            self._store = grown
        return self._store[self.n_frames:need]

    def _commit(self, F, label):
        self._offsets.append(self.n_frames)
        self._lengths.append(int(F))
        self._labels.append(int(label))
        self.n_frames += int(F)
        self._index = None

    def add_video(self, frames, label=0, channels_first=False):
        """Append one decoded video: uint8 [F, H, W, C] (channels_first: [F, C, H, W]) on the host or the device, any H, W,
        C = 1 or 3.  -> False, and nothing stored, for a video shorter than n_frame (make_dataset's filter)."""
        _check_frames(frames, "Ucf101OnDevice.add_video")
        if channels_first:
            frames = frames.permute(0, 2, 3, 1)             # a view: the kernel reads through strides
        F, H, W, Cn = frames.shape
        if Cn not in (1, 3):
            raise ValueError(f"Ucf101OnDevice.add_video: {Cn} channels; frames have 1 or 3")
        if F < self.n_frame:
            return False
        if self.device.type != "cuda":
            raise RuntimeError("Ucf101OnDevice.add_video: the resize runs on the GPU; libgode has no CPU or PyTorch fallback")
        key = (int(H), int(W))
        if key not in self._tables:
            self._tables[key] = ResizeTables(H, W, self.image_size, self.resized_width, self.crop_left, self.image_size,
                                             self.antialias, self.device)
        resize_u8(frames.to(self.device, non_blocking=True), self._tables[key], dst=self._reserve(F, Cn))
        self._commit(F, label)
        return True

    def add_resized(self, frames, label=0):
        """Append frames that already are uint8 [F, S, S, C] (a store built elsewhere).  -> False for F < n_frame."""
        _check_frames(frames, "Ucf101OnDevice.add_resized")
        S = self.image_size
        if tuple(frames.shape[1:3]) != (S, S) or frames.shape[3] not in (1, 3):
            raise ValueError(f"Ucf101OnDevice.add_resized: frames must be [F, {S}, {S}, 1 or 3], got {tuple(frames.shape)}")
        if frames.shape[0] < self.n_frame:
            return False
        self._reserve(frames.shape[0], frames.shape[3]).copy_(frames)
        self._commit(frames.shape[0], label)
        return True

    @classmethod
    def from_videos(cls, videos, labels=None, channels_first=False, **kw):
        """A set from a list of decoded videos (labels: one class per video, default 0); **kw: the constructor's."""
        ds = cls(**kw)
        for i, v in enumerate(videos):
            ds.add_video(v, 0 if labels is None else int(labels[i]), channels_first=channels_first)
        return ds

    def save(self, path):
        """The store, the per-video tables and the geometry in one torch.save file: decoding and resizing happen once per
        dataset, not once per run."""
        idx = self._tabs()
        torch.save({"format": 1, "frames": self.frames.cpu(), "offsets": idx[0], "lengths": idx[1], "labels": idx[2],
                    "geometry": {k: getattr(self, k) for k in self.GEOMETRY}}, path)

    @classmethod
    def load(cls, path, device="cuda", seed=None, gather=None, **geometry):
        """The set save() wrote.  Geometry fields (n_frame, image_size, resized_width, crop_left, antialias) passed explicitly
        must agree with the file's."""
        d = torch.load(path, map_location="cpu")
        unknown = set(geometry) - set(cls.GEOMETRY)
        if unknown:
            raise TypeError(f"Ucf101OnDevice.load: unknown arguments {sorted(unknown)}")
        for k, v in geometry.items():
            if d["geometry"][k] != v:
                raise ValueError(f"Ucf101OnDevice.load: {path} was built with {k}={d['geometry'][k]!r}, not {v!r}")
        ds = cls(device=device, seed=seed, gather=gather, **d["geometry"])
        frames = d["frames"]
        ds._store = frames.to(ds.device).contiguous()
        ds.n_frames = frames.shape[0]
        ds._offsets, ds._lengths, ds._labels = (d[k].tolist() for k in ("offsets", "lengths", "labels"))
        return ds

    # ---- sampling ----------------------------------------------------------------------------------------------
    def _tabs(self):
        if self._index is None:
            self._index = tuple(torch.tensor(t, dtype=torch.int64) for t in (self._offsets, self._lengths, self._labels))
        return self._index

    def _upload(self, t):
        """A small host tensor to the device: from pinned memory, without blocking the host."""
        if self.device.type != "cuda":
            return t
        return t.pin_memory().to(self.device, non_blocking=True)

    def _check_batch(self, batch):
        if batch < 1 or batch > len(self):
            raise ValueError(f"Ucf101OnDevice: batch {batch} with {len(self)} kept videos (drop_last would never yield)")

    def _epochs(self, batch):
        while True:
            perm = torch.randperm(len(self), generator=self.gen)
            for i in range(0, len(perm) - batch + 1, batch):
                yield perm[i:i + batch]

    def _draw(self, span):
        """One uniform integer on [0, span[i]) per entry, from the object's generator."""
        u = torch.rand(span.shape[0], generator=self.gen, dtype=torch.float64)
        return torch.minimum((u * span).long(), span - 1)

    def gather(self, first_frames, T):
        """The raw op: int64 [B] first stored frames (on the set's device) -> fp32 [B, T, S, S, C] = (x - 128) / 128."""
        if self._gather is not None:
            return self._gather(first_frames, T)
        return clip_gather(self.frames, first_frames, T)

    def videos(self, batch, labels=False):
        """Endless stream of [B, T, C, S, S] fp32 batches: permuted VIEWS of the gather's channels-last [B, T, S, S, C], which
        the driver's transpose(1, 2) and the discriminator's strided read consume without a copy.  labels=True: (batch,
        int64 [B] classes on the device)."""
        self._check_batch(batch)
        return self._video_stream(batch, labels)

    def _video_stream(self, batch, labels):
        for idx in self._epochs(batch):
            off, length, lab = self._tabs()
            start = self._draw((length[idx] - self.n_frame - 1).clamp_(min=1))
            v = self.gather(self._upload(off[idx] + start), self.n_frame).permute(0, 1, 4, 2, 3)
            yield (v, self._upload(lab[idx])) if labels else v

    def images(self, batch, labels=False):
        """Endless stream of [B, C, S, S] fp32 batches (views of [B, S, S, C]): one uniform frame of each drawn video."""
        self._check_batch(batch)
        return self._image_stream(batch, labels)

    def _image_stream(self, batch, labels):
        for idx in self._epochs(batch):
            off, length, lab = self._tabs()
            x = self.gather(self._upload(off[idx] + self._draw(length[idx])), 1)[:, 0].permute(0, 3, 1, 2)
            yield (x, self._upload(lab[idx])) if labels else x


def _torchvision_reader():
    try:
        from torchvision.io import read_video
    except ImportError as e:
        raise ImportError("UCF101Video / UCF101Image: no `reader` was given and the default one needs the package "
                          "torchvision (torchvision.io.read_video), which is not installed; pass reader=callable(path) -> "
                          "uint8 [F, H, W, 3]") from e
    return lambda path: read_video(path, pts_unit="sec")[0]


class UCF101Video(torch.utils.data.Dataset):
    """Host drop-in for dataset.UCF101Video (dataset/ucf101new.py:13-98; the reference's constructor arguments): `root` holds
    the videos under video_folder/<class>/<file> and classInd.txt / {train,test}list0<fold>.txt under annotation_folder.
    samples: (path, frames, class) of every listed video of a known class with at least n_frame frames.  An item is a random
    window of n_frame frames (start drawn on NumPy's global generator as the reference; 0 where that draw would raise),
    resized to image_size x 85, cropped to columns 10 .. 10 + image_size and normalised: (float32 [T, 3, S, S], class).
    reader: callable path -> uint8 [F, H, W, 3]; default torchvision.io.read_video (ImportError at construction without it).
    The resize is resize_crop_reference, the arithmetic gode_resize_u8 implements."""

    resized_width, crop_left, antialias = 85, 10, False
    drops_short_videos = True

    def __init__(self, root, video_folder, annotation_folder, n_frame=16, train=True, fold=1, image_size=64, reader=None):
        super().__init__()
        self._setup(root, video_folder, annotation_folder, n_frame, train, fold, image_size, reader)
        self.classes, self.class_to_idx = self.find_classes()
        self.samples = self.make_dataset()

    def _setup(self, root, video_folder, annotation_folder, n_frame, train, fold, image_size, reader):
        assert fold in [1, 2, 3], f"fold need to have value 1,2 or 3, not {fold}"
        self.video_folder = os.path.join(root, video_folder)
        self.annotation_folder = os.path.join(root, annotation_folder)
        self.train, self.n_frame, self.fold, self.image_size = train, n_frame, fold, image_size
        self.reader = _torchvision_reader() if reader is None else reader

    def find_classes(self):
        """classInd.txt: one '<index> <name>' per line -> (names, name -> index)."""
        classes, class_to_idx = [], {}
        with open(os.path.join(self.annotation_folder, "classInd.txt")) as f:
            for line in f:
                if line.strip():
                    index, name = line.split()[:2]
                    classes.append(name)
                    class_to_idx[name] = int(index)
        return classes, class_to_idx

    def make_dataset(self):
        """The listed videos ('<class>/<file> [label]' per line) of known classes: (path, frames, class)."""
        name = f"{'train' if self.train else 'test'}list0{self.fold}.txt"
        with open(os.path.join(self.annotation_folder, name)) as f:
            listed = [line.split()[0] for line in f if line.strip()]
        samples = []
        for rel in listed:
            cls = rel.split("/")[0]
            if cls not in self.class_to_idx:
                continue
            path = os.path.join(self.video_folder, rel)
            length = int(self.reader(path).shape[0])
            if self.drops_short_videos and length < self.n_frame:
                continue
            samples.append((path, length, self.class_to_idx[cls]))
        return samples

    def __len__(self):
        return len(self.samples)

    def resize_crop(self, x):
        """uint8 [..., 3, H, W] -> uint8 [..., 3, S, S]."""
        lead = x.shape[:-3]
        frames = x.reshape((-1,) + tuple(x.shape[-3:])).permute(0, 2, 3, 1)
        out = resize_crop_reference(frames, self.image_size, self.resized_width, self.crop_left, self.image_size,
                                    self.antialias)[1]
        return out.permute(0, 3, 1, 2).reshape(tuple(lead) + (x.shape[-3], self.image_size, self.image_size))

    def _normalise(self, x):
        return (x.float() - 128.0) / 128.0

    def __getitem__(self, index):
        path, length, cls = self.samples[index]
        span = length - self.n_frame - 1
        start = np.random.randint(0, span) if span > 0 else 0
        video = self.reader(path)[start:start + self.n_frame].permute(0, 3, 1, 2)
        return self._normalise(self.resize_crop(video)), cls

    def to_device(self, device="cuda", seed=None, gather=None):
        """The same samples as a Ucf101OnDevice (every video decoded once, resized on the GPU)."""
        ds = Ucf101OnDevice(device=device, n_frame=self.n_frame, image_size=self.image_size, resized_width=self.resized_width,
                            crop_left=self.crop_left, antialias=self.antialias, seed=seed, gather=gather)
        for path, _, cls in self.samples:
            ds.add_video(self.reader(path), cls)
        return ds


class UCF101Image(UCF101Video):
    """Host drop-in for dataset.UCF101Image (dataset/ucf101new.py:100-180): one uniform frame of video idx
    (np.random.randint(0, frames), as the reference) -> (float32 [3, S, S], class).  samples: share a UCF101Video's list
    (ucf_moco_ode.py:57); without it the list is built here, and, as in the reference, keeps videos shorter than n_frame."""

    drops_short_videos = False

    def __init__(self, root, video_folder, annotation_folder, samples=None, n_frame=16, train=True, fold=1, image_size=64,
                 reader=None):
        torch.utils.data.Dataset.__init__(self)
        self._setup(root, video_folder, annotation_folder, n_frame, train, fold, image_size, reader)
        if samples is None:
            self.classes, self.class_to_idx = self.find_classes()
            self.samples = self.make_dataset()
        else:
            self.samples = samples

    def __getitem__(self, index):
        path, length, cls = self.samples[index]
        image = self.reader(path)[np.random.randint(0, length)].permute(2, 0, 1)
        return self._normalise(self.resize_crop(image)), cls
