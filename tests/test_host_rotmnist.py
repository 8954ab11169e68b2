"""CPU: the host side of the Rotated-MNIST clip builder -- the float64 oracle rotate_reference against
scipy.ndimage.rotate, the angle modes and oracle against what the reference's own rotate_data returned
(tests/golden/rotmnist_ref.npz), the .mat round trip, the IDX readers, the labelled batch streams and every refusal of the op
wrapper.  No GPU."""
import gzip
import struct

import numpy as np
import pytest
import torch

import rotmnist_ref as R
from gan_ode_amd import _lib as L
from gan_ode_amd import data as D

# positive, negative, beyond 180 and beyond a turn.  Multiples of 90 other than 0 stay out: there source points lie on the input's
# edge to within an ulp, and on which side they fall follows from the order of three roundings, not from the arithmetic stated.
ANGLES = [0.0, 24.0, 96.0, 216.0, 359.99, -317.3, -45.5, 400.25]


@pytest.mark.parametrize("cval", [-0.5, 0.25])
@pytest.mark.parametrize("size", [(28, 28), (9, 13), (4, 4), (64, 64)])
def test_rotate_reference_is_scipy_ndimage_rotate_in_float64(size, cval):
    ndimage = pytest.importorskip("scipy.ndimage", reason="scipy is not installed")
    H, W = size
    x = np.random.RandomState(H * 100 + W).uniform(-0.5, 0.5, (2, H, W))
    angles = np.array([ANGLES, ANGLES[::-1]])
    got = D.rotate_reference(x, angles, cval)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, len(ANGLES), H, W)
    want = np.stack([[ndimage.rotate(x[i], a, reshape=False, cval=cval, order=3) for a in angles[i]] for i in range(2)])
    err = float(np.abs(got.numpy() - want).max())
    print(size, cval, "max |rotate_reference - scipy|", err)
    assert err <= 1e-12
    assert torch.equal(D.rotate_reference(torch.from_numpy(x).float(), angles, cval),
                       D.rotate_reference(x.astype(np.float32), angles, cval))         # NumPy and torch inputs alike


@pytest.mark.parametrize("mode", R.MODES)
def test_angles_and_oracle_reproduce_the_reference_rotate_data(mode):
    f = R.fixture()
    np.random.seed(int(f["seed"]))
    angles = D.rot_angles(3, int(f["K"]), mode)                        # the global stream, as the reference draws
    assert np.array_equal(angles, R.fixture_angles(mode))
    images = f["images"].reshape(3, 28, 28)
    assert images.dtype == np.float32
    X = D.normalise_reference(D.rotate_reference(images, angles, -0.5)).reshape(3, int(f["K"]), 784)
    want = f["X_" + mode]
    assert want.dtype == np.float64 and want.shape == (3, 16, 784)
    err = float((X - torch.from_numpy(want)).abs().max())
    print(mode, "max |oracle - rotate_data|", err)
    assert err <= 1e-6
    assert np.array_equal(D._class_labels(f["labels"], 3, "test").numpy(), f["Y_" + mode].astype(np.int64))
    assert f["Y_" + mode].tolist() == [7.0, 0.0, 3.0]


def test_angle_modes_draw_counts_fold_and_unknown_mode():
    n, K = 5, 7
    for mode, draws in (("normal", 0), ("rand-end", n), ("rsre", 2 * n)):
        np.random.seed(3)
        a = D.rot_angles(n, K, mode)
        after = np.random.uniform()
        np.random.seed(3)
        u = [np.random.uniform() for _ in range(draws)]
        assert np.random.uniform() == after, mode                     # exactly `draws` values were taken from the global stream
        assert a.dtype == np.float64 and a.shape == (n, K)
        rs = np.random.RandomState(3)
        assert np.array_equal(D.rot_angles(n, K, mode, rng=rs), a)    # a stream of one's own: the same draws
        if mode == "normal":
            assert all(np.array_equal(row, np.linspace(0, 359.99, K)) for row in a)
        elif mode == "rand-end":
            ends = np.array([-269.99 + 539.98 * v for v in u])
            assert (a[:, 0] == 0).all() and np.allclose(a[:, -1], ends + np.where(ends < 0, -90.0, 90.0), rtol=0, atol=1e-12)
            assert (np.abs(a[:, -1]) >= 90).all() and (ends < 0).any() and (ends >= 0).any()
        else:
            assert np.allclose(a[:, 0], [-89.99 + 179.98 * v for v in u[0::2]], rtol=0, atol=1e-12)     # the start is drawn first
            assert np.allclose(a[:, -1], [-269.99 + 539.98 * v for v in u[1::2]], rtol=0, atol=1e-12)
        assert np.allclose(np.diff(a, 2, axis=1), 0, atol=1e-10)      # equally spaced
    with pytest.raises(ValueError, match="mode"):
        D.rot_angles(3, 16, "random")
    with pytest.raises(ValueError):
        D.rot_angles(3, 0)


def test_normalise_reference_is_the_reference_expression_and_a_constant_frame_is_not_finite():
    x = np.random.RandomState(1).uniform(-0.5, 0.7, (2, 3, 6, 5))
    x[1, 2] = 0.125
    got = D.normalise_reference(x).numpy()
    flat = x.reshape(2, 3, 30)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = flat / (np.max(flat, 2, keepdims=True) - np.min(flat, 2, keepdims=True))
        q = q - np.min(q, 2, keepdims=True)
    assert np.array_equal(got.reshape(2, 3, 30), q, equal_nan=True)
    assert not np.isfinite(got[1, 2]).any() and np.isfinite(got[0]).all() and np.isfinite(got[1, :2]).all()
    assert got[0].min() == 0.0 and abs(got[0].max() - 1.0) < 1e-12


def _set(n=6, K=4, seed=2):
    g = torch.Generator().manual_seed(11)
    X = torch.rand((n, K, 1, 28, 28), generator=g)
    return D.RotMnistOnDevice(X, device="cpu", seed=seed, labels=[3, 1, 4, 1, 5, 9][:n]), X


def test_save_mat_round_trip_through_the_mat_readers(tmp_path):
    pytest.importorskip("scipy.io", reason="scipy is not installed")
    from scipy.io import loadmat
    ds, X = _set()
    path = str(tmp_path / "rot-mnist_rand.mat")
    ds.save_mat(path)
    m = loadmat(path)
    assert m["X"].dtype == np.float64 and m["X"].shape == (6, 4, 784) and m["Y"].dtype == np.float64 and m["Y"].shape == (6, 1)
    back, Y = D.load_rot_mnist(path, train=True, N=6, T=4)
    assert torch.equal(back, X) and Y.tolist() == [3.0, 1.0, 4.0, 1.0, 5.0, 9.0]
    vd = D.MNISTRotationVideo(path, train=True, N=4, T=4)
    assert len(vd) == 4 and torch.equal(vd[2][0], X[2]) and float(vd[2][1]) == 4.0
    assert len(D.MNISTRotationVideo(path, train=False, N=4, T=4)) == 2
    again = D.RotMnistOnDevice(path, device="cpu", N=6, T=4, seed=2)              # the file as a set: clips and classes
    assert torch.equal(again.X, X) and again.Y.tolist() == [3, 1, 4, 1, 5, 9]
    import dataset
    assert dataset.RotMnistOnDevice is D.RotMnistOnDevice
    unlabelled = D.RotMnistOnDevice(X, device="cpu")
    with pytest.raises(ValueError, match="labels"):
        unlabelled.save_mat(path)


def test_labelled_streams_have_the_documented_shapes_and_leave_the_plain_ones_unchanged():
    ds, X = _set(seed=5)
    plain, _ = _set(seed=5)
    sv, si = ds.videos(4, labels=True), ds.images(3, labels=True)
    pv, pi = plain.videos(4), plain.images(3)
    for _ in range(3):
        (v, vl), (i, il) = next(sv), next(si)
        assert tuple(v.shape) == (4, 4, 1, 28, 28) and tuple(i.shape) == (3, 1, 28, 28)
        assert vl.dtype == il.dtype == torch.int64 and tuple(vl.shape) == (4,) and tuple(il.shape) == (3,)
        assert torch.equal(v, next(pv)) and torch.equal(i, next(pi))             # labels=True draws nothing more
        for clip, lab in zip(v, vl):
            k = int((X == clip).flatten(1).all(1).nonzero())
            assert int(lab) == [3, 1, 4, 1, 5, 9][k]
    assert torch.is_tensor(next(plain.videos(2))) and torch.is_tensor(next(plain.images(2)))
    with pytest.raises(ValueError, match="labels"):
        next(D.RotMnistOnDevice(X, device="cpu").videos(2, labels=True))
    onehot = np.eye(10)[[3, 1, 4, 1, 5, 9]]
    assert D.RotMnistOnDevice(X, device="cpu", labels=onehot).Y.tolist() == [3, 1, 4, 1, 5, 9]
    with pytest.raises(ValueError, match="labels"):
        D.RotMnistOnDevice(X, device="cpu", labels=[1, 2])


def _write_idx(path, magic, dims, payload, gz):
    blob = struct.pack(">I", magic) + b"".join(struct.pack(">I", d) for d in dims) + payload
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(blob)


@pytest.mark.parametrize("gz", [False, True])
def test_idx_readers(tmp_path, gz):
    rs = np.random.RandomState(4)
    imgs = rs.randint(0, 256, (5, 28, 28)).astype(np.uint8)
    labs = rs.randint(0, 10, 5).astype(np.uint8)
    pi, pl = str(tmp_path / ("images.gz" if gz else "images")), str(tmp_path / ("labels.gz" if gz else "labels"))
    _write_idx(pi, 2051, imgs.shape, imgs.tobytes(), gz)
    _write_idx(pl, 2049, labs.shape, labs.tobytes(), gz)
    got = D.read_idx_images(pi)
    assert got.dtype == np.uint8 and np.array_equal(got, imgs) and got.flags.writeable
    assert np.array_equal(D.read_idx_images(pi, count=3), imgs[:3])
    y = D.read_idx_labels(pl)
    assert y.dtype == np.int64 and np.array_equal(y, labs) and np.array_equal(D.read_idx_labels(pl, 2), labs[:2])
    # what extract_data makes of the bytes is the expression the kernel applies on load
    assert np.array_equal((got.astype(np.float32) - (255 / 2.0)) / 255, ((torch.from_numpy(got).float() - 127.5) / 255.0).numpy())
    with pytest.raises(ValueError, match="magic"):
        D.read_idx_images(pl)
    with pytest.raises(ValueError, match="magic"):
        D.read_idx_labels(pi)
    with pytest.raises(ValueError, match="items"):
        D.read_idx_images(pi, count=6)
    _write_idx(pi, 2051, (6, 28, 28), imgs.tobytes(), gz)                        # a header that promises more than the file holds
    with pytest.raises(ValueError, match="ends after"):
        D.read_idx_images(pi)


def test_the_op_is_declared_once_and_the_wrapper_refuses_before_any_launch():
    assert L.RotClipsOp.KIND == L.OP_ROT_CLIPS == 40 and L.RotClipsOp.FN == "gode_rot_clips" in L.EXPORTS
    assert L.lib().gode_sizeof(L.OP_ROT_CLIPS) == 64
    a = np.zeros((2, 3))
    ok = torch.zeros((2, 28, 28), dtype=torch.uint8)
    for bad in (ok.double(), ok.to(torch.int32), ok.numpy()):
        with pytest.raises(ValueError, match="uint8 or float32"):
            D.rotate_clips(bad, a)
    with pytest.raises(ValueError, match="contiguous"):
        D.rotate_clips(torch.zeros((2, 28, 56), dtype=torch.uint8)[:, :, ::2], a)
    with pytest.raises(ValueError, match="contiguous"):
        D.rotate_clips(torch.zeros((2, 1, 28, 28), dtype=torch.uint8), a)
    for shape in ((2, 3, 28), (2, 28, 3), (2, 65, 28), (2, 28, 65)):
        with pytest.raises(ValueError, match="sides of 4 to 64"):
            D.rotate_clips(torch.zeros(shape, dtype=torch.float32), a)
    for angles in (np.zeros((2, 0)), np.zeros((3, 4)), np.zeros(2)):             # K < 1, another n, no [n, K]
        with pytest.raises(ValueError, match="angles"):
            D.rotate_clips(ok, angles)
    with pytest.raises(ValueError, match="neither"):
        D.rotate_clips(ok, a, want_out=False)
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D.rotate_clips(ok, a)                                                     # a valid call on the wrong device
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D.RotMnistOnDevice.from_digits(ok, device="cpu")
    with pytest.raises(ValueError, match="uint8 digits"):
        D.RotMnistOnDevice.from_digits(ok.float(), device="cpu")
    with pytest.raises(RuntimeError, match="from_digits"):
        D.RotMnistOnDevice(torch.zeros(2, 3, 1, 28, 28), device="cpu").resample()
    with pytest.raises(ValueError, match="at least 4"):
        D.rotate_reference(np.zeros((1, 3, 9)), np.zeros((1, 1)))
    # the C entry point's own refusals need no GPU either: they come before any launch
    lib = L.lib()
    assert lib.gode_rot_clips(None, None) == -1
    good = dict(images=16, cs=16, out=16, raw=16, n=1, K=1, H=28, W=28, in_u8=1, in_scale=1.0, in_shift=0.0, cval=-0.5)
    import ctypes as C
    for change, code in ((dict(images=None), -1), (dict(cs=None), -1), (dict(out=None, raw=None), -1), (dict(n=0), -1),
                         (dict(K=0), -1), (dict(in_u8=2), -1), (dict(H=3), -2), (dict(H=65), -2), (dict(W=3), -2), (dict(W=65), -2)):
        op = L.RotClipsOp(**{**good, **change})
        assert lib.gode_rot_clips(C.byref(op), None) == code, change
