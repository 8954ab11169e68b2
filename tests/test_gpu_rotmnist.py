"""GPU: gode_rot_clips on every cell of tests/rotmnist_ref.py against the float64 oracle within the derived
bounds, against what the reference's rotate_data returned (tests/golden/rotmnist_ref.npz), bit for bit across its input and
output forms, inside its buffers, and RotMnistOnDevice.from_digits / resample / the batch streams built on it."""
import ctypes as C

import numpy as np
import pytest
import torch

import rotmnist_ref as R
import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import data as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(R.CELLS))
def test_cell_against_the_float64_oracle(name):
    H, W, n, K, _ = R.CELLS[name]
    x, angles = R.cell_input(name), R.cell_angles(name)
    out, raw = D.rotate_clips(x.cuda(), angles, cval=R.CVAL, want_raw=True)
    assert out.dtype == raw.dtype == torch.float32 and tuple(out.shape) == tuple(raw.shape) == (n, K, H, W)
    assert out.is_contiguous() and raw.is_contiguous()
    R.check_frames(raw, out, R.cell_oracle(name), name)
    table = D.rot_table(angles)
    still = torch.from_numpy(angles == 0.0)
    if name in ("a_normal", "c_oblong", "d_min", "e_max"):
        assert bool(still[:, 0].any())
    for d, k in still.nonzero().tolist():                   # angle 0: the identity, nothing left out
        assert table[d, k].tolist() == [1.0, 0.0]
        err = float((raw[d, k].cpu() - x[d]).abs().max())
        print(name, "angle 0, digit", d, "max |raw - input|", err)
        assert err <= 1e-5
        assert not bool(R.cell_oracle(name)[3][d, k].any())


@pytest.mark.parametrize("mode", R.MODES)
def test_fixture_of_the_reference_rotate_data(mode):
    """The kernel against the reference's own output, not only against the restatement: same per-frame bound."""
    f = R.fixture()
    images = torch.from_numpy(f["images"].reshape(3, 28, 28))
    angles = R.fixture_angles(mode)
    got = D.rotate_clips(images.cuda(), angles, cval=-0.5)
    raw, _, r, edge = R.oracle(images, angles, -0.5)
    want = torch.from_numpy(f["X_" + mode]).reshape(3, 16, 28, 28)
    assert float(r.min()) >= R.MIN_RANGE and float(edge.double().mean()) <= R.MAX_EDGE_SHARE
    rel = (got.cpu().double() - want).abs() * r[..., None, None] / R.OUT_TOL
    print(mode, "max |out - rotate_data| * r", float(rel[~edge].max()) * R.OUT_TOL, "bound", R.OUT_TOL, "edge share",
          float(edge.double().mean()))
    assert float(rel[~edge].max()) <= 1.0


def test_input_and_output_forms_agree_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (5, 28, 28), dtype=torch.uint8, generator=g)
    angles = D.rot_angles(5, 4, "rsre", np.random.RandomState(1))
    f32 = (u8.float() - 127.5) / 255.0                       # utils/images.py:71 in fp32
    out, raw = D.rotate_clips(u8.cuda(), angles, want_raw=True)
    out_f, raw_f = D.rotate_clips(f32.cuda(), angles, want_raw=True)
    assert torch.equal(out, out_f) and torch.equal(raw, raw_f)
    assert torch.equal(D.rotate_clips(u8.cuda(), angles), out)                                   # out alone
    assert torch.equal(D.rotate_clips(u8.cuda(), angles, want_raw=True, want_out=False), raw)    # raw alone
    again = D.rotate_clips(u8.cuda(), angles, want_raw=True)                                     # a second run
    assert torch.equal(again[0], out) and torch.equal(again[1], raw)
    assert bool(torch.isfinite(out).all()) and float(out.min()) == 0.0
    # in_scale / in_shift on load: one fused multiply-add
    scaled = D.rotate_clips(f32.cuda(), angles, want_raw=True, want_out=False, in_scale=0.5, in_shift=0.125)
    assert torch.equal(scaled, D.rotate_clips((f32.double() * 0.5 + 0.125).float().cuda(), angles, want_raw=True, want_out=False))


@pytest.mark.parametrize("name", ["c_oblong", "a_normal"])
def test_nothing_is_written_outside_out_and_raw(name):
    H, W, n, K, _ = R.CELLS[name]
    x, angles = R.cell_input(name).cuda(), R.cell_angles(name)
    numel, guard = n * K * H * W, 4096
    buf = torch.full((2, guard + numel + guard), float("nan"), device="cuda")
    cs = D.rot_table(angles).cuda()
    op = L.RotClipsOp(images=x.data_ptr(), cs=cs.data_ptr(), out=buf[0, guard:].data_ptr(), raw=buf[1, guard:].data_ptr(), n=n, K=K,
                      H=H, W=W, in_u8=0, in_scale=1.0, in_shift=0.0, cval=R.CVAL)
    L.run_one(op, G.engine.stream_ptr())
    out, raw = D.rotate_clips(x, angles, cval=R.CVAL, want_raw=True)
    for row, want in ((buf[0], out), (buf[1], raw)):
        assert bool(torch.isnan(row[:guard]).all()) and bool(torch.isnan(row[guard + numel:]).all())
        assert torch.equal(row[guard:guard + numel], want.flatten())


def test_a_constant_image_gives_non_finite_frames_for_that_digit_only():
    """Zero is the constant every fp32 step carries exactly (prefilter, taps, cval = 0): max - min is exactly 0 and the frame
    divides by zero, as in the reference.  It is not special-cased."""
    x = R.cell_input("b_rsre").clone()
    x[1] = 0.0
    out, raw = D.rotate_clips(x.cuda(), R.cell_angles("b_rsre"), cval=0.0, want_raw=True)
    assert bool((raw[1] == 0).all()) and not bool(torch.isfinite(out[1]).any())
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all()) and bool(torch.isfinite(raw).all())


def _digits(n=12):
    g = torch.Generator().manual_seed(8)
    return torch.randint(0, 256, (n, 28, 28), dtype=torch.uint8, generator=g), torch.arange(n) % 10


def test_from_digits_streams_are_those_of_a_set_built_from_the_same_clips():
    digits, labels = _digits()
    ds = D.RotMnistOnDevice.from_digits(digits, labels, K=16, mode="rsre", seed=9, angle_rng=np.random.RandomState(2))
    assert ds.X.is_cuda and tuple(ds.X.shape) == (12, 16, 1, 28, 28) and ds.X.is_contiguous() and ds.X.dtype == torch.float32
    assert ds.Y.is_cuda and ds.Y.dtype == torch.int64 and ds.Y.tolist() == labels.tolist() and ds.digits.is_cuda
    assert np.array_equal(ds.angles, D.rot_angles(12, 16, "rsre", np.random.RandomState(2)))
    assert torch.equal(ds.X[:, :, 0], D.rotate_clips(digits.cuda(), ds.angles))
    twin = D.RotMnistOnDevice(ds.X.clone(), seed=9, labels=labels)
    streams = [(s.videos(5, labels=True), s.images(4, labels=True)) for s in (ds, twin)]
    for _ in range(5):                                       # more than two epochs of either
        (v, vl), (i, il) = next(streams[0][0]), next(streams[0][1])
        (wv, wvl), (wi, wil) = next(streams[1][0]), next(streams[1][1])
        assert v.is_cuda and vl.is_cuda and tuple(v.shape) == (5, 16, 1, 28, 28) and tuple(i.shape) == (4, 1, 28, 28)
        assert torch.equal(v, wv) and torch.equal(vl, wvl) and torch.equal(i, wi) and torch.equal(il, wil)
    onehot = torch.nn.functional.one_hot(labels, 10).double().numpy()         # the rows extract_labels builds
    assert D.RotMnistOnDevice.from_digits(digits.numpy(), onehot, K=2).Y.tolist() == labels.tolist()


def test_resample_rebuilds_in_place():
    """[0, 1]: the minimum of a frame is exactly 0 (x / r - min / r at x = min); its maximum is fl(fl(max / r) - fl(min / r)) with
    r = fl(max - min): both quotients are below 2 in magnitude (|x| <= 1, r >= 0.5), each carries the rounding of r and its own
    (2 * 2^-24 relative), so the difference lies within 2 * 2 * 2 * 2^-24 + 2^-24 < 2^-20 of 1."""
    digits, labels = _digits()
    ds = D.RotMnistOnDevice.from_digits(digits, labels, K=16, mode="normal", seed=9, angle_rng=np.random.RandomState(4))
    X0, ptr = ds.X.clone(), ds.X.data_ptr()
    assert ds.resample() is ds and ds.X.data_ptr() == ptr and torch.equal(ds.X, X0)          # "normal": bit for bit
    ds.resample("rsre")
    assert ds.X.data_ptr() == ptr and ds.mode == "rsre" and not torch.equal(ds.X, X0)
    assert np.array_equal(ds.angles, D.rot_angles(12, 16, "rsre", np.random.RandomState(4)))
    assert torch.equal(ds.X[:, :, 0], D.rotate_clips(digits.cuda(), ds.angles))
    X1 = ds.X.clone()
    ds.resample()                                            # the mode sticks; the stream moves on
    assert not torch.equal(ds.X, X1)
    for X in (X1, ds.X):
        print("resample: min", float(X.min()), "max - 1", float(X.max()) - 1.0)
        assert bool(torch.isfinite(X).all()) and float(X.min()) == 0.0 and float(X.max()) <= 1.0 + 2.0 ** -20
        assert bool((X.flatten(2).min(2).values == 0).all())


def test_c_abi_refusals_return_their_codes_without_launching():
    x = torch.zeros((1, 65, 65), dtype=torch.float32, device="cuda")          # large enough for every shape named below
    cs = torch.tensor([[[1.0, 0.0]]], device="cuda")
    out = torch.full((2, 65 * 65), float("nan"), device="cuda")
    good = dict(images=x.data_ptr(), cs=cs.data_ptr(), out=out[0].data_ptr(), raw=out[1].data_ptr(), n=1, K=1, H=28, W=28,
                in_u8=0, in_scale=1.0, in_shift=0.0, cval=-0.5)
    fn = L.lib().gode_rot_clips
    st = G.engine.stream_ptr()
    assert fn(None, st) == -1
    for change, code in ((dict(images=None), -1), (dict(cs=None), -1), (dict(out=None, raw=None), -1), (dict(n=0), -1),
                         (dict(n=-3), -1), (dict(K=0), -1), (dict(in_u8=2), -1), (dict(H=3), -2), (dict(H=65), -2),
                         (dict(W=3), -2), (dict(W=65), -2)):
        assert fn(C.byref(L.RotClipsOp(**{**good, **change})), st) == code, change
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                      # nothing ran
    assert fn(C.byref(L.RotClipsOp(**good)), st) == 0        # and the unchanged op is served
    torch.cuda.synchronize()
    assert bool((out[1, :784] == 0).all()) and bool(torch.isnan(out[:, 784:]).all())      # raw: the zero image at angle 0
    assert not bool(torch.isfinite(out[0, :784]).any())                                     # out: that constant frame
