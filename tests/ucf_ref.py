"""Shared by tests/test_host_ucf.py and tests/test_gpu_ucf.py (not collected): the resize cells, their seeded inputs and
float64 oracle results (computed once per cell), the derived tolerance, and a host twin of Ucf101OnDevice's batch streams."""
import functools

import torch

from gan_ode_amd import data as D

# the geometries the tap tables were checked at: (H, W, out_h, out_w)
GEOMETRIES = [(240, 320, 64, 85), (23, 31, 8, 11), (5, 7, 8, 11), (64, 85, 64, 85), (128, 171, 64, 85)]

# resize cells: name -> (H, W, out_h, out_w, crop_left, crop_w, F, C, channels_first)
CELLS = {
    "a_workload":   (240, 320, 64, 85, 10, 64, 2, 3, False),    # 15/16 taps antialiased, several bands, vector stores
    "b_ragged":     (23, 31, 8, 11, 1, 8, 4, 3, False),         # non-integer scale, one ragged band
    "c_upscale":    (5, 7, 8, 11, 0, 11, 4, 3, False),          # merged border taps, values beyond [0, 255], scalar stores
    "d_identity":   (64, 85, 64, 85, 10, 64, 2, 3, False),      # bytes == the input's kept columns
    "e_chw":        (23, 31, 8, 11, 1, 8, 4, 3, True),          # the reference's permuted [F, C, H, W] layout, read in place
    "f_gray":       (23, 31, 8, 11, 1, 8, 4, 1, False),         # C = 1, vector stores
    "g_gray_odd":   (5, 7, 8, 11, 0, 11, 4, 1, False),          # C = 1, scalar stores
}
MODES = [False, True]                                           # antialias
MAX_TIE_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def cell_input(name):
    """The seeded uint8 frames of a cell in the layout the cell feeds: [F, H, W, C], or [F, C, H, W] when channels_first."""
    H, W, _, _, _, _, F, C, chw = CELLS[name]
    torch.manual_seed(0)
    x = torch.randint(0, 256, (F, C, H, W) if chw else (F, H, W, C), dtype=torch.uint8)
    return x


@functools.lru_cache(maxsize=None)
def cell_oracle(name, antialias):
    """-> (v float64 [F, out_h, crop_w, C], bytes uint8, tolerance, ky, kx) of a cell; never modified by a test."""
    H, W, oh, ow, left, cw, F, C, chw = CELLS[name]
    x = cell_input(name)
    v, b = D.resize_crop_reference(x.permute(0, 2, 3, 1) if chw else x, oh, ow, left, cw, antialias)
    _, _, yw, ky = D.bicubic_taps(H, oh, antialias)
    _, _, xw, kx = D.bicubic_taps(W, ow, antialias, left, cw)
    return v, b, tolerance(yw, xw, ky, kx), ky, kx


def tolerance(yw, xw, ky, kx):
    """|dst_f32 - float64 oracle| bound: one rounding per tap of either pass, two for the two fp32 weights, two for the stores
    of the partial row and of the result, each at most half an ulp (2^-24 relative) of the largest partial sum, 255 * Sy * Sx
    with Sy, Sx = max over outputs of sum |w|."""
    sy, sx = float(yw.double().abs().sum(1).max()), float(xw.double().abs().sum(1).max())
    return (ky + kx + 4) * 2.0 ** -24 * 255.0 * sy * sx


def near_tie(v, tol):
    """Where clamp(v) lies within tol of a rounding tie k + 0.5."""
    c = v.clamp(0.0, 255.0)
    return ((c - c.floor()) - 0.5).abs() <= tol


def check_bytes(got, v, want, tol):
    """The stored bytes against the oracle's: equal wherever the value is farther than tol from a tie, within 1 elsewhere;
    -> share of values in the tie window."""
    tie = near_tie(v, tol)
    got, want = got.cpu().to(torch.int16), want.to(torch.int16)
    assert torch.equal(got[~tie], want[~tie]), int((got[~tie] != want[~tie]).sum())
    if bool(tie.any()):
        assert int((got[tie] - want[tie]).abs().max()) <= 1
    return float(tie.double().mean())


def host_gather(frames):
    """A gather hook over a host uint8 store: the reference's (x - 128.0) / 128.0 on the indexed frames."""
    def gather(first, T):
        idx = first.cpu()[:, None] + torch.arange(T)[None, :]
        return (frames[idx].float() - 128.0) / 128.0
    return gather


def host_twin(ds, seed):
    """Ucf101OnDevice on the host over the SAME stored bytes and tables as the device set `ds`, with the reference arithmetic
    as its gather: its streams are what the device set must deliver for the same seed."""
    frames = ds.frames.cpu()
    twin = D.Ucf101OnDevice(device="cpu", n_frame=ds.n_frame, image_size=ds.image_size, resized_width=ds.resized_width,
                            crop_left=ds.crop_left, antialias=ds.antialias, seed=seed, gather=host_gather(frames))
    off, length, lab = ds._tabs()
    for o, n, c in zip(off.tolist(), length.tolist(), lab.tolist()):
        assert twin.add_resized(frames[o:o + n], c)
    return twin
