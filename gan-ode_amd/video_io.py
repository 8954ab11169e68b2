"""Generated videos on disk: the drivers' genSamples (mnist_moco_ode.py:31-48, the same in all nine stage-3 drivers).

The reference samples n**2 videos in eval mode, copies them to the host, tiles them into one float64 [16, n*size, n*size, 3]
array, maps it through (x + 1) / 2 * 255 and hands it to skvideo.io.vwrite(...gif).  Here:

  gen_samples   the fast path: one gode_video_grid launch on the view sample_videos returns -- tiling, the float64 value map,
                clip, truncation and the palette index, bit for bit what NumPy computes -- one copy of T * (n*H) * (n*W)
                bytes to the host, and write_gif.
  vwrite        stands in for skvideo.io.vwrite on host arrays, so that a driver whose line 9 reads
                `from gan_ode_amd import video_io as io` runs its own genSamples unchanged.
  video_grid    the device op on any fp32 [B, C, T, H, W] view; write_gif: a GIF89a writer whose LZW runs in libgode
                (gode_gif_lzw, host C++).

Deviations from skvideo + ffmpeg, which pick a palette per file and dither: gray videos are written losslessly with a 256-gray
palette, colour ones are quantised to a fixed 6 x 7 x 6 cube without dithering.
"""
from __future__ import annotations

import math
import struct

import numpy as np
import torch

from . import _lib as L

MODES = {"tanh": 0, "unit": 1}      # gode_video_grid's `mode`: (x + 1) / 2 * 255 for [-1, 1]; x * 255 for [0, 1]
CUBE = (6, 7, 6)                    # levels per channel of the colour palette


def _cube_palette():
    pal = np.zeros((256, 3), dtype=np.uint8)                      # entries 252..255: black
    i = np.arange(CUBE[0] * CUBE[1] * CUBE[2])
    for c, q in enumerate((i // (CUBE[1] * CUBE[2]), (i // CUBE[2]) % CUBE[1], i % CUBE[2])):
        pal[:len(i), c] = (q * 255 + (CUBE[c] - 1) // 2) // (CUBE[c] - 1)
    return pal


GRAY_PALETTE = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
RGB676_PALETTE = _cube_palette()
GRAY_PALETTE.setflags(write=False)
RGB676_PALETTE.setflags(write=False)


def rgb676_index(rgb):
    """uint8 [..., 3] -> uint8 [...] cell of the 6 x 7 x 6 cube, the integer formula of gode_video_grid (include/gode.h)."""
    v = np.asarray(rgb).astype(np.int32)
    q = [(v[..., c] * (CUBE[c] - 1) + 127) // 255 for c in range(3)]
    return ((q[0] * CUBE[1] + q[1]) * CUBE[2] + q[2]).astype(np.uint8)


def video_grid(videos, n=None, mode="tanh", rgb=True, idx=False):
    """gode_video_grid: an fp32 GPU [B, C, T, H, W] tensor or view (C 1 or 3; read in place through its strides, never made
    contiguous) -> the n x n sample grid as device uint8 tensors: rgb [T, n*H, n*W, 3], idx [T, n*H, n*W] (palette indices:
    GRAY_PALETTE for C == 1, RGB676_PALETTE for C == 3), or the pair (rgb, idx) when both are asked for.  Video b fills tile
    (b // n, b % n); tiles behind the batch hold source value 0.  n defaults to ceil(sqrt(B)).  mode "tanh": values in [-1, 1]
    (generator output, UCF reals); "unit": values in [0, 1] (Rot-MNIST reals)."""
    from .engine import stream_ptr
    if not torch.is_tensor(videos) or videos.dtype != torch.float32 or videos.dim() != 5:
        raise ValueError("video_grid: a float32 [B, C, T, H, W] tensor expected, got "
                         f"{(videos.dtype, tuple(videos.shape)) if torch.is_tensor(videos) else type(videos).__name__}")
    if mode not in MODES:
        raise ValueError(f"video_grid: mode {mode!r}; one of {sorted(MODES)}")
    if not (rgb or idx):
        raise ValueError("video_grid: neither the colour frames nor the palette indices are wanted")
    B, C, T, H, W = videos.shape
    if C not in (1, 3):
        raise ValueError(f"video_grid: {C} channels; 1 or 3 expected")
    if min(B, T, H, W) < 1:
        raise ValueError(f"video_grid: empty videos {tuple(videos.shape)}")
    n = math.isqrt(B - 1) + 1 if n is None else int(n)
    if n < 1 or B > n * n:
        raise ValueError(f"video_grid: {B} videos do not fit a grid of {n} x {n}")
    if not videos.is_cuda:
        raise RuntimeError("video_grid: videos must be a GPU tensor: libgode has no CPU or PyTorch fallback")
    videos = videos.detach()
    with torch.cuda.device(videos.device):
        out_rgb = torch.empty((T, n * H, n * W, 3), dtype=torch.uint8, device=videos.device) if rgb else None
        out_idx = torch.empty((T, n * H, n * W), dtype=torch.uint8, device=videos.device) if idx else None
        op = L.VideoGridOp(src=videos.data_ptr(), xs=(L.i64 * 5)(*videos.stride()),
                           rgb=None if out_rgb is None else out_rgb.data_ptr(),
                           idx=None if out_idx is None else out_idx.data_ptr(),
                           B=B, C=C, T=T, H=H, W=W, rows=n, cols=n, mode=MODES[mode])
        L.run_one(op, stream_ptr())
    if rgb and idx:
        return out_rgb, out_idx
    return out_rgb if rgb else out_idx


def _lzw(frame, min_code_size):
    """One frame's indices (contiguous uint8) -> its GIF code stream, uint8 array (gode_gif_lzw)."""
    lib = L.lib()
    cap = lib.gode_gif_lzw_bound(frame.size)
    out = np.empty(cap, dtype=np.uint8)
    got = lib.gode_gif_lzw(frame.ctypes.data, frame.size, min_code_size, out.ctypes.data, cap)
    if got < 0:
        raise ValueError(f"write_gif: gode_gif_lzw failed with code {got}: an index outside the palette" if got == -1 else
                         f"write_gif: gode_gif_lzw failed with code {got}")
    return out[:got]


def _sub_blocks(data):
    """A code stream -> GIF data sub-blocks (a length byte, then at most 255 bytes), with the terminating empty block."""
    full, rest = divmod(len(data), 255)
    body = np.empty((full, 256), dtype=np.uint8)
    body[:, 0] = 255
    body[:, 1:] = data[:full * 255].reshape(full, 255)
    tail = bytes([rest]) + data[full * 255:].tobytes() + b"\0" if rest else b"\0"
    return body.tobytes() + tail


def write_gif(path, idx_frames, palette, fps=25, loop=0):
    """Writes palette-index frames as a GIF89a file.  idx_frames: host uint8 [T, H, W] (array or CPU tensor, any strides), every
    index below the palette's length; palette: uint8 [k, 3], 2 <= k <= 256 (the global colour table, padded with black to a
    power of two).  Every frame is shown for round(100 / fps) hundredths of a second; loop: the NETSCAPE2.0 repeat count, 0 =
    forever.  Returns path."""
    if torch.is_tensor(idx_frames):
        idx_frames = idx_frames.numpy()
    frames = np.asarray(idx_frames)
    if frames.dtype != np.uint8 or frames.ndim != 3 or frames.size == 0:
        raise ValueError(f"write_gif: uint8 [T, H, W] indices expected, got {frames.dtype} {frames.shape}")
    T, H, W = frames.shape
    if H > 65535 or W > 65535:
        raise ValueError(f"write_gif: a GIF screen is at most 65535 x 65535, got {H} x {W}")
    pal = np.asarray(palette)
    if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 2 <= pal.shape[0] <= 256:
        raise ValueError(f"write_gif: a uint8 [k, 3] palette with 2 <= k <= 256 expected, got {pal.dtype} {pal.shape}")
    if not fps > 0 or not 0 <= round(100 / fps) <= 65535:
        raise ValueError(f"write_gif: fps {fps}")
    if not 0 <= int(loop) <= 65535:
        raise ValueError(f"write_gif: loop {loop}")
    bits = max(1, (pal.shape[0] - 1).bit_length())                # colour table of 2 ** bits entries
    table = np.zeros((1 << bits, 3), dtype=np.uint8)
    table[:pal.shape[0]] = pal
    if int(frames.max()) >= pal.shape[0]:
        raise ValueError(f"write_gif: index {int(frames.max())} outside the palette of {pal.shape[0]} entries")
    min_code_size = max(2, bits)
    delay = round(100 / fps)
    with open(path, "wb") as f:
        f.write(b"GIF89a" + struct.pack("<HHBBB", W, H, 0x80 | ((bits - 1) << 4) | (bits - 1), 0, 0))
        f.write(table.tobytes())
        f.write(b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", int(loop)) + b"\0")
        for t in range(T):
            f.write(b"\x21\xf9\x04\x04" + struct.pack("<H", delay) + b"\0\0")            # disposal 1: leave in place
            f.write(b"\x2c" + struct.pack("<HHHHB", 0, 0, W, H, 0) + bytes([min_code_size]))
            f.write(_sub_blocks(_lzw(np.ascontiguousarray(frames[t]), min_code_size)))
        f.write(b"\x3b")
    return path


def _to_uint8(a):
    """What skvideo's FFmpegWriter.writeFrame makes of an array, clip(0, 255).astype(uint8) -- knowledge of the upstream package,
    not checked against it; uint8 passes unchanged."""
    return a if a.dtype == np.uint8 else np.clip(a, 0, 255).astype(np.uint8)


def vwrite(fname, videodata):
    """Stands in for skvideo.io.vwrite(fname, videodata) for GIF files: a host array [T, H, W, 3] or [T, H, W], float or
    integer, any strides (genSamples passes a transposed float64 view) is clipped to [0, 255], truncated to uint8 and written at
    write_gif's 25 frames a second, with the 256-gray palette when the three channels are equal everywhere, with the 6 x 7 x 6 cube
    otherwise.  Works frame by frame: no second copy of the whole array is made."""
    if not str(fname).lower().endswith(".gif"):
        raise ValueError(f"vwrite: {fname!r}: only GIF files are written")
    v = np.asarray(videodata)
    if not (v.ndim == 3 or (v.ndim == 4 and v.shape[3] == 3)) or v.size == 0 or v.dtype.kind not in "fiub":
        raise ValueError(f"vwrite: a numeric [T, H, W, 3] or [T, H, W] array expected, got {v.dtype} {v.shape}")
    T, H, W = v.shape[:3]
    idx = np.empty((T, H, W), dtype=np.uint8)
    gray = v.ndim == 3 or all(np.array_equal(v[t, ..., 0], v[t, ..., 1]) and np.array_equal(v[t, ..., 0], v[t, ..., 2])
                              for t in range(T))
    for t in range(T):
        if v.ndim == 3:
            idx[t] = _to_uint8(v[t])
        elif gray:
            idx[t] = _to_uint8(v[t, ..., 0])
        else:
            idx[t] = rgb676_index(_to_uint8(v[t]))
    return write_gif(fname, idx, GRAY_PALETTE if gray else RGB676_PALETTE)


def gen_samples(gen, n=8, e=1, size=None, video_sample_path="."):
    """genSamples on the device: n * n videos sampled in eval mode under no_grad (the generator is put back into training mode
    afterwards, unconditionally, as the reference does), one gode_video_grid launch on the returned view for the palette
    indices, one copy of T * (n*H) * (n*W) bytes to the host, and a GIF at f"{video_sample_path}/gensamples_id{e}.gif", whose
    path is returned.  size, when given, must be the generator's frame size (the reference's argument; 28 or 64)."""
    n = int(n)
    if n < 1:
        raise ValueError(f"gen_samples: n = {n}")
    frame = 28 if gen.mnist else 64
    if size is not None and int(size) != frame:
        raise ValueError(f"gen_samples: size={size}, but {type(gen).__name__} makes {frame} x {frame} frames")
    gen.eval()
    with torch.no_grad():
        videos = gen.sample_videos(n * n)[0]
    gen.train()
    idx = video_grid(videos, n=n, mode="tanh", rgb=False, idx=True)
    path = f"{video_sample_path}/gensamples_id{e}.gif"
    return write_gif(path, idx.cpu().numpy(), GRAY_PALETTE if videos.shape[1] == 1 else RGB676_PALETTE)
