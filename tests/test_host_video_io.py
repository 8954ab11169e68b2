"""CPU: the host side of gan_ode_amd.video_io -- gode_gif_lzw round trips through the decoder of
tests/gif_decode.py (one index, a run, the 4096-entry clear, a two-valued stream at min_code_size 2, streams that end exactly at
and one code behind every growth of the code width), its capacity contract, write_gif's blocks by parsing, vwrite on the array
the drivers' genSamples builds, the op's ABI, and every refusal of gode_video_grid (returned before any launch, so no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import video_io as V

from gif_decode import lzw_decode, read_gif

GUARD = 16


def _encode(idx, mcs=8, cap=None):
    """-> (return value, the whole buffer: cap bytes and GUARD bytes of 0xA5 behind them)"""
    idx = np.ascontiguousarray(idx, dtype=np.uint8)
    lib = L.lib()
    cap = lib.gode_gif_lzw_bound(idx.size) if cap is None else cap
    buf = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    rc = lib.gode_gif_lzw(idx.ctypes.data, idx.size, mcs, buf.ctypes.data, cap)
    return rc, buf


def _random_stream():
    return np.random.RandomState(7).randint(0, 256, 70000).astype(np.uint8)


def _width_cases():
    """Prefixes of the random stream whose code streams end exactly at (suffix 'at') and one code behind ('after') each growth
    of the code width: the decoder's table reaches 512 / 1024 / 2048 entries with data code 255 / 767 / 1791, so the end code of
    such a stream is the first code of the new width.  LZW is greedy, so the first j codes of a prefix that ends on a code
    boundary of the whole stream are the whole stream's first j codes."""
    full = _random_stream()[:6000]
    rc, buf = _encode(full)
    ends = np.cumsum(lzw_decode(buf[:rc], 8).code_lengths)
    cases = []
    for width, j in ((10, 255), (11, 767), (12, 1791)):
        cases.append((f"{width}bit_at", full[:ends[j - 1]], j, width))
        cases.append((f"{width}bit_after", full[:ends[j]], j + 1, width))
    cases.append(("9bit_before", full[:ends[253]], 254, 9))
    return cases


def _streams():
    rs = np.random.RandomState(3)
    return ([("one", np.array([200], dtype=np.uint8), 8),
             ("run", np.full(5000, 7, dtype=np.uint8), 8),
             ("random", _random_stream(), 8),
             ("two_valued", rs.randint(0, 2, 3000).astype(np.uint8), 2),
             ("four_valued_fills_table", rs.randint(0, 4, 40000).astype(np.uint8), 2)]
            + [(name, s, 8) for name, s, _, _ in _width_cases()])


STREAMS = _streams()


@pytest.mark.parametrize("name,idx,mcs", STREAMS, ids=[s[0] for s in STREAMS])
def test_lzw_round_trip_and_capacity(name, idx, mcs):
    rc, buf = _encode(idx, mcs)                                   # cap = bound
    bound = L.lib().gode_gif_lzw_bound(idx.size)
    assert 0 < rc <= bound, (rc, bound)
    assert (buf[bound:] == 0xA5).all()
    d = lzw_decode(buf[:rc], mcs)
    assert np.array_equal(d.data, idx)
    if name in ("random", "four_valued_fills_table"):
        assert d.clears >= 2, "the table never reached 4096 entries"
    else:
        assert d.clears == 1
    # exactly enough room: the same bytes; one byte short: refused, nothing behind out + cap written
    rc2, buf2 = _encode(idx, mcs, cap=rc)
    assert rc2 == rc and np.array_equal(buf2[:rc], buf[:rc]) and (buf2[rc:] == 0xA5).all()
    rc3, buf3 = _encode(idx, mcs, cap=rc - 1)
    assert rc3 < 0 and (buf3[rc - 1:] == 0xA5).all()
    assert np.array_equal(buf3[:rc - 1], buf[:rc - 1])            # what fitted is the stream's head


@pytest.mark.parametrize("name,idx,codes,width", _width_cases(), ids=[c[0] for c in _width_cases()])
def test_lzw_code_width_grows_where_the_decoder_expects_it(name, idx, codes, width):
    rc, buf = _encode(idx)
    d = lzw_decode(buf[:rc], 8)
    assert (d.codes, d.eoi_width, d.clears) == (codes, width, 1)
    assert np.array_equal(d.data, idx)


def test_lzw_refusals():
    lib = L.lib()
    one = np.array([4], dtype=np.uint8)
    out = np.zeros(8, dtype=np.uint8)
    assert lib.gode_gif_lzw(one.ctypes.data, 1, 2, out.ctypes.data, 8) == -1       # 4 needs three bits
    assert lib.gode_gif_lzw(one.ctypes.data, 1, 1, out.ctypes.data, 8) == -1
    assert lib.gode_gif_lzw(one.ctypes.data, 1, 9, out.ctypes.data, 8) == -1
    assert lib.gode_gif_lzw(None, 1, 8, out.ctypes.data, 8) == -1
    assert lib.gode_gif_lzw(one.ctypes.data, 1, 8, None, 8) == -1
    assert lib.gode_gif_lzw(one.ctypes.data, -1, 8, out.ctypes.data, 8) == -1
    assert lib.gode_gif_lzw(one.ctypes.data, 1, 8, out.ctypes.data, 0) == -2
    assert lib.gode_gif_lzw_bound(-1) == -1 and lib.gode_gif_lzw_bound(0) >= 3
    assert not out.any()


def test_palettes():
    assert V.GRAY_PALETTE.shape == (256, 3) and V.GRAY_PALETTE.dtype == np.uint8
    assert np.array_equal(V.GRAY_PALETTE, np.stack([np.arange(256)] * 3, axis=1))
    pal = V.RGB676_PALETTE
    assert pal.shape == (256, 3) and pal.dtype == np.uint8 and not pal[252:].any()
    levels = [[(k * 255 + (n - 1) // 2) // (n - 1) for k in range(n)] for n in (6, 7, 6)]
    assert levels[0] == [0, 51, 102, 153, 204, 255] and levels[1] == [0, 43, 85, 128, 170, 213, 255]
    for r in range(6):
        for g in range(7):
            for b in range(6):
                assert tuple(pal[(r * 7 + g) * 6 + b]) == (levels[0][r], levels[1][g], levels[2][b])
    # every palette colour is its own cell, and the cell of a colour is the nearest level per channel
    assert np.array_equal(V.rgb676_index(pal[:252]), np.arange(252))
    v = np.arange(256)
    for c, lv in enumerate(levels):
        rgb = np.zeros((256, 3), dtype=np.uint8)
        rgb[:, c] = v
        q = V.rgb676_index(rgb).astype(int)
        q = (q // 42, (q // 6) % 7, q % 6)[c]
        assert (np.abs(np.array(lv)[q] - v) == np.abs(np.array(lv)[None, :] - v[:, None]).min(axis=1)).all()


def _check_file(path, frames, palette, delay, loop=0):
    g = read_gif(path)
    assert g.version == b"GIF89a"
    assert (g.width, g.height) == (frames.shape[2], frames.shape[1])
    k = 1 << max(1, (len(palette) - 1).bit_length())
    assert g.palette.shape == (k, 3) and np.array_equal(g.palette[:len(palette)], palette) and not g.palette[len(palette):].any()
    assert g.loop == loop
    assert g.frames.shape == frames.shape and np.array_equal(g.frames, frames)
    assert g.delays == [delay] * len(frames)
    assert g.min_code_sizes == [max(2, (len(palette) - 1).bit_length())] * len(frames)
    assert 0 < g.max_sub_block <= 255
    return g


def _check_with_pil(path, frames, palette):
    """An additional check when PIL is there; the decoder of tests/gif_decode.py is the required one."""
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        assert im.n_frames == len(frames)
        for t in range(len(frames)):
            im.seek(t)
            assert np.array_equal(np.asarray(im.convert("RGB")), palette[frames[t]]), t


def test_write_gif_blocks_and_frames(tmp_path):
    rs = np.random.RandomState(11)
    frames = rs.randint(0, 256, (5, 37, 53)).astype(np.uint8)                 # 1961 indices a frame: several sub-blocks
    path = str(tmp_path / "a.gif")
    assert V.write_gif(path, frames, V.GRAY_PALETTE) == path
    g = _check_file(path, frames, V.GRAY_PALETTE, delay=4)
    assert g.max_sub_block == 255 and g.disposals == [1] * 5
    _check_with_pil(path, frames, V.GRAY_PALETTE)
    # a strided view, a CPU tensor, another rate and repeat count, a short palette (padded with black to 8 entries)
    pal5 = rs.randint(0, 256, (5, 3)).astype(np.uint8)
    small = rs.randint(0, 5, (3, 9, 14)).astype(np.uint8)
    V.write_gif(path, torch.from_numpy(small).transpose(1, 2), pal5, fps=10, loop=3)
    _check_file(path, small.transpose(0, 2, 1), pal5, delay=10, loop=3)
    _check_with_pil(path, small.transpose(0, 2, 1), pal5)
    V.write_gif(path, small[:, ::2, ::3] % 2, pal5[:2], fps=30)                # round(100 / 30) = 3
    _check_file(path, small[:, ::2, ::3] % 2, pal5[:2], delay=3)
    with pytest.raises(ValueError, match="outside the palette"):
        V.write_gif(path, small, pal5[:4])
    with pytest.raises(ValueError, match="uint8 \\[T, H, W\\]"):
        V.write_gif(path, small.astype(np.int32), pal5)
    with pytest.raises(ValueError, match="uint8 \\[T, H, W\\]"):
        V.write_gif(path, small[0], pal5)
    with pytest.raises(ValueError, match="palette"):
        V.write_gif(path, small, pal5.astype(np.float32))
    with pytest.raises(ValueError, match="fps"):
        V.write_gif(path, small, pal5, fps=0)


@pytest.mark.parametrize("C_", [1, 3])
def test_vwrite_on_the_array_gen_samples_builds(tmp_path, C_):
    """mnist_moco_ode.py:37-44 as written (n = 2, size = 6), from random fp32 samples in [-1, 1]."""
    n, size = 2, 6
    s = np.random.RandomState(5 + C_).uniform(-1, 1, (n * n, C_, 16, size, size)).astype(np.float32)
    out = np.zeros((3, 16, size * n, size * n))
    for j in range(n):
        for k in range(n):
            out[:, :, size * j:size * (j + 1), size * k:size * (k + 1)] = s[j * n + k, :, :, :, :]
    out = out.transpose((1, 2, 3, 0))
    out = (out + 1) / 2 * 255
    assert not out.flags.c_contiguous
    path = str(tmp_path / f"gensamples_id{C_}.gif")
    V.vwrite(path, out)
    u8 = np.clip(out, 0, 255).astype(np.uint8)
    if C_ == 1:
        want, pal = u8[..., 0], V.GRAY_PALETTE
    else:
        q = [(u8[..., c].astype(np.int64) * (lv - 1) + 127) // 255 for c, lv in enumerate((6, 7, 6))]
        want, pal = ((q[0] * 7 + q[1]) * 6 + q[2]).astype(np.uint8), V.RGB676_PALETTE
        assert len(np.unique(want)) > 100                                       # the cube is used, not one corner of it
    _check_file(path, want, pal, delay=4)
    _check_with_pil(path, want, pal)


def test_vwrite_takes_what_skvideo_takes(tmp_path):
    rs = np.random.RandomState(2)
    path = str(tmp_path / "v.gif")
    gray = rs.uniform(-40, 300, (3, 5, 7))                                        # values the clip has to catch
    V.vwrite(path, gray)
    _check_file(path, np.clip(gray, 0, 255).astype(np.uint8), V.GRAY_PALETTE, delay=4)
    u8 = rs.randint(0, 256, (2, 4, 4, 3)).astype(np.uint8)
    V.vwrite(path, u8)
    _check_file(path, V.rgb676_index(u8), V.RGB676_PALETTE, delay=4)
    eq = np.repeat(u8[..., :1], 3, axis=3)                                        # three equal channels: written as gray
    V.vwrite(path, eq.astype(np.float32))
    _check_file(path, u8[..., 0], V.GRAY_PALETTE, delay=4)
    with pytest.raises(ValueError, match="GIF"):
        V.vwrite(str(tmp_path / "v.mp4"), u8)
    with pytest.raises(ValueError, match="array expected"):
        V.vwrite(path, u8[0, 0])


def test_the_op_is_declared_once_and_exported():
    assert L.VideoGridOp.KIND == L.OP_VIDEO_GRID == 41 and L.VideoGridOp.FN == "gode_video_grid" in L.EXPORTS
    lib = L.lib()
    assert C.sizeof(L.VideoGridOp) == lib.gode_sizeof(41) == 96
    assert lib.gode_version() == 105
    assert G.video_io is V and "video_io" in G.__all__
    for name in ("video_grid", "write_gif", "vwrite", "gen_samples", "GRAY_PALETTE", "RGB676_PALETTE"):
        assert hasattr(V, name), name


def test_every_refusal_comes_before_any_launch():
    """A null stream and pointers to nothing: every case returns its code without touching the device or `out`."""
    lib = L.lib()
    rgb = np.full(64, 0x5A, dtype=np.uint8)
    idx = np.full(64, 0x5A, dtype=np.uint8)
    src = np.zeros(64, dtype=np.float32)
    good = dict(src=src.ctypes.data, xs=(L.i64 * 5)(48, 16, 16, 4, 1), rgb=rgb.ctypes.data, idx=idx.ctypes.data,
                B=1, C=1, T=1, H=4, W=4, rows=1, cols=1, mode=0)
    kind = L.i32(-7)
    assert lib.gode_video_grid(None, None) == -1
    assert lib.gode_video_grid_launch_kind(None, C.byref(kind)) == -1
    assert lib.gode_video_grid_launch_kind(C.byref(L.VideoGridOp(**good)), None) == -1
    cases = [(dict(src=None), -1), (dict(rgb=None, idx=None), -1), (dict(C=0), -1), (dict(C=2), -1), (dict(C=4), -1),
             (dict(mode=-1), -1), (dict(mode=2), -1), (dict(B=0), -1), (dict(B=-3), -1), (dict(B=2), -1),
             (dict(B=7, rows=2, cols=3), -1),
             (dict(T=0), -2), (dict(H=0), -2), (dict(W=0), -2), (dict(rows=0), -2), (dict(cols=0), -2), (dict(T=-1), -2),
             (dict(rows=4097), -2), (dict(cols=4097), -2), (dict(H=16385), -2), (dict(W=16385), -2),
             (dict(rows=65536, H=65536), -2)]
    for change, code in cases:
        op = L.VideoGridOp(**{**good, **change})
        assert lib.gode_video_grid(C.byref(op), None) == code, change
        assert lib.gode_video_grid_launch_kind(C.byref(op), C.byref(kind)) == code and kind.value == -7, change
        assert lib.gode_run((L.i32 * 1)(41), (L.ptr * 1)(C.addressof(op)), 1, None) == code * 1000, change
    assert (rgb == 0x5A).all() and (idx == 0x5A).all()
    # the branch a valid op would take, still without a launch: four pixels per thread, or one through the strides
    for change, want in ((dict(), 1), (dict(rows=4096, cols=4096), 1), (dict(W=3), 0), (dict(xs=(L.i64 * 5)(48, 16, 16, 4, 2)), 0),
                         (dict(xs=(L.i64 * 5)(48, 16, 16, 6, 1)), 0), (dict(src=src.ctypes.data + 4), 0),
                         (dict(idx=idx.ctypes.data + 1), 0), (dict(rgb=rgb.ctypes.data + 2), 0),
                         (dict(C=3, xs=(L.i64 * 5)(48, 1, 48, 12, 3)), 1), (dict(C=3, xs=(L.i64 * 5)(48, 16, 16, 4, 1)), 0)):
        op = L.VideoGridOp(**{**good, **change})
        assert lib.gode_video_grid_launch_kind(C.byref(op), C.byref(kind)) == 0 and kind.value == want, change


def test_python_wrappers_refuse_before_any_launch():
    ok = torch.zeros(4, 1, 2, 4, 4)
    with pytest.raises(ValueError, match="float32"):
        V.video_grid(ok.double())
    with pytest.raises(ValueError, match="float32"):
        V.video_grid(ok[0])
    with pytest.raises(ValueError, match="channels"):
        V.video_grid(torch.zeros(4, 2, 2, 4, 4))
    with pytest.raises(ValueError, match="mode"):
        V.video_grid(ok, mode="sigmoid")
    with pytest.raises(ValueError, match="neither"):
        V.video_grid(ok, rgb=False)
    with pytest.raises(ValueError, match="do not fit"):
        V.video_grid(ok, n=1)
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        V.video_grid(ok)
    gen = G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8)
    with pytest.raises(ValueError, match="28 x 28"):
        V.gen_samples(gen, n=2, size=64)
    assert gen.training                                                           # refused before eval() was called
    with pytest.raises(ValueError, match="64 x 64"):
        V.gen_samples(G.VideoGenerator(3, 50, 0, 16, 16, dim_hidden=16, ngf=8), n=2, size=28)
