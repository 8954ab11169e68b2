"""GPU: gode_video_grid and gan_ode_amd.video_io.gen_samples, exactly (torch.equal) against a NumPy float64 restatement of the
drivers' genSamples (mnist_moco_ode.py:37-44: zero-initialised float64 grid, tile (b // n, b % n), (x + 1) / 2 * 255) followed
by the writer's clip(0, 255).astype(uint8) and the palette formula of include/gode.h.

Launch branches of csrc/vidgrid.hip, each reached by a case below and asserted through gode_video_grid_launch_kind:
  vec4<1>   four pixels per thread, one channel: W % 4 == 0, unit stride along w, aligned source and outputs
            (`mnist_channels_last`: sample_videos' permuted view, 28 x 28, several workgroups; `gray_contiguous`)
  vec4<3>   four pixels per thread, channels-last colour (`colour_channels_last`, 8 x 8; `rows_ne_cols_vec` with empty tiles)
  strided   one pixel per thread through all five strides: W % 4 != 0 (`colour_5x6`, B = 3 in a 2 x 2 grid: one empty tile),
            a contiguous [B, C, T, H, W] colour tensor (`colour_contiguous`), outputs that are not 4-byte aligned (`unaligned_out`),
            a source that is not 16-byte aligned (`unaligned_src`), rows != cols (`rows_ne_cols_strided`)
  frame walk  more frames than the grid's y extent holds (T > 65535), both kernels (`long_vec`, `long_strided`)
Every case runs in both modes and with rgb alone, idx alone and both; the outputs lie between guard bytes that must stay
untouched.  The inputs hold, for every k in 1..255, the fp32 value nearest 2k/255 - 1 (mode 1: k/255) -- where the float64 map
crosses an integer, so where a rounding that differs from NumPy's shows -- and its two neighbours, +-1 and their outward
neighbours (clipped), +-0.0, and random values beyond both ends of the range."""
import ctypes as C

import numpy as np
import pytest
import torch

import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import video_io as V
from gan_ode_amd.engine import stream_ptr

from conftest import seed_all
from gif_decode import read_gif

pytestmark = pytest.mark.gpu

CUBE = (6, 7, 6)


def critical_values():
    out = []
    for k in range(1, 256):
        for c in (np.float32(2 * k / 255 - 1), np.float32(k / 255)):
            out += [c, np.nextafter(c, np.float32(-2)), np.nextafter(c, np.float32(2))]
    one = np.float32(1)
    out += [one, -one, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), np.float32(0.0), np.float32(-0.0),
            np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(0), np.float32(1))]
    return np.array(out, dtype=np.float32)


def fill(shape, seed):
    """fp32 values of `shape` in storage order: uniform random in [-1.1, 1.1] (clipped at both ends in mode 0, below in mode 1)
    with the critical values at random places -- all of them where the case has room (every kernel has such a case), else a
    random pick."""
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    a = rs.uniform(-1.1, 1.1, n).astype(np.float32)
    crit = critical_values()
    if n < len(crit):                                  # the long, narrow cases: a random pick of them
        crit = crit[rs.permutation(len(crit))[:n // 2]]
    pos = rs.permutation(n)[:len(crit)]
    a[pos] = crit
    return a.reshape(shape)


def reference(x, rows, cols, mode):
    """x: float32 ndarray [B, C, T, H, W] (any strides) -> (rgb uint8 [T, rows*H, cols*W, 3], idx uint8 [T, rows*H, cols*W])"""
    B, Cn, T, H, W = x.shape
    out = np.zeros((3, T, H * rows, W * cols))                     # float64, as genSamples'
    for b in range(B):
        j, k = divmod(b, cols)
        out[:, :, H * j:H * (j + 1), W * k:W * (k + 1)] = x[b]     # one channel broadcasts to three
    out = out.transpose((1, 2, 3, 0))
    out = (out + 1) / 2 * 255 if mode == 0 else out * 255
    rgb = np.clip(out, 0, 255).astype(np.uint8)
    if Cn == 1:
        idx = rgb[..., 0].copy()
    else:
        q = [(rgb[..., c].astype(np.int64) * (CUBE[c] - 1) + 127) // 255 for c in range(3)]
        idx = ((q[0] * CUBE[1] + q[1]) * CUBE[2] + q[2]).astype(np.uint8)
    return np.ascontiguousarray(rgb), idx


def run_op(view, rows, cols, mode, want_rgb, want_idx, guard=64):
    """The raw op on `view`, outputs inside guarded buffers -> (rgb or None, idx or None, launch kind)."""
    B, Cn, T, H, W = view.shape
    n_pix = T * rows * H * cols * W
    bufs, ptrs = {}, {}
    for name, size, want in (("rgb", 3 * n_pix, want_rgb), ("idx", n_pix, want_idx)):
        if want:
            bufs[name] = torch.full((size + 2 * guard,), 0xA5, dtype=torch.uint8, device=view.device)
            ptrs[name] = bufs[name].data_ptr() + guard
    op = L.VideoGridOp(src=view.data_ptr(), xs=(L.i64 * 5)(*view.stride()), rgb=ptrs.get("rgb"), idx=ptrs.get("idx"),
                       B=B, C=Cn, T=T, H=H, W=W, rows=rows, cols=cols, mode=mode)
    kind = L.i32(-1)
    assert L.lib().gode_video_grid_launch_kind(C.byref(op), C.byref(kind)) == 0
    L.run_one(op, stream_ptr())
    torch.cuda.synchronize()
    res = []
    for name, last in (("rgb", (3,)), ("idx", ())):
        if name not in bufs:
            res.append(None)
            continue
        b = bufs[name]
        assert bool((b[:guard] == 0xA5).all()) and bool((b[-guard:] == 0xA5).all()), f"{name}: guard bytes written"
        res.append(b[guard:-guard].view((T, rows * H, cols * W) + last))
    return res[0], res[1], kind.value


def _channels_last(a):
    """[B, T, H, W, C] storage, seen as sample_videos returns it: [B, C, T, H, W]"""
    return a.permute(0, 4, 1, 2, 3)


def _cases():
    # name -> (storage shape, storage -> [B, C, T, H, W] view, rows, cols, guard, the kernel expected (1 vec4, 0 strided))
    return {
        "mnist_channels_last": ((4, 16, 28, 28, 1), _channels_last, 2, 2, 64, 1),
        "colour_channels_last": ((4, 3, 8, 8, 3), _channels_last, 2, 2, 64, 1),
        "colour_5x6": ((3, 4, 5, 6, 3), _channels_last, 2, 2, 64, 0),
        "gray_contiguous": ((4, 1, 3, 8, 12), lambda a: a, 2, 2, 64, 1),
        "colour_contiguous": ((4, 3, 3, 8, 8), lambda a: a, 2, 2, 64, 0),
        "unaligned_out": ((4, 3, 8, 8, 3), _channels_last, 2, 2, 3, 0),
        "unaligned_src": ((1 + 4 * 3 * 8 * 8 * 3,), lambda a: _channels_last(a[1:].view(4, 3, 8, 8, 3)), 2, 2, 64, 0),
        "rows_ne_cols_vec": ((5, 2, 4, 8, 3), _channels_last, 3, 2, 64, 1),
        "rows_ne_cols_strided": ((3, 2, 3, 5, 1), _channels_last, 1, 3, 64, 0),
        "long_vec": ((1, 65540, 1, 4, 1), _channels_last, 1, 1, 64, 1),
        "long_strided": ((1, 65540, 1, 1, 3), _channels_last, 1, 1, 64, 0),
    }


@pytest.fixture(scope="module")
def case_data():
    """Per case: the device view and, per mode, the NumPy reference -- computed once, shared by the output variants."""
    data = {}
    for i, (name, (shape, to_view, rows, cols, guard, kind)) in enumerate(_cases().items()):
        host = torch.from_numpy(fill(shape, 100 + i))
        view = to_view(host.cuda())
        ref = {mode: reference(to_view(host).numpy(), rows, cols, mode) for mode in (0, 1)}
        data[name] = (view, ref)
    return data


@pytest.mark.parametrize("outputs", ["rgb", "idx", "both"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(_cases()))
def test_video_grid_equals_the_numpy_restatement(case_data, name, mode, outputs):
    _, _, rows, cols, guard, want_kind = _cases()[name]
    view, ref = case_data[name]
    rgb, idx, kind = run_op(view, rows, cols, mode, outputs != "idx", outputs != "rgb", guard)
    assert kind == want_kind
    want_rgb, want_idx = ref[mode]
    if rgb is not None:
        assert torch.equal(rgb.cpu(), torch.from_numpy(want_rgb))
    if idx is not None:
        assert torch.equal(idx.cpu(), torch.from_numpy(want_idx))


def test_the_critical_values_are_where_the_map_crosses_an_integer():
    """The inputs do what the module docstring says of them: around every k the three neighbours give two different bytes in
    float64 (so a map evaluated in fp32, or with another rounding, is told apart), and the outward neighbours of +-1 clip."""
    c = critical_values().astype(np.float64)
    v = np.clip((c + 1) / 2 * 255, 0, 255).astype(np.uint8)
    trip = v[:255 * 6].reshape(255, 2, 3)[:, 0]
    assert (trip.max(axis=1) - trip.min(axis=1) == 1).all()
    f32 = np.clip((critical_values() + np.float32(1)) / np.float32(2) * np.float32(255), 0, 255).astype(np.uint8)
    assert (f32 != v).any()                                       # an fp32 evaluation of the map fails on these inputs
    tail = (critical_values()[255 * 6:].astype(np.float64) + 1) / 2 * 255
    assert tail[2] > 255 and tail[3] < 0


def test_video_grid_wrapper(case_data):
    """The Python entry point on the two sampling layouts: n defaults to ceil(sqrt(B)), both outputs, both mode names."""
    for name, B in (("mnist_channels_last", 4), ("colour_5x6", 3)):
        view, ref = case_data[name]
        rgb, idx = V.video_grid(view, rgb=True, idx=True)
        assert rgb.is_cuda and rgb.dtype == torch.uint8 and idx.dtype == torch.uint8
        assert torch.equal(rgb.cpu(), torch.from_numpy(ref[0][0])) and torch.equal(idx.cpu(), torch.from_numpy(ref[0][1]))
        assert torch.equal(V.video_grid(view, n=2, mode="unit").cpu(), torch.from_numpy(ref[1][0]))
        assert torch.equal(V.video_grid(view, mode="unit", rgb=False, idx=True).cpu(), torch.from_numpy(ref[1][1]))
    one = case_data["mnist_channels_last"][0][:1]                                 # B = 1 -> a 1 x 1 grid
    assert tuple(V.video_grid(one).shape) == (16, 28, 28, 3)
    five = case_data["rows_ne_cols_vec"][0]                                       # B = 5 -> 3 x 3, four empty tiles
    want = reference(five.cpu().numpy(), 3, 3, 0)[0]
    assert torch.equal(V.video_grid(five).cpu(), torch.from_numpy(want))


GENERATORS = {
    "mnist_ode": lambda: G.VideoGeneratorMNISTODE(1, 50, 0, 16, 16, ngf=8),
    "ucf_ode": lambda: G.VideoGenerator(3, 50, 0, 16, 16, dim_hidden=16, ngf=8),
    "gru": lambda: G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=8),
    "ode_rnn": lambda: G.VideoGeneratorMNISTODERNN(1, 50, 0, 16, 16, ngf=8),
    "sde": lambda: G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=8),
    "cde": lambda: G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8),
    "mnist_tanh": lambda: G.VideoGeneratorMNISTTanh(1, 50, 0, 16, 16, ngf=8),
    "categorical": lambda: G.VideoGeneratorMNISTODE(1, 50, 3, 16, 16, ngf=8),
}


WARM_PASSES = 30


def _bn_state(gen):
    return {k: v.detach().clone() for k, v in gen.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


@pytest.mark.parametrize("tag", list(GENERATORS))
def test_gen_samples_writes_what_gen_samples_of_the_reference_computes(tmp_path, tag):
    n = 2
    seed_all(3)
    gen = GENERATORS[tag]().cuda()
    with torch.no_grad():                                         # training-mode passes: the running statistics leave their defaults
        for _ in range(WARM_PASSES):                              # and come close to the batch statistics (momentum 0.1), so that
            gen.sample_videos(4)                                  # eval mode gives pictures, not a flat gray
    torch.cuda.synchronize()
    bn = _bn_state(gen)
    assert bn and any(int(v) == WARM_PASSES for k, v in bn.items() if k.endswith("num_batches_tracked"))
    # the reference's route at the same seeds
    seed_all(17)
    gen.eval()
    with torch.no_grad():
        s = gen.sample_videos(n * n)[0].cpu().detach().numpy()
    gen.train()
    np_state, torch_state = np.random.get_state(), torch.get_rng_state()
    Cn, T, size = s.shape[1], s.shape[2], s.shape[3]
    assert size == (28 if gen.mnist else 64) and T == 16
    want = reference(s, n, n, 0)[1]
    # the fast path
    seed_all(17)
    gen.eval()                                                    # train() afterwards is unconditional, as the reference's
    path = V.gen_samples(gen, n=n, e=7, size=size, video_sample_path=str(tmp_path))
    assert path == f"{tmp_path}/gensamples_id7.gif"
    assert gen.training is True and all(m.training for m in gen.modules())
    after = _bn_state(gen)
    assert after.keys() == bn.keys() and all(torch.equal(after[k], bn[k]) for k in bn)
    st = np.random.get_state()
    assert st[0] == np_state[0] and np.array_equal(st[1], np_state[1]) and st[2:] == np_state[2:]
    assert torch.equal(torch.get_rng_state(), torch_state)
    g = read_gif(path)
    assert (g.width, g.height, g.loop) == (n * size, n * size, 0) and g.delays == [4] * T
    assert np.array_equal(g.palette, V.GRAY_PALETTE if Cn == 1 else V.RGB676_PALETTE)
    assert g.frames.shape == want.shape and np.array_equal(g.frames, want)
    assert len(np.unique(want)) > 4                               # a picture, not the flat gray of an untrained eval pass
