"""CPU: the host side of the device-resident UCF-101 feed -- the bicubic tap tables and their float64
evaluation against torch.nn.functional.interpolate, the two new op kinds of the C ABI, Ucf101OnDevice's index stream (through
its gather hook, on frames appended with add_resized), the dataset drop-ins over a temporary directory with a fake reader,
the refusals, and the cap on the share of near-tie values that tests/test_gpu_ucf.py excludes from its byte comparison."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ucf_ref as R
import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import data as D


# ---------------------------------------------------------------------------------------------------------------------
# tap tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", R.MODES)
@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_tables_evaluate_to_interpolate_in_float64(geom, antialias):
    H, W, oh, ow = geom
    x = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H * W))
    want = F.interpolate(x.permute(0, 3, 1, 2).double(), size=(oh, ow), mode="bicubic", align_corners=False,
                         antialias=antialias).permute(0, 2, 3, 1)
    v, b = D.resize_crop_reference(x, oh, ow, 0, ow, antialias)
    err = float((v - want).abs().max())
    print(geom, antialias, "max |tables - interpolate|", err)
    assert err < 1e-9
    assert torch.equal(b, want.clamp(0, 255).round().to(torch.uint8))
    # the fp32 table rows are the float64 ones rounded once: same ranges, zero behind count
    for n_in, n_out in ((H, oh), (W, ow)):
        first, count, w, k = D.bicubic_taps(n_in, n_out, antialias)
        dense = D._dense_taps64(n_in, n_out, antialias)
        assert first.dtype == count.dtype == torch.int32 and w.dtype == torch.float32 and tuple(w.shape) == (n_out, k)
        assert int(count.max()) == k and int(first.min()) >= 0 and int((first + count).max()) <= n_in
        for i in range(n_out):
            f, c = int(first[i]), int(count[i])
            assert torch.equal(w[i, :c], dense[i, f:f + c].float()) and float(w[i, c:].abs().sum()) == 0.0
            assert float(dense[i, :f].abs().sum()) == 0.0 and float(dense[i, f + c:].abs().sum()) == 0.0


def test_border_taps_that_clamp_to_one_index_are_merged():
    first, count, w, k = D.bicubic_taps(5, 8, False)
    assert k == 4 and first.tolist()[0] == 0 and int(count[0]) < 4 and int(count[-1]) < 4       # merged at both borders
    assert int((first + count)[-1]) == 5
    assert float((w.double().sum(1) - 1).abs().max()) < 1e-6                                   # the merged weights still sum to 1
    # output 0: src = 0.625 * 0.5 - 0.5 = -0.1875 -> ix = -1: taps at -2, -1, 0, 1 clamp to 0, 0, 0, 1
    assert (int(first[0]), int(count[0])) == (0, 2)
    first, count, w, k = D.bicubic_taps(7, 11, True)
    assert float((w.double().sum(1) - 1).abs().max()) < 1e-6 and int(first[0]) == 0 and int((first + count)[-1]) == 7


@pytest.mark.parametrize("antialias", R.MODES)
def test_crop_folded_into_the_table_is_resize_then_slice(antialias):
    x = torch.randint(0, 256, (1, 30, 40, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    full, fb = D.resize_crop_reference(x, 16, 21, 0, 21, antialias)
    part, pb = D.resize_crop_reference(x, 16, 21, 3, 16, antialias)
    assert torch.equal(part, full[:, :, 3:19]) and torch.equal(pb, fb[:, :, 3:19])
    f0, c0, w0, _ = D.bicubic_taps(40, 21, antialias)
    f1, c1, w1, k1 = D.bicubic_taps(40, 21, antialias, 3, 16)
    assert torch.equal(f1, f0[3:19]) and torch.equal(c1, c0[3:19]) and torch.equal(w1, w0[3:19, :k1])


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_two_ops():
    lib = L.lib()
    assert lib.gode_version() == 105
    assert (L.OP_RESIZE_U8, L.OP_CLIP_GATHER) == (37, 38)
    assert L.ResizeU8Op.KIND == 37 and L.ResizeU8Op.FN == "gode_resize_u8"
    assert L.ClipGatherOp.KIND == 38 and L.ClipGatherOp.FN == "gode_clip_gather"
    assert lib.gode_sizeof(37) == C.sizeof(L.ResizeU8Op) == 136
    assert lib.gode_sizeof(38) == C.sizeof(L.ClipGatherOp) == 56


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    one = C.c_void_p(16)            # never dereferenced: every case below is refused on the host
    def resize(**kw):
        a = dict(src=one, dst=one, dst_f32=None, y_first=one, y_count=one, y_w=one, x_first=one, x_count=one, x_w=one, F=1, Hin=8,
                 Win=8, C=3, out_h=4, out_w=4, ky=4, kx=4)
        a.update(kw)
        return lib.gode_resize_u8(C.byref(L.ResizeU8Op(**a)), None)
    assert resize(dst=None) == -1 and resize(C=2) == -1 and resize(ky=0) == -1 and resize(src=None) == -1 and resize(F=0) == -1
    assert resize(ky=L.RESIZE_MAX_TAPS + 1) == -2 and resize(kx=L.RESIZE_MAX_TAPS + 1) == -2
    assert resize(out_w=2000, ky=8) == -2               # 8 rows of 6,000 fp32 partial sums do not fit the kernel's LDS
    def gather(**kw):
        a = dict(frames=one, first=one, out=one, n_frames=4, frame_elems=16, B=1, T=1, sub=128.0, inv=1 / 128)
        a.update(kw)
        return lib.gode_clip_gather(C.byref(L.ClipGatherOp(**a)), None)
    assert gather(first=None) == -1 and gather(T=0) == -1 and gather(B=0) == -1 and gather(n_frames=0) == -1
    assert gather(frame_elems=1 << 30, T=2) == -2 and gather(frame_elems=1 << 20, T=16, B=1 << 12) == -2


# ---------------------------------------------------------------------------------------------------------------------
# index stream
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = [40, 16, 17, 18, 33, 120, 16, 25, 19]          # 16, 17: L <= n_frame + 1 -> start 0; 18: span 1 -> start 0


def _index_set(seed=3, lengths=LENGTHS, short=(5, 15)):
    """A host set whose stored frames carry their own global index in byte 0 and their video in byte 1, and whose gather
    hook records the indices it is asked for."""
    asked = []
    def gather(first, T):
        asked.append((first.clone(), T))
        return first[:, None, None, None, None].float().expand(-1, T, 2, 2, 1) + torch.arange(T).float()[None, :, None, None, None]
    ds = D.Ucf101OnDevice(device="cpu", n_frame=16, image_size=2, resized_width=2, crop_left=0, seed=seed, gather=gather)
    kept = []
    for i, n in enumerate(list(lengths[:4]) + list(short) + list(lengths[4:])):
        ok = ds.add_resized(torch.zeros(n, 2, 2, 1, dtype=torch.uint8), label=100 + i)
        assert ok == (n >= 16)
        if ok:
            kept.append((n, 100 + i))
    return ds, asked, kept


def _video_of(ds, first):
    off, length, _ = ds._tabs()
    v = int(torch.searchsorted(off, torch.tensor(first), right=True)) - 1
    return v, first - int(off[v]), int(length[v])


def test_index_stream_epochs_ranges_labels_and_views():
    ds, asked, kept = _index_set()
    assert len(ds) == len(LENGTHS) and ds.n_frames == sum(LENGTHS)          # the short videos were not stored
    assert ds._tabs()[1].tolist() == [n for n, _ in kept] and ds._tabs()[2].tolist() == [c for _, c in kept]
    B, per_epoch = 4, len(LENGTHS) // 4
    stream = ds.videos(B, labels=True)
    zero_start = set()
    for epoch in range(60):
        seen = []
        for _ in range(per_epoch):
            v, lab = next(stream)
            first, T = asked[-1]
            assert T == 16 and first.dtype == torch.int64 and tuple(first.shape) == (B,)
            assert tuple(v.shape) == (B, 16, 1, 2, 2) and v.permute(0, 1, 3, 4, 2).is_contiguous()
            for f, c in zip(first.tolist(), lab.tolist()):
                vid, start, n = _video_of(ds, f)
                assert c == kept[vid][1]                                     # labels aligned with the drawn videos
                assert 0 <= start < max(n - 16 - 1, 1), (start, n)           # np.random.randint(0, L - n_frame - 1)'s range
                if n <= 18:
                    assert start == 0
                    zero_start.add(n)
                seen.append(vid)
        assert len(set(seen)) == len(seen) == per_epoch * B                  # one permutation per epoch, the tail dropped
    assert zero_start == {16, 17, 18}
    # every legal start of a video is reached, none beyond: L = 19 -> {0, 1}, L = 25 -> {0..7}; L = 120 has 103 starts and is
    # drawn ~53 times here (~41 distinct values expected)
    starts = {}
    for first, _ in asked:
        for f in first.tolist():
            vid, start, n = _video_of(ds, f)
            starts.setdefault(n, set()).add(start)
    assert starts[19] == {0, 1} and starts[25] == set(range(8)) and max(starts[120]) <= 102 and len(starts[120]) > 20


def test_image_stream_draws_every_frame_of_a_video():
    ds, asked, kept = _index_set(seed=4, lengths=[16, 17, 20], short=())
    stream = ds.images(3, labels=True)
    frames = {16: set(), 17: set(), 20: set()}
    for _ in range(200):
        x, lab = next(stream)
        first, T = asked[-1]
        assert T == 1 and tuple(x.shape) == (3, 1, 2, 2) and x.permute(0, 2, 3, 1).is_contiguous()
        assert sorted(lab.tolist()) == [100, 101, 102]                       # batch == kept videos: each epoch holds all
        for f, c in zip(first.tolist(), lab.tolist()):
            vid, k, n = _video_of(ds, f)
            assert c == kept[vid][1] and 0 <= k < n
            frames[n].add(k)
    assert all(frames[n] == set(range(n)) for n in frames)                   # uniform on [0, L), the last frame included
    assert next(ds.images(3)).shape == (3, 1, 2, 2)                          # labels=False: the batch alone


def test_streams_are_seeded_and_leave_the_global_generators_alone():
    torch.manual_seed(11)
    np.random.seed(11)
    t0, n0 = torch.get_rng_state(), np.random.get_state()
    runs = []
    for _ in range(2):
        ds, asked, _ = _index_set(seed=9)
        vs, im = ds.videos(4), ds.images(2)
        for _ in range(5):
            next(vs), next(im)
        runs.append(torch.cat([a for a, _ in asked]))
    assert torch.equal(runs[0], runs[1])
    ds, asked, _ = _index_set(seed=10)
    vs, im = ds.videos(4), ds.images(2)
    for _ in range(5):
        next(vs), next(im)
    assert not torch.equal(torch.cat([a for a, _ in asked]), runs[0])
    assert torch.equal(torch.get_rng_state(), t0)
    n1 = np.random.get_state()
    assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:]


def test_save_and_load_round_trip_on_the_host(tmp_path):
    ds, _, _ = _index_set()
    ds._store[:ds.n_frames].copy_(torch.randint(0, 256, ds.frames.shape, dtype=torch.uint8))
    path = str(tmp_path / "ucf.pt")
    ds.save(path)
    rec = []
    back = D.Ucf101OnDevice.load(path, device="cpu", seed=3, gather=lambda f, T: rec.append(f) or torch.zeros(len(f), T, 2, 2, 1),
                                 n_frame=16, image_size=2)
    assert torch.equal(back.frames, ds.frames) and all(torch.equal(a, b) for a, b in zip(back._tabs(), ds._tabs()))
    assert all(getattr(back, k) == getattr(ds, k) for k in D.Ucf101OnDevice.GEOMETRY)
    with pytest.raises(ValueError, match="n_frame=16"):
        D.Ucf101OnDevice.load(path, device="cpu", gather=lambda f, T: None, n_frame=8)
    with pytest.raises(ValueError, match="crop_left=0"):
        D.Ucf101OnDevice.load(path, device="cpu", gather=lambda f, T: None, crop_left=1)


# ---------------------------------------------------------------------------------------------------------------------
# drop-ins
# ---------------------------------------------------------------------------------------------------------------------
def _fake_ucf(tmp_path):
    """root/annotations with three classes (one unlisted in classInd.txt) and four listed videos; the reader fabricates a
    video from its path: frames x 24 x 32 x 3, every byte of frame k equal to k + 10 * (video number)."""
    ann = tmp_path / "annotations"
    ann.mkdir()
    (ann / "classInd.txt").write_text("1 ApplyEyeMakeup\n2 Archery\n")
    (ann / "trainlist01.txt").write_text("ApplyEyeMakeup/v_1.avi 1\nArchery/v_2.avi 2\nUnknown/v_3.avi 3\nArchery/v_4.avi 2\n")
    (ann / "testlist01.txt").write_text("Archery/v_2.avi\n")
    lengths = {"v_1.avi": 20, "v_2.avi": 16, "v_3.avi": 30, "v_4.avi": 9}
    calls = []
    def reader(path):
        calls.append(path)
        name = os.path.basename(path)
        n, no = lengths[name], int(name[2])
        return (torch.arange(n, dtype=torch.uint8) + 10 * no)[:, None, None, None].expand(n, 24, 32, 3).contiguous()
    return str(tmp_path), reader, calls


def test_drop_ins_over_a_directory_with_a_fake_reader(tmp_path):
    import dataset
    assert dataset.UCF101Video is D.UCF101Video and dataset.UCF101Image is D.UCF101Image
    root, reader, calls = _fake_ucf(tmp_path)
    vd = dataset.UCF101Video(root, "videos_classified", "annotations", reader=reader)
    assert vd.classes == ["ApplyEyeMakeup", "Archery"] and vd.class_to_idx == {"ApplyEyeMakeup": 1, "Archery": 2}
    want = [(os.path.join(root, "videos_classified", "ApplyEyeMakeup/v_1.avi"), 20, 1),
            (os.path.join(root, "videos_classified", "Archery/v_2.avi"), 16, 2)]
    assert vd.samples == want and len(vd) == 2           # the unknown class and the 9-frame video are left out
    im = dataset.UCF101Image(root, "videos_classified", "annotations", samples=vd.samples, reader=reader)
    assert im.samples is vd.samples and len(im) == 2
    own = dataset.UCF101Image(root, "videos_classified", "annotations", reader=reader)
    assert [s[1] for s in own.samples] == [20, 16, 9]    # the image set's own list keeps short videos, as the reference
    assert len(dataset.UCF101Video(root, "videos_classified", "annotations", train=False, reader=reader)) == 1
    # items: constant frames stay constant under a resize whose weights sum to 1
    np.random.seed(0)
    v, c = vd[0]
    np.random.seed(0)
    start = np.random.randint(0, 20 - 16 - 1)
    assert c == 1 and v.dtype == torch.float32 and tuple(v.shape) == (16, 3, 64, 64)
    want = ((torch.arange(16) + start + 10).float() - 128.0) / 128.0
    assert torch.equal(v, want[:, None, None, None].expand(16, 3, 64, 64))
    v, c = vd[1]                                          # L = 16 <= n_frame + 1: start 0, no draw
    assert c == 2 and torch.equal(v[:, 0, 0, 0], ((torch.arange(16) + 20).float() - 128.0) / 128.0)
    np.random.seed(1)
    x, c = im[0]
    np.random.seed(1)
    k = np.random.randint(0, 20)
    assert c == 1 and tuple(x.shape) == (3, 64, 64) and torch.equal(x, torch.full((3, 64, 64), (k + 10 - 128.0) / 128.0))
    # resize_crop is the one definition
    g = torch.Generator().manual_seed(2)
    raw = torch.randint(0, 256, (2, 3, 24, 32), dtype=torch.uint8, generator=g)
    want = D.resize_crop_reference(raw.permute(0, 2, 3, 1), 64, 85, 10, 64, False)[1].permute(0, 3, 1, 2)
    assert torch.equal(vd.resize_crop(raw), want) and torch.equal(im.resize_crop(raw[0]), want[0])
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        vd.to_device(device="cpu")


def test_default_reader_names_the_missing_package(tmp_path):
    root, _, _ = _fake_ucf(tmp_path)
    try:
        import torchvision  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="torchvision"):
            D.UCF101Video(root, "videos_classified", "annotations")
        with pytest.raises(ImportError, match="torchvision"):
            D.UCF101Image(root, "videos_classified", "annotations", samples=[])
    else:
        assert callable(D._torchvision_reader())


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_say_why():
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D.Ucf101OnDevice(device="cpu")
    with pytest.raises(ValueError, match="leaves the resized width 85"):
        D.Ucf101OnDevice(device="cpu", gather=lambda f, T: None, crop_left=22)
    with pytest.raises(ValueError, match="leaves the resized width"):
        D.resize_crop_reference(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 4, 4, 2, 3, False)
    ds = D.Ucf101OnDevice(device="cpu", gather=lambda f, T: None)
    with pytest.raises(ValueError, match="uint8 frames expected"):
        ds.add_video(torch.zeros(16, 8, 8, 3))
    with pytest.raises(ValueError, match="uint8 frames expected"):
        D.resize_crop_reference(torch.zeros(1, 4, 4, 3), 4, 4, 0, 4, False)
    with pytest.raises(ValueError, match="2 channels"):
        ds.add_video(torch.zeros(16, 8, 8, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="4 channels"):
        ds.add_video(torch.zeros(16, 4, 8, 8, dtype=torch.uint8), channels_first=True)
    assert ds.add_video(torch.zeros(15, 8, 8, 3, dtype=torch.uint8)) is False and len(ds) == 0      # too short: not an error
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        ds.add_video(torch.zeros(16, 8, 8, 3, dtype=torch.uint8))                                   # the resize is a GPU op
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D.clip_gather(torch.zeros(4, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), 1)
    assert ds.add_resized(torch.zeros(16, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1-channel|1 channels"):
        ds.add_resized(torch.zeros(16, 64, 64, 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="batch 2 with 1 kept videos"):
        ds.videos(2)
    with pytest.raises(ValueError, match="batch 2 with 1 kept videos"):
        ds.images(2)
    # 9x antialiased downscale: 37 taps, beyond the kernel's 32
    with pytest.raises(ValueError, match="exceed the kernel's maximum of 32"):
        D.ResizeTables(576, 64, 64, 64, 0, 64, True, "cpu")
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        D.ResizeTables(64, 64, 64, 64, 0, 64, False, "cpu")
    f, c, _, k = D.bicubic_taps(8, 4, False)
    with pytest.raises(ValueError, match="leaves the input of 7"):
        D._check_taps(f, c, k, 7, "x")
    assert G.data is D


# ---------------------------------------------------------------------------------------------------------------------
# the tie-window cap of the GPU byte comparison
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", R.MODES)
@pytest.mark.parametrize("name", list(R.CELLS))
def test_share_of_near_tie_values_is_capped(name, antialias):
    v, _, tol, ky, kx = R.cell_oracle(name, antialias)
    share = float(R.near_tie(v, tol).double().mean())
    print(name, antialias, "ky kx", ky, kx, "tol", tol, "near-tie share", share)
    assert share <= R.MAX_TIE_SHARE
    if name == "a_workload" and antialias:
        assert (ky, kx) == (15, 16) and abs(tol - 7.5e-4) < 1e-4      # the workload: 15 / 16 taps, ~7.5e-4
