"""GPU: the device-resident UCF-101 feed -- gode_resize_u8 on every cell of tests/ucf_ref.py against the
float64 oracle within the derived rounding bound, gode_clip_gather bitwise against the reference's (x - 128.0) / 128.0 on both
of its paths, Ucf101OnDevice (store, save / load, batch streams against a host twin of the same seed) and one GanTrainer
iteration fed from it, bitwise against the same iteration fed with clones of oracle-built batches."""
import pytest
import torch

from conftest import seed_all

import ucf_ref as R
import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import data as D

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
def _run_cell(name, antialias):
    H, W, oh, ow, left, cw, F, C, chw = R.CELLS[name]
    x = R.cell_input(name).cuda()
    tables = D.ResizeTables(H, W, oh, ow, left, cw, antialias, "cuda")
    return D.resize_u8(x.permute(0, 2, 3, 1) if chw else x, tables, want_f32=True)


@pytest.mark.parametrize("antialias", R.MODES)
@pytest.mark.parametrize("name", list(R.CELLS))
def test_resize_cell_against_the_float64_oracle(name, antialias):
    v, want, tol, ky, kx = R.cell_oracle(name, antialias)
    got_b, got_v = _run_cell(name, antialias)
    assert got_v.dtype == torch.float32 and got_b.dtype == torch.uint8 and tuple(got_v.shape) == tuple(got_b.shape) == tuple(v.shape)
    err = float((got_v.cpu().double() - v).abs().max())
    print(name, "antialias", antialias, "ky kx", ky, kx, "max |dst_f32 - oracle|", err, "bound", tol)
    assert err <= tol
    share = R.check_bytes(got_b, v, want, tol)
    print(name, "near-tie share", share)
    assert share <= R.MAX_TIE_SHARE
    if name == "d_identity":
        H, W, oh, ow, left, cw, F, C, chw = R.CELLS[name]
        assert torch.equal(got_b.cpu(), R.cell_input(name)[:, :, left:left + cw])         # exactly the kept columns


def test_resize_outputs_are_independent_and_bad_table_rows_poison_only_their_outputs():
    name = "b_ragged"
    H, W, oh, ow, left, cw, F, C, chw = R.CELLS[name]
    x = R.cell_input(name).cuda()
    tables = D.ResizeTables(H, W, oh, ow, left, cw, False, "cuda")
    both_b, both_v = D.resize_u8(x, tables, want_f32=True)
    only_b = D.resize_u8(x, tables)
    assert torch.equal(only_b, both_b)
    only_v = torch.empty_like(both_v)
    op = L.ResizeU8Op(src=x.data_ptr(), dst=None, dst_f32=only_v.data_ptr(), y_first=tables.y_first.data_ptr(),
                      y_count=tables.y_count.data_ptr(), y_w=tables.y_w.data_ptr(), x_first=tables.x_first.data_ptr(),
                      x_count=tables.x_count.data_ptr(), x_w=tables.x_w.data_ptr(), ss=(L.i64 * 4)(*x.stride()), F=F, Hin=H, Win=W,
                      C=C, out_h=oh, out_w=cw, ky=tables.ky, kx=tables.kx)
    L.run_one(op, G.engine.stream_ptr())
    assert torch.equal(only_v, both_v)
    # a row range that leaves the input (row 3) and a column count beyond kx (column 2): NaN / 0 there, the rest untouched
    bad = D.ResizeTables(H, W, oh, ow, left, cw, False, "cuda")
    bad.y_first[3] = H - 1
    bad.x_count[2] = tables.kx + 1
    b, v = D.resize_u8(x, bad, want_f32=True)
    hit = torch.zeros(oh, cw, dtype=torch.bool, device="cuda")
    hit[3, :] = True
    hit[:, 2] = True
    assert bool(torch.isnan(v[:, hit]).all()) and int(b[:, hit].max()) == 0
    assert torch.equal(v[:, ~hit], both_v[:, ~hit]) and torch.equal(b[:, ~hit], both_b[:, ~hit])


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
def _store(n, shape, offset=0):
    g = torch.Generator().manual_seed(n)
    elems = n * shape[0] * shape[1] * shape[2]
    raw = torch.randint(0, 256, (elems + offset,), dtype=torch.uint8, generator=g).cuda()
    return raw[offset:].view(n, *shape)


@pytest.mark.parametrize("T", [16, 1])
@pytest.mark.parametrize("kind", ["vector", "scalar"])
def test_gather_is_bitwise_the_reference_normalisation(kind, T):
    frames = _store(40, (64, 64, 3)) if kind == "vector" else _store(40, (5, 5, 3), offset=1)
    assert (frames.data_ptr() % 16 == 0) == (kind == "vector") and frames[0].numel() == (12288 if kind == "vector" else 75)
    first = torch.tensor([0, 24 if T == 16 else 39, 7, 3, 7], dtype=torch.int64)
    got = D.clip_gather(frames, first.cuda(), T)
    idx = first[:, None] + torch.arange(T)[None, :]
    want = (frames.cpu()[idx].float() - 128.0) / 128.0
    assert tuple(got.shape) == (5, T) + tuple(frames.shape[1:]) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("kind", ["vector", "scalar"])
def test_gather_fills_a_clip_that_leaves_the_store_with_nan(kind):
    frames = _store(20, (64, 64, 3)) if kind == "vector" else _store(20, (5, 5, 3), offset=1)
    T = 4
    first = torch.tensor([0, 17, 16, -1, 5, 1 << 40], dtype=torch.int64)       # 17 + 4 > 20, -1 < 0, far outside
    got = D.clip_gather(frames, first.cuda(), T).cpu()
    for b, f in enumerate(first.tolist()):
        if 0 <= f <= 20 - T:
            assert torch.equal(got[b], (frames.cpu()[f:f + T].float() - 128.0) / 128.0), b
        else:
            assert bool(torch.isnan(got[b]).all()), b


def _videos(sizes, seed=0, C=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (n, h, w, C), dtype=torch.uint8, generator=g) for n, h, w in sizes]


def test_batch_views_have_the_documented_strides_over_one_channels_last_buffer():
    ds = D.Ucf101OnDevice.from_videos(_videos([(20, 64, 85), (17, 64, 85), (30, 64, 85)]), seed=1)
    v = next(ds.videos(2))
    S = 64
    assert tuple(v.shape) == (2, 16, 3, S, S) and v.stride() == (16 * S * S * 3, S * S * 3, 1, S * 3, 3)
    assert v.permute(0, 1, 3, 4, 2).is_contiguous() and v.storage_offset() == 0
    assert v.untyped_storage().nbytes() == v.numel() * 4                       # one buffer, nothing behind the view
    d = v.transpose(1, 2)                                                      # the driver's [B, C, T, H, W]
    assert G.modules._strides5(d) == (16 * S * S * 3, S * S * 3, S * 3, 3, 1)  # {N, D, H, W, C}: channels-last, read in place
    x = next(ds.images(3))
    assert tuple(x.shape) == (3, 3, S, S) and x.stride() == (S * S * 3, 1, S * 3, 3) and x.permute(0, 2, 3, 1).is_contiguous()
    assert x.untyped_storage().nbytes() == x.numel() * 4


# ---------------------------------------------------------------------------------------------------------------------
# dataset
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", R.MODES)
def test_dataset_store_round_trip_and_streams(antialias, tmp_path):
    vids = _videos([(20, 60, 80), (17, 96, 128), (10, 60, 80), (33, 60, 80)], seed=2)
    ds = D.Ucf101OnDevice(antialias=antialias, seed=7)
    added = [ds.add_video(vids[0], 4), ds.add_video(vids[1].permute(0, 3, 1, 2).contiguous().cuda(), 9, channels_first=True),
             ds.add_video(vids[2], 5), ds.add_video(vids[3].cuda(), 2)]
    assert added == [True, True, False, True] and len(ds) == 3 and ds.n_frames == 70
    assert sorted(ds._tables) == [(60, 80), (96, 128)]                         # one table pair per source size
    off, length, lab = ds._tabs()
    assert (off.tolist(), length.tolist(), lab.tolist()) == ([0, 20, 37], [20, 17, 33], [4, 9, 2])
    assert tuple(ds.frames.shape) == (70, 64, 64, 3) and ds._store.shape[0] >= 70
    for k, o in ((0, 0), (1, 20), (3, 37)):
        v, want = D.resize_crop_reference(vids[k], 64, 85, 10, 64, antialias)
        t = ds._tables[tuple(vids[k].shape[1:3])]
        tol = R.tolerance(t.y_w.cpu(), t.x_w.cpu(), t.ky, t.kx)
        assert R.check_bytes(ds.frames[o:o + vids[k].shape[0]], v, want, tol) <= R.MAX_TIE_SHARE
    # growth keeps what is stored
    before = ds.frames.clone()
    cap = ds._store.shape[0]
    big = _videos([(cap, 8, 8)], seed=3)[0]
    assert ds.add_video(big, 1) and ds._store.shape[0] >= 2 * cap and torch.equal(ds.frames[:70], before)
    # save / load: bitwise, and the same streams for the same seed
    path = str(tmp_path / "ucf.pt")
    ds.save(path)
    back = D.Ucf101OnDevice.load(path, seed=7, antialias=antialias)
    assert back.frames.is_cuda and torch.equal(back.frames, ds.frames)
    assert all(torch.equal(a, b) for a, b in zip(back._tabs(), ds._tabs()))
    with pytest.raises(ValueError, match="antialias"):
        D.Ucf101OnDevice.load(path, antialias=not antialias)
    twin = R.host_twin(ds, seed=7)
    streams = [(s.videos(2, labels=True), s.images(3, labels=True)) for s in (ds, back, twin)]
    for _ in range(5):                                                          # 4 videos: more than two epochs of either
        got = [(next(sv), next(si)) for sv, si in streams]
        (wv, wvl), (wi, wil) = got[2]
        for (v, vl), (i, il) in got[:2]:
            assert v.is_cuda and vl.is_cuda and vl.dtype == torch.int64
            assert torch.equal(v.cpu(), wv) and torch.equal(vl.cpu(), wvl) and torch.equal(i.cpu(), wi) and torch.equal(il.cpu(), wil)
            assert v.stride() == wv.stride() and i.stride() == wi.stride()
        assert not bool(torch.isnan(wv).any())


# ---------------------------------------------------------------------------------------------------------------------
# trainer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("categories", [0, 4])
def test_trainer_iteration_fed_from_the_device_set_is_bitwise_the_oracle_fed_one(categories):
    """UCF shapes at ngf = ndf = 8, batch 2; the source frames already are 64 x 85, so the stored bytes are the kept columns."""
    vids = _videos([(20, 64, 85), (18, 64, 85), (25, 64, 85)], seed=4)
    ds = D.Ucf101OnDevice.from_videos(vids, labels=[1, 3, 0], seed=5)
    assert all(torch.equal(ds.frames[o:o + v.shape[0]].cpu(), v[:, :, 10:74]) for o, v in zip((0, 20, 38), vids))

    def batches(src, dev):
        sv, si = src.videos(2, labels=True), src.images(2, labels=True)
        vs, ims = [next(sv) for _ in range(2)], [next(si) for _ in range(2)]
        if not dev:          # oracle-built on the host: uploaded channels-last, viewed as the device set views its own
            vs = [(v.permute(0, 1, 3, 4, 2).contiguous().cuda().permute(0, 1, 4, 2, 3).clone(), l.cuda()) for v, l in vs]
            ims = [(i.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2).clone(), l.cuda()) for i, l in ims]
        return [i for i, _ in ims], [v for v, _ in vs], [l for _, l in vs]

    def run(dev):
        seed_all(60)
        gen = G.VideoGenerator(3, 50, categories, 16, 16, dim_hidden=16, ngf=8)
        dv = (G.CategoricalVideoDiscriminator(3, categories, ndf=8) if categories else G.VideoDiscriminator(3, ndf=8))
        di = G.PatchImageDiscriminator(3, ndf=8)
        nets = [m.cuda() for m in (gen, dv, di)]
        tr = G.GanTrainer(*nets)
        imgs, vs, labels = batches(ds if dev else R.host_twin(ds, seed=5), dev)
        seed_all(61)
        losses = tr.step(imgs, vs, labels if categories else None)
        torch.cuda.synchronize()
        return [l.clone() for l in losses], [p.detach().clone() for m in nets for p in m.parameters()], (imgs, vs)

    ds.gen.manual_seed(5)
    l0, w0, (i0, v0) = run(True)
    l1, w1, (i1, v1) = run(False)
    assert all(a.stride() == b.stride() and torch.equal(a, b) for a, b in zip(i0 + v0, i1 + v1))
    assert all(bool(torch.isfinite(a).all()) for a in l0)
    assert all(torch.equal(a, b) for a, b in zip(l0, l1)) and all(torch.equal(a, b) for a, b in zip(w0, w1))
