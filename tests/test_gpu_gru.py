"""GPU: the GRU (original MoCoGAN) motion latent -- gode_gru_fwd / gode_gru_bwd and their _multi forms against the float64
restatement of tests/gru_ref.py, VideoGeneratorGRU against the reference's own class (tests/golden/gen_gru_tiny*.npz,
written by scripts/make_gru_golden.py), and GanTrainer iterations against a stock-torch loop and across its schedule
options."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import gru_ref as R
from conftest import assert_weights_after_adam, golden, load_sd, rel_err, seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L
from oracle import mocogan_ref as M

pytestmark = pytest.mark.gpu
GUARD = 64
ZC = 96
TOL = 1e-4
NAN = float("nan")


def stream():
    return torch.cuda.current_stream().cuda_stream


def dptr(t):
    return None if t is None else t.data_ptr()


def _params(seed):
    seed_all(seed)
    cell = nn.GRUCell(16, 16)
    P = [cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh]
    return [p.detach().cuda().contiguous() for p in P], [p.detach().double().numpy() for p in P]


class Chain:
    """Inputs and outputs of one forward + backward pair, every output buffer inside NaN guards."""

    def __init__(self, P32, N, T, seed, select=False):
        g = torch.Generator().manual_seed(seed)
        self.P32, self.N, self.T = P32, N, T
        self.noise = torch.randn(T + 1, N, 16, generator=g)
        self.content = torch.randn(N, 50, generator=g)
        self.sel = torch.randint(0, T, (N,), generator=g, dtype=torch.int32) if select else None
        rows = N if select else N * T
        self.rows = rows
        self.gz = torch.randn(rows, ZC, generator=g)
        self.d_noise, self.d_content = self.noise.cuda(), self.content.cuda()
        self.d_sel = self.sel.cuda() if select else None
        self.d_gz = self.gz.cuda()
        self.zbuf = torch.full((rows * ZC + 2 * GUARD,), NAN, device="cuda")
        self.z = self.zbuf[GUARD:GUARD + rows * ZC].view(rows, ZC)
        self.hbuf = torch.full((N * (T + 1) * 16 + 2 * GUARD,), NAN, device="cuda")
        self.hs = self.hbuf[GUARD:-GUARD].view(N, T + 1, 16)
        self.work = torch.full((L.lib().gode_gru_bwd_work_size(N),), NAN, device="cuda")
        self.gbuf = torch.full((L.GRU_NPARAM + 2 * GUARD,), NAN, device="cuda")
        self.grads = self.gbuf[GUARD:GUARD + L.GRU_NPARAM]

    def fwd_op(self):
        return L.GruFwdOp(p=L.GruParams(*[dptr(p) for p in self.P32]), noise=dptr(self.d_noise),
                          content=dptr(self.d_content), sel_t=dptr(self.d_sel), z=dptr(self.z), hs=dptr(self.hs), N=self.N,
                          T=self.T, zcols=ZC)

    def bwd_op(self, accumulate=0, grads=None):
        return L.GruBwdOp(p=L.GruParams(*[dptr(p) for p in self.P32]), noise=dptr(self.d_noise), hs=dptr(self.hs),
                          sel_t=dptr(self.d_sel), gz=dptr(self.d_gz), work=dptr(self.work),
                          grads=dptr(self.grads if grads is None else grads), N=self.N, T=self.T, accumulate=accumulate,
                          zcols=ZC)

    def g_rows(self):
        """the upstream gradient of every h_{t+1} as [N, T, 16] (zero for the rows sel_t does not pick)"""
        g = np.zeros((self.N, self.T, 16))
        m = self.gz[:, :16].double().numpy()
        if self.sel is None:
            g[:] = m.reshape(self.N, self.T, 16)
        else:
            g[np.arange(self.N), self.sel.long().numpy()] = m
        return g


def _guards_nan(buf):
    b = buf.cpu()
    return bool(torch.isnan(b[:GUARD]).all() and torch.isnan(b[-GUARD:]).all())


@pytest.mark.parametrize("N", [1, 16, 33, 4096])
@pytest.mark.parametrize("T", [1, 16])
def test_gru_kernels_against_float64_restatement(N, T):
    P32, P64 = _params(7 + N + T)
    c = Chain(P32, N, T, seed=N * 31 + T)
    lib = L.lib()
    L.check(lib.gode_gru_fwd(C.byref(c.fwd_op()), stream()), "gode_gru_fwd")
    torch.cuda.synchronize()
    hs64 = R.forward(*P64, c.noise.double().numpy())
    assert rel_err(c.hs.cpu(), hs64) <= 1e-6
    assert rel_err(c.z[:, :16].cpu(), R.latent_rows(hs64)) <= 1e-6
    z = c.z.cpu()
    assert torch.equal(z[:, 16:66], c.content.repeat_interleave(T, dim=0)) and (z[:, 66:] == 0).all()
    assert _guards_nan(c.zbuf) and _guards_nan(c.hbuf)
    want = R.backward(*P64, c.noise.double().numpy(), hs64, c.g_rows())
    runs = []
    for acc in (0, 1):
        c.grads.copy_(torch.linspace(-1, 1, L.GRU_NPARAM))
        base = c.grads.clone()
        for rep in range(2):
            if rep:
                c.grads.copy_(base)
            L.check(lib.gode_gru_bwd(C.byref(c.bwd_op(accumulate=acc)), stream()), "gode_gru_bwd")
            got = c.grads.clone()
            torch.cuda.synchronize()
            assert _guards_nan(c.gbuf), acc
            runs.append(got)
        assert torch.equal(runs[-1], runs[-2])                  # run to run: bit-identical
        g = runs[-1].cpu().double().numpy() - (base.cpu().double().numpy() if acc else 0.0)
        for a, b in zip(R.split(g), R.split(want)):
            assert rel_err(a, b) <= 1e-5, (acc, rel_err(a, b))
    # accumulate = 1 adds exactly the accumulate = 0 result in fp32
    assert torch.equal(runs[2], (base + runs[0]))


def test_gru_select_rows_against_float64_restatement():
    P32, P64 = _params(5)
    c = Chain(P32, 50, 16, seed=9, select=True)
    lib = L.lib()
    L.check(lib.gode_gru_fwd(C.byref(c.fwd_op()), stream()), "gode_gru_fwd")
    L.check(lib.gode_gru_bwd(C.byref(c.bwd_op()), stream()), "gode_gru_bwd")
    torch.cuda.synchronize()
    hs64 = R.forward(*P64, c.noise.double().numpy())
    picked = hs64[np.arange(50), c.sel.long().numpy() + 1]
    assert rel_err(c.z[:, :16].cpu(), picked) <= 1e-6
    assert torch.equal(c.z[:, 16:66].cpu(), c.content)
    want = R.backward(*P64, c.noise.double().numpy(), hs64, c.g_rows())
    for a, b in zip(R.split(c.grads.cpu().double().numpy()), R.split(want)):
        assert rel_err(a, b) <= 1e-5
    assert _guards_nan(c.gbuf) and _guards_nan(c.zbuf)


@pytest.mark.parametrize("sizes", [(16, 16), (40, 100), (33, 1)])
def test_gru_multi_launches_are_bitwise_the_separate_launches(sizes):
    lib = L.lib()
    P32, _ = _params(11)
    chains = [Chain(P32, n, 16, seed=100 + k, select=bool(k % 2)) for k, n in enumerate(sizes)]
    shared = torch.full((L.GRU_NPARAM,), 0.25, device="cuda")
    results = []
    for multi in (False, True):
        for c in chains:
            c.z.fill_(NAN); c.hs.fill_(NAN)
        shared.fill_(0.25)
        fops = [c.fwd_op() for c in chains]
        bops = [c.bwd_op(accumulate=k, grads=shared) for k, c in enumerate(chains)]    # store, then add
        if multi:
            arr = (L.GruFwdOp * len(fops))(*fops)
            L.check(lib.gode_gru_fwd_multi(arr, len(fops), stream()), "gode_gru_fwd_multi")
            arr = (L.GruBwdOp * len(bops))(*bops)
            L.check(lib.gode_gru_bwd_multi(arr, len(bops), stream()), "gode_gru_bwd_multi")
        else:
            for op in fops:
                L.check(lib.gode_gru_fwd(C.byref(op), stream()), "gode_gru_fwd")
            for op in bops:
                L.check(lib.gode_gru_bwd(C.byref(op), stream()), "gode_gru_bwd")
        torch.cuda.synchronize()
        results.append([t.clone() for c in chains for t in (c.z, c.hs)] + [shared.clone()])
    for a, b in zip(*results):
        assert torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))
    assert torch.isfinite(results[1][-1]).all()


def test_gru_sample_z_m_is_differentiable_and_matches_restatement():
    seed_all(3)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=8).cuda()
    seed_all(4)
    noise = torch.empty(9, 5, 16)
    for i in range(9):
        noise[i].normal_()
    seed_all(4)
    zm = gen.sample_z_m(5, video_len=8)
    assert tuple(zm.shape) == (40, 16) and zm.requires_grad
    P64 = [p.detach().double().cpu().numpy() for p in gen._param_list()[1]]
    hs64 = R.forward(*P64, noise.double().numpy())
    assert rel_err(zm.detach().cpu(), R.latent_rows(hs64)) <= 1e-6
    g = torch.randn(40, 16)
    (zm * g.cuda()).sum().backward()
    want = R.split(R.backward(*P64, noise.double().numpy(), hs64, g.double().numpy().reshape(5, 8, 16)))
    for p, w in zip(gen._param_list()[1], want):
        assert rel_err(p.grad.cpu(), w) <= 1e-5
    z, labels = gen.sample_z_video(3)
    assert tuple(z.shape) == (48, 66) and np.array_equal(labels, np.zeros(3))


def _gru_fixture():
    merged = {}
    for name in ("gen_gru_tiny.npz", "gen_gru_tiny_grads.npz", "gen_gru_tiny_videos.npz", "gen_gru_tiny_eval.npz"):
        part = golden(name)
        for k in part.files:
            merged[k] = part[k]
    return merged


def _f32(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32))


def robust_rel(a, b):
    """median error over the RMS of the reference (tests/test_gpu_modules.py's measure): robust against one flipped
    BatchNorm / ReLU kink in these tiny nets"""
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64).flatten()
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64).flatten()
    return float((a - b).abs().median() / (b.norm() / b.numel() ** 0.5).clamp_min(1e-300))


def test_gru_generator_against_reference_fixture():
    g = _gru_fixture()
    s = int(g["seed"])
    from models.mocogan import VideoGenerator
    gen = VideoGenerator(3, 50, 0, 16, 16, ngf=int(g["ngf"]))
    load_sd(gen, g, "w")
    gen.cuda()
    seed_all(s + 1)
    vid, labels = gen.sample_videos(1)
    seed_all(s + 2)
    img, _ = gen.sample_images(3)
    assert tuple(vid.shape) == g["videos"].shape and tuple(img.shape) == g["images"].shape
    assert labels.dtype == torch.float64 and labels.is_cuda and float(labels.abs().sum()) == 0.0
    assert rel_err(vid.detach().cpu(), g["videos"]) < TOL
    assert rel_err(img.detach().cpu(), g["images"]) < TOL
    ((vid * _f32(g["wv"]).cuda()).sum() + (img * _f32(g["wi"]).cuda()).sum()).backward()
    seen_rec = 0
    for k, p in gen.named_parameters():
        ref = g[f"g/{k}"]
        assert ref.size > 0, k
        seen_rec += k.startswith("recurrent.")
        assert robust_rel(p.grad.cpu(), ref) < 5e-3, (k, robust_rel(p.grad.cpu(), ref), rel_err(p.grad.cpu(), ref))
        assert rel_err(p.grad.cpu(), ref) < 5e-2, (k, rel_err(p.grad.cpu(), ref))
    assert seen_rec == 4
    for k, v in gen.state_dict().items():
        if "running_" in k:
            assert rel_err(v.cpu(), g[f"w_after/{k}"]) < TOL, k
        if "num_batches" in k:
            assert int(v) == int(g[f"w_after/{k}"]), k
    gen.eval()
    seed_all(s + 4)
    with torch.no_grad():
        ev, _ = gen.sample_videos(1)
    assert rel_err(ev.cpu(), g["videos_eval"]) < TOL


class _RefGru(nn.Module):
    """Stock torch: the reference's MoCoGAN VideoGenerator (nn.GRUCell + the 64x64 decoder) with the noise drawn on the
    CPU generator in the reference's order and moved to the module's device."""

    def __init__(self, ngf):
        super().__init__()
        self.recurrent = nn.GRUCell(16, 16)
        self.main = M._decoder(66, ngf, 3, mnist=False)
        self.video_length = 16

    def _dev(self):
        return self.main[0].weight.device

    def sample_z_m(self, n, T):
        h = [torch.FloatTensor(n, 16).normal_().to(self._dev())]
        for _ in range(T):
            h.append(self.recurrent(torch.FloatTensor(n, 16).normal_().to(self._dev()), h[-1]))
        return torch.cat([k.view(-1, 1, 16) for k in h[1:]], dim=1).view(-1, 16)

    def sample_z_video(self, n, T=None):
        T = T or self.video_length
        c = np.random.normal(0, 1, (n, 50)).astype(np.float32)
        zc = torch.from_numpy(np.repeat(c, T, axis=0)).to(self._dev())
        return torch.cat([zc, self.sample_z_m(n, T)], dim=1), np.zeros(n)

    def sample_videos(self, n, video_len=None):
        T = video_len or self.video_length
        z, labels = self.sample_z_video(n, T)
        h = self.main(z.view(z.size(0), z.size(1), 1, 1))
        return h.view(h.size(0) // T, T, 3, h.size(3), h.size(3)).permute(0, 2, 1, 3, 4), torch.from_numpy(labels)

    def sample_images(self, n):
        z, _ = self.sample_z_video(n * self.video_length * 2)
        j = np.sort(np.random.choice(z.size(0), n, replace=False)).astype(np.int64)
        z = z[j]
        return self.main(z.view(z.size(0), z.size(1), 1, 1)), None


def _trainer_data(B, seed):
    rng = torch.Generator().manual_seed(seed)
    imgs = [torch.rand(B, 3, 64, 64, generator=rng) * 2 - 1 for _ in range(2)]
    vids = [torch.rand(B, 16, 3, 64, 64, generator=rng) * 2 - 1 for _ in range(2)]
    return imgs, vids


def _check_against_stock(nets, refs):
    for m, o in zip(nets, refs):
        osd = o.state_dict()
        for k, v in m.state_dict().items():
            w = osd[k].cpu()
            if v.dtype == torch.int64:
                assert int(v) == int(w), k
            elif "running_" in k:
                assert rel_err(v.cpu(), w) < 5e-3, k
            else:
                assert_weights_after_adam(v.cpu(), w, k)


def test_gru_trainer_two_iterations_against_stock_torch_loop():
    """Two GanTrainer iterations against the reference loop body on stock torch modules (nn.GRUCell, the reference
    decoder and discriminators, torch.optim.Adam) with the same draws.  Each iteration starts from the same weights: the
    stock networks take ours before the second (post-Adam weights differ by sign-like 2 lr flips of near-zero
    gradients, which a second step would compound); the optimisers keep their own moments."""
    B, W = 8, 8
    seed_all(81)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=W)
    dv, di = G.VideoDiscriminator(3, ndf=W), G.PatchImageDiscriminator(3, ndf=W)
    ogen, odv, odi = _RefGru(W), M.VideoDisc(3, ndf=W), M.PatchImageDisc(3, ndf=W)
    nets, refs = (gen, dv, di), (ogen, odv, odi)
    for m, o in zip(nets, refs):
        o.load_state_dict(m.state_dict())
        m.cuda()
        o.cuda()
    tr = G.GanTrainer(gen, dv, di)
    opts = M.make_optimizers(ogen, odv, odi)
    for it in range(2):
        if it:
            for m, o in zip(nets, refs):
                with torch.no_grad():
                    for k, v in o.state_dict().items():
                        v.copy_(m.state_dict()[k])
        imgs, vids = _trainer_data(B, 20 + it)
        seed_all(82 + it)
        got = [float(v) for v in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])]
        seed_all(82 + it)
        want = [float(v) for v in M.train_step(ogen, odv, odi, opts, [t.cuda() for t in imgs], [t.cuda() for t in vids])]
        # the second iteration's D losses come after an Adam step whose moments differ in the last bits
        assert np.allclose(got, want, rtol=1e-5 if it == 0 else 1e-4, atol=0), (it, got, want)
        _check_against_stock(nets, refs)
        for p in gen.recurrent.parameters():
            assert p.grad is not None and float(p.grad.abs().max()) > 0


def _run_trainer(**kw):
    seed_all(91)
    gen = G.VideoGeneratorGRU(3, 50, 0, 16, 16, ngf=8)
    dv, di = G.VideoDiscriminator(3, ndf=8), G.PatchImageDiscriminator(3, ndf=8)
    gen.cuda(); dv.cuda(); di.cuda()
    tr = G.GanTrainer(gen, dv, di, **kw)
    losses = []
    for it in range(2):
        imgs, vids = _trainer_data(4, 30 + it)
        seed_all(700 + it)
        losses.append([float(x) for x in tr.step([t.cuda() for t in imgs], [t.cuda() for t in vids])])
    torch.cuda.synchronize()
    assert not gen.__dict__.get("_prefetched")
    assert all(np.isfinite(v) for row in losses for v in row)
    state = {f"{i}/{k}": t.detach().clone() for i, m in enumerate((gen, dv, di)) for k, t in m.state_dict().items()}
    grads = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
    return losses, state, grads


@pytest.mark.parametrize("option", ["prefetch_latents", "direct_grads", "overlap_image_d"])
def test_gru_trainer_options_are_bitwise_neutral(option):
    on, off = _run_trainer(**{option: True}), _run_trainer(**{option: False})
    assert on[0] == off[0], (option, on[0], off[0])
    for k in on[1]:
        assert torch.equal(on[1][k], off[1][k]), (option, k)
    for k in on[2]:                        # every generator tensor received its gradient, recurrent.* included
        assert torch.equal(on[2][k], off[2][k]), (option, k)


def test_gru_trainer_joint_generator_passes():
    """One decoder pass over both batches sums the decoder's weight gradients in another order (as for every generator:
    main.{3,6,9}.weight differ in the last bits); the GRU latent, its gradients' order of accumulation (video path, then
    image path) and the first iteration's losses are bitwise the two-call schedule's."""
    on, off = _run_trainer(joint_generator_passes=True), _run_trainer(joint_generator_passes=False)
    assert on[0][0] == off[0][0], (on[0], off[0])
    assert np.allclose(on[0][1], off[0][1], rtol=1e-4, atol=0), (on[0], off[0])
    for k in on[1]:
        if "num_batches" in k:
            assert torch.equal(on[1][k], off[1][k]), k
        elif "running_" in k:
            assert rel_err(on[1][k].cpu(), off[1][k].cpu()) < 1e-4, k
        else:
            assert_weights_after_adam(on[1][k].cpu(), off[1][k].cpu(), k)

