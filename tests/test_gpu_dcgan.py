"""GPU: stage 2's CIFAR DCGAN on libgode -- GODE_ACT_LRELU01 and gode_bce_logits_t through the C ABI against fp64 NumPy, the
modules against the fp64 restatement of tests/dc_ref.py, GANODETrainer with the notebook's closures on the new modules, the
regulariser's rewind of the device generator, and drop-in behaviour.

Module and trainer allowances are the rule of DESIGN sections 14 and 16: per tensor, conftest.rel_err against the fp64 restatement
may be 8x the error of the fp32 CPU restatement against the fp64 one on the same problem -- figures stored in
tests/golden/dcgan_own.npz (scripts/make_dcgan_goldens.py), because they depend on the host's BLAS and thread count.  The op tests'
bounds are counted roundings (U = 2^-24), written where they are used.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dc_ref as R
from conftest import rel_err

import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import dcgan
from gan_ode_amd.engine import dptr, make_geom, stream_ptr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SLOPE = float(np.float32(0.1))          # the kernels' slope: fp32(0.1), 0.25 U above 0.1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(op):
    L.run_one(op, stream_ptr())
    torch.cuda.synchronize()


def _lrelu64(v):
    return np.where(v > 0, v, 0.1 * v)


def _worst(err, bound):
    return float((err / (bound + 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------
# GODE_ACT_LRELU01 through the ops of the convolution stack
@pytest.mark.parametrize("C_", [6, 64])
@pytest.mark.parametrize("M", [1, 130])
def test_lrelu01_through_bn_apply_bn_bwd_and_the_igemm_operand_load(M, C_):
    rng = np.random.RandomState(1000 * M + C_)
    lib = L.lib()
    y = (rng.randn(M, C_) * 1.5).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C_).astype(np.float32), rng.randn(C_).astype(np.float32)
    mean = y.astype(np.float64).mean(0).astype(np.float32)
    invstd = (1.0 / np.sqrt(y.astype(np.float64).var(0) + 1e-5)).astype(np.float32)
    scale = (gamma * invstd).astype(np.float32)
    shift = (beta - mean * scale).astype(np.float32)
    # no element within 1e-3 of either kink (of y itself, or of y * scale + shift): fp32 and fp64 agree about every slope
    y = np.where(np.abs(y) < 1e-3, np.float32(0.5), y)
    z = y.astype(np.float64) * scale + shift
    y = np.where(np.abs(z) < 1e-3, ((0.5 - shift.astype(np.float64)) / scale).astype(np.float32), y).astype(np.float32)
    z = y.astype(np.float64) * scale + shift
    assert np.abs(z).min() > 1e-4 and np.abs(y).min() > 1e-4
    g = rng.randn(M, C_).astype(np.float32)
    yd, gd, scd, shd = _dev(y), _dev(g), _dev(scale), _dev(shift)
    zmag = np.abs(y.astype(np.float64) * scale) + np.abs(shift)

    # gode_bn_apply: C % 4 == 0 is its stated contract, anything else is an argument error before any launch
    out = torch.full((M, C_), float("nan"), device="cuda")
    if C_ % 4:
        op = L.BnApplyOp(y=dptr(yd), out=dptr(out), scale=dptr(scd), shift=dptr(shd), M=M, C=C_, act=L.ACT_LRELU01)
        assert lib.gode_bn_apply(C.byref(op), stream_ptr()) == -1
    else:
        _run(L.BnApplyOp(y=dptr(yd), out=dptr(out), scale=dptr(scd), shift=dptr(shd), M=M, C=C_, act=L.ACT_LRELU01))
        # t = y * scale + shift: <= 2 U (|y scale| + |shift|) (one rounding when fused); times fp32(0.1): 0.25 U + 1 U of the value
        err, bound = np.abs(out.cpu().numpy() - _lrelu64(z)), 4 * U * zmag
        assert (err <= bound).all(), _worst(err, bound)
        print(f"M={M} C={C_}: bn_apply {_worst(err, bound):.3f} of its bound")
        _run(L.BnApplyOp(y=dptr(yd), out=dptr(out), scale=None, shift=None, M=M, C=C_, act=L.ACT_LRELU01))
        err, bound = np.abs(out.cpu().numpy() - _lrelu64(y.astype(np.float64))), 2 * U * np.abs(y)
        assert (err <= bound).all(), _worst(err, bound)

    # gode_bn_bwd without BatchNorm (any C): g_y = g * act'(y), in place and from a separate upstream tensor
    want = g.astype(np.float64) * np.where(y > 0, 1.0, 0.1)
    for separate in (False, True):
        buf = torch.full((M, C_), float("nan"), device="cuda") if separate else gd.clone()
        _run(L.BnBwdOp(g=dptr(buf), y=dptr(yd), M=M, C=C_, act=L.ACT_LRELU01, gin=dptr(gd) if separate else None))
        err, bound = np.abs(buf.cpu().numpy() - want), 2 * U * np.abs(g)       # the slope's 0.25 U and one product
        assert (err <= bound).all(), (separate, _worst(err, bound))

    # gode_bn_bwd with BatchNorm (C % 4 == 0)
    work = torch.empty(lib.gode_bn_bwd_work_size(M, C_), device="cuda")
    gam, mu, isd = _dev(gamma), _dev(mean), _dev(invstd)
    dgam, dbet = torch.full((C_,), float("nan"), device="cuda"), torch.full((C_,), float("nan"), device="cuda")
    buf = gd.clone()
    op = L.BnBwdOp(g=dptr(buf), y=dptr(yd), M=M, C=C_, act=L.ACT_LRELU01, gamma=dptr(gam), mean=dptr(mu), invstd=dptr(isd),
                   scale=dptr(scd), shift=dptr(shd), dgamma=dptr(dgam), dbeta=dptr(dbet), work=dptr(work))
    if C_ % 4:
        assert lib.gode_bn_bwd(C.byref(op), stream_ptr()) == -1
    else:
        _run(op)
        gz = g.astype(np.float64) * np.where(z > 0, 1.0, 0.1)
        xhat = (y.astype(np.float64) - mean) * invstd
        dbeta, dgamma = gz.sum(0), (gz * xhat).sum(0)
        k = np.abs(gamma.astype(np.float64) * invstd)
        want = gamma.astype(np.float64) * invstd * (gz - dbeta / M - xhat * dgamma / M)
        # the sums run in double over fp32 terms: g_z carries 1.25 U (slope + product), g_z * xhat 4.25 U (xhat: a difference and
        # a product); then per element three coefficient products, a difference and two additions: 12 U of the terms' magnitudes
        sb, sg = np.abs(gz).sum(0), np.abs(gz * xhat).sum(0)
        bound = 12 * U * k * (np.abs(gz) + np.abs(dbeta) / M + np.abs(xhat * dgamma) / M) + 5 * U * k * (sb / M + np.abs(xhat) * sg / M)
        err = np.abs(buf.cpu().numpy() - want)
        assert (err <= bound + 1e-45).all(), _worst(err, bound)
        assert (np.abs(dbet.cpu().numpy() - dbeta) <= 3 * U * sb + 1e-45).all()
        assert (np.abs(dgam.cpu().numpy() - dgamma) <= 6 * U * sg + 1e-45).all()
        print(f"M={M} C={C_}: bn_bwd g_y {_worst(err, bound):.3f}, dbeta {_worst(np.abs(dbet.cpu().numpy() - dbeta), 3 * U * sb):.3f}, "
              f"dgamma {_worst(np.abs(dgam.cpu().numpy() - dgamma), 6 * U * sg):.3f} of their bounds")

    # gode_igemm: a 1x1 convolution of M pixels, C -> 8 channels, the transform applied while the operand is loaded (any C)
    Co = 8
    w = (rng.randn(Co, C_) * 0.3).astype(np.float32)
    geom = make_geom(M, C_, Co, (1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0))
    n = lib.gode_pack_size(C.byref(geom), L.FPROP)
    assert n > 0
    wd, wp = _dev(w), torch.empty(n, device="cuda")
    L.check(lib.gode_pack_weights(C.byref(geom), L.FPROP, dptr(wd), dptr(wp), None, 0, stream_ptr()), "gode_pack_weights")
    for xf in (True, False):
        out = torch.full((M, Co), float("nan"), device="cuda")
        op = L.IgemmOp(g=geom, dir=L.FPROP, act=L.ACT_LRELU01, epilogue=L.EPI_RAW, tile=0, src=dptr(yd), wpack=dptr(wp), out=dptr(out),
                       scale=dptr(scd) if xf else None, shift=dptr(shd) if xf else None)
        need = lib.gode_igemm_work_size(C.byref(op))
        assert need >= 0
        wk = torch.empty(max(need, 1), device="cuda")
        op.work = dptr(wk)
        _run(op)
        a = _lrelu64(z if xf else y.astype(np.float64))
        amag = zmag if xf else np.abs(y.astype(np.float64))
        want = a @ w.astype(np.float64).T
        # every operand within 4 U of its magnitude (as gode_bn_apply above), then C products accumulated in fp32: (C + 2) U
        bound = 4 * U * (amag @ np.abs(w).astype(np.float64).T) + (C_ + 2) * U * (np.abs(a) @ np.abs(w).astype(np.float64).T)
        err = np.abs(out.cpu().numpy() - want)
        assert (err <= bound).all(), (xf, _worst(err, bound))
        print(f"M={M} C={C_}: igemm operand load (scale/shift {xf}) {_worst(err, bound):.3f} of its bound")


# ---------------------------------------------------------------------------------------------------------------
# gode_bce_logits_t
def _bce_case(n):
    rng = np.random.RandomState(n)
    x = (rng.randn(n) * 3).astype(np.float32)
    t = np.asarray([0.0, 1.0, 0.3], dtype=np.float32)[np.arange(n) % 3]
    if n >= 8:
        x[:8] = [100, 100, 100, -100, -100, -100, 0, 30]         # +-100 against each of the three targets
    else:
        x[0] = 100
    return x, t


def _bce64(x, t, gscale=1.0):
    x, t = x.astype(np.float64), t.astype(np.float64)
    l = np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))
    sig = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    # per element: the product x t (1 U), log1pf(expf()) (<= 4 U of <= 0.7), a difference and a sum (2 U of the larger term)
    lbound = 4 * U * (np.abs(x) * (1 + np.abs(t)) + 0.7)
    # sigmoid: expf (<= 3 U), a sum, a division: 6 U of it; sigmoid - t, times gscale, times fp32(1 / n): 4 U of the result.  Below
    # fp32's smallest normal number the device's value may be zero (expf(100) is infinite): 2^-126 on top
    gbound = (6 * U * sig + 4 * U * np.abs(sig - t)) * abs(gscale) / len(x) + 2.0 ** -126
    return float(l.mean()), gscale * (sig - t) / len(x), float(lbound.mean()), gbound


@pytest.mark.parametrize("n", [1, 100, 257])
def test_bce_logits_t_against_fp64(n):
    x, t = _bce_case(n)
    xd, td = _dev(x), _dev(t)
    want_l, want_g, lbound, gbound = _bce64(x, t)
    runs = []
    for _ in range(2):
        loss, grad = torch.full((1,), float("nan"), device="cuda"), torch.full((n + 4,), float("nan"), device="cuda")
        _run(L.BceTOp(logits=dptr(xd), target=dptr(td), grad=dptr(grad), loss=dptr(loss), n=n, gscale=1.0, accumulate=0))
        runs.append((loss.cpu().numpy(), grad.cpu().numpy()))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(runs[0], runs[1])), "two runs differ"
    gl, gg = float(runs[0][0][0]), runs[0][1]
    assert np.isnan(gg[n:]).all(), "wrote past n"
    gg = gg[:n]
    assert np.isfinite(gl) and np.isfinite(gg).all()
    print(f"n={n}: loss {gl:.9g} fp64 {want_l:.9g}: {abs(gl - want_l) / (lbound + U * abs(want_l)):.3f} of its bound; "
          f"gradient {_worst(np.abs(gg - want_g), gbound):.3f}")
    assert abs(gl - want_l) <= lbound + U * abs(want_l)              # the double sum is exact to fp32; one final rounding
    assert (np.abs(gg - want_g) <= gbound).all(), _worst(np.abs(gg - want_g), gbound)
    # no gradient wanted
    loss = torch.full((1,), float("nan"), device="cuda")
    _run(L.BceTOp(logits=dptr(xd), target=dptr(td), grad=None, loss=dptr(loss), n=n, gscale=1.0, accumulate=0))
    assert float(loss[0]) == gl
    # accumulate and gscale
    loss, grad = torch.full((1,), 2.5, device="cuda"), torch.empty(n, device="cuda")
    _run(L.BceTOp(logits=dptr(xd), target=dptr(td), grad=dptr(grad), loss=dptr(loss), n=n, gscale=-2.0, accumulate=1))
    assert float(loss[0]) == float(np.float32(2.5) + np.float32(gl))
    _, want_g2, _, gbound2 = _bce64(x, t, -2.0)
    assert (np.abs(grad.cpu().numpy() - want_g2) <= gbound2).all()
    # a constant-valued target tensor: gode_bce_logits' loss and gradient bit for bit
    for target in (0.0, 1.0, 0.3):
        tc = torch.full((n,), target, device="cuda")
        outs = []
        for op in (L.BceTOp(logits=dptr(xd), target=dptr(tc), n=n, gscale=1.5, accumulate=0),
                   L.BceOp(logits=dptr(xd), target=target, n=n, gscale=1.5, accumulate=0, stride=0)):
            loss, grad = torch.full((1,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
            op.loss, op.grad = dptr(loss), dptr(grad)
            _run(op)
            outs.append((loss.cpu().numpy(), grad.cpu().numpy()))
        assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)), target
        assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32)), target


def test_bce_module_against_stock_torch_on_the_cpu():
    x, t = _bce_case(100)
    crit = dcgan.BCEWithLogitsLoss()
    for shape in ((100,), (100, 1), (4, 25)):
        for tdt in (torch.float32, torch.float64):
            xd = _dev(x.reshape(shape)).requires_grad_(True)
            mine = crit(xd, _dev(t.reshape(shape)).to(tdt))
            (3.0 * mine).backward()
            xc = torch.from_numpy(x.reshape(shape)).double().requires_grad_(True)
            want = torch.nn.BCEWithLogitsLoss()(xc, torch.from_numpy(t.reshape(shape)).to(tdt))
            (3.0 * want).backward()
            _, _, lbound, gbound = _bce64(x, t, 3.0)
            assert mine.shape == () and mine.dtype == torch.float32              # fp32 whatever the target (recorded deviation)
            assert abs(float(mine.detach()) - float(want.detach())) <= lbound + U * abs(float(want.detach()))
            assert xd.grad.shape == shape and xd.grad.dtype == torch.float32
            # (+ 1 U: the upstream factor is applied by a torch multiply)
            gerr = np.abs(xd.grad.cpu().numpy().reshape(-1) - xc.grad.numpy().reshape(-1))
            assert (gerr <= gbound + U * np.abs(xc.grad.numpy().reshape(-1))).all()
    with pytest.raises(ValueError):
        crit(_dev(x.reshape(100, 1)), _dev(t))
    with pytest.raises(ValueError):
        dcgan.BCEWithLogitsLoss(reduction="sum")
    with pytest.raises(RuntimeError):
        crit(_dev(x), _dev(t).to(torch.float16))
    with pytest.raises(RuntimeError):
        crit(_dev(x), _dev(t).requires_grad_(True))


# ---------------------------------------------------------------------------------------------------------------
def _check(tag, got, ref64, prefix):
    """the 8x rule, per tensor; prints the ratios"""
    assert set(got) == set(ref64), set(got) ^ set(ref64)
    bad, worst = {}, (0.0, None)
    for n in ref64:
        err, own = rel_err(got[n], ref64[n]), R.stored_own()[f"{prefix}/{n}"]
        ratio = err / own if own > 0 else (0.0 if err == 0 else float("inf"))
        print(f"{tag} {n}: err {err:.3e}, fp32 CPU restatement {own:.3e}, ratio {ratio:.2f}")
        worst = max(worst, (ratio, n))
        if not err <= 8 * own:
            bad[n] = (err, own)
    print(f"{tag}: worst ratio {worst[0]:.2f} ({worst[1]})")
    assert not bad, (tag, bad)


def _product_a(w, seed):
    Gn, Dn = R.a_load_product(dcgan.Generator(1, nz=R.A_NZ, ngf=w), dcgan.Discriminator(1, ndf=w), w, seed)
    return Gn.cuda(), Dn.cuda()


@pytest.mark.parametrize("w,B", R.A_CASES)
def test_narrow_networks_both_losses_against_the_restatement(w, B):
    ref64 = R.a_reference(w, B)[0]
    seed = R.A_SEED[w, B]
    Gn, Dn = _product_a(w, seed)
    z, real = R.a_inputs(B, seed)
    got = R.run_pair(Gn, Dn, dcgan.BCEWithLogitsLoss(), z, real)
    _check(f"a ngf=ndf={w} B={B}", got, ref64, f"a/{w}/{B}")


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("B", R.B_CASES)
def test_full_width_discriminator_sign_definite(B, sign):
    ref64 = R.b_reference(B, sign, False)[0]
    Dn = dcgan.Discriminator(1)
    Dn.load_state_dict(R.b_weights(sign))
    Dn.cuda()
    x, r = R.b_input(B, sign)
    got = R.run_disc(Dn, x, r)
    _check(f"b B={B} sign={sign}", got, ref64, f"b/{B}/{sign}")
    # the same values behind channels-last strides (what the generator hands over): read in place, the same bits
    xv = x.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert xv.stride() != x.cuda().stride() and torch.equal(xv, x.cuda())
    again = R.run_disc(Dn, xv, r)
    for n in got:
        assert torch.equal(again[n], got[n]), n


@pytest.mark.parametrize("B", R.C_CASES)
def test_full_width_generator_kink_free(B):
    ref64 = R.c_reference(B, False)[0]
    Gn = dcgan.Generator(1)
    Gn.load_state_dict(R.c_weights())
    Gn.cuda()
    got = R.run_gen_train_then_eval(Gn, B)
    assert tuple(got["train/project.weight"].shape) == (8192, 128, 1, 1)
    _check(f"c B={B}", got, ref64, f"c/{B}")


def test_full_width_forward_at_the_stock_initialisation():
    ref64 = R.f_reference()[0]
    Gn, Dn = R.f_load(dcgan.Generator(1), dcgan.Discriminator(1))
    got = R.run_forward(Gn.cuda(), Dn.cuda(), dcgan.BCEWithLogitsLoss())
    assert tuple(got["G(z)"].shape) == (R.F_B, 3, 32, 32) and tuple(got["D(G(z))"].shape) == (R.F_B,)
    _check("forward B=16", got, ref64, "f")


# ---------------------------------------------------------------------------------------------------------------
# GANODETrainer with the notebook's closures
def _trainer(Gn, Dn, method, reg, randn=None, modules=None):
    d_loss, g_loss = R.closures(Gn, Dn, dcgan.BCEWithLogitsLoss(), "cuda", torch.float32, randn=randn)
    tr = G.GANODETrainer(Gn.parameters(), Dn.parameters(), None, g_loss, d_loss, None, lr=R.TRAINER_LR, reg=reg, method=method,
                         modules=modules)
    return tr, g_loss


@pytest.mark.parametrize("method", ["euler", "rk2", "rk4"])
def test_trainer_steps_against_the_restatement(method):
    d64, g64 = R.trainer_reference(method)[0]
    seed = R.TRAINER_SEED[method]
    Gn, Dn = _product_a(R.T_W, seed)
    tr, _ = _trainer(Gn, Dn, method, 0.0)
    bD, bG = R.params_of(Dn), R.params_of(Gn)
    R.seed_all(seed)
    l1 = tr.step(R.real_batch(seed), model="dis_img")
    after_d = R.params_of(Gn)
    l2 = tr.step(model="gen")
    assert np.isfinite(float(l1.detach())) and np.isfinite(float(l2.detach()))
    assert all(torch.equal(after_d[n], bG[n]) for n in bG), "the discriminator's step moved the generator"
    _check(f"{method} dis_img delta", R.delta_of(Dn, bD), d64, f"step/{method}/D")
    _check(f"{method} gen delta", R.delta_of(Gn, bG), g64, f"step/{method}/G")


def test_penalty_against_the_central_difference_and_a_penalised_step():
    seed = R.PENALTY_SEED
    Gn, Dn = _product_a(R.T_W, seed)
    tr, g_loss = _trainer(Gn, Dn, "euler", 0.01, modules=(Gn, Dn, None))
    gp64 = R.penalty_reference(tr.fd_h)[0]
    before = R.params_of(Gn)
    R.seed_all(seed)
    g_loss()                                    # what ONE call leaves behind: generator states and running statistics
    want_rng = torch.get_rng_state()
    want_buf = {n: b.detach().cpu().clone() for n, b in Gn.named_buffers()}
    Gn.load_state_dict(R.a_weights(R.T_W, seed)[0])
    R.seed_all(seed)
    gp = tr.grad_penalty("dis_img")
    assert torch.equal(torch.get_rng_state(), want_rng)
    after = R.params_of(Gn)
    assert all(torch.equal(after[n], before[n]) for n in before), "generator not restored bitwise"
    for n, b in Gn.named_buffers():
        assert torch.equal(b.detach().cpu(), want_buf[n]), n
    got = {n: g.detach().cpu() for (n, _), g in zip(Dn.named_parameters(), gp)}
    _check("penalty", got, gp64, "penalty")
    # one penalised Euler dis_img step: the generator as found, every discriminator tensor moved
    bD = R.params_of(Dn)
    loss = tr.step(R.real_batch(seed), model="dis_img")
    assert np.isfinite(float(loss.detach()))
    after = R.params_of(Gn)
    assert all(torch.equal(after[n], before[n]) for n in before), "generator not restored bitwise by the penalised step"
    assert all(not torch.equal(p.detach().cpu(), bD[n]) for n, p in Dn.named_parameters())


def test_penalty_rewinds_the_device_generator():
    """The notebook draws z with torch.randn(..., device=device): all three g_loss evaluations of the regulariser see the same z,
    and the CUDA generator is left where ONE call leaves it."""
    seed = R.PENALTY_SEED
    Gn, Dn = _product_a(R.T_W, seed)
    zs = []

    def randn(*shape):
        zs.append(torch.randn(*shape, device="cuda"))
        return zs[-1]

    tr, g_loss = _trainer(Gn, Dn, "euler", 0.01, randn=randn)
    torch.cuda.manual_seed(1234)
    start = torch.cuda.get_rng_state()
    cpu_before = torch.get_rng_state()
    g_loss()
    want_after, z_first = torch.cuda.get_rng_state(), zs[-1].clone()
    assert not torch.equal(want_after, start)
    zs.clear()
    torch.cuda.set_rng_state(start)
    gp = tr.grad_penalty("dis_img")
    assert len(zs) == 3 and all(torch.equal(z, z_first) for z in zs), "the evaluations saw different z"
    assert torch.equal(torch.cuda.get_rng_state(), want_after)
    assert torch.equal(torch.get_rng_state(), cpu_before)            # nothing was drawn on the host
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in gp)
    # ... and a whole penalised step: d_loss's draw, then one g_loss call's worth
    zs.clear()
    torch.cuda.set_rng_state(start)
    torch.randn(R.T_B, R.A_NZ, 1, 1, device="cuda"), torch.randn(R.T_B, R.A_NZ, 1, 1, device="cuda")
    want_step = torch.cuda.get_rng_state()
    torch.cuda.set_rng_state(start)
    tr.step(R.real_batch(seed), model="dis_img")
    assert len(zs) == 4 and all(torch.equal(z, zs[1]) for z in zs[1:]) and not torch.equal(zs[0], zs[1])
    assert torch.equal(torch.cuda.get_rng_state(), want_step)


# ---------------------------------------------------------------------------------------------------------------
# drop-in behaviour
def test_state_dict_round_trip_and_pack_invalidation():
    w, seed = 8, 3
    Gn, Dn = _product_a(w, seed)
    rG, rD = R.Generator(1, R.A_NZ, w), R.Discriminator(1, w)
    rG.load_state_dict(Gn.state_dict()), rD.load_state_dict(Dn.state_dict())           # strict: the keys are the stock classes'
    for mine, ref in ((Gn, rG), (Dn, rD)):
        assert list(mine.state_dict()) == list(ref.state_dict())
        assert all(torch.equal(v.cpu(), ref.state_dict()[k]) for k, v in mine.state_dict().items())
    z = torch.randn(3, R.A_NZ, 1, 1, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        first = (Gn(z).clone(), Dn(Gn(z)).clone())
    # other weights through load_state_dict (from the stock classes): the next forward runs on them
    gsd, dsd = R.a_weights(w, seed + 1)
    rG.load_state_dict(gsd), rD.load_state_dict(dsd)
    Gn.load_state_dict(rG.state_dict()), Dn.load_state_dict(rD.state_dict())
    fresh = _product_a(w, seed + 1)
    with torch.no_grad():
        second = (Gn(z).clone(), Dn(Gn(z)).clone())
        want = (fresh[0](z), fresh[1](fresh[0](z)))
    assert all(torch.equal(a, b) for a, b in zip(second, want)) and not torch.equal(first[0], second[0])
    assert not torch.equal(first[1], second[1])
    # a fused trainer step writes through raw pointers and bumps _gode_ver: the next forward runs on the new weights
    tr, _ = _trainer(Gn, Dn, "euler", 0.0)
    R.seed_all(seed)
    tr.step(R.real_batch(seed), model="dis_img")
    tr.step(model="gen")
    fresh = (dcgan.Generator(1, nz=R.A_NZ, ngf=w).cuda(), dcgan.Discriminator(1, ndf=w).cuda())
    fresh[0].load_state_dict(Gn.state_dict()), fresh[1].load_state_dict(Dn.state_dict())
    with torch.no_grad():
        third = (Gn(z).clone(), Dn(Gn(z)).clone())
        want = (fresh[0](z), fresh[1](fresh[0](z)))
    assert all(torch.equal(a, b) for a, b in zip(third, want))
    assert not torch.equal(third[0], second[0]) and not torch.equal(third[1], second[1])
    # stock nn.BCEWithLogitsLoss on the new modules: regular CUDA tensors with a grad_fn
    out = Dn(Gn(z))
    assert out.grad_fn is not None and tuple(out.shape) == (3,)
    loss = torch.nn.BCEWithLogitsLoss()(out, torch.ones(3, device="cuda"))
    grads = torch.autograd.grad(loss, list(Gn.parameters()) + list(Dn.parameters()))
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    # eval mode leaves the running statistics alone, train mode counts its batches
    nbt = int(Gn.main[1].num_batches_tracked)
    Gn.eval()
    with torch.no_grad():
        Gn(z)
    assert int(Gn.main[1].num_batches_tracked) == nbt
    Gn.train()
    with torch.no_grad():
        Gn(z)
    assert int(Gn.main[1].num_batches_tracked) == nbt + 1


def test_alternating_batch_sizes_give_the_results_of_fresh_modules():
    """The CIFAR loader's last batch has 16 images: B = 64, 16, 64 on one pair of modules (a plan per batch size; at full width
    the head changes kernel family with B) against fresh modules per batch."""
    Gn, Dn = R.f_load(dcgan.Generator(1), dcgan.Discriminator(1))
    Gn, Dn = Gn.cuda(), Dn.cuda()
    crit = dcgan.BCEWithLogitsLoss()
    for i, B in enumerate((64, 16, 64)):
        z = torch.randn(B, R.NZ, 1, 1, generator=torch.Generator().manual_seed(40 + i)).cuda()
        fG, fD = R.f_load(dcgan.Generator(1), dcgan.Discriminator(1))
        fG, fD = fG.cuda(), fD.cuda()
        res = []
        for gn, dn in ((Gn, Dn), (fG, fD)):
            fake = gn(z)
            out = dn(fake)
            grads = torch.autograd.grad(crit(out, torch.ones(B, device="cuda")), list(gn.parameters()) + list(dn.parameters()))
            res.append([fake.detach(), out.detach()] + list(grads))
        assert tuple(res[0][0].shape) == (B, 3, 32, 32) and tuple(res[0][1].shape) == (B,)
        for k, (a, b) in enumerate(zip(*res)):
            assert torch.equal(a, b), (B, k)
