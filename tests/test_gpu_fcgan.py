"""GPU: stage 2's fully-connected MNIST GAN on libgode -- the three passes of csrc/fc.hip through the C ABI against fp64
NumPy, the modules against the fp64 restatement of tests/fc_ref.py fed the same masks, GANODETrainer and the notebook's Adam
cell on the new modules.

Module and trainer allowances are the rule of DESIGN section 14: per tensor, conftest.rel_err against the fp64 restatement may be
8x the error of the fp32 CPU restatement against the fp64 one on the same inputs -- figures stored in
tests/golden/fcgan_own.npz (scripts/make_fcgan_goldens.py), because they depend on the host's BLAS and thread count: the
allowance must not change with the machine the suite runs on.  The op tests' bounds are counted roundings (U = 2^-24), written
where they are used.
"""
import numpy as np
import pytest
import torch

import fc_ref as R
import odegan_ref
from conftest import assert_weights_after_adam, rel_err

import gan_ode_amd as G
from gan_ode_amd import _lib as L
from gan_ode_amd import fcgan
from gan_ode_amd.engine import dptr, stream_ptr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
P = float(R.DROP_P)
ACTS = {"none": L.ACT_NONE, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH, "sigmoid": L.ACT_SIGMOID}
KEY = (0x5DEECE6 << 32) | 0x6D2B79F5          # both key words in use


def _act64(v, act):
    if act == "lrelu":
        return np.where(v > 0, v, 0.2 * v)
    if act == "tanh":
        return np.tanh(v)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    return v


def _dact64(a, act):
    if act == "lrelu":
        return np.where(a > 0, 1.0, 0.2)
    if act == "tanh":
        return 1.0 - a * a
    if act == "sigmoid":
        return a * (1.0 - a)
    return np.ones_like(a)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(op):
    L.run_one(op, stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("C_", [1, 4, 6, 1024])
@pytest.mark.parametrize("M", [1, 3, 130])
def test_fc_act_forward_and_backward_ops(M, C_):
    rng = np.random.RandomState(100 * M + C_)
    y = rng.randn(M, C_).astype(np.float32) * 1.5
    b = rng.randn(C_).astype(np.float32)
    g_out = rng.randn(M, C_).astype(np.float32)
    d0 = rng.randn(C_).astype(np.float32)
    keep = R.keep_mask(KEY, 1, M * C_).reshape(M, C_)
    yd, bd, gd = _dev(y), _dev(b), _dev(g_out)
    scale32 = float(np.float32(1.0) / (np.float32(1.0) - R.DROP_P))
    worst = {"fwd": 0.0, "g_y": 0.0, "db": 0.0}
    for act in ACTS:
        for bias in (True, False):
            for drop in (True, False):
                p = P if drop else 0.0
                v = y.astype(np.float64) + (b.astype(np.float64) if bias else 0.0)
                ref = _act64(v, act) * (keep * scale32 if drop else 1.0)
                outs = []
                for in_place in (False, True):
                    out = yd.clone() if in_place else torch.full((M, C_), float("nan"), device="cuda")
                    src = out if in_place else yd
                    _run(L.FcActOp(y=dptr(src), b=dptr(bd) if bias else None, out=dptr(out), M=M, C=C_, act=ACTS[act], key=KEY,
                                   layer=1, p=p))
                    outs.append(out.cpu().numpy())
                tag = (act, bias, drop)
                assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), tag     # in place == out of place
                got = outs[0]
                assert np.isfinite(got).all(), tag
                # roundings: y + b (1), the activation (tanhf / expf + add + divide: <= ~6 with the amplification |v| (1 - sigmoid)
                # <= ~5 of the sum's rounding at these inputs), the keep scale (2): 16 U of the value covers them
                err = np.abs(got - ref)
                assert (err <= 16 * U * np.abs(ref)).all(), (tag, float((err / (U * np.abs(ref) + 1e-300)).max()))
                worst["fwd"] = max(worst["fwd"], float((err / (U * np.abs(ref) + 1e-300)).max()))
                if drop:
                    assert (got[~keep] == 0).all() and (got[keep] != 0).all(), tag       # zeros exactly where the mask says
                # backward from the forward's own output
                a = got.astype(np.float64) * ((1.0 - P) if drop else 1.0)
                gref = g_out.astype(np.float64) * (keep * scale32 if drop else 1.0) * _dact64(a, act)
                od = _dev(got)
                work_n = L.lib().gode_fc_act_bwd_work_size(M, C_)
                assert work_n == (0 if M <= 128 else 2 * C_)
                work = torch.empty(max(work_n, 1), device="cuda")
                runs = []
                for alias in (False, True, True):
                    gy = gd.clone() if alias else torch.full((M, C_), float("nan"), device="cuda")
                    gin = gy if alias else gd
                    db = torch.full((C_,), float("nan"), device="cuda")
                    _run(L.FcActBwdOp(g_out=dptr(gin), out=dptr(od), g_y=dptr(gy), db=dptr(db), work=dptr(work), M=M, C=C_,
                                      act=ACTS[act], key=KEY, layer=1, p=p, accumulate=0))
                    runs.append((gy.cpu().numpy(), db.cpu().numpy()))
                for gy, db in runs[1:]:
                    assert np.array_equal(gy.view(np.uint32), runs[0][0].view(np.uint32)), tag
                    assert np.array_equal(db.view(np.uint32), runs[0][1].view(np.uint32)), (tag, "db differs between reruns")
                gy, db = runs[0]
                # act' has an absolute error of <= 3 U (1 - a^2 and a (1 - a) from a rounded a, |act'| <= 1), then three
                # products: 8 U of |g_out| / (1 - p)
                bound = 8 * U * np.abs(g_out.astype(np.float64)) * (scale32 if drop else 1.0)
                err = np.abs(gy - gref)
                assert (err <= bound + 1e-45).all(), (tag, float((err / (bound + 1e-300)).max()))
                worst["g_y"] = max(worst["g_y"], float((err / (bound + 1e-300)).max()))
                # the column sum of M fp32 terms in a fixed tree: (M + 8) U of sum |g_y|, plus the terms' own errors
                dbound = (M + 8) * U * np.abs(gref).sum(0) + bound.sum(0)
                derr = np.abs(db - gref.sum(0))
                assert (derr <= dbound + 1e-45).all(), (tag, float((derr / (dbound + 1e-300)).max()))
                worst["db"] = max(worst["db"], float((derr / (dbound + 1e-300)).max()))
                # accumulate adds the same sum to what db held, in one fp32 addition
                acc = _dev(d0)
                gy2 = torch.empty(M, C_, device="cuda")
                _run(L.FcActBwdOp(g_out=dptr(gd), out=dptr(od), g_y=dptr(gy2), db=dptr(acc), work=dptr(work), M=M, C=C_,
                                  act=ACTS[act], key=KEY, layer=1, p=p, accumulate=1))
                assert np.array_equal(acc.cpu().numpy().view(np.uint32), (d0 + db).astype(np.float32).view(np.uint32)), tag
    print(f"M={M} C={C_}: worst fwd {worst['fwd']:.2f} U (bound 16), g_y {worst['g_y']:.3f} and db {worst['db']:.3f} of their bounds")


@pytest.mark.parametrize("n,key,layer", [(1, 0, 0), (7, KEY, 2), (130 * 1024, KEY, 0), (100 * 1024 + 3, 2 ** 62 - 1, 255)])
def test_dropout_mask_equals_the_numpy_stream_bit_for_bit(n, key, layer):
    out = torch.full((n + 4,), float("nan"), device="cuda")
    L.check(L.lib().gode_dropout_mask(dptr(out), n, key, layer, P, stream_ptr()), "gode_dropout_mask")
    got = out.cpu().numpy()
    assert np.isnan(got[n:]).all(), "wrote past n"
    assert np.array_equal(got[:n], R.keep_mask(key, layer, n).astype(np.float32))


def _bce_case(n):
    rng = np.random.RandomState(n)
    p = rng.uniform(0.001, 0.999, n).astype(np.float32)
    t = (rng.rand(n) > 0.5).astype(np.float32)
    if n >= 8:
        p[:8] = [0, 0, 1, 1, 1e-30, 1 - 2.0 ** -24, 0.5, 2.0 ** -24]
        t[:8] = [0, 1, 0, 1, 1, 0, 0.25, 0.75]           # soft targets too
    return p, t


@pytest.mark.parametrize("n,edge", [(1, None), (1, (0.0, 1.0)), (1, (1.0, 0.0)), (1, (0.0, 0.0)), (100, None), (257, None)])
def test_bce_prob_against_torch(n, edge):
    p, t = _bce_case(n)
    if edge is not None:
        p[0], t[0] = edge
    pt = torch.from_numpy(p).requires_grad_(True)
    want = torch.nn.BCELoss()(pt, torch.from_numpy(t))
    want.backward()
    wl, wg = float(want.detach()), pt.grad.numpy()
    pd, td = _dev(p), _dev(t)
    runs = []
    for _ in range(3):
        loss, grad = torch.full((1,), float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        _run(L.BceProbOp(p=dptr(pd), t=dptr(td), grad=dptr(grad), loss=dptr(loss), n=n, gscale=1.0, accumulate=0))
        runs.append((loss.cpu().numpy(), grad.cpu().numpy()))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for r in runs[1:] for a, b in zip(r, runs[0])), "reruns differ"
    gl, gg = float(runs[0][0][0]), runs[0][1]
    assert np.isfinite(gl) and np.isfinite(gg).all()
    # every term is >= 0 (no cancellation): logf / log1pf within a few U, the double sum exact to fp32, torch's own fp32 sum
    # within n U -- 16 U of the loss, and 8 U per gradient element (a subtraction, a product, a clamp, two divisions)
    print(f"n={n} edge={edge}: loss {gl:.9g} torch {wl:.9g}, |diff| / U / loss {abs(gl - wl) / (U * max(abs(wl), 1e-30)):.2f}")
    assert abs(gl - wl) <= (16 + n / 16) * U * abs(wl)
    assert (np.abs(gg - wg) <= 8 * U * np.abs(wg)).all(), float((np.abs(gg - wg) / (U * np.abs(wg) + 1e-300)).max())
    # accumulate and gscale
    loss = torch.full((1,), 2.5, device="cuda")
    grad = torch.empty(n, device="cuda")
    _run(L.BceProbOp(p=dptr(pd), t=dptr(td), grad=dptr(grad), loss=dptr(loss), n=n, gscale=-2.0, accumulate=1))
    assert float(loss[0]) == float(np.float32(2.5) + np.float32(gl))
    assert (np.abs(grad.cpu().numpy() + 2.0 * gg) <= 2 * U * np.abs(2.0 * gg)).all()


def test_bce_module_matches_stock_bceloss_on_the_device():
    p, t = _bce_case(100)
    for shape in ((100, 1), (100,)):
        pd = _dev(p.reshape(shape)).requires_grad_(True)
        td = _dev(t.reshape(shape))
        mine = fcgan.BCELoss()(pd, td)
        (3.0 * mine).backward()
        pc = torch.from_numpy(p.reshape(shape)).requires_grad_(True)
        want = torch.nn.BCELoss()(pc, torch.from_numpy(t.reshape(shape)))
        (3.0 * want).backward()
        assert mine.shape == () and abs(float(mine.detach()) - float(want.detach())) <= 24 * U * float(want.detach())
        assert pd.grad.shape == shape and (np.abs(pd.grad.cpu().numpy() - pc.grad.numpy()) <= 10 * U * np.abs(pc.grad.numpy())).all()
    with pytest.raises(ValueError):
        fcgan.BCELoss()(_dev(p.reshape(100, 1)), _dev(t))


# ---------------------------------------------------------------------------------------------------------------
def _product(seed):
    Gn, Dn = R.load_product(fcgan.Generator(R.Z_DIM, R.MNIST_DIM), fcgan.Discriminator(R.MNIST_DIM), seed)
    return Gn.cuda(), Dn.cuda()


def _check(tag, got, ref64, prefix):
    """the 8x rule, per tensor; prints the ratios"""
    bad = {}
    for n in ref64:
        err, own = rel_err(got[n], ref64[n]), R.stored_own()[f"{prefix}/{n}"]
        print(f"{tag} {n}: err {err:.3e}, fp32 CPU restatement {own:.3e}, ratio {err / max(own, 1e-300):.2f}")
        if not err <= 8 * own:
            bad[n] = (err, own)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("B", R.MODULE_B)
@pytest.mark.parametrize("tag", ["G", "D"])
def test_module_forward_and_gradients_against_the_restatement(tag, B):
    ref64 = R.module_reference(tag, B)[0]
    seed = R.MODULE_SEED[tag, B]
    net = _product(seed)[0 if tag == "G" else 1]
    x, r = R.module_inputs(tag, B, seed)
    got = R.run_module(net, tag, x, r, seed)
    assert set(got) == set(ref64)
    _check(f"{tag} B={B}", got, ref64, f"module/{tag}/{B}")


def test_discriminator_drops_in_eval_mode_and_follows_the_cpu_generator():
    _, D = _product(1)
    D.eval()
    x = (torch.rand(3, R.MNIST_DIM, generator=torch.Generator().manual_seed(3)) * 2 - 1).cuda()
    torch.manual_seed(21)
    state = torch.get_rng_state()
    key = int(torch.randint(0, 2 ** 62, (1,)))
    torch.set_rng_state(state)
    with torch.no_grad():
        a, b = D(x), D(x)
        torch.set_rng_state(state)
        c = D(x)
    assert not torch.equal(a, b), "two forwards used the same masks"
    assert torch.equal(a, c), "restoring the CPU generator did not reproduce the forward"
    # eval mode still drops: the forward equals the restatement WITH the masks of the drawn key, not the one without
    rD = R.restated(1, torch.float64)[1]
    torch.set_rng_state(state)
    with torch.no_grad():
        with_masks = rD(x.cpu().double())
    assert rD.keys == [key]
    rD.mask_fn = lambda key, layer, shape, dtype: torch.full(tuple(shape), 1.0 - P, dtype=dtype)       # identity "dropout"
    with torch.no_grad():
        without = rD(x.cpu().double())
    assert rel_err(a.cpu(), with_masks) < 1e-5 < rel_err(a.cpu(), without)


def _trainer(Gn, Dn, criterion, device, dtype, method, reg):
    d_loss, g_loss = R.closures(Gn, Dn, criterion, device, dtype)
    return G.GANODETrainer(Gn.parameters(), Dn.parameters(), None, g_loss, d_loss, None, lr=R.TRAINER_LR, reg=reg, method=method)


@pytest.mark.parametrize("method", ["euler", "rk2", "rk4"])
def test_trainer_steps_against_the_restatement(method):
    d64, g64 = R.trainer_reference(method)[0]
    seed = R.TRAINER_SEED[method]
    Gn, Dn = _product(seed)
    tr = _trainer(Gn, Dn, fcgan.BCELoss(), "cuda", torch.float32, method, 0.0)
    bD, bG = R._params(Dn), R._params(Gn)
    R.seed_all(seed)
    l1 = tr.step(R.real_batch(seed), model="dis_img")
    after_d = R._params(Gn)
    l2 = tr.step(model="gen")
    assert np.isfinite(float(l1.detach())) and np.isfinite(float(l2.detach()))
    assert all(torch.equal(after_d[n], bG[n]) for n in bG), "the discriminator's step moved the generator"
    _check(f"{method} dis_img delta", R._delta(Dn, bD), d64, f"step/{method}/D")
    _check(f"{method} gen delta", R._delta(Gn, bG), g64, f"step/{method}/G")


def test_penalty_against_the_central_difference_and_generators_restored():
    seed = R.PENALTY_SEED
    Gn, Dn = _product(seed)
    tr = _trainer(Gn, Dn, fcgan.BCELoss(), "cuda", torch.float32, "euler", 0.01)
    gp64, _, state, _ = R.penalty_reference(tr.fd_h)
    before = R._params(Gn)
    R.seed_all(seed)
    gp = tr.grad_penalty("dis_img")
    got_state = odegan_ref.rng_state()
    after = R._params(Gn)
    assert all(torch.equal(after[n], before[n]) for n in before), "generator not restored bitwise"
    assert torch.equal(got_state[0], state[0]) and all(np.array_equal(a, b) for a, b in zip(got_state[1], state[1]))
    got = {n: g.detach().cpu() for (n, _), g in zip(Dn.named_parameters(), gp)}
    _check("penalty", got, gp64, "penalty")
    # a whole penalised step leaves both host generators where the restatement's sequence does, and the generator as found
    want_state = R.penalised_step_rng(tr.fd_h)
    R.seed_all(seed)
    bD = R._params(Dn)
    loss = tr.step(R.real_batch(seed), model="dis_img")
    got_state = odegan_ref.rng_state()
    assert np.isfinite(float(loss.detach()))
    assert torch.equal(got_state[0], want_state[0]) and all(np.array_equal(a, b) for a, b in zip(got_state[1], want_state[1]))
    after = R._params(Gn)
    assert all(torch.equal(after[n], before[n]) for n in before), "generator not restored bitwise by the penalised step"
    assert all(not torch.equal(p.detach().cpu(), bD[n]) for n, p in Dn.named_parameters())


def test_notebook_adam_iteration_against_the_restatement():
    res, _ = R.adam_reference()
    dl64, gl64, D64, G64 = res[torch.float64]
    Gn, Dn = _product(R.ADAM_SEED)
    R.seed_all(R.ADAM_SEED)
    dl, gl = R.adam_iteration(Gn, Dn, fcgan.BCELoss(), "cuda", torch.float32, R.real_batch(R.ADAM_SEED), lr=R.ADAM_LR)
    for name, got, w64 in (("D loss", dl, dl64), ("G loss", gl, gl64)):
        # the fp32 CPU restatement's own error, 8x as elsewhere, but not below 32 U of the value: a single number's fp32 error
        # can be zero by chance, and the device's expf / logf differ from the host's by a few U per sample
        allow = max(8 * R.stored_own()["adam/" + name.replace(" ", "_")], 32 * U * abs(w64))
        print(f"adam {name}: {got:.9g} vs {w64:.9g}, |diff| {abs(got - w64):.3e}, allowance {allow:.3e}")
        assert abs(got - w64) <= allow, name
    for net, ref in ((Dn, D64), (Gn, G64)):
        for n, p in net.named_parameters():
            assert_weights_after_adam(p, ref[n].float(), n)
    # stock nn.BCELoss on the discriminator's output still works: a regular CUDA tensor with a grad_fn
    out = Dn(torch.rand(4, R.MNIST_DIM, device="cuda"))
    assert out.grad_fn is not None
    loss = torch.nn.BCELoss()(out, torch.ones(4, 1, device="cuda"))
    grads = torch.autograd.grad(loss, list(Dn.parameters()))
    assert all(torch.isfinite(g).all() for g in grads)
