"""Stage-1 block on the MI355X: GResBlock / ConditionalNorm / SpectralNorm on the HIP kernels against the fixtures of the
reference's own GResBlock (scripts/make_gres_golden.py), and every new op alone against tests/gres_ref.py.

conv0's bias gradient in the bn cases: see tests/test_host_gres.py (zero in exact arithmetic; held to GTOL times the natural
scale of the sum instead of a relative error against the reference's rounding noise)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gres_ref
from conftest import golden, rel_err, seed_all
from gres_cases import CASES
from test_host_gres import grad_err, hip_block, load_sd0

pytestmark = pytest.mark.gpu
TOL, GTOL = 1e-4, 5e-4
_RUNS = {}


def run_case(name, x_layout="contiguous"):
    """The fixtures' recipe on the GPU: train forward, backward, train forward, state, eval forward."""
    case, g = CASES[name], golden(f"gres_tiny_{name}.npz")
    blk = load_sd0(hip_block(case), g).cuda()
    x0 = torch.from_numpy(g["x"]).cuda()
    if x_layout == "channels_last":
        x0 = x0.contiguous(memory_format=torch.channels_last)
    elif x_layout == "slice":
        big = torch.zeros(x0.shape[0], x0.shape[1] + 2, x0.shape[2] + 1, x0.shape[3] + 3, device="cuda")
        big[:, 1:-1, 1:, 2:-1] = x0
        x0 = big[:, 1:-1, 1:, 2:-1]
        assert not x0.is_contiguous()
    x = x0.detach().requires_grad_(True)
    cond = torch.from_numpy(g["condition"]).cuda().requires_grad_(True)
    y1 = blk(x, cond)
    y1.backward(torch.from_numpy(g["gy"]).cuda())
    out = {"y1": y1.detach().cpu(), "g/x": x.grad.cpu(), "g/condition": None if cond.grad is None else cond.grad.cpu()}
    for k, p in blk.named_parameters():
        out[f"g/{k}"] = None if p.grad is None else p.grad.cpu()
    out["y2"] = blk(x.detach(), cond.detach()).detach().cpu()
    for k, v in blk.state_dict().items():
        out[f"sd2/{k}"] = v.cpu().clone()
    blk.eval()
    out["y_eval"] = blk(x.detach(), cond.detach()).detach().cpu()
    return out


def cached(name):
    if name not in _RUNS:
        _RUNS[name] = run_case(name)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_outputs(name):
    r, g = cached(name), golden(f"gres_tiny_{name}.npz")
    for k in ("y1", "y2", "y_eval"):
        err = rel_err(r[k], g[k])
        print(name, k, err)
        assert r[k].shape == g[k].shape and err < TOL, (k, err)


@pytest.mark.parametrize("name", list(CASES))
def test_state_after_two_forwards(name):
    r, g = cached(name), golden(f"gres_tiny_{name}.npz")
    for k in [k for k in g.files if k.startswith("sd2/")]:
        if k.endswith("num_batches_tracked"):
            assert int(r[k]) == int(g[k]), k
        elif k.endswith(("weight_u", "weight_v", "running_mean", "running_var")):
            err = rel_err(r[k], g[k])
            print(name, k, err)
            assert err < TOL, (k, err)
        else:
            assert np.array_equal(r[k].numpy(), g[f"sd0/{k[4:]}"]), k       # parameters are not touched by a forward


@pytest.mark.parametrize("name", list(CASES))
def test_gradients(name):
    case, r, g = CASES[name], cached(name), golden(f"gres_tiny_{name}.npz")
    for k in [k for k in r if k.startswith("g/")]:
        if k not in g.files:
            assert r[k] is None, k          # CBN parameters out of use (and u, v) receive no gradient
            continue
        # (conv0.module.bias in the bn cases goes through grad_err's absolute form, which the exact zeros the kernel returns
        # cannot fail: the real check of that tensor is test_op_cbn_apply_and_backward's dbias == 0 against autograd)
        err = grad_err(k[2:], r[k], g, case) if k not in ("g/x", "g/condition") else rel_err(r[k], g[k])
        print(name, k, err)
        assert err < GTOL, (k, err)
    assert all(k in r and r[k] is not None for k in g.files if k.startswith("g/"))


@pytest.mark.parametrize("name", list(CASES))
def test_rerun_is_bit_identical(name):
    a, b = cached(name), run_case(name)
    for k, v in a.items():
        assert (v is None and b[k] is None) or torch.equal(v, b[k]), k


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("layout", ["channels_last", "slice"])
def test_input_layouts_give_the_same_bits(name, layout):
    a, b = cached(name), run_case(name, layout)
    for k, v in a.items():
        assert (v is None and b[k] is None) or torch.equal(v, b[k]), k


def _grads(blk, x, cond, backward):
    blk.zero_grad(set_to_none=True)
    xr = x.detach().requires_grad_(True)
    cr = None if cond is None else cond.detach().requires_grad_(True)
    y = blk(xr, cr)
    backward(y)
    out = {"y": y.detach().clone(), "x": xr.grad.clone()}
    if cr is not None and cr.grad is not None:
        out["cond"] = cr.grad.clone()
    out.update({k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None})
    return out


@pytest.mark.parametrize("name", ["A", "D", "E"])
def test_expanded_gradient_and_input(name):
    """`.sum().backward()` hands the block a gradient expanded from ONE element (all strides zero), and x may be expanded
    too: both must behave as their dense copies, bit for bit (all-zero strides are the C ABI's sentinel for a dense
    channels-last tensor and must not be mistaken for it)."""
    case, g = CASES[name], golden(f"gres_tiny_{name}.npz")
    x = torch.from_numpy(g["x"]).cuda()
    cond = torch.from_numpy(g["condition"]).cuda() if case["bn"] and case["down"] == 1 else None

    def fresh():
        return load_sd0(hip_block(case), g).cuda()
    a = _grads(fresh(), x, cond, lambda y: y.sum().backward())
    b = _grads(fresh(), x, cond, lambda y: y.backward(torch.ones_like(y).contiguous()))
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ref = load_sd0(gres_ref.GResBlock(case["cin"], case["cout"], n_class=case["n_class"], bn=case["bn"],
                                      upsample_factor=case["up"], downsample_factor=case["down"]), g).cuda()
    r = _grads(ref, x, cond, lambda y: y.sum().backward())
    assert rel_err(a["conv1.module.bias"].cpu(), r["conv1.module.bias"].cpu()) < GTOL
    assert rel_err(a["x"].cpu(), r["x"].cpu()) < GTOL
    for xe in (x[:1, :1, :1, :1].expand(x.shape), x[:, :, :, :1].expand(x.shape)):
        assert 0 in xe.stride()
        c = _grads(fresh(), xe, cond, lambda y: y.sum().backward())
        d = _grads(fresh(), xe.contiguous(), cond, lambda y: y.sum().backward())
        for k in c:
            assert torch.equal(c[k], d[k]), k


# ---- each op alone ---------------------------------------------------------------------------------------------
def _L():
    from gan_ode_amd import _lib as L
    from gan_ode_amd.engine import stream_ptr
    return L, (lambda op: L.run_one(op, stream_ptr()))


def _nhwc(t):
    return (t.stride(0), t.stride(2), t.stride(3), t.stride(1))


def _setv(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = int(v)


@pytest.mark.parametrize("C_, layout, rows", [(3, "nchw", 3), (10, "nhwc", 5), (100, "nhwc", 2), (300, "nhwc", 1)])
def test_op_chstats(C_, layout, rows):
    L, run = _L()
    seed_all(1)
    x = torch.randn(3, C_, 7, 5, device="cuda") + 0.5
    if layout == "nhwc":
        x = x.contiguous(memory_format=torch.channels_last)
    stats = torch.full((2, C_, rows), float("nan"), device="cuda")
    op = L.ChstatsOp(x=x.data_ptr(), stats=stats.data_ptr(), N=3, H=7, W=5, C=C_, rows=rows)
    _setv(op.xs, _nhwc(x))
    run(op)
    s = stats.sum(2).cpu()
    assert rel_err(s[0], x.double().sum((0, 2, 3)).cpu()) < 1e-6
    assert rel_err(s[1], (x.double() ** 2).sum((0, 2, 3)).cpu()) < 1e-6


@pytest.mark.parametrize("C_", [3, 10])
def test_op_embed_and_backward(C_):
    L, run = _L()
    seed_all(2)
    N, K = 5, 6
    cond, W, b, dgb = (torch.randn(*s, device="cuda") for s in ((N, K), (2 * C_, K), (2 * C_,), (N, 2 * C_)))
    gb, dW, db, dc = (torch.empty(*s, device="cuda") for s in ((N, 2 * C_), (2 * C_, K), (2 * C_,), (N, K)))
    run(L.CbnEmbedOp(cond=cond.data_ptr(), W=W.data_ptr(), b=b.data_ptr(), gb=gb.data_ptr(), N=N, K=K, C2=2 * C_))
    run(L.CbnEmbedBwdOp(cond=cond.data_ptr(), W=W.data_ptr(), dgb=dgb.data_ptr(), dW=dW.data_ptr(), db=db.data_ptr(),
                        dcond=dc.data_ptr(), N=N, K=K, C2=2 * C_))
    c64, W64, g64 = cond.double(), W.double(), dgb.double()
    assert rel_err(gb.cpu(), (c64 @ W64.t() + b.double()).cpu()) < 1e-6
    assert rel_err(dW.cpu(), (g64.t() @ c64).cpu()) < 1e-6 and rel_err(db.cpu(), g64.sum(0).cpu()) < 1e-6
    assert rel_err(dc.cpu(), (g64 @ W64).cpu()) < 1e-6


@pytest.mark.parametrize("C_, f, bn, eval_mode", [(3, 2, True, False), (10, 1, True, False), (10, 2, True, True),
                                                  (3, 2, False, False), (10, 1, False, False)])
def test_op_cbn_apply_and_backward(C_, f, bn, eval_mode):
    """apply + backward against autograd through gres_ref.cbn on a strided NCHW source with a bias, in double."""
    L, run = _L()
    seed_all(3)
    N, H, W = 3, 7, 5
    lib = L.lib()
    big = torch.randn(N, C_ + 1, H, W + 2, device="cuda")
    x = big[:, 1:, :, 1:-1]
    bias = torch.randn(C_, device="cuda") * (0.0 if bn and not eval_mode else 1.0)
    gb = torch.randn(N, 2 * C_, device="cuda") if bn else None
    bnm = torch.nn.BatchNorm2d(C_, affine=False).double().cuda()
    bnm.running_mean.normal_(); bnm.running_var.uniform_(0.5, 2.0)
    bnm.train(not eval_mode)
    x64 = x.double().detach().requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    gb64 = gb.double().requires_grad_(True) if bn else None
    v = x64 + b64[None, :, None, None]
    if bn:
        if eval_mode:
            mean, var = bnm.running_mean.clone(), bnm.running_var.clone()
        else:
            mean, var = v.detach().mean((0, 2, 3)), v.detach().var((0, 2, 3), unbiased=False)
        z = gres_ref.cbn(v, gb64, bnm)
    else:
        z = v
    assert float((z.detach().abs().min())) > 1e-6
    a_ref = F.relu(z)
    if f == 2:
        a_ref = F.interpolate(a_ref, scale_factor=2)
    g_a = torch.randn(N, H * f, W * f, C_, device="cuda")
    gadd = torch.randn(N, H, W, C_, device="cuda")
    a_ref.backward(g_a.permute(0, 3, 1, 2).double())
    m32 = mean.float() if bn else None
    i32 = (1.0 / torch.sqrt(var + 1e-5)).float() if bn else None
    out = torch.empty(N, H * f, W * f, C_, device="cuda")
    op = L.CbnApplyOp(src=x.data_ptr(), bias=bias.data_ptr(), mean=None if not bn else m32.data_ptr(),
                      invstd=None if not bn else i32.data_ptr(), gb=None if not bn else gb.data_ptr(), out=out.data_ptr(),
                      N=N, H=H, W=W, C=C_, f=f, act=L.ACT_RELU)
    _setv(op.ss, _nhwc(x))
    run(op)
    assert rel_err(out.permute(0, 3, 1, 2).cpu(), a_ref.detach().cpu()) < 1e-6
    work = torch.empty(lib.gode_cbn_bwd_work_size(N, H, W, C_) // 2 + 1, dtype=torch.float64, device="cuda")
    dgb, dbias, gx = torch.empty(N, 2 * C_, device="cuda"), torch.empty(C_, device="cuda"), torch.empty(N, C_, H, W, device="cuda")
    op = L.CbnBwdOp(g_a=g_a.data_ptr(), a=out.data_ptr(), src=x.data_ptr(), bias=bias.data_ptr(),
                    mean=None if not bn else m32.data_ptr(), invstd=None if not bn else i32.data_ptr(),
                    gb=None if not bn else gb.data_ptr(), gadd=gadd.data_ptr(), work=work.data_ptr(),
                    dgb=dgb.data_ptr() if bn else None, dbias=dbias.data_ptr(), g_out=gx.data_ptr(), N=N, H=H, W=W, C=C_, f=f,
                    act=L.ACT_RELU, eval_mode=1 if eval_mode else 0)
    _setv(op.ss, _nhwc(x)); _setv(op.gos, _nhwc(gx))
    run(op)
    assert rel_err(gx.cpu(), (x64.grad + gadd.permute(0, 3, 1, 2).double()).cpu()) < 5e-6
    if bn:
        assert rel_err(dgb.cpu(), gb64.grad.cpu()) < 5e-6
    if bn and not eval_mode:
        assert float(dbias.abs().max()) == 0.0 and float(b64.grad.abs().max()) < 1e-9 * float(g_a.abs().sum())
    else:
        assert rel_err(dbias.cpu(), b64.grad.cpu()) < 5e-6


@pytest.mark.parametrize("C_, f, down, H, W", [(10, 2, 1, 5, 6), (3, 1, 1, 5, 6), (10, 1, 2, 7, 6), (40, 2, 1, 7, 5)])
def test_op_block_output_and_inverse(C_, f, down, H, W):
    L, run = _L()
    seed_all(4)
    N = 3
    lib = L.lib()
    main = torch.randn(N, C_, H * f, W * f, device="cuda", dtype=torch.float64).requires_grad_(True)
    sc = torch.randn(N, C_, H, W, device="cuda", dtype=torch.float64).requires_grad_(True)
    bm, bs = (torch.randn(C_, device="cuda", dtype=torch.float64).requires_grad_(True) for _ in range(2))
    y_ref = gres_ref.block_out(main, sc, bm, bs, f, down)
    gy = torch.randn(y_ref.shape, device="cuda")                       # NCHW: read through strides
    y_ref.backward(gy.double())
    m32, s32 = (t.detach().float().permute(0, 2, 3, 1).contiguous() for t in (main, sc))
    b1, b2 = bm.detach().float(), bs.detach().float()
    Ho, Wo = y_ref.shape[2:]
    y = torch.empty(N, Ho, Wo, C_, device="cuda")
    run(L.GresOutOp(main=m32.data_ptr(), sc=s32.data_ptr(), b_main=b1.data_ptr(), b_sc=b2.data_ptr(), y=y.data_ptr(), N=N, H=H,
                    W=W, C=C_, f=f, down=down))
    assert rel_err(y.permute(0, 3, 1, 2).cpu(), y_ref.detach().cpu()) < 1e-6
    g_sc = torch.empty(N, H, W, C_, device="cuda")
    g_main = torch.empty(N, H * f, W * f, C_, device="cuda") if down == 1 else None
    db = torch.empty(C_, device="cuda")
    work = torch.empty(lib.gode_gres_out_bwd_work_size(N, H, W, C_, f, down), device="cuda")
    op = L.GresOutBwdOp(g_y=gy.data_ptr(), g_sc=g_sc.data_ptr(), g_main=None if g_main is None else g_main.data_ptr(),
                        db=db.data_ptr(), work=work.data_ptr(), N=N, H=H, W=W, C=C_, f=f, down=down)
    _setv(op.gys, _nhwc(gy))
    run(op)
    assert rel_err(g_sc.permute(0, 3, 1, 2).cpu(), sc.grad.cpu()) < 1e-6
    assert rel_err((g_main if down == 1 else g_sc).permute(0, 3, 1, 2).cpu(), main.grad.cpu()) < 1e-6
    assert rel_err(db.cpu(), bm.grad.cpu()) < 1e-6 and rel_err(db.cpu(), bs.grad.cpu()) < 1e-6


@pytest.mark.parametrize("h, w", [(10, 27), (40, 360), (8, 8), (100, 900)])
def test_op_spectral_norm_forward_and_backward(h, w):
    L, run = _L()
    seed_all(5)
    wbar = torch.randn(h, w, device="cuda")
    u0, v0 = gres_ref.l2n(torch.randn(h, device="cuda")), gres_ref.l2n(torch.randn(w, device="cuda"))
    u, v = u0.clone(), v0.clone()
    wout, sigma, work = torch.empty(h, w, device="cuda"), torch.empty(1, device="cuda"), torch.empty(h + w, device="cuda")
    run(L.SnOp(wbar=wbar.data_ptr(), u=u.data_ptr(), v=v.data_ptr(), wout=wout.data_ptr(), sigma=sigma.data_ptr(),
               work=work.data_ptr(), h=h, w=w))
    ur, vr = u0.double(), v0.double()
    w_ref, s_ref = gres_ref.sn_step(wbar.double(), ur, vr)
    assert rel_err(v.cpu(), vr.cpu()) < 1e-6 and rel_err(u.cpu(), ur.cpu()) < 1e-6
    assert rel_err(sigma.cpu(), s_ref.reshape(1).cpu()) < 1e-6 and rel_err(wout.cpu(), w_ref.cpu()) < 1e-6
    G = torch.randn(h, w, device="cuda")
    dw = torch.empty(h, w, device="cuda")
    work2 = torch.empty(L.SN_BWD_BLOCKS, dtype=torch.float64, device="cuda")
    run(L.SnBwdOp(G=G.data_ptr(), wbar=wbar.data_ptr(), u=u.data_ptr(), v=v.data_ptr(), sigma=sigma.data_ptr(),
                  dwbar=dw.data_ptr(), work=work2.data_ptr(), h=h, w=w))
    wb = wbar.double().requires_grad_(True)
    (wb / ur.dot(wb.mv(vr)) * G.double()).sum().backward()        # autograd through sigma with u, v constant
    assert rel_err(dw.cpu(), wb.grad.cpu()) < 2e-6
    assert rel_err(dw.cpu(), gres_ref.sn_grad(G, wbar, u, v, sigma).cpu()) < 2e-6


def test_standalone_conditional_norm_and_spectral_norm():
    import gan_ode_amd as G
    seed_all(6)
    ref = gres_ref.ConditionalNorm(10, 6)
    mod = G.ConditionalNorm(10, 6)
    mod.load_state_dict(ref.state_dict())
    mod.cuda()
    x, cond, gy = torch.randn(3, 10, 7, 5), torch.rand(3, 6), torch.randn(3, 10, 7, 5)
    xr, cr = x.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    xg, cg = x.cuda().requires_grad_(True), cond.cuda().requires_grad_(True)
    yr = ref(xr, cr)
    yr.backward(gy)
    y = mod(xg, cg)
    y.backward(gy.cuda())
    assert rel_err(y.detach().cpu(), yr.detach()) < TOL
    assert rel_err(mod.bn.running_var.cpu(), ref.bn.running_var) < TOL and int(mod.bn.num_batches_tracked) == 1
    assert rel_err(xg.grad.cpu(), xr.grad) < GTOL and rel_err(cg.grad.cpu(), cr.grad) < GTOL
    assert rel_err(mod.embed.weight.grad.cpu(), ref.embed.weight.grad) < GTOL
    assert rel_err(mod.embed.bias.grad.cpu(), ref.embed.bias.grad) < GTOL
    seed_all(7)
    lin_r, lin_g = gres_ref.SpectralNorm(torch.nn.Linear(12, 9)), G.SpectralNorm(torch.nn.Linear(12, 9))
    lin_g.load_state_dict(lin_r.state_dict())
    lin_g.cuda()
    z = torch.randn(4, 12)
    for _ in range(2):                                               # u and v are carried
        yr, yg = lin_r(z), lin_g(z.cuda())
        assert rel_err(yg.detach().cpu(), yr.detach()) < TOL
    yr.square().sum().backward(); yg.square().sum().backward()
    assert rel_err(lin_g.module.weight_bar.grad.cpu(), lin_r.module.weight_bar.grad) < GTOL
    assert rel_err(lin_g.module.weight_u.cpu(), lin_r.module.weight_u.detach()) < TOL


def test_block_with_several_position_chunks():
    """gres_cells.BLOCK_CASE: the second norm's map is 18 x 16, so gode_cbn_bwd runs five position chunks and the statistics
    nine rows (the fixtures above stay within one chunk).  Against gres_ref.GResBlock in float64 on the device with the same
    state: forward, every gradient, the carried state and the eval forward.  tests/test_host_gres_cells.py holds the case's
    pre-activations away from the ReLU kink; nothing is excluded here."""
    from gres_cells import BLOCK_CASE as case, block_case_tensors
    sd, x, cond, gy = block_case_tensors()
    blk = hip_block(case)
    blk.load_state_dict(sd)
    blk.cuda()
    ref = gres_ref.GResBlock(case["cin"], case["cout"], n_class=case["n_class"], bn=case["bn"], upsample_factor=case["up"],
                             downsample_factor=case["down"]).double()
    ref.load_state_dict(sd)
    ref.cuda()
    a = _grads(blk, x.cuda(), cond.cuda(), lambda y: y.backward(gy.cuda()))
    r = _grads(ref, x.cuda().double(), cond.cuda().double(), lambda y: y.backward(gy.cuda().double()))
    assert a["y"].shape == r["y"].shape and rel_err(a["y"].cpu(), r["y"].cpu()) < TOL
    zero = "conv0.module.bias"          # in front of a train-mode BatchNorm: exact zeros here, rounding noise in the reference
    assert set(a) == set(r) and zero in a
    for k in a:
        if k == zero:
            assert float(a[k].abs().max()) == 0.0 and float(r[k].abs().max()) < 1e-9 * float(gy.abs().sum())
        elif k != "y":
            err = rel_err(a[k].cpu(), r[k].cpu())
            print("chunked block", k, err)
            assert err < GTOL, (k, err)
    blk.eval(); ref.eval()
    with torch.no_grad():
        ye, yr = blk(x.cuda(), cond.cuda()), ref(x.cuda().double(), cond.cuda().double())
    assert rel_err(ye.cpu(), yr.cpu()) < TOL
    sa, sr = blk.state_dict(), ref.state_dict()
    assert list(sa) == list(sr)
    for k in sa:
        if k.endswith("num_batches_tracked"):
            assert int(sa[k]) == int(sr[k]) == 1, k
        elif k.endswith(("weight_u", "weight_v", "running_mean", "running_var")):
            err = rel_err(sa[k].cpu(), sr[k].cpu())
            print("chunked block", k, err)
            assert err < TOL, (k, err)
        else:
            assert torch.equal(sa[k].cpu(), sd[k]), k


def test_spectral_norm_two_power_iterations():
    import gan_ode_amd as G
    seed_all(8)
    lin = torch.nn.Linear(12, 9)
    wbar = lin.weight.data.clone()
    mod = G.SpectralNorm(lin, power_iterations=2).cuda()
    assert mod.power_iterations == 2
    ur, vr = mod.module.weight_u.detach().double().clone(), mod.module.weight_v.detach().double().clone()
    w = mod.normalized_weight()
    w64 = wbar.double().cuda()
    w_one, _ = gres_ref.sn_step(w64, ur, vr)
    w_ref, _ = gres_ref.sn_step(w64, ur, vr)
    assert rel_err(w_one.cpu(), w_ref.cpu()) > 10 * TOL             # one iteration is not two: the comparison can tell them apart
    assert rel_err(w.detach().cpu(), w_ref.cpu()) < TOL
    assert rel_err(mod.module.weight_u.detach().cpu(), ur.cpu()) < TOL and rel_err(mod.module.weight_v.detach().cpu(), vr.cpu()) < TOL
