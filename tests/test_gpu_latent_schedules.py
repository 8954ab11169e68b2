"""GPU: the SDE and CDE motion latents on step schedules in which one step carries several outputs (the rows of
tests/latent_sched_cases.py): gode_sde_fwd / gode_sde_bwd against the float64 restatement of tests/sde_ref.py on
sde_grid_arrays(T, dt) with dt up to the whole interval, gode_cde_fwd / gode_cde_bwd at loosened tolerances against the
float64 replay of tests/cde_ref.py on the schedule the kernel itself accepted.  Every multi-output row asserts on the
schedule it ran on that some step does carry several outputs.  The nearby edges ride along: T = 1 / S = 0, states NULL,
N = 1 / 16 / 17, zcols = 68, content NULL (SDE); T = 2 and 3, a content code at the kernel level (CDE).  Class level:
VideoGeneratorSDE at sde_dt = 0.2 and VideoGeneratorCDE at cde_rtol, cde_atol = 1e-1, 1e-2 against the restated oracles, and
the way back to the defaults bitwise equal to a fresh generator.

Measured on the MI355X (pytest -s prints every figure before it is asserted; DESIGN.md sections 8 and 9): SDE rows states and
outputs <= 3.7e-7, gradients <= 1.7e-6; CDE rows <= 3.8e-6 forward and <= 5.3e-6 gradients except five-per-step (1.21e-4,
5.48e-5, 1.86e-3: the bounds of that row are 4 x the error of the restatement run in fp32, see CDE_ROW_BOUNDS)."""
import pytest
import torch

import cde_ref as R
import latent_sched_cases as C
import test_gpu_cde as TC
import test_gpu_sde as TS
from cde_driver import KINK, NAMES, Solve, _guarded, _guards_intact, _params, _split
from conftest import golden, rel_err, seed_all
from sde_ref import _ops, _params as sde_params, _sched_dev, grads_of, restate
from test_gpu_cde import schedules  # noqa: F401  (the fixture that records every CDE solve's accepted schedule)

import gan_ode_amd as G
import gan_ode_amd._lib as L
from gan_ode_amd.modules import sde_grid_arrays

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # SDE: the bound of tests/test_gpu_sde.py
CDE_OUT, CDE_GRAD = 2e-5, 1e-4  # CDE: the bounds of tests/test_gpu_cde.py
# Rows whose steps are long enough that fp32 itself misses those bounds: 4 x the error of the restatement run in torch fp32 on
# the kernel's schedule against the same restatement in float64 (the 4: fast_tanh and the fma order differ from torch's fp32).
# five-per-step (steps up to 5.1 long, the last one extrapolating the spline to t = 16.9): fp32 replay outputs 3.55e-5,
# states 4.16e-5, gradients up to 2.70e-3 (b1); the kernel: 1.21e-4, 5.48e-5, up to 1.86e-3.  DESIGN.md section 9.
CDE_ROW_BOUNDS = {"five-per-step": (4 * 4.16e-5, 4 * 2.70e-3)}
# The class at rtol 1e-1: frames and decoder gradients hold the bounds of test_cde_generator_against_replayed_oracle (1e-4,
# 1e-3).  The eight latent tensors' gradients come through the fp32 decoder's gradient with respect to its input, which
# amplifies the latent's rounding (2e-6 of the latent at these steps, 4e-7 at the defaults) to 1e-3: the oracle with its latent
# replayed in torch fp32 (_RefCde32) differs from the float64 one by up to 1.28e-3 (f.2.bias), the kernel by 1.27e-3, tensor by
# tensor the same figures.  The same rule: 4 x the fp32 restatement's own error.
CDE_CLASS_LATENT_GRAD = 4 * 1.28e-3
GUARD = 64


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- SDE ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prenet", C.SDE_CASES)
def test_sde_rows_against_float64_restatement(name, prenet):
    row = C.SDE_BY_NAME[name]
    N, T, zc = row.N, row.T, row.zcols
    grid, x, content, sel, g = C.sde_inputs(row)
    S = grid["S"]
    per = C.sde_per_step(grid)
    assert S == row.S and (max(per) if per else 0) == row.per_step, (S, per)      # the row still reaches its schedule
    if row.per_step >= 2:
        emit = grid["emit_at"].tolist()
        assert any(emit[j] == emit[j + 1] for j in range(1, T - 1))
    if not row.content:
        content = None
    params = sde_params(prenet)
    P64 = [p.double().requires_grad_() for p in params]
    st_ref, out_ref = restate(P64, x.double(), grid, prenet)
    P = [p.cuda() for p in params]
    sd = _sched_dev(grid)
    xd, seld = x.cuda(), sel.cuda()
    cd = content.cuda() if content is not None else None
    npar = L.SDE_NPARAM if prenet else L.SDE_NPARAM - 2128
    work = torch.empty(L.lib().gode_sde_bwd_work_size(N), device="cuda")
    ar = torch.arange(N)
    for select in ((False, True) if row.sel else (False,)):
        rows = N if select else N * T
        zb, z = _guarded(rows * zc)
        sb, states = _guarded(N * (S + 1) * 16)
        fop, bop = _ops(P, prenet, N, T, sd, xd, cd, seld if select else None, z, states, zc)
        L.run_one(fop, stream())
        _guards_intact(zb)
        _guards_intact(sb)
        zz = z.cpu().view(rows, zc)
        e_st = rel_err(states.cpu().view(N, S + 1, 16), st_ref.detach())
        want = out_ref[ar, sel.long()] if select else out_ref
        e_z = rel_err(zz[:, :16].reshape(want.shape), want.detach())
        print(f"sde {name} prenet={prenet} select={select}: states {e_st:.2e} outputs {e_z:.2e}")
        assert e_st < TOL and e_z < TOL
        assert not torch.isnan(zz[:, :16]).any()
        if content is not None:
            cols = content if select else content[:, None, :].expand(N, T, 50).reshape(rows, 50)
            assert torch.equal(zz[:, 16:66], cols)                                  # bit-exact
            assert float(zz[:, 66:].abs().max()) == 0
        else:
            assert zc == 16
        # a second forward is bitwise the first; so is the z of a forward that stores no states (states NULL)
        zb2, z2 = _guarded(rows * zc)
        sb2, st2 = _guarded(N * (S + 1) * 16)
        fop2, _ = _ops(P, prenet, N, T, sd, xd, cd, seld if select else None, z2, st2, zc)
        L.run_one(fop2, stream())
        assert zb2.cpu().numpy().tobytes() == zb.cpu().numpy().tobytes()
        assert sb2.cpu().numpy().tobytes() == sb.cpu().numpy().tobytes()
        zb3, z3 = _guarded(rows * zc)
        fop3, _ = _ops(P, prenet, N, T, sd, xd, cd, seld if select else None, z3, None, zc)
        L.run_one(fop3, stream())
        assert zb3.cpu().numpy().tobytes() == zb.cpu().numpy().tobytes()
        # backward: gradients of sum(out * gup) wrt all 12 (8) tensors, into a buffer with NaN guards on both sides
        gup = torch.randn(want.shape, generator=g, dtype=torch.float64)
        ref = grads_of((want * gup).sum(), P64)
        gz = torch.zeros(rows, zc, device="cuda")
        gz[:, :16] = gup.float().reshape(rows, 16).cuda()
        bop.gz, bop.work = gz.data_ptr(), work.data_ptr()
        for acc in (0, 1):
            buf = torch.full((npar + 2 * GUARD,), float("nan"), device="cuda")
            base = torch.randn(npar, generator=g)
            if acc:
                buf[GUARD:GUARD + npar] = base.cuda()
            bop.grads, bop.accumulate = buf[GUARD:].data_ptr(), acc
            L.run_one(bop, stream())
            b = buf.cpu()
            assert torch.isnan(b[:GUARD]).all() and torch.isnan(b[GUARD + npar:]).all()
            got = b[GUARD:GUARD + npar] - (base if acc else 0)
            assert torch.isfinite(got).all()
            o, errs = 0, []
            for r, p in zip(ref, params):
                k = p.numel()
                if float(r.abs().max()) == 0:           # S = 0: nothing reaches the drift and diffusion nets
                    assert S == 0
                    if not acc:
                        assert float(got[o:o + k].abs().max()) == 0, (select, o)
                    else:
                        assert torch.equal(b[GUARD + o:GUARD + o + k], base[o:o + k]), (select, o)
                    errs.append(0.0)
                else:
                    errs.append(rel_err(got[o:o + k].view(p.shape), r))
                o += k
            assert o == npar
            print(f"sde {name} prenet={prenet} select={select} acc={acc}: gradients {max(errs):.2e}")
            assert max(errs) < TOL, (select, acc, errs)
            if S == 0 and not acc:                      # the drift and diffusion part of grads is exactly 0
                assert float(got[-1088:].abs().max()) == 0
            if not acc:
                first = b[GUARD:GUARD + npar].clone()
                L.run_one(bop, stream())                      # a second backward is bitwise the first
                assert torch.equal(buf.cpu()[GUARD:GUARD + npar], first)


# ---- CDE ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cde_params():
    return _params()


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", [r.name for r in C.CDE_ROWS])
def test_cde_rows_against_float64_replay(name, cde_params):
    row = C.CDE_BY_NAME[name]
    N, T, zc = row.N, row.T, row.zcols
    P32, P64 = cde_params
    x, content, gen = C.cde_inputs(row)
    OUT, GRAD = CDE_ROW_BOUNDS.get(name, (CDE_OUT, CDE_GRAD))
    kw = dict(rtol=row.rtol, atol=row.atol, content=content, zcols=zc)
    s = Solve(P32, x, T, **kw)
    assert s.acc > 0 and s.trials >= s.acc, (s.acc, s.trials)
    for b in (s.zb, s.sb, s.hb):
        _guards_intact(b)
    _guards_intact(s.cb, -7)
    st, sh = s.schedule()
    assert abs(float((st + sh)[-1]) - (T - 1)) < float(sh[-1]) + 1e-12 and float(st[0]) == 0.0
    assert float((st + sh)[-1]) >= T - 1
    assert torch.equal(st[1:], (st + sh)[:-1])
    per = C.cde_per_step(st, sh, T)
    print(f"cde {name}: {s.acc} accepted / {s.trials} trials, outputs per step {per}, ends at {float((st + sh)[-1]):.3f}")
    assert sum(per) == T - 1
    if row.multi:       # the row still reaches its schedule: some accepted step covers at least two output times
        assert C.cde_covers_two(st, sh) and max(per) >= 2, per
    print(f"cde {name}: schedule t0 {[float(v).hex() for v in st]} h {[float(v).hex() for v in sh]}")
    mg = {}
    outs, states, z0 = R.replay(P64, x, T, st, sh, margin=mg)
    # the restatement's own fp32 rounding on this schedule (torch fp32 on the CPU against float64): printed next to the
    # kernel's figures
    C32 = [p.detach().float().requires_grad_() for p in P64]
    o32, s32, _ = R.replay(C32, x, T, st, sh)
    print(f"cde {name}: fp32 replay outputs {rel_err(o32.detach(), outs.detach()):.2e} "
          f"states {rel_err(s32.detach(), states.detach()):.2e}")
    zfull = s.z.cpu().view(N, T, zc)
    z = zfull[:, :, :16]
    got_states = s.states.cpu().view(N, s.S_cap + 1, 16)
    e_z, e_st = rel_err(z, outs.detach()), rel_err(got_states[:, :s.acc + 1], states.detach())
    print(f"cde {name}: outputs {e_z:.2e} states {e_st:.2e} z0 {rel_err(z[:, 0], z0.detach()):.2e}")
    # (the figures are all printed before the first of them is asserted, at the end)
    checks = [("outputs", e_z, OUT), ("states", e_st, OUT), ("z0", rel_err(z[:, 0], z0.detach()), CDE_OUT)]
    assert torch.isnan(got_states[:, s.acc + 1:]).all()         # nothing past the accepted steps

    sel = torch.randint(0, T, (N,), generator=gen)
    s2 = Solve(P32, x, T, sel=sel, **kw)
    assert (s2.acc, s2.trials) == (s.acc, s.trials)
    assert torch.equal(s2.sched.cpu()[:s.acc], s.sched.cpu()[:s.acc])
    _guards_intact(s2.zb)
    z2full = s2.z.cpu().view(N, zc)
    assert torch.equal(z2full[:, :16], z[torch.arange(N), sel])
    if content is not None:
        # content columns bit-exact in every emitted row of both layouts, zeros behind them, and the motion columns
        # bitwise those of the same solve without a content code
        assert torch.equal(zfull[:, :, 16:66], content[:, None, :].expand(N, T, 50))
        assert torch.equal(z2full[:, 16:66], content)
        assert float(zfull[:, :, 66:].abs().max()) == 0 and float(z2full[:, 66:].abs().max()) == 0
        plain = Solve(P32, x, T, rtol=row.rtol, atol=row.atol)
        assert (plain.acc, plain.trials) == (s.acc, s.trials) and _bytes(plain.hb) == _bytes(s.hb)
        assert torch.equal(plain.z.cpu().view(N, T, 16), z) and _bytes(plain.sb) == _bytes(s.sb)
        plain2 = Solve(P32, x, T, sel=sel, rtol=row.rtol, atol=row.atol)
        assert torch.equal(plain2.z.cpu().view(N, 16), z2full[:, :16])

    # backward: all rows, then sel_t rows; accumulate 0 and 1, under the ReLU-kink mask of tests/test_gpu_cde.py
    keep = (mg["relu"] > KINK).to(torch.float32)[:, None, None]
    assert float(keep.mean()) > 0.5, float(keep.mean())
    gz = torch.randn(N, T, 16, generator=gen) * keep
    ref = torch.autograd.grad((outs * gz.double()).sum(), P64, retain_graph=True)
    r32 = torch.autograd.grad((o32 * gz).sum(), C32, retain_graph=True)
    print(f"cde {name}: fp32 replay gradients (all rows) " + " ".join(f"{n} {rel_err(a, b):.2e}" for n, a, b in zip(NAMES, r32, ref)))
    g, gb = s.backward(gz.view(N * T, 16))
    _guards_intact(gb)
    errs = [rel_err(a, b) for a, b in zip(_split(g), ref)]
    print(f"cde {name}: gradients (all rows) " + " ".join(f"{n} {v:.2e}" for n, v in zip(NAMES, errs)))
    checks += [(f"gradient {n} (all rows)", v, GRAD) for n, v in zip(NAMES, errs)]
    g2, _ = s.backward(gz.view(N * T, 16))
    assert torch.equal(g, g2)                                      # re-runs are bitwise equal
    init = torch.randn(L.CDE_NPARAM, generator=gen)
    g3, gb3 = s.backward(gz.view(N * T, 16), accumulate=1, init=init)
    _guards_intact(gb3)
    checks.append(("accumulate (all rows)", rel_err(g3 - init, g), 1e-5))

    gzs = torch.randn(N, 16, generator=gen) * keep[:, 0]
    full = torch.zeros(N, T, 16, dtype=torch.float64)
    full[torch.arange(N), sel] = gzs.double()
    ref = torch.autograd.grad((outs * full).sum(), P64)
    r32 = torch.autograd.grad((o32 * full.float()).sum(), C32)
    print(f"cde {name}: fp32 replay gradients (sel_t) " + " ".join(f"{n} {rel_err(a, b):.2e}" for n, a, b in zip(NAMES, r32, ref)))
    g, gb = s2.backward(gzs)
    _guards_intact(gb)
    errs = [rel_err(a, b) for a, b in zip(_split(g), ref)]
    print(f"cde {name}: gradients (sel_t) " + " ".join(f"{n} {v:.2e}" for n, v in zip(NAMES, errs)))
    checks += [(f"gradient {n} (sel_t)", v, GRAD) for n, v in zip(NAMES, errs)]
    g3, gb3 = s2.backward(gzs, accumulate=1, init=init)
    _guards_intact(gb3)
    checks.append(("accumulate (sel_t)", rel_err(g3 - init, g), 1e-5))

    s3 = Solve(P32, x, T, **kw)                                    # forward re-run: bitwise
    for u, v in ((s3.zb, s.zb), (s3.sb, s.sb), (s3.hb, s.hb), (s3.cb, s.cb)):
        assert _bytes(u) == _bytes(v)
    missed = [(label, v, bound) for label, v, bound in checks if not v <= bound]
    assert not missed, missed


# ---- class level ----------------------------------------------------------------------------------------------------
def _grads(gen):
    return [(k, p.grad.clone()) for k, p in gen.named_parameters() if p.grad is not None]


def _calls_with_gradients(gen, seed):
    """sample_videos(8), sample_z_m(3) and their gradients under fixed weights of the sum, from a clean .grad state"""
    for p in gen.parameters():
        p.grad = None
    seed_all(seed)
    vid, _ = gen.sample_videos(8)
    zm = gen.sample_z_m(3)
    wv = torch.linspace(-1, 1, vid.numel(), device="cuda").view(vid.shape)
    wz = torch.linspace(1, -1, zm.numel(), device="cuda").view(zm.shape)
    ((vid * wv).sum() + (zm * wz).sum()).backward()
    torch.cuda.synchronize()
    return vid.detach().clone(), zm.detach().clone(), _grads(gen)


def _assert_bitwise(a, b):
    (v0, z0, g0), (v1, z1, g1) = a, b
    assert torch.equal(v0, v1) and torch.equal(z0, z1)
    assert [k for k, _ in g0] == [k for k, _ in g1] and g0
    for (k, p), (_, q) in zip(g0, g1):
        assert torch.equal(p, q), k


def test_sde_generator_at_dt_02_and_back_to_the_default():
    gen, ref = TS._gen_pair(5)
    gen.sde_dt = 0.2
    ref.grid = sde_grid_arrays(16, 0.2)
    assert ref.grid["S"] == 5 and max(C.sde_per_step(ref.grid)) == 4
    seed_all(6)
    vid, _ = gen.sample_videos(8)
    img, _ = gen.sample_images(8)
    zm = gen.sample_z_m(3)
    seed_all(6)
    rvid, _ = ref.sample_videos(8)
    rimg, _ = ref.sample_images(8)
    rzm = ref.sample_z_m(3)
    assert vid.shape == (8, 1, 16, 28, 28) and img.shape == (8, 1, 28, 28) and zm.shape == (48, 16)
    errs = [rel_err(a.detach().cpu(), b.detach()) for a, b in ((vid, rvid), (img, rimg), (zm, rzm))]
    print("sde class dt=0.2: videos {:.2e} images {:.2e} z_m {:.2e}".format(*errs))
    assert max(errs) < TS.TOL
    wv = torch.randn(vid.shape, generator=torch.Generator().manual_seed(1))
    wi = torch.randn(img.shape, generator=torch.Generator().manual_seed(2))
    wz = torch.randn(zm.shape, generator=torch.Generator().manual_seed(3))
    ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum() + (zm * wz.cuda()).sum()).backward()
    ((rvid * wv).sum() + (rimg * wi).sum() + (rzm * wz).sum()).backward()
    worst = {}
    for (k, p), (_, q) in zip(gen.named_parameters(), ref.named_parameters()):
        if q.grad is None:
            assert p.grad is None, k          # the GRU cell is dead weight
            continue
        worst[k] = rel_err(p.grad.cpu(), q.grad)
    print(f"sde class dt=0.2: gradients {max(worst.values()):.2e}")
    assert all(v < 1e-3 for v in worst.values()), {k: v for k, v in worst.items() if not v < 1e-3}
    assert float(gen.ode_fn.diffusion_fn[0].weight.grad.abs().max()) > 0
    # back to the default dt on the same object: the plan pool and the grid cache are rebuilt
    gen.sde_dt = 2.5e-2
    fresh = G.VideoGeneratorSDE(1, 50, 0, 16, 16, ngf=8)
    fresh.load_state_dict(gen.state_dict())
    fresh.cuda()
    assert gen._steps(16) == 41
    _assert_bitwise(_calls_with_gradients(gen, 9), _calls_with_gradients(fresh, 9))


class _RefCde32(TC._RefCde):
    """_RefCde with the latent replayed in torch fp32: against _RefCde it measures what fp32 rounding of the latent alone does
    to the frames and gradients (the decoder is fp32 in both)."""

    def _P(self):
        fn = self.ode_fn
        return [self.f[0].weight, self.f[0].bias, self.f[2].weight, self.f[2].bias, fn.linear1.weight, fn.linear1.bias,
                fn.linear2.weight, fn.linear2.bias]


def test_cde_generator_at_loose_tolerances_and_back_to_the_defaults(schedules):  # noqa: F811
    ref_npz = golden("gen_cde_init.npz")
    assert int(ref_npz["ngf"]) == 8
    gen = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8)
    gen.load_state_dict({k[2:]: torch.from_numpy(ref_npz[k]) for k in ref_npz.files if k.startswith("w/")})
    ref = TC._RefCde(8, schedules)
    ref.load_state_dict(gen.state_dict())
    gen.cuda()
    gen.cde_rtol, gen.cde_atol = 1e-1, 1e-2
    seed_all(6)
    vid, _ = gen.sample_videos(32)
    img, _ = gen.sample_images(32)
    zm = gen.sample_z_m(3)
    assert len(schedules) == 3
    print("cde class: outputs per step " + " | ".join(str(C.cde_per_step(st, sh, 16)) for st, sh in schedules))
    assert any(C.cde_covers_two(st, sh) for st, sh in schedules)
    assert all(len(st) < 30 for st, _ in schedules)                 # (the defaults take 50 to 60 steps)
    ref32 = _RefCde32(8, list(schedules))
    ref32.load_state_dict(ref.state_dict())
    seed_all(6)
    rvid, _ = ref.sample_videos(32)
    rimg, _ = ref.sample_images(32)
    rzm = ref.sample_z_m(3)
    assert not schedules
    assert vid.shape == (32, 1, 16, 28, 28) and img.shape == (32, 1, 28, 28) and zm.shape == (48, 16)
    errs = [rel_err(a.detach().cpu(), b.detach()) for a, b in ((vid, rvid), (img, rimg), (zm, rzm))]
    print("cde class rtol=1e-1: videos {:.2e} images {:.2e} z_m {:.2e}".format(*errs))
    assert max(errs) < 1e-4
    wv = torch.randn(vid.shape, generator=torch.Generator().manual_seed(1))
    wi = torch.randn(img.shape, generator=torch.Generator().manual_seed(2))
    wz = torch.randn(zm.shape, generator=torch.Generator().manual_seed(3))
    ((vid * wv.cuda()).sum() + (img * wi.cuda()).sum() + (zm * wz.cuda()).sum()).backward()
    ((rvid * wv).sum() + (rimg * wi).sum() + (rzm * wz).sum()).backward()
    refp = dict(ref.named_parameters())
    worst = {}
    for k, p in gen.named_parameters():
        q = refp[k]
        if k.startswith(("recurrent.", "linear.")):
            assert p.grad is None and q.grad is None, k               # dead parameters
            continue
        worst[k] = rel_err(p.grad.cpu(), q.grad)
    print(f"cde class rtol=1e-1: gradients {max(worst.values()):.2e} " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    seed_all(6)
    fvid, _ = ref32.sample_videos(32)
    fimg, _ = ref32.sample_images(32)
    fzm = ref32.sample_z_m(3)
    ((fvid * wv).sum() + (fimg * wi).sum() + (fzm * wz).sum()).backward()
    f32p = dict(ref32.named_parameters())
    e32 = {k: rel_err(f32p[k].grad, q.grad) for k, q in refp.items() if q.grad is not None}
    print("cde class rtol=1e-1: fp32 replay videos {:.2e} images {:.2e} z_m {:.2e}".format(
        *[rel_err(a.detach(), b.detach()) for a, b in ((fvid, rvid), (fimg, rimg), (fzm, rzm))]))
    print(f"cde class rtol=1e-1: fp32 replay gradients {max(e32.values()):.2e} " + " ".join(f"{k} {v:.2e}" for k, v in e32.items()))
    bad = {k: v for k, v in worst.items() if not v < (CDE_CLASS_LATENT_GRAD if k.startswith(("f.", "ode_fn.")) else 1e-3)}
    assert not bad, bad
    assert float(gen.ode_fn.linear2.weight.grad.abs().max()) > 0
    # back to the defaults on the same object: the op key on (cde_rtol, cde_atol) rebuilds the op
    gen.cde_rtol, gen.cde_atol = 1e-4, 1e-6
    fresh = G.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=8)
    fresh.load_state_dict(gen.state_dict())
    fresh.cuda()
    a = _calls_with_gradients(gen, 9)
    back = [len(st) for st, _ in schedules]
    b = _calls_with_gradients(fresh, 9)
    assert len(schedules) == 4 and back == [len(st) for st, _ in schedules[2:]] and min(back) > 30, back
    _assert_bitwise(a, b)
