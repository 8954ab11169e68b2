"""GPU: gan-ode_amd/csrc/elementwise.hip on every launch branch -- the rows of tests/elementwise_cells.py, one test per row;
tests/test_host_elementwise_cells.py shows on the CPU what the rows reach and that the references and bounds stand on their own.

Every output, and the work buffer where there is one, sits between 64 guard floats of a fixed bit pattern, which must survive,
and starts as NaN; outputs come back finite; a second run over fresh buffers gives the same bits.

gode_col2im.  Reference: the fp32 overlap-add on the CPU in the kernels' tap order ((kd,) kh, kw ascending from 0.f; the kernels
only add, so the compiler's contraction has nothing to fuse).  Raw rows equal it bit for bit (torch.equal), whichever of the four
kernels runs -- which is also what the kernels' comments promise of one another; `pix-cols-off` and `pix-aniso-off` equal their
aligned twins (row-group kernel) bit for bit.  The kind and reason gode_col2im_launch_kind reports for the real op are the row's.
Tanh rows: |got - tanh64(s32)| against the float64 tanh of that exact fp32 sum.  The device's tanhf error is not documented, so
it was measured: over all tanh rows the worst error is TANH_WORST_U = 1.302 U (U = 2^-24; per row: rows-basic 1.172, pix-lds-over
1.302, pix-cols-off 1.172, fixed-p1 1.299, gen-k244 1.041); the assertion is twice that, the margin covering another libm build
(the inputs are fixed by their seeds).  rel_err < 1e-4 is kept beside it.

gode_bn_bwd, gode_bn_apply, gode_bn_finalize, Adam: float64 NumPy from the same fp32 inputs, per-element bounds derived in
elementwise_cells.py (counted roundings, not measured); the worst ratio of every row is printed.  Adam's bounds apply per step, from
the device's own state of the previous step; gode_adam_multi_dev fed FusedAdam.step_coefficients and gode_adam_noise_multi with
sigma = 0 (philox.h's normals are finite -- 23-bit uniforms strictly inside (0, 1) -- so noise_add adds +-0) give gode_adam_multi's
bits; nothing outside the tensors is written."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err

import gan_ode_amd as G
import gan_ode_amd._lib as L
import elementwise_cells as T

pytestmark = pytest.mark.gpu

U = T.U
TANH_WORST_U = 1.302          # measured (module docstring); asserted at twice this
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _placed(t, off=0):
    """t's values on the GPU, `off` floats past a 16-byte boundary."""
    t = torch.as_tensor(t)
    buf = torch.empty(t.numel() + 4, device="cuda", dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


class Guarded:
    """n floats on a 16-byte boundary between GUARD floats of PATTERN on either side; NaN, or `fill`'s values."""

    def __init__(self, n, fill=None):
        self.n = n
        self.buf = torch.empty(2 * T.GUARD + n, device="cuda")
        self.buf.view(torch.int32).fill_(T.PATTERN)
        self.data = self.buf[T.GUARD:T.GUARD + n]
        if fill is None:
            self.data.fill_(NAN)
        else:
            self.data.copy_(torch.as_tensor(fill).reshape(-1))
        assert self.data.data_ptr() % 16 == 0

    def ptr(self):
        return self.data.data_ptr()

    def intact(self):
        g = self.buf.view(torch.int32)
        return bool((g[:T.GUARD] == T.PATTERN).all()) and bool((g[T.GUARD + self.n:] == T.PATTERN).all())

    def cpu(self, shape=None):
        return self.data.cpu().view(shape if shape is not None else (self.n,))


def _worst(err, bound):
    return float((np.abs(err) / (bound + 1e-300)).max())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# gode_col2im
_C2_FIRST = {}


def _c2_run(r):
    cols = _placed(T.c2_cols(r.name), r.off)
    out = Guarded(T.c2_out_numel(r))
    op = T.c2_op(r, cols.data_ptr(), out.ptr())
    kind = T.c2_kind(op)
    rc = L.lib().gode_col2im(C.byref(op), _stream())
    torch.cuda.synchronize()
    assert out.intact()
    return rc, kind, out.cpu((r.N, *T.c2_out_dims(r), r.C))


def _c2_first(name):
    """The first run of the row (shared with the row's twin)."""
    if name not in _C2_FIRST:
        _C2_FIRST[name] = _c2_run(T.C2_BY_NAME[name])
    return _C2_FIRST[name]


@pytest.mark.parametrize("r", T.C2_ROWS, ids=[r.name for r in T.C2_ROWS])
def test_col2im_row(r):
    rc, kind, out = _c2_first(r.name)
    assert rc == 0 and kind == (r.kind, r.why)
    assert bool(torch.isfinite(out).all())
    s32 = T.c2_sum32(r.name)
    if r.tanh:
        want = torch.tanh(s32.double())
        worst = float((out.double() - want).abs().max()) / U
        print(f"{r.name}: {T.KINDS[r.kind]}: worst |got - tanh64(s32)| = {worst:.3f} U, rel_err = {rel_err(out, want):.2e}")
        assert worst <= 2 * TANH_WORST_U
        assert rel_err(out, want) < 1e-4
    else:
        print(f"{r.name}: {T.KINDS[r.kind]}: bit-identical to the fp32 overlap-add: {torch.equal(out, s32)}")
        assert torch.equal(out, s32)
    rc2, _, out2 = _c2_run(r)
    assert rc2 == 0 and _same_bits(out.numpy(), out2.numpy())
    if r.twin:        # the per-pixel kernel against the row-group kernel on the same values
        rct, kt, outt = _c2_first(r.twin)
        assert rct == 0 and kt == (T.ROWS_K, 0) and _same_bits(out.numpy(), outt.numpy())


# ---------------------------------------------------------------------------------------------------------------
# gode_bn_bwd
def _bnb_run(r, x):
    lib = L.lib()
    dev = {k: _placed(v) for k, v in x.items()}
    g = Guarded(r.M * r.C, fill=None if r.gin else x["g"])
    if not r.bn:
        op = L.BnBwdOp(g=g.ptr(), y=dev["y"].data_ptr(), M=r.M, C=r.C, act=r.act, gin=dev["g"].data_ptr() if r.gin else None)
        rc = lib.gode_bn_bwd(C.byref(op), _stream())
        torch.cuda.synchronize()
        assert g.intact()
        return rc, dict(g_y=g.cpu((r.M, r.C)).numpy())
    work = Guarded(lib.gode_bn_bwd_work_size(r.M, r.C))
    dgam = Guarded(r.C, fill=x["dgamma0"] if r.accumulate else None)
    dbet = Guarded(r.C, fill=x["dbeta0"] if r.accumulate else None)
    assert work.ptr() % 8 == 0
    op = L.BnBwdOp(g=g.ptr(), y=dev["y"].data_ptr(), M=r.M, C=r.C, act=r.act, gamma=dev["gamma"].data_ptr() if r.gamma else None,
                   mean=dev["mean"].data_ptr(), invstd=dev["invstd"].data_ptr(), scale=dev["scale"].data_ptr(),
                   shift=dev["shift"].data_ptr(), dgamma=dgam.ptr(), dbeta=dbet.ptr(), work=work.ptr(), accumulate=r.accumulate,
                   eval_mode=r.eval_mode, gin=dev["g"].data_ptr() if r.gin else None, groups=r.groups, M0=r.M0)
    rc = lib.gode_bn_bwd(C.byref(op), _stream())
    torch.cuda.synchronize()
    assert g.intact() and work.intact() and dgam.intact() and dbet.intact()
    if r.gin:
        assert torch.equal(dev["g"].cpu(), torch.from_numpy(x["g"]))          # the upstream gradient is left alone
    return rc, dict(g_y=g.cpu((r.M, r.C)).numpy(), dgamma=dgam.cpu().numpy(), dbeta=dbet.cpu().numpy())


@pytest.mark.parametrize("r", T.BNB_CASES, ids=[r.name for r in T.BNB_CASES])
def test_bn_bwd_row(r):
    x = T.bnb_inputs(r.name)
    ref = T.bnb_reference(r, x)
    rc, got = _bnb_run(r, x)
    assert rc == 0
    ratios = {}
    for k, v in got.items():
        assert np.isfinite(v).all(), k
        ratios[k] = _worst(v.astype(np.float64) - ref[k], ref["b_" + k])
    print(f"{r.name}: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in got.items():
        assert (np.abs(v.astype(np.float64) - ref[k]) <= ref["b_" + k] + 1e-45).all(), (k, ratios[k])
    rc2, again = _bnb_run(r, x)
    assert rc2 == 0 and all(_same_bits(got[k], again[k]) for k in got)


@pytest.mark.parametrize("M,C_,groups,M0,code", T.BNB_REFUSALS)
def test_bn_bwd_refusal_leaves_the_buffers_alone(M, C_, groups, M0, code):
    n = M * C_
    g, work = Guarded(n), Guarded(max(L.lib().gode_bn_bwd_work_size(M, C_), 1))
    y, vec = torch.zeros(n, device="cuda"), torch.ones(2 * C_ + 4, device="cuda")
    op = L.BnBwdOp(g=g.ptr(), y=y.data_ptr(), M=M, C=C_, act=T.RELU, gamma=vec.data_ptr(), mean=vec.data_ptr(), invstd=vec.data_ptr(),
                   scale=vec.data_ptr(), shift=vec.data_ptr(), dgamma=None, dbeta=None, work=work.ptr(), groups=groups, M0=M0)
    assert T.ERRORS[L.lib().gode_bn_bwd(C.byref(op), _stream())] == code
    torch.cuda.synchronize()
    assert g.intact() and work.intact() and bool(torch.isnan(g.data).all()) and bool(torch.isnan(work.data).all())


# ---------------------------------------------------------------------------------------------------------------
# gode_bn_apply, gode_bn_finalize
@pytest.mark.parametrize("r", T.BNA_CASES, ids=[r.name for r in T.BNA_CASES])
def test_bn_apply_row(r):
    x = T.bna_inputs(r.name)
    ref, bound = T.bna_reference(r, x)
    y, sc, sh = _placed(x["y"]), _placed(x["scale"]), _placed(x["shift"])
    runs = []
    for _ in range(2):
        out = Guarded(r.M * r.C)
        op = L.BnApplyOp(y=y.data_ptr(), out=out.ptr(), scale=sc.data_ptr() if r.affine else None,
                         shift=sh.data_ptr() if r.affine else None, M=r.M, C=r.C, act=r.act, M0=r.M0)
        assert L.lib().gode_bn_apply(C.byref(op), _stream()) == 0
        torch.cuda.synchronize()
        assert out.intact()
        runs.append(out.cpu((r.M, r.C)).numpy())
    got = runs[0]
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{r.name}: worst |got - ref| / bound: {_worst(err, bound):.3f}")
    assert (err <= bound).all(), _worst(err, bound)
    assert _same_bits(runs[0], runs[1])


def test_bn_finalize_row():
    x = T.bnf_inputs()
    ref, bound, var_raw = T.bnf_reference(x)
    assert var_raw[T.BNF_CONST] < 0
    Cc = T.BNF_C
    dev = {k: _placed(x[k]) for k in ("stats", "gamma", "beta")}
    runs = []
    for _ in range(2):
        outs = {k: Guarded(Cc) for k in ("mean", "invstd", "scale", "shift")}
        outs.update(running_mean=Guarded(Cc, fill=x["running_mean"]), running_var=Guarded(Cc, fill=x["running_var"]))
        nbt = torch.tensor([-7, 41, -7], dtype=torch.int64, device="cuda")
        op = L.BnFinalizeOp(stats=dev["stats"].data_ptr(), rows=T.BNF_ROWS, ncols=T.BNF_REPS * Cc, C=Cc, count=x["count"],
                            gamma=dev["gamma"].data_ptr(), beta=dev["beta"].data_ptr(), running_mean=outs["running_mean"].ptr(),
                            running_var=outs["running_var"].ptr(), num_batches_tracked=nbt[1:].data_ptr(), mean=outs["mean"].ptr(),
                            invstd=outs["invstd"].ptr(), scale=outs["scale"].ptr(), shift=outs["shift"].ptr(),
                            momentum=T.BNF_MOMENTUM, eps=T.BNF_EPS, training=1)
        assert L.lib().gode_bn_finalize(C.byref(op), _stream()) == 0
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs.values()) and nbt.tolist() == [-7, 42, -7]
        runs.append({k: o.cpu().numpy() for k, o in outs.items()})
    got = runs[0]
    ratios = {k: _worst(got[k].astype(np.float64) - ref[k], bound[k]) for k in ref}
    print("bn_finalize: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k in ref:
        assert np.isfinite(got[k]).all(), k
        assert (np.abs(got[k].astype(np.float64) - ref[k]) <= bound[k]).all(), (k, ratios[k])
        assert _same_bits(runs[0][k], runs[1][k])
    assert got["invstd"][T.BNF_CONST] == np.float32(1.0 / np.sqrt(T.BNF_EPS))       # the clamp: var = 0 exactly


# ---------------------------------------------------------------------------------------------------------------
# Adam
class _AdamState:
    """p, g, m, v of a list of tensors, each kind carved out of one NaN-filled buffer (T.guarded_layout)."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.offs, self.total = T.guarded_layout(self.sizes)
        p0, m0, v0, self.grads = T.adam_data(tuple(self.sizes))
        self.bufs = {k: torch.full((self.total,), NAN, device="cuda") for k in "pgmv"}
        for k, init in (("p", p0), ("m", m0), ("v", v0)):
            for o, t in zip(self.offs, init):
                self.bufs[k][o:o + t.numel()].copy_(t)
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for o, n in zip(self.offs, self.sizes):
            self.inside[o:o + n] = True
        for k, o in enumerate(self.offs):
            assert (self.bufs["p"].data_ptr() + 4 * o) % 16 == 4 * ((k + 1) % 2)

    def ptr(self, kind, k):
        return self.bufs[kind].data_ptr() + 4 * self.offs[k]

    def load_grads(self, step):
        for o, t in zip(self.offs, self.grads[step]):
            self.bufs["g"][o:o + t.numel()].copy_(t)

    def snapshot(self):
        """(p, m, v) on the CPU as whole buffers, after checking that nothing outside the tensors was written."""
        torch.cuda.synchronize()
        out = {k: self.bufs[k].cpu() for k in "pgmv"}
        for k, b in out.items():
            assert bool(torch.isnan(b[~self.inside]).all()), k
            assert k == "g" or bool(torch.isfinite(b[self.inside]).all()), k
        return out["p"].numpy(), out["m"].numpy(), out["v"].numpy()

    def tensors(self, snap, k):
        o, n = self.offs[k], self.sizes[k]
        return tuple(a[o:o + n] for a in snap)


def _adam_trajectory(variant, gscale, sizes=T.ADAM_SIZES):
    """ADAM_STEPS steps of one entry point; the (p, m, v) snapshots before the first step and after every step."""
    lib, hp = L.lib(), T.ADAM_HP
    st = _AdamState(sizes)
    n = len(st.sizes)
    rows = [[st.ptr(kind, k) for kind in "pgmv"] + [st.sizes[k]] for k in range(n)]
    if variant == "noise0":
        rows = [row + [off] for row, off in zip(rows, G.FusedAdam.noise_offsets([torch.empty(s) for s in st.sizes]))]
    table = torch.tensor(rows, dtype=torch.int64).cuda()
    snaps = [st.snapshot()]
    for s in range(T.ADAM_STEPS):
        st.load_grads(s)
        step = s + 1
        if variant == "multi":
            rc = lib.gode_adam_multi(table.data_ptr(), n, max(st.sizes), hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"],
                                     gscale, step, _stream())
        elif variant == "dev":
            coef = torch.tensor(G.FusedAdam.step_coefficients(hp["lr"], hp["beta1"], hp["beta2"], step), dtype=torch.float32).cuda()
            rc = lib.gode_adam_multi_dev(table.data_ptr(), n, max(st.sizes), hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"],
                                         gscale, coef.data_ptr(), _stream())
        elif variant == "noise0":
            rc = lib.gode_adam_noise_multi(table.data_ptr(), n, max(st.sizes), hp["lr"], hp["beta1"], hp["beta2"], hp["eps"],
                                           hp["weight_decay"], gscale, step, 1234, 1, step, 0.0, _stream())
        else:           # "l2": one gode_adam_l2 launch per tensor
            rc = 0
            for k in range(n):
                op = L.AdamOp(p=st.ptr("p", k), g=st.ptr("g", k), m=st.ptr("m", k), v=st.ptr("v", k), n=st.sizes[k], lr=hp["lr"],
                              beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"], weight_decay=hp["weight_decay"], gscale=gscale, step=step)
                rc = rc or lib.gode_adam_l2(C.byref(op), _stream())
        assert rc == 0
        snaps.append(st.snapshot())
    return st, snaps


def _adam_check_bounds(tag, st, snaps, gscale):
    worst = np.zeros(3)
    for s in range(T.ADAM_STEPS):
        for k in range(len(st.sizes)):
            p, m, v = st.tensors(snaps[s], k)
            ref, bnd = T.adam_reference(p, st.grads[s][k].numpy(), m, v, gscale, s + 1)
            got = st.tensors(snaps[s + 1], k)
            for i in range(3):
                err = np.abs(got[i].astype(np.float64) - ref[i])
                assert (err <= bnd[i]).all(), (tag, "step", s + 1, "tensor", k, "pmv"[i], _worst(err, bnd[i]))
                worst[i] = max(worst[i], _worst(err, bnd[i]))
    print(f"{tag} gscale {gscale}: worst |got - ref| / bound over {T.ADAM_STEPS} steps: p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")


def _same_trajectory(a, b):
    return all(_same_bits(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


@pytest.mark.parametrize("gscale", T.ADAM_GSCALES)
def test_adam_multi_against_float64(gscale):
    st, snaps = _adam_trajectory("multi", gscale)
    _adam_check_bounds("gode_adam_multi", st, snaps, gscale)


@pytest.mark.parametrize("gscale", T.ADAM_GSCALES)
def test_adam_multi_variants_bitwise(gscale):
    _, base = _adam_trajectory("multi", gscale)
    _, again = _adam_trajectory("multi", gscale)
    assert _same_trajectory(base, again)
    _, dev = _adam_trajectory("dev", gscale)
    assert _same_trajectory(base, dev)
    st, noise0 = _adam_trajectory("noise0", gscale)
    # (-0 and +0 compare equal: noise_add with sigma = 0 adds +-0, which can only turn a -0 parameter into +0)
    ins = st.inside.numpy()
    assert all(torch.equal(torch.from_numpy(x[ins]), torch.from_numpy(y[ins])) for sa, sb in zip(base, noise0) for x, y in zip(sa, sb))


@pytest.mark.parametrize("gscale", T.ADAM_GSCALES)
def test_adam_l2_against_float64(gscale):
    st, snaps = _adam_trajectory("l2", gscale, T.ADAM_L2_SIZES)
    _adam_check_bounds("gode_adam_l2", st, snaps, gscale)
    _, again = _adam_trajectory("l2", gscale, T.ADAM_L2_SIZES)
    assert _same_trajectory(snaps, again)
