"""GPU: gan-ode_amd/csrc/gres.hip on every launch branch -- the rows of tests/gres_cells.py, one test per row;
tests/test_host_gres_cells.py shows on the CPU what the rows reach and that the references and bounds stand on their own.

Every output, and every work buffer, sits between 64 guard floats of a fixed bit pattern, which must survive; it starts as NaN and
lies one to three floats off a 16-byte boundary (work buffers that hold doubles: 8 bytes off).  Strided outputs are windows of
such a buffer: what lies around the window must still be NaN afterwards.  An output whose pointer the row leaves NULL is
allocated all the same and must stay NaN; gode_cbn_bwd without sums must not touch its work buffer.  Every element is held to
its own bound (gres_cells.py: counted roundings, not measured), outputs come back finite, a second run over fresh buffers gives
the same bits, and for the ops that read through strides (chstats, cbn_apply, cbn_bwd, gres_out_bwd) every source layout of a
row gives the same bits.  The references of the capped rows are computed on the device.

Worst |got - ref| / bound per op over all rows, as printed by test_worst_ratios_report on an MI355X (all 95 tests of this file and
the two new ones of tests/test_gpu_gres.py pass, 3.9 s together; the slowest row takes 0.4 s):
    chstats        stats 0.981
    cbn_embed      gb 0.252
    cbn_embed_bwd  dW 0.453, db 0.332, dcond 0.184
    cbn_apply      out 0.872
    cbn_bwd        g_out 0.980, dgb 0.811, dbias 0.296
    gres_out       y 0.947
    gres_out_bwd   g_sc 0.681, g_main 0.000 (a copy), db 0.650
    sn_fwd         v 0.526, u 0.070, sigma 0.041, wout 0.064
    sn_bwd         dwbar 0.859
These are within a few per cent of what the fp32 restatement of tests/test_host_gres_cells.py reaches on the CPU: the kernels
round where the restatement does.  The rows are sensitive where they claim to be: with the chunk loop of cbn_bwd_sample_kernel
cut one chunk short, and sn_bwd_kernel's re-addition of the partial dots cut at 63, exactly the rows with more than one position
chunk that take sums and the rows with 64 sn_dot blocks fail (a library built for that check only, not kept).
"""
import ctypes as C
import math

import pytest
import torch

import gan_ode_amd._lib as L
import gres_cells as T

pytestmark = pytest.mark.gpu

U, f64 = T.U, T.f64
NAN = float("nan")
WORST = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(op):
    rc = getattr(L.lib(), op.FN)(C.byref(op), _stream())
    torch.cuda.synchronize()
    assert rc == 0, (op.FN, rc)


class Guarded:
    """n floats, `off` floats past a 16-byte boundary, between GUARD floats of PATTERN on either side; NaN, or `fill`'s values."""

    def __init__(self, n, off=1, fill=None):
        self.n, self.lo = n, T.GUARD + off
        self.buf = torch.empty(2 * T.GUARD + n + 4, device="cuda")
        self.buf.view(torch.int32).fill_(T.PATTERN)
        self.data = self.buf[self.lo:self.lo + n]
        if fill is None:
            self.data.fill_(NAN)
        else:
            self.data.copy_(torch.as_tensor(fill).reshape(-1))
        assert self.data.data_ptr() % 16 == 4 * off

    def ptr(self):
        return self.data.data_ptr()

    def intact(self):
        g = self.buf.view(torch.int32)
        return bool((g[:self.lo] == T.PATTERN).all()) and bool((g[self.lo + self.n:] == T.PATTERN).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.data).all())

    def get(self, shape=None):
        assert self.intact()
        return self.data.clone().view(shape if shape is not None else (self.n,))


class GuardedWindow:
    """A strided [N, H, W, C] output: a window (gres_cells.window) of a guarded NaN buffer."""

    def __init__(self, shape, layout, off=1):
        bs = T.base_shape(shape, layout)
        self.g = Guarded(math.prod(bs), off)
        self.view = T.window(self.g.data.view(bs), layout)
        self.strides = T.op_strides(self.view, layout)

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        """The window's values; the rest of the buffer must still be NaN and the guards whole."""
        got = self.view.clone().contiguous()
        self.view.fill_(NAN)
        assert self.g.untouched()
        return got


def _dev(x):
    return {k: (v.cuda().contiguous() if v is not None else None) for k, v in x.items()}


def _ptrs(d):
    return {k: (v.data_ptr() if v is not None else None) for k, v in d.items()}


def _check(op_name, tag, key, got, ref, bound):
    """Every element of got within its bound of ref (compared where ref lives); records and returns the worst ratio."""
    assert bool(torch.isfinite(got).all()), (tag, key)
    got = got.to(ref.device)
    assert got.shape == ref.shape, (tag, key, got.shape, ref.shape)
    err = (got.to(f64) - ref).abs()
    worst = float((err / (bound + 1e-300)).max())
    WORST.setdefault(op_name, {})[key] = max(WORST.get(op_name, {}).get(key, 0.0), worst)
    assert bool((err <= bound).all()), (tag, key, worst)
    return worst


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------
# gode_chstats
def _ch_run(r, vals, layout):
    x, strides = T.place(vals, layout, "cuda")
    rows = T.ch_rows_of(r)
    stats = Guarded(2 * r.C * rows)
    _run(T.ch_op(r, x.data_ptr(), strides, stats.ptr()))
    return stats.get((2, r.C, rows))


@pytest.mark.parametrize("r", T.CH_ROWS, ids=[r.name for r in T.CH_ROWS])
def test_chstats_row(r):
    vals = T.ch_values(r.N, r.H, r.W, r.C)
    rows = T.ch_rows_of(r)
    ref, bound = T.ch_reference(T.effective(vals, r.layout), rows)
    got = _ch_run(r, vals, r.layout)
    print(f"{r.name}: worst |got - ref| / bound: {_check('chstats', r.name, 'stats', got, ref, bound):.3f}")
    if r.empty:
        assert bool((got[:, :, rows - r.empty:] == 0).all())              # empty workgroups write exact zeros
    assert _same_bits(got, _ch_run(r, vals, r.layout))


@pytest.mark.parametrize("C_", [1, 3, 100, 256, 257])
def test_chstats_layouts_give_the_same_bits(C_):
    """The order of every sum is the same for every memory layout: all layouts of the same values, bit for bit."""
    rows = [r for r in T.CH_ROWS if r.C == C_ and r.rows == "auto" and r.N == 2]
    assert {r.layout for r in rows} == set(T.LAYOUTS)
    vals = T.ch_values(rows[0].N, rows[0].H, rows[0].W, C_)
    got = {r.layout: _ch_run(r, vals, r.layout) for r in rows}
    for lay in T.LAYOUTS:
        if lay != "expand":
            assert _same_bits(got[lay], got["dense"]), lay
    dense = [r for r in rows if r.layout == "dense"][0]
    assert _same_bits(got["expand"], _ch_run(dense, T.effective(vals, "expand"), "dense"))
    assert not _same_bits(got["expand"], got["dense"])


# ---------------------------------------------------------------------------------------------------------------
# gode_cbn_embed / gode_cbn_embed_bwd
def _em_run(r, x):
    d = _dev(x)
    outs = dict(gb=Guarded(r.N * r.C2, 1), dW=Guarded(r.C2 * r.K, 1), db=Guarded(r.C2, 3), dcond=Guarded(r.N * r.K, 2))
    p = _ptrs(d)
    p.update({k: g.ptr() for k, g in outs.items()})
    fwd, bwd = T.em_ops(r, p)
    _run(fwd)
    _run(bwd)
    got = {}
    for k, g in outs.items():
        if k == r.null:
            assert g.untouched(), k
        else:
            got[k] = g.get()
    return got


@pytest.mark.parametrize("r", T.EM_ROWS, ids=[r.name for r in T.EM_ROWS])
def test_embed_row(r):
    x = T.em_inputs(r.N, r.K, r.C2)
    ref, bound = T.em_reference(r, x)
    got = _em_run(r, x)
    assert set(got) == set(ref) - {r.null}
    ratios = {k: _check("cbn_embed" if k == "gb" else "cbn_embed_bwd", r.name, k, v, ref[k].reshape(-1), bound[k].reshape(-1))
              for k, v in got.items()}
    print(f"{r.name}: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    again = _em_run(r, x)
    assert all(_same_bits(got[k], again[k]) for k in got)
    if r.null:                       # the other two are what they are with all three pointers
        full = _em_run(r._replace(null=None), x)
        assert all(_same_bits(got[k], full[k]) for k in got)


# ---------------------------------------------------------------------------------------------------------------
# gode_cbn_apply
def _ap_run(r, d, layout):
    src, strides = T.place(d["src"], layout, "cuda")
    out = Guarded(r.N * r.H * r.f * r.W * r.f * r.C)
    p = _ptrs(d)
    p.update(src=src.data_ptr(), out=out.ptr())
    _run(T.apply_op(r, p, strides))
    return out.get((r.N, r.H * r.f, r.W * r.f, r.C))


@pytest.mark.parametrize("r", T.AP_ROWS, ids=[r.name for r in T.AP_ROWS])
def test_apply_row(r):
    x = T.ap_inputs(r.name)
    d = _dev(x)
    ref, bound = T.apply_reference(d if r.strides_loop else x, r.C, r.f, r.act)
    layouts = T.SRC_LAYOUTS[:1] if r.strides_loop else T.SRC_LAYOUTS
    got = {lay: _ap_run(r, d, lay) for lay in layouts}
    print(f"{r.name}: worst |got - ref| / bound: {_check('cbn_apply', r.name, 'out', got['dense'], ref, bound):.3f}")
    assert all(_same_bits(got[lay], got["dense"]) for lay in layouts)
    assert _same_bits(got["dense"], _ap_run(r, d, "dense"))


# ---------------------------------------------------------------------------------------------------------------
# gode_cbn_bwd
def _bw_run(r, d, layout):
    lib = L.lib()
    shape = (r.N, r.H, r.W, r.C)
    src, ss = T.place(d["src"], layout, "cuda")
    g_out = GuardedWindow(shape, layout)
    ws = lib.gode_cbn_bwd_work_size(r.N, r.H, r.W, r.C)
    work, dgb, dbias = Guarded(ws, 2), Guarded(r.N * 2 * r.C, 1), Guarded(r.C, 3)
    assert work.ptr() % 8 == 0 and work.ptr() % 16 != 0
    p = _ptrs(d)
    p.update(src=src.data_ptr(), g_out=g_out.ptr(), work=work.ptr(), dgb=dgb.ptr(), dbias=dbias.ptr())
    _run(T.bw_op(r, p, ss, g_out.strides))
    got = dict(g_out=g_out.get())
    for k, g, on in (("dgb", dgb, r.dgb), ("dbias", dbias, r.dbias)):
        if on:
            got[k] = g.get((r.N, 2 * r.C) if k == "dgb" else None)
        else:
            assert g.untouched(), k
    assert work.intact()
    if r.mode == T.DIRECT_NOSUMS:
        assert work.untouched()
    for k in ("g_a", "a", "gadd"):          # the inputs are left alone
        assert d[k] is None or not bool(torch.isnan(d[k]).any())
    return got


@pytest.mark.parametrize("r", T.BW_ROWS, ids=[r.name for r in T.BW_ROWS])
def test_cbn_bwd_row(r):
    x = T.bw_inputs(r.name)
    d = _dev(x)
    ref = T.bw_reference(r, d if r.strides_loop else x)
    layouts = T.SRC_LAYOUTS[:1] if r.strides_loop else T.SRC_LAYOUTS
    got = {lay: _bw_run(r, d, lay) for lay in layouts}
    first = got["dense"]
    assert set(first) == {k for k in ref if not k.startswith("b_")}
    ratios = {k: _check("cbn_bwd", r.name, k, v, ref[k], ref["b_" + k]) for k, v in first.items()}
    print(f"{r.name}: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    if r.mode == T.TRAIN and r.dbias:
        assert bool((first["dbias"] == 0).all())
    for lay in layouts:
        assert all(_same_bits(got[lay][k], first[k]) for k in first), lay
    again = _bw_run(r, d, "dense")
    assert all(_same_bits(again[k], first[k]) for k in first)


# ---------------------------------------------------------------------------------------------------------------
# gode_gres_out / gode_gres_out_bwd
def _go_run(r, d, layout):
    lib = L.lib()
    Ho, Wo = T.out_dims(r.H, r.W, r.f, r.down)
    y = Guarded(r.N * Ho * Wo * r.C, 1)
    g_y, gys = T.place(d["g_y"], layout, "cuda")
    g_sc, g_main, db = Guarded(r.N * r.H * r.W * r.C, 1), Guarded(r.N * Ho * Wo * r.C, 3), Guarded(r.C, 1)
    work = Guarded(lib.gode_gres_out_bwd_work_size(r.N, r.H, r.W, r.C, r.f, r.down), 1)
    p = _ptrs(d)
    p.update(y=y.ptr(), g_y=g_y.data_ptr(), g_sc=g_sc.ptr(), g_main=g_main.ptr(), db=db.ptr(), work=work.ptr())
    fwd, bwd = T.go_ops(r, p, gys)
    _run(fwd)
    _run(bwd)
    got = dict(y=y.get((r.N, Ho, Wo, r.C)), g_sc=g_sc.get((r.N, r.H, r.W, r.C)))
    if r.g_main:
        got["g_main"] = g_main.get((r.N, Ho, Wo, r.C))
    else:
        assert g_main.untouched()
    if r.db:
        got["db"] = db.get()
        assert work.intact()
    else:
        assert db.untouched() and work.untouched()
    return got


@pytest.mark.parametrize("r", T.GO_ROWS, ids=[r.name for r in T.GO_ROWS])
def test_gres_out_row(r):
    x = T.go_inputs(r.name)
    d = _dev(x)
    src = d if r.strides_loop else x
    ref, bound = T.go_reference(r, src)
    bref = T.go_bwd_reference(r, src)
    layouts = T.SRC_LAYOUTS[:1] if r.strides_loop else T.SRC_LAYOUTS
    got = {lay: _go_run(r, d, lay) for lay in layouts}
    first = got["dense"]
    ratios = {"y": _check("gres_out", r.name, "y", first["y"], ref, bound)}
    assert set(first) - {"y"} == {k for k in bref if not k.startswith("b_")}
    for k in first:
        if k != "y":
            ratios[k] = _check("gres_out_bwd", r.name, k, first[k], bref[k], bref["b_" + k])
    print(f"{r.name}: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    if r.g_main:
        assert _same_bits(first["g_main"], d["g_y"])
    for lay in layouts:
        assert all(_same_bits(got[lay][k], first[k]) for k in first), lay
    again = _go_run(r, d, "dense")
    assert all(_same_bits(again[k], first[k]) for k in first)


# ---------------------------------------------------------------------------------------------------------------
# gode_sn_fwd / gode_sn_bwd
def _sn_run(r, x, b):
    d, db_ = _dev(x), _dev(b)
    outs = dict(u=Guarded(r.h, 1, x["u"]), v=Guarded(r.w, 3, x["v"]), wout=Guarded(r.h * r.w, 1), sigma=Guarded(1, 2),
                work=Guarded(r.h + r.w, 1), dwbar=Guarded(r.h * r.w, 3), work2=Guarded(2 * L.SN_BWD_BLOCKS, 2))
    assert outs["work2"].ptr() % 8 == 0
    p = {k: g.ptr() for k, g in outs.items()}
    p.update(wbar=d["wbar"].data_ptr(), G=d["G"].data_ptr(), u_in=db_["u"].data_ptr(), v_in=db_["v"].data_ptr(),
             sigma_in=db_["sigma"].data_ptr())
    fwd, bwd = T.sn_ops(r, p)
    _run(fwd)
    _run(bwd)
    assert outs["work"].intact() and outs["work2"].intact()
    assert torch.equal(db_["u"].cpu(), b["u"]) and torch.equal(db_["v"].cpu(), b["v"]) and torch.equal(d["wbar"].cpu(), x["wbar"])
    return dict(u=outs["u"].get(), v=outs["v"].get(), sigma=outs["sigma"].get(), wout=outs["wout"].get((r.h, r.w)),
                dwbar=outs["dwbar"].get((r.h, r.w)))


@pytest.mark.parametrize("r", T.SN_ROWS, ids=[r.name for r in T.SN_ROWS])
def test_sn_row(r):
    x = T.sn_inputs(r.name)
    b = T.sn_bwd_inputs(x)
    ref, bound = T.sn_fwd_reference(x)
    ref["dwbar"], bound["dwbar"] = T.sn_bwd_reference(b)
    got = _sn_run(r, x, b)
    ratios = {k: _check("sn_bwd" if k == "dwbar" else "sn_fwd", r.name, k, got[k], ref[k], bound[k]) for k in ref}
    print(f"{r.name}: worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    again = _sn_run(r, x, b)
    assert all(_same_bits(again[k], got[k]) for k in got)


def test_worst_ratios_report():
    """Runs last: the worst ratio of every op over the rows run in this session (the module docstring's table)."""
    for op_name in sorted(WORST):
        print(f"{op_name}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST[op_name].items())))
    assert all(v <= 1.0 for d in WORST.values() for v in d.values())
