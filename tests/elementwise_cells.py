"""The launch branches of gan-ode_amd/csrc/elementwise.hip as plain data: named rows for gode_col2im (its four kernels and the
reasons an op leaves the row-group / fixed kernel: gan-ode_amd/csrc/col2im_plan.h, reported by gode_col2im_launch_kind),
gode_bn_bwd, gode_bn_apply, gode_bn_finalize and the Adam entry points, each at the smallest shape that reaches its branch, with
the references and per-element bounds they are held to.  Shared by tests/test_host_elementwise_cells.py (every row reaches what
it names, the references and bounds stand on their own against fp32 restatements, the refusals) and
tests/test_gpu_elementwise_cells.py (every row on the GPU).

Left out: the grid-stride loop of the fixed 3-D col2im kernel (col2im3d_fixed_kernel) -- 16384 blocks of 256 voxels of the fixed
4x4x4 / C = 3 geometry need about 800 MB of cols.  Its body is the generic kernel's loop with constants; the generic kernel's
stride is run by `gen-cap`.

U = 2^-24 throughout (half an fp32 ulp of a value in [1, 2))."""
import collections
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

import gan_ode_amd._lib as L

U = 2.0 ** -24
GUARD = 64
PATTERN = 0x5A5AA5A5                 # the guard floats' bits
ERRORS = {-1: "E_ARG", -2: "E_SHAPE"}
f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------
# gode_col2im
ROWS_K, PIXEL, FIXED3D, GEN3D = 0, 1, 2, 3
KINDS = {ROWS_K: "row-group", PIXEL: "per-pixel", FIXED3D: "3d-fixed", GEN3D: "3d-generic"}
WHY_ROWLEN, WHY_COLS, WHY_LDS, WHY_GRID = 1, 2, 4, 8          # 2-D
WHY_TAPS, WHY_CHANNELS, WHY_VOXELS = 1, 2, 4                   # 3-D
LDS_MAX, PIXEL_BLOCKS, GEN3D_BLOCKS = 48 * 1024, 8192, 16384

C2Row = collections.namedtuple("C2Row", "name N C xi k s p tanh off kind why twin")


def c2(name, N, C_, xi, k, s, p, kind, why=0, tanh=False, off=0, twin=None):
    """xi / k / s / p: (H, W) tuples for the 2-D op, (D, H, W) for the 3-D one.  off: floats cols lies past a 16-byte boundary.
    twin: the row this one repeats but for `off` (their raw outputs must agree bit for bit)."""
    return C2Row(name, N, C_, tuple(xi), tuple(k), tuple(s), tuple(p), tanh, off, kind, why, twin)


_FX = dict(k=(4, 4, 4), s=(1, 2, 2), p=(0, 1, 1))             # the fixed kernel's taps and strides
C2_ROWS = [
    c2("rows-basic", 2, 3, (5, 6), (4, 4), (2, 2), (1, 1), ROWS_K, tanh=True),
    c2("rows-wide", 1, 3, (3, 80), (4, 4), (2, 2), (1, 1), ROWS_K),              # sh*Wo = 320 > 256
    c2("rows-longrow", 1, 1, (3, 68), (4, 4), (2, 2), (1, 1), ROWS_K),           # C = 1, rowlen/4 = 272 > 256, sh*Wo = 272
    c2("rows-aniso", 2, 4, (4, 7), (3, 5), (2, 3), (1, 2), ROWS_K),              # uneven phases, all three pairs unequal
    c2("rows-k-lt-s", 2, 4, (4, 4), (2, 2), (3, 3), (0, 0), ROWS_K),             # R = 1; 456 outputs with no tap
    c2("rows-s1p2", 1, 2, (6, 6), (3, 3), (1, 1), (2, 2), ROWS_K),               # R = 3, output smaller than input
    c2("rows-lds-at", 1, 4, (3, 48), (4, 4), (1, 1), (1, 1), ROWS_K),            # exactly 49152 B of LDS
    c2("pix-lds-over", 1, 4, (3, 52), (4, 4), (1, 1), (1, 1), PIXEL, WHY_LDS, tanh=True),    # 53248 B
    c2("pix-rowlen", 2, 1, (5, 5), (3, 3), (2, 2), (1, 1), PIXEL, WHY_ROWLEN),
    c2("pix-cols-off", 2, 3, (5, 6), (4, 4), (2, 2), (1, 1), PIXEL, WHY_COLS, tanh=True, off=1, twin="rows-basic"),
    c2("pix-aniso-off", 2, 4, (4, 7), (3, 5), (2, 3), (1, 2), PIXEL, WHY_COLS, off=1, twin="rows-aniso"),
    c2("pix-cap", 1, 1, (1449, 1449), (1, 1), (1, 1), (0, 0), PIXEL, WHY_ROWLEN),            # 8202 blocks > 8192
    # ---- 3-D
    c2("fixed-p0", 2, 3, (2, 3, 3), kind=FIXED3D, **_FX),
    c2("fixed-p1", 2, 3, (3, 3, 4), (4, 4, 4), (1, 2, 2), (1, 1, 1), FIXED3D, tanh=True),    # pd > 0
    c2("gen-c1", 2, 1, (2, 3, 3), kind=GEN3D, why=WHY_CHANNELS, **_FX),
    c2("gen-c2", 2, 2, (2, 3, 3), kind=GEN3D, why=WHY_CHANNELS, **_FX),
    c2("gen-c4", 2, 4, (2, 3, 3), kind=GEN3D, why=WHY_CHANNELS, **_FX),
    c2("gen-k333", 2, 3, (3, 4, 4), (3, 3, 3), (2, 2, 2), (1, 1, 1), GEN3D, WHY_TAPS),
    c2("gen-k244", 2, 3, (2, 3, 3), (2, 4, 4), (1, 2, 2), (0, 1, 1), GEN3D, WHY_TAPS, tanh=True),
    c2("gen-k-lt-s", 2, 4, (2, 3, 3), (1, 2, 2), (2, 3, 3), (0, 0, 0), GEN3D, WHY_TAPS | WHY_CHANNELS),   # voxels with no tap
    c2("gen-cap", 1, 1, (1, 2049, 2049), (1, 1, 1), (1, 1, 1), (0, 0, 0), GEN3D, WHY_TAPS | WHY_CHANNELS),  # 16401 blocks > 16384
]
C2_BY_NAME = {r.name: r for r in C2_ROWS}
assert len(C2_BY_NAME) == len(C2_ROWS)


def c2_out_dims(r):
    return tuple((r.xi[a] - 1) * r.s[a] - 2 * r.p[a] + r.k[a] for a in range(len(r.xi)))


def c2_taps(r):
    return int(np.prod(r.k))


def c2_cols_numel(r):
    return r.N * int(np.prod(r.xi)) * c2_taps(r) * r.C


def c2_out_numel(r):
    return r.N * int(np.prod(c2_out_dims(r))) * r.C


def c2_op(r, cols, out):
    """The row's op over the given addresses (integers; nothing here dereferences them)."""
    xo = c2_out_dims(r)
    epi = L.EPI_TANH if r.tanh else L.EPI_RAW
    if len(r.xi) == 2:
        return L.Col2imOp(cols=cols, out=out, N=r.N, Hi=r.xi[0], Wi=r.xi[1], Ho=xo[0], Wo=xo[1], C=r.C, kh=r.k[0], kw=r.k[1],
                          sh=r.s[0], sw=r.s[1], ph=r.p[0], pw=r.p[1], epilogue=epi)
    return L.Col2imOp(cols=cols, out=out, N=r.N, Di=r.xi[0], Hi=r.xi[1], Wi=r.xi[2], Do=xo[0], Ho=xo[1], Wo=xo[2], C=r.C,
                      kd=r.k[0], kh=r.k[1], kw=r.k[2], sd=r.s[0], sh=r.s[1], sw=r.s[2], pd=r.p[0], ph=r.p[1], pw=r.p[2], epilogue=epi)


def c2_fake_op(r):
    """The row's op over fake non-null pointers of the row's alignment."""
    return c2_op(r, (1 << 20) + 4 * r.off, 2 << 20)


def c2_kind(op):
    """(kind, why) of the op from gode_col2im_launch_kind, or the error's name."""
    kind = (C.c_int32 * 2)(-1, -1)
    rc = L.lib().gode_col2im_launch_kind(C.byref(op), kind)
    return ERRORS[rc] if rc else (kind[0], kind[1])


def c2_geometry(r):
    """What the launcher's arithmetic makes of the row, restated from the row alone: KC, rowlen, R, nq, LDS bytes, sh*Wo,
    outputs, and the blocks an uncapped per-pixel / per-voxel grid would have."""
    xo = c2_out_dims(r)
    KC = c2_taps(r) * r.C
    outputs = r.N * int(np.prod(xo))
    g = dict(KC=KC, outputs=outputs, blocks=(outputs + 255) // 256)
    if len(r.xi) == 2:
        R = -(-r.k[0] // r.s[0])
        g.update(rowlen=r.xi[1] * KC, R=R, nq=(xo[0] - 1 + r.p[0]) // r.s[0] + 1, lds=R * r.xi[1] * KC * 4, group=r.s[0] * xo[1])
    return g


@functools.lru_cache(maxsize=None)
def c2_cols(name):
    """The row's cols, fp32 [N, (Di,) Hi, Wi, taps, C]: random normal values, halved for a tanh row (sums stay unsaturated).
    A twin shares its twin's values."""
    r = C2_BY_NAME[name]
    if r.twin:
        return c2_cols(r.twin)
    gen = torch.Generator().manual_seed(7000 + [x.name for x in C2_ROWS].index(name))
    cols = torch.randn(r.N, *r.xi, c2_taps(r), r.C, generator=gen)
    return cols * 0.5 if r.tanh else cols


def _tap_slices(r, tap):
    """For one tap: the input and output slices per spatial axis that it connects (o = i*s - p + k), or None."""
    sl_in, sl_out = [], []
    xo = c2_out_dims(r)
    for a, kk in enumerate(tap):
        s, p = r.s[a], r.p[a]
        lo = max(0, -((kk - p) // s))                  # ceil((p - kk) / s)
        hi = min(r.xi[a] - 1, (xo[a] - 1 + p - kk) // s)
        if lo > hi:
            return None
        sl_in.append(slice(lo, hi + 1))
        sl_out.append(slice(lo * s - p + kk, hi * s - p + kk + 1, s))
    return sl_in, sl_out


def _overlap_add(r, cols):
    """The overlap-add in cols' precision, taps (kd,) kh, kw ascending, every output element starting from 0: an output element
    receives at most one term per tap, so adding whole tap planes in this order adds each element's terms in the kernels' order."""
    out = torch.zeros(r.N, *c2_out_dims(r), r.C, dtype=cols.dtype)
    for t, tap in enumerate(np.ndindex(*r.k)):
        sl = _tap_slices(r, tap)
        if sl is None:
            continue
        si, so = sl
        out[(slice(None), *so)] += cols[(slice(None), *si, t)]
    return out


@functools.lru_cache(maxsize=None)
def c2_sum32(name):
    """The fp32 emulation of the kernels' sums (before the epilogue), [N, (Do,) Ho, Wo, C]."""
    r = C2_BY_NAME[name]
    return _overlap_add(r, c2_cols(name))


def c2_reference64(name):
    """Independent of the emulation: float64 F.conv_transpose2d / 3d of cols (its taps x C values as channels) with identity tap
    weights; the sum of magnitudes; and the number of taps T of every output element.  All [N, (Do,) Ho, Wo, C]."""
    r = C2_BY_NAME[name]
    nd, T, C_ = len(r.xi), c2_taps(r), r.C
    conv = Fn.conv_transpose2d if nd == 2 else Fn.conv_transpose3d
    w = torch.zeros(T * C_, C_, *r.k, dtype=torch.float64)
    for t, tap in enumerate(np.ndindex(*r.k)):
        for c in range(C_):
            w[(t * C_ + c, c, *tap)] = 1.0
    x = c2_cols(name).double().reshape(r.N, *r.xi, T * C_).movedim(-1, 1)
    back = (lambda y: y.movedim(1, -1).contiguous())
    ref = back(conv(x, w, stride=r.s, padding=r.p))
    mag = back(conv(x.abs(), w, stride=r.s, padding=r.p))
    cnt = back(conv(torch.ones_like(x), w, stride=r.s, padding=r.p))
    return ref, mag, cnt


# ---------------------------------------------------------------------------------------------------------------
# gode_bn_bwd / gode_bn_apply / gode_bn_finalize
NONE, RELU, LRELU, TANH_OUT, LRELU01 = L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH_OUT, L.ACT_LRELU01
SLOPE = {NONE: 1.0, RELU: 0.0, LRELU: float(f32(0.2)), LRELU01: float(f32(0.1))}      # the kernels' fp32 slopes
BNB_ROWS, BNB_CL, EW_BLOCKS, APPLY_BLOCKS = 256, 16, 4096, 8192

BnbRow = collections.namedtuple("BnbRow", "name M C act groups M0 eval_mode gin accumulate gamma bn")


def bnb(M, C_, act, groups=1, M0=0, eval_mode=0, gin=False, accumulate=0, gamma=True, bn=True, tag=""):
    name = f"{M}x{C_}-{ {NONE: 'none', RELU: 'relu', LRELU: 'lrelu', TANH_OUT: 'tanh-out', LRELU01: 'lrelu01'}[act]}" + tag
    return BnbRow(name, M, C_, act, groups, M0, eval_mode, gin, accumulate, gamma, bn)


BNB_CASES = [
    bnb(700, 96, LRELU),                                   # partly masked channel group, three row chunks, a short last one
    bnb(257, 8, RELU),                                     # CL = 2, a chunk of one row
    bnb(300, 512, LRELU01),                                # eight channel groups
    bnb(377, 32, LRELU, groups=2, M0=300, tag="-g2-m0"),   # unequal groups, boundary off a chunk
    bnb(514, 64, RELU, groups=2, tag="-g2"),               # equal halves
    bnb(300, 32, RELU, eval_mode=1, tag="-eval"),
    bnb(300, 32, LRELU, gin=True, accumulate=1, gamma=False, tag="-gin-acc-nogamma"),
    bnb(8200, 512, LRELU),                                 # 1 049 600 float4 > 4096 * 256: the apply kernel strides
    bnb(349527, 3, TANH_OUT, bn=False),                    # 1 048 581 elements: act_bwd_kernel strides
    bnb(5, 7, NONE, bn=False),
]
BNB_BY_NAME = {r.name: r for r in BNB_CASES}
assert len(BNB_BY_NAME) == len(BNB_CASES)

# (M, C, groups, M0, bn) -> the code gode_bn_bwd returns before any launch
BNB_REFUSALS = [(300, c, 1, 0, "E_SHAPE") for c in (12, 20, 24, 40, 48)] + [
    (300, 6, 1, 0, "E_ARG"), (301, 32, 2, 0, "E_ARG"), (300, 32, 2, 300, "E_ARG")]


def bnb_group_rows(r):
    """[(first row, end row)] of the row's BatchNorm batches."""
    if r.groups != 2:
        return [(0, r.M)]
    M0 = r.M0 if r.M0 > 0 else r.M // 2
    return [(0, M0), (M0, r.M)]


def bnb_launch_shape(r):
    """The reduce kernel's grid and masking, restated from gode_bn_bwd: row chunks per group, channel lanes, channel groups,
    dead lanes of the last channel group, float4 of the apply kernel."""
    C4 = r.C // 4
    CL = min(C4, BNB_CL)
    chunks = [-(-(e - b) // BNB_ROWS) for b, e in bnb_group_rows(r)]
    ngr = -(-C4 // CL)
    return dict(CL=CL, chunks=chunks, cgroups=ngr, dead=ngr * CL - C4, last=[(e - b) - (n - 1) * BNB_ROWS for (b, e), n in
                                                                            zip(bnb_group_rows(r), chunks)], n4=r.M * r.C // 4)


def _away_from_kink(y, scale, shift):
    """y with every element whose pre-activation y*scale + shift (or y itself) lies within 1e-3 of 0 moved to pre-activation 0.5:
    fp32 and fp64 then agree about every slope."""
    y = np.where(np.abs(y) < 1e-3, f32(0.5), y).astype(f32)
    z = y.astype(np.float64) * scale + shift
    y = np.where(np.abs(z) < 1e-3, ((0.5 - shift.astype(np.float64)) / scale).astype(f32), y).astype(f32)
    assert np.abs(y.astype(np.float64) * scale + shift).min() > 1e-4
    return y


@functools.lru_cache(maxsize=None)
def bnb_inputs(name):
    """fp32 inputs of the row: y, g [M, C]; gamma [C]; mean, invstd, scale, shift [groups][C]; the dgamma / dbeta pre-fill."""
    r = BNB_BY_NAME[name]
    rng = np.random.RandomState(4000 + [x.name for x in BNB_CASES].index(name))
    M, C_ = r.M, r.C
    if not r.bn:
        y = np.tanh(rng.randn(M, C_) * 1.5).astype(f32) if r.act == TANH_OUT else (rng.randn(M, C_) * 1.5).astype(f32)
        assert np.abs(y).max() < 1.0 or r.act != TANH_OUT
        return dict(y=y, g=rng.randn(M, C_).astype(f32))
    y = (rng.randn(M, C_) * 1.5 + rng.randn(C_)).astype(f32)
    gamma = rng.uniform(0.5, 1.5, C_).astype(f32) * np.where(rng.rand(C_) < 0.5, -1, 1).astype(f32)
    beta = rng.randn(C_).astype(f32)
    gam = gamma if r.gamma else np.ones(C_, f32)
    G = r.groups
    mean, invstd, scale, shift = (np.zeros((G, C_), f32) for _ in range(4))
    for gi, (b, e) in enumerate(bnb_group_rows(r)):
        y64 = y[b:e].astype(np.float64)
        mu, var = y64.mean(0), y64.var(0)
        if r.eval_mode:                               # running statistics: constants near the batch's, not the batch's
            mu, var = mu + 0.1 * rng.randn(C_), var * rng.uniform(0.8, 1.25, C_)
        mean[gi], invstd[gi] = mu.astype(f32), (1.0 / np.sqrt(var + 1e-5)).astype(f32)
        scale[gi] = gam * invstd[gi]
        shift[gi] = beta - mean[gi] * scale[gi]
        y[b:e] = _away_from_kink(y[b:e], scale[gi], shift[gi])
    return dict(y=y, g=rng.randn(M, C_).astype(f32), gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift,
                dgamma0=rng.randn(C_).astype(f32), dbeta0=rng.randn(C_).astype(f32))


def bnb_reference(r, x, dtype=np.float64):
    """gode_bn_bwd's contract (gode.h) evaluated in `dtype` from the fp32 inputs, and -- for float64 -- the per-element bounds.
    Returns dict(g_y, dgamma, dbeta[, b_g_y, b_dgamma, b_dbeta]).  The bounds are those of tests/test_gpu_dcgan.py with each
    group's own row count Mg:
        g_y     12U k (|g_z| + |dbeta|/Mg + |xhat dgamma|/Mg) + 5U k (sum|g_z|/Mg + |xhat| sum|g_z xhat|/Mg),  k = |gamma invstd|
        dbeta   3U sum|g_z|;  dgamma  6U sum|g_z xhat|    (+ U |result| when the sums are added to a pre-fill)
        eval mode: g_y = k g_z within 4U k |g_z|;   no BatchNorm, tanh from the output: g (1 - y*y) within 4U |g|
    The sums are taken in float64 under either dtype (the kernel accumulates them in double)."""
    t = (lambda a: np.asarray(a, dtype))
    y, g = t(x["y"]), t(x["g"])
    want = dtype == np.float64
    if not r.bn:
        if r.act == TANH_OUT:
            out = dict(g_y=g * (t(1) - y * y))
            if want:
                out["b_g_y"] = 4 * U * np.abs(g)
            return out
        out = dict(g_y=g * np.where(y > 0, t(1), t(SLOPE[r.act])))
        if want:
            out["b_g_y"] = 2 * U * np.abs(g) * (SLOPE[r.act] not in (0.0, 1.0))   # a product by 0 or 1 is exact
        return out
    gam = t(x["gamma"]) if r.gamma else np.ones(r.C, dtype)
    g_y, b_g_y = np.zeros((r.M, r.C), dtype), np.zeros((r.M, r.C))
    dgamma, dbeta, sb_all, sg_all = (np.zeros(r.C) for _ in range(4))
    for gi, (b, e) in enumerate(bnb_group_rows(r)):
        Mg = e - b
        mu, isd, sc, sh = (t(x[k][gi]) for k in ("mean", "invstd", "scale", "shift"))
        z = y[b:e] * sc + sh
        gz = g[b:e] * np.where(z > 0, t(1), t(SLOPE[r.act]))
        xhat = (y[b:e] - mu) * isd
        db, dg = gz.astype(np.float64).sum(0), (gz.astype(np.float64) * xhat.astype(np.float64)).sum(0)
        sb, sg = np.abs(gz).astype(np.float64).sum(0), np.abs(gz * xhat).astype(np.float64).sum(0)
        k = gam * isd
        if r.eval_mode:
            g_y[b:e] = k * gz
            b_g_y[b:e] = 4 * U * np.abs(k * gz)
        else:
            if want:
                g_y[b:e] = k * (gz - db / Mg - xhat * dg / Mg)
            else:       # the kernel's form: three coefficient vectors rounded to fp32, (mean - y) formed first
                cB, cC = t(k.astype(np.float64) * isd * dg / Mg), t(k.astype(np.float64) * db / Mg)
                g_y[b:e] = k * gz + cB * (mu - y[b:e]) - cC
            ka = np.abs(k).astype(np.float64)
            b_g_y[b:e] = (12 * U * ka * (np.abs(gz) + np.abs(db) / Mg + np.abs(xhat * dg) / Mg)
                          + 5 * U * ka * (sb / Mg + np.abs(xhat) * sg / Mg))
        dgamma, dbeta, sb_all, sg_all = dgamma + dg, dbeta + db, sb_all + sb, sg_all + sg
    if r.accumulate:
        dgamma, dbeta = dgamma + x["dgamma0"], dbeta + x["dbeta0"]
    out = dict(g_y=g_y, dgamma=t(dgamma), dbeta=t(dbeta))
    if want:
        out.update(b_g_y=b_g_y, b_dbeta=3 * U * sb_all + (U * np.abs(dbeta) if r.accumulate else 0),
                   b_dgamma=6 * U * sg_all + (U * np.abs(dgamma) if r.accumulate else 0))
    return out


def bnb_fake_op(M, C_, groups, M0):
    """A BatchNorm backward op over fake non-null pointers: for the refusals, which return before anything is read."""
    p = [(k + 1) << 20 for k in range(10)]
    return L.BnBwdOp(g=p[0], y=p[1], M=M, C=C_, act=RELU, gamma=p[2], mean=p[3], invstd=p[4], scale=p[5], shift=p[6], dgamma=p[7],
                     dbeta=p[8], work=p[9], groups=groups, M0=M0)


BnaRow = collections.namedtuple("BnaRow", "name M C act M0 affine")
BNA_CASES = [
    BnaRow("37x8-lrelu-m0", 37, 8, LRELU, 13, True),
    BnaRow("37x8-none-noscale", 37, 8, NONE, 0, False),
    BnaRow("66000x128-relu", 66000, 128, RELU, 0, True),        # 2 112 000 float4 > 8192 * 256
]
BNA_BY_NAME = {r.name: r for r in BNA_CASES}


@functools.lru_cache(maxsize=None)
def bna_inputs(name):
    r = BNA_BY_NAME[name]
    rng = np.random.RandomState(5000 + [x.name for x in BNA_CASES].index(name))
    G = 2 if r.M0 > 0 else 1
    return dict(y=(rng.randn(r.M, r.C) * 1.5).astype(f32),
                scale=(rng.uniform(0.5, 1.5, (G, r.C)) * np.where(rng.rand(G, r.C) < 0.5, -1, 1)).astype(f32),
                shift=rng.randn(G, r.C).astype(f32))


def bna_reference(r, x, dtype=np.float64):
    """act(y*scale + shift), rows >= M0 with the second coefficient set, in `dtype`; for float64 also the bound
    4U (|y scale| + |shift|): the product, the sum, the slope's product and the slope's own 0.25 U."""
    y = np.asarray(x["y"], dtype)
    G = 2 if r.M0 > 0 else 1
    sc = np.asarray(x["scale"], dtype) if r.affine else np.ones((G, r.C), dtype)
    sh = np.asarray(x["shift"], dtype) if r.affine else np.zeros((G, r.C), dtype)
    grp = (np.arange(r.M) >= r.M0).astype(int) if r.M0 > 0 else np.zeros(r.M, int)
    z = y * sc[grp] + sh[grp]
    out = np.maximum(z, z * np.asarray(SLOPE[r.act], dtype))
    return out, 4 * U * (np.abs(y.astype(np.float64) * sc[grp]) + np.abs(sh[grp]).astype(np.float64))


# gode_bn_finalize, training mode: C = 8 channels in ncols = 4*C statistics columns (reps = 4), rows = 300 partial rows -- 1200
# items per channel, more than one pass of the 256 threads -- each partial the fp32 sum / sum of squares of KPER elements.
# Channel BNF_CONST holds the constant 1000.0: its sums of squares, 1e6 * KPER, are not representable in fp32 and round DOWN, so
# sum2/n - mean^2 is negative before the clamp.
BNF_C, BNF_REPS, BNF_ROWS, BNF_KPER, BNF_CONST = 8, 4, 300, 1125, 5
BNF_MOMENTUM, BNF_EPS = float(f32(0.1)), float(f32(1e-5))


@functools.lru_cache(maxsize=None)
def bnf_inputs():
    rng = np.random.RandomState(6000)
    Cc, ncols = BNF_C, BNF_C * BNF_REPS
    per = 25
    assert BNF_KPER % per == 0
    sig, mu = np.tile(rng.uniform(0.5, 2.0, Cc), BNF_REPS), np.tile(rng.randn(Cc), BNF_REPS)      # column = rep*C + c
    d = rng.randn(ncols, BNF_ROWS, per) * sig[:, None, None] + mu[:, None, None]
    rep = BNF_KPER // per                          # each partial: `rep` copies of its 25 values
    s1, s2 = rep * d.sum(2), rep * (d * d).sum(2)
    for q in range(BNF_REPS):
        s1[q * Cc + BNF_CONST], s2[q * Cc + BNF_CONST] = 1000.0 * BNF_KPER, 1e6 * BNF_KPER
    stats = np.stack([s1, s2]).astype(f32)         # [2][ncols][rows]
    return dict(stats=stats, count=BNF_ROWS * BNF_REPS * BNF_KPER, gamma=rng.uniform(0.5, 1.5, Cc).astype(f32),
                beta=rng.randn(Cc).astype(f32), running_mean=rng.randn(Cc).astype(f32), running_var=rng.uniform(0.5, 2, Cc).astype(f32))


def bnf_reference(x):
    """gode_bn_finalize's contract in float64 from the fp32 partials, the variance before its clamp, and bounds: mean and invstd
    are double results rounded once (U of the value; 1e-9 relative covers the order of the double sums); scale is one more
    fp32 product (2U); shift = beta - fp32(mean)*scale carries mean's and scale's roundings, the product and the difference
    (6U (|beta| + |mean scale|)); a running statistic is (1 - m) r + m s with fp32(1 - m), two products and a sum
    (4U (|r| + |m s|))."""
    st = x["stats"].astype(np.float64).reshape(2, BNF_REPS, BNF_C, BNF_ROWS)
    n = float(x["count"])
    mean = st[0].sum((0, 2)) / n
    var_raw = st[1].sum((0, 2)) / n - mean * mean
    var = np.maximum(var_raw, 0.0)
    invstd = 1.0 / np.sqrt(var + BNF_EPS)
    g, b = x["gamma"].astype(np.float64), x["beta"].astype(np.float64)
    scale = g * invstd
    shift = b - mean * scale
    m = BNF_MOMENTUM
    unb = var * n / (n - 1)
    rm0, rv0 = x["running_mean"].astype(np.float64), x["running_var"].astype(np.float64)
    ref = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=(1 - m) * rm0 + m * mean,
               running_var=(1 - m) * rv0 + m * unb)
    tiny = 1e-9
    bound = dict(mean=(U + tiny) * np.abs(mean), invstd=(U + tiny) * invstd, scale=(2 * U + tiny) * np.abs(scale),
                 shift=6 * U * (np.abs(b) + np.abs(mean * scale)), running_mean=4 * U * (np.abs(rm0) + np.abs(m * mean)),
                 running_var=4 * U * (np.abs(rv0) + np.abs(m * unb)))
    return ref, bound, var_raw


# ---------------------------------------------------------------------------------------------------------------
# Adam
# Counting from one, even-numbered tensors are 16-byte aligned and odd-numbered ones one float off: the eighth, 2 097 159 elements,
# runs 524 289 float4 > 2048 blocks * 256 (the float4 loop strides), the ninth, 524 293, as many scalars (the scalar loop strides).
ADAM_SIZES = [1, 5, 64, 1003, 4096, 70001, 9, 2097159, 524293]
ADAM_L2_SIZES = [1003, 524293, 1048583]                             # gode_adam_l2: 1 048 583 > 4096 * 256
ADAM_STEPS = 3
ADAM_GSCALES = [1.0, 0.25]
ADAM_HP = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, weight_decay=1e-5)
ADAM_BLOCKS = 2048


def adam_paths(k, n):
    """What adam_tensor does with tensor k of n elements: float4 items, scalar items, and whether either loop strides."""
    vec = k % 2 == 1
    n4 = n // 4 if vec else 0
    scalar = n - 4 * n4
    threads = ADAM_BLOCKS * 256
    return dict(n4=n4, scalar=scalar, vec_strides=n4 > threads, scalar_strides=scalar > threads)


@functools.lru_cache(maxsize=None)
def adam_data(sizes=tuple(ADAM_SIZES)):
    """Initial p, m, v and the gradient of each step, per tensor: p, g random normal, g times a power of ten in [1e-4, 10]
    that changes with tensor and step; m, v the state of an optimiser that has already run (v > 0)."""
    gen = torch.Generator().manual_seed(8000)
    p = [torch.randn(n, generator=gen) for n in sizes]
    m = [torch.randn(n, generator=gen) * 0.1 for n in sizes]
    v = [torch.rand(n, generator=gen) * 0.01 for n in sizes]
    g = [[torch.randn(n, generator=gen) * 10.0 ** ((k + 2 * s) % 6 - 4) for k, n in enumerate(sizes)] for s in range(ADAM_STEPS)]
    return p, m, v, g


def adam_coefficients(step, hp=ADAM_HP):
    """The fp32 constants the kernels see, as float64 numbers: 1 - b1, 1 - b2 (fp32 differences), b2, eps, wd, step_size, bc2_sqrt."""
    lr, b1, b2 = float(f32(hp["lr"])), float(f32(hp["beta1"])), float(f32(hp["beta2"]))
    return dict(omb1=float(f32(1) - f32(hp["beta1"])), omb2=float(f32(1) - f32(hp["beta2"])), b2=b2, eps=float(f32(hp["eps"])),
                wd=float(f32(hp["weight_decay"])), step_size=float(f32(lr / (1.0 - b1 ** float(step)))),
                bc2=float(f32((1.0 - b2 ** float(step)) ** 0.5)))


def adam_reference(p, g, m, v, gscale, step):
    """One Adam(L2) step in float64 from fp32 state (torch.optim.Adam's single-tensor operation order, the kernels'), and the
    per-element bounds on p', m', v':
        gi = g gscale + wd p,  eg = 2U (|g gscale| + |wd p|),  den = sqrt(v')/bc2 + eps,  upd = step_size m'/den
        dm = eg (1-b1) + 3U (|m| + |gi - m| (1-b1))
        dv = 2 |gi| eg (1-b2) + 4U (|v| b2 + (1-b2) gi^2)
        dden = (dv / (2 sqrt(v')) + 2U sqrt(v')) / bc2 + U den
        dp = 2U (|p| + |upd|) + step_size (dm/den + |m'| dden/den^2) + 4U |upd|"""
    c = adam_coefficients(step)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gs = float(f32(gscale))
    gi = g * gs + c["wd"] * p
    eg = 2 * U * (np.abs(g * gs) + np.abs(c["wd"] * p))
    m1 = m + (gi - m) * c["omb1"]
    v1 = v * c["b2"] + c["omb2"] * gi * gi
    rt = np.sqrt(v1)
    den = rt / c["bc2"] + c["eps"]
    upd = c["step_size"] * m1 / den
    dm = eg * c["omb1"] + 3 * U * (np.abs(m) + np.abs(gi - m) * c["omb1"])
    dv = 2 * np.abs(gi) * eg * c["omb2"] + 4 * U * (np.abs(v) * c["b2"] + c["omb2"] * gi * gi)
    dden = (dv / (2 * rt) + 2 * U * rt) / c["bc2"] + U * den
    dp = 2 * U * (np.abs(p) + np.abs(upd)) + c["step_size"] * (dm / den + np.abs(m1) * dden / den ** 2) + 4 * U * np.abs(upd)
    return (p - upd, m1, v1), (dp, dm, dv)


def adam_restated32(p, g, m, v, gscale, step):
    """The kernels' update written out in fp32 NumPy, every operation rounded on its own."""
    c = adam_coefficients(step)
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    one = f32(1)
    b1, b2 = f32(ADAM_HP["beta1"]), f32(ADAM_HP["beta2"])
    gi = g * f32(gscale) + f32(c["wd"]) * p
    m1 = m + (gi - m) * (one - b1)
    v1 = v * b2 + (one - b2) * gi * gi
    den = np.sqrt(v1) / f32(c["bc2"]) + f32(c["eps"])
    return p - f32(c["step_size"]) * (m1 / den), m1, v1


def guarded_layout(sizes, gap=9):
    """Offsets (in floats) of tensors carved out of one buffer with gaps around each: counting from one, even-numbered ones on a
    16-byte boundary, odd-numbered ones one float past one; and the buffer's length."""
    offs, off = [], gap
    for k, n in enumerate(sizes):
        off = (off + 3) // 4 * 4 + (k + 1) % 2
        offs.append(off)
        off += n + gap
    return offs, off + 4
