"""The launch branches of gan-ode_amd/csrc/gres.hip as plain data: named rows for gode_chstats, gode_cbn_embed(_bwd),
gode_cbn_apply, gode_cbn_bwd, gode_gres_out(_bwd) and gode_sn_fwd / gode_sn_bwd, each at the smallest shape that reaches the
branch it is named after, with the launch arithmetic restated in Python (every function names the line of gres.hip it mirrors;
the rows carry the values expected of them), the float64 references and the per-element bounds.  Shared by
tests/test_host_gres_cells.py (every row reaches what it names, the restated numbers are the library's, an fp32 restatement of
every op stays inside the bounds, the refusals) and tests/test_gpu_gres_cells.py (every row on the GPU).

References and restatements are written once, in torch, over a dtype: float64 is the reference, float32 (on the CPU every
operation is rounded on its own, no contraction) the restatement; sums that the kernels accumulate in double are taken in
double under either dtype.  They run wherever their inputs live, so the GPU test computes the capped rows' references on the
device.

Bounds.  U = 2^-24 (half an fp32 ulp of a value in [1, 2)).  Every bound is first order: the number of fp32 roundings a term
passes through times U times the term's magnitude in the float64 reference, an fma counted as the two roundings it replaces
(so the compiler may contract or not).  A double sum rounded once to fp32: U |value| + 1e-9 sum|terms| -- n terms added in
double in any order are within (n - 1) 2^-53 sum|terms|, below 1e-9 sum|terms| for n < 9e6.  fp32 division is one rounding
(HIP's default is the correctly rounded divide).  The constants are counted below where they are used; none was measured.

Left out: element counts of 2^31 and more run only as refusals (a tensor of 8 GB); the `N > 65535` refusal of gode_cbn_bwd
likewise; sn_wtu / sn_wv beyond w = 513, h = 513 (their loops have no further branch)."""
import collections
import functools

import numpy as np
import torch

import gan_ode_amd._lib as L

U = 2.0 ** -24
TINY = 1e-9
GUARD = 64
PATTERN = 0x5A5AA5A5                 # the guard floats' bits
ERRORS = {0: "OK", -1: "E_ARG", -2: "E_SHAPE"}
NONE, RELU, LRELU = L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU
ACT_NAMES = {NONE: "none", RELU: "relu", LRELU: "lrelu"}
SLOPE = float(np.float32(0.2))       # the kernels' fp32 slope
f32, f64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------
# the launch arithmetic of gres.hip
def pow2_ge(x):
    """gres_pow2_ge (gres.hip:10)."""
    p = 1
    while p < x:
        p <<= 1
    return p


def gres_tc(C_):
    """gres_tc (gres.hip:23): channel threads of the logical [TP][TC] grid."""
    return 256 if C_ >= 256 else pow2_ge(C_)


def gres_tp(C_):
    """TP = 256 / TC (gres.hip:33 and :200)."""
    return 256 // gres_tc(C_)


def channel_groups(C_):
    """Trips of the `cb` loop (gres.hip:38 and :204), and the live channels of the last one."""
    tc = gres_tc(C_)
    n = -(-C_ // tc)
    return n, C_ - (n - 1) * tc


def cbn_bwd_nblk(HW):
    """cbn_bwd_nblk (gres.hip:195) and the chunk of gode_cbn_bwd (gres.hip:311): (chunks, positions per chunk, positions of
    the last chunk)."""
    b = min(max((HW + 63) // 64, 1), 32)
    chunk = -(-HW // b)
    return b, chunk, HW - (b - 1) * chunk


def chstats_rows(P):
    """gode_chstats_rows (gres.hip:62)."""
    return min(max((P + 63) // 64, 1), 1024)


def chstats_chunk(P, rows):
    """launch_chstats (gres.hip:71): (positions per workgroup, workgroups whose chunk is empty)."""
    chunk = -(-P // rows)
    return chunk, sum(1 for b in range(rows) if b * chunk >= P)


def gres_blocks(total, cap=16384):
    """gres_blocks (gres.hip:17): (blocks, whether the grid-stride loop takes a second trip)."""
    b = min(max((total + 255) // 256, 1), cap)
    return b, total > b * 256


def sn_bwd_blocks(n):
    """gode_sn_bwd (gres.hip:552-554): (sn_dot's blocks, its span)."""
    nblk = min((n + 1023) // 1024, L.SN_BWD_BLOCKS)
    return nblk, -(-n // nblk)


def embed_blocks(N, K, C2):
    """gode_cbn_embed (gres.hip:101) and gode_cbn_embed_bwd (gres.hip:136-138): (forward blocks, backward blocks, the backward's
    segment starts [dW, db, dcond, end])."""
    nW, nb, nc = C2 * K, C2, N * K
    return (N * C2 + 255) // 256, (nW + nb + nc + 255) // 256, [0, nW, nW + nb, nW + nb + nc]


def out_dims(H, W, f, down):
    """gres_out_dims (gres.hip:363)."""
    return H * f // down, W * f // down


# ---------------------------------------------------------------------------------------------------------------
# memory layouts of a logical [N, H, W, C] tensor
LAYOUTS = ("dense", "nhwc", "nchw", "nchw-slice", "cl-pad", "expand")
SRC_LAYOUTS = ("dense", "nchw", "nchw-slice")        # what the strided ops other than chstats are run through


def effective(vals, layout):
    """The values a layout presents: `expand` repeats the first row of every map over H (a zero stride)."""
    return vals[:, :1].expand(vals.shape).contiguous() if layout == "expand" else vals


def base_shape(shape, layout):
    """The buffer a layout's view is cut out of."""
    N, H, W, C_ = shape
    return {"dense": (N, H, W, C_), "nhwc": (N, H, W, C_), "nchw": (N, C_, H, W), "nchw-slice": (N, C_ + 1, H + 1, W + 2),
            "cl-pad": (N, H, W + 1, C_ + 3)}[layout]


def window(base, layout):
    """The view indexed [n, h, w, c] of a base_shape buffer."""
    if layout in ("dense", "nhwc"):
        return base
    if layout == "nchw":
        return base.permute(0, 2, 3, 1)
    if layout == "nchw-slice":
        return base[:, 1:, 1:, 1:-1].permute(0, 2, 3, 1)
    if layout == "cl-pad":
        return base[:, :, :-1, 1:-2]
    raise ValueError(layout)


def op_strides(v, layout):
    """The op's {N, H, W, C} strides of a view: the all-zero sentinel for `dense`; a dimension of one element, whose stride
    is never used, reports at least 1 (so that nothing else is mistaken for the sentinel)."""
    if layout == "dense":
        return (0, 0, 0, 0)
    return tuple(max(s, 1) if n == 1 else s for s, n in zip(v.stride(), v.shape))


def place(vals, layout, device="cpu"):
    """fp32 [N, H, W, C] values -> (a view indexed [n, h, w, c] over memory laid out as `layout`, the op's {N, H, W, C} strides).
    dense: channels-last contiguous through the all-zero sentinel; nhwc: the same with its strides spelled out; nchw;
    nchw-slice: a window of a larger NCHW buffer; cl-pad: a window of a larger channels-last buffer (channel stride 1, padded
    pixels and rows); expand: see effective().  Memory outside the view is NaN."""
    if layout == "expand":
        v = vals[:, :1].to(device).contiguous().expand(vals.shape)
    else:
        v = window(torch.full(base_shape(vals.shape, layout), float("nan"), device=device), layout)
        v.copy_(vals)
    return v, op_strides(v, layout)


def setv(arr, vals):
    for i, v in enumerate(vals):
        arr[i] = int(v)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _signed(g, *shape):
    """Values of both signs in +-[0.5, 1.5]."""
    return (torch.rand(*shape, generator=g) + 0.5) * torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------
# gode_chstats
ChRow = collections.namedtuple("ChRow", "name N H W C layout rows TP groups live chunk empty")


def _ch(name, N, H, W, C_, layout, rows, TP, groups, live, chunk, empty):
    """rows: "one", "auto" (gode_chstats_rows(P)) or "over" (P + 5).  TP, groups (trips of the cb loop), live (channels of the
    last trip), chunk, empty (workgroups with no position): what the launcher must make of the row."""
    return ChRow(name, N, H, W, C_, layout, rows, TP, groups, live, chunk, empty)


_CH_C = {1: (256, 1, 1), 3: (64, 1, 3), 100: (2, 1, 100), 256: (1, 1, 256), 257: (1, 2, 1)}
CH_ROWS = [_ch(f"c{c}-{lay}", 2, 7, 5, c, lay, "auto", *_CH_C[c], 35, 0) for c in _CH_C for lay in LAYOUTS] + [
    _ch("rows-one", 2, 7, 5, 3, "dense", "one", 64, 1, 3, 70, 0),
    _ch("rows-over-empty-tail", 2, 7, 5, 3, "dense", "over", 64, 1, 3, 1, 5),
    _ch("rows-over-pfast-c257", 2, 7, 5, 257, "nchw", "over", 1, 2, 1, 1, 5),
    _ch("rows-cap-1024", 257, 256, 1, 3, "dense", "auto", 64, 1, 3, 65, 11),    # workgroups 1013..1023 empty, 1012 short
]
CH_BY_NAME = {r.name: r for r in CH_ROWS}
assert len(CH_BY_NAME) == len(CH_ROWS)


def ch_rows_of(r):
    P = r.N * r.H * r.W
    return {"one": 1, "auto": chstats_rows(P), "over": P + 5}[r.rows]


@functools.lru_cache(maxsize=None)
def ch_values(N, H, W, C_):
    """One set of values per shape: every layout of a shape presents the same numbers."""
    return torch.randn(N, H, W, C_, generator=_gen(1000 + C_ + N)) + 0.5


def ch_reference(x, rows):
    """Per-workgroup partial sums in float64 over the documented chunking (positions in n, h, w order, chunk = ceil(P / rows)):
    (stats [2][C][rows], bound).  A double sum rounded once: U |value| + 1e-9 sum|terms|; v * v of an fp32 v is exact in double."""
    N, H, W, C_ = x.shape
    P = N * H * W
    chunk = -(-P // rows)
    v = torch.cat([x.to(f64).reshape(P, C_), torch.zeros(rows * chunk - P, C_, dtype=f64, device=x.device)]).reshape(rows, chunk, C_)
    s1, s2, m1 = v.sum(1).t(), (v * v).sum(1).t(), v.abs().sum(1).t()
    ref = torch.stack([s1, s2])
    return ref, U * ref.abs() + TINY * torch.stack([m1, s2])


def ch_op(r, x_ptr, strides, stats_ptr):
    op = L.ChstatsOp(x=x_ptr, stats=stats_ptr, N=r.N, H=r.H, W=r.W, C=r.C, rows=ch_rows_of(r))
    setv(op.xs, strides)
    return op


# ---------------------------------------------------------------------------------------------------------------
# gode_cbn_embed / gode_cbn_embed_bwd
EmRow = collections.namedtuple("EmRow", "name N K C2 b null fwd_blocks bwd_blocks")
EM_ROWS = [
    EmRow("one-output-pair", 1, 1, 2, True, None, 1, 1),
    EmRow("one-workgroup", 5, 6, 20, True, None, 1, 1),
    EmRow("fwd-two-workgroups", 5, 6, 60, True, None, 2, 2),           # 300 forward outputs
    EmRow("real-layer-96-to-200", 3, 96, 200, True, None, 3, 77),      # dW: blocks 0..74; db opens block 75; dcond crosses into 76
    EmRow("db-straddles-blocks", 2, 5, 300, True, None, 3, 8),         # dW ends inside block 5; db [1500, 1800) crosses 1536 and 1792
    EmRow("b-null", 5, 6, 20, False, None, 1, 1),
    EmRow("dW-null", 5, 6, 20, True, "dW", 1, 1),
    EmRow("db-null", 5, 6, 20, True, "db", 1, 1),
    EmRow("dcond-null", 5, 6, 20, True, "dcond", 1, 1),
]
EM_BY_NAME = {r.name: r for r in EM_ROWS}


@functools.lru_cache(maxsize=None)
def em_inputs(N, K, C2):
    g = _gen(2000 + N + K + C2)
    return dict(cond=torch.randn(N, K, generator=g), W=torch.randn(C2, K, generator=g), b=torch.randn(C2, generator=g),
                dgb=torch.randn(N, C2, generator=g))


def _dot(a, b, dtype):
    """sum_k a[i, k] b[j, k], added in k order from 0 in `dtype`; and the sum of magnitudes in float64."""
    s = torch.zeros(a.shape[0], b.shape[0], dtype=dtype)
    for k in range(a.shape[1]):
        s = s + a[:, k:k + 1].to(dtype) * b[:, k].to(dtype)
    return s, a.abs().to(f64) @ b.abs().to(f64).t()


def em_reference(r, x, dtype=f64):
    """gb = cond W^T + b; dW = dgb^T cond; db = sum_n dgb; dcond = dgb W.  An fp32 sum of n products added in order passes every
    term through at most n + 1 roundings (its product, n - 1 partial sums, the bias): (n + 2) U sum|terms| covers gamma_(n+1)."""
    gb, m_gb = _dot(x["cond"], x["W"], dtype)
    if r.b:
        gb, m_gb = gb + x["b"].to(dtype), m_gb + x["b"].abs().to(f64)
    dW, m_dW = _dot(x["dgb"].t(), x["cond"].t(), dtype)
    db, m_db = _dot(x["dgb"].t(), torch.ones(1, r.N), dtype)
    dc, m_dc = _dot(x["dgb"], x["W"].t(), dtype)
    ref = dict(gb=gb, dW=dW, db=db.reshape(-1), dcond=dc)
    bound = dict(gb=(r.K + 2) * U * m_gb, dW=(r.N + 2) * U * m_dW, db=(r.N + 2) * U * m_db.reshape(-1), dcond=(r.C2 + 2) * U * m_dc)
    return ref, bound


def em_ops(r, p):
    """(forward op, backward op) over the addresses in p (integers or None)."""
    fwd = L.CbnEmbedOp(cond=p["cond"], W=p["W"], b=p["b"] if r.b else None, gb=p["gb"], N=r.N, K=r.K, C2=r.C2)
    bwd = L.CbnEmbedBwdOp(cond=p["cond"], W=p["W"], dgb=p["dgb"], N=r.N, K=r.K, C2=r.C2,
                          **{k: (None if r.null == k else p[k]) for k in ("dW", "db", "dcond")})
    return fwd, bwd


# ---------------------------------------------------------------------------------------------------------------
# gode_cbn_apply and gode_cbn_bwd share their rows' inputs
def _up_first(t, f):
    """[N, H*f, W*f, C] -> [N, H, W, C]: the first element of every f x f block."""
    return t[:, ::f, ::f]


def _blocks(t, f):
    """[N, H*f, W*f, C] -> the f*f tensors [N, H, W, C] of a block's elements, in the kernels' (di, dj) order."""
    return [t[:, di::f, dj::f] for di in range(f) for dj in range(f)]


def cbn_inputs(N, H, W, C_, f, act, bias, bn, seed, gadd=True):
    """fp32 inputs of an apply / backward row.  With an activation, every source element whose pre-activation z lies within 1e-3
    of 0 is moved to z = 0.5, so that fp32 and float64 agree about every slope (asserted: min |z| > 1e-4)."""
    g = _gen(seed)
    x = dict(src=torch.randn(N, H, W, C_, generator=g) * 1.5 + torch.randn(C_, generator=g),
             bias=torch.randn(C_, generator=g) if bias else None, mean=None, invstd=None, gb=None)
    if bn:
        v = x["src"].to(f64) + (x["bias"].to(f64) if bias else 0.0)
        x["mean"] = (v.mean((0, 1, 2)) + 0.1 * torch.randn(C_, generator=g).to(f64)).float()
        x["invstd"] = (1.0 / torch.sqrt(v.var((0, 1, 2), unbiased=False) * (torch.rand(C_, generator=g).to(f64) * 0.45 + 0.8) + 1e-5)).float()
        x["gb"] = torch.cat([_signed(g, N, C_), torch.randn(N, C_, generator=g)], 1)           # gammas of both signs per sample
    if act != NONE:
        z = _preact(x, C_, f64)
        bad = z.abs() < 1e-3
        b64 = x["bias"].to(f64) if bias else torch.zeros(C_, dtype=f64)
        if bn:
            gam, bet = x["gb"][:, None, None, :C_].to(f64), x["gb"][:, None, None, C_:].to(f64)
            want = (0.5 - bet) / (gam * x["invstd"].to(f64)) + x["mean"].to(f64) - b64
        else:
            want = (0.5 - b64).expand(z.shape)
        x["src"] = torch.where(bad, want.float().expand(z.shape), x["src"])
        assert float(_preact(x, C_, f64).abs().min()) > 1e-4
    x["g_a"] = torch.randn(N, H * f, W * f, C_, generator=g)
    x["gadd"] = torch.randn(N, H, W, C_, generator=g) if gadd else None
    return x


def _preact(x, C_, dtype):
    """(src + bias - mean) invstd gamma + beta in the kernels' operation order, or src + bias."""
    v = x["src"].to(dtype)
    if x["bias"] is not None:
        v = v + x["bias"].to(dtype)
    if x["mean"] is None:
        return v
    xh = (v - x["mean"].to(dtype)) * x["invstd"].to(dtype)
    return x["gb"][:, None, None, :C_].to(dtype) * xh + x["gb"][:, None, None, C_:].to(dtype)


def _act(z, act):
    if act == RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == LRELU:
        return torch.where(z > 0, z, z * SLOPE)
    return z


def _e_v(x):
    """Error of v = src + bias: one rounding."""
    return U * (x["src"].abs().to(f64) + x["bias"].abs().to(f64)) if x["bias"] is not None else torch.zeros_like(x["src"], dtype=f64)


def apply_reference(x, C_, f, act, dtype=f64):
    """act(z) replicated f x f, [N, H*f, W*f, C]; for float64 also the bound.  z = gamma xh + beta, xh = (v - mean) invstd,
    v = src + bias.  v: one rounding, e_v = U (|src| + |bias|).  v - mean: e_v + U |v - mean|; times invstd, one more:
    e_xh = invstd e_v + 2U |xh|.  gamma xh + beta: |gamma| e_xh plus the product's and the sum's roundings,
    2U (|gamma xh| + |beta|) -- so e_z = |gamma| invstd e_v + 4U |gamma xh| + 2U |beta|.  ReLU and identity add nothing;
    the leaky slope's product adds U |out| (and scales e_z by 0.2, not taken)."""
    z = _preact(x, C_, dtype)
    out = _act(z, act)
    rep = (lambda t: t.repeat_interleave(f, 1).repeat_interleave(f, 2) if f > 1 else t)
    if dtype != f64:
        return rep(out)
    e = _e_v(x)
    if x["mean"] is not None:
        gam, bet, isd = x["gb"][:, None, None, :C_].to(f64).abs(), x["gb"][:, None, None, C_:].to(f64).abs(), x["invstd"].to(f64)
        xh = (x["src"].to(f64) + (x["bias"].to(f64) if x["bias"] is not None else 0.0) - x["mean"].to(f64)) * isd
        e = gam * isd * e + 4 * U * gam * xh.abs() + 2 * U * bet
    if act == LRELU:
        e = e + U * out.abs()
    return rep(out), rep(e)


def apply_op(r, p, strides):
    op = L.CbnApplyOp(src=p["src"], bias=p.get("bias"), mean=p.get("mean"), invstd=p.get("invstd"), gb=p.get("gb"), out=p["out"],
                      N=r.N, H=r.H, W=r.W, C=r.C, f=r.f, act=r.act)
    setv(op.ss, strides)
    return op


ApRow = collections.namedtuple("ApRow", "name N H W C f act bias bn blocks strides_loop")


def _ap(name, N, H, W, C_, f, act, bias=True, bn=True, blocks=None, strides_loop=False):
    return ApRow(name, N, H, W, C_, f, act, bias, bn, blocks, strides_loop)


AP_ROWS = [_ap(f"{ACT_NAMES[a]}-f{f}", 3, 7, 5, 3, f, a, blocks=2) for a in (NONE, RELU, LRELU) for f in (1, 2)] + [
    _ap("c1-bias-null", 3, 7, 5, 1, 2, RELU, bias=False, blocks=1),
    _ap("c257-mean-null", 2, 3, 5, 257, 1, LRELU, bn=False, blocks=31),
    _ap("c257-mean-null-bias-null", 2, 3, 5, 257, 2, RELU, bias=False, bn=False, blocks=31),
    _ap("c257-f2", 2, 3, 5, 257, 2, LRELU, blocks=31),
    _ap("capped-f1", 2, 128, 128, 129, 1, RELU, blocks=16384, strides_loop=True),      # 4 227 072 source elements
    _ap("capped-f2", 2, 128, 128, 129, 2, LRELU, blocks=16384, strides_loop=True),
]
AP_BY_NAME = {r.name: r for r in AP_ROWS}
assert len(AP_BY_NAME) == len(AP_ROWS)


@functools.lru_cache(maxsize=4)
def ap_inputs(name):
    r = AP_BY_NAME[name]
    return cbn_inputs(r.N, r.H, r.W, r.C, r.f, r.act, r.bias, r.bn, 3000 + [q.name for q in AP_ROWS].index(name))


# ---- gode_cbn_bwd
TRAIN, EVAL, DIRECT, DIRECT_NOSUMS = "train", "eval", "direct+dbias", "direct-no-sums"
BwRow = collections.namedtuple("BwRow", "name N H W C f act mode dgb dbias gadd TP groups nblk chunk last strides_loop")


def _bw(name, N, H, W, C_, f, act, mode, TP, groups, nblk, chunk, last, dgb=True, dbias=True, gadd=True, strides_loop=False):
    """mode: BatchNorm train / eval, or direct (mean == NULL) with or without dbias.  dgb / dbias / gadd False: that pointer is
    NULL.  TP, groups, nblk, chunk, last (positions of the last chunk): what the launcher must make of the row."""
    if mode in (DIRECT, DIRECT_NOSUMS):
        dgb, dbias = False, mode == DIRECT
    return BwRow(name, N, H, W, C_, f, act, mode, dgb, dbias, gadd, TP, groups, nblk, chunk, last, strides_loop)


BW_ROWS = [
    _bw("one-chunk-8x8-c3", 3, 8, 8, 3, 2, RELU, TRAIN, 64, 1, 1, 64, 64),
    _bw("one-chunk-8x8-c257-eval", 1, 8, 8, 257, 1, LRELU, EVAL, 1, 2, 1, 64, 64),
    _bw("two-chunks-13x5-c1", 3, 13, 5, 1, 1, NONE, TRAIN, 256, 1, 2, 33, 32),
    _bw("two-chunks-13x5-c100-direct", 3, 13, 5, 100, 2, RELU, DIRECT, 2, 1, 2, 33, 32),
    _bw("two-chunks-13x5-c257", 3, 13, 5, 257, 2, RELU, TRAIN, 1, 2, 2, 33, 32),
    _bw("two-chunks-9x8-c3-direct-no-sums", 3, 9, 8, 3, 1, LRELU, DIRECT_NOSUMS, 64, 1, 2, 36, 36),
    _bw("two-chunks-9x8-c256-dgb-null", 1, 9, 8, 256, 1, RELU, TRAIN, 1, 1, 2, 36, 36, dgb=False),
    _bw("cap32-48x43-c3-dbias-null", 3, 48, 43, 3, 1, LRELU, TRAIN, 64, 1, 32, 65, 49, dbias=False),
    _bw("cap32-48x43-c100-eval-gadd-null", 1, 48, 43, 100, 2, NONE, EVAL, 2, 1, 32, 65, 49, gadd=False),
    _bw("direct-gadd-null", 3, 9, 8, 3, 2, NONE, DIRECT, 64, 1, 2, 36, 36, gadd=False),
    _bw("capped-pass2", 2, 128, 128, 129, 1, RELU, TRAIN, 1, 1, 32, 512, 512, strides_loop=True),   # 4 227 072 elements
]
BW_BY_NAME = {r.name: r for r in BW_ROWS}
assert len(BW_BY_NAME) == len(BW_ROWS)


@functools.lru_cache(maxsize=4)
def bw_inputs(name):
    """The row's inputs; `a` is the float64 apply reference rounded to fp32, so the backward rows do not depend on the apply
    kernel and the activation's branch is decided by an input."""
    r = BW_BY_NAME[name]
    bn = r.mode in (TRAIN, EVAL)
    x = cbn_inputs(r.N, r.H, r.W, r.C, r.f, r.act, True, bn, 4000 + [q.name for q in BW_ROWS].index(name), gadd=r.gadd)
    x["a"] = apply_reference(x, r.C, r.f, r.act)[0].float()
    return x


def bw_reference(r, x, dtype=f64):
    """gode_cbn_bwd's contract in `dtype` (sums in double), and for float64 the bounds, dict b_<output>.
        g   = the f x f sum of g_a, added in order from 0:    e_g  = (f f - 1) U sum|g_a|
        g_z = g, or g where a > 0 else 0 / 0.2 g:              e_gz = e_g + U |g_z| (leaky only)
      direct:  g_out = g_z + gadd: e_gz + U (|g_z| + |gadd|);  dbias = fp32(sum g_z): sum e_gz + U |dbias| + 1e-9 sum|g_z|
      BatchNorm:  xh as in apply_reference (e_xh = invstd e_v + 2U |xh|);  the s2 terms are fp32 products g_z xh:
        e_t = |xh| e_gz + |g_z| e_xh + U |g_z xh|
        dgb[n] = fp32(sum_p g_z xh | sum_p g_z): sum e_t + U |value| + 1e-9 sum|terms| (likewise with e_gz)
        S1 = sum_n gamma_n s1_n, S2 = sum_n gamma_n s2_n in double: E1 = sum_n |gamma_n| sum e_gz (+ 1e-9 ...), E2 with e_t
        eval:   dbias = invstd fp32(S1): invstd E1 + 2U |dbias|;     g_out = invstd (gamma g_z) + gadd:
                invstd |gamma| e_gz + 3U invstd |gamma g_z| + U |gadd|     (two products, the sum)
        train:  dbias = 0 exactly;  g_out = invstd (gamma g_z - fp32(S1/M) - xh fp32(S2/M)) + gadd,  T = |gamma g_z| + |S1/M| + |xh S2/M|:
                invstd (|gamma| e_gz + E1/M + e_xh |S2|/M + |xh| E2/M) + 6U invstd T + U |gadd|
                (inside the bracket: the product gamma g_z, two casts, the product xh c2 and two differences are at most 4U T;
                 invstd's product and the last sum 2U invstd T + U |gadd|)"""
    t = (lambda a: a.to(dtype))
    d = (lambda a: a.to(f64))
    C_, f, want = r.C, r.f, dtype == f64
    parts = _blocks(t(x["g_a"]), f)
    g = torch.zeros_like(parts[0])
    for part in parts:
        g = g + part
    av = _up_first(x["a"], f)
    gz = g if r.act == NONE else torch.where(av > 0, g, torch.zeros_like(g) if r.act == RELU else g * SLOPE)
    out = {}
    if want:
        e_gz = (f * f - 1) * U * sum(p.abs() for p in parts) + (U * gz.abs() if r.act == LRELU else 0.0)
        m_gz = gz.abs().sum((1, 2))
    s1 = d(gz).sum((1, 2))                                             # [N, C]
    if r.mode in (DIRECT, DIRECT_NOSUMS):
        out["g_out"] = gz + t(x["gadd"]) if r.gadd else gz
        if r.dbias:
            out["dbias"] = t(s1.sum(0))
        if want:
            out["b_g_out"] = e_gz + (U * (gz.abs() + d(x["gadd"]).abs()) if r.gadd else 0.0)
            out["b_dbias"] = e_gz.sum((0, 1, 2)) + U * s1.sum(0).abs() + TINY * m_gz.sum(0)
        return out
    M = r.N * r.H * r.W
    isd = t(x["invstd"])
    v = t(x["src"]) + t(x["bias"])
    xh = (v - t(x["mean"])) * isd
    term = gz * xh
    s2 = d(term).sum((1, 2))
    gam = x["gb"][:, :C_]
    S1, S2 = (d(gam) * s1).sum(0), (d(gam) * s2).sum(0)
    gx = t(gam)[:, None, None, :] * gz
    if r.mode == TRAIN:
        gx = gx - t(S1 / M) - xh * t(S2 / M)
        dbias = torch.zeros(C_, dtype=dtype, device=gz.device)
    else:
        dbias = isd * t(S1)
    go = isd * gx
    out["g_out"] = go + t(x["gadd"]) if r.gadd else go
    if r.dgb:
        out["dgb"] = t(torch.cat([s2, s1], 1))
    if r.dbias:
        out["dbias"] = dbias
    if not want:
        return out
    ga = d(gam).abs()
    e_xh = isd * _e_v(x) + 2 * U * xh.abs()
    e_t = xh.abs() * e_gz + gz.abs() * e_xh + U * term.abs()
    m_t = term.abs().sum((1, 2))
    se_gz, se_t = e_gz.sum((1, 2)) + TINY * m_gz, e_t.sum((1, 2)) + TINY * m_t
    out["b_dgb"] = torch.cat([se_t + U * s2.abs(), se_gz + U * s1.abs()], 1)
    E1, E2 = (ga * se_gz).sum(0), (ga * se_t).sum(0)
    gabs = ga[:, None, None, :] * gz.abs()
    egad = U * d(x["gadd"]).abs() if r.gadd else 0.0
    if r.mode == TRAIN:
        T = gabs + (S1 / M).abs() + (xh * (S2 / M)).abs()
        out["b_g_out"] = isd * (ga[:, None, None, :] * e_gz + E1 / M + e_xh * S2.abs() / M + xh.abs() * E2 / M) + 6 * U * isd * T + egad
        out["b_dbias"] = torch.zeros(C_, dtype=f64, device=gz.device)
    else:
        out["b_g_out"] = isd * ga[:, None, None, :] * e_gz + 3 * U * isd * gabs + egad
        out["b_dbias"] = isd * E1 + 2 * U * dbias.abs()
    return out


def bw_work_chunks(ws, N, H, W, C_):
    """The chunk count gode_cbn_bwd_work_size (gres.hip:295) was computed with."""
    num = (ws - N * H * W * C_) // 2 - 2 * N * C_ - 2 * C_
    assert num % (2 * N * C_) == 0
    return num // (2 * N * C_)


def bw_op(r, p, ss, gos):
    bn = r.mode in (TRAIN, EVAL)
    op = L.CbnBwdOp(g_a=p["g_a"], a=p["a"], src=p["src"] if bn else None, bias=p["bias"] if bn else None,
                    mean=p["mean"] if bn else None, invstd=p["invstd"] if bn else None, gb=p["gb"] if bn else None,
                    gadd=p["gadd"] if r.gadd else None, work=p["work"], dgb=p["dgb"] if r.dgb else None,
                    dbias=p["dbias"] if r.dbias else None, g_out=p["g_out"], N=r.N, H=r.H, W=r.W, C=r.C, f=r.f, act=r.act,
                    eval_mode=1 if r.mode == EVAL else 0)
    setv(op.ss, ss)
    setv(op.gos, gos)
    return op


# ---------------------------------------------------------------------------------------------------------------
# gode_gres_out / gode_gres_out_bwd
GoRow = collections.namedtuple("GoRow", "name N H W C f down b_main b_sc db g_main strides_loop db_rows")


def _go(name, N, H, W, C_, f, down, b_main=True, b_sc=True, db=True, g_main=None, strides_loop=False, db_rows=None):
    """b_main / b_sc / db / g_main False: that pointer is NULL (g_main is always NULL with down = 2).  db_rows: the rows of the
    bias gradient's statistics pass."""
    return GoRow(name, N, H, W, C_, f, down, b_main, b_sc, db, (down == 1) if g_main is None else g_main, strides_loop, db_rows)


GO_ROWS = [
    _go("f1-c3", 3, 5, 6, 3, 1, 1, db_rows=2),
    _go("f2-c257", 2, 5, 6, 257, 2, 1, db_rows=4),
    _go("pool-odd-7x5-c3", 3, 7, 5, 3, 1, 2, db_rows=1),                 # the last row and column are dropped
    _go("pool-c1", 2, 6, 6, 1, 1, 2, db_rows=1),
    _go("b-main-null", 3, 5, 6, 3, 2, 1, b_main=False, db_rows=6),
    _go("b-sc-null-pool", 3, 6, 6, 3, 1, 2, b_sc=False, db_rows=1),
    _go("db-null", 3, 5, 6, 3, 1, 1, db=False),
    _go("g-main-null-f2", 3, 5, 6, 3, 2, 1, g_main=False, db_rows=6),
    _go("capped", 2, 128, 128, 129, 1, 1, strides_loop=True, db_rows=512),     # 4 227 072 elements
    _go("db-rows-cap-1024", 1, 257, 256, 1, 1, 1, db_rows=1024),               # 65 792 positions: chunk 65, empty workgroups
]
GO_BY_NAME = {r.name: r for r in GO_ROWS}
assert len(GO_BY_NAME) == len(GO_ROWS)


@functools.lru_cache(maxsize=4)
def go_inputs(name):
    r = GO_BY_NAME[name]
    g = _gen(5000 + [q.name for q in GO_ROWS].index(name))
    Ho, Wo = out_dims(r.H, r.W, r.f, r.down)
    return dict(main=torch.randn(r.N, r.H * r.f, r.W * r.f, r.C, generator=g), sc=torch.randn(r.N, r.H, r.W, r.C, generator=g),
                b_main=torch.randn(r.C, generator=g), b_sc=torch.randn(r.C, generator=g), g_y=torch.randn(r.N, Ho, Wo, r.C, generator=g))


def _pool(t, Ho, Wo):
    """The four elements of every 2 x 2 window, in the kernel's order (e, e + dw, e + dh, e + dh + dw)."""
    return [t[:, i:2 * Ho:2, j:2 * Wo:2] for i in (0, 1) for j in (0, 1)]


def go_reference(r, x, dtype=f64):
    """y = (main + b_main) + (up_f(sc) + b_sc): three roundings, 2U (|main| + |b_main| + |sc| + |b_sc|) (a sum's rounding is
    within U of the magnitudes under it).  Pooled: 0.25 (sum of the four (main + b_main)) + 0.25 (... sc ...): every term passes
    its bias sum, three additions and the last sum, the products by 0.25 are exact -- 5U times a quarter of the magnitudes."""
    t = (lambda a: a.to(dtype))
    bm = t(x["b_main"]) if r.b_main else torch.zeros(r.C, dtype=dtype, device=x["main"].device)
    bs = t(x["b_sc"]) if r.b_sc else torch.zeros(r.C, dtype=dtype, device=x["main"].device)
    mag = (lambda a, b: a.abs().to(f64) + b.abs().to(f64))
    if r.down == 1:
        up = (lambda a: a.repeat_interleave(r.f, 1).repeat_interleave(r.f, 2) if r.f > 1 else a)
        y = (t(x["main"]) + bm) + (up(t(x["sc"])) + bs)
        return y, 2 * U * (mag(x["main"], bm) + up(mag(x["sc"], bs)))
    Ho, Wo = out_dims(r.H, r.W, r.f, r.down)
    tot, m = [], 0.0
    for src, b in ((x["main"], bm), (x["sc"], bs)):
        q = [p + b for p in _pool(t(src), Ho, Wo)]
        tot.append(((q[0] + q[1]) + q[2]) + q[3])
        m = m + sum(mag(p, b) for p in _pool(src, Ho, Wo))
    return 0.25 * tot[0] + 0.25 * tot[1], 5 * U * 0.25 * m


def go_bwd_reference(r, x, dtype=f64):
    """g_main = g_y (exact); g_sc = the f x f sum of g_y in order from 0, (f f - 1) U sum|g_y| -- exact for f = 1 -- or, pooled,
    0.25 g_y (exact) on the window's four elements and exact zeros on a dropped last row / column; db = fp32(sum over the rows of
    fp32 partial sums): U sum|partials| + U |db| + 1e-9 sum|g_y|."""
    t = (lambda a: a.to(dtype))
    gy = t(x["g_y"])
    out = {}
    if r.down == 1:
        parts = _blocks(gy, r.f)
        s = torch.zeros_like(parts[0])
        for p in parts:
            s = s + p
        out["g_sc"], out["b_g_sc"] = s, (r.f * r.f - 1) * U * sum(p.abs().to(f64) for p in parts)
        if r.g_main:
            out["g_main"], out["b_g_main"] = gy, torch.zeros_like(gy, dtype=f64)
    else:
        Ho, Wo = gy.shape[1:3]
        s = torch.zeros(r.N, r.H, r.W, r.C, dtype=dtype, device=gy.device)
        s[:, :2 * Ho, :2 * Wo] = (0.25 * gy).repeat_interleave(2, 1).repeat_interleave(2, 2)
        out["g_sc"], out["b_g_sc"] = s, torch.zeros_like(s, dtype=f64)
    if r.db:
        rows = chstats_rows(gy.shape[0] * gy.shape[1] * gy.shape[2])
        part, _ = ch_reference(x["g_y"], rows)
        p1 = part[0] if dtype == f64 else part[0].float().to(f64)           # the partials are stored as fp32
        out["db"] = t(p1.sum(1))
        out["b_db"] = U * part[0].abs().sum(1) + U * part[0].sum(1).abs() + TINY * x["g_y"].abs().to(f64).sum((0, 1, 2))
    return out


def go_ops(r, p, gys):
    fwd = L.GresOutOp(main=p["main"], sc=p["sc"], b_main=p["b_main"] if r.b_main else None, b_sc=p["b_sc"] if r.b_sc else None,
                      y=p["y"], N=r.N, H=r.H, W=r.W, C=r.C, f=r.f, down=r.down)
    bwd = L.GresOutBwdOp(g_y=p["g_y"], g_sc=p["g_sc"], g_main=p["g_main"] if r.g_main else None, db=p["db"] if r.db else None,
                         work=p["work"] if r.db else None, N=r.N, H=r.H, W=r.W, C=r.C, f=r.f, down=r.down)
    setv(bwd.gys, gys)
    return fwd, bwd


# ---------------------------------------------------------------------------------------------------------------
# gode_sn_fwd / gode_sn_bwd
SnRow = collections.namedtuple("SnRow", "name h w dot_blocks span ew_blocks strides_loop")
SN_ROWS = [
    SnRow("h1", 1, 5, 1, 5, 1, False),
    SnRow("w1", 5, 1, 1, 5, 1, False),
    SnRow("h4-w64-one-wave-trip", 4, 64, 1, 256, 1, False),
    SnRow("h5-w65-second-row-block", 5, 65, 1, 325, 2, False),
    SnRow("w256-one-column-block", 3, 256, 1, 768, 3, False),
    SnRow("w257-second-column-block", 3, 257, 1, 771, 4, False),
    SnRow("dot-one-block", 32, 32, 1, 1024, 4, False),
    SnRow("dot-63-blocks", 252, 256, 63, 1024, 252, False),
    SnRow("dot-64-blocks-exact", 256, 256, 64, 1024, 256, False),
    SnRow("dot-cap-span-1028", 257, 256, 64, 1028, 257, False),
    SnRow("elementwise-cap-1024", 513, 512, 64, 4104, 1024, True),      # 262 656 elements > 1024 * 256
]
SN_BY_NAME = {r.name: r for r in SN_ROWS}


@functools.lru_cache(maxsize=4)
def sn_inputs(name):
    r = SN_BY_NAME[name]
    g = _gen(6000 + [q.name for q in SN_ROWS].index(name))
    l2n = (lambda v: v / (v.norm() + 1e-12))
    return dict(wbar=torch.randn(r.h, r.w, generator=g), u=l2n(torch.randn(r.h, generator=g)), v=l2n(torch.randn(r.w, generator=g)),
                G=torch.randn(r.h, r.w, generator=g))


def _l2n(x, e_x, dtype):
    """out = x / (fp32(|x|) + 1e-12): (out, its error bound, |x|).  The norm is a double sum, a double square root and one cast:
    relative error rho = sum|x| e_x / |x|^2 + U; adding 1e-12 and dividing are two more roundings."""
    n = x.to(f64).norm()
    if dtype == f64:
        out = x / (n + 1e-12)
        rho = float((x.abs() * e_x).sum() / (n * n)) + U
        return out, e_x / n + out.abs() * (rho + 2 * U)
    return x / (n.float() + torch.tensor(1e-12, dtype=f32)), None


def sn_fwd_reference(x, dtype=f64):
    """One power iteration (gres_ref.sn_step's), with an error bound carried through it for float64:
        t = wbar^T u, a double sum cast once: e_t = U |t| + 1e-9 |wbar|^T |u|;   v = l2n(t) (see _l2n)
        s = wbar v:  e_s = |wbar| e_v + U |s| + 1e-9 |wbar| |v|;                 u = l2n(s)
        sigma = fp32(sum u_i s_i) over the fp32 u and s: sum(|u| e_s + |s| e_u) + U |sigma| + 1e-9 sum|u s|
        wout = wbar / sigma: |wout| (e_sigma / sigma + U)"""
    W = x["wbar"].to(f64)
    if dtype == f64:
        A = W.abs()
        t = W.t() @ x["u"].to(f64)
        e_t = U * t.abs() + TINY * (A.t() @ x["u"].to(f64).abs())
        v, e_v = _l2n(t, e_t, f64)
        s = W @ v
        e_s = A @ e_v + U * s.abs() + TINY * (A @ v.abs())
        u, e_u = _l2n(s, e_s, f64)
        sigma = u.dot(s)
        e_sig = (u.abs() * e_s + s.abs() * e_u).sum() + U * sigma.abs() + TINY * (u * s).abs().sum()
        wout = W / sigma
        return dict(v=v, u=u, sigma=sigma.reshape(1), wout=wout), dict(v=e_v, u=e_u, sigma=e_sig.reshape(1),
                                                                         wout=wout.abs() * (e_sig / sigma.abs() + U))
    t = (W.t() @ x["u"].to(f64)).float()
    v, _ = _l2n(t, None, f32)
    s = (W @ v.to(f64)).float()
    u, _ = _l2n(s, None, f32)
    sigma = u.to(f64).dot(s.to(f64)).float()
    return dict(v=v, u=u, sigma=sigma.reshape(1), wout=x["wbar"] / sigma), None


def sn_bwd_inputs(x):
    """The backward's u, v, sigma: the float64 forward reference rounded to fp32, and sigma = fp32(u . wbar v) of those rounded
    vectors in double -- so the backward rows do not depend on the forward kernel."""
    ref, _ = sn_fwd_reference(x)
    u, v = ref["u"].float(), ref["v"].float()
    sigma = u.to(f64).dot(x["wbar"].to(f64) @ v.to(f64)).float().reshape(1)
    return dict(G=x["G"], wbar=x["wbar"], u=u, v=v, sigma=sigma)


def sn_bwd_reference(b, dtype=f64):
    """Float64: autograd through sigma = u . (wbar v) with u and v constant.  The kernel's sigma input is that value rounded to
    fp32 (relative U): dwbar = G / s - k u_r v_c, k = fp32(dot / s^2).  G / s: the input's U and the division, 2U |G / s|.
    k: the input's 2U and the cast, and 1e-9 for the double sum; the products u v and k (u v): 2 more, 5U |k u v|; the
    difference's rounding is within U (|G / s| + |k u v|).  Together 3U |G / s| + 6U |k u v| + 1e-9 sum|G wbar| / s^2 |u v|."""
    G, W, u, v = (b[k].to(f64) for k in ("G", "wbar", "u", "v"))
    if dtype == f64:
        wb = W.clone().requires_grad_(True)
        (wb / u.dot(wb.mv(v)) * G).sum().backward()
        s = u.dot(W @ v)
        uv = torch.outer(u, v).abs()
        k = (G * W).sum() / (s * s)
        bound = 3 * U * (G / s).abs() + 6 * U * k.abs() * uv + TINY * (G * W).abs().sum() / (s * s) * uv
        return wb.grad, bound
    s = b["sigma"][0]
    k = ((G * W).sum() / (s.to(f64) * s.to(f64))).float()
    return b["G"] / s - k * (b["u"][:, None] * b["v"][None, :]), None


def sn_ops(r, p):
    fwd = L.SnOp(wbar=p["wbar"], u=p["u"], v=p["v"], wout=p["wout"], sigma=p["sigma"], work=p["work"], h=r.h, w=r.w)
    bwd = L.SnBwdOp(G=p["G"], wbar=p["wbar"], u=p["u_in"], v=p["v_in"], sigma=p["sigma_in"], dwbar=p["dwbar"], work=p["work2"], h=r.h, w=r.w)
    return fwd, bwd


# ---------------------------------------------------------------------------------------------------------------
# the block-level case with more than one position chunk (tests/test_gpu_gres.py): the second norm has HW = 18 x 16 = 288,
# five chunks of 58 (the last of 56), and its statistics 2 x 288 / 64 = 9 rows.  The seed is chosen in
# tests/test_host_gres_cells.py so that no pre-activation lies near the ReLU kink.
BLOCK_CASE = dict(cin=3, cout=10, bt=2, map=(9, 8), n_class=6, up=2, down=1, bn=True, seed=1)


def block_case_tensors(case=None):
    """(state dict of a freshly seeded reference block, x, condition, gy) of BLOCK_CASE, fp32 on the CPU."""
    import gres_ref
    case = case or BLOCK_CASE
    torch.manual_seed(case["seed"])
    blk = gres_ref.GResBlock(case["cin"], case["cout"], n_class=case["n_class"], bn=case["bn"], upsample_factor=case["up"],
                             downsample_factor=case["down"])
    H, W = case["map"]
    x = torch.randn(case["bt"], case["cin"], H, W)
    cond = torch.rand(case["bt"], case["n_class"])
    gy = torch.randn(case["bt"], case["cout"], H * case["up"], W * case["up"])
    return {k: v.clone() for k, v in blk.state_dict().items()}, x, cond, gy


def fake_ptrs(*names):
    """Distinct non-null aligned addresses for ops that must be refused before anything is read."""
    return {n: (k + 1) << 20 for k, n in enumerate(names)}
