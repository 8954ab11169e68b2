"""GPU: gode_bn_finalize against a NumPy float64 emulation of its documented order of additions.

Thread t of a channel's 256 adds its items t, t + 256, ... (item i = rep * rows + row of the segment, segments in order)
in double; the 256 partial sums go through the pairwise tree red[t] += red[t + s], s = 128 ... 1; the groups of a
two-batch launch are finalised in `order`, the second momentum update continuing from the first.  The epilogue is
emulated with exactly rounded fused multiply-adds where the kernel has them (var, shift, running_var) and with two rounded
products for running_mean, as the compiler contracts the kernel's expressions.  The emulation is bit-exact on the kernel,
every field and every case below (the double sqrt / divide included: no 1-ulp allowance is needed), so every field is
asserted bitwise: a change to the kernel that moves an addition, or a contraction, shows here."""
import zlib
from fractions import Fraction

import numpy as np
import pytest
import torch

import gan_ode_amd._lib as L

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64


def _f32_round(fr):
    """the float32 nearest to the exact rational fr, ties to even"""
    c = f32(float(fr))
    best = None
    for x in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
        err = abs(Fraction(float(x)) - fr)
        even = (int(np.array(x, dtype=f32).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, x)
    return f32(best[1])


def _fmaf(a, b, c):
    return _f32_round(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))      # (int / int: correctly rounded)


def _sums(pieces):
    """pieces: [(float32 [2][items])] per segment -> (s1, s2) through the per-thread sums and the tree"""
    acc = np.zeros((2, 256), dtype=f64)
    for items in pieces:
        n = items.shape[1]
        for k in range(0, n, 256):
            w = min(256, n - k)
            acc[:, :w] += items[:, k:k + w].astype(f64)
    s = 128
    while s > 0:
        acc[:, :s] += acc[:, s:2 * s]
        s >>= 1
    return acc[0, 0], acc[1, 0]


def _emulate(case, stats, stats1, gamma, beta, rm, rv, nbt):
    Cc, reps = case["C"], case["reps"]
    groups = case.get("groups", 1)
    out = {k: np.zeros((groups, Cc), dtype=f32) for k in ("mean", "invstd", "scale", "shift")}
    rm, rv = rm.copy(), rv.copy()
    mom, eps = f32(case["momentum"]), f32(case["eps"])
    order = [1, 0] if (groups == 2 and case.get("order", 0)) else list(range(groups))
    for c in range(Cc):
        for grp in order:
            src, segs = stats, [(0, case["rows"])]
            if groups == 2:
                if stats1 is not None:
                    if grp == 1:
                        src, segs = stats1, [(0, case["rows1"])]
                elif case.get("seg"):
                    sg = case["seg"]
                    segs = [(sg[3 * i], sg[3 * i + 1]) if grp == 0 else (sg[3 * i + 1], sg[3 * i + 2]) for i in range(len(sg) // 3)]
                else:
                    segs = [(0, case["rows0"])] if grp == 0 else [(case["rows0"], case["rows"])]
            pieces = [np.stack([src[w, c::Cc, lo:hi].reshape(-1) for w in range(2)]) for lo, hi in segs]   # rep-major items
            s1, s2 = _sums(pieces)
            n = f64(case["count1"] if (grp == 1 and case.get("count1", 0) > 0) else case["count"])
            mean = f64(s1) / n
            var = max(_fma(-mean, mean, f64(s2) / n), 0.0)
            invstd = f32(f64(1.0) / np.sqrt(f64(var) + f64(eps)))
            g = gamma[c] if gamma is not None else f32(1)
            b = beta[c] if beta is not None else f32(0)
            sc = f32(g * invstd)
            out["mean"][grp, c], out["invstd"][grp, c], out["scale"][grp, c] = f32(mean), invstd, sc
            out["shift"][grp, c] = _fmaf(-f32(mean), sc, b)
            unbiased = f64(var) * n / (n - f64(1.0)) if n > 1.0 else f64(var)
            keep = f32(f32(1) - mom)
            rm[c] = f32(f32(keep * rm[c]) + f32(mom * f32(mean)))
            rv[c] = _fmaf(mom, f32(unbiased), f32(keep * rv[c]))
    return out, rm, rv, nbt + groups


def _case(rows, reps, C_=3, **kw):
    return dict(rows=rows, reps=reps, C=C_, momentum=0.1, eps=1e-5, **kw)


CASES = {
    "1x1": _case(1, 1),
    "convT0_4x16": _case(4, 16, 8),
    "255": _case(255, 1),
    "256": _case(256, 1),
    "257": _case(257, 1),
    "4096x1": _case(4096, 1, 2),
    "51x5": _case(51, 5),                       # 255 items over several reps
    "3x200": _case(3, 200, 2),                  # rows < 256: a step of 256 items is 85 reps and one row, with carries
    "100x7": _case(100, 7, 5),
    "300x3": _case(300, 3, 2),                  # rows > 256: the row index wraps on most steps
    "rows0_o0": _case(300, 2, groups=2, rows0=130, order=0, count1=77),
    "rows0_o1": _case(300, 2, groups=2, rows0=130, order=1, count1=77),
    "seg4_o0": _case(700, 3, groups=2, seg=(0, 100, 150, 150, 400, 420, 420, 420, 500, 500, 690, 700), order=0, count1=500),
    "seg4_o1": _case(40, 3, groups=2, seg=(0, 3, 5, 5, 5, 9, 9, 20, 20, 20, 31, 40), order=1, count1=31),
    "stats1_o0": _case(300, 2, groups=2, rows1=70, order=0, count1=900),
    "stats1_o1": _case(300, 2, groups=2, rows1=70, order=1, count1=900),
    "no_affine": _case(257, 2, affine=False),
    "no_affine_2": _case(64, 1, groups=2, rows0=20, order=1, count1=50, affine=False),
}


def _run(case, training=1):
    rng = np.random.default_rng(zlib.crc32(repr(sorted(case.items())).encode()))
    Cc, reps, rows, groups = case["C"], case["reps"], case["rows"], case.get("groups", 1)
    ncols = Cc * reps

    def partials(r):      # rows of (sum, sum of squares) over 5 samples each, as a GEMM epilogue delivers them
        y = (rng.standard_normal((5, ncols, r)) * 2 + 1).astype(f32)
        return np.stack([y.sum(0), (y * y).sum(0)]).astype(f32)
    stats = partials(rows)
    stats1 = partials(case["rows1"]) if "rows1" in case else None
    affine = case.get("affine", True)
    gamma = (rng.random(Cc) + 0.5).astype(f32) if affine else None
    beta = rng.standard_normal(Cc).astype(f32) if affine else None
    rm0, rv0 = rng.standard_normal(Cc).astype(f32), (rng.random(Cc) + 0.5).astype(f32)
    count = 5 * rows * reps
    case = dict(case, count=count)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()      # noqa: E731
    st, st1, ga, be = dev(stats), dev(stats1), dev(gamma), dev(beta)
    rm, rv = dev(rm0), dev(rv0)
    nbt = torch.full((), 7, dtype=torch.int64, device="cuda")
    d = {k: torch.full((groups, Cc), float("nan"), device="cuda") for k in ("mean", "invstd", "scale", "shift")}
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    op = L.BnFinalizeOp(stats=st.data_ptr(), rows=rows, ncols=ncols, C=Cc, count=count, gamma=ptr(ga), beta=ptr(be),
                        running_mean=rm.data_ptr(), running_var=rv.data_ptr(), num_batches_tracked=nbt.data_ptr(),
                        mean=d["mean"].data_ptr(), invstd=d["invstd"].data_ptr(), scale=d["scale"].data_ptr(),
                        shift=d["shift"].data_ptr(), momentum=case["momentum"], eps=case["eps"], training=training,
                        groups=groups if groups == 2 else 0, rows0=case.get("rows0", 0), order=case.get("order", 0),
                        count1=case.get("count1", 0), stats1=ptr(st1), rows1=case.get("rows1", 0))
    sg = case.get("seg", ())
    op.nseg = len(sg) // 3
    for i, v in enumerate(sg):
        op.seg[i] = v
    L.run_one(op, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    got.update(running_mean=rm.cpu().numpy(), running_var=rv.cpu().numpy(), num_batches_tracked=int(nbt))
    return case, got, (stats, stats1, gamma, beta, rm0, rv0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_training_matches_the_documented_order_bitwise(name):
    case, got, (stats, stats1, gamma, beta, rm0, rv0) = _run(CASES[name])
    want, rm, rv, nbt = _emulate(case, stats, stats1, gamma, beta, rm0, rv0, 7)
    for k in ("mean", "invstd", "scale", "shift"):
        print(k, "max |diff|:", float(np.abs(got[k].astype(f64) - want[k].astype(f64)).max()))
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert np.array_equal(_bits(got["running_mean"]), _bits(rm)), "running_mean"
    assert np.array_equal(_bits(got["running_var"]), _bits(rv)), "running_var"
    assert got["num_batches_tracked"] == nbt


@pytest.mark.parametrize("groups", [1, 2])
def test_eval_mode_uses_the_running_statistics(groups):
    base = _case(9, 2, 8) if groups == 1 else _case(9, 2, 8, groups=2, rows0=4)
    case, got, (_, _, gamma, beta, rm0, rv0) = _run(base, training=0)
    invstd = (f32(1) / np.sqrt(rv0 + f32(case["eps"]))).astype(f32)
    sc = (gamma * invstd).astype(f32)
    shift = np.array([_fmaf(-sc[c], rm0[c], beta[c]) for c in range(case["C"])], dtype=f32)
    for grp in range(groups):
        assert np.array_equal(_bits(got["mean"][grp]), _bits(rm0)) and np.array_equal(_bits(got["invstd"][grp]), _bits(invstd))
        assert np.array_equal(_bits(got["scale"][grp]), _bits(sc)) and np.array_equal(_bits(got["shift"][grp]), _bits(shift))
    assert np.array_equal(_bits(got["running_mean"]), _bits(rm0)) and np.array_equal(_bits(got["running_var"]), _bits(rv0))
    assert got["num_batches_tracked"] == 7
