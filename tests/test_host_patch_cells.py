"""CPU: every shape of tests/patch_cells.py gets exactly the plan written there, and the shapes together reach every
instantiation of the two LDS-patch kernels and every launch form listed below.  The plans come from a stand-alone C++ program
(tests/hostcheck/patch_plan_check.cpp, its own main: conv_patch_plan of igemm_plan.h, wgrad_make_plan of wgrad_plan.h) built
here with AddressSanitizer + UBSan and run as a child process over the table's rows, which it reads from stdin -- so
patch_cells.py is the only list and no golden changes.  The library's own answers (gode_igemm_launch_cell,
gode_wgrad_work_size) are asked through ctypes over fake pointers of each cell's alignment.  A planner change that moves a
shape off its kernel, or off the second table chunk, fails here by name instead of silently thinning
tests/test_gpu_patch_cells.py, which runs the same cells on the GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import REPO

import gan_ode_amd._lib as L
import igemm_cells as I
import patch_cells as T
import test_gpu_patch_cells as G      # (its references and bounds are plain CPU code)
from gan_ode_amd.engine import make_geom

SRC = os.path.join(REPO, "tests", "hostcheck", "patch_plan_check.cpp")
WGRAD_PLAN_H = os.path.join(REPO, "gan-ode_amd", "csrc", "wgrad_plan.h")
K_PATCH = I.KERNELS.index("patch")
WG_PATCH = 0
CP_TAB_ITERS, WP_TAB = 32, 128       # iterations / slabs per chunk of the kernels' 128-entry LDS tables (CP_TAB / 4, WP_TAB)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """name -> (kind, fields) of every line the program prints for the table: the shapes, the cells, the declined ops."""
    exe = str(tmp_path_factory.mktemp("patch_plan") / "patch_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe])
    lines = [T.plan_line("F:" + s, s, "fprop") for s in T.SHAPES] + [T.plan_line("W:" + s, s, "wgrad") for s in T.SHAPES]
    lines += [T.cell_line(c) for c in T.CELLS]
    lines += [T.plan_line("D:" + name, s, "fprop", stats=stats, xform=int(xf), act=T.ACT_LRELU if xf else T.ACT_NONE, tile=tile)
              for name, s, stats, xf, tile in T.DECLINED]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GODE_WGRAD_")}
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        name, kind, *rest = line.split(" ")
        f = dict(kv.split("=", 1) for kv in rest if "=" in kv)
        f["declined"] = rest[-1] == "no"
        out[name] = (kind.rstrip(":"), f)
    assert len(out) == len(lines)
    return out


def _fplan(f):
    return None if f["declined"] else T.FPlan(*(int(f[k]) for k in T.FPlan._fields))


def _wplan(f):
    return None if f["declined"] else T.WPlan(*(int(f[k]) for k in T.WPlan._fields))


def _geom(shape):
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    return make_geom(N, Ci, Co, xi, T.out_extent(shape), k, s, p)


def _kt(shape):
    N, Ci, Co, xi, k, s, p = T.SHAPES[shape]
    return k[0] * k[1] * k[2] * Ci


def test_every_shape_gets_its_plan(plans):
    for s in T.SHAPES:
        assert _fplan(plans["F:" + s][1]) == T.FPROP_PLANS.get(s), s
    for s in T.WGRAD_PLANS:
        assert _wplan(plans["W:" + s][1]) == T.WGRAD_PLANS[s], s
    for s in T.WGRAD_DECLINED:
        assert s in T.FPROP_PLANS and plans["W:" + s][1]["path"] == "2"       # the forward kernel takes it, the weight gradient is a tiled GEMM
    # a cell's layout and offsets move no plan, and the program's launch cell of a forward cell is the patch kernel
    for c in T.CELLS:
        kind, f = plans[c.name]
        assert kind == c.kernel
        if c.kernel == "fprop":
            assert _fplan(f) == T.FPROP_PLANS[c.shape] and f["cell"] == f"{K_PATCH}/0", c.name
        else:
            assert _wplan(f) == T.WGRAD_PLANS[c.shape] and int(f["path"]) == WG_PATCH, c.name
            assert int(f["vy"]) == (c.y == 0), c.name
            assert int(f["work_size"]) == int(f["work_floats"]) == int(f["splits"]) * T.SHAPES[c.shape][2] * _kt(c.shape)
            # PL = kw * Ci (mod 32), and the kernel's two buffers [patch | 32 x Co | dump slot]
            N, Ci, Co, xi, k, s, p = T.SHAPES[c.shape]
            assert int(f["PL"]) % 32 == (k[2] * Ci) % 32 and int(f["PL"]) >= int(f["LW"]) * Ci
            assert int(f["lds_bytes"]) == 2 * (int(f["PR"]) * int(f["PL"]) + 32 * Co + 4) * 4 <= 64 * 1024


def test_forward_shapes_reach_every_instantiation_and_column_count():
    have = {(p.variant, p.CB) for p in T.FPROP_PLANS.values()}
    assert have == {(v, cb) for v in T.VARIANTS for cb in (1, 2, 4)}
    for s, p in T.FPROP_PLANS.items():
        N, Ci, Co, xi, k, st, pad = T.SHAPES[s]
        assert (k[0], k[1], k[2] * Ci // 2) == T.VARIANTS[p.variant] and p.CB == Co // 32 and p.SPI == 4 // p.CB, s
    # the instantiations are keyed on kw * Ci / 2: each (kw, Ci) pair that shares one
    pairs = {(p.variant, T.SHAPES[s][4][2], T.SHAPES[s][1]) for s, p in T.FPROP_PLANS.items()}
    assert pairs == {(1, 4, 3), (2, 4, 3), (2, 3, 4), (3, 2, 1), (4, 4, 1), (4, 2, 2)}
    # every instantiation in every x layout and with x one float off
    for v in T.VARIANTS:
        for want in (dict(layout="ncdhw"), dict(layout="pad1"), dict(src=1)):
            assert any(c.kernel == "fprop" and T.FPROP_PLANS[c.shape].variant == v and all(getattr(c, k) == x for k, x in want.items())
                       for c in T.CELLS), (v, want)


def test_weight_gradient_shapes_reach_every_instantiation():
    with open(WGRAD_PLAN_H) as f:
        text = f.read().replace("\\\n", " ")
    macro = re.search(r"#define WGRAD_PATCH_KERNELS\(X\)(.*)", text).group(1)
    kernels = {(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", macro)}
    assert len(kernels) == 12
    assert {(p.nbw, T.SHAPES[s][2]) for s, p in T.WGRAD_PLANS.items()} == kernels
    for s, p in T.WGRAD_PLANS.items():
        Co = T.SHAPES[s][2]
        assert p.RB == Co // 32 and p.CB == -(-_kt(s) // 32) and p.nbw == -(-p.CB // (4 // p.RB)) and _kt(s) > 16, s
    wc = [c for c in T.CELLS if c.kernel == "wgrad"]
    co = lambda c: T.SHAPES[c.shape][2]         # noqa: E731
    for Co in (32, 64, 128):
        for want in (dict(layout="ncdhw"), dict(layout="pad1"), dict(src=1), dict(xform=True), dict(xform=True, scale=1)):
            assert any(co(c) == Co and all(getattr(c, k) == x for k, x in want.items()) for c in wc), (Co, want)
    assert {co(c) for c in wc if c.y == 1} >= {32, 128}
    assert any(c.layout != "cl" and T.SHAPES[c.shape][4][0] > 1 for c in wc)          # a depth stride that is not the channels-last one


def test_rows_reach_every_launch_form(plans):
    fp, wp = T.FPROP_PLANS, T.WGRAD_PLANS
    wo = lambda s: T.out_extent(s)[2]           # noqa: E731
    for table in (fp, wp):
        assert {p.nseg for p in table.values()} == {1, 2}
        assert {"d-", "d+", "h-", "h+", "w-", "w+"} == set().union(*(T.padded_sides(s) for s in table))
        assert all(p.nseg == -(-wo(s) // 32) for s, p in table.items())
    assert {min(wo(s) % 32, 2) for s in fp} == {0, 1, 2}                     # whole segments, a segment of one position, a partial one
    assert {T.SHAPES[s][5][2] for s in fp} == {1, 2, 3}                      # sw
    assert {T.SHAPES[s][5][2] for s in wp} == {1, 2}
    assert any(p.segs % p.SPI != 0 for p in fp.values())                     # table slots past the last slab
    nit = lambda p: -(-p.segs // p.SPI)         # noqa: E731
    assert all(p.wgs == -(-nit(p) // p.iters_per_wg) for p in fp.values())
    assert any(nit(p) % p.iters_per_wg != 0 and p.wgs > 1 for p in fp.values())       # a last workgroup with fewer iterations
    assert all(p.splits == -(-p.segs // p.segs_per_wg) for p in wp.values())
    assert any(p.segs % p.segs_per_wg != 0 and p.splits > 1 for p in wp.values())     # ... with fewer slabs
    # the second chunk of the 128-entry table: only the two big shapes, by one iteration / one slab
    assert {s for s, p in fp.items() if p.iters_per_wg > CP_TAB_ITERS} == {"f_chunk2"} and fp["f_chunk2"].iters_per_wg == CP_TAB_ITERS + 1
    assert {s for s, p in wp.items() if p.segs_per_wg > WP_TAB} == {"w_chunk2"} and wp["w_chunk2"].segs_per_wg == WP_TAB + 1
    assert T.BIG == {"f_chunk2", "w_chunk2"}
    # all three reduce kernels behind the patch kernel; the cell with work one float off leaves the float4 reduce for the scalar one
    reduce_of = lambda name: int(plans[name][1]["reduce"])       # noqa: E731
    assert {reduce_of(c.name) for c in T.CELLS if c.kernel == "wgrad"} == {0, 1, 2}
    off = [c for c in T.CELLS if c.work == 1]
    assert off and all(reduce_of(c.base) == 1 and reduce_of(c.name) == 2 for c in off)


def test_every_declined_op_is_declined(plans):
    for name, s, stats, xf, tile in T.DECLINED:
        f = plans["D:" + name][1]
        assert f["declined"] and not f["cell"].startswith(f"{K_PATCH}/") and not f["cell"].startswith("rc="), name
    assert {"d_mnist_video", "d_mnist_image", "d_patch8", "d_lwc", "d_k3"} <= {s for _, s, *_ in T.DECLINED}
    assert T.SHAPES["d_patch8"] == I.SHAPES["patch8"] and T.SHAPES["f2d3_64"] == I.SHAPES["patch"]
    # why: an output row under 16 positions (both MNIST first layers), more staged columns than CP_MAXCOL per thread, odd kw * Ci
    assert [T.out_extent(s)[2] for s in ("d_mnist_video", "d_mnist_image", "d_patch8")] == [15, 14, 8]
    N, Ci, Co, xi, k, s, p = T.SHAPES["d_lwc"]
    assert (31 * s[2] + k[2]) * Ci > 2 * (256 // (4 // (Co // 32))) and T.out_extent("d_lwc")[2] >= 16
    assert (T.SHAPES["d_k3"][4][2] * T.SHAPES["d_k3"][1]) % 2 == 1
    # the one-channel instantiations are reached by one-channel inputs with Wo >= 16 only
    assert all(T.out_extent(s)[2] >= 16 for s in T.FPROP_PLANS)


def _igemm_op(shape, layout="cl", src=0, stats=False, xform=False, tile=0):
    base = 1 << 20
    op = L.IgemmOp(g=_geom(shape), dir=L.FPROP, act=L.ACT_LRELU if xform else L.ACT_NONE, epilogue=L.EPI_RAW, tile=tile, src=base + 4 * src,
                   wpack=2 * base, out=3 * base, scale=4 * base if xform else None, shift=5 * base if xform else None,
                   stats=6 * base if stats else None, work=7 * base, groups=1, border=0)
    gs, _ = T.x_strides(shape, layout)
    for i in range(5):
        op.gs[i] = gs[i] if gs else 0
    return op


def test_library_reports_the_patch_cell_for_every_forward_cell_and_for_no_declined_op():
    for c in T.CELLS:
        if c.kernel == "fprop":
            assert I.cell_label(_igemm_op(c.shape, c.layout, c.src)) == "patch", c.name
    for name, s, stats, xf, tile in T.DECLINED:
        label = I.cell_label(_igemm_op(s, stats=stats, xform=xf, tile=tile))
        assert I.parse(label)["kernel"] in ("generic-scalar", "generic-vec4", "fast-xf", "fast-dma"), (name, label)
        assert I.parse(label)["tile"] is not None, (name, label)
    # what the MNIST first layers run
    assert I.cell_label(_igemm_op("d_mnist_video")).startswith("generic-scalar 128x64 ")
    assert I.cell_label(_igemm_op("d_mnist_image")).startswith("generic-scalar 128x64 ")


def test_library_work_size_is_splits_times_co_times_kt():
    lib = L.lib()
    base = 1 << 20
    for c in T.CELLS:
        if c.kernel != "wgrad":
            continue
        xf = c.xform
        op = L.WgradOp(g=_geom(c.shape), act=L.ACT_LRELU if xf else L.ACT_NONE, xform_on_y=int(xf), splits=0, accumulate=0,
                       x=base + 4 * c.src, y=2 * base + 4 * c.y, scale=3 * base + 4 * c.scale if xf else None,
                       shift=4 * base + 4 * c.scale if xf else None, dw=5 * base)
        assert lib.gode_wgrad_work_size(C.byref(op)) == T.WGRAD_PLANS[c.shape].splits * T.SHAPES[c.shape][2] * _kt(c.shape), c.name


def test_the_probe_of_w_chunk2_would_see_a_dropped_slab():
    """What the second run of w_chunk2 in tests/test_gpu_patch_cells.py is for, shown on the references alone: were the one
    slab of every workgroup's second table chunk (local index 128) dropped, nearly every element of dw would move by more than
    the probe's bound, and by less than the bound of the full run."""
    plan = T.WGRAD_PLANS["w_chunk2"]
    assert plan.segs_per_wg - 1 == WP_TAB >= G.PROBE_FROM + 2
    dropped, _ = G._wgrad_reference("w_chunk2", False, (WP_TAB, WP_TAB + 1))
    _, mag_probe = G._wgrad_reference("w_chunk2", False, G.PROBE)
    _, mag_full = G._wgrad_reference("w_chunk2", False)
    probe_bound = 2 * (32 * (plan.segs_per_wg - G.PROBE_FROM) + 2) * G.U * mag_probe
    full_bound = 2 * (32 * plan.segs_per_wg + 2) * G.U * mag_full
    assert float((dropped.abs() > 10 * probe_bound).double().mean()) > 0.95
    assert float((dropped.abs() < full_bound).double().mean()) > 0.5
