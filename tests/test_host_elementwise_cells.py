"""CPU: the rows of tests/elementwise_cells.py reach the branches of gan-ode_amd/csrc/elementwise.hip they name, and the
references and bounds tests/test_gpu_elementwise_cells.py holds the kernels to stand on their own.

gode_col2im: the op of every row, built over fake non-null pointers of the row's alignment (nothing dereferences them on the
host), reports the row's kind and reason through gode_col2im_launch_kind -- the plan gode_col2im itself dispatches on
(gan-ode_amd/csrc/col2im_plan.h); what the rows reach together is asserted from their geometry.  The fp32 emulation of the
overlap-add that the GPU test compares bit for bit is checked against float64 F.conv_transpose2d / 3d over identity tap weights:
an element with T taps lies within (T - 1) U sum|terms| of it (T - 1 fp32 additions, each within U of a partial sum that is at
most the sum of magnitudes), so the emulation is not the kernel's code agreeing with itself.

BatchNorm and Adam: an fp32 NumPy restatement of each update stays inside the per-element bounds around the float64 reference
(the bounds are derived, elementwise_cells.py; this shows that a correct fp32 evaluation passes them).  The refusals of
gode_bn_bwd return their codes without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import gan_ode_amd as G
import gan_ode_amd._lib as L
import elementwise_cells as T

U = T.U


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", T.C2_ROWS, ids=[r.name for r in T.C2_ROWS])
def test_col2im_row_reaches_its_kind(r):
    assert T.c2_kind(T.c2_fake_op(r)) == (r.kind, r.why)
    assert all(d >= 1 for d in T.c2_out_dims(r))
    # the same op on a 16-byte boundary (the twins' other half): only the alignment bit moves
    if r.off:
        kind, why = T.c2_kind(T.c2_op(r, 1 << 20, 2 << 20))
        assert why == r.why & ~T.WHY_COLS and kind == (T.ROWS_K if why == 0 else T.PIXEL)


def test_col2im_rows_cover_the_launcher():
    rows = T.C2_ROWS
    geo = {r.name: T.c2_geometry(r) for r in rows}
    two_d = [r for r in rows if len(r.xi) == 2]
    assert {r.kind for r in rows} == {T.ROWS_K, T.PIXEL, T.FIXED3D, T.GEN3D}
    assert {r.kind for r in two_d} == {T.ROWS_K, T.PIXEL} and {r.kind for r in rows if len(r.xi) == 3} == {T.FIXED3D, T.GEN3D}
    # the reasons, from the geometry: each reachable 2-D bit alone, and exactly when the launcher's condition holds
    for r in two_d:
        g = geo[r.name]
        why = (T.WHY_ROWLEN * (g["rowlen"] % 4 != 0) | T.WHY_COLS * (r.off % 4 != 0) | T.WHY_LDS * (g["lds"] > T.LDS_MAX)
               | T.WHY_GRID * (r.N * g["nq"] >= 2 ** 31))
        assert why == r.why and (r.kind == T.ROWS_K) == (why == 0), r.name
    assert {r.why for r in two_d} == {0, T.WHY_ROWLEN, T.WHY_COLS, T.WHY_LDS}
    for r in rows:
        if len(r.xi) == 3:
            why = (T.WHY_TAPS * ((r.k, r.s) != ((4, 4, 4), (1, 2, 2))) | T.WHY_CHANNELS * (r.C != 3)
                   | T.WHY_VOXELS * (geo[r.name]["outputs"] >= 2 ** 31))
            assert why == r.why and (r.kind == T.FIXED3D) == (why == 0), r.name
    assert {T.WHY_TAPS, T.WHY_CHANNELS} <= {r.why for r in rows if r.kind == T.GEN3D}
    # tanh on all four kernels, raw on all four
    assert {r.kind for r in rows if r.tanh} == {r.kind for r in rows if not r.tanh} == set(T.KINDS)
    by = T.C2_BY_NAME
    # the row-group kernel: a second iteration of the output loop and of the LDS fill; the LDS boundary from both sides
    rk = [r for r in rows if r.kind == T.ROWS_K]
    assert any(geo[r.name]["group"] > 256 for r in rk) and any(geo[r.name]["rowlen"] // 4 > 256 for r in rk)
    assert geo["rows-wide"]["group"] == 320 and geo["rows-longrow"]["rowlen"] // 4 == 272 and geo["rows-longrow"]["group"] == 272
    assert geo["rows-lds-at"]["lds"] == T.LDS_MAX == 49152 and geo["pix-lds-over"]["lds"] == 53248
    assert {geo[r.name]["R"] for r in rk} >= {1, 2, 3, 4}
    assert any(r.C == 1 for r in rk) and {r.C for r in rows if r.kind == T.GEN3D} >= {1, 2, 3, 4}
    an = by["rows-aniso"]
    assert an.k[0] != an.k[1] and an.s[0] != an.s[1] and an.p[0] != an.p[1] and an.k[0] % an.s[0] and an.k[1] % an.s[1]
    # kernel smaller than stride: output elements with no tap at all, which must come out 0
    for name in ("rows-k-lt-s", "gen-k-lt-s"):
        r = by[name]
        assert all(k < s for k, s in zip(r.k, r.s) if s > 1)
        assert int((T.c2_reference64(name)[2] == 0).sum()) > 0
    assert int((T.c2_reference64("rows-k-lt-s")[2] == 0).sum()) == 456
    assert T.c2_out_dims(by["rows-s1p2"]) < by["rows-s1p2"].xi                   # an output smaller than its input
    assert by["fixed-p1"].p[0] > 0 and by["fixed-p1"].kind == T.FIXED3D
    # both grid caps exceeded, by a few blocks
    assert geo["pix-cap"]["blocks"] == 8202 > T.PIXEL_BLOCKS and by["pix-cap"].kind == T.PIXEL
    assert geo["gen-cap"]["blocks"] == 16401 > T.GEN3D_BLOCKS and by["gen-cap"].kind == T.GEN3D
    assert all(geo[r.name]["blocks"] <= (T.PIXEL_BLOCKS if r.kind == T.PIXEL else T.GEN3D_BLOCKS)
               for r in rows if r.kind != T.ROWS_K and not r.name.endswith("-cap"))
    # the twins: the same row but for cols' offset
    for r in rows:
        if r.twin:
            assert r._replace(name="", off=0, kind=0, why=0, twin=None) == by[r.twin]._replace(name="", kind=0, why=0)
            assert by[r.twin].kind == T.ROWS_K and r.kind == T.PIXEL and r.why == T.WHY_COLS
    # only the cap rows are above 1 MB
    assert [r.name for r in rows if 4 * max(T.c2_cols_numel(r), T.c2_out_numel(r)) > 1 << 20] == ["pix-cap", "gen-cap"]


def test_col2im_refusals():
    r = T.C2_BY_NAME["rows-basic"]
    ok = T.c2_fake_op(r)
    assert T.c2_kind(ok) == (T.ROWS_K, 0)
    for field, value, code in [("cols", None, "E_ARG"), ("out", None, "E_ARG"), ("C", 5, "E_ARG"), ("C", 0, "E_ARG"), ("Ho", r.xi[0], "E_SHAPE"),
                               ("Wo", 1, "E_SHAPE"), ("epilogue", 2, "E_ARG"), ("sh", 0, "E_ARG"), ("ph", -1, "E_ARG")]:
        op = T.c2_fake_op(r)
        setattr(op, field, value)
        assert T.c2_kind(op) == code, field
    op3 = T.c2_fake_op(T.C2_BY_NAME["fixed-p0"])
    op3.Do += 1
    assert T.c2_kind(op3) == "E_SHAPE"
    assert L.lib().gode_col2im_launch_kind(C.byref(ok), None) == -1


@pytest.mark.parametrize("r", T.C2_ROWS, ids=[r.name for r in T.C2_ROWS])
def test_col2im_fp32_emulation_against_float64_conv_transpose(r):
    s32 = T.c2_sum32(r.name).double()
    ref, mag, cnt = T.c2_reference64(r.name)
    assert s32.shape == ref.shape == (r.N, *T.c2_out_dims(r), r.C)
    assert float(cnt.max()) <= np.prod([-(-k // s) for k, s in zip(r.k, r.s)])
    bound = (cnt - 1).clamp_min(0) * U * mag
    err = (s32 - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{r.name}: taps per element {int(cnt.min())}..{int(cnt.max())}, worst |fp32 - fp64| / bound = {worst:.2f}")
    assert bool((err <= bound).all()), worst
    assert bool((s32[cnt == 0] == 0).all())
    if r.tanh:
        assert float(s32.abs().max()) < 6.0          # unsaturated: tanh's slope is still above fp32's resolution


# ---------------------------------------------------------------------------------------------------------------
def _worst(err, bound):
    return float((np.abs(err) / (bound + 1e-300)).max())


def test_bn_bwd_rows_cover_the_launcher():
    shp = {r.name: T.bnb_launch_shape(r) for r in T.BNB_CASES if r.bn}
    a = shp["700x96-lrelu"]
    assert (a["CL"], a["cgroups"], a["dead"], a["chunks"], a["last"]) == (16, 2, 8, [3], [188])
    b = shp["257x8-relu"]
    assert (b["CL"], b["chunks"], b["last"]) == (2, [2], [1])
    assert shp["300x512-lrelu01"]["cgroups"] == 8
    c = shp["377x32-lrelu-g2-m0"]
    assert c["chunks"] == [2, 1] and c["last"] == [44, 77] and 300 % T.BNB_ROWS != 0 and 300 != 377 // 2
    assert shp["514x64-relu-g2"]["chunks"] == [2, 2] and T.bnb_group_rows(T.BNB_BY_NAME["514x64-relu-g2"]) == [(0, 257), (257, 514)]
    threads = T.EW_BLOCKS * 256
    assert shp["8200x512-lrelu"]["n4"] == 1049600 > threads
    assert all(s["n4"] <= threads for n, s in shp.items() if n != "8200x512-lrelu")
    nobn = [r for r in T.BNB_CASES if not r.bn]
    assert [(r.M * r.C, r.act) for r in nobn] == [(1048581, T.TANH_OUT), (35, T.NONE)] and 1048581 > threads
    assert any(r.eval_mode for r in T.BNB_CASES) and any(r.gin and r.accumulate and not r.gamma for r in T.BNB_CASES)
    assert {r.act for r in T.BNB_CASES} == {T.NONE, T.RELU, T.LRELU, T.LRELU01, T.TANH_OUT}
    # the work buffer the callers size covers both groups' chunks and coefficient sets
    lib = L.lib()
    for r in T.BNB_CASES:
        if r.bn:
            assert lib.gode_bn_bwd_work_size(r.M, r.C) >= sum(shp[r.name]["chunks"]) * 4 * r.C + 6 * r.C


@pytest.mark.parametrize("M,C_,groups,M0,code", T.BNB_REFUSALS)
def test_bn_bwd_refusals_before_any_launch(M, C_, groups, M0, code):
    op = T.bnb_fake_op(M, C_, groups, M0)
    assert T.ERRORS[L.lib().gode_bn_bwd(C.byref(op), None)] == code
    if code == "E_SHAPE":
        CL = min(C_ // 4, T.BNB_CL)
        assert C_ % 4 == 0 and 256 % CL != 0


@pytest.mark.parametrize("r", T.BNB_CASES, ids=[r.name for r in T.BNB_CASES])
def test_bn_bwd_fp32_restatement_inside_the_bounds(r):
    x = T.bnb_inputs(r.name)
    ref = T.bnb_reference(r, x)
    own = T.bnb_reference(r, x, np.float32)
    ratios = {k: _worst(own[k].astype(np.float64) - ref[k], ref["b_" + k]) for k in own}
    print(f"{r.name}: fp32 restatement / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k in own:
        assert (np.abs(own[k].astype(np.float64) - ref[k]) <= ref["b_" + k] + 1e-45).all(), (k, ratios[k])
    assert np.isfinite(ref["g_y"]).all()


@pytest.mark.parametrize("r", T.BNA_CASES, ids=[r.name for r in T.BNA_CASES])
def test_bn_apply_fp32_restatement_inside_the_bound(r):
    x = T.bna_inputs(r.name)
    ref, bound = T.bna_reference(r, x)
    own, _ = T.bna_reference(r, x, np.float32)
    print(f"{r.name}: fp32 restatement / bound: {_worst(own.astype(np.float64) - ref, bound):.3f}")
    assert (np.abs(own.astype(np.float64) - ref) <= bound).all()
    assert (r.M * r.C // 4 > T.APPLY_BLOCKS * 256) == (r.name == "66000x128-relu") and r.M * r.C // 4 in (74, 2112000)
    assert any(0 < q.M0 < q.M and (q.M0 * q.C // 4) % 256 != 0 for q in T.BNA_CASES)


def test_bn_finalize_row():
    x = T.bnf_inputs()
    ref, bound, var_raw = T.bnf_reference(x)
    assert x["stats"].shape == (2, T.BNF_REPS * T.BNF_C, T.BNF_ROWS) and T.BNF_REPS > 1 and T.BNF_ROWS * T.BNF_REPS > 256
    # the constant channel: a negative variance before the clamp (without it invstd would be NaN), the others far from it
    assert var_raw[T.BNF_CONST] < -0.01 and ref["invstd"][T.BNF_CONST] == 1.0 / np.sqrt(T.BNF_EPS)
    assert (np.delete(var_raw, T.BNF_CONST) > 0.1).all() and np.isfinite(list(ref.values())).all()
    assert float(ref["mean"][T.BNF_CONST]) == 1000.0
    # an fp32 evaluation from the double sums stays inside the bounds
    f = np.float32
    mean32 = ref["mean"].astype(f)
    is32 = ref["invstd"].astype(f)
    sc32 = x["gamma"] * is32
    own = dict(mean=mean32, invstd=is32, scale=sc32, shift=x["beta"] - mean32 * sc32,
               running_mean=(f(1) - f(T.BNF_MOMENTUM)) * x["running_mean"] + f(T.BNF_MOMENTUM) * mean32)
    for k, v in own.items():
        assert (np.abs(v.astype(np.float64) - ref[k]) <= bound[k]).all(), k


# ---------------------------------------------------------------------------------------------------------------
def test_adam_rows_cover_adam_tensor():
    paths = [T.adam_paths(k, n) for k, n in enumerate(T.ADAM_SIZES)]
    threads = T.ADAM_BLOCKS * 256
    assert T.ADAM_SIZES[7] == 2097159 > threads * 4 and T.ADAM_SIZES[8] == 524293 > threads
    # float4 body with a scalar tail, scalar only, each loop striding in one tensor, by a few items past one pass of the grid
    assert any(p["n4"] > 0 and 0 < p["scalar"] < 4 for p in paths) and any(p["n4"] == 0 and p["scalar"] > 256 for p in paths)
    assert [k for k, p in enumerate(paths) if p["vec_strides"]] == [7] and paths[7]["n4"] == threads + 1
    assert [k for k, p in enumerate(paths) if p["scalar_strides"]] == [8] and paths[8]["scalar"] == threads + 5
    offs, total = T.guarded_layout(T.ADAM_SIZES)
    assert all(o % 4 == (k + 1) % 2 for k, o in enumerate(offs)) and total > offs[-1] + T.ADAM_SIZES[-1]
    assert max(T.ADAM_L2_SIZES) > T.EW_BLOCKS * 256 and T.ADAM_L2_SIZES[:2] == [1003, 524293]


@pytest.mark.parametrize("gscale", T.ADAM_GSCALES)
def test_adam_fp32_restatement_inside_the_bounds(gscale):
    sizes = (1, 5, 64, 1003, 4096, 70001, 9)
    p0, m0, v0, g = T.adam_data(sizes)
    worst = np.zeros(3)
    for k in range(len(sizes)):
        p, m, v = p0[k].numpy(), m0[k].numpy(), v0[k].numpy()
        for s in range(T.ADAM_STEPS):
            ref, bnd = T.adam_reference(p, g[s][k].numpy(), m, v, gscale, s + 1)
            own = T.adam_restated32(p, g[s][k].numpy(), m, v, gscale, s + 1)
            for i in range(3):
                err = np.abs(own[i].astype(np.float64) - ref[i])
                assert (err <= bnd[i]).all(), (k, s, "pmv"[i], _worst(err, bnd[i]))
                worst[i] = max(worst[i], _worst(err, bnd[i]))
            p, m, v = own
    print(f"gscale {gscale}: fp32 restatement / bound over {T.ADAM_STEPS} steps: p {worst[0]:.2f}, m {worst[1]:.2f}, v {worst[2]:.2f}")
    # the coefficients are FusedAdam's
    for step in (1, 2, 3):
        c = T.adam_coefficients(step)
        assert (c["step_size"], c["bc2"]) == G.FusedAdam.step_coefficients(T.ADAM_HP["lr"], T.ADAM_HP["beta1"], T.ADAM_HP["beta2"], step)
