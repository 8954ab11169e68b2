"""CPU: every row of tests/igemm_cells.py reaches the launch cell it names, and the rows together reach every cell.  The op of a
row is built over fake non-null pointers of the row's alignment (nothing dereferences them on the host) and asked for its
cell through gode_igemm_launch_cell -- the function gode_igemm itself dispatches on (gan-ode_amd/csrc/igemm_plan.h:
igemm_launch_cell).  A planner change that moves a shape off its cell fails here by the row's name instead of silently
thinning tests/test_gpu_igemm_cells.py, which runs the same rows on the GPU."""
import ctypes as C

import pytest

import gan_ode_amd._lib as L
import igemm_cells as T

TILED = ["fast-dma", "fast-dma-live", "fast-xf", "generic-vec4", "generic-scalar"]     # (fast-reg needs a 2 GiB operand:
BESIDE = ["pointwise1", "pointwise-tap1", "pointwise-taps", "smallk", "dot", "patch"]   # test_operands_beyond_2_gib_...)
TRANSFORMS = ["relu", "lrelu", "lrelu01", "act-only", "affine-only"]
ROWS = [(r, T.parse(r.label)) for r in T.ROWS]


@pytest.mark.parametrize("r", T.ROWS, ids=[r.name for r in T.ROWS])
def test_row_reaches_its_cell(r):
    op = T.fake_op(r)
    assert T.cell_label(op) == r.label
    lib = L.lib()
    p = T.parse(r.label)
    if p["tile"] is not None:
        # the queries callers size their buffers with agree with the cell
        assert (lib.gode_igemm_work_size(C.byref(op)) > 0) == (p["reduce"] != "none")
        assert lib.gode_igemm_stats_rows(C.byref(op)) > 0


def test_every_tile_on_every_tiled_kernel():
    have = {(p["kernel"], p["tile"]) for _, p in ROWS if p["tile"] is not None}
    assert have >= {(k, t) for k in TILED for t in T.TILES.values()}
    assert {r.tile for r, p in ROWS if p["tile"] == "256x128"} == {6}       # reached by request


def test_every_reduce_grid_order_table_and_family():
    tiled = [p for _, p in ROWS if p["tile"] is not None]
    assert {p["reduce"] for p in tiled} == {"none", "vec", "scalar"}
    assert {p["xcd"] for p in tiled} == {0, 1, 2, 3}
    assert {p["table"] for p in tiled} == {"plain", "border", "interleaved"}
    assert {p["kernel"] for _, p in ROWS if p["tile"] is None} == set(BESIDE)
    # the split-K finish on LDS-DMA, live-tap and register-staged launches
    assert {p["kernel"] for p in tiled if p["ksplit"] > 1} == {"fast-dma", "fast-dma-live", "fast-xf"}
    # the scalar finish for each of its three reasons, the tanh epilogue in both, statistics plain and grouped in both
    sc = [r for r, p in ROWS if p.get("reduce") == "scalar"]
    vc = [r for r, p in ROWS if p.get("reduce") == "vec"]
    assert any(T.out_dims(r)[-1] % 4 != 0 for r in sc) and any(r.out == 1 for r in sc) and any(r.work == 1 for r in sc)
    for rows in (sc, vc):
        assert any(r.epi == L.EPI_TANH for r in rows)
        assert any(r.stats and r.groups == 1 for r in rows) and any(r.stats and r.groups == 2 for r in rows)


def test_every_transform_on_both_transforming_kernels_over_padding_taps():
    for kernel in ("fast-xf", "generic-vec4"):
        have = {T.transform(r) for r, p in ROWS if p["kernel"] == kernel and T.has_padding_taps(r)}
        assert have >= set(TRANSFORMS), kernel
    # (the input gradient of k3 s2 p1 on 7x7 gathers no padding: that shape is there for its uneven stride phases)
    assert {(r.shape, r.dir) for r, _ in ROWS if T.transform(r) is not None and not T.has_padding_taps(r)} <= {("k3s2", T.D), ("g24", T.D)}
    assert T.has_padding_taps(T.BY_NAME["xf-k3s2-fprop"]) and not T.has_padding_taps(T.BY_NAME["xf-k3s2"])


def test_transform_with_every_plan_feature():
    xf = [(r, p) for r, p in ROWS if p["kernel"] == "fast-xf"]
    assert any(p["ksplit"] > 1 and r.stats and r.groups == 1 for r, p in xf)
    assert any(r.groups == 2 and r.stats for r, p in xf)
    assert any(p["table"] == "border" and r.border == 1 for r, p in xf)
    assert any(p["table"] == "interleaved" and r.border == 2 for r, p in xf)
    assert any(p["tapskip"] and p["ksplit"] == 1 for r, p in xf) and any(p["tapskip"] and p["ksplit"] > 1 for r, p in xf)
    assert any(r.shape == "k3s2" and r.dir == T.D for r, p in xf)           # uneven stride phases
    assert T.SHAPES["k3s2"][3:] == ((1, 7, 7), (1, 3, 3), (1, 2, 2), (0, 1, 1))


def test_strides_fallbacks_and_refusals():
    by = T.BY_NAME
    # padded vector strides stay on the vector kernels, odd ones land on generic scalar
    assert {T.parse(r.label)["kernel"] for r in T.ROWS if r.strides == "pad4"} == {"fast-dma", "fast-xf", "generic-vec4"}
    assert {T.parse(r.label)["kernel"] for r in T.ROWS if r.strides == "pad1"} == {"generic-scalar"}
    # each family next to its twin one float off: same row but for the offset, and the label shows the move
    for name, twin, field in [("pointwise1", "pointwise1-src-off", "src"), ("pointwise-taps", "pointwise-taps-src-off", "src"),
                              ("smallk", "smallk-out-off", "out"), ("dot", "dot-src-off", "src"), ("patch", "patch-src-off", "src")]:
        a, b = by[name], by[twin]
        assert a._replace(name="", label="") == b._replace(name="", label="", **{field: 0}) and getattr(b, field) == 1
        moved = T.parse(b.label)["tile"] is not None
        assert moved == (name != "patch")       # the LDS-patch kernel gathers scalars: no alignment to lose
    # a plan that splits K without its workspace, with src one float off, with scale one float off: each differs from a split
    # row only in that, runs unsplit on the generic kernel and keeps the split-K finish (hence the plan's statistics layout)
    split, split_xf = by["dma-fprop"], by["xf-t4-act-only"]._replace(tile=0, **T.XF_RELU)
    assert T.parse(split.label)["ksplit"] > 1 and T.parse(T.cell_label(T.fake_op(split_xf)))["ksplit"] > 1
    assert by["unsplit-work-null"]._replace(work=0, label=split.label, name=split.name) == split
    assert by["unsplit-src-off"]._replace(src=0, label=split.label, name=split.name) == split
    assert by["unsplit-scale-off"]._replace(scale=0, label="", name="") == split_xf._replace(label="", name="")
    unsplit = [(r, T.parse(r.label)) for r in T.ROWS if r.name.startswith("unsplit-")]
    assert all(p["ksplit"] == 1 and p["reduce"] != "none" and p["kernel"].startswith("generic-") for _, p in unsplit)
    assert {p["reduce"] for _, p in unsplit} == {"vec", "scalar"}
    assert any(r.work is None and r.stats and r.groups == 2 for r, _ in unsplit) and any(r.epi == L.EPI_TANH for r, _ in unsplit)
    assert all(p["ksplit"] > 1 for r, p in ROWS if p.get("reduce", "none") != "none" and not r.name.startswith("unsplit-"))
