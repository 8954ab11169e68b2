"""CPU: gode_igemm_op.border == 2 (gan-ode_amd/csrc/igemm_plan.h) -- the border-split table taken without the cost model's
comparison, and the phase-interleaved grid order -- checked by a stand-alone C++ program (tests/hostcheck/border_grid_check.cpp,
its own main) built here with AddressSanitizer + UBSan and run as a child process.  It plans every input-gradient op of the
plan corpus with the value, for tile 0 and the requested tiles 2 and 4, and walks the whole workgroup -> tile map of every plan
that takes the table through the very function the kernel decodes its block id with."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "hostcheck", "border_grid_check.cpp")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgrid") / "border_grid_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe])
    r = subprocess.run([exe, "-v"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    return r.stdout.splitlines()


def test_border_2_plans_and_grid_maps(report):
    assert report[-1] == "OK (0 failures)"
    m = re.search(r"taken (\d+) \(phase-interleaved (\d+), order kept (\d+)\), declined (\d+)", report[-2])
    taken, inter, kept, declined = map(int, m.groups())
    assert taken == inter + kept and inter > 0 and kept > 0 and declined > 0


def test_the_decoder_layers_at_the_benchmark_rows(report):
    """The three k4 s2 p1 decoder layers at 512 rows, tile 0: all take the table with the 128x64 tile, four entries (interior,
    h-edge, w-edge, corner) of four stride phases each; the 8x8 -> 16x16 layer is the one the model's tie kept plain."""
    by = {line.split(":")[0]: line for line in report if ": tile " in line}
    for layer, grid in (("mnist.G512.L1", 1024), ("mnist.G512.L2", 2048), ("mnist.G512.L3", 4096)):
        line = by[layer + " t0"]
        assert "tile 2, 4 entries x 4 sub-phases [0," in line and f",{grid}]" in line
    # k3 s2 p1: the stride phases differ in taps and extents -- sub-phase after sub-phase, as before
    assert "x 1 sub-phases" in by["gt.k3s2p1.7 t2"] and "x 1 sub-phases" in by["gt.k3s2p1.7 t4"]
    assert "x 1 sub-phases" in by["gt.3d.k344.2x1x1 t2"]          # two depth runs per stride phase


def _convt(n, cin, cout, h):
    from gan_ode_amd.engine import make_geom
    return make_geom(n, cout, cin, (1, 2 * h, 2 * h), (1, h, h), (1, 4, 4), (1, 2, 2), (0, 1, 1))


def test_dead_tap_share_and_launch_info_queries():
    """The host-side queries ConvStack's rule reads.  A k4 s2 p1 ConvTranspose on h x h: every output position has two taps
    per dimension, and of the 2h positions of a dimension the first and the last have one of theirs on padding -- a share of
    1 / (2h) of the taps per dimension, 1 - (1 - 1/(2h))^2 over both."""
    import gan_ode_amd._lib as L
    lib = L.lib()
    for h, cin, cout in ((4, 512, 256), (8, 256, 128), (16, 128, 64)):
        g = _convt(512, cin, cout, h)
        dead = lib.gode_igemm_dead_taps(C.byref(L.IgemmOp(g=g, dir=L.DGRAD, tile=0)))
        assert dead == pytest.approx(1 - (1 - 1 / (2 * h)) ** 2, abs=1e-12)
        info = (C.c_int32 * 4)()
        assert lib.gode_igemm_launch_info(C.byref(L.IgemmOp(g=g, dir=L.DGRAD, tile=0, border=2)), info) == 0
        assert list(info) == [1, 2, 4 * 512 * h * h // 128 * (cout // 64), 768]
    assert lib.gode_igemm_dead_taps(C.byref(L.IgemmOp(g=_convt(512, 512, 256, 4), dir=L.FPROP, tile=0))) == 0.0
    info = (C.c_int32 * 4)()
    assert lib.gode_igemm_launch_info(C.byref(L.IgemmOp(g=_convt(512, 256, 128, 8), dir=L.DGRAD, tile=0)), info) == 0
    assert list(info) == [0, 6, 512, 256]                                  # plain: 256x128 tiles, one per CU


def test_which_layers_convstack_flags():
    """The rule of gan_ode_amd.engine.border_value on the measured layers (profiles/border_order_layers.md).  512 rows: the
    8x8 and 16x16 layers (2.67 / 5.33 tiles per slot); the 4x4 layer (1.33) stays with the model, which takes the table there
    by itself.  256 rows: the 4x4 layer has no tile on offer, the 8x8 layer (1.33, measured 5 % slower than its plain launch)
    stays with the model, the 16x16 layer (2.67) is taken.  Small batches: nothing."""
    from gan_ode_amd.engine import border_value
    layers = ((512, 256, 4), (256, 128, 8), (128, 64, 16))
    assert [border_value(_convt(512, *l)) for l in layers] == [1, 2, 2]
    assert [border_value(_convt(256, *l)) for l in layers] == [1, 1, 2]
    assert [border_value(_convt(48, *l)) for l in layers] == [1, 1, 1]
