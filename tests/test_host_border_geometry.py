"""CPU: the border-split DGRAD phase table (gan-ode_amd/csrc/conv_geom.h, gode_build_igemm_geom_border) against the plain
table, checked by a stand-alone C++ program (tests/hostcheck/border_check.cpp, its own main) built here with
AddressSanitizer + UBSan and run as a child process: coverage of the output, the multiset of live (position, tap, input)
triples, no out-of-range gather, tap order, packed-panel sources, the fallback to the plain table; plus the library's
host-side queries, which must follow the op's `border` flag consistently."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

import gan_ode_amd._lib as L
from gan_ode_amd.engine import make_geom

SRC = os.path.join(REPO, "tests", "hostcheck", "border_check.cpp")


def test_border_split_table_against_the_plain_table(tmp_path):
    exe = str(tmp_path / "border_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "OK (0 failures)" in r.stdout
    # the shapes the issue names are all there
    for name in ("k4s2p1 1x1", "k4s2p1 2x2", "k4s2p1 3x3", "k4s2p1 4x4", "k4s2p1 8x8", "k4s2p1 16x16", "k4s2p1 2x5",
                 "k3s2p1 4x4 -> 7x7", "3-D k(1,4,4) s(1,2,2) 3x4x4", "fallback"):
        assert name in r.stdout, name


def _convt(n, cin, cout, h, k=4, s=2, p=1):
    """The conv whose input gradient is ConvTranspose2d(cin, cout, k, s, p) on h x h."""
    ho = (h - 1) * s - 2 * p + k
    return make_geom(n, cout, cin, (1, ho, ho), (1, h, h), (1, k, k), (1, s, s), (0, p, p))


def test_pack_size_extends_the_plain_pack():
    lib = L.lib()
    g = _convt(4, 64, 96, 4)
    plain = lib.gode_pack_size(C.byref(g), L.DGRAD)
    assert plain == 96 * 64 * 16
    # interior 4 taps (the plain panels) + 2 + 2 + 1 taps per phase
    assert lib.gode_pack_size(C.byref(g), L.DGRAD | L.PACK_BORDER) == 96 * 64 * (16 + 4 * 5)
    assert lib.gode_pack_size(C.byref(g), L.FPROP | L.PACK_BORDER) == lib.gode_pack_size(C.byref(g), L.FPROP)
    full = make_geom(4, 32, 64, (1, 4, 4), (1, 1, 1), (1, 4, 4), (1, 1, 1), (0, 0, 0))      # fullk: never split
    assert lib.gode_pack_size(C.byref(full), L.DGRAD | L.PACK_BORDER) == lib.gode_pack_size(C.byref(full), L.DGRAD)


@pytest.mark.parametrize("tile", [1, 2, 6])
def test_queries_follow_the_flag(tile):
    """A requested tile takes the border form whenever the table splits: one statistics row per m-block of every
    sub-phase; never a K split; FPROP / grouped ops ignore the flag in every query."""
    lib = L.lib()
    bm = {1: 128, 2: 128, 6: 256}[tile]
    g = _convt(512, 64, 96, 4)
    plain = L.IgemmOp(g=g, dir=L.DGRAD, tile=tile)
    flag = L.IgemmOp(g=g, dir=L.DGRAD, tile=tile, border=1)
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    assert lib.gode_igemm_work_size(C.byref(plain)) == 0
    assert lib.gode_igemm_stats_rows(C.byref(plain)) == 4 * cdiv(512 * 16, bm)
    # per phase of a 4x4 input: 9 interior, 3 + 3 edge, 1 corner position per image
    assert lib.gode_igemm_stats_rows(C.byref(flag)) == 4 * (cdiv(512 * 9, bm) + 2 * cdiv(512 * 3, bm) + cdiv(512, bm))
    assert lib.gode_igemm_stats_rows0(C.byref(flag)) == lib.gode_igemm_stats_rows(C.byref(flag))
    assert lib.gode_igemm_work_size(C.byref(flag)) == 0
    seg = (C.c_int32 * 24)()
    assert lib.gode_igemm_stats_segments(C.byref(flag), 256, seg) == -1       # the joint pass never takes the flag
    for kw in (dict(dir=L.FPROP), dict(dir=L.FPROP, groups=2)):
        a, b = L.IgemmOp(g=g, tile=tile, **kw), L.IgemmOp(g=g, tile=tile, border=1, **kw)
        assert lib.gode_igemm_stats_rows(C.byref(a)) == lib.gode_igemm_stats_rows(C.byref(b)) > 0
        assert lib.gode_igemm_work_size(C.byref(a)) == lib.gode_igemm_work_size(C.byref(b))


def test_a_k_split_launch_ignores_the_flag():
    """Few rows and a long K: the plain plan splits K (its partial sums are added in another order), so the op stays plain,
    and split, in every query."""
    lib = L.lib()
    g = _convt(2, 512, 256, 16)            # 16 sub-phases of >= 2 rows x >= 512 deep: a handful of tiles, 16+ slabs each
    a, b = L.IgemmOp(g=g, dir=L.DGRAD, tile=1), L.IgemmOp(g=g, dir=L.DGRAD, tile=1, border=1)
    assert lib.gode_igemm_work_size(C.byref(a)) > 0
    assert lib.gode_igemm_work_size(C.byref(b)) == lib.gode_igemm_work_size(C.byref(a))
    assert lib.gode_igemm_stats_rows(C.byref(b)) == lib.gode_igemm_stats_rows(C.byref(a))


def test_model_chooses_per_layer_and_never_prices_the_flag_above_plain():
    lib = L.lib()
    for cin, cout, h in ((512, 256, 4), (256, 128, 8), (128, 64, 16)):
        g = _convt(512, cin, cout, h)
        plain = lib.gode_igemm_model_cycles(C.byref(L.IgemmOp(g=g, dir=L.DGRAD, tile=0)))
        flag = lib.gode_igemm_model_cycles(C.byref(L.IgemmOp(g=g, dir=L.DGRAD, tile=0, border=1)))
        assert 0 < flag <= plain


@pytest.mark.parametrize("tile", [5, 7, 12, -1])
def test_a_tile_that_does_not_exist_is_refused(tile):
    """Only 0 (auto) and the tiles 1, 2, 3, 4 and 6 exist: anything else is an argument error in every query (the model
    estimate is -1 for any requested tile, existing or not)."""
    lib = L.lib()
    g = _convt(512, 64, 96, 4)
    for kw in (dict(dir=L.DGRAD), dict(dir=L.DGRAD, border=1), dict(dir=L.FPROP), dict(dir=L.FPROP, groups=2)):
        op = L.IgemmOp(g=g, tile=tile, **kw)
        assert lib.gode_igemm_stats_rows(C.byref(op)) == -1
        assert lib.gode_igemm_stats_rows0(C.byref(op)) == -1
        assert lib.gode_igemm_work_size(C.byref(op)) == -1
        assert lib.gode_igemm_model_cycles(C.byref(op)) == -1.0
    assert lib.gode_igemm_model_cycles(C.byref(L.IgemmOp(g=g, dir=L.DGRAD, tile=2))) == -1.0
    assert lib.gode_igemm_model_cycles(C.byref(L.IgemmOp(g=g, dir=L.DGRAD, tile=0))) > 0
