"""CPU: the launch plan of every weight-gradient op (gan-ode_amd/csrc/wgrad_plan.h: path, tile, position splits, kernel family and
its vector / LDS-DMA flags, grid, strides, the reduce kernel, workspace) over a fixed corpus, printed by a stand-alone C++
program (tests/hostcheck/wgrad_plan_check.cpp, its own main) built here with AddressSanitizer + UBSan and run as a child process,
against tests/golden/wgrad_plans.txt.  The plans the configs get (splits 0, channels-last, aligned pointers: no transform,
BN+ReLU on x, BN+ReLU on y), the same op with x, y or work alone 4 bytes off, and the plans a tuning knob changes are lines of
their own; the other variants of an op (requested splits, strided x, the remaining transform / alignment combinations; all ops
of the kernel-test and border shapes) are one "<name> rest: <count> <hash>" line per geometry -- `wgrad_plan_check -v` prints
those in full.  The program also checks every plan itself (workspace part independent of the pointers and equal to the size
queries, splits * chunk >= M, grid z, patch LDS, a kernel case for every plan) and exits non-zero when one fails.  The golden
was recorded from the planning functions as they stood in wgrad.hip, copied verbatim and driven by gode_wgrad's own sequence of
decisions, before they were restructured into the plan: a change to the cost model shows up here as the lines it moves."""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "hostcheck", "wgrad_plan_check.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "wgrad_plans.txt")

# name sp<splits> xf<xform_on_y> sc<scale> a<act> st<strided> x<off> y<off> w<off> (or name k:<knob>): rule/split_tile/splits path tile
# family vx vy glds M taps Kt chunk/chunk_thin grid block lds xs x_bytes reduce/blocks work_floats patch[...]
FIELDS = ("work", "path", "tile", "family", "vx", "vy", "glds", "M", "taps", "Kt", "chunk", "grid", "block", "lds", "xs", "x_bytes",
          "reduce", "work_floats", "patch")


def _parse(line):
    key, _, rest = line.partition(": ")
    d = dict(zip(FIELDS, rest.split(" ")), name=key.split(" ")[0], key=key, knob=key.split(" k:")[1] if " k:" in key else "")
    d["rule"], d["split_tile"], d["splits"] = d["work"].split("/")
    d["reduce"] = d["reduce"].split("/")[0]
    return d


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GODE_WGRAD_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_plans_match_the_golden(plans):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    moved = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, plans)) if w != g]
    for i, w, g in moved[:20]:
        print(f"line {i}:\n  golden {w}\n  now    {g}")
    assert not moved, f"{len(moved)} plans differ from tests/golden/wgrad_plans.txt"
    assert len(plans) == len(want)


def test_golden_reaches_every_kind_of_plan():
    with open(GOLDEN) as f:
        lines = f.read().splitlines()
    rows = [_parse(line) for line in lines if " rest: " not in line]
    rest = [line.split(" ") for line in lines if " rest: " in line]
    assert len(rest) == 163 and sum(int(r[2]) for r in rest) + len(rows) == 27823      # every variant of every op is pinned
    assert all(len(r["key"].split(" ")) in (2, 9) and r["patch"].count(",") == 8 for r in rows)
    assert {r["path"] for r in rows} == {"patch", "thin", "gemm"}
    assert {r["split_tile"] for r in rows if r["path"] == "gemm" and not r["knob"]} == {"0", "1", "2", "3", "4"}
    assert {r["tile"] for r in rows if r["family"] == "fast"} == {"0", "1", "2", "3", "4"}
    assert {r["family"] for r in rows if r["path"] == "gemm"} == {"fast", "generic"}
    assert {(r["vx"], r["vy"]) for r in rows if r["family"] == "generic" and not r["knob"]} == {("0", "0"), ("0", "1"), ("1", "0")}
    assert any(     # both operands vectorisable on the generic kernel: only under GODE_WGRAD_GENERIC
        (r["vx"], r["vy"]) == ("1", "1") for r in rows if r["family"] == "generic" and r["knob"] == "generic")
    assert {r["glds"] for r in rows if r["family"] == "fast"} == {"0", "1"}
    assert {r["reduce"] for r in rows} == {"small", "vec4", "scalar"}
    assert any(r["reduce"] == "small" and r["path"] == "patch" for r in rows)
    # the three kept oddities
    #  a thin-eligible op with y off 16-byte alignment: the THIN rule's split count on the generic 32-wide tile
    odd1 = [r for r in rows if r["rule"] == "thin" and r["path"] == "gemm"]
    assert odd1 and all(r["family"] == "generic" and r["vy"] == "0" and " y4 " in r["key"] for r in odd1)
    assert any(int(r["splits"]) > 256 for r in odd1)
    #  splits chosen for an 8-wave tile, launched on 128x128 because x or y is not vectorisable
    odd2 = [r for r in rows if r["split_tile"] in "34" and r["tile"] == "2" and not r["knob"]]
    assert odd2 and all(r["family"] == "generic" and (r["vx"], r["vy"]) != ("1", "1") for r in odd2)
    #  GODE_WGRAD_GENERIC changes the tile of an 8-wave plan, not only its kernel
    odd3 = [r for r in rows if r["knob"] == "generic" and r["split_tile"] in "34"]
    assert odd3 and all(r["tile"] == "2" and r["family"] == "generic" for r in odd3)
    # GODE_WGRAD_GLDS=0 does not reach the 8-wave tiles: no such plan differs from the plain one, so none is listed
    assert not [r for r in rows if r["knob"] == "noglds" and r["tile"] in "34"]
    assert any(r["knob"] == "noglds" and r["tile"] in "012" and r["glds"] == "0" for r in rows)
