"""CPU: the launch plan of every implicit-GEMM op (gan-ode_amd/csrc/igemm_plan.h: phase table, tile, K split, live-tap mode,
XCD order, kernel family, model cycles) over a fixed corpus, printed by a stand-alone C++ program
(tests/hostcheck/plan_check.cpp, its own main) built here with AddressSanitizer + UBSan and run as a child process, against
tests/golden/igemm_plans.txt.  The plans the configs get (tile 0, channels-last) are lines of their own; the other variants of
an op (requested tiles, image groups, the flag on FPROP, strided sources; all ops of the kernel-test and geometry-test
shapes) are one "<name> rest: <count> <hash>" line per op -- `plan_check -v` prints those in full.  The golden was recorded from the planning functions as they stood in igemm.hip, moved into
the header verbatim, before they were restructured: a change to the cost model shows up here as the lines it moves."""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "hostcheck", "plan_check.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "igemm_plans.txt")

# name s<strided> g<groups> b<border> t<tile>: family tile vec fast ksplit/slabs positions max_mblk rows/rows0 tapskip dmajor
# xcd_mode MB NB ntab[tile0...] cycles table/nphase/hash
FIELDS = ("family", "tile", "vec", "fast", "ksplit", "positions", "max_mblk", "rows", "tapskip", "dmajor", "xcd", "MB", "NB", "ntab",
          "cycles", "table")


def _parse(line):
    key, _, rest = line.partition(": ")
    name, s, g, b, t = key.split(" ")
    d = dict(zip(FIELDS, rest.split(" ")), name=name, strided=s[1:], groups=g[1:], border=b[1:], req=t[1:])
    d["ksplit"] = int(d["ksplit"].split("/")[0])
    d["kind"] = d["table"].split("/")[0]
    return d


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           SRC, "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_plans_match_the_golden(plans):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    moved = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, plans)) if w != g]
    for i, w, g in moved[:20]:
        print(f"line {i}:\n  golden {w}\n  now    {g}")
    assert not moved, f"{len(moved)} plans differ from tests/golden/igemm_plans.txt"
    assert len(plans) == len(want)


def test_golden_reaches_every_kind_of_plan():
    with open(GOLDEN) as f:
        lines = f.read().splitlines()
    rows = [_parse(line) for line in lines if " rest: " not in line]
    rest = [line.split(" ") for line in lines if " rest: " in line]
    assert len(rest) == 236 and sum(int(r[2]) for r in rest) + len(rows) == 5088       # every variant of every op is pinned
    assert all(len(r) == len(FIELDS) + 6 for r in rows)
    auto = [r for r in rows if r["req"] == "0"]
    assert {r["tile"] for r in auto} == {"1", "2", "3", "4", "6"}                  # every tile is chosen for some op
    assert any(r["ksplit"] > 1 for r in rows)
    assert any(r["tapskip"] == "1" and r["dmajor"] != "0" for r in rows)
    assert any(r["kind"] == "grouped" for r in rows)
    assert {"0", "2", "3"} <= {r["xcd"] for r in rows}
    assert {r["family"] for r in rows} == {"gemm", "patch", "pointwise", "smallk", "dot"}
    assert any(r["cycles"] == "-1" for r in auto) and any(r["cycles"].startswith("0x") for r in auto)
    # the border form under the model (tile 0): taken on the decoder's 512 -> 256 layer at 512 rows, priced and declined on
    # its 128 -> 64 layer
    by = {(r["name"], r["strided"], r["groups"], r["border"], r["req"]): r for r in rows}
    taken, declined = by[("mnist.G512.L1.d", "0", "1", "1", "0")], by[("mnist.G512.L3.d", "0", "1", "1", "0")]
    assert taken["kind"] == "border" and taken["ntab"].startswith("16[") and taken["ksplit"] == 1
    assert declined["kind"] == "plain" and declined["cycles"].startswith("0x")
    assert float.fromhex(taken["cycles"]) < float.fromhex(by[("mnist.G512.L1.d", "0", "1", "0", "0")]["cycles"])
    assert declined["cycles"] == by[("mnist.G512.L3.d", "0", "1", "0", "0")]["cycles"]
