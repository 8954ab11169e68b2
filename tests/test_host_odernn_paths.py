"""CPU: every row of tests/odernn_paths.py takes the route it names, the rows together take every route, and the refusals trip
every clause of rnn_fwd_args_ok / rnn_bwd_args_ok.  The ops of a row are built over fake non-null pointers (nothing
dereferences them on the host) and asked for their route through gode_odernn_fwd_route / gode_odernn_bwd_route, which run
route_ops and jobs_direct -- the decisions gode_odernn_fwd_multi / gode_odernn_bwd_multi dispatch on
(gan-ode_amd/csrc/odernn_valu.hip).  A router change that moves a shape off its path fails here by the row's name instead of
silently thinning tests/test_gpu_odernn_paths.py, which runs the same rows on the GPU.

The oracle helper the GPU test compares with is checked here too: in float64 against the fp32 recipe of
tests/test_gpu_odernn.py, and its per-64-chunk form against the whole-batch form."""
import os
import re

import pytest
import torch

from conftest import rel_err

import odernn_paths as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("r", P.ROWS, ids=[r.name for r in P.ROWS])
def test_row_takes_its_route(r):
    if r.fwd is not None:
        assert P.route(P.fake_ops(r.ops, "f"), len(r.ops), "f") == (0, r.fwd)
    assert P.route(P.fake_ops(r.ops, "b"), len(r.ops), "b") == (0, r.bwd)
    # each op alone (what the GPU test's single-op baselines run) is accepted too
    for o in r.ops:
        assert P.route(P.fake_ops([o], "f"), 1, "f")[0] == 0 and P.route(P.fake_ops([o], "b"), 1, "b")[0] == 0


def test_rows_cover_every_route_value_in_both_directions():
    fwd = [r.fwd for r in P.ROWS if r.fwd is not None]
    bwd = [r.bwd for r in P.ROWS]
    for vecs in (fwd, bwd):
        assert {v for vec in vecs for v in vec[:-2]} == {0, 1}
        # a shared launch next to MFMA ops (forward), none at all, and one of several jobs
        assert any(vec[-2] == 0 for vec in vecs) and any(vec[-2] > 0 and len(vec) > 3 for vec in vecs)
    assert {vec[-1] for vec in fwd} == {0} and {vec[-1] for vec in bwd} == {0, 1, 2}
    assert any(1 in vec[:-2] and vec[-2] > 0 for vec in fwd)                  # over the cap, the one-workgroup op stays
    # the co-residency limit from both sides, in one op and summed over a call
    spin = lambda ops: sum((o.N + 31) // 32 for o in ops if o.N > 32)        # noqa: E731
    assert {spin(r.ops) for r in P.ROWS if len(r.ops) == 1 and r.fwd[0] == 0 and r.bwd[0] == 0} >= {0, 2, 128}
    assert {spin(r.ops) for r in P.ROWS if len(r.ops) == 1 and r.fwd[0] == 1} >= {129}
    assert spin(P.BY_NAME["multi-at-cap"].ops) == 128 and spin(P.BY_NAME["multi-over-cap"].ops) == 130
    # the sequential route for each of its reasons: a fixed-substeps op, ops over the cap
    seq = [r for r in P.ROWS if r.bwd[-1] == 2]
    assert any(o.substeps > 0 for r in seq for o in r.ops) and any(all(o.substeps == 0 for o in r.ops) for r in seq)
    # shared grads on the fused and on the sequential route, under flags (0, 1) and (0, 0)
    for kind in (0, 2):
        flags = {tuple(o.acc for o in r.ops if o.share is not None) for r in P.ROWS if r.bwd[-1] == kind and any(o.share is not None for o in r.ops)}
        assert flags == {(0,), (1,)}, (kind, flags)


def _refused(base, fields, direction):
    st = P.fake_ops([base], direction)[0]
    P.apply_fields(st, fields)
    return P.route(P.as_array([st], direction), 1, direction)


@pytest.mark.parametrize("r", P.REFUSALS, ids=[r.name for r in P.REFUSALS])
def test_refused_op(r):
    for d in "fb":
        assert P.route(P.fake_ops([r.base], d), 1, d)[0] == 0, "the base op is valid"
        rc, vec = _refused(r.base, r.set, d)
        if d in r.dirs:
            assert (rc, vec) == (P.E_ARG, None)


def test_refusals_cover_every_clause():
    assert {r.clause for r in P.REFUSALS if "f" in r.dirs} == P.CLAUSES_FWD
    assert {r.clause for r in P.REFUSALS if "b" in r.dirs} == P.CLAUSES_BWD
    assert {next(iter(r.set))[2:] for r in P.REFUSALS if r.clause == "params"} == set(P.NAMES)
    # CLAUSES_* name what the two functions test: every `op->field` (or p.field) they read is named by a refusal's overwrite
    src = open(os.path.join(REPO, "gan-ode_amd", "csrc", "odernn_valu.hip")).read()
    for fn, d in (("rnn_fwd_args_ok", "f"), ("rnn_bwd_args_ok", "b")):
        body = src[src.index(f"static bool {fn}("):]
        body = body[:body.index("\n}\n")]
        fields = set(re.findall(r"op->(?:p\.)?(\w+)", body))
        named = {k[2:] if k.startswith("p.") else k for r in P.REFUSALS if d in r.dirs for k in r.set}
        assert fields == named, (fn, fields ^ named)


@pytest.mark.parametrize("name,ops,count", P.CALL_REFUSALS, ids=[c[0] for c in P.CALL_REFUSALS])
def test_refused_call(name, ops, count):
    for d in "fb":
        structs = [P.apply_fields(P.fake_ops([b], d)[0], f) for b, f in ops]
        assert P.route(P.as_array(structs, d), count, d) == (P.E_ARG, None)
        if name.startswith("valid-then"):
            assert P.route(P.as_array(structs[:1], d), 1, d)[0] == 0


@pytest.mark.parametrize("name,base,fields", P.ACCEPTED_BWD, ids=[c[0] for c in P.ACCEPTED_BWD])
def test_fixed_substeps_adjoint_needs_neither_sync_nor_tolerances(name, base, fields):
    st = P.apply_fields(P.fake_ops([base], "b")[0], fields)
    assert P.route(P.as_array([st], "b"), 1, "b") == (0, [1, 0, 2])


def test_header_says_who_zeroes_sync():
    """tests/test_gpu_odernn_paths.py hands every launch an exchange buffer filled with a non-zero pattern: gode.h promises
    that the launch zeroes what it needs."""
    text = " ".join(open(os.path.join(REPO, "include", "gode.h")).read().split())
    assert "caller-owned, zeroed by * the launch" in text


# ---- the oracle helper -------------------------------------------------------------------------------------------------
def _fp32_recipe(f, gru, noise, gup):
    """The oracle of tests/test_gpu_odernn.py::test_odernn_kernels_against_oracle, on the fp32 modules themselves."""
    from oracle import ode_ref
    h, hps = [noise[0]], []
    t01 = torch.tensor([0.0, 1.0])
    for t in range(noise.shape[0] - 1):
        hp = ode_ref.odeint_adjoint(f, h[-1], t01)[-1]
        hps.append(hp)
        h.append(gru(noise[t + 1], hp))
    zref = torch.stack(h[1:], dim=1)
    (zref * gup).sum().backward()
    g = torch.cat([p.grad.reshape(-1) for p in P.net_params(f, gru)])
    return zref.detach(), torch.stack(hps, dim=1).detach(), g


def _blocks(g):
    out, off = {}, 0
    for name, n in zip(P.NAMES, P.SIZES):
        out[name] = g[off:off + n]
        off += n
    return out


def test_float64_oracle_against_the_fp32_recipe():
    N, T = 20, 5
    f, gru = P.make_nets(20)
    gen = torch.Generator().manual_seed(7)
    noise, gup = torch.randn(T + 1, N, 16, generator=gen), torch.randn(N, T, 16, generator=gen)
    hs, hp, g = P.oracle(f, gru, noise, gup)
    assert hs.dtype == torch.float64 and torch.equal(hs[:, 0], noise[0].double())
    z32, hp32, g32 = _fp32_recipe(f, gru, noise, gup)
    es = max(rel_err(z32, hs[:, 1:]), rel_err(hp32, hp))
    eg = max(rel_err(a, b) for a, b in zip(_blocks(g32).values(), _blocks(g).values()))
    print(f"float64 oracle vs fp32 recipe at (20, 5): states {es:.2e}, gradients {eg:.2e}")
    assert es < 1e-5 and eg < 1e-5, (es, eg)
    # sel_t masks the upstream gradient to frame sel[n]: the same as zeroing the other frames by hand
    sel = torch.randint(0, T, (N,), generator=gen, dtype=torch.int32)
    masked = torch.zeros_like(gup)
    masked[torch.arange(N), sel.long()] = gup[torch.arange(N), sel.long()]
    assert torch.equal(P.oracle(f, gru, noise, gup, sel=sel)[2], P.oracle(f, gru, noise, masked)[2])
    # the fp32 form counts its trial steps per frame
    *_, counts = P.oracle(f, gru, noise, gup, dtype=torch.float32, trials=True, backward=False)
    assert len(counts) == T and all(2 <= c < 200 for c in counts), counts


def test_chunked_oracle_against_the_whole_batch_form():
    N, T = 256, 2
    f, gru = P.make_nets(256)
    gen = torch.Generator().manual_seed(8)
    noise, gup = torch.randn(T + 1, N, 16, generator=gen), torch.randn(N, T, 16, generator=gen)
    hs, hp, g = P.oracle(f, gru, noise, gup)
    hs64, hp64, g64 = P.oracle(f, gru, noise, gup, chunk=64)
    assert hs64.shape == hs.shape and hp64.shape == hp.shape
    es = max(rel_err(hs64, hs), rel_err(hp64, hp))
    eg = max(rel_err(a, b) for a, b in zip(_blocks(g64).values(), _blocks(g).values()))
    print(f"per-64 oracle vs whole-batch oracle at N = 256: states {es:.2e}, gradients {eg:.2e}")
    assert 0 < es < 1e-5 and 0 < eg < 1e-5, (es, eg)       # (0: the chunks would not have been solved on their own)
