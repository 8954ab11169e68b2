"""GPU: every dispatch path of the ODE-RNN motion latent (gode_odernn_fwd / gode_odernn_bwd and their _multi forms) against
a float64 oracle: tests/odernn_paths.py:oracle (oracle.ode_ref.odeint_adjoint per frame + torch.nn.GRUCell on float64 copies of
the fp32 parameters and inputs).  The rows are those of tests/odernn_paths.py; tests/test_host_odernn_paths.py pins the route
each takes.  An op on the MFMA kernels is compared with the oracle's per-64-trajectory form (one error norm per workgroup
there), every other one with the whole-batch form.

Every output buffer is NaN-filled (step counts: -7) with spare space behind what the kernels own, every exchange buffer is
filled with a non-zero pattern (header words included) before each launch, and `work` starts as NaN.  Bounds are those of
tests/test_gpu_odernn.py: states 2e-5, each gradient tensor 1e-4 (adaptive and substeps = 32 alike); trial counts on the
vector-ALU routes follow the fp32 oracle's per frame (none differs by more than one, at most max(1, T // 8) differ).

accumulate = 1 is held to torch.equal: grads pre-filled with a random `base` must end as the fp32 sum base + g0, g0 being the
accumulate = 0 result -- every route ends in one fp32 add of a deterministic value.  The one exception is by construction, not
by rounding: a pair sharing grads on the one-op-at-a-time route adds twice, so it must equal (base + g_first) + g_second, and
its accumulate = 0 result g_first + g_second, the two ops' own single-op results (still torch.equal)."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

import gan_ode_amd._lib as L
import odernn_paths as P

pytestmark = pytest.mark.gpu

NP = L.ODERNN_NPARAM
NAN = float("nan")
PATTERN = 0x5A5A5A5A            # what every word of an exchange buffer holds before a launch


def stream():
    return torch.cuda.current_stream().cuda_stream


def identical(a, b):
    """Identical results: equal values (torch.equal) with the NaN sentinels in the same places."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = a.isnan(), b.isnan()
    return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def blocks(g):
    off = 0
    for name, n in zip(P.NAMES, P.SIZES):
        yield name, g[off:off + n]
        off += n


class Rnn:
    """One ODE-RNN op: fp32 parameters and inputs (CPU), their device copies, the two op structs and sentinel-filled outputs
    with spare space behind what the kernels own: two rows of z, one trajectory of hp and hs, 16 floats of grads, one step
    count."""

    def __init__(self, o, seed):
        self.o, self.N, self.T = o, o.N, o.T
        N, T = o.N, o.T
        self.f, self.gru = P.make_nets(seed)
        gen = torch.Generator().manual_seed(seed)
        self.noise = torch.randn(T + 1, N, 16, generator=gen)
        self.gup = torch.randn(N, T, 16, generator=gen)
        self.sel = torch.randint(0, T, (N,), generator=gen, dtype=torch.int32) if o.sel else None
        self.content = torch.randn(N, 50, generator=gen) if o.content else None
        self.base = torch.randn(NP, generator=gen)
        self.rows = N if o.sel else N * T
        self.dev = [p.detach().cuda() for p in P.net_params(self.f, self.gru)]
        self.noise_d = self.noise.cuda()
        self.content_d = self.content.cuda() if o.content else None
        self.sel_d = self.sel.cuda() if o.sel else None
        gz = torch.full((self.rows, o.gz_zcols), NAN)           # only the 16 motion columns may be read
        gz[:, :16] = self.gup[torch.arange(N), self.sel.long()] if o.sel else self.gup.reshape(N * T, 16)
        self.gz = gz.cuda()
        nsync = max(L.lib().gode_odernn_sync_size(N), 1)
        self.sync_f = torch.empty(nsync, dtype=torch.int32, device="cuda") if o.sync else None
        self.sync_b = torch.empty(nsync, dtype=torch.int32, device="cuda") if o.bsync else None
        self.work = torch.full((L.lib().gode_odernn_bwd_work_size(N),), NAN, device="cuda")
        self.z = torch.empty(self.rows + 2, o.zcols, device="cuda")
        self.hp = torch.empty(N + 1, T, 16, device="cuda")
        self.hs = torch.empty(N + 1, T + 1, 16, device="cuda") if o.hs else None
        self.grads = torch.empty(NP + 16, device="cuda")
        self.nst = torch.empty(T + 1, dtype=torch.int32, device="cuda")
        self.nstb = torch.empty(T + 1, dtype=torch.int32, device="cuda")
        self.reset()
        self.fill_grads()
        ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
        ptrs = dict(params=[p.data_ptr() for p in self.dev], noise=ptr(self.noise_d), content=ptr(self.content_d),
                    sel_t=ptr(self.sel_d), z=ptr(self.z), hs=ptr(self.hs), hp=ptr(self.hp), nsteps=ptr(self.nst),
                    sync=ptr(self.sync_f), gz=ptr(self.gz), work=ptr(self.work), grads=ptr(self.grads), bsync=ptr(self.sync_b),
                    bnsteps=ptr(self.nstb))
        self.fop, self.bop = P.fwd_struct(o, ptrs), P.bwd_struct(o, ptrs)

    # ---- buffers ---------------------------------------------------------------------------------------------------
    def fwd_buffers(self):
        return [t for t in (self.z, self.hp, self.hs, self.nst) if t is not None]

    def reset(self):
        """Refill every forward output with its sentinel, in place (the op structs keep their pointers)."""
        for t in self.fwd_buffers():
            t.fill_(-7 if t.dtype == torch.int32 else NAN)

    def fill_grads(self, base=False):
        self.grads.fill_(NAN)
        if base:
            self.grads[:NP] = self.base.cuda()
        self.nstb.fill_(-7)

    def dirty_sync(self):
        for s in (self.sync_f, self.sync_b):
            if s is not None:
                s.fill_(PATTERN)

    def outputs(self):
        return [t.clone() for t in self.fwd_buffers()]

    # ---- launches --------------------------------------------------------------------------------------------------
    def fwd(self):
        self.dirty_sync()
        L.check(L.lib().gode_odernn_fwd(C.byref(self.fop), stream()), "gode_odernn_fwd")
        torch.cuda.synchronize()

    def bwd(self, accumulate):
        self.dirty_sync()
        self.bop.accumulate = accumulate
        L.check(L.lib().gode_odernn_bwd(C.byref(self.bop), stream()), "gode_odernn_bwd")
        torch.cuda.synchronize()

    # ---- oracle ----------------------------------------------------------------------------------------------------
    def oracle(self, chunk=None):
        """float64: hs [N, T + 1, 16], hp [N, T, 16], gradient vector [2176] (cached per grouping)."""
        cache = self.__dict__.setdefault("_oracle", {})
        if chunk not in cache:
            cache[chunk] = P.oracle(self.f, self.gru, self.noise, self.gup, sel=self.sel, chunk=chunk)
        return cache[chunk]

    def trials_fp32(self):
        """Trial steps per frame of the same solves in fp32 (at rtol 1e-7 the fp32 round-off in the error estimate is about half
        the tolerance: an fp32 controller rejects steps a float64 one accepts, so the device is compared with this count)."""
        return P.oracle(self.f, self.gru, self.noise, self.gup, dtype=torch.float32, trials=True, backward=False)[3]

    # ---- checks ----------------------------------------------------------------------------------------------------
    def check_fwd(self, chunk, tag):
        N, T, rows, o = self.N, self.T, self.rows, self.o
        hs_ref, hp_ref, _ = self.oracle(chunk)
        z, hp = self.z.cpu(), self.hp.cpu()
        pick = (torch.arange(N), self.sel.long()) if o.sel else None
        want = hs_ref[:, 1:][pick] if o.sel else hs_ref[:, 1:].reshape(N * T, 16)
        errs = {"hp": rel_err(hp[:N], hp_ref), "z": rel_err(z[:rows, :16], want)}
        if o.hs:
            hs = self.hs.cpu()
            errs["hs"] = rel_err(hs[:N], hs_ref)
            assert torch.equal(hs[:N, 0], self.noise[0])
            assert torch.equal(hs[:N, 1:][pick] if o.sel else hs[:N, 1:].reshape(N * T, 16), z[:rows, :16])
            assert bool(hs[N:].isnan().all())
        print(f"{tag}: states " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) < 2e-5, errs
        if o.content:
            c = self.content if o.sel else self.content.repeat_interleave(T, 0)
            assert torch.equal(z[:rows, 16:66], c)
            assert bool((z[:rows, 66:] == 0).all())                   # pad columns
        else:
            assert bool(z[:rows, 16:].isnan().all())                  # content NULL: those columns are left alone
        assert bool(z[rows:].isnan().all()) and bool(hp[N:].isnan().all())

    def check_nsteps(self, mfma, tag):
        v = self.nst.cpu()
        assert int(v[self.T]) == -7, v.tolist()
        steps = v[:self.T].tolist()
        assert min(steps) >= 2 and max(steps) < 200, steps
        if mfma:
            print(f"{tag}: forward trial steps of workgroup 0 per frame {steps}")
            return
        ref = self.trials_fp32()
        diff = [abs(a - b) for a, b in zip(steps, ref)]
        assert max(diff) <= 1 and sum(1 for d in diff if d) <= max(1, self.T // 8), (steps, ref)

    def check_grads(self, gref, tag, g=None):
        g = self.grads.cpu() if g is None else g
        assert bool(g[NP:].isnan().all())
        errs = {name: rel_err(a, b) for (name, a), (_, b) in zip(blocks(g[:NP]), blocks(gref))}
        print(f"{tag}: gradients " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) < 1e-4, errs

    def check_nsteps_bwd(self, tag, mfma=False):
        v = self.nstb.cpu()
        if self.o.substeps:
            assert bool((v == -7).all()), v.tolist()                  # adaptive only
            return
        assert int(v[self.T]) == -7, v.tolist()
        steps = v[:self.T].tolist()
        assert min(steps) >= 2 and max(steps) < 400, steps
        if mfma:
            print(f"{tag}: adjoint trial steps of workgroup 0 per frame {steps}")

    def check_accumulated(self, g0, expect=None):
        """grads after an adjoint with accumulate = 1 over `base`: exactly the fp32 sum base + g0."""
        g = self.grads.cpu()
        expect = self.base + g0[:NP].cpu() if expect is None else expect
        assert torch.equal(g[:NP], expect), f"{int((g[:NP] != expect).sum())} of {NP} floats differ, worst " \
                                            f"{float((g[:NP] - expect).abs().max()):.3e}"
        assert bool(g[NP:].isnan().all())


def single_op_battery(lat, mfma_fwd, mfma_bwd, tag):
    """The op alone through gode_odernn_fwd / gode_odernn_bwd: oracle, sentinels, determinism, accumulate.  -> forward outputs,
    the accumulate = 0 gradient buffer."""
    lat.reset()
    lat.fwd()
    lat.check_fwd(64 if mfma_fwd else None, tag)
    lat.check_nsteps(mfma_fwd, tag)
    out = lat.outputs()
    lat.reset()
    lat.fwd()
    assert all(identical(a, b) for a, b in zip(out, lat.outputs())), "forward not deterministic"
    # the adaptive adjoint on the MFMA kernels takes one norm per 64 trajectories; the fixed substeps take none
    gref = lat.oracle(64 if (mfma_bwd and not lat.o.substeps) or mfma_fwd else None)[2]
    lat.fill_grads()
    lat.bwd(0)
    lat.check_grads(gref, tag)
    lat.check_nsteps_bwd(tag, mfma_bwd)
    g0 = lat.grads.clone()
    lat.fill_grads()
    lat.bwd(0)
    assert identical(lat.grads, g0), "adjoint not deterministic"
    lat.fill_grads(base=True)
    lat.bwd(1)
    lat.check_accumulated(g0)
    lat.check_nsteps_bwd(tag, False)
    return out, g0


SINGLE = [r for r in P.ROWS if len(r.ops) == 1]
MULTI = [r for r in P.ROWS if len(r.ops) > 1]


@pytest.mark.parametrize("r", SINGLE, ids=[r.name for r in SINGLE])
def test_one_op_against_float64_oracle(r):
    lat = Rnn(r.ops[0], 3000 + P.ROWS.index(r))
    single_op_battery(lat, r.fwd[0] == 1, r.bwd[0] == 1, r.name)


# ---------------------------------------------------------------------------------------------------------------------
def _fwd_multi(lats):
    for a in lats:
        a.dirty_sync()
    arr = P.as_array([a.fop for a in lats], "f")
    L.check(L.lib().gode_odernn_fwd_multi(arr, len(lats), stream()), "gode_odernn_fwd_multi")
    torch.cuda.synchronize()


def _bwd_multi(lats, flags):
    for a, acc in zip(lats, flags):
        a.dirty_sync()
        a.bop.accumulate = acc
    arr = P.as_array([a.bop for a in lats], "b")
    L.check(L.lib().gode_odernn_bwd_multi(arr, len(lats), stream()), "gode_odernn_bwd_multi")
    torch.cuda.synchronize()


@pytest.mark.parametrize("r", MULTI, ids=[r.name for r in MULTI])
def test_multi_against_single_ops_and_float64_oracle(r):
    """Forward outputs of every op and own-grads adjoints are bitwise those of the single-op calls (one workgroup writing grads
    itself against the work-row route included: 0.f + row is the same value); the ops a call moves to the MFMA kernels are
    held to the per-64 oracle instead.  A grads vector shared by two ops holds the oracle's sum, whatever the second op's flag
    says, and the second op's own buffer stays NaN."""
    ops = r.ops
    seed0 = 4000 + 10 * [x.name.replace("-flags00", "") for x in P.ROWS].index(r.name.replace("-flags00", ""))
    lats = [Rnn(o, seed0 + k) for k, o in enumerate(ops)]
    count = len(ops)
    fwd_route = r.fwd if r.fwd is not None else [0] * count
    # an op whose route in the call is the one it takes alone (alone, only N > 4096 or substeps > 0 leave the shared launch)
    moved_f = [fwd_route[k] == 1 for k in range(count)]
    moved_b = [r.bwd[k] == 1 and not ops[k].substeps for k in range(count)]
    singles = {}
    for k, a in enumerate(lats):
        if not (moved_f[k] or moved_b[k]):
            singles[k] = single_op_battery(a, False, ops[k].substeps > 0, f"{r.name}[{k}] alone")
    # ---- forward
    if r.fwd is not None:
        for a in lats:
            a.reset()
        _fwd_multi(lats)
        for k, a in enumerate(lats):
            if moved_f[k]:
                a.check_fwd(64, f"{r.name}[{k}]")
                a.check_nsteps(True, f"{r.name}[{k}]")
            else:
                assert all(identical(u, v) for u, v in zip(singles[k][0], a.outputs())), f"forward of op {k} != its single-op call"
        out = [a.outputs() for a in lats]
        for a in lats:
            a.reset()
        _fwd_multi(lats)
        assert all(identical(u, v) for o, a in zip(out, lats) for u, v in zip(o, a.outputs())), "forward not deterministic"
    # ---- adjoint
    owner = [k if o.share is None else o.share for k, o in enumerate(ops)]
    for k, a in enumerate(lats):
        a.bop.grads = lats[owner[k]].grads.data_ptr()
    flags = [o.acc for o in ops]

    def run(flags, base):
        for a in lats:
            a.fill_grads(base)
        _bwd_multi(lats, flags)

    run(flags, False)
    sequential = r.bwd[-1] == 2
    for k, a in enumerate(lats):
        tag = f"{r.name}[{k}]"
        group = [j for j in range(count) if owner[j] == k]
        if owner[k] != k:
            assert bool(a.grads.isnan().all()), f"op {k} adds into op {owner[k]}'s grads: its own buffer is not its to write"
        elif len(group) > 1:
            a.check_grads(sum(lats[j].oracle()[2] for j in group), tag + " (shared)")
            if sequential:      # 0-store, then one add per later op: exactly the sum of the single-op results
                assert len(group) == 2 and torch.equal(a.grads.cpu()[:NP], singles[group[0]][1].cpu()[:NP] + singles[group[1]][1].cpu()[:NP])
        elif moved_b[k] or moved_f[k]:
            a.check_grads(a.oracle(64)[2], tag)
        else:
            assert identical(a.grads, singles[k][1]), f"adjoint of op {k} != its single-op call"
        a.check_nsteps_bwd(tag, moved_b[k])
    saved = [a.grads.clone() for a in lats]
    run(flags, False)
    assert all(identical(a.grads, s) for a, s in zip(lats, saved)), "adjoint not deterministic"
    run([1] * count, True)
    for k, a in enumerate(lats):
        group = [j for j in range(count) if owner[j] == k]
        if owner[k] != k:
            assert identical(a.grads[NP:], saved[k][NP:]) and torch.equal(a.grads.cpu()[:NP], a.base)      # untouched
        elif len(group) > 1 and sequential:
            a.check_accumulated(None, (a.base + singles[group[0]][1].cpu()[:NP]) + singles[group[1]][1].cpu()[:NP])
        else:
            a.check_accumulated(saved[k])


# ---------------------------------------------------------------------------------------------------------------------
def _sentinels_intact(lat):
    torch.cuda.synchronize()
    bufs = lat.fwd_buffers() + [lat.grads, lat.nstb, lat.work]
    syncs = [s for s in (lat.sync_f, lat.sync_b) if s is not None]
    return all(bool((t == -7).all()) if t.dtype == torch.int32 else bool(t.isnan().all()) for t in bufs) and \
        all(bool((s == PATTERN).all()) for s in syncs)


def test_refusals_return_e_arg_and_write_nothing():
    lib = L.lib()
    lats = {}

    def structs(base, fields, d):
        key = (base, d == "b" and base.substeps)
        if key not in lats:
            lats[key] = Rnn(base._replace(hs=True, content=True), 5000 + len(lats))
        lat = lats[key]
        lat.dirty_sync()
        kind = L.OdeRnnFwdOp if d == "f" else L.OdeRnnBwdOp
        st = kind.from_buffer_copy(lat.fop if d == "f" else lat.bop)
        return lat, P.apply_fields(st, fields)

    for ref in P.REFUSALS:
        for d in ref.dirs:
            lat, st = structs(ref.base, ref.set, d)
            one, multi = (lib.gode_odernn_fwd, lib.gode_odernn_fwd_multi) if d == "f" else (lib.gode_odernn_bwd, lib.gode_odernn_bwd_multi)
            assert one(C.byref(st), stream()) == P.E_ARG, (ref.name, d)
            assert multi(P.as_array([st], d), 1, stream()) == P.E_ARG, (ref.name, d)
            assert _sentinels_intact(lat), (ref.name, d)
    for name, ops, count in P.CALL_REFUSALS:
        for d in "fb":
            pairs = [structs(b, f, d) for b, f in ops]
            multi = lib.gode_odernn_fwd_multi if d == "f" else lib.gode_odernn_bwd_multi
            assert multi(P.as_array([st for _, st in pairs], d), count, stream()) == P.E_ARG, (name, d)
            assert all(_sentinels_intact(lat) for lat, _ in pairs), (name, d)     # the valid first op did not run either
