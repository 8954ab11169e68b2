"""The dispatch paths of the ODE-RNN motion latent (gode_odernn_fwd / gode_odernn_bwd and their _multi forms; the router is
route_ops / fwd_multi / bwd_multi in gan-ode_amd/csrc/odernn_valu.hip) as plain data: one row per path, each at the smallest
shapes that reach it.  Shared by tests/test_host_odernn_paths.py (every row's ops, built over fake non-null pointers, get the
row's route vectors from gode_odernn_fwd_route / gode_odernn_bwd_route -- the decisions the launchers dispatch on) and
tests/test_gpu_odernn_paths.py (every row runs on the GPU against the float64 oracle below).

A route vector is route[count + 2]: per op 0 = the call's shared vector-ALU launch, 1 = the MFMA kernels with launches of its
own; then the workgroups of the shared launch; then, for adjoints, 0 = work rows added by latent_rows_kernel, 1 = the launch's
one workgroup writes grads itself, 2 = the ops run one at a time (forward: 0).

All solves use rtol 1e-7, atol 1e-9.  A workgroup of the vector-ALU kernels holds 32 trajectories; 128 spinning workgroups
(workgroups of ops with more than one) is the co-residency limit of a call."""
import collections
import copy
import ctypes as C

import torch

import gan_ode_amd._lib as L
from oracle import ode_ref

RTOL, ATOL = 1e-7, 1e-9
E_ARG = -1
NAMES = ("W1", "b1", "W2", "b2", "Wih", "Whh", "bih", "bhh")
SIZES = (256, 16, 256, 16, 768, 768, 48, 48)

# One op.  sync: the forward op gets an exchange buffer; bsync: the adjoint op does (default: as the forward).  gz_zcols: row
# stride of the upstream gradient (default: zcols).  share: index of the earlier op of the call whose grads this op adds into
# (None: grads of its own).  acc: the op's accumulate flag in the row's base run.
Op = collections.namedtuple("Op", "N T sync bsync sel content hs zcols gz_zcols substeps share acc")


def op(N, T, sync=False, bsync=None, sel=False, content=False, hs=False, zcols=72, gz_zcols=None, substeps=0, share=None, acc=0):
    return Op(N, T, sync, sync if bsync is None else bsync, sel, content, hs, zcols, zcols if gz_zcols is None else gz_zcols,
              substeps, share, acc)


# fwd / bwd: the expected route vectors (fwd None: the row is about the adjoint call only; its forwards run op by op)
Row = collections.namedtuple("Row", "name ops fwd bwd reaches")

_FUSED = [op(20, 4), op(100, 3, sync=True), op(40, 4, sync=True, sel=True), op(24, 4, sel=True, share=2, acc=1)]
_SEQ = [op(20, 3), op(40, 3, sync=True, bsync=False, substeps=32), op(24, 3, share=0, acc=1)]


def _flags(ops, *acc):
    return [o._replace(acc=a) for o, a in zip(ops, acc)]


ROWS = [
    # ---- one op per call (gode_odernn_fwd, gode_odernn_bwd)
    Row("one", [op(1, 1, content=True, zcols=68)], [0, 1, 0], [0, 1, 1],
        "one workgroup, one trajectory, one frame; adjoint direct"),
    Row("direct-sel", [op(20, 4, sel=True, hs=True)], [0, 1, 0], [0, 1, 1],
        "direct; sel_t, content NULL: the columns from 16 on keep their NaN"),
    Row("full-wg", [op(32, 3, content=True, zcols=96, gz_zcols=16)], [0, 1, 0], [0, 1, 1],
        "the last N that needs no sync; gz rows of 16 floats"),
    Row("two-wg", [op(33, 2, sync=True, sel=True, content=True)], [0, 2, 0], [0, 2, 0],
        "the second workgroup holds one trajectory; work rows + latent_rows_kernel"),
    Row("four-wg", [op(100, 3, sync=True, hs=True)], [0, 4, 0], [0, 4, 0], "rows route, hs, content NULL"),
    Row("cap", [op(4096, 2, sync=True, sel=True)], [0, 128, 0], [0, 128, 0], "128 spinning workgroups, the limit"),
    Row("over-cap", [op(4097, 2, sel=True, content=True)], [1, 0, 0], [1, 0, 2],
        "MFMA kernels, the last workgroup holds one trajectory, sync NULL"),
    Row("over-cap-sync", [op(4128, 2, sync=True, hs=True)], [1, 0, 0], [1, 0, 2], "MFMA kernels, sync given and unused"),
    Row("fixed-20", [op(20, 3, sel=True, substeps=32)], [0, 1, 0], [1, 0, 2],
        "odernn_bwd_kernel: two rows of 16 trajectories, the last holding four; sel_t; one-level gode_reduce_rows"),
    Row("fixed-33", [op(33, 3, sync=True, bsync=False, substeps=32)], [0, 2, 0], [1, 0, 2],
        "odernn_bwd_kernel: three rows, the last holding one; sync NULL accepted"),
    Row("fixed-100", [op(100, 3, sync=True, bsync=False, substeps=32)], [0, 4, 0], [1, 0, 2],
        "odernn_bwd_kernel: seven rows, the last holding four"),
    # ---- several ops per call (gode_odernn_fwd_multi, gode_odernn_bwd_multi)
    Row("multi-fused", _FUSED, [0, 0, 0, 0, 8, 0], [0, 0, 0, 0, 8, 0],
        "one launch of 1 + 4 + 2 + 1 workgroups and its job table; latent_rows_kernel over groups; a pair sharing grads (0, 1)"),
    Row("multi-fused-flags00", _flags(_FUSED, 0, 0, 0, 0), [0, 0, 0, 0, 8, 0], [0, 0, 0, 0, 8, 0],
        "the same call with the shared pair's flags (0, 0): the group rule on the fused route"),
    Row("multi-at-cap", [op(2048, 2, sync=True), op(2048, 2, sync=True)], [0, 0, 128, 0], [0, 0, 128, 0],
        "64 + 64 = 128 spinning workgroups: stays fused"),
    Row("multi-over-cap", [op(33, 3, sync=True, sel=True), op(4090, 2, sync=True), op(20, 3)], [1, 1, 0, 1, 0], [1, 1, 0, 0, 2],
        "2 + 128 = 130 spinning workgroups: both multi-workgroup ops on the MFMA kernels (N = 33: one workgroup of three waves, "
        "the last holding one trajectory), the one-workgroup op stays"),
    Row("multi-sequential", _SEQ, None, [0, 1, 0, 0, 2],
        "a substeps = 32 op sends the adjoint call down the one-op-at-a-time route; ops 0 and 2 share grads, flags (0, 1)"),
    Row("multi-sequential-flags00", _flags(_SEQ, 0, 0, 0), None, [0, 1, 0, 0, 2],
        "the same call with the shared pair's flags (0, 0): the group rule on the sequential route"),
]
BY_NAME = {r.name: r for r in ROWS}

# ---- refusals.  (name, directions, clause of rnn_fwd_args_ok / rnn_bwd_args_ok it trips, base op, fields to overwrite).  A
# field value None is a NULL pointer.  The clause names are those of CLAUSES below.
Refusal = collections.namedtuple("Refusal", "name dirs clause base set")
CLAUSES_FWD = {"noise", "z", "N", "T", "rtol", "atol", "zcols-min", "zcols-mod4", "params", "sync"}
CLAUSES_BWD = {"noise", "hp", "gz", "work", "grads", "N", "T", "substeps", "rtol", "atol", "zcols-min", "zcols-mod4", "params",
               "sync"}
_B20, _B33, _B4096 = op(20, 2), op(33, 2, sync=True), op(4096, 2, sync=True)
REFUSALS = [
    Refusal("sync-null-33", "fb", "sync", _B33, {"sync": None}),
    Refusal("sync-null-4096", "fb", "sync", _B4096, {"sync": None}),
    Refusal("T-0", "fb", "T", _B20, {"T": 0}),
    Refusal("N-0", "fb", "N", _B20, {"N": 0}),
    Refusal("rtol-0", "fb", "rtol", _B20, {"rtol": 0.0}),
    Refusal("atol-negative", "fb", "atol", _B20, {"atol": -1e-9}),
    Refusal("fwd-zcols-64", "f", "zcols-min", _B20, {"zcols": 64}),
    Refusal("fwd-zcols-70", "f", "zcols-mod4", _B20, {"zcols": 70}),
    Refusal("bwd-zcols-12", "b", "zcols-min", _B20, {"zcols": 12}),
    Refusal("bwd-zcols-18", "b", "zcols-mod4", _B20, {"zcols": 18}),
    Refusal("substeps-negative", "b", "substeps", _B20, {"substeps": -1}),
    Refusal("noise-null", "fb", "noise", _B20, {"noise": None}),
    Refusal("z-null", "f", "z", _B20, {"z": None}),
    Refusal("hp-null", "b", "hp", _B20, {"hp": None}),
    Refusal("gz-null", "b", "gz", _B20, {"gz": None}),
    Refusal("work-null", "b", "work", _B20, {"work": None}),
    Refusal("grads-null", "b", "grads", _B20, {"grads": None}),
] + [Refusal(f"{n}-null", "fb", "params", _B20, {"p." + n: None}) for n in NAMES]
# refusals of the call: (name, ops as (base, overwrites) pairs -- empty: count 0; the count handed in)
CALL_REFUSALS = [
    ("count-0", [(_B20, {})], 0),
    ("count-9", [(_B20, {})] * 9, 9),
    ("valid-then-refused", [(_B20, {}), (_B20, {"T": 0})], 2),
    ("valid-then-sync-null", [(_B20, {}), (_B33, {"sync": None})], 2),
]
# ops the entry points accept although a neighbouring clause refuses their like (adjoint only: substeps > 0 needs neither
# tolerances nor an exchange)
ACCEPTED_BWD = [
    ("fixed-sync-null-33", _B33._replace(substeps=32), {"sync": None}),
    ("fixed-sync-null-4096", _B4096._replace(substeps=32), {"sync": None}),
    ("fixed-rtol-0", _B20._replace(substeps=32), {"rtol": 0.0, "atol": -1.0}),
]


# ---- op structs ------------------------------------------------------------------------------------------------------
def apply_fields(st, fields):
    """Overwrite the named fields of an op struct ("p.Whh": a member of its parameter block) that the struct has."""
    for k, v in fields.items():
        tgt, name = (st.p, k[2:]) if k.startswith("p.") else (st, k)
        if hasattr(tgt, name):
            setattr(tgt, name, v)
    return st


def fwd_struct(o, ptrs):
    """gode_odernn_fwd_op of op `o` over the pointers ptrs[name] (params: the eight parameter pointers)."""
    opt = lambda flag, name: ptrs[name] if flag else None    # noqa: E731
    return L.OdeRnnFwdOp(p=L.OdeRnnParams(*ptrs["params"]), noise=ptrs["noise"], content=opt(o.content, "content"),
                         sel_t=opt(o.sel, "sel_t"), z=ptrs["z"], hs=opt(o.hs, "hs"), hp=ptrs["hp"], nsteps=ptrs["nsteps"], N=o.N,
                         T=o.T, rtol=RTOL, atol=ATOL, zcols=o.zcols, sync=opt(o.sync, "sync"))


def bwd_struct(o, ptrs):
    opt = lambda flag, name: ptrs[name] if flag else None    # noqa: E731
    return L.OdeRnnBwdOp(p=L.OdeRnnParams(*ptrs["params"]), noise=ptrs["noise"], hp=ptrs["hp"], sel_t=opt(o.sel, "sel_t"),
                         gz=ptrs["gz"], work=ptrs["work"], grads=ptrs["grads"], N=o.N, T=o.T, substeps=o.substeps, accumulate=o.acc,
                         zcols=o.gz_zcols, rtol=RTOL, atol=ATOL, sync=opt(o.bsync, "bsync"), nsteps=ptrs["bnsteps"])


_FAKE = ("noise", "content", "sel_t", "z", "hs", "hp", "nsteps", "sync", "gz", "work", "grads", "bsync", "bnsteps")


def fake_ptrs(k):
    """Fake non-null pointers for op k of a call (nothing dereferences them on the host)."""
    base = (k + 1) << 32
    ptrs = {n: base + ((i + 1) << 20) for i, n in enumerate(_FAKE)}
    ptrs["params"] = [base + ((32 + i) << 20) for i in range(8)]
    return ptrs


def fake_ops(ops, direction):
    """ctypes array of the call's ops over fake pointers (direction "f" / "b"); ops sharing grads share the fake pointer."""
    out = []
    for k, o in enumerate(ops):
        ptrs = fake_ptrs(k)
        if o.share is not None:
            ptrs["grads"] = fake_ptrs(o.share)["grads"]
        out.append(fwd_struct(o, ptrs) if direction == "f" else bwd_struct(o, ptrs))
    return as_array(out, direction)


def as_array(structs, direction):
    kind = L.OdeRnnFwdOp if direction == "f" else L.OdeRnnBwdOp
    return (kind * max(len(structs), 1))(*structs)


def route(arr, count, direction):
    """-> (return code, route vector as a list; None when refused)"""
    vec = (C.c_int32 * (max(count, 0) + 2))(*([-9] * (max(count, 0) + 2)))
    fn = L.lib().gode_odernn_fwd_route if direction == "f" else L.lib().gode_odernn_bwd_route
    rc = fn(arr, count, vec)
    return rc, (list(vec) if rc == 0 else None)


# ---- the float64 oracle ------------------------------------------------------------------------------------------------
def make_nets(seed):
    """The fp32 ODEFunc (Linear(16,16) - Tanh - Linear(16,16)) and GRUCell(16,16) of one op."""
    from oracle import mocogan_ref as M
    torch.manual_seed(seed)
    return M.OdeRhs(16, 16), torch.nn.GRUCell(16, 16)


def net_params(f, gru):
    return list(f.parameters()) + [gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh]


def oracle(f, gru, noise, gup, sel=None, chunk=None, dtype=torch.float64, trials=False, backward=True):
    """h' = odeint_adjoint(f, h, [0, 1])[-1] per frame, h = GRUCell(e_t, h'), on `dtype` copies of the fp32 modules and inputs.
    noise [T + 1, N, 16], gup [N, T, 16] (the upstream gradient; with sel [N] masked to frame sel[n]).  chunk: one solve per
    consecutive `chunk` trajectories (the MFMA kernels' norm per 64-trajectory workgroup); the gradient is then the sum of the
    chunks'.  -> hs [N, T + 1, 16], hp [N, T, 16], the eight gradient tensors flattened into one vector [2176] (None with
    backward=False), and (trials=True) the dopri5 trial steps per frame of the first chunk (2 evaluations for the initial step +
    6 per trial)."""
    f, gru = copy.deepcopy(f).to(dtype), copy.deepcopy(gru).to(dtype)
    calls = [0]
    f.register_forward_pre_hook(lambda *_: calls.__setitem__(0, calls[0] + 1))
    T, N = noise.shape[0] - 1, noise.shape[1]
    w = gup.to(dtype)
    if sel is not None:
        w = w * (torch.arange(T)[None, :] == sel.long()[:, None]).to(dtype)[:, :, None]
    t01 = torch.tensor([0.0, 1.0], dtype=dtype)
    step = chunk or N
    hs_all, hp_all, counts = [], [], []
    loss = 0.0
    for n0 in range(0, N, step):
        sl = slice(n0, min(N, n0 + step))
        h = [noise[0, sl].to(dtype)]
        hps = []
        for t in range(T):
            c0 = calls[0]
            hp = ode_ref.odeint_adjoint(f, h[-1], t01, rtol=RTOL, atol=ATOL)[-1]
            if n0 == 0:
                counts.append((calls[0] - c0 - 2) // 6)
            hps.append(hp)
            h.append(gru(noise[t + 1, sl].to(dtype), hp))
        hs, hp = torch.stack(h, dim=1), torch.stack(hps, dim=1)
        loss = loss + (hs[:, 1:] * w[sl]).sum()
        hs_all.append(hs.detach())
        hp_all.append(hp.detach())
    g = None
    if backward:
        loss.backward()
        g = torch.cat([p.grad.reshape(-1) for p in net_params(f, gru)])
    out = (torch.cat(hs_all), torch.cat(hp_all), g)
    return out + (counts,) if trials else out
