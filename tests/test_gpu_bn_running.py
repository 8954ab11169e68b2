"""GPU, library level: the deferred form of gode_bn_finalize followed by gode_bn_running against the in-place finalize,
bit for bit -- mean / invstd / scale / shift of every call and running_mean / running_var / num_batches_tracked after each
of three successive calls -- and gode_run_pair: argument errors, two objects used in turn, a capturing stream."""
import ctypes as C

import pytest
import torch

import gan_ode_amd._lib as L

pytestmark = pytest.mark.gpu

MOMENTUM, EPS = 0.1, 1e-5


def _st():
    return torch.cuda.current_stream().cuda_stream


def _partials(C_, rows, count, seed):
    """Partial sums [2][C][rows] of `count` values per channel with a channel-dependent mean and spread."""
    g = torch.Generator().manual_seed(seed)
    per = count / rows
    mean = torch.randn(C_, 1, generator=g) * 2.0
    std = torch.rand(C_, 1, generator=g) + 0.75
    s1 = per * (mean + 0.01 * torch.randn(C_, rows, generator=g))      # (keeps the variance well above zero)
    s2 = per * (std ** 2 + mean ** 2) * (1.0 + 0.05 * torch.rand(C_, rows, generator=g))
    return torch.stack([s1, s2]).float().contiguous().cuda()


class _Side:
    """One BatchNorm layer's tensors and its finalize op; deferred: with a slot and the running op."""

    def __init__(self, C_, rows, count, deferred, running, seed):
        f = dict(dtype=torch.float32, device="cuda")
        g = torch.Generator().manual_seed(seed)
        self.gamma, self.beta = (torch.randn(C_, generator=g).cuda() for _ in range(2))
        self.rm = torch.randn(C_, generator=g).cuda() if running else None
        self.rv = (torch.rand(C_, generator=g) + 0.5).cuda() if running else None
        self.nbt = torch.full((1,), 41, dtype=torch.int64, device="cuda")
        self.mean, self.invstd, self.scale, self.shift = (torch.zeros(C_, **f) for _ in range(4))
        self.slot = torch.full((C_,), float("nan"), **f) if deferred else None
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        self.fin = L.BnFinalizeOp(rows=rows, ncols=C_, C=C_, count=count, gamma=p(self.gamma), beta=p(self.beta),
                                  running_mean=p(self.rm), running_var=p(self.rv), num_batches_tracked=p(self.nbt),
                                  mean=p(self.mean), invstd=p(self.invstd), scale=p(self.scale), shift=p(self.shift),
                                  momentum=MOMENTUM, eps=EPS, training=1, batch_var=p(self.slot))
        self.run = L.BnRunningOp(n=1, momentum=MOMENTUM)
        y = self.run.layer[0]
        y.mean, y.var, y.C = p(self.mean), p(self.slot), C_
        y.running_mean, y.running_var, y.num_batches_tracked = p(self.rm), p(self.rv), p(self.nbt)

    def state(self):
        ts = [self.mean, self.invstd, self.scale, self.shift, self.nbt] + ([self.rm, self.rv] if self.rm is not None else [])
        return [t.clone() for t in ts]


@pytest.mark.parametrize("running", [True, False], ids=["running", "running_null"])
@pytest.mark.parametrize("rows", [1, 7, 1024])
@pytest.mark.parametrize("C_", [8, 64])
def test_deferred_finalize_plus_running_op_gives_the_bits_of_the_in_place_finalize(C_, rows, running):
    lib = L.lib()
    count = rows * 48
    a = _Side(C_, rows, count, False, running, seed=C_ + rows)
    b = _Side(C_, rows, count, True, running, seed=C_ + rows)
    for call in range(3):
        stats = _partials(C_, rows, count, seed=1000 * call + rows + C_)
        a.fin.stats = b.fin.stats = stats.data_ptr()
        assert lib.gode_bn_finalize(C.byref(a.fin), _st()) == 0
        before = b.state()[4:]
        assert lib.gode_bn_finalize(C.byref(b.fin), _st()) == 0
        for x, y in zip(before, b.state()[4:]):     # the deferred form leaves the running tensors and the counter alone
            assert torch.equal(x, y)
        assert lib.gode_bn_running(C.byref(b.run), _st()) == 0
        sa, sb = a.state(), b.state()
        for k, (x, y) in enumerate(zip(sa, sb)):
            assert torch.equal(x, y), (call, k, (x.view(-1)[:4], y.view(-1)[:4]))
        assert int(sb[4]) == 42 + call
        if running:      # ... and the update did move them: the comparison above is not of two untouched tensors
            assert not torch.equal(before[1], sb[5]) and not torch.equal(before[2], sb[6])
        assert torch.isfinite(b.slot).all()


def test_one_value_per_channel_keeps_the_biased_variance_in_both_forms():
    lib = L.lib()
    a, b = (_Side(8, 1, 1, d, True, seed=3) for d in (False, True))
    stats = torch.tensor([[[0.5]] * 8, [[0.25]] * 8], device="cuda")
    a.fin.stats = b.fin.stats = stats.data_ptr()
    assert lib.gode_bn_finalize(C.byref(a.fin), _st()) == 0
    assert lib.gode_bn_finalize(C.byref(b.fin), _st()) == 0 and lib.gode_bn_running(C.byref(b.run), _st()) == 0
    for x, y in zip(a.state(), b.state()):
        assert torch.equal(x, y)


def test_several_layers_in_one_launch_and_the_refusals():
    lib = L.lib()
    sides = [(_Side(c, 7, 7 * 48, False, True, seed=c), _Side(c, 7, 7 * 48, True, True, seed=c)) for c in (8, 64, 300)]
    run = L.BnRunningOp(n=3, momentum=MOMENTUM)
    for k, (a, b) in enumerate(sides):
        stats = _partials(a.fin.C, 7, 7 * 48, seed=k)
        a.fin.stats = b.fin.stats = stats.data_ptr()
        assert lib.gode_bn_finalize(C.byref(a.fin), _st()) == 0 and lib.gode_bn_finalize(C.byref(b.fin), _st()) == 0
        run.layer[k] = b.run.layer[0]
        torch.cuda.synchronize()      # (`stats` goes out of scope)
    assert lib.gode_bn_running(C.byref(run), _st()) == 0
    for a, b in sides:
        for x, y in zip(a.state(), b.state()):
            assert torch.equal(x, y)
    b = sides[0][1]
    for k, v in (("groups", 2), ("training", 0), ("nseg", 1)):
        op = L.BnFinalizeOp.from_buffer_copy(b.fin)
        setattr(op, k, v)
        if k == "groups":
            op.rows0 = 1
        assert lib.gode_bn_finalize(C.byref(op), _st()) == -1, k
    run.n = L.BN_RUNNING_MAX + 1
    assert lib.gode_bn_running(C.byref(run), _st()) == -1
    run.n, run.layer[1].var = 3, None
    assert lib.gode_bn_running(C.byref(run), _st()) == -1


def _chain(x):
    """Three ops y -> relu -> negate-free copies: out = relu(x) through two intermediates."""
    bufs = [torch.zeros_like(x) for _ in range(3)]
    srcs = [x] + bufs[:2]
    ops = [L.BnApplyOp(y=s.data_ptr(), out=d.data_ptr(), M=64, C=64, act=L.ACT_RELU if k == 0 else L.ACT_NONE)
           for k, (s, d) in enumerate(zip(srcs, bufs))]
    kinds, ptrs = (L.i32 * 3)(*[o.KIND for o in ops]), (L.ptr * 3)(*[C.addressof(o) for o in ops])
    return bufs, ops, kinds, ptrs


def test_run_pair_argument_errors_two_objects_in_turn_and_a_capturing_stream():
    lib = L.lib()
    ha, hb = L.ptr(), L.ptr()
    assert lib.gode_lanes_create(C.byref(ha)) == 0 and lib.gode_lanes_create(C.byref(hb)) == 0
    x = torch.arange(4096, dtype=torch.float32, device="cuda").view(64, 64) - 2000.0
    (bufs_a, ops_a, ka, pa), (bufs_b, ops_b, kb, pb) = _chain(x), _chain(x)
    st = _st()
    for args in ((None, hb, ka, pa, 3, 1, 0, st), (ha, ha, ka, pa, 3, 1, 0, st), (ha, hb, ka, pa, 3, 0, 0, st),
                 (ha, hb, ka, pa, 3, 3, 0, st), (ha, hb, ka, pa, 3, 1, 2, st), (ha, hb, None, pa, 3, 1, 0, st)):
        assert lib.gode_run_pair(*args) == -1, args
    # a capture takes every op on the capturing stream, in order: the replayed graph writes what one stream writes
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cst = torch.cuda.current_stream().cuda_stream
        assert lib.gode_run_pair(ha, hb, ka, pa, 3, 1, L.LANES_OVERLAP, cst) == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bufs_a[2], x.clamp_min(0))
    # outside a capture: the two objects in turn, no synchronisation in between; a reader queued on the caller's stream
    # behind each call sees the whole program's result
    reads = []
    for k in range(6):
        bufs, kinds, ptrs, own, peer = (bufs_a, ka, pa, ha, hb) if k % 2 == 0 else (bufs_b, kb, pb, hb, ha)
        x.add_(1.0)                       # queued on the caller's stream: the next call reads it, so that call is ORDERED
        assert lib.gode_run_pair(own, peer, kinds, ptrs, 3, 1, L.LANES_ORDERED, st) == 0
        reads.append((bufs[2].clone(), x.clamp_min(0)))
    y = torch.full_like(x, 3.0)
    (bufs_c, ops_c, kc, pc), (bufs_d, ops_d, kd, pd) = _chain(y), _chain(y)
    for k in range(6):                    # ... and overlapping: nothing the programs read is written in between
        bufs, kinds, ptrs, own, peer = (bufs_c, kc, pc, ha, hb) if k % 2 == 0 else (bufs_d, kd, pd, hb, ha)
        assert lib.gode_run_pair(own, peer, kinds, ptrs, 3, 1, L.LANES_OVERLAP, st) == 0
        reads.append((bufs[2].clone(), y))
        bufs[2].zero_()                   # on the caller's stream, behind the call: the plan's next call rewrites it
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(reads):
        assert torch.equal(got, want), k
    del g
    assert lib.gode_lanes_destroy(ha) == 0 and lib.gode_lanes_destroy(hb) == 0
