"""GPU: the FusedAdam class -- its rows without a gradient, its fall-back for a parameter on a lagging step count, its
grads= / gscale override, its refusals under graph capture and its pointer table -- against libgode's entry points
(gode_adam_multi, gode_adam_noise_multi, gode_adam_l2, gode_param_noise) driven directly on hand-built tables.  Both
sides run the same kernels on the same values at the same alignments, so every comparison is bitwise."""
import ctypes as C

import pytest
import torch

import wgan_ref as W
from guarded import guarded_tensors, guards_are_nan

import gan_ode_amd as G
import gan_ode_amd._lib as L

pytestmark = pytest.mark.gpu

# the smallest sizes that reach every branch of adam_tensor / adam_noise_tensor (elementwise.hip)
SIZES = [1, 5, 64, 1003, 4099]
LR, B1, B2, EPS, WD = 2e-4, 0.5, 0.999, 1e-8, 1e-5          # FusedAdam's defaults
NOISE = dict(noise_sigma=1e-3, noise_seed=99, noise_stream=1)
SEED, NSTREAM, SIGMA = 99, 1, 1e-3
ALL = [True] * 5
TWO_NONE = [True, False, True, True, False]
NO_GRAD = [False] * 5


def stream():
    return torch.cuda.current_stream().cuda_stream


def _values(sizes=SIZES):
    rng = torch.Generator().manual_seed(4)
    return [torch.randn(n, generator=rng) for n in sizes], [torch.randn(n, generator=rng) for n in sizes]


class _Oracle:
    """p, g, m, v in guarded buffers and the entry points on tables over them."""

    def __init__(self, sizes, init, grads, gviews=None):
        self.sizes = sizes
        self.bufs = [guarded_tensors(sizes) for _ in range(4)]
        self.P, self.G, self.M, self.V = [b[1] for b in self.bufs]
        for k in range(len(sizes)):
            self.P[k].copy_(init[k]); self.G[k].copy_(grads[k]); self.M[k].zero_(); self.V[k].zero_()
        if gviews is not None:
            self.G = gviews
        self.tables = []

    def launch(self, ks, step, has_grad=ALL, offs=None, nstep=0, gscale=1.0):
        """One table launch over the tensors ks.  offs given: Adam + noise, a row without a gradient is noise-only."""
        rows = []
        for k in ks:
            row = [self.P[k].data_ptr()] + [t[k].data_ptr() if has_grad[k] else 0 for t in (self.G, self.M, self.V)]
            rows.append(row + [self.sizes[k]] + ([offs[k]] if offs is not None else []))
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        self.tables.append(table)
        lib, max_n = L.lib(), max(self.sizes[k] for k in ks)
        if offs is None:
            L.check(lib.gode_adam_multi(table.data_ptr(), len(ks), max_n, LR, B1, B2, EPS, WD, gscale, step, stream()),
                    "gode_adam_multi")
        else:
            L.check(lib.gode_adam_noise_multi(table.data_ptr(), len(ks), max_n, LR, B1, B2, EPS, WD, gscale, step, SEED,
                                              NSTREAM, nstep, SIGMA, stream()), "gode_adam_noise_multi")

    def single(self, k, step, off=None, nstep=0):
        """gode_adam_l2 on tensor k; off given: gode_param_noise behind it."""
        lib = L.lib()
        op = L.AdamOp(p=self.P[k].data_ptr(), g=self.G[k].data_ptr(), m=self.M[k].data_ptr(), v=self.V[k].data_ptr(),
                      n=self.sizes[k], lr=LR, beta1=B1, beta2=B2, eps=EPS, weight_decay=WD, gscale=1.0, step=step)
        L.check(lib.gode_adam_l2(C.byref(op), stream()), "gode_adam_l2")
        if off is not None:
            L.check(lib.gode_param_noise(self.P[k].data_ptr(), self.sizes[k], SEED, NSTREAM, nstep, off, SIGMA, 1, stream()),
                    "gode_param_noise")

    def guards_ok(self):
        return all(guards_are_nan(b, views) for b, views in self.bufs)


class _Side:
    """The class's side: nn.Parameters over views of one guarded buffer, gradients over views of another."""

    def __init__(self, sizes, init, grads):
        self.pbuf, self.pv = guarded_tensors(sizes)
        self.gbuf, self.gv = guarded_tensors(sizes)
        self.params = []
        for k in range(len(sizes)):
            self.pv[k].copy_(init[k]); self.gv[k].copy_(grads[k])
            self.params.append(torch.nn.Parameter(self.pv[k]))
            assert self.params[k].data_ptr() == self.pv[k].data_ptr()

    def set_grads(self, mask):
        for p, g, has in zip(self.params, self.gv, mask):
            p.grad = g if has else None

    def guards_ok(self):
        return guards_are_nan(self.pbuf, self.pv) and guards_are_nan(self.gbuf, self.gv)


def _vers(params):
    return [getattr(p, "_gode_ver", 0) for p in params]


def _assert_same(opt, params, ora, ks=None, stateless=()):
    """p, exp_avg, exp_avg_sq of the class bitwise the oracle's; parameters in `stateless` never got a state."""
    torch.cuda.synchronize()
    for j, p in enumerate(params):
        k = j if ks is None else ks[j]
        assert torch.equal(p.data, ora.P[k]), k
        if j in stateless:
            assert not opt.state.get(p), k
        else:
            assert torch.equal(opt.state[p]["exp_avg"], ora.M[k]), k
            assert torch.equal(opt.state[p]["exp_avg_sq"], ora.V[k]), k
    assert ora.guards_ok()


@pytest.mark.parametrize("mask", [ALL, TWO_NONE, NO_GRAD], ids=["all", "two_none", "no_grad"])
def test_plain_steps_skip_parameters_without_a_gradient(mask):
    init, grads = _values()
    side, ora = _Side(SIZES, init, grads), _Oracle(SIZES, init, grads)
    opt = G.FusedAdam(side.params)
    side.set_grads(mask)
    ks = [k for k in range(5) if mask[k]]
    for step in (1, 2):
        opt.step()
        if ks:
            ora.launch(ks, step)
    none = [k for k in range(5) if not mask[k]]
    _assert_same(opt, side.params, ora, stateless=none)
    assert side.guards_ok()
    for k in none:                               # untouched altogether
        assert torch.equal(side.params[k].data.cpu(), init[k])
    assert _vers(side.params) == [2 if m else 0 for m in mask]
    assert "noise_step" not in opt.param_groups[0]


@pytest.mark.parametrize("mask", [ALL, TWO_NONE, NO_GRAD], ids=["all", "two_none", "no_grad"])
def test_noisy_steps_give_parameters_without_a_gradient_noise_only_rows(mask):
    init, grads = _values()
    side, ora = _Side(SIZES, init, grads), _Oracle(SIZES, init, grads)
    opt = G.FusedAdam(side.params, **NOISE)
    side.set_grads(mask)
    offs = W.noise_offsets(side.params)
    for step in (1, 2):
        opt.step()
        ora.launch(range(5), step, has_grad=mask, offs=offs, nstep=step)
    none = [k for k in range(5) if not mask[k]]
    _assert_same(opt, side.params, ora, stateless=none)
    assert side.guards_ok()
    for k in none:                               # (noised, not left alone)
        assert not torch.equal(side.params[k].data.cpu(), init[k])
    assert opt.param_groups[0]["noise_step"] == 2
    assert _vers(side.params) == [2] * 5


def test_second_noisy_group_continues_the_offsets_of_the_first():
    init, grads = _values()
    side, ora = _Side(SIZES, init, grads), _Oracle(SIZES, init, grads)
    opt = G.FusedAdam([dict(params=side.params[:3]), dict(params=side.params[3:])], **NOISE)
    mask = [True, False, True, True, True]
    side.set_grads(mask)
    offs = W.noise_offsets(side.params)          # group 1 starts at the roundup4 sum of group 0: 4 + 8 + 64
    assert offs[3] == 76
    for step in (1, 2):
        opt.step()
        ora.launch([0, 1, 2], step, has_grad=mask, offs=offs, nstep=step)
        ora.launch([3, 4], step, has_grad=mask, offs=offs, nstep=step)
    _assert_same(opt, side.params, ora, stateless=[1])
    assert side.guards_ok()
    assert [g["noise_step"] for g in opt.param_groups] == [2, 2]


def test_grads_override_from_a_flat_buffer_with_gscale():
    init, grads = _values()
    side = _Side(SIZES, init, grads)
    flats = [torch.cat([g * 3.0 for g in grads]).cuda() for _ in range(2)]       # (the class's, the oracle's)
    views = [list(f.split(SIZES)) for f in flats]
    ora = _Oracle(SIZES, init, grads, gviews=views[1])
    opt = G.FusedAdam(side.params)
    side.set_grads(ALL)                          # .grad is set and must not be read; parameter 2 is not in the dict
    ks = [0, 1, 3, 4]
    for step in (1, 2):
        opt.step(grads={side.params[k]: views[0][k] for k in ks}, gscale=0.5)
        ora.launch(ks, step, gscale=0.5)
    _assert_same(opt, side.params, ora, stateless=[2])
    assert side.guards_ok()
    assert torch.equal(side.params[2].data.cpu(), init[2])


@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "noisy"])
def test_parameter_on_a_lagging_step_takes_the_single_tensor_path(noisy):
    init, grads = _values()
    side, ora = _Side(SIZES, init, grads), _Oracle(SIZES, init, grads)
    opt = G.FusedAdam(side.params, **(NOISE if noisy else {}))
    offs = W.noise_offsets(side.params) if noisy else None
    lag, rest = 3, [0, 1, 2, 4]
    first = [k != lag for k in range(5)]
    side.set_grads(first)
    opt.step()
    side.set_grads(ALL)
    opt.step()                                   # parameter 3 on step 1, the others on step 2
    if noisy:
        ora.launch(range(5), 1, has_grad=first, offs=offs, nstep=1)
        ora.single(lag, 1, off=offs[lag], nstep=2)
        ora.launch(rest, 2, offs=offs, nstep=2)
    else:
        ora.launch(rest, 1)
        ora.single(lag, 1)
        ora.launch(rest, 2)
    _assert_same(opt, side.params, ora)
    assert side.guards_ok()
    assert [int(opt.state[p]["step"]) for p in side.params] == [2, 2, 2, 1, 2]


def _snapshot(opt, side):
    torch.cuda.synchronize()
    return [(p.data.clone(), {k: v.clone() for k, v in opt.state.get(p, {}).items() if k != "step"}) for p in side.params]


def _assert_untouched(opt, side, snap):
    torch.cuda.synchronize()
    for p, (data, st) in zip(side.params, snap):
        assert torch.equal(p.data, data)
        for k, v in st.items():
            assert torch.equal(opt.state[p][k], v)
        for k in ("exp_avg", "exp_avg_sq"):      # a state created by the refused call is still all zero
            if k not in st and opt.state.get(p):
                assert not opt.state[p][k].any()
    assert side.guards_ok()


@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "noisy"])
def test_capture_refuses_a_group_on_two_step_counts(noisy):
    init, grads = _values()
    side = _Side(SIZES, init, grads)
    opt = G.FusedAdam(side.params, **(NOISE if noisy else {}))
    side.set_grads([k != 3 for k in range(5)])
    opt.step()
    side.set_grads(ALL)
    snap = _snapshot(opt, side)
    with pytest.raises(RuntimeError, match="all parameters of a group on the same Adam step"):
        opt.step(feed=object())
    _assert_untouched(opt, side, snap)


@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "noisy"])
def test_capture_refuses_a_first_step(noisy):
    init, grads = _values()
    side = _Side(SIZES, init, grads)
    opt = G.FusedAdam(side.params, **(NOISE if noisy else {}))
    side.set_grads(ALL)
    snap = _snapshot(opt, side)
    with pytest.raises(RuntimeError, match="the Adam pointer table must exist already"):
        opt.step(feed=object())
    _assert_untouched(opt, side, snap)


@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "noisy"])
def test_cpu_parameter_is_refused(noisy):
    p = torch.nn.Parameter(torch.arange(7.0))
    p.grad = torch.ones(7)
    opt = G.FusedAdam([p], **(NOISE if noisy else {}))
    with pytest.raises(RuntimeError, match="runs only on the GPU"):
        opt.step()
    assert torch.equal(p.data, torch.arange(7.0))


@pytest.mark.parametrize("noisy", [False, True], ids=["plain", "noisy"])
def test_pointer_table_is_uploaded_only_when_a_pointer_changed(noisy):
    init, grads = _values()
    side, ora = _Side(SIZES, init, grads), _Oracle(SIZES, init, grads)
    opt = G.FusedAdam(side.params, **(NOISE if noisy else {}))
    offs = W.noise_offsets(side.params) if noisy else None
    side.set_grads(ALL)
    opt.step()
    table = opt.pointer_table(0)
    dev = table.dev
    assert table.uploads == 1 and tuple(dev.shape) == (5, 6 if noisy else 5)
    opt.step()
    assert opt.pointer_table(0) is table and table.dev is dev and table.uploads == 1
    side.params[2].grad = side.gv[2].clone()     # the same values at another address
    opt.step()
    assert table.uploads == 2
    assert int(table.dev[2, 1]) == side.params[2].grad.data_ptr()
    for step in (1, 2, 3):
        ora.launch(range(5), step, offs=offs, nstep=step)
    _assert_same(opt, side.params, ora)
    assert side.guards_ok()
