"""GPU: the autograd glue between the public API and the plans -- the one loss node (train._LossFn) behind the twelve
public loss functions and the one discriminator node (modules._DiscFn) behind forward / forward_pair_joint.  These nodes
can only go wrong in indexing (which input, which offset, which gradient slot), so the shapes are tiny."""
import pytest
import torch

from conftest import seed_all

import gan_ode_amd as G
import gan_ode_amd._lib as L

pytestmark = pytest.mark.gpu
C = 3


def _labels(n, seed):
    return torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(seed)).cuda()


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


# name -> (shapes of the tensor inputs, call(*tensors))
LOGITS, JOINT, HEAD, JOINT_HEAD, PATCH_HEAD = (5,), (6, 1, 1, 1, 1), (4, 1 + C), (8, 1 + C), (2, 1, 2, 2, 1 + C)
BCE_CE = {
    "bce_with_logits_const": ([LOGITS], lambda a: G.bce_with_logits_const(a, 0.9)),
    "bce_with_logits_pair": ([LOGITS, JOINT], lambda a, b: G.bce_with_logits_pair(a, 1.0, b, 0.0)),
    "bce_with_logits_halves": ([JOINT], lambda a: G.bce_with_logits_halves(a, 1.0, 0.0)),
    "categorical_cross_entropy": ([(4, C)], lambda a: G.categorical_cross_entropy(a, _labels(4, 1))),
    "bce_ce_head": ([HEAD], lambda a: G.bce_ce_head(a, 1.0, _labels(4, 2))),
    "bce_ce_head/patch": ([PATCH_HEAD], lambda a: G.bce_ce_head(a, 1.0, _labels(2, 3))),
    "bce_ce_head_pair": ([HEAD, LOGITS], lambda a, b: G.bce_ce_head_pair(a, 1.0, _labels(4, 4), b, 1.0)),
    "bce_ce_head_halves": ([JOINT_HEAD], lambda a: G.bce_ce_head_halves(a, 1.0, 0.0, _labels(4, 5))),
    "bce_ce_heads": ([HEAD, HEAD], lambda a, b: G.bce_ce_heads(a, 1.0, _labels(4, 6), b, 0.0)),
}
WGAN = {
    "wasserstein_generator_loss": ([LOGITS], lambda a: G.wasserstein_generator_loss(a)),
    "wasserstein_generator_loss_pair": ([LOGITS, JOINT], lambda a, b: G.wasserstein_generator_loss_pair(a, b)),
    "wasserstein_discriminator_loss": ([LOGITS, LOGITS], lambda a, b: G.wasserstein_discriminator_loss(a, b)),
    "wasserstein_discriminator_loss_halves": ([JOINT], lambda a: G.wasserstein_discriminator_loss_halves(a)),
}


def _inputs(shapes):
    return [_rand(s, 10 + i).requires_grad_() for i, s in enumerate(shapes)]


@pytest.mark.parametrize("name", list(BCE_CE))
def test_upstream_gradient_scales_the_stored_gradients(name):
    """backward(gradient=unit_grad) hands the stored gradients on as they are; any other upstream gradient multiplies
    them: (loss * 3).backward() gives exactly 3 x the unit gradients (one fp32 product per element) and the same loss."""
    shapes, call = BCE_CE[name]
    xs1, xs3 = _inputs(shapes), _inputs(shapes)
    loss1 = call(*xs1)
    loss1.backward(gradient=G.unit_grad(loss1.device))
    loss3 = call(*xs3)
    (loss3 * 3.0).backward()
    assert torch.equal(loss1.detach(), loss3.detach()) and bool(torch.isfinite(loss1))
    for a, b in zip(xs1, xs3):
        assert a.grad.shape == a.shape and bool(a.grad.abs().sum() > 0)
        assert torch.equal(b.grad, a.grad * 3.0)


def test_cross_entropy_reads_a_view_of_a_head_in_place():
    """categ = head[:, 1:] (rows 1 + C apart) is read where it lies and gives, bit for bit, what its compact clone gives;
    the gradient reaches the head through the view: column 0 zero, the class columns the clone's gradient."""
    labels = _labels(4, 1)
    got = {}
    for how in ("view", "clone"):
        head = _rand(HEAD, 20).requires_grad_()
        categ = head[:, 1:] if how == "view" else head[:, 1:].clone()
        assert categ.is_contiguous() == (how == "clone")
        g1 = {}
        for scale in (1.0, 3.0):
            head.grad = None
            loss = G.categorical_cross_entropy(categ, labels)
            if scale == 1.0:
                loss.backward(gradient=G.unit_grad(loss.device), retain_graph=True)
            else:
                (loss * scale).backward()
            g1[scale] = head.grad.clone()
        assert torch.equal(g1[3.0], g1[1.0] * 3.0)
        got[how] = (loss.detach().clone(), g1[1.0])
    assert torch.equal(got["view"][0], got["clone"][0]) and torch.equal(got["view"][1], got["clone"][1])
    g = got["view"][1]
    assert g.shape == HEAD and bool((g[:, 0] == 0).all()) and bool(g[:, 1:].abs().sum() > 0)


# the libgode launches of each public loss call, in order (read off the five loss nodes this one replaced): per launch
# (op, input, first element) -- where the op's `logits` / `fake` pointer must point.  The order is the order of the fp32 sum.
B_, CE_, W_ = L.BceOp, L.CeOp, L.WganOp
LAUNCHES = {
    "bce_with_logits_const": [(B_, 0, 0)], "categorical_cross_entropy": [(CE_, 0, 0)],
    "wasserstein_generator_loss": [(W_, 0, 0)], "wasserstein_discriminator_loss": [(W_, 1, 0)],
    "wasserstein_discriminator_loss_halves": [(W_, 0, 3)],
    "bce_with_logits_pair": [(B_, 0, 0), (B_, 1, 0)], "bce_with_logits_halves": [(B_, 0, 0), (B_, 0, 3)],
    "bce_ce_head": [(B_, 0, 0), (CE_, 0, 1)], "bce_ce_head/patch": [(B_, 0, 0), (CE_, 0, 1)],
    "wasserstein_generator_loss_pair": [(W_, 0, 0), (W_, 1, 0)],
    "bce_ce_head_pair": [(B_, 0, 0), (B_, 1, 0), (CE_, 0, 1)],
    "bce_ce_head_halves": [(B_, 0, 0), (B_, 0, 4 * (1 + C)), (CE_, 0, 1)],
    "bce_ce_heads": [(B_, 0, 0), (B_, 1, 0), (CE_, 0, 1), (CE_, 1, 1)],
}
# the two-tensor Wasserstein terms also read `real`: input 0 from its first element
REAL = {"wasserstein_discriminator_loss": (0, 0), "wasserstein_discriminator_loss_halves": (0, 0)}


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_launches_per_loss_call(name):
    shapes, call = {**BCE_CE, **WGAN}[name]
    xs = _inputs(shapes)
    L.TRACE = []
    try:
        loss = call(*xs)
        forward = [op for op, _, _ in L.TRACE]
        loss.backward(gradient=G.unit_grad(loss.device))
        (call(*xs) * 3.0).backward()
        total = len(L.TRACE)
    finally:
        L.TRACE = None
    torch.cuda.synchronize()
    assert [type(op) for op in forward] == [cls for cls, _, _ in LAUNCHES[name]]
    for k, (op, (cls, i, first)) in enumerate(zip(forward, LAUNCHES[name])):
        assert (op.fake if cls is W_ else op.logits) == xs[i].data_ptr() + 4 * first, (name, k)
        assert op.accumulate == (1 if k else 0) and op.loss == loss.data_ptr(), (name, k)
        if cls is W_:
            want = REAL.get(name)
            assert op.real == (None if want is None else xs[want[0]].data_ptr() + 4 * want[1]), (name, k)
    assert total == 2 * len(forward)          # neither backward launched anything through libgode


# -- the discriminator node -------------------------------------------------------------------------------------------------
DISCS = {"image": (lambda: G.PatchImageDiscriminator(1, ndf=8), (2, 1, 28, 28)),
         "video": (lambda: G.VideoDiscriminator(1, ksize=2, ndf=8), (4, 1, 16, 28, 28))}


@pytest.mark.parametrize("kind", list(DISCS))
def test_discriminator_node_without_an_arena(kind):
    make, shape = DISCS[kind]
    seed_all(7)
    dis = make().cuda()
    params = list(dis.parameters())
    x, y = torch.rand(shape).cuda(), torch.rand(shape).cuda()

    # single pass, frozen parameters: only the input receives a gradient
    for p in params:
        p.requires_grad_(False)
    xg = x.clone().requires_grad_()
    out, _ = dis(xg)
    out.sum().backward()
    assert xg.grad.shape == xg.shape and bool(xg.grad.abs().sum() > 0)
    assert all(p.grad is None for p in params)

    # the paired pass is the discriminator-update pass: an input that wants a gradient is refused
    with pytest.raises(RuntimeError, match="inputs must be detached"):
        dis.forward_pair_joint(xg, y)
    with pytest.raises(RuntimeError, match="inputs must be detached"):
        dis.forward_pair_joint(y, xg)

    # trainable parameters, no arena: both arities hand every parameter a gradient of its own shape
    for p in params:
        p.requires_grad_(True)
    for run in (lambda: dis(x)[0], lambda: dis.forward_pair_joint(x, y)):
        for p in params:
            p.grad = None
        run().sum().backward()
        for p in params:
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all())
    assert x.grad is None and y.grad is None
