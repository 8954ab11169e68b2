"""Stage-1 block, host side: the plain-torch restatement (tests/gres_ref.py) against the fixtures the reference's own
GResBlock wrote (scripts/make_gres_golden.py), the HIP module's construction against the same fixtures, and the ABI mirrors.

conv0's bias gradient in the bn cases is zero in exact arithmetic (the bias sits in front of a train-mode BatchNorm); the
fp32 reference returns rounding noise there (spread/g/conv0.module.bias ~ 3e8 against its fp64 run), so a relative error
against it is undefined: that one tensor is held to TOL times its natural scale, sum |g| of conv0's output, recorded by the
golden script."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gres_ref
from conftest import golden, rel_err, seed_all
from gres_cases import CASES

TOL = 1e-5


def ref_block(case):
    return gres_ref.GResBlock(case["cin"], case["cout"], n_class=case["n_class"], bn=case["bn"], upsample_factor=case["up"],
                              downsample_factor=case["down"])


def load_sd0(blk, g):
    blk.load_state_dict({k: torch.from_numpy(np.asarray(g[f"sd0/{k}"])).clone() for k in blk.state_dict()}, strict=True)
    return blk


def grad_err(name, got, g, case):
    """rel_err, except for the identically-zero bias gradient described in the module docstring.  The HIP path returns exact
    zeros for that tensor, so this form cannot fail there; its real check is the op test of gode_cbn_bwd's dbias."""
    if name == "conv0.module.bias" and case["bn"] and case["down"] == 1:
        return float(np.abs(np.asarray(got, dtype=np.float64) - g[f"g/{name}"]).max() / float(g["scale/g/conv0.module.bias"]))
    return rel_err(got, g[f"g/{name}"])


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_reference_fixture(name):
    case, g = CASES[name], golden(f"gres_tiny_{name}.npz")
    assert float(g["margin"]) >= 1e-4
    blk = load_sd0(ref_block(case), g)
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    cond = torch.from_numpy(g["condition"]).requires_grad_(True)
    y1 = blk(x, cond)
    y1.backward(torch.from_numpy(g["gy"]))
    assert rel_err(y1.detach(), g["y1"]) < TOL
    assert rel_err(x.grad, g["g/x"]) < TOL
    if "g/condition" in g.files:
        assert rel_err(cond.grad, g["g/condition"]) < TOL
    else:
        assert cond.grad is None
    for k, p in blk.named_parameters():
        if f"g/{k}" in g.files:
            assert grad_err(k, p.grad, g, case) < TOL, k
        else:
            assert p.grad is None, k
    y2 = blk(x.detach(), cond.detach())
    assert rel_err(y2.detach(), g["y2"]) < TOL
    for k, v in blk.state_dict().items():
        assert rel_err(v.double(), g[f"sd2/{k}"].astype(np.float64)) < TOL, k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(g[f"sd2/{k}"]), k
    blk.eval()
    assert rel_err(blk(x.detach(), cond.detach()).detach(), g["y_eval"]) < TOL


def hip_block(case):
    import gan_ode_amd as G
    return G.GResBlock(case["cin"], case["cout"], [3, 3], n_class=case["n_class"], bn=case["bn"], upsample_factor=case["up"],
                       downsample_factor=case["down"])


@pytest.mark.parametrize("name", list(CASES))
def test_seeded_construction_is_bit_identical(name):
    case, g = CASES[name], golden(f"gres_tiny_{name}.npz")
    seed_all(int(g["seed"]))
    blk = hip_block(case)
    sd = blk.state_dict()
    assert list(sd) == [k[4:] for k in g.files if k.startswith("sd0/")]
    for k, v in sd.items():
        assert v.shape == g[f"sd0/{k}"].shape and np.array_equal(v.numpy(), g[f"sd0/{k}"]), k
    for k, p in blk.named_parameters():
        assert p.requires_grad == (not k.endswith(("weight_u", "weight_v"))), k
    assert not hasattr(blk.conv0.module, "weight") or "weight" not in blk.conv0.module._parameters


def test_drop_in_module_exports():
    import importlib
    m = importlib.import_module("stage1.GResBlock")
    import gan_ode_amd.gres as gres
    for n in ("l2normalize", "SpectralNorm", "ConditionalNorm", "GResBlock"):
        assert getattr(m, n) is getattr(gres, n)
    v = torch.tensor([3.0, 4.0])
    assert torch.allclose(m.l2normalize(v), v / 5.0)


@pytest.mark.parametrize("kw", [dict(activation=F.leaky_relu), dict(stride=2), dict(kernel_size=[3, 3], padding=0),
                                dict(kernel_size=[5, 3], padding=1), dict(upsample_factor=3), dict(downsample_factor=4),
                                dict(upsample_factor=0)])
def test_unsupported_configurations_are_refused(kw):
    import gan_ode_amd as G
    with pytest.raises(NotImplementedError):
        G.GResBlock(3, 8, **kw)


def test_supported_nondefault_configurations_construct():
    import gan_ode_amd as G
    G.GResBlock(3, 8, kernel_size=[5, 5], padding=2)
    G.GResBlock(3, 8, kernel_size=1, padding=0, upsample_factor=1)
    b = G.GResBlock(3, 8, upsample_factor=2, downsample_factor=2)
    assert b.upsample_factor == 1 and b.bn is False and hasattr(b, "CBNorm1")


def test_no_cpu_fallback():
    import gan_ode_amd as G
    blk = G.GResBlock(3, 8, n_class=6)
    with pytest.raises(RuntimeError):
        blk(torch.randn(2, 3, 4, 4), torch.rand(2, 6))
    with pytest.raises(RuntimeError):
        G.ConditionalNorm(3, 6)(torch.randn(2, 3, 4, 4), torch.rand(2, 6))


def test_struct_sizes_match_the_library():
    from gan_ode_amd import _lib as L
    lib = L.lib()
    kinds = {L.OP_CHSTATS: L.ChstatsOp, L.OP_CBN_EMBED: L.CbnEmbedOp, L.OP_CBN_EMBED_BWD: L.CbnEmbedBwdOp,
             L.OP_CBN_APPLY: L.CbnApplyOp, L.OP_CBN_BWD: L.CbnBwdOp, L.OP_GRES_OUT: L.GresOutOp,
             L.OP_GRES_OUT_BWD: L.GresOutBwdOp, L.OP_SN_FWD: L.SnOp, L.OP_SN_BWD: L.SnBwdOp}
    assert sorted(kinds) == list(range(24, 33))
    for kind, st in kinds.items():
        assert lib.gode_sizeof(kind) == C.sizeof(st) and st.KIND == kind, kind
    assert lib.gode_version() == 105
    assert lib.gode_chstats_rows(1) == 1 and lib.gode_chstats_rows(120) == 2 and lib.gode_chstats_rows(10 ** 9) == 1024
    assert lib.gode_cbn_bwd_work_size(4, 5, 6, 3) > 4 * 5 * 6 * 3 and lib.gode_cbn_bwd_work_size(0, 5, 6, 3) < 0
    assert lib.gode_gres_out_bwd_work_size(4, 5, 6, 10, 2, 2) < 0     # up and down together are refused
