"""Writes tests/golden/odegan_tiny.npz by running the REFERENCE's GANODETrainer (stage2/ode_training.py, imported from
the read-only reference checkout, not copied) on CPU, on stock torch.nn copies of the tiny networks (oracle/mocogan_ref.py
with the weights of the existing tiny fixtures).  Runs in the build container only; no test imports this file or reads
the reference.

  python scripts/make_odegan_goldens.py

Contents (data only):
  quad/init/<t>, quad/<method>/<t>            the quadratic problem of tests/odegan_cases.py before / after one step
  d<img|vid>/fake                              the fixed fake batch (float16-exact)
  d<img|vid>/<method>/delta/<param>            parameter change of one reg=0 step, reference in fp32
  d<img|vid>/<method>/self/<param>             max|delta32 - delta64| / max|delta64|: the reference against itself in fp64
  gen/rk4/delta/<param>, gen/rk4/self/<param>  the same for one RK4 generator step (recurrent.*: empty arrays, untouched)
  pen/exact/<param>                            grad_thetaD ||grad_thetaG L_G||^2 by double backward in fp64 (stored as float32)
  pen/err32/<param>                            max|gp - exact| / max|exact| of the central difference of tests/odegan_ref.py
                                               run in fp32 on CPU (h = eps32^(1/3))
  pen/central64/<param>, pen/self/<param>      that central difference in fp64, and max|gp32 - gp64| / max|gp64|
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import odegan_cases as K  # noqa: E402
import odegan_ref as R  # noqa: E402
from oracle import mocogan_ref as M  # noqa: E402
from oracle import ode_ref  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")


def reference_trainer():
    spec = importlib.util.spec_from_file_location("_ref_ode_training", os.path.join(REF, "stage2", "ode_training.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GANODETrainer


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def load(module, npz, prefix="w"):
    module.load_state_dict({k: torch.from_numpy(np.asarray(npz[f"{prefix}/{k}"])).clone() for k in module.state_dict()})
    return module


def step_delta(Trainer, module, role, loss, method, before_step=None):
    """One reference step on `module`'s parameters; returns {name: after - before}"""
    names = [n for n, _ in module.named_parameters()]
    params = list(module.parameters())
    before = [p.detach().clone() for p in params]
    kw = dict(g_params=[], dImg_params=[], dVid_params=None, g_loss=None, dImg_loss=None, dVid_loss=None)
    kw[{"gen": "g_params", "dis_img": "dImg_params"}[role]] = params
    kw[{"gen": "g_loss", "dis_img": "dImg_loss"}[role]] = loss
    t = Trainer(lr=K.LR, reg=0.0, method=method, **kw)
    if before_step:
        before_step()
    t.step(model=role)
    return {n: (p.detach() - b) for n, p, b in zip(names, params, before)}


def with_self_diff(out, prefix, d32, d64, untouched=()):
    for n in d32:
        if n in untouched:
            assert float(d32[n].abs().max()) == 0.0
            out[f"{prefix}/delta/{n}"] = np.zeros(0, np.float32)
            out[f"{prefix}/self/{n}"] = np.float64(0.0)
            continue
        out[f"{prefix}/delta/{n}"] = d32[n].numpy().astype(np.float32)
        out[f"{prefix}/self/{n}"] = np.float64(K.delta_err(d32[n].numpy(), d64[n].numpy()))


def main():
    Trainer = reference_trainer()
    out = {}

    # -- the quadratic problem ---------------------------------------------------------------------------------------------
    init = K.quad_init()
    for n, v in init.items():
        out[f"quad/init/{n}"] = v.numpy()
    for method in K.METHODS:
        ps = [init[n].clone().requires_grad_() for n in K.QUAD_NAMES]
        t = Trainer(ps, [], None, lambda: K.quad_loss(*ps), None, None, lr=K.QUAD_LR, reg=0.0, method=method)
        t.step(model="gen")
        for n, p in zip(K.QUAD_NAMES, ps):
            out[f"quad/{method}/{n}"] = p.detach().numpy().copy()

    # -- one discriminator step per method, reg = 0 ------------------------------------------------------------------------
    cfg = {"img": ("disc_img_mnist_tiny.npz", lambda: M.PatchImageDisc(1, ndf=8), 101),
           "vid": ("disc_vid_mnist_tiny.npz", lambda: M.VideoDisc(1, ksize=2, ndf=8), 102)}
    for tag, (fix, ctor, s) in cfg.items():
        z = np.load(os.path.join(GOLDEN, fix))
        real = torch.from_numpy(z["x"]).float()
        fake = K.fake_like(real, s)
        out[f"d{tag}/fake"] = fake.numpy().astype(np.float16)
        for method in K.METHODS:
            d32m = load(ctor(), z)
            d64m = copy.deepcopy(d32m).double()
            d32 = step_delta(Trainer, d32m, "dis_img", K.disc_loss(d32m, real, fake), method)
            d64 = step_delta(Trainer, d64m, "dis_img", K.disc_loss(d64m, real.double(), fake.double()), method)
            with_self_diff(out, f"d{tag}/{method}", d32, d64)

    # -- one RK4 generator step through the latent ODE ------------------------------------------------------------------------
    zg = np.load(os.path.join(GOLDEN, "gen_mnist_tiny.npz"))
    zv = np.load(os.path.join(GOLDEN, "disc_vid_mnist_tiny.npz"))
    zi = np.load(os.path.join(GOLDEN, "disc_img_mnist_tiny.npz"))
    mk_gen = lambda: load(M.Generator(1, 50, 0, 16, 16, ngf=8, mnist=True), zg)  # noqa: E731
    deltas = []
    for dbl in (False, True):
        gen, dv = mk_gen(), load(M.VideoDisc(1, ksize=2, ndf=8), zv)
        if dbl:
            gen, dv = gen.double(), dv.double()
        deltas.append(step_delta(Trainer, gen, "gen", K.gen_video_loss(gen, dv), "rk4", before_step=lambda: seed_all(K.GEN_SEED)))
    with_self_diff(out, "gen/rk4", deltas[0], deltas[1], untouched=[n for n in deltas[0] if n.startswith("recurrent.")])

    # -- the penalty: exact in fp64, and the error of the fp32 central difference on CPU ---------------------------------------
    gen, di = mk_gen().double(), load(M.PatchImageDisc(1, ndf=8), zi).double()
    names = [n for n, _ in di.named_parameters()]
    adjoint = ode_ref.odeint_adjoint
    ode_ref.odeint_adjoint = lambda f, y0, t, **kw: ode_ref.odeint(f, y0, t, **{k: v for k, v in kw.items() if k != "adjoint_params"})
    try:        # (the adjoint is a first-order autograd node; the plain solve has the same forward values)
        seed_all(K.PEN_SEED)
        exact = R.exact_penalty(K.gen_image_loss(gen, di), list(gen.parameters()), list(di.parameters()))
    finally:
        ode_ref.odeint_adjoint = adjoint
    gen, di = mk_gen(), load(M.PatchImageDisc(1, ndf=8), zi)
    seed_all(K.PEN_SEED)
    gp32, eps = R.central_penalty(K.gen_image_loss(gen, di), list(gen.parameters()), list(di.parameters()),
                                  float(np.finfo(np.float32).eps) ** (1.0 / 3.0))
    gen, di = mk_gen().double(), load(M.PatchImageDisc(1, ndf=8), zi).double()
    seed_all(K.PEN_SEED)
    gp64, _ = R.central_penalty(K.gen_image_loss(gen, di), list(gen.parameters()), list(di.parameters()),
                                float(np.finfo(np.float32).eps) ** (1.0 / 3.0))
    out["pen/eps32"] = np.float64(eps)
    for n, e, g, c in zip(names, exact, gp32, gp64):
        out[f"pen/exact/{n}"] = e.numpy().astype(np.float32)
        out[f"pen/err32/{n}"] = np.float64(K.delta_err(g.numpy(), e.numpy()))
        out[f"pen/central64/{n}"] = c.numpy()
        out[f"pen/self/{n}"] = np.float64(K.delta_err(g.numpy(), c.numpy()))

    path = os.path.join(GOLDEN, "odegan_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")
    for k in sorted(out):
        if k.startswith("pen/self/") or "/err32/" in k or k == "pen/eps32":
            print(f"  {k}: {float(out[k]):.3e}")


if __name__ == "__main__":
    main()
