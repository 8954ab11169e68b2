"""Writes tests/golden/gen_cde_init.npz: the initial state_dict of the reference's VideoGeneratorCDE
(models/mocogan_cde.py) built on the CPU under a fixed seed, which pins the drop-in class's construction order (and
so its seeded weights and state_dict key order).  Data only: no reference source enters the repository.

  python scripts/make_cde_golden.py /path/to/reference

The reference's models/mocogan_cde.py imports `on_dev.mocogan_ode` (a package it does not ship) and torchcde; neither
is needed to construct the module, so `on_dev.mocogan_ode` is aliased to its models/mocogan_ode.py and torchcde /
torchdiffeq are stubbed.  The files are loaded by path: this repository's drop-in `models` package would otherwise
shadow the reference's.  Width ngf = 8 (as the other generator fixtures) keeps the file small; the construction order
does not depend on it.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "gen_cde_init.npz")
SEED, NGF = 1234, 8


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _never(*a, **k):
    raise RuntimeError("stub: the fixture only constructs the module")


def main(ref):
    models = os.path.join(ref, "models")
    _stub("torchcde", cdeint=_never, CubicSpline=_never, hermite_cubic_coefficients_with_backward_differences=_never)
    _stub("torchdiffeq", odeint=_never, odeint_adjoint=_never)
    pkg = _stub("models")
    pkg.__path__ = [models]
    pkg.mocogan = _load("models.mocogan", os.path.join(models, "mocogan.py"))
    ode = _load("on_dev.mocogan_ode", os.path.join(models, "mocogan_ode.py"))
    on_dev = _stub("on_dev")
    on_dev.__path__ = []
    on_dev.mocogan_ode = ode
    cde = _load("models.mocogan_cde", os.path.join(models, "mocogan_cde.py"))
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    gen = cde.VideoGeneratorCDE(1, 50, 0, 16, 16, ngf=NGF)
    arrays = {f"w/{k}": v.detach().cpu().numpy().copy() for k, v in gen.state_dict().items()}
    arrays["seed"], arrays["ngf"] = np.int64(SEED), np.int64(NGF)
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB, {len(arrays) - 2} tensors")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(REPO), "reference"))
