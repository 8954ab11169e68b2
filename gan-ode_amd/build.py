"""Builds libgode.so (all HIP kernels + the C ABI of include/gode.h) for gfx950 with hipcc, in-tree."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libgode.so")
SOURCES = ["igemm.hip", "conv_patch.hip", "wgrad.hip", "ode.hip", "ode_valu.hip", "odernn.hip", "odernn_valu.hip", "adj_adaptive.hip", "sde_valu.hip", "cde_valu.hip", "gru_valu.hip", "latent_reduce.hip", "elementwise.hip", "dnoise.hip", "categ.hip", "odestep.hip", "gres.hip", "fc.hip", "clips.hip", "rotclips.hip", "vidgrid.hip", "latent_draw.hip", "diffaug.hip", "api.hip"]
HEADERS = ["common.h", "philox.h", "conv_geom.h", "igemm_plan.h", "wgrad_plan.h", "col2im_plan.h", "ode_common.h", "valu_common.h", "dopri5.h", "gif_lzw.h", os.path.join("..", "..", "include", "gode.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Compile every translation unit and link the shared library.  hipcc cross-compiles gfx950 without a GPU."""
    os.makedirs(LIBDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    procs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(LIBDIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = ["hipcc"] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + out.decode(errors="replace"))
    if force or procs or _stale(LIB, objs):
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n" + r.stdout.decode(errors="replace"))
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
