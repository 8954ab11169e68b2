"""gan_ode_amd -- MI355X-native implementation of chechaohp/gan-ode's MoCoGAN + Neural-ODE hot path.

The arithmetic lives in libgode.so (hand-written HIP for gfx950, C ABI in include/gode.h); this package is the
Python host side that mirrors the reference's class surface.  Importing the package does not need a GPU; running
anything does, and there is no fallback path.
"""
from . import _lib
from .modules import (CategoricalVideoDiscriminator, CDEFunc, DiffAugment, Noise, ODEFunc, ODEFuncTanh, PatchImageDiscriminator, SDEFunc, VideoDiscriminator, VideoGenerator,
                      VideoGeneratorCDE, VideoGeneratorGRU, VideoGeneratorMNIST, VideoGeneratorMNISTODE, VideoGeneratorMNISTODERNN,
                      VideoGeneratorMNISTODETanh, VideoGeneratorMNISTTanh, VideoGeneratorSDE, VideoGeneratorTanh, diffaug_params)
from .ode_training import GANODETrainer
from .gres import ConditionalNorm, GResBlock, SpectralNorm
from . import data, dcgan, fcgan, video_io
from .train import (FusedAdam, GanTrainer, WassersteinDiscriminatorLoss, WassersteinGeneratorLoss, bce_with_logits_const,
                    bce_with_logits_halves, bce_with_logits_pair, bce_ce_head, bce_ce_head_halves, bce_ce_head_pair,
                    bce_ce_heads, categorical_cross_entropy, build_mnist, build_ucf, freeze_host_gc, host_cpu_quota,
                    limit_host_threads, train_step, unit_grad, wasserstein_discriminator_loss,
                    wasserstein_discriminator_loss_halves, wasserstein_generator_loss, wasserstein_generator_loss_pair)

__all__ = ["Noise", "DiffAugment", "diffaug_params", "ODEFunc", "ODEFuncTanh", "VideoGeneratorTanh", "VideoGeneratorMNISTTanh", "VideoGeneratorMNISTODETanh", "PatchImageDiscriminator", "VideoDiscriminator", "CategoricalVideoDiscriminator", "VideoGenerator",
           "VideoGeneratorMNIST", "VideoGeneratorMNISTODE", "VideoGeneratorMNISTODERNN", "SDEFunc", "VideoGeneratorSDE", "CDEFunc", "VideoGeneratorCDE", "VideoGeneratorGRU", "FusedAdam", "GanTrainer", "GANODETrainer", "SpectralNorm", "ConditionalNorm", "GResBlock", "bce_with_logits_const",
           "bce_with_logits_pair", "bce_with_logits_halves", "categorical_cross_entropy", "bce_ce_head", "bce_ce_head_pair",
           "bce_ce_head_halves", "bce_ce_heads", "WassersteinGeneratorLoss", "WassersteinDiscriminatorLoss",
           "wasserstein_generator_loss", "wasserstein_generator_loss_pair", "wasserstein_discriminator_loss",
           "wasserstein_discriminator_loss_halves", "unit_grad", "fcgan", "dcgan", "video_io", "build_mnist", "build_ucf", "train_step", "host_cpu_quota", "limit_host_threads", "freeze_host_gc", "_lib"]

# Process-global host tuning is opt-in (nothing happens at import): call limit_host_threads() once at start-up when
# torch's intra-op pool is larger than the container's CPU quota (see its docstring; bench.py and tests/conftest.py
# do), and freeze_host_gc() after warm-up in long loops (GanTrainer(freeze_gc=True) does it after its 2nd iteration).
