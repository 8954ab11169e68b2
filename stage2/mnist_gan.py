"""Drop-in for the class cell of the reference's stage2/test_ODE_training_with_MNIST_GAN.ipynb: the fully-connected
Generator and Discriminator, and nn.BCELoss, on the HIP kernels."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.fcgan import BCELoss, Discriminator, Generator  # noqa: E402,F401
