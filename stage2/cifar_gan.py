"""Drop-in for the class cell of the reference's stage2/test_ODE_training_with_cifar_GAN.ipynb: the convolutional
Generator and Discriminator (nz, ngf, ndf and nc as keyword arguments with the notebook's values), and nn.BCEWithLogitsLoss,
on the HIP kernels."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.dcgan import BCEWithLogitsLoss, Discriminator, Generator  # noqa: E402,F401
