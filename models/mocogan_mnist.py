"""Drop-in for the reference's models/mocogan_mnist.py: the generators whose ODEFunc is the one-layer tanh(W x + b).
`VideoGenerator(n_channels, 50, 0, 16, 16)` -- the call of ucf_moco_ode.py:80 -- constructs against this module."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.modules import ODEFuncTanh as ODEFunc  # noqa: E402,F401
from gan_ode_amd.modules import VideoGeneratorTanh as VideoGenerator  # noqa: E402,F401
from gan_ode_amd.modules import VideoGeneratorMNISTTanh as VideoGeneratorMNIST  # noqa: E402,F401
from gan_ode_amd.modules import VideoGeneratorMNISTODETanh as VideoGeneratorMNISTODE  # noqa: E402,F401
