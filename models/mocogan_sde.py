"""Drop-in for the reference's models/mocogan_sde.py (mnist_moco_sde.py:6)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.modules import SDEFunc, VideoGeneratorSDE  # noqa: E402,F401
