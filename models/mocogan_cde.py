"""Drop-in for the reference's models/mocogan_cde.py (mnist_moco_cde.py:6)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.modules import CDEFunc, VideoGeneratorCDE  # noqa: E402,F401
