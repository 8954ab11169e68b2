"""Drop-in for the reference's stage1/GResBlock.py (l2normalize, SpectralNorm, ConditionalNorm, GResBlock)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.gres import ConditionalNorm, GResBlock, SpectralNorm, l2normalize  # noqa: E402,F401
