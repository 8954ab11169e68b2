"""Drop-in for the reference's stage2/ode_training.py (GANODETrainer)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.ode_training import GANODETrainer  # noqa: E402,F401
