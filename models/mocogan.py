"""Drop-in for the reference's models/mocogan.py: the discriminators the stage-3 ODE drivers import
(mnist_moco_ode.py:5), the categorical video discriminator (models/mocogan.py:167-182) and the original GRU generator (models/mocogan.py:185-301, as VideoGenerator), backed by
libgode.so."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.modules import CategoricalVideoDiscriminator, Noise, PatchImageDiscriminator, VideoDiscriminator  # noqa: E402,F401
from gan_ode_amd.modules import VideoGeneratorGRU as VideoGenerator  # noqa: E402,F401
