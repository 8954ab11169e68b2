"""Drop-in `dataset` package for the reference drivers' `from dataset import MNISTRotationVideo, MNISTRotationImage`
(mnist_moco_ode.py:4) and `from dataset import UCF101Video, UCF101Image` (ucf_moco_ode.py:4).  The Rotated-MNIST classes and
the UCF-101 classes of dataset/ucf101new.py are provided, the latter with the bicubic resize of DESIGN section 21 and a
`to_device()` that builds the GPU-resident set (gan_ode_amd.data.Ucf101OnDevice).  Video DECODING stays out of scope (SURVEY
section 2, row 10): the UCF classes take a `reader` callable and default to torchvision.io.read_video when it is installed.
The legacy jpg-frame dataset (dataset/ucf101.py, dataset/transform/*) is not provided."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_ode_amd.data import MNISTRotationImage, MNISTRotationVideo, UCF101Image, UCF101Video  # noqa: E402,F401
from gan_ode_amd.data import RotMnistOnDevice  # noqa: E402,F401  (from_digits builds the clips on the GPU)
