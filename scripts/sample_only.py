"""The headline workload alone, for a kernel trace: build_mnist(), 220 calls of gen.sample_videos(32) under no_grad, seeded as
bench.py seeds its timed loop.   rocprofv3 --kernel-trace --output-format csv -- python scripts/sample_only.py [pair|always]
(the argument sets gen.sample_lanes: under the profiler the host is barely ahead of the GPU and the default gate shows nothing)
(profiles/sampling_small_kernels.md averages the trace per kernel and grid size after dropping each kernel's first 10 %.)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_ode_amd as G  # noqa: E402

torch.manual_seed(1234); np.random.seed(1234)
gen, _, _ = G.build_mnist()
gen.cuda()
if len(sys.argv) > 1:
    gen.sample_lanes = sys.argv[1]
with torch.no_grad():
    for _ in range(220):
        gen.sample_videos(32)
torch.cuda.synchronize()
