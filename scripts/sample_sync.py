"""One sampling call on its own, and what a call costs the host:  python scripts/sample_sync.py [calls]
Prints one JSON line: the median / min / max ms of `calls` (200) gen.sample_videos(32) calls each followed by a synchronise,
and the host ms per call of a loop of the same calls that synchronises only at its end (time until the last call returns;
the loop is host-bound once this exceeds the GPU's step), then ms per step of 10 x `calls` calls back to back with the paths
they took (gen.lane_stats(), where the tree has it).  build_mnist(), no_grad, seeded as bench.py's timed loop."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_ode_amd as G  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
G.limit_host_threads()
torch.manual_seed(1234); np.random.seed(1234)
gen, _, _ = G.build_mnist()
gen.cuda()
with torch.no_grad():
    for _ in range(30):
        gen.sample_videos(32)
    torch.cuda.synchronize()
    G.freeze_host_gc()
    one = []
    for _ in range(n):
        t0 = time.perf_counter()
        gen.sample_videos(32)
        torch.cuda.synchronize()
        one.append((time.perf_counter() - t0) * 1e3)
    # host cost: every call returns as soon as its work is queued; the queue is kept short so that the host never waits
    host = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen.sample_videos(32)
        host.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    # the benchmark's loop: back to back, one synchronise at the end -- and which path its calls took
    before = gen.lane_stats() if hasattr(gen, "lane_stats") else None
    t0 = time.perf_counter()
    for _ in range(10 * n):
        gen.sample_videos(32)
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) / (10 * n) * 1e3
    stats = {k: v - before[k] for k, v in gen.lane_stats().items()} if before is not None else None
one.sort(); host.sort()
print(json.dumps({"calls": n, "loop": {"calls": 10 * n, "ms_per_step": round(loop_ms, 4), "lane_stats": stats},
                  "sync_call_ms": {"median": round(one[n // 2], 4), "min": round(one[0], 4), "max": round(one[-1], 4),
                                   "p10": round(one[n // 10], 4), "p90": round(one[9 * n // 10], 4)},
                  "host_ms_per_call": {"median": round(host[n // 2], 4), "p90": round(host[9 * n // 10], 4)}}))
