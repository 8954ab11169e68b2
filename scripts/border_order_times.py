"""Per-layer timings of the decoder's three k4 s2 p1 ConvTranspose GEMMs for gode_igemm_op.border = 0 / 1 / 2 (tile 0: the
plan's own choice), HIP events around 30 launches, five repeats -- as profiles/border_split_layers.md was taken.  The grid
order of border = 2 is fixed per process (GODE_IGEMM_BORDER_ORDER=0 keeps sub-phase after sub-phase), so the two orders are
two runs of this script; each prints and writes one JSON line per (rows, layer, border).

    python scripts/border_order_times.py --rows 512 256 --out profiles/border_order_layers.jsonl --tag interleaved
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan_ode_amd._lib as L  # noqa: E402
from gan_ode_amd.engine import make_geom  # noqa: E402

LAYERS = (("512->256 4x4", 512, 256, 4), ("256->128 8x8", 256, 128, 8), ("128->64 16x16", 128, 64, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=300, help="untimed launches first (the clock settles over ~50 ms of load)")
    ap.add_argument("--borders", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    out_f = open(a.out, "a") if a.out else None
    for rows in a.rows:
        for name, cin, cout, h in LAYERS:
            g = make_geom(rows, cout, cin, (1, 2 * h, 2 * h), (1, h, h), (1, 4, 4), (1, 2, 2), (0, 1, 1))
            gen = torch.Generator().manual_seed(h)
            x = torch.randn(rows, 1, h, h, cin, generator=gen).cuda()
            w = (torch.randn(cin, cout, 4, 4, generator=gen) * 0.05).cuda()
            d = L.DGRAD | L.PACK_BORDER        # (the border-form pack extends the plain one: every form reads it)
            wp = torch.empty(lib.gode_pack_size(C.byref(g), d), device="cuda")
            L.check(lib.gode_pack_weights(C.byref(g), d, w.data_ptr(), wp.data_ptr(), None, 0, st))
            first = None
            for border in a.borders:
                y = torch.full((rows, 1, 2 * h, 2 * h, cout), float("nan"), device="cuda")
                op = L.IgemmOp(g=g, dir=L.DGRAD, act=L.ACT_NONE, epilogue=L.EPI_RAW, tile=0, src=x.data_ptr(), wpack=wp.data_ptr(),
                               out=y.data_ptr(), border=border)
                nrow = lib.gode_igemm_stats_rows(C.byref(op))
                stats = torch.empty(2 * cout * nrow, device="cuda")
                op.stats = stats.data_ptr()
                for _ in range(a.warmup):
                    L.run_one(op, st)
                torch.cuda.synchronize()
                us = []
                for _ in range(a.repeats):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches):
                        L.run_one(op, st)
                    e1.record()
                    torch.cuda.synchronize()
                    us.append(round(1e3 * e0.elapsed_time(e1) / a.launches, 1))
                first = y if first is None else first
                rec = dict(tag=a.tag, order_env=os.environ.get("GODE_IGEMM_BORDER_ORDER"), rows=rows, layer=name, border=border,
                           stats_rows=nrow, dead_taps=round(lib.gode_igemm_dead_taps(C.byref(op)), 4),
                           model_cycles=lib.gode_igemm_model_cycles(C.byref(op)), us=us, median=sorted(us)[len(us) // 2],
                           equal=bool(torch.equal(first, y)))
                print(json.dumps(rec), flush=True)
                if out_f:
                    out_f.write(json.dumps(rec) + "\n")
                    out_f.flush()


if __name__ == "__main__":
    main()
