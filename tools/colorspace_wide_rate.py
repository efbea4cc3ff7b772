"""Kernel time of the colorspace filter's constant-luminance / ICtCp forms beside the nearest pre-existing ones: one
launch of 16 frames 1920 x 1080 4:2:0 10-bit through process_dev, the context's kernel timer, microseconds per launch.
Two rounds over the forms in one process (the first form a process times reads high in its first round).

    python tools/colorspace_wide_rate.py [launches per form, default 20]      -> one JSON line
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from handbrake_amd import hip, synth                       # noqa: E402

BT709 = (1, 1, 1, 1)
FORMS = [
    ("pq_nc_709_hable (parent form)", (9, 16, 9, 1), BT709, dict(peak=100.0)),
    ("709_nc (parent form)", BT709, (9, 14, 9, 1), {}),
    ("pq_ictcp_709_hable", (9, 16, 14, 1), BT709, dict(peak=100.0)),
    ("pq_cl_709_hable", (9, 16, 10, 1), BT709, dict(peak=100.0)),
    ("cl_nc", (9, 14, 10, 1), (9, 14, 9, 1), {}),
]
W, H, N = 1920, 1080, 16


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    frames = synth.stream("progressive", W, H, 2, depth=10)
    ctx = hip.Ctx(0)
    dev_in = [[torch.from_numpy(np.ascontiguousarray(p).view(np.int16)).cuda() for p in frames[i % 2]] for i in range(N)]
    outs = [[torch.zeros(p.shape, dtype=torch.int16, device="cuda") for p in frames[0]] for _ in range(N)]
    torch.cuda.synchronize()
    arr_in = (hip.DevFrame * N)(*[hip.dev_frame(f) for f in dev_in])
    arr_out = (hip.DevFrame * N)(*[hip.dev_frame(o) for o in outs])
    res = {}
    for _ in range(2):
        for name, src, dst, kw in FORMS:
            flt = hip.colorspace_device_filter(ctx, W, H, src, dst, depth=10, **kw)
            for _ in range(3):
                assert flt.process_dev(arr_in, 0, arr_out) == N
            ctx.sync(); ctx.profile(True); ctx.profile_reset()
            for _ in range(reps):
                flt.process_dev(arr_in, 0, arr_out)
            ctx.sync()
            n, ms = ctx.profile_stats()["colorspace"]
            ctx.profile(False)
            res.setdefault(name, []).append(round(ms / n * 1000, 1))
            flt.close()
    ctx.close()
    print(json.dumps({"us_per_launch_of_16": res}))


if __name__ == "__main__":
    main()
