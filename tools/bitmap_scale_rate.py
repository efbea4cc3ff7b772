#!/usr/bin/env python3
"""What a bitmap subtitle costs on the GPU: hbhip_blend_set_bitmaps (csrc/blend.hip, csrc/bitmap_scale.hip) on a 3840 x 2160
frame with a 1920 x 160 bitmap authored on a 1920 x 1080 canvas (factor 2), when the call misses the object's cache - a new
key every call: tables, pack, one upload, the scale kernel, the previous key's allocation freed - and when it hits, which is
what every further frame under the subtitle pays.  Wall times are host clocks around the call plus a synchronise of the
context's stream; the kernel's time is the context's own event bracket (hbhip_ctx_profile_*), taken in a pass of its own.
The overlay is checked against the model at the size timed.  Prints one JSON object.
usage: bitmap_scale_rate.py [repeats]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from handbrake_amd import hip  # noqa: E402
import bitmap_scale_model as bm  # noqa: E402

W, H = 3840, 2160
CANVAS = (1920, 1080)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    sub = bm.random_sub(1920, 160, 0, 880, CANVAS)
    want = bm.render(W, H, sub)
    ctx = hip.Ctx(0)
    try:
        b = hip.BlendDevice(ctx, W, H)
        try:
            b.set_bitmaps([sub + (1,)])
            (gx, gy, gp), = b.overlays(0, 0)
            assert (gx, gy) == want[:2] and all(np.array_equal(g, w) for g, w in zip(gp, want[2]))
            for k in range(5):                                              # warm: buffers sized, code loaded
                b.set_bitmaps([sub + (100 + k,)])
            ctx.sync()
            t = {"miss": [], "hit": []}
            for k in range(repeats):
                for what, key in (("miss", 1000 + k), ("hit", 1000 + k)):
                    t0 = time.perf_counter()
                    b.set_bitmaps([sub + (key,)])
                    ctx.sync()
                    t[what].append((time.perf_counter() - t0) * 1e6)
            assert b.bitmap_stats() == (6 + repeats, 6 + repeats, repeats)
            ctx.profile(True)
            ctx.profile_reset()
            for k in range(repeats):
                b.set_bitmaps([sub + (5000 + k,)])
            ctx.sync()
            launches, ms = ctx.profile_stats()["bitmap_scale"]
            ctx.profile(False)
        finally:
            b.close()
        res = {"device": ctx.name(), "frame": [W, H], "bitmap": [1920, 160], "canvas": list(CANVAS),
               "overlay": list(want[2][0].shape[::-1]), "source_bytes": 4 * 1920 * 160,
               "overlay_bytes": int(sum(p.size for p in want[2])), "scale_kernel_us": round(ms * 1e3 / launches, 2),
               "set_bitmaps_miss_wall_us": {"median": round(statistics.median(t["miss"]), 1), "min": round(min(t["miss"]), 1)},
               "set_bitmaps_hit_wall_us": {"median": round(statistics.median(t["hit"]), 1), "min": round(min(t["hit"]), 1)},
               "repeats": repeats}
    finally:
        ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
