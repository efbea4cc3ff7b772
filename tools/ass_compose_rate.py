#!/usr/bin/env python3
"""What a changed text subtitle costs on the GPU: hbhip_blend_set_ass_images (pack + one upload + the compose kernel,
csrc/ass_compose.hip) against hbhip_blend_set_overlays fed the finished overlays - the device-side part of the path that
composes on the CPU (rendersub.c:474-612) first, i.e. that path WITHOUT its CPU compose: a floor for it.  Two lists on a
1920 x 1080 4:2:0 frame: a line of text (40 overlapping glyph images in a box of about 1280 x 160) and the same line
over a full-screen image.  Wall times are host clocks around the call plus a synchronise of the context's stream, the two
calls alternated; the kernel's time is the context's own event bracket (hbhip_ctx_profile_*), taken in a pass of its own.
The overlays are checked against the numpy model at the sizes timed.  Prints one JSON object.
usage: ass_compose_rate.py [repeats]"""
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
import ass_compose_model as am  # noqa: E402

W, H = 1920, 1080


def glyphs(rng, n=20, x0=320, y0=880):
    """a line of n glyphs, each an outline image under a fill image, neighbours overlapping by 6 pixels"""
    out = []
    for i in range(n):
        for w, h, dx, dy, a in ((70, 160, 0, 0, 0), (60, 150, 5, 5, 32)):
            bitmap = rng.integers(1, 256, (h, w), dtype=np.uint8)
            bitmap[rng.random((h, w)) < 0.5] = 0
            out.append((bitmap, w, x0 + 64 * i + dx, y0 + dy, tuple(int(v) for v in rng.integers(16, 240, 3)) + (a,)))
    return out


def measure(ctx, name, images, repeats):
    b = hip.BlendDevice(ctx, W, H, overlay_log2_cw=1, overlay_log2_ch=1)
    want, masks = am.render(images, 1, 1, 1)
    try:
        b.set_ass_images(images)
        got = b.overlays()
        assert len(got) == len(want)
        for (gx, gy, gp), (wx, wy, wp), mask in zip(got, want, masks):
            assert (gx, gy) == (wx, wy) and np.array_equal(gp[0], wp[0]) and np.array_equal(gp[3], wp[3])
            assert np.array_equal(gp[1][mask], wp[1][mask]) and np.array_equal(gp[2][mask], wp[2][mask])
        for _ in range(5):                                                  # both paths warm: buffers sized, code loaded
            b.set_ass_images(images)
            b.set_overlays(want)
        ctx.sync()
        t = {"set_ass_images": [], "set_overlays": []}
        for _ in range(repeats):
            for key, call in (("set_ass_images", lambda: b.set_ass_images(images)), ("set_overlays", lambda: b.set_overlays(want))):
                t0 = time.perf_counter()
                call()
                ctx.sync()
                t[key].append((time.perf_counter() - t0) * 1e6)
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(repeats):
            b.set_ass_images(images)
        ctx.sync()
        launches, ms = ctx.profile_stats()["ass_compose"]
        ctx.profile(False)
    finally:
        b.close()
    boxes = [(x, y) + p[0].shape[::-1] for x, y, p in want]
    return {"list": name, "images": len(images), "glyph_bytes": int(sum(bm.shape[0] * w for bm, w, *_ in images)),
            "boxes": boxes, "overlay_bytes": int(sum(sum(p.size for p in planes) for _, _, planes in want)),
            "compose_kernel_us": round(ms * 1e3 / launches, 2),
            "set_ass_images_wall_us": {"median": round(statistics.median(t["set_ass_images"]), 1), "min": round(min(t["set_ass_images"]), 1)},
            "set_overlays_wall_us": {"median": round(statistics.median(t["set_overlays"]), 1), "min": round(min(t["set_overlays"]), 1)},
            "repeats": repeats}


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rng = np.random.default_rng(11)
    line = glyphs(rng)
    full = rng.integers(1, 256, (H, W), dtype=np.uint8)
    full[rng.random((H, W)) < 0.5] = 0
    screen = [(full, W, 0, 0, (90, 120, 140, 128))] + line
    ctx = hip.Ctx(0)
    try:
        res = {"device": ctx.name(), "frame": [W, H], "format": "4:2:0, left-sited",
               "lists": [measure(ctx, "line of text", line, repeats), measure(ctx, "full screen", screen, repeats)]}
    finally:
        ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
