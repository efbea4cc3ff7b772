#!/usr/bin/env python3
"""`format=bgra` behind a device run, hb_get_preview's list: what the pack kernel and a whole preview cost.

  kernel                  16 resident 3840 x 2160 frames and 16 of 1920 x 1080 through hbhip_frame_download_rgb32 (bgra, BT.709
                          limited), two rounds behind one warm-up launch a size.  Under
                          `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/preview_rates.py kernel`
  kernel-summarize TRACE.csv
                          rgb32_pack_kernel's [mean, min, median] µs per launch at each size, and the bytes a launch moves
                          over the mean (GB/s)
  wall                    the wall time of hbrt.preview_run of [decomb mode=7, crop/scale to the frame's size] + the display
                          rescale + format=bgra at 1080p and 2160p: the first call of the process at each size, then five more
JSON on stdout."""
import csv
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
FRAMES, ROUNDS = 16, 2


def kernel():
    from handbrake_amd import hip
    ctx = hip.Ctx(0)
    rng = np.random.default_rng(1)
    for w, h in SIZES:
        frames = [hip.Frame(ctx, w, h, 8) for _ in range(FRAMES)]
        for fr in frames:
            fr.upload([rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))])
        frames[0].download_rgb32()                                          # the code object, the staging buffer
        for _ in range(ROUNDS):
            for fr in frames:
                fr.download_rgb32()
        for fr in frames:
            fr.close()
    ctx.close()


def kernel_summarize(trace):
    t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
         for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
         if re.search(r"rgb32_pack_kernel", r["Kernel_Name"])]
    n = 1 + FRAMES * ROUNDS
    assert len(t) == n * len(SIZES), len(t)
    out = {}
    for k, (w, h) in enumerate(SIZES):
        timed = t[k * n + 1:(k + 1) * n]
        moved = w * h * 3 // 2 + 4 * w * h
        out["%dx%d" % (w, h)] = {"mean_us": round(float(np.mean(timed)), 2), "min_us": round(min(timed), 2),
                                 "median_us": round(float(np.median(timed)), 2), "bytes_moved": moved,
                                 "GBps_at_mean": round(moved / float(np.mean(timed)) / 1e3, 1)}
    print(json.dumps(out, indent=1))


def wall():
    from handbrake_amd import hbrt, hip, synth
    hip.filters()
    F = hbrt.FILTER_ID
    keep = {}
    for name in ("decomb", "crop_scale", "format"):                       # CPU stand-ins: the swap puts the drop-ins in
        addr, keep[name] = hbrt.filter_stub(F[name], name)
        hbrt.runtime().hbhip_rt_register_filter(F[name], addr)
    out = {"list": "[decomb mode=7, crop_scale to the frame's size] + display rescale (PAR 1:1) + format=bgra"}
    for w, h in reversed(SIZES):
        fr = synth.stream("interlaced", w, h, 1)[0]
        filters = [(F["decomb"], "mode=7"), (F["crop_scale"], "width=%d:height=%d" % (w, h))]
        ms = []
        for _ in range(6):
            t0 = time.perf_counter()
            entries, got = hbrt.preview_run(filters, fr)
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            assert got.shape == (h, w, 4) and all("HIP" in n for n, _ in entries)
        out["%dx%d" % (w, h)] = {"first_ms": ms[0], "second_ms": ms[1], "later_ms": ms[2:]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernel":
        kernel()
    elif mode == "kernel-summarize":
        kernel_summarize(sys.argv[2])
    elif mode == "wall":
        wall()
    else:
        sys.exit(__doc__)
