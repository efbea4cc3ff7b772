"""What the title scan on a device picture costs, and what it saves: the device time of the five launches
of hbhip_scan_push for one 1080p preview, from the context's kernel timer, beside the D2H copy of the same yuv420p picture
into pinned host memory - its bytes from hbhip_ctx_bus_bytes, its time from two events around the copy on the context's
stream and from a host clock around the synchronous hbhip_frame_download.

    python tools/scan_measure.py [pictures]        one JSON line"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from handbrake_amd import hip, synth  # noqa: E402

W, H = 1920, 1080


def preview():
    """combed content behind a matte and pillars: every walk has rows and columns to pass"""
    y, cb, cr = [np.ascontiguousarray(p) for p in synth.interlaced_frame(W, H, 1)]
    y[:H // 8] = 16
    y[H - H // 6:] = 17
    y[:, :W // 10] = 16
    y[:, W - W // 7:] = 18
    return [y, cb, cr]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    L = hip.lib()
    ctx = hip.Ctx(0)
    fr = hip.Frame(ctx, W, H)
    fr.upload(preview())
    scan = hip.ScanDevice(ctx, W, H)
    for _ in range(8):                                    # warm-up: code objects, the slots' allocations
        scan.push(fr)
    first = [scan.pull().as_tuple() for _ in range(8)]
    assert all(r == first[0] for r in first)

    # the five launches, one picture at a time
    ctx.sync(); ctx.profile(True); ctx.profile_reset()
    for _ in range(n):
        scan.push(fr)
        assert scan.pull().as_tuple() == first[0]
    ctx.sync()
    stats = ctx.profile_stats(); ctx.profile(False)
    kernels = {k: round(ms / cnt * 1e3, 2) for k, (cnt, ms) in stats.items() if k.startswith("scan_")}
    assert all(stats[k][0] == n for k in kernels) and len(kernels) == 5, stats

    # the same with eight pictures in flight, timer off: stream time per picture, launch gaps and the record's copy included
    ctx.sync(); ctx.mark(0)
    for _ in range(n // 8):
        for _ in range(8):
            scan.push(fr)
        for _ in range(8):
            scan.pull()
    ctx.mark(1)
    stream_us = ctx.elapsed_ms(0, 1) * 1e3 / (n // 8 * 8)

    # what it replaces: the picture's D2H into pinned memory
    d = hip.DevFrame()
    L.hbhip_frame_describe.argtypes = [C.c_void_p, C.POINTER(hip.DevFrame), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    hip.check(L.hbhip_frame_describe(fr.h, C.byref(d), None, None), ctx.h, "describe")
    rows = (H, H // 2, H // 2)
    nbytes = sum(d.stride[c] * rows[c] for c in range(3))
    L.hbhip_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.hbhip_host_free.argtypes = [C.c_void_p]
    L.hbhip_host_free.restype = None
    pinned = C.c_void_p()
    hip.check(L.hbhip_host_alloc(nbytes, C.byref(pinned)), ctx.h, "host_alloc")
    host = hip.HostFrame()
    off = 0
    for c in range(3):                                    # the frame's own layout: the download is one block
        host.plane[c] = pinned.value + off
        host.stride[c] = d.stride[c]
        off += d.stride[c] * rows[c]
    for _ in range(5):
        hip.check(L.hbhip_frame_download(fr.h, C.byref(host)), ctx.h, "download")
    b0 = ctx.bus_bytes()
    walls = []
    for _ in range(50):
        t = time.perf_counter()
        hip.check(L.hbhip_frame_download(fr.h, C.byref(host)), ctx.h, "download")
        walls.append((time.perf_counter() - t) * 1e6)
    b1 = ctx.bus_bytes()
    events = []
    for _ in range(50):
        ctx.mark(2)
        hip.check(L.hbhip_dev_download(ctx.h, pinned, d.plane[0], nbytes), ctx.h, "dev_download")
        ctx.mark(3)
        events.append(ctx.elapsed_ms(2, 3) * 1e3)
    L.hbhip_host_free(pinned)
    print(json.dumps({
        "device": ctx.name(), "picture": f"{W}x{H} yuv420p", "pictures": n,
        "scan_kernel_us": kernels, "scan_kernels_sum_us": round(sum(kernels.values()), 2),
        "scan_stream_us_per_picture_8_in_flight": round(stream_us, 2),
        "scan_bus_bytes_per_picture": hip.SCAN_RECORD_BYTES,
        "d2h_bytes": (b1[1] - b0[1]) // 50, "d2h_event_us_median": round(float(np.median(events)), 2),
        "d2h_event_us_min": round(min(events), 2), "d2h_wall_us_median": round(float(np.median(walls)), 2),
        "d2h_wall_us_min": round(min(walls), 2),
    }))
    scan.close(); fr.close(); ctx.close()


if __name__ == "__main__":
    main()
