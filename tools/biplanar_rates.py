#!/usr/bin/env python3
"""NV12 / P010LE at the ends of a run: what the repack kernels and the adapters cost.

  repack [out.json]       64 frames of 1920 x 1080 and of 3840 x 2160, at 8 and 10 bits, through hbhip_frame_upload_biplanar /
                          hbhip_frame_download_biplanar (the staging pair) and through hbhip_frame_import_surface /
                          hbhip_frame_export_surface on a surface with a 256-byte pitch and 16 padded rows (the surface pair:
                          the same bytes, no host copy); writes the box's copy ceiling (hbhip_ctx_copy_bandwidth) and the
                          bytes a kernel must move per frame.  Meant to run under
                          `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/biplanar_rates.py repack DIR/repack.json`
  summarize TRACE.csv REPACK.json
                          the kernel trace of that run, per kernel and frame size: mean time, achieved GB/s and the fraction
                          of the copy ceiling - what tools/kernel_rooflines.py reports for the other secondary kernels
  company                 the surface pair in two kinds of company, 64 rounds each, at the two points with 3 840-byte rows (2160p
                          8 bits, 1080p 10 bits): A, export and import back to back; B, between the bus copies the staging
                          pair runs between (upload_biplanar, export, import, download_biplanar).  Under rocprofv3 as above
  company-summarize TRACE.csv
                          per kernel [mean, min, median] µs: the surface kernels' first 64 launches (A) and next 64 (B), the
                          staging kernels of loop B
  widen                   P010LE out of 16 resident 1080p frames a form, the forms alternated, two rounds: the 10-bit merges
                          (bi_merge_kernel, bi_surface_merge_kernel on ten-bit frames) and the widening merge of 8-bit frames
                          into the staging buffer and into a surface.  Under rocprofv3 as above
  widen-summarize TRACE.csv
                          per form [mean, min, median] µs and the widening forms over their siblings
  adapters [frames]       [upload, lapsharp, download] at 1080p through the plugin surface (a thread per filter, pinned
                          hb_buffer_t in and out, as handbrake_amd/hostpath.py runs its lists): NV12 in and out against
                          planar 8 bits, three runs each, alternated
JSON on stdout."""
import csv
import ctypes as C
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SIZES = [(1920, 1080), (3840, 2160)]
NV12, P010LE = 23, 158
LAP = "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap"


def align64(n):
    return -(-n // 64) * 64


def repack(out_path):
    from handbrake_amd import hip
    L = hip.lib()
    ctx = hip.Ctx(0)
    bw = C.c_double()
    L.hbhip_ctx_copy_bandwidth.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    hip.check(L.hbhip_ctx_copy_bandwidth(ctx.h, 1 << 30, 5, C.byref(bw)), ctx.h, "copy_bandwidth")
    res = {"copy_ceiling_GBps": round(bw.value, 1), "frames": 64, "cases": []}
    rng = np.random.default_rng(1)
    for w, h in SIZES:
        for depth, bps in ((8, 1), (10, 2)):
            pitch = align64(w * bps)                                   # luma and interleaved chroma rows alike (w even)
            host = rng.integers(0, 256, pitch * (h + h // 2), dtype=np.uint8)       # the staging layout: one 1-D copy
            hb = hip.HostBiplanar()
            hb.plane[0], hb.plane[1] = host.ctypes.data, host.ctypes.data + pitch * h
            hb.stride[0] = hb.stride[1] = pitch
            fr = C.c_void_p()
            hip.check(L.hbhip_frame_alloc(ctx.h, w, h, depth, 1, 1, C.byref(fr)), ctx.h, "frame_alloc")
            for _ in range(res["frames"]):
                hip.check(L.hbhip_frame_upload_biplanar(fr, C.byref(hb)), ctx.h, "upload_biplanar")
                hip.check(L.hbhip_frame_download_biplanar(fr, C.byref(hb)), ctx.h, "download_biplanar")
            surface = hip.Surface(ctx, w, h, depth)
            for _ in range(res["frames"]):
                hip.check(L.hbhip_frame_export_surface(fr, surface.h), ctx.h, "export_surface")
                hip.check(L.hbhip_frame_import_surface(fr, surface.h), ctx.h, "import_surface")
            surface.close()
            L.hbhip_frame_release(fr)
            # a kernel reads one layout and writes the other: the samples of the frame twice
            res["cases"].append({"width": w, "height": h, "depth": depth, "bytes_per_frame": 2 * (w * h * 3 // 2) * bps})
    ctx.close()
    txt = json.dumps(res, indent=1)
    if out_path:
        open(out_path, "w").write(txt)
    print(txt)


def summarize(trace, repack_json):
    info = json.load(open(repack_json))
    ceiling = info["copy_ceiling_GBps"]
    groups = {}
    for r in csv.DictReader(open(trace)):
        m = re.search(r"(bi_split_kernel|bi_merge_kernel|bi_surface_split_kernel|bi_surface_merge_kernel)<([^>]*)>", r["Kernel_Name"])
        if not m:
            continue
        depth = 8 if "char" in m.group(2) else 10
        # what tells the two frame sizes apart: the staging kernels' grids are one-dimensional, the surface kernels' rows are on y
        size = int(r["Grid_Size_Y"] if "surface" in m.group(1) else r["Grid_Size_X"])
        groups.setdefault((m.group(1), depth, size), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = {"copy_ceiling_GBps": ceiling, "kernels": []}
    for kernel in ("bi_split_kernel", "bi_merge_kernel", "bi_surface_split_kernel", "bi_surface_merge_kernel"):
        for depth in (8, 10):
            grids = sorted(g for k, d, g in groups if k == kernel and d == depth)        # the smaller grid is the smaller frame
            for (w, h), grid in zip(SIZES, grids):
                ns = groups[(kernel, depth, grid)]
                case = next(c for c in info["cases"] if (c["width"], c["height"], c["depth"]) == (w, h, depth))
                us = sum(ns) / len(ns) / 1e3
                gbps = case["bytes_per_frame"] / (us * 1e-6) / 1e9
                out["kernels"].append({"kernel": kernel, "depth": depth, "frame": f"{w}x{h}", "launches": len(ns),
                                       "avg_us": round(us, 2), "min_us": round(min(ns) / 1e3, 2),
                                       "bytes_per_launch": case["bytes_per_frame"], "achieved_GBps": round(gbps, 1),
                                       "frac_of_copy_ceiling": round(gbps / ceiling, 4)})
    print(json.dumps(out, indent=1))


def company():
    from handbrake_amd import hip
    L = hip.lib()
    ctx = hip.Ctx(0)
    rng = np.random.default_rng(1)
    for w, h, depth, bps in ((3840, 2160, 8, 1), (1920, 1080, 10, 2)):
        pitch = align64(w * bps)
        host = rng.integers(0, 256, pitch * (h + h // 2), dtype=np.uint8)
        hb = hip.HostBiplanar()
        hb.plane[0], hb.plane[1] = host.ctypes.data, host.ctypes.data + pitch * h
        hb.stride[0] = hb.stride[1] = pitch
        fr = C.c_void_p()
        hip.check(L.hbhip_frame_alloc(ctx.h, w, h, depth, 1, 1, C.byref(fr)), ctx.h, "frame_alloc")
        surface = hip.Surface(ctx, w, h, depth)
        hip.check(L.hbhip_frame_upload_biplanar(fr, C.byref(hb)), ctx.h, "upload_biplanar")
        for _ in range(64):                                                   # A
            hip.check(L.hbhip_frame_export_surface(fr, surface.h), ctx.h, "export_surface")
            hip.check(L.hbhip_frame_import_surface(fr, surface.h), ctx.h, "import_surface")
        for _ in range(64):                                                   # B
            hip.check(L.hbhip_frame_upload_biplanar(fr, C.byref(hb)), ctx.h, "upload_biplanar")
            hip.check(L.hbhip_frame_export_surface(fr, surface.h), ctx.h, "export_surface")
            hip.check(L.hbhip_frame_import_surface(fr, surface.h), ctx.h, "import_surface")
            hip.check(L.hbhip_frame_download_biplanar(fr, C.byref(hb)), ctx.h, "download_biplanar")
        surface.close()
        L.hbhip_frame_release(fr)
    ctx.close()


def company_summarize(trace):
    seq = {}
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"(bi_split_kernel|bi_merge_kernel|bi_surface_split_kernel|bi_surface_merge_kernel)<([^>]*)>", r["Kernel_Name"])
        if m:
            seq.setdefault((m.group(1), 8 if "char" in m.group(2) else 10), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    stats = lambda v: [round(float(np.mean(v)), 2), round(min(v), 2), round(float(np.median(v)), 2)]
    out = {}
    for (k, d), v in seq.items():
        out[f"{k} {d}"] = {"A_back_to_back": stats(v[:64]), "B_between_copies": stats(v[64:128])} if "surface" in k else {"B": stats(v)}
    print(json.dumps(out, indent=1))


WIDEN_FRAMES, WIDEN_ROUNDS = 16, 2
WIDEN_FORMS = ["bi_merge_kernel<uint16_t>", "widen, staging", "bi_surface_merge_kernel<uint16_t>", "widen, surface"]


def widen():
    """P010LE out of 1080p frames four ways, 16 resident frames a form, the forms alternated, two rounds behind one
    warm-up launch a form: the 10-bit merges (ten-bit frames) and the widening merges (8-bit frames), into a host picture
    of the staging layout and into a (256, 16) surface"""
    from handbrake_amd import hip
    L = hip.lib()
    ctx = hip.Ctx(0)
    w, h, n = 1920, 1080, WIDEN_FRAMES
    rng = np.random.default_rng(1)
    ch, cw = h // 2, w // 2
    f8, f10 = [hip.Frame(ctx, w, h, 8) for _ in range(n)], [hip.Frame(ctx, w, h, 10) for _ in range(n)]
    for k in range(n):
        f8[k].upload([rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw))])
        f10[k].upload([rng.integers(0, 1024, s).astype(np.uint16) for s in ((h, w), (ch, cw), (ch, cw))])
    pitch = align64(2 * w)
    host = np.zeros(pitch * (h + ch), dtype=np.uint8)
    hb = hip.HostBiplanar()
    hb.plane[0], hb.plane[1] = host.ctypes.data, host.ctypes.data + pitch * h
    hb.stride[0] = hb.stride[1] = pitch
    surface = hip.Surface(ctx, w, h, 10)
    forms = [lambda k: L.hbhip_frame_download_biplanar(f10[k].h, C.byref(hb)),
             lambda k: L.hbhip_frame_download_widen(f8[k].h, C.byref(hb)),
             lambda k: L.hbhip_frame_export_surface(f10[k].h, surface.h),
             lambda k: L.hbhip_frame_export_surface_widen(f8[k].h, surface.h)]
    for form in forms:                                                      # code objects, the staging buffer
        hip.check(form(0), ctx.h, "warm-up")
    for _ in range(WIDEN_ROUNDS):
        for form in forms:
            for k in range(n):
                hip.check(form(k), ctx.h, "widen")
    surface.close()
    for fr in f8 + f10:
        fr.close()
    ctx.close()


def widen_summarize(trace):
    """per form [mean, min, median] µs of its 2 x 16 timed launches, and the widening forms' means over their siblings'.
    The two widening forms are one kernel on one grid: told apart by their place in widen()'s order."""
    seq = {}
    for r in sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"bi_merge_kernel<|bi_surface_merge_kernel<|bi_widen_merge_kernel", r["Kernel_Name"])
        if m:
            seq.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    n = WIDEN_FRAMES
    wide = seq["bi_widen_merge_kernel"]
    assert len(wide) == 2 + 2 * n * WIDEN_ROUNDS and all(len(seq[k]) == 1 + n * WIDEN_ROUNDS for k in ("bi_merge_kernel<", "bi_surface_merge_kernel<"))
    timed = wide[2:]
    per = {WIDEN_FORMS[0]: seq["bi_merge_kernel<"][1:], WIDEN_FORMS[2]: seq["bi_surface_merge_kernel<"][1:],
           WIDEN_FORMS[1]: [t for r in range(WIDEN_ROUNDS) for t in timed[2 * n * r:2 * n * r + n]],
           WIDEN_FORMS[3]: [t for r in range(WIDEN_ROUNDS) for t in timed[2 * n * r + n:2 * n * (r + 1)]]}
    out = {k: {"mean_us": round(float(np.mean(per[k])), 2), "min_us": round(min(per[k]), 2),
               "median_us": round(float(np.median(per[k])), 2),
               "round_means_us": [round(float(np.mean(per[k][n * r:n * (r + 1)])), 2) for r in range(WIDEN_ROUNDS)]} for k in WIDEN_FORMS}
    out["widen_over_sibling"] = {"staging": round(out[WIDEN_FORMS[1]]["mean_us"] / out[WIDEN_FORMS[0]]["mean_us"], 3),
                                 "surface": round(out[WIDEN_FORMS[3]]["mean_us"] / out[WIDEN_FORMS[2]]["mean_us"], 3)}
    print(json.dumps(out, indent=1))


def adapters(n_in):
    from handbrake_amd import hbrt, hip, synth
    w, h, n_warm = 1920, 1080, 64
    planar = synth.stream("progressive", w, h, 48)
    nv12 = [(f[0], np.ascontiguousarray(np.stack([f[1], f[2]], axis=2).reshape(f[1].shape[0], -1))) for f in planar]
    lists = {"planar": (planar, 0, ""), "nv12": (nv12, NV12, "format=nv12")}

    def one(which):
        frames, pix_fmt, fmt = lists[which]
        chain = [("hb_filter_hip_upload", ""), ("hb_filter_lapsharp_hip", LAP), ("hb_filter_hip_download", fmt)]
        hbrt.set_threaded(True)
        hbrt.set_discard_output(True)
        try:
            with hbrt.Chain(hip.filters(), chain, w, h, pix_fmt) as ch:
                ch.feed(frames, 0, n_warm, flags=0x10, threads=4)
                t_end = time.perf_counter() + 10
                while ch.produced() < n_warm - 16 and time.perf_counter() < t_end:      # (the adapters keep a few frames in flight)
                    time.sleep(0.002)
                t0 = time.perf_counter()
                busy0 = [ch.stage_busy_ms(k) for k in range(3)]
                ch.feed(frames, n_warm, n_in, flags=0x10, threads=4)
                ch.push_eof()
                dt = time.perf_counter() - t0
                assert ch.produced() == n_warm + n_in
                busy[which].append([round((ch.stage_busy_ms(k) - busy0[k]) / (dt * 1e3), 3) for k in range(3)])
        finally:
            hbrt.set_discard_output(False)
            hbrt.set_threaded(False)
        return n_in / dt

    busy = {"planar": [], "nv12": []}
    one("planar"), one("nv12")                                            # pinned pool, code objects
    runs = {"planar": [], "nv12": []}
    busy = {"planar": [], "nv12": []}
    for _ in range(3):
        for which in ("planar", "nv12"):
            runs[which].append(round(one(which), 1))
    out = {"list": "[hip_upload, lapsharp_hip, hip_download] 1920x1080, a thread per filter", "frames_per_run": n_in}
    for which, v in runs.items():
        out[which] = {"fps": v, "mean": round(sum(v) / 3, 1), "spread_pct": round((max(v) - min(v)) / (sum(v) / 3) * 100, 2),
                      "thread_busy_fraction [upload, lapsharp, download]": busy[which]}
    out["nv12_over_planar"] = round(out["nv12"]["mean"] / out["planar"]["mean"], 4)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "repack":
        repack(sys.argv[2] if len(sys.argv) > 2 else None)
    elif mode == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    elif mode == "company":
        company()
    elif mode == "company-summarize":
        company_summarize(sys.argv[2])
    elif mode == "widen":
        widen()
    elif mode == "widen-summarize":
        widen_summarize(sys.argv[2])
    elif mode == "adapters":
        adapters(int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
    else:
        sys.exit(__doc__)
