#!/usr/bin/env python3
"""Times one stateless filter's batch path (16 device-resident 1080p frames per call) with the context's kernel timer.
usage: quick_filter.py unsharp|chroma_smooth|lapsharp|colorspace_sdr|colorspace_matrix|colorspace_pq[_loc<0..6>]|grayscale|rotate|scale<W>x<H>|
                      format8to10|format10to8|format_422_420[_10]|format_444_422[_10]|format_444_420[_10]|
                      format_<444|422|420>_<422|420>_<10to8|12to8|12to10> (a lower depth; 420_420: the depth alone)|
                      format_<444|422>_<422|420>_<8to10|8to12|10to12> (fewer chroma samples at a higher depth)|
                     format_<420|422>_<422|444>_up[_10|_8to10|_8to12|_10to12] (more chroma samples, equal or higher depth)|
                      deblock_<preset>_<tune>[_10]|deband[_<range>][_10][_tile|_gather]|bm3d[_<sigma>][_10] [reps]
Prints one line per kernel: name, launches, average us.  For knob experiments with tools/dev_run.sh."""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from handbrake_amd import hip, synth

W, H, NB = int(os.environ.get("QF_W", 1920)), int(os.environ.get("QF_H", 1080)), 16


def planes(w, h, dtype=torch.uint8, sub=(1, 1)):
    def plane(pw, ph):
        return torch.empty((ph, (pw + 63) // 64 * 64), dtype=dtype, device="cuda")[:, :pw]
    return [plane(w, h), plane(w >> sub[0], h >> sub[1]), plane(w >> sub[0], h >> sub[1])]


def deint(ctx, what, reps):
    """FFmpeg yadif / bwdif as the Deinterlace / Bwdif filters configure them: frames pushed one by one (decomb's surface)"""
    bob = 1 if what == "yadif_bob" else 0
    if what == "bwdif":
        flt = hip._create("hbhip_bwdif_create", ctx, [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p)], ctx.h, bob, 0, -1, W, H, 8, 1, 1)
    else:
        flt = hip._create("hbhip_yadif_create", ctx, [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_void_p)], ctx.h, 1, bob, 0, -1, W, H, 8, 1, 1)
    frames = synth.stream("interlaced", W, H, 4)
    dev_in = [[torch.from_numpy(p).cuda() for p in fr] for fr in frames]
    out = planes(W, H)
    torch.cuda.synchronize()
    fin = [hip.dev_frame(f) for f in dev_in]
    fo = hip.dev_frame(out)

    def feed(i):
        hip.decomb_push_dev(flt, fin[i % 4], i, 0x0008, 2)
        while flt.pending():
            flt.pull_dev(fo)
    for i in range(3):
        feed(i)
    ctx.sync(); ctx.profile(True); ctx.profile_reset()
    for i in range(NB * reps // 4):
        feed(3 + i)
    ctx.sync()
    st = ctx.profile_stats(); ctx.profile(False)
    digest = int(out[0].to(torch.int64).sum().item())
    for k, (n, ms) in st.items():
        print(f"{what} {k} launches {n} avg_us {ms / n * 1e3:.2f} digest {digest}")
    flt.close(); ctx.close()


def main():
    what = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    ctx = hip.Ctx(0)

    def mk_blur(fn, luma_amount=16384, size=7):
        class BP(C.Structure):
            _fields_ = [("amount", C.c_int * 3), ("size", C.c_int * 3)]
        p = BP((C.c_int * 3)(luma_amount, 16384, 16384), (C.c_int * 3)(size, size, size))
        return hip._create(fn, ctx, [C.c_void_p, C.POINTER(BP)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                           ctx.h, C.byref(p), W, H, 8, 1, 1)
    ow, oh = W, H
    depth_in = depth_out = 8
    picture = "progressive"
    sub_in = sub_out = (1, 1)                          # log2 chroma subsampling of the frames going in / coming out
    if what == "unsharp": make = lambda: mk_blur("hbhip_unsharp_create")
    elif what == "unsharp5": make = lambda: mk_blur("hbhip_unsharp_create", size=5)
    elif what == "chroma_smooth": make = lambda: mk_blur("hbhip_chroma_smooth_create", 0)
    elif what == "lapsharp": make = lambda: hip.lapsharp_device_filter(ctx, W, H)
    elif what == "lapsharp10":
        make = lambda: hip.lapsharp_device_filter(ctx, W, H, depth=10)
        depth_in = depth_out = 10
    elif what == "colorspace_sdr": make = lambda: hip.colorspace_device_filter(ctx, W, H, (6, 6, 6, 1), (1, 1, 1, 1))
    elif what == "colorspace_matrix": make = lambda: hip.colorspace_device_filter(ctx, W, H, (1, 1, 1, 1), (1, 1, 6, 2))
    elif what.startswith("colorspace_pq"):             # colorspace_pq, colorspace_pq_loc3: HDR10 -> BT.709 hable at 10 bits, a chroma location
        loc = int(what.split("_loc")[1]) if "_loc" in what else None
        make = lambda: hip.colorspace_device_filter(ctx, W, H, (9, 16, 9, 1), (1, 1, 1, 1), tonemap="hable", peak=100.0, depth=10,
                                                    chroma_location=loc)
        depth_in = depth_out = 10
    elif what == "grayscale":
        make = lambda: hip._create("hbhip_grayscale_create", ctx, [C.c_void_p] + [C.c_double] * 4 + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, 0.0, 0.0, 1.0, 0.0, W, H, 8, 1, 1)
    elif what == "rotate":
        make = lambda: hip._create("hbhip_rotate_create", ctx, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p)], ctx.h, 90, 0, W, H, 8, 1, 1)
        ow, oh = H, W
    elif what in ("format8to10", "format10to8"):
        sd, dd = (8, 10) if what == "format8to10" else (10, 8)
        make = lambda: hip._create("hbhip_format_create", ctx, [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p)], ctx.h, W, H, sd, dd, 1, 1, 0)
        depth_in, depth_out = sd, dd
    elif what.startswith("format_"):                   # format_422_420, format_444_420_10 ...: chroma down-sampling
        parts = what.split("_")
        subs = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
        sub_in, sub_out = subs[parts[1]], subs[parts[2]]
        if "up" in parts:                              # format_420_422_up, format_422_444_up_10, format_420_444_up_8to10 ...: MORE chroma
            depth_in, depth_out = (int(v) for v in parts[-1].split("to")) if "to" in parts[-1] else (10, 10) if parts[-1] == "10" else (8, 8)
            make = lambda: hip.format_upsample_device_filter(ctx, W, H, sub_in, sub_out, depth_in, depth_out)
        elif "to" in parts[-1]:                         # format_422_420_10to8, format_420_420_12to10 ...: the scaled form
            depth_in, depth_out = (int(v) for v in parts[-1].split("to"))
            if depth_out > depth_in:                   # format_422_420_8to10, format_444_422_10to12 ...: the deepen form
                make = lambda: hip.format_deepen_device_filter(ctx, W, H, sub_in, sub_out, depth_in, depth_out)
            else:
                make = lambda: hip.format_scaled_device_filter(ctx, W, H, sub_in, sub_out, depth_in, depth_out)
        else:
            depth_in = depth_out = 10 if parts[-1] == "10" else 8
            make = lambda: hip.format_resample_device_filter(ctx, W, H, sub_in, sub_out, depth_in)
    elif what.startswith("scale"):                     # scale960x540, scale1280x720, scale3840x2160 ...
        ow, oh = (int(v) for v in what[5:].split("x"))
        make = lambda: hip.cropscale_device_filter(ctx, W, H, ow, oh)
    elif what == "pad":
        class PP(C.Structure):
            _fields_ = [("width", C.c_int), ("height", C.c_int), ("x", C.c_int), ("y", C.c_int), ("fill", C.c_int * 3)]
        pp = PP(W + 128, H + 72, 64, 36, (C.c_int * 3)(16, 128, 128))
        make = lambda: hip._create("hbhip_pad_create", ctx, [C.c_void_p, C.POINTER(PP)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)], ctx.h, C.byref(pp), W, H, 8, 1, 1)
        ow, oh = W + 128, H + 72
    elif what.startswith("deblock"):                   # deblock_<preset>_<tune>[_10]: deblock_medium_medium, deblock_medium_small_10 ...
        parts = what.split("_")
        tunes = {"small": ":blocksize=4", "medium": "", "large": ":blocksize=16"}
        presets = {"ultralight": "strength=weak:thresh=20", "light": "strength=weak:thresh=50", "medium": "strength=strong:thresh=20",
                   "strong": "strength=strong:thresh=50", "stronger": "strength=strong:thresh=75", "verystrong": "strength=strong:thresh=100"}
        depth_in = depth_out = 10 if parts[-1] == "10" else 8
        dp = hip.DeblockParams()
        F = hip.filters()
        F.hbhip_deblock_params_from_settings.argtypes = [C.c_char_p] + [C.c_int] * 5 + [C.POINTER(hip.DeblockParams)]
        if F.hbhip_deblock_params_from_settings((presets[parts[1]] + tunes[parts[2]]).encode(), depth_in, W, H, 1, 1, C.byref(dp)):
            raise SystemExit("deblock declines " + what)
        make = lambda: hip._create("hbhip_deblock_create", ctx, [C.c_void_p, C.POINTER(hip.DeblockParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, C.byref(dp), W, H, depth_in, 1, 1)
        picture = "blocky"
    elif what.startswith("deband"):                    # deband[_<range>][_10][_tile|_gather]: deband, deband_10, deband_64_gather ...
        parts = what.split("_")[1:]
        kernel = {"tile": 1, "gather": 2}.get(parts[-1], 0) if parts else 0
        if kernel:
            parts = parts[:-1]
        depth_in = depth_out = 10 if parts and parts[-1] == "10" else 8
        if depth_in == 10:
            parts = parts[:-1]
        rng = int(parts[0]) if parts else 16
        bp = hip.DebandParams()
        F = hip.filters()
        F.hbhip_deband_params_from_settings.argtypes = [C.c_char_p, C.c_int, C.POINTER(hip.DebandParams)]
        if F.hbhip_deband_params_from_settings(f"range={rng}".encode(), depth_in, C.byref(bp)):
            raise SystemExit("deband declines " + what)

        def make():
            f = hip._create("hbhip_deband_create", ctx, [C.c_void_p, C.POINTER(hip.DebandParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                            ctx.h, C.byref(bp), W, H, depth_in, 1, 1)
            hip.lib().hbhip_deband_set_kernel.argtypes = [C.c_void_p, C.c_int]
            if hip.lib().hbhip_deband_set_kernel(f.h, kernel):
                raise SystemExit("no such kernel for " + what)
            return f
        picture = "banded"
    elif what.startswith("bm3d"):                      # bm3d[_<sigma>][_10]: bm3d (sigma 3), bm3d_6, bm3d_10, bm3d_6_10
        parts = what.split("_")[1:]
        depth_in = depth_out = 10 if parts and parts[-1] == "10" else 8
        if depth_in == 10:
            parts = parts[:-1]
        mp = hip.Bm3dParams()
        if hip.lib().hbhip_bm3d_params_from_settings(f"sigma={parts[0] if parts else 3}".encode(), depth_in, C.byref(mp)):
            raise SystemExit("bm3d declines " + what)
        make = lambda: hip._create("hbhip_bm3d_create", ctx, [C.c_void_p, C.POINTER(hip.Bm3dParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                                   ctx.h, C.byref(mp), W, H, depth_in, 1, 1)
    elif what in ("yadif", "yadif_bob", "bwdif"):
        return deint(ctx, what, reps)
    else:
        raise SystemExit("unknown filter " + what)
    if sub_in != (1, 1):
        chroma = {(1, 0): "2x1", (0, 0): "1x1"}[sub_in]
        frames = [synth.picture(picture, W, H, t, depth=depth_in, chroma=chroma) for t in range(4)]
    else:
        frames = synth.stream(picture, W, H, 4, depth=depth_in) if depth_in != 8 else synth.stream(picture, W, H, 4)
    dev_in = [[torch.from_numpy(p.view(np.int16) if depth_in != 8 else p).cuda() for p in fr] for fr in frames]
    outs = [planes(ow, oh, torch.int16 if depth_out != 8 else torch.uint8, sub_out) for _ in range(NB)]
    torch.cuda.synchronize()
    flt = make()
    arr_in = (hip.DevFrame * NB)(*[hip.dev_frame(dev_in[i % 4]) for i in range(NB)])
    arr_out = (hip.DevFrame * NB)(*[hip.dev_frame(o) for o in outs])
    for _ in range(2):
        flt.process_dev(arr_in, 0, arr_out)
    ctx.sync(); ctx.profile(True); ctx.profile_reset()
    for _ in range(reps):
        flt.process_dev(arr_in, 0, arr_out)
    ctx.sync()
    st = ctx.profile_stats(); ctx.profile(False)
    digest = int(sum(int(o[0].to(torch.int64).sum().item()) for o in outs[:2]))
    for k, (n, ms) in st.items():
        print(f"{what} {k} launches {n} avg_us {ms / n * 1e3:.2f} digest {digest}")
    flt.close(); ctx.close()


if __name__ == "__main__":
    main()
