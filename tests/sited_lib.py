"""Test-side plumbing for the chroma-siting tests: the sited colour-conversion checker (tools/colorspace_sited_check.c,
built as tools/libcolorspace_sited_check.so) and the crop/scale oracle's planes called with the shifts of
tests/chroma_siting_model.py.  Beside oracle_lib.py, which stays as it is."""
import ctypes as C
import os
import subprocess

import numpy as np

import chroma_siting_model as csm
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "tools", "libcolorspace_sited_check.so")
_lib = None


def checker():
    global _lib
    if _lib is None:
        if not os.path.exists(CHECKER):                # built by `make product` (__graft_entry__.build())
            subprocess.run(["make", "-C", ROOT, "tools/libcolorspace_sited_check.so"], capture_output=True, timeout=600)
        assert os.path.exists(CHECKER), "tools/libcolorspace_sited_check.so is not built (make product)"
        _lib = C.CDLL(CHECKER)
    return _lib


def colorspace_frame_sited(frame, params, depth=8, subw=1, subh=1, h_centred=False, v_cosited=False):
    """orc_colorspace_frame with the two siting axes (both off: orc_colorspace_frame itself)"""
    fn = checker().orc_colorspace_frame_sited
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(ol.ColorspaceParams), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                   C.POINTER(C.c_void_p), C.POINTER(C.c_int)] + [C.c_int] * 7
    src = [np.ascontiguousarray(p) for p in frame]
    dst = [np.zeros_like(p) for p in src]
    h, w = src[0].shape
    sp = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    dp = (C.c_void_p * 3)(*[p.ctypes.data for p in dst])
    ss = (C.c_int * 3)(*[p.strides[0] for p in src])
    ds = (C.c_int * 3)(*[p.strides[0] for p in dst])
    rc = fn(C.byref(params), sp, ss, dp, ds, w, h, depth, subw, subh, int(h_centred), int(v_cosited))
    if rc != 0:
        raise ValueError("conversion not covered by the oracle")
    return tuple(dst)


def colorspace_frame_at(frame, params, loc, depth=8, subw=1, subh=1):
    hc, vc = csm.colour_forms(loc)
    return colorspace_frame_sited(frame, params, depth, subw, subh, hc and subw, vc and subh)


def cropscale_plane(plane, dw, dh, shift_x, shift_y, depth=8, arithmetic="fixed"):
    """one plane through the crop/scale oracle (no crop) with the shifts given"""
    p = np.ascontiguousarray(plane)
    h, w = p.shape
    dst = np.zeros((dh, dw), p.dtype)
    common = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
              C.c_double, C.c_double]
    args = [p.ctypes.data, p.strides[0], 0, 0, w, h, dst.ctypes.data, dst.strides[0], dw, dh, shift_x, shift_y]
    if arithmetic == "fixed" and depth == 8:
        fn = ol.oracle().orc_cropscale_plane_fx
        fn.argtypes = common
    else:
        fn = ol.oracle().orc_cropscale_plane_fx16 if arithmetic == "fixed" else ol.oracle().orc_cropscale_plane_d
        fn.argtypes = common + [C.c_int]
        args.append(depth)
    fn.restype = None
    fn(*args)
    return dst


def cropscale_frame_at(frame, width, height, loc, depth=8, sub="2x2", arithmetic="fixed"):
    """crop/scale oracle of a frame whose chroma sits at AVCHROMA_LOC_* `loc`: the model's shifts per plane"""
    h0, w0 = frame[0].shape
    lw, lh = ol.SUBSAMPLING[sub]
    sx, sy = csm.shifts(loc, lw, lh, w0, width, h0, height)
    out = [cropscale_plane(frame[0], width, height, 0.0, 0.0, depth, arithmetic)]
    for p in frame[1:]:
        out.append(cropscale_plane(p, -(-width >> lw), -(-height >> lh), sx, sy, depth, arithmetic))
    return tuple(out)


def process_dev(flt, ctx, frames, out_shapes, depth):
    """the frames (tuples of numpy planes) through hbhip_filter_process_dev in ONE call -> list of lists of planes"""
    import torch
    from handbrake_amd import hip
    npdt, tdt = (np.uint8, torch.uint8) if depth == 8 else (np.int16, torch.int16)
    dev_in = [[torch.from_numpy(np.ascontiguousarray(p).view(npdt)).cuda() for p in f] for f in frames]
    outs = [[torch.zeros(s, dtype=tdt, device="cuda") for s in out_shapes] for _ in frames]
    torch.cuda.synchronize()
    n = len(frames)
    arr_in = (hip.DevFrame * n)(*[hip.dev_frame(f) for f in dev_in])
    arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
    assert flt.process_dev(arr_in, 0, arr_out) == n
    ctx.sync()
    return [[p.cpu().numpy().view(np.uint8 if depth == 8 else np.uint16) for p in o] for o in outs]

