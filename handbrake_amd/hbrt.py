"""ctypes binding of the filter-chain driver (libhb/hb_harness.c in libhbrt.so).

The driver plays work.c's role for a list of ``hb_filter_object_t`` - it does
not care whether they are the HIP drop-ins (``libhbhip_filters.so``) or the
reference's own objects (``oracle/_ref/libhbref.so``, tests only).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

AV_PIX_FMT_YUV420P = 0
AV_PIX_FMT_YUV420P10 = 62
AV_PIX_FMT_YUV420P12 = 123
PIX_FMT_FOR_DEPTH = {8: AV_PIX_FMT_YUV420P, 10: AV_PIX_FMT_YUV420P10, 12: AV_PIX_FMT_YUV420P12}
# (chroma subsampling "WxH" of a chroma sample in luma samples, depth) -> AVPixelFormat, hbffmpeg.c:893-909
PIX_FMT = {("2x2", 8): 0, ("2x1", 8): 4, ("1x1", 8): 5, ("2x2", 10): 62, ("2x1", 10): 64, ("1x1", 10): 68,
           ("2x2", 12): 123, ("2x1", 12): 127, ("1x1", 12): 131}

# biplanar 4:2:0: frames are two arrays, Y and the interleaved CbCr rows of shape (ceil(h / 2), 2 * ceil(w / 2)); P010LE
# samples are uint16 with their 10 bits in the high end
AV_PIX_FMT_NV12, AV_PIX_FMT_P010LE = 23, 158
BIPLANAR = (AV_PIX_FMT_NV12, AV_PIX_FMT_P010LE)
# the four packed 32-bit RGB orders with alpha, FFmpeg's numbers: what hb_get_preview asks `format` for
RGB32_BY_NAME = {"argb": 25, "rgba": 26, "abgr": 27, "bgra": 28}
RGB32 = tuple(RGB32_BY_NAME.values())

HB_COMB_NONE, HB_COMB_LIGHT, HB_COMB_HEAVY = 0, 1, 2


class FrameInfo(C.Structure):
    _fields_ = [("is_eof", C.c_int), ("start", C.c_int64), ("stop", C.c_int64),
                ("flags", C.c_int), ("combed", C.c_int), ("width", C.c_int),
                ("height", C.c_int), ("fmt", C.c_int), ("nplanes", C.c_int),
                ("plane_width", C.c_int * 4), ("plane_height", C.c_int * 4),
                ("plane_stride", C.c_int * 4)]


_rt = None


def runtime() -> C.CDLL:
    """libhbrt.so, loaded RTLD_GLOBAL so filter libraries resolve against it."""
    global _rt
    if _rt is None:
        path = os.path.join(_HERE, "libhbrt.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing - run `make` (or __graft_entry__.build())")
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        lib.hbh_chain_open.restype = C.c_void_p
        lib.hbh_chain_open.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p),
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.hbh_chain_push.restype = C.c_int
        lib.hbh_chain_push.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                       C.c_int64, C.c_int64, C.c_int, C.c_int]
        lib.hbh_chain_push_eof.restype = C.c_int
        lib.hbh_chain_push_eof.argtypes = [C.c_void_p]
        lib.hbh_chain_pending.restype = C.c_int
        lib.hbh_chain_pending.argtypes = [C.c_void_p]
        lib.hbh_chain_produced.restype = C.c_int
        lib.hbh_chain_produced.argtypes = [C.c_void_p]
        lib.hbh_chain_stage_busy_ms.restype = C.c_double
        lib.hbh_chain_stage_busy_ms.argtypes = [C.c_void_p, C.c_int]
        lib.hbh_chain_peek.restype = C.c_int
        lib.hbh_chain_peek.argtypes = [C.c_void_p, C.POINTER(FrameInfo)]
        lib.hbh_chain_pop.restype = C.c_int
        lib.hbh_chain_pop.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        lib.hbh_chain_output_geometry.restype = None
        lib.hbh_chain_output_geometry.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        lib.hbh_chain_close.restype = None
        lib.hbh_chain_close.argtypes = [C.c_void_p]
        lib.hbh_job_open.restype = C.c_void_p
        lib.hbh_job_open.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p)] + [C.c_int] * 6
        lib.hbh_chain_describe.restype = C.c_int
        lib.hbh_chain_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        lib.hbhip_rt_register_filter.restype = None
        lib.hbhip_rt_register_filter.argtypes = [C.c_int, C.c_void_p]
        lib.hbhip_set_log_level.argtypes = [C.c_int]
        lib.hbhip_set_cpu_count.argtypes = [C.c_int]
        _rt = lib
    return _rt


@dataclass
class OutFrame:
    planes: tuple          # (Y, Cb, Cr) uint8 arrays, cropped to plane width; (Y, CbCr) for NV12 / P010LE
    start: int
    stop: int
    flags: int
    combed: int
    width: int
    height: int


class Chain:
    """A filter chain: ``Chain(lib, [("hb_filter_nlmeans", "y-strength=6")], w, h)``."""

    def __init__(self, lib: C.CDLL, stages, width: int, height: int,
                 pix_fmt: int = AV_PIX_FMT_YUV420P, vrate=(30000, 1001)):
        self._rt = runtime()
        n = len(stages)
        protos = (C.c_void_p * n)()
        settings = (C.c_char_p * n)()
        for i, (sym, st) in enumerate(stages):
            protos[i] = C.addressof(C.c_char.in_dll(lib, sym))
            settings[i] = (st or "").encode()
        self._keep = (lib, protos, settings)
        self.width, self.height = width, height
        self._h = self._rt.hbh_chain_open(n, protos, settings, pix_fmt, width, height,
                                          vrate[0], vrate[1])
        if not self._h:
            raise RuntimeError(f"filter chain init failed: {stages}")
        self.eof = False

    def push(self, planes, start: int = 0, stop: int = 3003, flags: int = 0x10, combed: int = 0):
        ptrs = (C.c_void_p * 3)()
        strides = (C.c_int * 3)()
        keep = []
        for i, p in enumerate(planes):
            a = np.ascontiguousarray(p)
            keep.append(a)
            ptrs[i] = a.ctypes.data
            strides[i] = a.strides[0]
        rc = self._rt.hbh_chain_push(self._h, ptrs, strides, start, stop, flags, combed)
        if rc != 0:
            raise RuntimeError(f"hbh_chain_push failed ({rc})")

    def feed(self, frames, first: int, count: int, duration: int = 3003, flags: int = 0x10, threads: int = 4):
        """`count` frames cycling through the pictures of `frames` (same shapes), numbered from `first`: copied into
        hb_buffer_t's by `threads` C threads and pushed in order (hbh_chain_feed) - a source that keeps up"""
        n = len(frames)
        keep = [[np.ascontiguousarray(p) for p in fr] for fr in frames]
        ptrs = (C.c_void_p * (3 * n))(*[fr[k].ctypes.data if k < len(fr) else None for fr in keep for k in range(3)])
        strides = (C.c_int * 3)(*[p.strides[0] for p in keep[0]])
        for fr in keep:
            assert [p.strides[0] for p in fr] == list(strides)[:len(fr)]      # (two planes: NV12 / P010LE)
        self._rt.hbh_chain_feed.restype = C.c_int
        self._rt.hbh_chain_feed.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                            C.c_int64, C.c_int, C.c_int]
        rc = self._rt.hbh_chain_feed(self._h, ptrs, strides, n, first, count, duration, flags, threads)
        if rc != 0:
            raise RuntimeError(f"hbh_chain_feed failed ({rc})")

    def push_surface(self, surface, flags: int = 0x10, pts: int = 0):
        """A frame that lies in device memory already: `surface` is a hip.Surface (NV12 / P010LE, the chain's pix_fmt); the
        buffer gets a reference of its own."""
        self._rt.hbh_chain_push_surface.restype = C.c_int
        self._rt.hbh_chain_push_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64]
        surface.retain()                                   # the call takes a reference over
        rc = self._rt.hbh_chain_push_surface(self._h, surface.h, flags, pts)
        if rc != 0:
            raise RuntimeError(f"hbh_chain_push_surface failed ({rc})")

    def feed_surfaces(self, surfaces, first: int, count: int, duration: int = 3003, flags: int = 0x10):
        """the surface form of feed(): `count` buffers cycling through the hip.Surface objects of `surfaces`, nothing copied"""
        from . import hip
        n = len(surfaces)
        ptrs = (C.c_void_p * n)(*[s.h.value for s in surfaces])
        self._rt.hbh_chain_feed_surfaces.restype = C.c_int
        self._rt.hbh_chain_feed_surfaces.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int64,
                                                     C.c_int, C.c_void_p]
        retain = C.cast(hip.lib().hbhip_surface_retain, C.c_void_p)
        rc = self._rt.hbh_chain_feed_surfaces(self._h, ptrs, n, first, count, duration, flags, retain)
        if rc != 0:
            raise RuntimeError(f"hbh_chain_feed_surfaces failed ({rc})")

    def pop_surface(self):
        """Next output as (hip.Surface, FrameInfo) when it is a surface buffer - the buffer's reference is the object's, close()
        gives the surface back; None for the EOF marker, an empty queue or a host frame (which stays queued for pop())."""
        from . import hip
        info = FrameInfo()
        if self._rt.hbh_chain_peek(self._h, C.byref(info)) != 0:
            return None
        if info.is_eof:
            self._rt.hbh_chain_pop(self._h, None, None)
            self.eof = True
            return None
        self._rt.hbh_chain_pop_surface.restype = C.c_int
        self._rt.hbh_chain_pop_surface.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        if self._rt.hbh_chain_pop_surface(self._h, C.byref(h)) != 0:
            return None
        return hip.Surface.adopt(h), info

    def push_eof(self):
        rc = self._rt.hbh_chain_push_eof(self._h)
        if rc != 0:
            raise RuntimeError(f"hbh_chain_push_eof failed ({rc})")

    def pending(self) -> int:
        return self._rt.hbh_chain_pending(self._h)

    def produced(self) -> int:
        """Threaded mode: frames the last stage has made so far (callable while the stages run)."""
        return self._rt.hbh_chain_produced(self._h)

    def stage_busy_ms(self, stage: int) -> float:
        """Threaded mode: milliseconds the stage's thread has spent inside work() so far."""
        return self._rt.hbh_chain_stage_busy_ms(self._h, stage)

    def pop(self):
        """Next output frame, or None for the EOF marker / empty queue."""
        info = FrameInfo()
        if self._rt.hbh_chain_peek(self._h, C.byref(info)) != 0:
            return None
        if info.is_eof or info.nplanes == 0:
            self._rt.hbh_chain_pop(self._h, None, None)
            self.eof = True
            return None
        ptrs = (C.c_void_p * 3)()
        strides = (C.c_int * 3)()
        arrs = []
        for p in range(info.nplanes):
            a = np.empty((info.plane_height[p], info.plane_stride[p]), dtype=np.uint8)
            arrs.append(a)
            ptrs[p] = a.ctypes.data
            strides[p] = a.strides[0]
        self._rt.hbh_chain_pop(self._h, ptrs, strides)
        bps = 2 if info.fmt in (62, 123, 64, 68, 127, 131, AV_PIX_FMT_P010LE) else 1
        # plane 1 of a biplanar frame holds two samples, Cb and Cr, per chroma position
        # ... and the one plane of a packed 32-bit RGB picture four bytes a pixel
        per = [4 if info.fmt in RGB32 else 2 if info.fmt in BIPLANAR and p == 1 else 1 for p in range(info.nplanes)]
        planes = tuple(a[:, : info.plane_width[p] * bps * per[p]] for p, a in enumerate(arrs))
        if bps == 2:                      # 10 / 12-bit samples in 16-bit containers
            planes = tuple(np.ascontiguousarray(p).view(np.uint16) for p in planes)
        return OutFrame(planes, info.start, info.stop, info.flags, info.combed,
                        info.width, info.height)

    def drain(self):
        out = []
        while self.pending():
            f = self.pop()
            if f is not None:
                out.append(f)
        return out

    def output_geometry(self):
        v = [C.c_int() for _ in range(4)]
        self._rt.hbh_chain_output_geometry(self._h, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def close(self):
        if self._h:
            self._rt.hbh_chain_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_layout(pix_fmt: int, width: int, height: int) -> FrameInfo:
    """What hb_frame_buffer_init makes of a format: nplanes (max_plane + 1), plane_width / _height / _stride per plane;
    plane_width[3] is the byte distance from plane 0 to the last plane."""
    rt = runtime()
    rt.hbh_frame_layout.restype = C.c_int
    rt.hbh_frame_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(FrameInfo)]
    info = FrameInfo()
    if rt.hbh_frame_layout(pix_fmt, width, height, C.byref(info)) != 0:
        raise RuntimeError(f"no frame layout for pix_fmt {pix_fmt}")
    return info


# hb_filter_object_t ids (handbrake/common.h:1729-1778; include/hbhip_libhb.h)
FILTER_ID = {"detelecine": 3, "comb_detect": 4, "decomb": 6, "yadif": 7, "bwdif": 9, "vfr": 11, "deblock": 12, "deband": 13, "bm3d": 15, "render_sub": 21, "denoise": 14, "nlmeans": 16, "chroma_smooth": 17,
             "rotate": 19, "crop_scale": 22, "lapsharp": 24, "unsharp": 26, "grayscale": 28, "pad": 30,
             "colorspace": 32, "format": 33}


def register_filters(lib: C.CDLL, symbols: dict):
    """What hb_filter_get's switch holds inside libhb: {filter id: symbol of the registered object in `lib`}."""
    rt = runtime()
    for fid, sym in symbols.items():
        rt.hbhip_rt_register_filter(fid, None if sym is None else C.addressof(C.c_char.in_dll(lib, sym)))
    return lib


class Job(Chain):
    """A chain built the way do_job() builds it (hbh_job_open): filters by id from the registered objects, the HIP
    swap + adapters (hb_hip_setup_hw_filters) when use_hip, CPU fallback when a drop-in's init declines."""

    def __init__(self, filters, width: int, height: int, pix_fmt: int = AV_PIX_FMT_YUV420P, vrate=(30000, 1001),
                 use_hip: bool = True):
        self._rt = runtime()
        n = len(filters)
        ids = (C.c_int * n)(*[f[0] for f in filters])
        settings = (C.c_char_p * n)(*[(f[1] or "").encode() for f in filters])
        self._keep = (ids, settings)
        self.width, self.height = width, height
        self._h = self._rt.hbh_job_open(n, ids, settings, pix_fmt, width, height, vrate[0], vrate[1], int(use_hip))
        if not self._h:
            raise RuntimeError(f"job init failed: {filters}")
        self.eof = False

    def push_subtitle(self, overlay, start: int, stop: int = -1, window=None):
        """A decoded bitmap subtitle for the job's burn-in track: overlay = (x, y, (Y, Cb, Cr, A) uint8 4:4:4 planes), shown
        from start to stop (90 kHz; -1: until the next one) on a canvas of `window` = (w, h) (default: the frame)."""
        arr, keep = overlay_array([overlay])
        self._rt.hbh_chain_push_subtitle.restype = C.c_int
        self._rt.hbh_chain_push_subtitle.argtypes = [C.c_void_p, C.POINTER(Overlay), C.c_int64, C.c_int64, C.c_int, C.c_int]
        ww, wh = window if window else (self.width, self.height)
        if self._rt.hbh_chain_push_subtitle(self._h, arr, start, stop, ww, wh) != 0:
            raise RuntimeError("hbh_chain_push_subtitle failed (no burn-in track on this job?)")

    def job_ptr(self):
        """address of the job's hb_job_t (what the drop-ins see as init->job)"""
        self._rt.hbh_chain_job.restype = C.c_void_p
        self._rt.hbh_chain_job.argtypes = [C.c_void_p]
        return self._rt.hbh_chain_job(self._h)

    def stages(self):
        buf = C.create_string_buffer(2048)
        self._rt.hbh_chain_describe(self._h, buf, 2048)
        return [s for s in buf.value.decode().split("|") if s]


def run_job(filters, frames, flags: int = 0x10, pix_fmt: int = AV_PIX_FMT_YUV420P, duration: int = 3003, combed=None,
            use_hip: bool = True):
    """run_stream for a Job; returns (stage names, OutFrames)."""
    h, w = frames[0][0].shape
    out = []
    with Job(filters, w, h, pix_fmt, use_hip=use_hip) as ch:
        names = ch.stages()
        for i, fr in enumerate(frames):
            ch.push(fr, start=i * duration, stop=(i + 1) * duration, flags=flags,
                    combed=0 if combed is None else combed[i])
            out += ch.drain()
        ch.push_eof()
        out += ch.drain()
    return names, out


class Preview(Job):
    """A preview's filters built the way hb_get_preview builds them, with the hook of INTEGRATION.md 2b (hbh_preview_open): the
    job's filters by id, the display rescale for `par`, `format=<pix_fmt>`; yuv420p frames in."""

    def __init__(self, filters, width: int, height: int, par=(1, 1), pix_fmt="bgra", rescale: bool = True, use_hip: bool = True):
        rt = self._rt = runtime()
        rt.hbh_preview_open.restype = C.c_void_p
        rt.hbh_preview_open.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_char_p)] + [C.c_int] * 5 + [C.c_char_p, C.c_int]
        rt.hbh_chain_stage.restype = C.c_void_p
        rt.hbh_chain_stage.argtypes = [C.c_void_p, C.c_int]
        n = len(filters)
        ids = (C.c_int * max(n, 1))(*[f[0] for f in filters])
        settings = (C.c_char_p * max(n, 1))(*[(f[1] or "").encode() for f in filters])
        self._keep = (ids, settings)
        self.width, self.height = width, height
        self._h = rt.hbh_preview_open(n, ids, settings, width, height, par[0], par[1], int(rescale),
                                      pix_fmt.encode() if pix_fmt else None, int(use_hip))
        if not self._h:
            raise RuntimeError(f"preview init failed: {filters}")
        self.eof = False

    def entries(self):
        """the list as initialised: [(name, {settings})]"""
        out, i = [], 0
        while True:
            p = self._rt.hbh_chain_stage(self._h, i)
            if not p:
                return out
            f = _FilterObject.from_address(p)
            settings, d = {}, f.settings
            e = C.cast(d, C.POINTER(C.c_void_p))[0] if d else None            # hbhip_dict_s { kv *head, *tail }
            while e:
                k, v, e = C.cast(e, C.POINTER(C.c_void_p))[0:3]                # kv_s { char *k, *v; kv *next }
                settings[C.cast(k, C.c_char_p).value.decode()] = C.cast(v, C.c_char_p).value.decode()
            out.append((f.name.decode(), settings))
            i += 1


def preview_run(filters, planes, par=(1, 1), pix_fmt="bgra", rescale: bool = True, use_hip: bool = True, run: bool = True):
    """One yuv420p picture (Y, Cb, Cr) through a preview's list; returns ([(name, {settings})] of the list as initialised,
    the picture that comes out - (height, width, 4) uint8 for a packed RGB format, else the planes - or None when not `run`)."""
    h, w = planes[0].shape
    with Preview(filters, w, h, par, pix_fmt, rescale, use_hip) as pv:
        entries = pv.entries()
        if not run:
            return entries, None
        pv.push(planes)
        pv.push_eof()
        out = pv.drain()
    if len(out) != 1:
        raise RuntimeError(f"preview: {len(out)} pictures came out of {entries}")
    got = out[0].planes
    if len(got) == 1 and got[0].shape[1] == 4 * out[0].width:
        return entries, np.ascontiguousarray(got[0]).reshape(out[0].height, out[0].width, 4)
    return entries, got


class _FilterObject(C.Structure):
    """hb_filter_object_t (include/hbhip_libhb.h; tests/golden/filter_object_layout.txt pins the offsets)"""
    _fields_ = [("id", C.c_int), ("enforce_order", C.c_int), ("skip", C.c_int), ("aliased", C.c_int),
                ("name", C.c_char_p), ("short_name", C.c_char_p), ("settings", C.c_void_p),
                ("init", C.c_void_p), ("init_thread", C.c_void_p), ("post_init", C.c_void_p), ("work", C.c_void_p),
                ("work_thread", C.c_void_p), ("close", C.c_void_p), ("info", C.c_void_p),
                ("settings_template", C.c_char_p), ("fifo_in", C.c_void_p), ("fifo_out", C.c_void_p),
                ("subtitle", C.c_void_p), ("private_data", C.c_void_p), ("thread", C.c_void_p), ("done", C.c_void_p),
                ("status", C.c_int), ("chapter_val", C.c_int), ("chapter_time", C.c_int64), ("sub_filter", C.c_void_p)]


class _Job(C.Structure):
    """hb_job_t, the stand-in's fields (include/hbhip_libhb.h)"""
    _fields_ = [("list_filter", C.c_void_p), ("hw_pix_fmt", C.c_int), ("input_pix_fmt", C.c_int),
                ("hw_device_index", C.c_int), ("h", C.c_void_p), ("done", C.c_int), ("crop", C.c_int * 4),
                ("title", C.c_void_p), ("list_subtitle", C.c_void_p), ("list_attachment", C.c_void_p),
                ("vcodec", C.c_int), ("hw_decode", C.c_int)]


class _Init(C.Structure):
    """hb_filter_init_t as far as a source fills it in (hb_harness.c:source_init); the tail is room for the rest"""
    _fields_ = [("job", C.c_void_p), ("pix_fmt", C.c_int), ("hw_pix_fmt", C.c_int), ("hw_frames_ctx", C.c_void_p),
                ("color", C.c_int * 4), ("chroma_location", C.c_int), ("geometry", C.c_int * 4), ("crop", C.c_int * 4),
                ("grayscale", C.c_int), ("vrate", C.c_int * 2), ("cfr", C.c_int), ("time_base", C.c_int * 2),
                ("tail", C.c_int * 32)]


_INIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
_CLOSE_FN = C.CFUNCTYPE(None, C.c_void_p)


def filter_stub(filter_id: int, name: str, init_result: int = 0):
    """A registered (CPU) filter of the given id that does nothing: its init() answers init_result.  For list tests that
    never push a frame.  Returns (address for register_filters' table, what must stay alive)."""
    fn = _INIT_FN(lambda f, init: init_result)
    obj = _FilterObject()
    obj.id, obj.enforce_order = filter_id, 1
    obj.name = obj.short_name = name.encode()
    obj.init = C.cast(fn, C.c_void_p)
    return C.addressof(obj), (obj, fn)


class JobList:
    """A job's filter list WITHOUT a chain around it - what do_job() has before it starts its threads: built from the
    registered objects by id (hb_filter_init + hb_add_filter_dict), handed to hb_hip_setup_hw_filters (setup()), and
    initialised the way work.c:1820-1870 / hbh_job_open do it, with hb_hip_filter_init_failed as the fallback
    (init_all()).  entries() says what the list holds at any point: [(name, {settings})]."""

    def __init__(self, filters, width: int, height: int, pix_fmt: int = AV_PIX_FMT_YUV420P):
        from . import hip
        rt = self._rt = runtime()
        self._flt = hip.filters()
        for fn, res, args in (("hb_list_init", C.c_void_p, []), ("hb_list_count", C.c_int, [C.c_void_p]),
                              ("hb_list_item", C.c_void_p, [C.c_void_p, C.c_int]), ("hb_list_rem", None, [C.c_void_p, C.c_void_p]),
                              ("hb_list_close", None, [C.POINTER(C.c_void_p)]), ("hb_filter_init", C.c_void_p, [C.c_int]),
                              ("hb_filter_close", None, [C.POINTER(C.c_void_p)]),
                              ("hb_add_filter_dict", None, [C.c_void_p, C.c_void_p, C.c_void_p]),
                              ("hbhip_dict_from_string", C.c_void_p, [C.c_char_p]), ("hb_dict_free", None, [C.POINTER(C.c_void_p)])):
            getattr(rt, fn).restype, getattr(rt, fn).argtypes = res, args
        self._flt.hb_hip_setup_hw_filters.restype, self._flt.hb_hip_setup_hw_filters.argtypes = None, [C.c_void_p]
        self._flt.hb_hip_filter_init_failed.restype = C.c_int
        self._flt.hb_hip_filter_init_failed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.job = _Job()
        self.job.hw_pix_fmt, self.job.input_pix_fmt, self.job.hw_device_index = -1, pix_fmt, -1
        self.job.list_filter = rt.hb_list_init()
        for fid, settings in filters:
            f = rt.hb_filter_init(fid)
            if not f:
                raise RuntimeError(f"no filter registered for id {fid}")
            d = C.c_void_p(rt.hbhip_dict_from_string((settings or "").encode()))
            rt.hb_add_filter_dict(self.job.list_filter, f, d)
            rt.hb_dict_free(C.byref(d))
        self.init = _Init()
        self.init.job = C.addressof(self.job)
        self.init.pix_fmt, self.init.hw_pix_fmt, self.init.chroma_location = pix_fmt, -1, _source_chroma_location
        self.init.color[:] = [1, 1, 1, 1]
        self.init.geometry[:] = [width, height, 1, 1]
        self.init.vrate[:] = [30000, 1001]
        self.init.time_base[:] = [1, 90000]

    def _items(self):
        n = self._rt.hb_list_count(self.job.list_filter)
        return [self._rt.hb_list_item(self.job.list_filter, i) for i in range(n)]

    def entries(self):
        out = []
        for p in self._items():
            f = _FilterObject.from_address(p)
            settings, d = {}, f.settings
            e = C.cast(d, C.POINTER(C.c_void_p))[0] if d else None            # hbhip_dict_s { kv *head, *tail }
            while e:
                k, v, e = C.cast(e, C.POINTER(C.c_void_p))[0:3]                # kv_s { char *k, *v; kv *next }
                settings[C.cast(k, C.c_char_p).value.decode()] = C.cast(v, C.c_char_p).value.decode()
            out.append((f.name.decode(), settings))
        return out

    def setup(self):
        self._flt.hb_hip_setup_hw_filters(C.byref(self.job))
        return self.entries()

    def init_all(self):
        rt, i = self._rt, 0
        while i < rt.hb_list_count(self.job.list_filter):
            p = rt.hb_list_item(self.job.list_filter, i)
            f = _FilterObject.from_address(p)
            f.private_data = None
            if f.init and _INIT_FN(f.init)(p, C.addressof(self.init)):
                back = self._flt.hb_hip_filter_init_failed(C.byref(self.job), i, C.byref(self.init))
                if back > 0:
                    i -= back - 1
                    continue
                rt.hb_list_rem(self.job.list_filter, p)
                rt.hb_filter_close(C.byref(C.c_void_p(p)))
                continue
            i += 1
        return self.entries()

    def close(self):
        if not self.job.list_filter:
            return
        for p in self._items():
            f = _FilterObject.from_address(p)
            if f.private_data and f.close:
                _CLOSE_FN(f.close)(p)
            self._rt.hb_list_rem(self.job.list_filter, p)
            self._rt.hb_filter_close(C.byref(C.c_void_p(p)))
        lst = C.c_void_p(self.job.list_filter)
        self._rt.hb_list_close(C.byref(lst))
        self.job.list_filter = None


def set_job_device(index: int = -1):
    """job->hw_device_index (common.h:991) of jobs opened from now on: the GPU their drop-ins run on; -1 = not set."""
    rt = runtime()
    rt.hbh_set_job_device.argtypes = [C.c_int]
    rt.hbh_set_job_device.restype = None
    rt.hbh_set_job_device(index)


SUBSOURCE = {"vobsub": 0, "pgs": 6, "dvb": 9}          # enum subsource, handbrake/common.h:1286-1298


def set_job_subtitle(source=None):
    """Jobs opened from now on carry one subtitle track of this source ("pgs", "vobsub", "dvb") marked for burn-in - what
    rendersub.c's init looks for in job->list_subtitle (:1199-1209); None = no track."""
    rt = runtime()
    rt.hbh_set_job_subtitle.argtypes = [C.c_int]
    rt.hbh_set_job_subtitle.restype = None
    rt.hbh_set_job_subtitle(-1 if source is None else SUBSOURCE[source])


def set_threaded(on: bool):
    """Chains / jobs opened from now on run one thread per filter, as libhb's filter_loop does."""
    rt = runtime()
    rt.hbh_set_threaded.argtypes = [C.c_int]
    rt.hbh_set_threaded.restype = None
    rt.hbh_set_threaded(int(on))


def set_discard_output(on: bool):
    """Threaded chains opened from now on drop (and count) the frames their last stage makes: Chain.produced()."""
    rt = runtime()
    rt.hbh_set_discard_output.argtypes = [C.c_int]
    rt.hbh_set_discard_output.restype = None
    rt.hbh_set_discard_output(int(on))


def set_source_color(prim: int = 1, transfer: int = 1, matrix: int = 1, color_range: int = 1):
    """Colour description (init->color_*) of the source of chains opened from now on."""
    rt = runtime()
    rt.hbh_set_source_color.argtypes = [C.c_int] * 4
    rt.hbh_set_source_color.restype = None
    rt.hbh_set_source_color(prim, transfer, matrix, color_range)


_source_chroma_location = 1          # AVCHROMA_LOC_LEFT


def set_source_chroma_location(chroma_location: int = 1):
    """Chroma sample location (init->chroma_location and every frame's; AVCHROMA_LOC_*: 0 unspecified, 1 left, 2 center,
    3 topleft, 4 top, 5 bottomleft, 6 bottom) of the source of chains and jobs opened from now on."""
    global _source_chroma_location
    rt = runtime()
    rt.hbh_set_source_chroma_location.argtypes = [C.c_int]
    rt.hbh_set_source_chroma_location.restype = None
    rt.hbh_set_source_chroma_location(chroma_location)
    _source_chroma_location = chroma_location


def run_stream(lib, stages, frames, flags: int = 0x10, pix_fmt: int = AV_PIX_FMT_YUV420P,
               duration: int = 3003, combed=None):
    """Push every frame then EOF; return all OutFrames in output order.
    combed: optional per-frame HB_COMB_* values stamped on the input buffers."""
    h, w = frames[0][0].shape
    out = []
    with Chain(lib, stages, w, h, pix_fmt) as ch:
        for i, fr in enumerate(frames):
            ch.push(fr, start=i * duration, stop=(i + 1) * duration, flags=flags,
                    combed=0 if combed is None else combed[i])
            out += ch.drain()
        ch.push_eof()
        out += ch.drain()
    return out


# ---- compositor objects (hb_blend_object_t) -------------------------------------------------
AV_PIX_FMT_YUVA420P, AV_PIX_FMT_YUVA422P, AV_PIX_FMT_YUVA444P = 33, 78, 79


class Overlay(C.Structure):
    """One rendered subtitle bitmap (Y, Cb, Cr, alpha planes, 8-bit) placed at (x, y)."""
    _fields_ = [("plane", C.c_void_p * 4), ("stride", C.c_int * 4),
                ("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


def overlay_array(overlays):
    """overlays: list of (x, y, (Y, Cb, Cr, A) uint8 arrays).  Returns (ctypes array, keep-alive list)."""
    arr = (Overlay * max(len(overlays), 1))()
    keep = []
    for i, (x, y, planes) in enumerate(overlays):
        planes = [np.ascontiguousarray(p) for p in planes]
        keep.append(planes)
        for k, p in enumerate(planes):
            arr[i].plane[k] = p.ctypes.data
            arr[i].stride[k] = p.strides[0]
        arr[i].x, arr[i].y = x, y
        arr[i].height, arr[i].width = planes[0].shape
    return arr, keep


def blend_run(lib, symbol, frame, overlays, pix_fmt=AV_PIX_FMT_YUV420P, overlay_fmt=AV_PIX_FMT_YUVA444P,
              chroma_location=1, passes=1):
    """Run the compositor object `symbol` of `lib` (e.g. "hb_blend_hip") on a copy of `frame`."""
    rt = runtime()
    rt.hbh_blend_run.restype = C.c_int
    rt.hbh_blend_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.POINTER(Overlay), C.c_int]
    out = [np.ascontiguousarray(p).copy() for p in frame]
    h, w = out[0].shape
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    strides = (C.c_int * 3)(*[p.strides[0] for p in out])
    arr, keep = overlay_array(overlays)
    proto = C.addressof(C.c_char.in_dll(lib, symbol))
    rc = rt.hbh_blend_run(proto, pix_fmt, w, h, chroma_location, overlay_fmt, ptrs, strides, len(overlays), arr, passes)
    if rc != 0:
        raise RuntimeError(f"hbh_blend_run({symbol}) failed ({rc})")
    return tuple(out)


class AssImage(C.Structure):
    """hbhip_ass_image: one glyph image of libass's list - coverage bitmap, position, colour and transparency."""
    _fields_ = [("bitmap", C.c_void_p), ("stride", C.c_int), ("w", C.c_int), ("h", C.c_int), ("dst_x", C.c_int),
                ("dst_y", C.c_int), ("y", C.c_uint8), ("cb", C.c_uint8), ("cr", C.c_uint8), ("a", C.c_uint8)]


def ass_image_array(images):
    """images: list of (bitmap, w, dst_x, dst_y, (y, cb, cr, a)) - bitmap a 2-D uint8 array whose row pitch is the stride
    and whose first w columns are the image (w = 0: an empty one).  Returns (ctypes array, keep-alive list)."""
    arr = (AssImage * max(len(images), 1))()
    keep = []
    for i, (bitmap, w, x, y, (cy, cb, cr, a)) in enumerate(images):
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        keep.append(bitmap)
        arr[i].bitmap = bitmap.ctypes.data
        arr[i].stride = bitmap.strides[0]
        arr[i].w, arr[i].h, arr[i].dst_x, arr[i].dst_y = w, bitmap.shape[0], x, y
        arr[i].y, arr[i].cb, arr[i].cr, arr[i].a = cy, cb, cr, a
    return arr, keep


def blend_run_ass(lib, symbol, frame, lists, crop=(0, 0, 0, 0), pix_fmt=AV_PIX_FMT_YUV420P, overlay_fmt=AV_PIX_FMT_YUVA420P,
                  chroma_location=1, dev_ctx=None, depth=8):
    """A text subtitle through the compositor object `symbol` of `lib` ("hb_blend_hip"): every list of `lists` (see
    ass_image_array) is handed to hb_blend_hip_set_ass_images in order, then work() composites the last one on a copy of
    `frame`.  crop = (top, bottom, left, right).  dev_ctx: a hip.Ctx - the frame is then a device-resident one of it."""
    rt = runtime()
    rt.hbh_blend_run_ass.restype = C.c_int
    rt.hbh_blend_run_ass.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                     C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_int)]
    out = [np.ascontiguousarray(p).copy() for p in frame]
    h, w = out[0].shape
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    strides = (C.c_int * 3)(*[p.strides[0] for p in out])
    arrs = [ass_image_array(images) for images in lists]
    counts = (C.c_int * max(len(lists), 1))(*[len(images) for images in lists])
    tables = (C.c_void_p * max(len(lists), 1))(*[C.cast(a, C.c_void_p) for a, _ in arrs])
    proto = C.addressof(C.c_char.in_dll(lib, symbol))
    setter = C.cast(lib.hb_blend_hip_set_ass_images, C.c_void_p)
    fr_in, fr_out = None, C.c_void_p()
    if dev_ctx is not None:
        from . import hip
        lch, lcw = (out[0].shape[0] // out[1].shape[0]) >> 1, (out[0].shape[1] // out[1].shape[1]) >> 1
        fr = hip.Frame(dev_ctx, w, h, depth, lcw, lch)
        fr.upload(out)
        fr_in, fr.h = fr.h, None                           # the call takes the reference over
    rc = rt.hbh_blend_run_ass(proto, setter, pix_fmt, w, h, chroma_location, overlay_fmt, ptrs, strides, fr_in,
                              C.byref(fr_out), len(lists), counts, tables, (C.c_int * 4)(*crop))
    if rc != 0:
        raise RuntimeError(f"hbh_blend_run_ass({symbol}) failed ({rc})")
    if dev_ctx is not None:
        fr.h = fr_out
        try:
            out = fr.download()
        finally:
            fr.close()
    return tuple(out)


class Bitmap(C.Structure):
    """hbh_bitmap_t: a decoded bitmap subtitle - the bitmap at (x, y) of its canvas, the canvas, its start time"""
    _fields_ = [("ov", Overlay), ("window_width", C.c_int), ("window_height", C.c_int), ("start", C.c_int64)]


def blend_run_bitmaps(lib, symbol, frame, subs, calls, crop=(0, 0, 0, 0), pix_fmt=AV_PIX_FMT_YUV420P,
                      overlay_fmt=AV_PIX_FMT_YUVA444P, chroma_location=1, dev_ctx=None, depth=8):
    """Bitmap subtitles through the compositor object `symbol` of `lib` ("hb_blend_hip").  subs: the track's decoded
    subtitles, (x, y, (Y, Cb, Cr, A), (window_width, window_height), start); calls: for each call of
    hb_blend_hip_set_bitmaps, in order, the indices into `subs` it lists.  Then work() composites the last list on a copy of
    `frame`.  crop = (top, bottom, left, right).  dev_ctx: a hip.Ctx - the frame is then a device-resident one of it."""
    rt = runtime()
    rt.hbh_blend_run_bitmaps.restype = C.c_int
    rt.hbh_blend_run_bitmaps.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                         C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(Bitmap), C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_int)), C.POINTER(C.c_int)]
    out = [np.ascontiguousarray(p).copy() for p in frame]
    h, w = out[0].shape
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    strides = (C.c_int * 3)(*[p.strides[0] for p in out])
    ovs, keep = overlay_array([(x, y, planes) for x, y, planes, _, _ in subs])
    arr = (Bitmap * max(len(subs), 1))()
    for i, (_, _, _, window, start) in enumerate(subs):
        arr[i].ov = ovs[i]
        arr[i].window_width, arr[i].window_height = window
        arr[i].start = start
    idx = [(C.c_int * max(len(c), 1))(*c) for c in calls]
    counts = (C.c_int * max(len(calls), 1))(*[len(c) for c in calls])
    tables = (C.POINTER(C.c_int) * max(len(calls), 1))(*[C.cast(a, C.POINTER(C.c_int)) for a in idx])
    proto = C.addressof(C.c_char.in_dll(lib, symbol))
    setter = C.cast(lib.hb_blend_hip_set_bitmaps, C.c_void_p)
    fr_in, fr_out = None, C.c_void_p()
    if dev_ctx is not None:
        from . import hip
        lch, lcw = (out[0].shape[0] // out[1].shape[0]) >> 1, (out[0].shape[1] // out[1].shape[1]) >> 1
        fr = hip.Frame(dev_ctx, w, h, depth, lcw, lch)
        fr.upload(out)
        fr_in, fr.h = fr.h, None                           # the call takes the reference over
    rc = rt.hbh_blend_run_bitmaps(proto, setter, pix_fmt, w, h, chroma_location, overlay_fmt, ptrs, strides, fr_in,
                                  C.byref(fr_out), len(subs), arr, len(calls), counts, tables, (C.c_int * 4)(*crop))
    if rc != 0:
        raise RuntimeError(f"hbh_blend_run_bitmaps({symbol}) failed ({rc})")
    if dev_ctx is not None:
        fr.h = fr_out
        try:
            out = fr.download()
        finally:
            fr.close()
    return tuple(out)


def motion_metric_run(lib, symbol, luma_a, luma_b, pix_fmt=AV_PIX_FMT_YUV420P) -> float:
    """Run the metric object `symbol` of `lib` (e.g. "hb_motion_metric_hip") on two luma planes."""
    rt = runtime()
    rt.hbh_motion_metric_run.restype = C.c_int
    rt.hbh_motion_metric_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    a, b = np.ascontiguousarray(luma_a), np.ascontiguousarray(luma_b)
    h, w = a.shape
    out = C.c_float()
    proto = C.addressof(C.c_char.in_dll(lib, symbol))
    rc = rt.hbh_motion_metric_run(proto, pix_fmt, w, h, a.ctypes.data, a.strides[0], b.ctypes.data, b.strides[0], C.byref(out))
    if rc != 0:
        raise RuntimeError(f"hbh_motion_metric_run({symbol}) failed ({rc})")
    return out.value


def scan_run(lib, planes, flags: int = 0, open_size=None, frame=None, surface=None, pix_fmt=None):
    """One preview through the title scan's helper of `lib` (hb_hip_scan_open / _picture / _close, libhb/scan_hip.c), the
    way scan.c:972-1052 would use it.  planes: the (Y, Cb, Cr) host picture; frame / surface: a hip.Frame / hip.Surface in
    its place - the buffer takes the object's reference over - with planes giving the size only.  open_size: the (width,
    height) the helper is opened for, the picture's by default.  Returns (rc, (combed, top, bottom, left, right, recorded)):
    rc 0, 1 when open declined, 2 when picture did."""
    rt = runtime()
    rt.hbh_scan_run.restype = C.c_int
    rt.hbh_scan_run.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p,
                                C.c_int, C.c_int, C.POINTER(C.c_int)]
    planes = [np.ascontiguousarray(p) for p in planes]
    h, w = planes[0].shape
    ow, oh = open_size if open_size is not None else (w, h)
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    strides = (C.c_int * 3)(*[p.strides[0] for p in planes])
    storage, kind = None, 0
    if frame is not None:
        storage, kind, frame.h = frame.h, 1, None
    elif surface is not None:
        storage, kind, surface.h = surface.h, 2, None
    if pix_fmt is None:
        pix_fmt = AV_PIX_FMT_NV12 if kind == 2 else AV_PIX_FMT_YUV420P
    fns = [C.cast(getattr(lib, n), C.c_void_p) for n in ("hb_hip_scan_open", "hb_hip_scan_picture", "hb_hip_scan_close")]
    out = (C.c_int * 6)()
    rc = rt.hbh_scan_run(*fns, pix_fmt, ow, oh, w, h, ptrs, strides, storage, kind, flags, out)
    if rc < 0:
        raise RuntimeError(f"hbh_scan_run failed ({rc})")
    return rc, tuple(out)


def scan_preview_run(lib, planes, flags: int = 0, open_size=None, frame=None, surface=None, pix_fmt=None, cap=1 << 24):
    """scan_run through hb_hip_scan_picture_preview: the analysis and the preview's JPEG of one picture, the way scan.c would
    use the helper when store_previews is set.  Returns (rc, (combed, top, bottom, left, right, recorded), file or None,
    whether the helper left a buffer behind)."""
    rt = runtime()
    rt.hbh_scan_preview_run.restype = C.c_int
    rt.hbh_scan_preview_run.argtypes = [C.c_void_p] * 3 + [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p,
                                        C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_int)]
    planes = [np.ascontiguousarray(p) for p in planes]
    h, w = planes[0].shape
    ow, oh = open_size if open_size is not None else (w, h)
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    strides = (C.c_int * 3)(*[p.strides[0] for p in planes])
    storage, kind = None, 0
    if frame is not None:
        storage, kind, frame.h = frame.h, 1, None
    elif surface is not None:
        storage, kind, surface.h = surface.h, 2, None
    if pix_fmt is None:
        pix_fmt = AV_PIX_FMT_NV12 if kind == 2 else AV_PIX_FMT_YUV420P
    fns = [C.cast(getattr(lib, n), C.c_void_p) for n in ("hb_hip_scan_open", "hb_hip_scan_picture_preview", "hb_hip_scan_close")]
    out = (C.c_int * 6)()
    buf = (C.c_uint8 * cap)()
    size, left = C.c_size_t(), C.c_int()
    rc = rt.hbh_scan_preview_run(*fns, pix_fmt, ow, oh, w, h, ptrs, strides, storage, kind, flags, out, buf, cap, C.byref(size),
                                 C.byref(left))
    if rc < 0:
        raise RuntimeError(f"hbh_scan_preview_run failed ({rc})")
    data = bytes(memoryview(buf)[:size.value]) if rc == 0 and size.value <= cap else None
    return rc, tuple(out), data, bool(left.value)
