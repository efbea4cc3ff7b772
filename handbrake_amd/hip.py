"""ctypes binding of the product C ABI (include/hbhip.h -> libhbhip.so) and of
the HIP filter objects (libhbhip_filters.so).  Fails loudly when the native
libraries are missing - there is no Python/CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

from . import hbrt

_HERE = os.path.dirname(os.path.abspath(__file__))

HBHIP_OK, HBHIP_AGAIN = 0, 1

#: every entry point include/hbhip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "hbhip_host_alloc", "hbhip_host_free", "hbhip_mem_live",
    "hbhip_abi_version", "hbhip_device_count", "hbhip_strerror", "hbhip_ctx_create",
    "hbhip_ctx_create_on_stream", "hbhip_ctx_destroy", "hbhip_ctx_sync", "hbhip_ctx_last_error",
    "hbhip_debug_mask_chain", "hbhip_cropscale_sws_create", "hbhip_ctx_copy_bandwidth", "hbhip_ctx_device_name", "hbhip_ctx_device_index", "hbhip_frame_context", "hbhip_filter_context",
    "hbhip_ctx_profile_enable", "hbhip_ctx_profile_reset",
    "hbhip_ctx_profile_count", "hbhip_ctx_profile_get", "hbhip_ctx_mark", "hbhip_ctx_elapsed_ms",
    "hbhip_dev_alloc", "hbhip_dev_free", "hbhip_dev_upload", "hbhip_dev_download",
    "hbhip_frame_alloc", "hbhip_frame_retain", "hbhip_frame_release", "hbhip_frame_refs", "hbhip_frame_use_on", "hbhip_frame_describe", "hbhip_frame_copy",
    "hbhip_frame_upload", "hbhip_frame_upload_async", "hbhip_ctx_upload_done", "hbhip_frame_download", "hbhip_frame_mark_ready", "hbhip_frame_download_async", "hbhip_frame_download_wait",
    "hbhip_frame_upload_biplanar", "hbhip_frame_download_biplanar", "hbhip_frame_upload_biplanar_async", "hbhip_frame_download_biplanar_async",
    "hbhip_surface_alloc", "hbhip_surface_wrap", "hbhip_surface_retain", "hbhip_surface_release", "hbhip_surface_describe", "hbhip_surface_set_ready_event",
    "hbhip_frame_import_surface", "hbhip_frame_import_surface_async", "hbhip_frame_export_surface", "hbhip_frame_export_surface_async", "hbhip_ctx_bus_bytes",
    "hbhip_frame_download_widen", "hbhip_frame_download_widen_async", "hbhip_frame_export_surface_widen", "hbhip_frame_export_surface_widen_async",
    "hbhip_frame_download_rgb32", "hbhip_frame_download_rgb32_async",
    "hbhip_filter_use_frames", "hbhip_filter_push_frame", "hbhip_filter_pull_frame", "hbhip_filter_push", "hbhip_filter_push_dev", "hbhip_filter_pull", "hbhip_filter_pull_dev",
    "hbhip_filter_process_dev", "hbhip_filter_submit_async", "hbhip_filter_wait", "hbhip_filter_inflight", "hbhip_filter_flush", "hbhip_filter_pending", "hbhip_filter_defer", "hbhip_filter_kick", "hbhip_filter_destroy",
    "hbhip_filter_out_geometry",
    "hbhip_chain_create", "hbhip_chain_process_dev", "hbhip_chain_flush_dev", "hbhip_chain_pending", "hbhip_chain_sync", "hbhip_chain_destroy",
    "hbhip_nlmeans_create", "hbhip_nlmeans_set_batch", "hbhip_nlmeans_plan", "hbhip_nlmeans_forms",
    "hbhip_lapsharp_create", "hbhip_unsharp_create", "hbhip_chroma_smooth_create",
    "hbhip_hqdn3d_create", "hbhip_decomb_create", "hbhip_decomb_push", "hbhip_decomb_push_dev", "hbhip_decomb_push_frame", "hbhip_decomb_debug_eedi_plane",
    "hbhip_comb_detect_create", "hbhip_comb_detect_set_gamma_lut", "hbhip_comb_detect_store",
    "hbhip_comb_detect_store_dev",
    "hbhip_comb_detect_classify", "hbhip_comb_detect_classify_many_dev", "hbhip_comb_detect_overlay", "hbhip_comb_detect_overlay_dev",
    "hbhip_comb_detect_debug_mask",
    "hbhip_rotate_create", "hbhip_grayscale_create", "hbhip_cropscale_create", "hbhip_cropscale_create_sited", "hbhip_colorspace_create", "hbhip_colorspace_create_sited", "hbhip_pad_create", "hbhip_yadif_create", "hbhip_bwdif_create", "hbhip_format_create", "hbhip_format_resample_create", "hbhip_format_scaled_create", "hbhip_format_upsample_create", "hbhip_format_deepen_create",
    "hbhip_blend_create", "hbhip_blend_set_overlays", "hbhip_blend_apply", "hbhip_blend_apply_dev", "hbhip_blend_destroy",
    "hbhip_blend_create_biplanar", "hbhip_blend_apply_biplanar",
    "hbhip_blend_set_ass_images", "hbhip_blend_debug_overlay_count", "hbhip_blend_debug_get_overlay",
    "hbhip_blend_set_bitmaps", "hbhip_blend_debug_bitmap_stats",
    "hbhip_motion_metric_create", "hbhip_motion_metric_run", "hbhip_motion_metric_run_dev", "hbhip_motion_metric_destroy",
    "hbhip_detelecine_create", "hbhip_detelecine_push", "hbhip_detelecine_push_frame",
    "hbhip_deblock_create", "hbhip_deblock_set_warmup",
    "hbhip_deband_create", "hbhip_deband_offsets", "hbhip_deband_set_kernel",
    "hbhip_bm3d_params_from_settings", "hbhip_bm3d_create",
    "hbhip_scan_create", "hbhip_scan_destroy", "hbhip_scan_push", "hbhip_scan_pull", "hbhip_scan_inflight",
    "hbhip_jpeg_create", "hbhip_jpeg_destroy", "hbhip_jpeg_bound", "hbhip_jpeg_push", "hbhip_jpeg_pull", "hbhip_jpeg_inflight",
]


class HostFrame(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_int * 3)]


class HostBiplanar(C.Structure):
    """hbhip_host_biplanar: an NV12 / P010LE host picture (luma, interleaved Cb Cr)"""
    _fields_ = [("plane", C.c_void_p * 2), ("stride", C.c_int * 2)]


class DevFrame(C.Structure):
    _fields_ = [("plane", C.c_void_p * 3), ("stride", C.c_int * 3)]


class DevSurface(C.Structure):
    """hbhip_dev_surface: an NV12 / P010LE picture in device memory (luma, interleaved Cb Cr), a pitch per plane"""
    _fields_ = [("plane", C.c_void_p * 2), ("pitch", C.c_int * 2)]


SURFACE_RELEASE = C.CFUNCTYPE(None, C.c_void_p)


class BitmapSub(C.Structure):
    """hbhip_bitmap_sub: a decoded bitmap subtitle - the 4:4:4 YUVA bitmap, its place on its canvas, the canvas, a key"""
    _fields_ = [("plane", C.c_void_p * 4), ("stride", C.c_int * 4), ("x", C.c_int), ("y", C.c_int), ("width", C.c_int),
                ("height", C.c_int), ("window_width", C.c_int), ("window_height", C.c_int), ("key", C.c_uint64)]


class NLMeansParams(C.Structure):
    _fields_ = [("strength", C.c_double * 3), ("origin_tune", C.c_double * 3),
                ("patch_size", C.c_int * 3), ("range", C.c_int * 3),
                ("nframes", C.c_int * 3), ("prefilter", C.c_int * 3),
                ("exptable", (C.c_float * 128) * 3), ("weight_fact_table", C.c_float * 3),
                ("diff_max", C.c_int * 3)]


class NLMeansLaunch(C.Structure):
    """hbhip_nlmeans_launch: the kernel form one launch of a frame takes (hbhip_nlmeans_plan)"""
    _fields_ = [(n, C.c_int) for n in ("patch_size", "planes", "generic", "wide", "fast", "pitch", "pre", "pairs", "origin_f32",
                                       "max_rh", "cmp_rows", "job_arith", "tile_w", "tile_h")] + \
               [("lds_bytes", C.c_uint), ("diff_cap", C.c_int * 3), ("imul4", C.c_uint * 3), ("ishift", C.c_int * 3)]

    def as_dict(self):
        return {n: (getattr(self, n) if t in (C.c_int, C.c_uint) else list(getattr(self, n))) for n, t in self._fields_}


class DeblockParams(C.Structure):
    _fields_ = [("strong", C.c_int), ("block", C.c_int), ("ath", C.c_int), ("bth", C.c_int), ("gth", C.c_int), ("dth", C.c_int)]


class DebandParams(C.Structure):
    _fields_ = [("thr", C.c_int * 3), ("blur", C.c_int), ("range", C.c_int), ("direction", C.c_float)]


class Bm3dParams(C.Structure):
    _fields_ = [("sigma", C.c_float)] + [(n, C.c_int) for n in ("block", "bstep", "group", "range", "mstep")] + \
               [("thmse", C.c_float), ("hdthr", C.c_float), ("estim", C.c_int), ("planes", C.c_int),
                ("thr", C.c_float * 3), ("dct", C.c_float * 256)]


class ScanParams(C.Structure):
    """hbhip_scan_params: hb_detect_comb's six sensitivities (scan.c:973 passes 10, 30, 9, 10, 30, 9)"""
    _fields_ = [(n, C.c_int) for n in ("color_equal", "color_diff", "threshold", "prog_equal", "prog_diff", "prog_threshold")]


class ScanResult(C.Structure):
    """hbhip_scan_result: a preview's crop, whether scan.c would record it, hb_detect_comb's scores and verdict"""
    _fields_ = [(n, C.c_int) for n in ("top", "bottom", "left", "right", "recorded")] + \
               [("cc", C.c_int * 3), ("average_cc", C.c_int), ("combed", C.c_int)]

    def as_tuple(self):
        return (self.top, self.bottom, self.left, self.right, self.recorded, tuple(self.cc), self.average_cc, self.combed)


RGB32_ORDERS = ("bgra", "rgba", "argb", "abgr")      #: HBHIP_RGB32_*, by number
SCAN_INFLIGHT_MAX = 32      #: HBHIP_SCAN_INFLIGHT_MAX
SCAN_RECORD_BYTES = 48      #: HBHIP_SCAN_RECORD_BYTES: what a scanned picture sends over the bus
JPEG_INFLIGHT_MAX = 4       #: HBHIP_JPEG_INFLIGHT_MAX


_lib = None
_flt = None


def lib() -> C.CDLL:
    """libhbhip.so (HIP kernels + C ABI)."""
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "libhbhip.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: the HIP extension is not built "
                               "(run __graft_entry__.build() / make)")
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        L.hbhip_strerror.restype = C.c_char_p
        L.hbhip_strerror.argtypes = [C.c_int]
        L.hbhip_ctx_last_error.restype = C.c_char_p
        L.hbhip_ctx_last_error.argtypes = [C.c_void_p]
        L.hbhip_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.hbhip_ctx_create_on_stream.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.hbhip_ctx_destroy.argtypes = [C.c_void_p]
        L.hbhip_ctx_destroy.restype = None
        L.hbhip_ctx_sync.argtypes = [C.c_void_p]
        L.hbhip_ctx_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.hbhip_ctx_profile_enable.argtypes = [C.c_void_p, C.c_int]
        L.hbhip_ctx_profile_reset.argtypes = [C.c_void_p]
        L.hbhip_ctx_profile_count.argtypes = [C.c_void_p]
        L.hbhip_ctx_profile_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.hbhip_ctx_mark.argtypes = [C.c_void_p, C.c_int]
        L.hbhip_ctx_elapsed_ms.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.hbhip_dev_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.hbhip_dev_free.argtypes = [C.c_void_p, C.c_void_p]
        L.hbhip_dev_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.hbhip_dev_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.hbhip_filter_push.argtypes = [C.c_void_p, C.POINTER(HostFrame), C.c_int64]
        L.hbhip_filter_push_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame), C.c_int64]
        L.hbhip_filter_pull.argtypes = [C.c_void_p, C.POINTER(HostFrame), C.POINTER(C.c_int64)]
        L.hbhip_filter_pull_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame), C.POINTER(C.c_int64)]
        L.hbhip_filter_flush.argtypes = [C.c_void_p]
        L.hbhip_filter_process_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame), C.c_int, C.c_int64,
                                               C.POINTER(DevFrame), C.c_int, C.POINTER(C.c_int)]
        L.hbhip_filter_pending.argtypes = [C.c_void_p]
        L.hbhip_filter_destroy.argtypes = [C.c_void_p]
        L.hbhip_filter_destroy.restype = None
        L.hbhip_filter_out_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.hbhip_nlmeans_create.argtypes = [C.c_void_p, C.POINTER(NLMeansParams), C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.hbhip_nlmeans_set_batch.argtypes = [C.c_void_p, C.c_int]
        L.hbhip_nlmeans_plan.argtypes = [C.POINTER(NLMeansParams)] + [C.c_int] * 5 + [C.POINTER(NLMeansLaunch), C.POINTER(C.c_int)]
        L.hbhip_nlmeans_forms.argtypes = [C.POINTER(NLMeansLaunch), C.c_int]
        L.hbhip_chain_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
        L.hbhip_chain_process_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.c_int, C.c_int64, C.POINTER(DevFrame), C.POINTER(C.c_int64), C.c_int,
                                              C.POINTER(C.c_int)]
        L.hbhip_chain_flush_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int)]
        L.hbhip_chain_pending.argtypes = [C.c_void_p]
        L.hbhip_chain_sync.argtypes = [C.c_void_p]
        L.hbhip_chain_destroy.argtypes = [C.c_void_p]
        L.hbhip_chain_destroy.restype = None
        L.hbhip_frame_alloc.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)]
        for fn in ("hbhip_frame_retain", "hbhip_frame_release"):
            getattr(L, fn).argtypes = [C.c_void_p]
            getattr(L, fn).restype = None
        L.hbhip_frame_refs.argtypes = [C.c_void_p]
        L.hbhip_frame_copy.argtypes = [C.c_void_p, C.c_void_p]
        for fn in ("hbhip_frame_upload", "hbhip_frame_download"):
            getattr(L, fn).argtypes = [C.c_void_p, C.POINTER(HostFrame)]
        L.hbhip_frame_upload_async.argtypes = [C.c_void_p, C.POINTER(HostFrame), C.POINTER(C.c_void_p)]
        for fn in ("hbhip_frame_upload_biplanar", "hbhip_frame_download_biplanar", "hbhip_frame_download_widen"):
            getattr(L, fn).argtypes = [C.c_void_p, C.POINTER(HostBiplanar)]
        for fn in ("hbhip_frame_upload_biplanar_async", "hbhip_frame_download_biplanar_async", "hbhip_frame_download_widen_async"):
            getattr(L, fn).argtypes = [C.c_void_p, C.POINTER(HostBiplanar), C.POINTER(C.c_void_p)]
        L.hbhip_frame_download_rgb32.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4
        L.hbhip_frame_download_rgb32_async.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.POINTER(C.c_void_p)]
        L.hbhip_frame_download_wait.argtypes = [C.c_void_p, C.c_void_p]
        L.hbhip_ctx_upload_done.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hbhip_surface_alloc.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)]
        L.hbhip_surface_wrap.argtypes = [C.c_void_p, C.POINTER(DevSurface), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_void_p)]
        for fn in ("hbhip_surface_retain", "hbhip_surface_release"):
            getattr(L, fn).argtypes = [C.c_void_p]
            getattr(L, fn).restype = None
        L.hbhip_surface_describe.argtypes = [C.c_void_p, C.POINTER(DevSurface)] + [C.POINTER(C.c_int)] * 3
        L.hbhip_surface_set_ready_event.argtypes = [C.c_void_p, C.c_void_p]
        for fn in ("hbhip_frame_import_surface", "hbhip_frame_export_surface", "hbhip_frame_export_surface_widen"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p]
        for fn in ("hbhip_frame_import_surface_async", "hbhip_frame_export_surface_async", "hbhip_frame_export_surface_widen_async"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.hbhip_ctx_bus_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.hbhip_mem_live.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.hbhip_filter_use_frames.argtypes = [C.c_void_p]
        L.hbhip_decomb_push_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int]
        L.hbhip_bm3d_params_from_settings.argtypes = [C.c_char_p, C.c_int, C.POINTER(Bm3dParams)]
        L.hbhip_scan_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.hbhip_scan_destroy.argtypes = [C.c_void_p]
        L.hbhip_scan_destroy.restype = None
        L.hbhip_scan_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(ScanParams)]
        L.hbhip_scan_pull.argtypes = [C.c_void_p, C.POINTER(ScanResult)]
        L.hbhip_scan_inflight.argtypes = [C.c_void_p]
        L.hbhip_jpeg_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.hbhip_jpeg_destroy.argtypes = [C.c_void_p]
        L.hbhip_jpeg_destroy.restype = None
        L.hbhip_jpeg_bound.argtypes = [C.c_void_p]
        L.hbhip_jpeg_bound.restype = C.c_size_t
        L.hbhip_jpeg_push.argtypes = [C.c_void_p, C.c_void_p]
        L.hbhip_jpeg_pull.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.hbhip_jpeg_inflight.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def filters() -> C.CDLL:
    """libhbhip_filters.so: the hb_filter_object_t drop-ins (hb_filter_*_hip)."""
    global _flt
    if _flt is None:
        hbrt.runtime()
        lib()
        path = os.path.join(_HERE, "libhbhip_filters.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run __graft_entry__.build() / make")
        F = C.CDLL(path, mode=C.RTLD_GLOBAL)
        F.hbhip_host_ctx_ptr.restype = C.c_void_p
        F.hbhip_filter_get.restype = C.c_void_p
        F.hbhip_filter_get.argtypes = [C.c_int]
        F.hbhip_nlmeans_params_from_settings.restype = None
        F.hbhip_nlmeans_params_from_settings.argtypes = [C.c_char_p, C.c_int, C.POINTER(NLMeansParams)]
        _flt = F
    return _flt


class HipError(RuntimeError):
    pass


def check(rc: int, ctx=None, what: str = ""):
    if rc < 0:
        msg = lib().hbhip_strerror(rc).decode()
        if ctx:
            msg += " | " + lib().hbhip_ctx_last_error(ctx).decode()
        raise HipError(f"{what}: {msg}")
    return rc


def mem_live():
    """(device, pinned) bytes the library holds right now, process-wide (hbhip_mem_live)"""
    dev, pin = C.c_size_t(), C.c_size_t()
    check(lib().hbhip_mem_live(C.byref(dev), C.byref(pin)), what="mem_live")
    return dev.value, pin.value


class Ctx:
    """A device context (one GPU, one stream)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        L = lib()
        h = C.c_void_p()
        if stream is None:
            check(L.hbhip_ctx_create(device, C.byref(h)), what="hbhip_ctx_create")
        else:
            check(L.hbhip_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)),
                  what="hbhip_ctx_create_on_stream")
        self.h = h

    def sync(self):
        check(lib().hbhip_ctx_sync(self.h), self.h, "sync")

    def name(self) -> str:
        buf = C.create_string_buffer(256)
        lib().hbhip_ctx_device_name(self.h, buf, 256)
        return buf.value.decode()

    def profile(self, on: bool):
        check(lib().hbhip_ctx_profile_enable(self.h, int(on)), self.h)

    def profile_reset(self):
        check(lib().hbhip_ctx_profile_reset(self.h), self.h)

    def profile_stats(self) -> dict:
        L = lib()
        out = {}
        for i in range(L.hbhip_ctx_profile_count(self.h)):
            name = C.create_string_buffer(128)
            n = C.c_int64()
            ms = C.c_double()
            L.hbhip_ctx_profile_get(self.h, i, name, 128, C.byref(n), C.byref(ms))
            out[name.value.decode()] = (n.value, ms.value)
        return out

    def mark(self, slot: int):
        check(lib().hbhip_ctx_mark(self.h, slot), self.h, "mark")

    def elapsed_ms(self, a: int, b: int) -> float:
        ms = C.c_double()
        check(lib().hbhip_ctx_elapsed_ms(self.h, a, b, C.byref(ms)), self.h, "elapsed")
        return ms.value

    def bus_bytes(self):
        """(H2D, D2H) bytes the frame upload / download entry points have queued over the bus on this context"""
        up, down = C.c_uint64(), C.c_uint64()
        check(lib().hbhip_ctx_bus_bytes(self.h, C.byref(up), C.byref(down)), self.h, "bus_bytes")
        return up.value, down.value

    def close(self):
        if self.h:
            lib().hbhip_ctx_destroy(self.h)
            self.h = None


def dev_frame(tensors) -> DevFrame:
    """DevFrame over three 2-D torch CUDA tensors (kept alive by the caller): uint8 planes, or int16 ones for 10 / 12-bit
    samples; the stride is taken in bytes."""
    f = DevFrame()
    for i, t in enumerate(tensors):
        f.plane[i] = t.data_ptr()
        f.stride[i] = t.stride(0) * t.element_size()
    return f


class Frame:
    """A device-resident frame (hbhip_frame_*) from a context's pool, holding one reference until close()."""

    def __init__(self, ctx: Ctx, width, height, depth=8, lcw=1, lch=1):
        h = C.c_void_p()
        check(lib().hbhip_frame_alloc(ctx.h, width, height, depth, lcw, lch, C.byref(h)), ctx.h, "frame_alloc")
        self.ctx, self.h, self.shape = ctx, h, (width, height, depth, lcw, lch)

    def planes(self):
        """zeroed host planes of the frame's geometry"""
        import numpy as np
        w, h, depth, lcw, lch = self.shape
        dt = np.uint8 if depth == 8 else np.uint16
        return [np.zeros((h, w), dt), np.zeros((-(-h >> lch), -(-w >> lcw)), dt), np.zeros((-(-h >> lch), -(-w >> lcw)), dt)]

    def upload(self, planes):
        check(lib().hbhip_frame_upload(self.h, C.byref(host_frame(planes))), self.ctx.h, "frame_upload")

    def upload_async(self, planes):
        """queued on the upload stream; `planes` must stay alive until upload_done(token) has returned"""
        token = C.c_void_p()
        check(lib().hbhip_frame_upload_async(self.h, C.byref(host_frame(planes)), C.byref(token)), self.ctx.h, "frame_upload_async")
        return token

    def upload_done(self, token):
        check(lib().hbhip_ctx_upload_done(self.ctx.h, token, 1), self.ctx.h, "upload_done")

    def download(self):
        out = self.planes()
        check(lib().hbhip_frame_download(self.h, C.byref(host_frame(out))), self.ctx.h, "frame_download")
        return out

    def download_rgb32(self, order="bgra", matrix=1, full_range=False):
        """the 8-bit 4:2:0 frame as a packed 32-bit RGB picture, (height, width, 4) uint8 in memory order"""
        import numpy as np
        w, h = self.shape[:2]
        out = np.zeros((h, w, 4), np.uint8)
        check(lib().hbhip_frame_download_rgb32(self.h, out.ctypes.data, 4 * w, RGB32_ORDERS.index(order), matrix, int(full_range)),
              self.ctx.h, "frame_download_rgb32")
        return out

    def import_surface(self, surface: "Surface"):
        check(lib().hbhip_frame_import_surface(self.h, surface.h), self.ctx.h, "frame_import_surface")

    def export_surface(self, surface: "Surface"):
        check(lib().hbhip_frame_export_surface(self.h, surface.h), self.ctx.h, "frame_export_surface")

    def export_surface_widen(self, surface: "Surface"):
        """an 8-bit 4:2:0 frame into a depth-10 surface, every sample t as t | t << 8"""
        check(lib().hbhip_frame_export_surface_widen(self.h, surface.h), self.ctx.h, "frame_export_surface_widen")

    def copy_from(self, src: "Frame"):
        check(lib().hbhip_frame_copy(self.h, src.h), self.ctx.h, "frame_copy")

    def refs(self) -> int:
        return lib().hbhip_frame_refs(self.h)

    def retain(self):
        lib().hbhip_frame_retain(self.h)

    def release(self):
        lib().hbhip_frame_release(self.h)

    def close(self):
        if self.h:
            self.release()
            self.h = None


class Surface:
    """An NV12 / P010LE picture in device memory (hbhip_surface_*), holding one reference until close()."""

    def __init__(self, ctx: Ctx, width, height, depth=8, pitch_align=256, rows_align=16):
        h = C.c_void_p()
        check(lib().hbhip_surface_alloc(ctx.h, width, height, depth, pitch_align, rows_align, C.byref(h)), ctx.h, "surface_alloc")
        self.h = h

    @classmethod
    def adopt(cls, handle):
        """around an hbhip_surface* whose reference becomes the object's"""
        s = cls.__new__(cls)
        s.h = handle
        return s

    @classmethod
    def wrap(cls, ctx: Ctx, planes, pitches, width, height, depth=8, release=None, opaque=None):
        """caller-owned device memory: planes = two device addresses; release: a SURFACE_RELEASE the caller keeps alive"""
        mem = DevSurface((C.c_void_p * 2)(*planes), (C.c_int * 2)(*pitches))
        h = C.c_void_p()
        fn = C.cast(release, C.c_void_p) if release is not None else None
        check(lib().hbhip_surface_wrap(ctx.h, C.byref(mem), width, height, depth, fn, opaque, C.byref(h)), ctx.h, "surface_wrap")
        return cls.adopt(h)

    def describe(self):
        """((plane addresses), (pitches), width, height, depth)"""
        d = DevSurface()
        w, h, depth = C.c_int(), C.c_int(), C.c_int()
        check(lib().hbhip_surface_describe(self.h, C.byref(d), C.byref(w), C.byref(h), C.byref(depth)), what="surface_describe")
        return tuple(d.plane), tuple(d.pitch), w.value, h.value, depth.value

    def retain(self):
        lib().hbhip_surface_retain(self.h)

    def close(self):
        if self.h:
            lib().hbhip_surface_release(self.h)
            self.h = None


class ScanDevice:
    """The title scan's analysis of device pictures (hbhip_scan_*): crop and combing of 8-bit 4:2:0 previews."""

    def __init__(self, ctx: Ctx, width, height):
        h = C.c_void_p()
        check(lib().hbhip_scan_create(ctx.h, width, height, C.byref(h)), ctx.h, "scan_create")
        self.ctx, self.h = ctx, h

    def push_rc(self, frame: Frame, flags: int = 0, params=None) -> int:
        """the raw return code (the refusals are part of the interface)"""
        p = C.byref(ScanParams(*params)) if params is not None else None
        return lib().hbhip_scan_push(self.h, frame.h, flags, p)

    def push(self, frame: Frame, flags: int = 0, params=None):
        check(self.push_rc(frame, flags, params), self.ctx.h, "scan_push")

    def pull(self):
        """the oldest picture's ScanResult, or None when nothing is in flight"""
        r = ScanResult()
        rc = check(lib().hbhip_scan_pull(self.h, C.byref(r)), self.ctx.h, "scan_pull")
        return None if rc == HBHIP_AGAIN else r

    def inflight(self) -> int:
        return lib().hbhip_scan_inflight(self.h)

    def close(self):
        if self.h:
            lib().hbhip_scan_destroy(self.h)
            self.h = None


class JpegDevice:
    """A preview's JPEG from a device picture (hbhip_jpeg_*): libjpeg's file for 8-bit 4:2:0 planes at one quality."""

    def __init__(self, ctx: Ctx, width, height, quality=90):
        h = C.c_void_p()
        check(lib().hbhip_jpeg_create(ctx.h, width, height, quality, C.byref(h)), ctx.h, "jpeg_create")
        self.ctx, self.h = ctx, h

    def bound(self) -> int:
        return lib().hbhip_jpeg_bound(self.h)

    def push_rc(self, frame: Frame) -> int:
        """the raw return code (the refusals are part of the interface)"""
        return lib().hbhip_jpeg_push(self.h, frame.h)

    def push(self, frame: Frame):
        check(self.push_rc(frame), self.ctx.h, "jpeg_push")

    def pull_rc(self, cap=None):
        """(return code, the file's length, the file or None): the oldest picture's, into a buffer of `cap` bytes"""
        cap = self.bound() if cap is None else cap
        if getattr(self, "_buf", None) is None or len(self._buf) < max(cap, 1):
            self._buf = (C.c_uint8 * max(cap, 1))()                  # kept: ctypes clears it, 80 MB at 2160p
        buf = self._buf
        size = C.c_size_t()
        rc = lib().hbhip_jpeg_pull(self.h, buf, cap, C.byref(size))
        return rc, size.value, (bytes(memoryview(buf)[:size.value]) if rc == HBHIP_OK else None)

    def pull(self):
        """the oldest picture's file, or None when nothing is in flight"""
        rc, _, data = self.pull_rc()
        check(rc, self.ctx.h, "jpeg_pull")
        return None if rc == HBHIP_AGAIN else data

    def inflight(self) -> int:
        return lib().hbhip_jpeg_inflight(self.h)

    def close(self):
        if self.h:
            lib().hbhip_jpeg_destroy(self.h)
            self.h = None


class DeviceFilter:
    """Thin wrapper of an hbhip_filter* for device-resident frames (bench / tests)."""

    def __init__(self, ctx: Ctx, handle):
        self.ctx, self.h = ctx, handle

    def push_dev(self, frame: DevFrame, tag: int = 0):
        check(lib().hbhip_filter_push_dev(self.h, C.byref(frame), tag), self.ctx.h, "push_dev")

    def pull_dev(self, frame: DevFrame):
        tag = C.c_int64()
        rc = check(lib().hbhip_filter_pull_dev(self.h, C.byref(frame), C.byref(tag)), self.ctx.h, "pull_dev")
        return None if rc == HBHIP_AGAIN else tag.value

    def process_dev(self, frames_in, tag0: int, frames_out) -> int:
        """frames_in / frames_out: ctypes arrays of DevFrame.  Returns frames written."""
        n = C.c_int()
        check(lib().hbhip_filter_process_dev(self.h, frames_in, len(frames_in), tag0,
                                             frames_out, len(frames_out), C.byref(n)),
              self.ctx.h, "process_dev")
        return n.value

    def flush(self):
        check(lib().hbhip_filter_flush(self.h), self.ctx.h, "flush")

    def pending(self) -> int:
        return lib().hbhip_filter_pending(self.h)

    def close(self):
        if self.h:
            lib().hbhip_filter_destroy(self.h)
            self.h = None


class Chain:
    """hbhip_chain: a run of device filters fused into one object (frames stay in HBM between the
    stages, handed over by pointer).  `stages` = DeviceFilter objects on `ctx`, or each on a context of
    its own (then every stage runs on its own HIP stream and batches overlap; outputs are complete after
    sync()); the chain closes them itself, last stage first."""

    def __init__(self, ctx: Ctx, stages):
        self.ctx, self.stages = ctx, list(stages)
        arr = (C.c_void_p * len(self.stages))(*[s.h for s in self.stages])
        h = C.c_void_p()
        check(lib().hbhip_chain_create(ctx.h, arr, len(self.stages), C.byref(h)), ctx.h, "hbhip_chain_create")
        self.h = h

    def process_dev(self, frames_in, frames_out, tag0: int = 0, flags=None, combed=None, tags=None) -> int:
        n = C.c_int()
        nin = len(frames_in)
        fl = (C.c_int * nin)(*flags) if flags is not None else None
        cb = (C.c_int * nin)(*combed) if combed is not None else None
        check(lib().hbhip_chain_process_dev(self.h, frames_in, fl, cb, nin, tag0, frames_out, tags, len(frames_out),
                                            C.byref(n)), self.ctx.h, "chain_process_dev")
        return n.value

    def flush_dev(self, frames_out, tags=None) -> int:
        n = C.c_int()
        check(lib().hbhip_chain_flush_dev(self.h, frames_out, tags, len(frames_out), C.byref(n)), self.ctx.h, "chain_flush_dev")
        return n.value

    def sync(self):
        check(lib().hbhip_chain_sync(self.h), self.ctx.h, "chain_sync")

    def close(self):
        if self.h:
            lib().hbhip_chain_destroy(self.h)
            self.h = None
            for s in reversed(self.stages):
                s.close()


NLMEANS_MEDIUM = ("y-strength=6:y-origin-tune=1:y-patch-size=7:y-range=3:y-frame-count=2:y-prefilter=0:"
                  "cb-strength=6:cb-origin-tune=1:cb-patch-size=7:cb-range=3:cb-frame-count=2:cb-prefilter=0")


def nlmeans_plan(settings: str, width: int, height: int, depth: int = 8, log2_chroma_w: int = 1, log2_chroma_h: int = 1):
    """The launches a frame of this geometry takes under `settings`, as dicts of hbhip_nlmeans_launch's fields (no
    device needed); HipError where hbhip_nlmeans_create would decline."""
    par = NLMeansParams()
    filters().hbhip_nlmeans_params_from_settings(settings.encode(), depth, C.byref(par))
    out = (NLMeansLaunch * 3)()
    n = C.c_int(0)
    check(lib().hbhip_nlmeans_plan(C.byref(par), width, height, depth, log2_chroma_w, log2_chroma_h, out, C.byref(n)),
          None, "hbhip_nlmeans_plan")
    return [out[i].as_dict() for i in range(n.value)]


def nlmeans_forms():
    """Every kernel instantiation the NLMeans dispatcher holds (hbhip_nlmeans_forms), as dicts"""
    n = lib().hbhip_nlmeans_forms(None, 0)
    out = (NLMeansLaunch * n)()
    assert lib().hbhip_nlmeans_forms(out, n) == n
    return [out[i].as_dict() for i in range(n)]


def nlmeans_device_filter(ctx: Ctx, settings: str, width: int, height: int, batch: int = 1,
                          depth: int = 8) -> DeviceFilter:
    """An NLMeans instance driven through the C ABI with device-resident frames
    (depth 10 / 12: uint16 planes)."""
    par = NLMeansParams()
    filters().hbhip_nlmeans_params_from_settings(settings.encode(), depth, C.byref(par))
    h = C.c_void_p()
    check(lib().hbhip_nlmeans_create(ctx.h, C.byref(par), width, height, depth, 1, 1, C.byref(h)),
          ctx.h, "hbhip_nlmeans_create")
    check(lib().hbhip_nlmeans_set_batch(h, batch), ctx.h, "set_batch")
    return DeviceFilter(ctx, h)


class DecombParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("mode", "parity", "magnitude_threshold", "variance_threshold",
                                       "laplacian_threshold", "dilation_threshold", "erosion_threshold",
                                       "noise_threshold", "maximum_search_distance", "post_processing")]


def host_frame(planes) -> HostFrame:
    """HostFrame over three 2-D uint8 numpy arrays (kept alive by the caller)."""
    f = HostFrame()
    for i, a in enumerate(planes):
        f.plane[i] = a.ctypes.data
        f.stride[i] = a.strides[0]
    return f


class CombDetectParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("spatial_metric", C.c_int), ("motion_threshold", C.c_int),
                ("spatial_threshold", C.c_int), ("filter_mode", C.c_int), ("block_threshold", C.c_int),
                ("block_width", C.c_int), ("block_height", C.c_int), ("gamma_lut", C.c_float * 256)]


class CombDetectDevice:
    """Comb detection through the raw C ABI on device-resident luma planes (bench.py; the
    hb_filter_object_t path is hb_filter_comb_detect_hip).  Defaults = param.c:204-207."""

    def __init__(self, ctx: Ctx, width, height, mode=3, spatial_metric=2, motion_thresh=1, spatial_thresh=1,
                 filter_mode=2, block_thresh=40, block_width=16, block_height=16, depth=8):
        import numpy as np
        L = lib()
        L.hbhip_comb_detect_create.argtypes = [C.c_void_p, C.POINTER(CombDetectParams)] + [C.c_int] * 3 + [C.POINTER(C.c_void_p)]
        L.hbhip_comb_detect_store.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hbhip_comb_detect_store_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hbhip_comb_detect_set_gamma_lut.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hbhip_comb_detect_classify.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.hbhip_comb_detect_debug_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        par = CombDetectParams(mode, spatial_metric, motion_thresh, spatial_thresh, filter_mode, block_thresh,
                               block_width, block_height)
        # comb_detect.c:1074-1081: pow((float)i / (float)max, 2.2f), evaluated in double, stored as float
        maxv = (1 << depth) - 1
        lut = np.power((np.arange(maxv + 1, dtype=np.float32) / np.float32(maxv)).astype(np.float64),
                       np.float64(np.float32(2.2))).astype(np.float32)
        if depth == 8:
            for i in range(256):
                par.gamma_lut[i] = float(lut[i])
        h = C.c_void_p()
        check(L.hbhip_comb_detect_create(ctx.h, C.byref(par), width, height, depth, C.byref(h)), ctx.h, "comb_detect_create")
        self.ctx, self.h, self.width, self.height, self.depth = ctx, h, width, height, depth
        if depth > 8:        # more entries than the params struct holds (comb_detect.c:1102)
            lut = np.ascontiguousarray(lut)
            check(L.hbhip_comb_detect_set_gamma_lut(h, lut.ctypes.data, maxv + 1), ctx.h, "comb_detect_set_gamma_lut")

    def store(self, luma):
        """A luma plane in host memory (2-D uint8, or uint16 for depth > 8) becomes the newest of the ring; None repeats it."""
        if luma is None:
            check(lib().hbhip_comb_detect_store(self.h, None, 0), self.ctx.h, "comb_detect_store")
            return
        check(lib().hbhip_comb_detect_store(self.h, luma.ctypes.data, luma.strides[0]), self.ctx.h, "comb_detect_store")

    def debug_mask(self, which, frame=0):
        """Test hook: mask `which` (0 detector, 1 filtered, 2 intermediate) of a frame of the last classify /
        classify_many as it lies in HBM: (height, stride) uint8."""
        import numpy as np
        st = C.c_int()
        lib().hbhip_comb_detect_debug_mask(self.h, frame, which, None, 0, C.byref(st))          # the stride (no buffer: refused)
        a = np.full((self.height, st.value), 0xAA, np.uint8)
        check(lib().hbhip_comb_detect_debug_mask(self.h, frame, which, a.ctypes.data, a.nbytes, C.byref(st)), self.ctx.h,
              "comb_detect_debug_mask")
        return a

    def store_dev(self, luma_ptr, stride):
        check(lib().hbhip_comb_detect_store_dev(self.h, C.c_void_p(luma_ptr), stride), self.ctx.h, "comb_detect_store_dev")

    def classify(self, force=False):
        out = C.c_int()
        check(lib().hbhip_comb_detect_classify(self.h, int(force), C.byref(out)), self.ctx.h, "comb_detect_classify")
        return out.value

    def classify_many(self, luma_ptrs, stride, force_bits=0):
        """len(luma_ptrs) - 2 verdicts in one go: frame i from lumas i, i+1, i+2 (device pointers)."""
        n = len(luma_ptrs) - 2
        L = lib()
        L.hbhip_comb_detect_classify_many_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint,
                                                          C.POINTER(C.c_int)]
        arr = (C.c_void_p * len(luma_ptrs))(*luma_ptrs)
        out = (C.c_int * n)()
        check(L.hbhip_comb_detect_classify_many_dev(self.h, arr, stride, n, force_bits, out), self.ctx.h, "comb_detect_classify_many")
        return list(out)

    def close(self):
        if self.h:
            lib().hbhip_filter_destroy(self.h)
            self.h = None


class DecombDevice:
    """A decomb instance driven through the raw C ABI with host frames (tests of the
    EEDI2 scratch buffers; the hb_filter_object_t path is hb_filter_decomb_hip)."""

    def __init__(self, ctx: Ctx, width, height, mode=8, parity=-1, magnitude=10, variance=20, laplacian=20,
                 dilation=4, erosion=2, noise=50, search=24, postproc=1, depth=8, lcw=1, lch=1):
        L = lib()
        L.hbhip_decomb_create.argtypes = [C.c_void_p, C.POINTER(DecombParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)]
        L.hbhip_decomb_push.argtypes = [C.c_void_p, C.POINTER(HostFrame), C.c_int64, C.c_int, C.c_int]
        L.hbhip_decomb_debug_eedi_plane.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                    C.POINTER(C.c_int), C.POINTER(C.c_int)]
        par = DecombParams(mode, parity, magnitude, variance, laplacian, dilation, erosion, noise, search, postproc)
        h = C.c_void_p()
        check(L.hbhip_decomb_create(ctx.h, C.byref(par), width, height, depth, lcw, lch, C.byref(h)), ctx.h, "decomb_create")
        self.ctx, self.h, self.w, self.hgt, self.depth = ctx, h, width, height, depth
        self.lcw, self.lch = lcw, lch
        self.tag = 0

    def push(self, planes, flags=0x0008, combed=2):
        import numpy as np
        keep = [np.ascontiguousarray(p) for p in planes]
        fr = host_frame(keep)
        check(lib().hbhip_decomb_push(self.h, C.byref(fr), self.tag, flags, combed), self.ctx.h, "decomb_push")
        self.tag += 1

    def use_frames(self):
        check(lib().hbhip_filter_use_frames(self.h), self.ctx.h, "use_frames")

    def push_frame(self, frame: Frame, flags=0x0008, combed=2):
        check(lib().hbhip_decomb_push_frame(self.h, frame.h, self.tag, flags, combed), self.ctx.h, "decomb_push_frame")
        self.tag += 1

    def pull(self):
        import numpy as np
        if lib().hbhip_filter_pending(self.h) <= 0:
            return None
        cw, ch = -(-self.w >> self.lcw), -(-self.hgt >> self.lch)
        dt = np.uint8 if self.depth == 8 else np.uint16
        out = [np.zeros((self.hgt, self.w), dt), np.zeros((ch, cw), dt), np.zeros((ch, cw), dt)]
        fr = host_frame(out)
        tag = C.c_int64()
        check(lib().hbhip_filter_pull(self.h, C.byref(fr), C.byref(tag)), self.ctx.h, "pull")
        return tag.value, out

    def flush(self):
        check(lib().hbhip_filter_flush(self.h), self.ctx.h, "flush")

    def eedi_plane(self, buffer, plane):
        import numpy as np
        st, ht = C.c_int(), C.c_int()
        check(lib().hbhip_decomb_debug_eedi_plane(self.h, buffer, plane, None, 0, C.byref(st), C.byref(ht)), self.ctx.h)
        a = np.zeros((ht.value, st.value), np.uint8)
        check(lib().hbhip_decomb_debug_eedi_plane(self.h, buffer, plane, a.ctypes.data, st.value, C.byref(st), C.byref(ht)),
              self.ctx.h, "debug_eedi_plane")
        return a if self.depth == 8 else a.view(np.uint16)          # (height, stride in samples)

    def close(self):
        if self.h:
            lib().hbhip_filter_destroy(self.h)
            self.h = None


class LapsharpParams(C.Structure):
    _fields_ = [("strength", C.c_double * 3), ("kernel", C.c_int * 3)]


class CropScaleParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "height", "crop_top", "crop_bottom", "crop_left", "crop_right")]


def _create(fn_name, ctx, argtypes, *args):
    L = lib()
    fn = getattr(L, fn_name)
    fn.argtypes = argtypes
    h = C.c_void_p()
    check(fn(*args, C.byref(h)), ctx.h, fn_name)
    return DeviceFilter(ctx, h)


def lapsharp_device_filter(ctx, width, height, strength=0.2, kernel=1, depth=8):
    """lapsharp 'medium' = strength 0.2, isolap (param.c:932-935)."""
    p = LapsharpParams((C.c_double * 3)(strength, strength, strength), (C.c_int * 3)(kernel, kernel, kernel))
    return _create("hbhip_lapsharp_create", ctx,
                   [C.c_void_p, C.POINTER(LapsharpParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                   ctx.h, C.byref(p), width, height, depth, 1, 1)


def cropscale_device_filter(ctx, width, height, out_w, out_h, crop=(0, 0, 0, 0), depth=8, sws=False, log2_cw=1, log2_ch=1,
                            chroma_location=None):
    """sws: libswscale's arithmetic (the reference's branch for odd sizes) instead of zimg's.  chroma_location: the
    stream's AVCHROMA_LOC_* number (zimg's arithmetic only; None = the call without one, which is left-sited)"""
    p = CropScaleParams(out_w, out_h, *crop)
    if chroma_location is not None:
        if sws:
            raise ValueError("the libswscale form stays left-sited")
        return _create("hbhip_cropscale_create_sited", ctx,
                       [C.c_void_p, C.POINTER(CropScaleParams)] + [C.c_int] * 6 + [C.POINTER(C.c_void_p)],
                       ctx.h, C.byref(p), width, height, depth, log2_cw, log2_ch, chroma_location)
    return _create("hbhip_cropscale_sws_create" if sws else "hbhip_cropscale_create", ctx,
                   [C.c_void_p, C.POINTER(CropScaleParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                   ctx.h, C.byref(p), width, height, depth, log2_cw, log2_ch)


class ColorspaceParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("in_prim", "in_transfer", "in_matrix", "in_range",
                                       "out_prim", "out_transfer", "out_matrix", "out_range", "tonemap")] + \
               [(n, C.c_double) for n in ("param", "desat", "npl", "peak")]


TONEMAPS = {"none": 0, "linear": 1, "gamma": 2, "clip": 3, "reinhard": 4, "hable": 5, "mobius": 6}


def colorspace_device_filter(ctx, width, height, src, dst, tonemap="hable", param=float("nan"), desat=0.0,
                             npl=100.0, peak=10.0, depth=8, log2_cw=1, log2_ch=1, chroma_location=None):
    """src / dst = (primaries, transfer, matrix, range) in AVCOL_* numbers, range 1 = tv, 2 = pc.  Matrix 12
    (chroma-derived-nc) on primaries with known chromaticities, 10 / 13 (bt2020c, chroma-derived-c) on BT.2020
    primaries and 14 (ICtCp) on BT.2020 primaries with PQ or HLG are accepted on either side.  chroma_location: the
    stream's AVCHROMA_LOC_* number (None = the call without one: left-sited horizontally, centred vertically)."""
    p = ColorspaceParams(*src, *dst, TONEMAPS[tonemap], param, desat, npl, peak)
    if chroma_location is not None:
        return _create("hbhip_colorspace_create_sited", ctx,
                       [C.c_void_p, C.POINTER(ColorspaceParams)] + [C.c_int] * 6 + [C.POINTER(C.c_void_p)],
                       ctx.h, C.byref(p), width, height, depth, log2_cw, log2_ch, chroma_location)
    return _create("hbhip_colorspace_create", ctx,
                   [C.c_void_p, C.POINTER(ColorspaceParams)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                   ctx.h, C.byref(p), width, height, depth, log2_cw, log2_ch)


def format_resample_device_filter(ctx, width, height, src=(1, 0), dst=(1, 1), depth=8, chroma_location=1):
    """format's chroma down-sampling: src / dst = (log2_chroma_w, log2_chroma_h) of the stream and of the target"""
    return _create("hbhip_format_resample_create", ctx, [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p)],
                   ctx.h, width, height, depth, src[0], src[1], dst[0], dst[1], chroma_location)


def format_scaled_device_filter(ctx, width, height, src=(1, 0), dst=(1, 1), src_depth=10, dst_depth=8, chroma_location=1):
    """format's scaler pass to a lower depth, with or without fewer chroma samples: src / dst = (log2_chroma_w,
    log2_chroma_h) of the stream and of the target"""
    return _create("hbhip_format_scaled_create", ctx, [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_void_p)],
                   ctx.h, width, height, src_depth, dst_depth, src[0], src[1], dst[0], dst[1], chroma_location)


def format_deepen_device_filter(ctx, width, height, src=(1, 0), dst=(1, 1), src_depth=8, dst_depth=10, chroma_location=1):
    """format's scaler pass to FEWER chroma samples at a higher depth: src / dst = (log2_chroma_w, log2_chroma_h) of the
    stream and of the target"""
    return _create("hbhip_format_deepen_create", ctx, [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_void_p)],
                   ctx.h, width, height, src_depth, dst_depth, src[0], src[1], dst[0], dst[1], chroma_location)


def format_upsample_device_filter(ctx, width, height, src=(1, 1), dst=(1, 0), src_depth=8, dst_depth=8, chroma_location=1):
    """format's scaler pass to MORE chroma samples at equal or higher depth: src / dst = (log2_chroma_w, log2_chroma_h) of
    the stream and of the target"""
    return _create("hbhip_format_upsample_create", ctx, [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_void_p)],
                   ctx.h, width, height, src_depth, dst_depth, src[0], src[1], dst[0], dst[1], chroma_location)


def decomb_push_dev(flt, frame: DevFrame, tag: int, flags: int = 0x0008, combed: int = 2):
    L = lib()
    L.hbhip_decomb_push_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame), C.c_int64, C.c_int, C.c_int]
    check(L.hbhip_decomb_push_dev(flt.h, C.byref(frame), tag, flags, combed), flt.ctx.h, "decomb_push_dev")


class BlendDevice:
    """hbhip_blend*: the subtitle compositor on device frames (tests / bench)."""

    def __init__(self, ctx: Ctx, width, height, depth=8, log2_cw=1, log2_ch=1, chroma_location=1,
                 overlay_log2_cw=0, overlay_log2_ch=0):
        L = lib()
        L.hbhip_blend_create.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p)]
        L.hbhip_blend_set_overlays.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hbhip_blend_apply_dev.argtypes = [C.c_void_p, C.POINTER(DevFrame)]
        L.hbhip_blend_destroy.argtypes = [C.c_void_p]
        L.hbhip_blend_destroy.restype = None
        h = C.c_void_p()
        check(L.hbhip_blend_create(ctx.h, width, height, depth, log2_cw, log2_ch, chroma_location,
                                   overlay_log2_cw, overlay_log2_ch, C.byref(h)), ctx.h, "hbhip_blend_create")
        self.ctx, self.h = ctx, h

    def set_overlays(self, overlays):
        """overlays: list of (x, y, (Y, Cb, Cr, A) uint8 arrays)."""
        from . import hbrt
        arr, keep = hbrt.overlay_array(overlays)       # same layout as hbhip_overlay
        check(lib().hbhip_blend_set_overlays(self.h, C.cast(arr, C.c_void_p), len(overlays)), self.ctx.h, "set_overlays")

    def apply_dev(self, frame: DevFrame):
        check(lib().hbhip_blend_apply_dev(self.h, C.byref(frame)), self.ctx.h, "blend_apply_dev")

    def set_ass_images(self, images, crop_left=0, crop_top=0):
        """images: libass's glyph images as hbrt.ass_image_array takes them; composed into overlays on the device"""
        from . import hbrt
        L = lib()
        L.hbhip_blend_set_ass_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        arr, keep = hbrt.ass_image_array(images)
        check(L.hbhip_blend_set_ass_images(self.h, C.cast(arr, C.c_void_p), len(images), crop_left, crop_top), self.ctx.h,
              "set_ass_images")

    def set_bitmaps(self, subs, crop=(0, 0, 0, 0), strides=None, raise_on_error=True):
        """subs: decoded bitmap subtitles, a list of (x, y, (Y, Cb, Cr, A) uint8 arrays, (window_width, window_height), key);
        scaled and placed on the device as scale_subtitle would, once per key.  crop = (top, bottom, left, right).
        strides: row pitches to declare in place of the arrays' own (per sub, four each).  Returns the HBHIP_* code where
        raise_on_error is off."""
        import numpy as np
        L = lib()
        L.hbhip_blend_set_bitmaps.argtypes = [C.c_void_p, C.POINTER(BitmapSub), C.c_int, C.POINTER(C.c_int)]
        arr = (BitmapSub * max(len(subs), 1))()
        keep = []
        for i, (x, y, planes, window, key) in enumerate(subs):
            planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
            keep.append(planes)
            for k, p in enumerate(planes):
                arr[i].plane[k] = p.ctypes.data
                arr[i].stride[k] = p.strides[0] if strides is None else strides[i][k]
            arr[i].x, arr[i].y = x, y
            arr[i].height, arr[i].width = planes[0].shape
            arr[i].window_width, arr[i].window_height = window
            arr[i].key = key
        rc = L.hbhip_blend_set_bitmaps(self.h, arr, len(subs), (C.c_int * 4)(*crop))
        return check(rc, self.ctx.h, "set_bitmaps") if raise_on_error else rc

    def bitmap_stats(self):
        """(scale launches, bitmaps uploaded, cache hits) of set_bitmaps since the object was made (test hook)"""
        L = lib()
        L.hbhip_blend_debug_bitmap_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
        v = [C.c_int64() for _ in range(3)]
        check(L.hbhip_blend_debug_bitmap_stats(self.h, *[C.byref(x) for x in v]), self.ctx.h, "bitmap_stats")
        return tuple(x.value for x in v)

    def overlays(self, log2_cw=1, log2_ch=1):
        """the object's overlay list read back from its device store (test hook): [(x, y, (Y, Cb, Cr, A))], the chroma
        planes in the overlay subsampling given"""
        import numpy as np
        L = lib()
        L.hbhip_blend_debug_overlay_count.argtypes = [C.c_void_p]
        L.hbhip_blend_debug_get_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        out = []
        for i in range(check(L.hbhip_blend_debug_overlay_count(self.h), self.ctx.h, "overlay_count")):
            g = (C.c_int * 4)()
            check(L.hbhip_blend_debug_get_overlay(self.h, i, None, None, g), self.ctx.h, "get_overlay")
            x, y, w, h = g
            cw, ch = -(-w >> log2_cw), -(-h >> log2_ch)
            planes = [np.zeros(s, np.uint8) for s in ((h, w), (ch, cw), (ch, cw), (h, w))]
            ptrs = (C.c_void_p * 4)(*[p.ctypes.data for p in planes])
            strides = (C.c_int * 4)(*[p.strides[0] for p in planes])
            check(L.hbhip_blend_debug_get_overlay(self.h, i, ptrs, strides, g), self.ctx.h, "get_overlay")
            out.append((x, y, tuple(planes)))
        return out

    def close(self):
        if self.h:
            lib().hbhip_blend_destroy(self.h)
            self.h = None
