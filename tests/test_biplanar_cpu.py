"""NV12 / P010LE without a GPU: the numpy model (tests/biplanar_model.py) against the reference's own hb_blend
(libhb/blend.c compiled in place, oracle/ref_wrap/wrap_blend.c), the repack identities, the two-plane layout of the
stand-in runtime, and the additive ABI."""
import os
import re

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import oracle_lib as ol
import biplanar_model as bm
import biplanar_cases as bc

needs_ref = pytest.mark.skipif(ol.ref() is None, reason="oracle/_ref/libhbref.so not built (no /root/reference)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_blend(frame2, ovs, pix_fmt, overlay_fmt, loc):
    return hbrt.blend_run(ol.ref(), "hb_blend", frame2, ovs, pix_fmt=pix_fmt, overlay_fmt=overlay_fmt, chroma_location=loc)


@needs_ref
@pytest.mark.parametrize("w,h", [(66, 38), (130, 74)])
@pytest.mark.parametrize("pix_fmt,overlay_fmt,loc", bc.CASES)
def test_model_is_the_references_hb_blend(built, pix_fmt, overlay_fmt, loc, w, h):
    frame = bc.frame(pix_fmt, w, h)
    ovs = bc.overlays(w, h, overlay_fmt)
    want = ref_blend(frame, ovs, pix_fmt, overlay_fmt, loc)
    got = bm.blend_bi(frame, ovs, bc.DEPTH[pix_fmt], loc, bc.SHIFTS[overlay_fmt])
    assert any((a != b).any() for a, b in zip(want, frame))
    for p in range(2):
        np.testing.assert_array_equal(got[p], want[p], err_msg=f"plane {p}")


@needs_ref
def test_nine_disjoint_overlays(built):
    frame = bc.frame(bc.NV12, 258, 130)
    ovs = bc.nine_disjoint(258, 130, bc.YUVA444P)
    want = ref_blend(frame, ovs, bc.NV12, bc.YUVA444P, 1)
    got = bm.blend_bi(frame, ovs, 8, 1, (0, 0))
    for p in range(2):
        np.testing.assert_array_equal(got[p], want[p], err_msg=f"plane {p}")


@pytest.mark.parametrize("overlay_fmt", [bc.YUVA420P, bc.YUVA444P])
def test_p010_is_composited_msb_aligned(built, overlay_fmt):
    """The 1x biplanar forms take the overlay sample as v << 8 against max = 1023 and alpha << 2 (blend.c:193, :747): the
    low six bits of a result are generally not zero, and splitting to planar 10-bit, compositing there and merging back
    gives other numbers."""
    frame = bc.frame(bc.P010LE, 66, 38)
    ovs = bc.overlays(66, 38, overlay_fmt)
    got = bm.blend_bi(frame, ovs, 10, 1, bc.SHIFTS[overlay_fmt])
    assert all((p & 63 == 0).all() for p in frame)
    assert any((p & 63 != 0).any() for p in got)


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", [(2, 2), (66, 38), (67, 39)])
def test_repack_identities(depth, w, h):
    rng = np.random.default_rng(w + depth)
    dt = np.uint8 if depth == 8 else np.uint16
    ch, cw = (h + 1) // 2, (w + 1) // 2
    x = tuple(rng.integers(0, 1 << depth, s).astype(dt) for s in ((h, w), (ch, cw), (ch, cw)))
    for a, b in zip(bm.split(bm.merge(x, depth), depth), x):
        np.testing.assert_array_equal(a, b)
    y = bc.frame(bc.NV12 if depth == 8 else bc.P010LE, w, h)          # P010LE: low six bits zero
    for a, b in zip(bm.merge(bm.split(y, depth), depth), y):
        np.testing.assert_array_equal(a, b)
    if depth == 10:
        assert all((p & 63 == 0).all() for p in bm.merge(x, depth))


def test_model_declines_what_the_drop_in_declines():
    frame = bc.frame(bc.NV12, 66, 38)
    with pytest.raises(bm.Declined):
        bm.blend_bi(frame, [], 12)
    with pytest.raises(bm.Declined):
        bm.blend_bi(frame, [], 8, overlay_shifts=(1, 0))
    with pytest.raises(bm.Declined):
        bm.split(bc.frame(bc.NV12, 1, 4), 8)


@pytest.mark.parametrize("pix_fmt,bps", [(bc.NV12, 1), (bc.P010LE, 2)])
def test_runtime_lays_two_planes_out(built, pix_fmt, bps):
    """hb_frame_buffer_init (fifo.c:820-881): luma, then ceil(h / 2) rows of interleaved Cb Cr, rows rounded up to 64
    bytes, the planes back to back, f.max_plane == 1"""
    w, h = 66, 38
    info = hbrt.frame_layout(pix_fmt, w, h)
    assert info.nplanes == 2
    assert list(info.plane_height[:2]) == [38, 19]
    assert list(info.plane_width[:2]) == [66, 33]
    assert list(info.plane_stride[:2]) == [-(-66 * bps // 64) * 64, -(-2 * 33 * bps // 64) * 64]
    assert info.plane_width[3] == info.plane_stride[0] * 38


def test_runtime_knows_the_names(built):
    rt = hbrt.runtime()
    rt.av_get_pix_fmt.argtypes = [hbrt.C.c_char_p]
    assert rt.av_get_pix_fmt(b"nv12") == 23 and rt.av_get_pix_fmt(b"p010le") == 158
    assert rt.av_pix_fmt_count_planes(23) == 2 and rt.av_pix_fmt_count_planes(158) == 2
    assert rt.av_pix_fmt_count_planes(0) == 3


def test_header_and_binding_agree_on_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    declared = set(re.findall(r"\b(hbhip_\w*biplanar\w*)\s*\(", text))
    assert declared == {s for s in hip.ABI_SYMBOLS if "biplanar" in s}
    assert declared == {"hbhip_frame_upload_biplanar", "hbhip_frame_download_biplanar", "hbhip_frame_upload_biplanar_async",
                        "hbhip_frame_download_biplanar_async", "hbhip_blend_create_biplanar", "hbhip_blend_apply_biplanar"}
    L = hip.lib()
    for s in declared:
        assert hasattr(L, s), s


@pytest.mark.parametrize("pix_fmt", [101, 207])        # NV16, P012LE (the stand-in runtime's own numbers for them)
def test_blend_drop_in_still_refuses_other_two_plane_formats(built, pix_fmt):
    """Without a device init() refuses everything before it reaches the two-plane rule; what this holds is that the
    runtime knows the two as two-plane formats and that nothing takes them.  The rule itself is held where a device is:
    tests/test_biplanar_gpu.py::test_compositor_refuses_other_two_plane_formats."""
    assert hbrt.runtime().av_pix_fmt_count_planes(pix_fmt) == 2
    frame = bc.frame(bc.P010LE if pix_fmt == 207 else bc.NV12, 66, 38)
    with pytest.raises(RuntimeError):
        hbrt.blend_run(hip.filters(), "hb_blend_hip", frame, bc.overlays(66, 38, bc.YUVA444P), pix_fmt=pix_fmt)


def test_adapters_fail_cleanly_without_a_device(built):
    if hip.lib().hbhip_device_count() > 0:
        pytest.skip("a GPU is present: tests/test_biplanar_gpu.py runs the adapters")
    with pytest.raises(RuntimeError):
        hbrt.Chain(hip.filters(), [("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "format=nv12")], 66, 38,
                   pix_fmt=bc.NV12)
