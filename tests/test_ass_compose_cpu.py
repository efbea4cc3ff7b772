"""CPU: text subtitles.  tests/ass_compose_model.py - the numpy restatement the GPU tests hold hbhip_blend_set_ass_images
to - against tests/golden/ass_compose_*.npz, recorded from the reference's own render_ssa_subs / compose_subsample_ass
(rendersub.c:474-665; tests/golden/make_ass_compose_golden.py): the same boxes at the same positions, luma and alpha equal
everywhere, chroma equal wherever the reference defines it (accu_c > 0, :593 - elsewhere it leaves what its buffer pool
held).  And what the new entry points answer without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import ass_compose_model as am

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOXES = {"pair": 1, "stack": 1, "gap": 2, "wide": 1, "tiny": 2, "stride": 1, "origin": 2}


def golden(name):
    """{(fmt, crop_left, crop_top, loc): [(x, y, (Y, Cb, Cr, A))]} of a case"""
    z = np.load(os.path.join(GOLDEN, f"ass_compose_{name}.npz"))
    out = {}
    for fmt, cl, ct, loc, x, y, w, h, cw, ch, at in z["table"].tolist():
        planes = []
        for pw, ph in ((w, h), (cw, ch), (cw, ch), (w, h)):
            planes.append(z["data"][at:at + pw * ph].reshape(ph, pw))
            at += pw * ph
        out.setdefault((str(fmt), cl, ct, loc), []).append((x, y, tuple(planes)))
    return out


@pytest.mark.parametrize("name", sorted(am.CASES))
def test_model_equals_the_reference(name):
    recorded = golden(name)
    assert len(recorded) == 10
    for (fmt, cl, ct, loc), want in recorded.items():
        ws, hs = am.SHIFTS[fmt]
        _, _, images = am.build(name, fmt)
        got, masks = am.render(images, ws, hs, loc, cl, ct)
        what = f"{name} {fmt} crop {cl},{ct} loc {loc}"
        assert len(got) == len(want) == BOXES[name], what
        for (gx, gy, gp), (wx, wy, wp), mask in zip(got, want, masks):
            assert (gx, gy) == (wx, wy), what
            assert [p.shape for p in gp] == [p.shape for p in wp], what
            np.testing.assert_array_equal(gp[0], wp[0], err_msg=what + " Y")
            np.testing.assert_array_equal(gp[3], wp[3], err_msg=what + " A")
            for c in (1, 2):
                np.testing.assert_array_equal(gp[c][mask], wp[c][mask], err_msg=what + f" plane {c}")
            # an undefined sample has alpha 0 at its block's first pixel, the one whose alpha the compositor applies to a
            # chroma sample of an overlay in the frame's subsampling (blend.c:485-505): it cannot reach a frame
            assert not gp[3][::1 << hs, ::1 << ws][~mask].any(), what


@pytest.mark.parametrize("name", sorted(am.CASES))
def test_most_chroma_samples_are_defined(name):
    """the comparison on the mask compares something: 70 % of the chroma samples at least, in every combination the GPU
    tests run"""
    for fmt in am.SHIFTS:
        ws, hs = am.SHIFTS[fmt]
        _, _, images = am.build(name, fmt)
        for loc in (1, 2, 3):
            for crop in ((0, 0), (1, 1)):
                _, masks = am.render(images, ws, hs, loc, *crop)
                assert am.defined_share(masks) >= 0.7, (name, fmt, loc, crop)


def test_boxes_merge_across_eight_pixels_not_nine():
    _, _, images = am.build("gap")
    assert am.boxes_of(images) == [[4, 4, 52, 14], [61, 4, 81, 14]]
    # a box the merge has cleared takes part in the rest of the pass as (0, 0, 0, 0): one near the origin joins it
    _, _, images = am.build("origin")
    assert am.boxes_of(images) == [[30, 30, 72, 48], [0, 0, 10, 10]]
    assert am.boxes_of(images[:2]) == [[30, 30, 70, 46], [1, 1, 10, 10]]


def test_entry_points_without_an_object(built):
    """no object, no images: HBHIP_ERR_ARG; no GPU: no context to make an object on (HBHIP_ERR_NODEVICE), and the drop-in's
    init() has failed, so its private data is missing"""
    L = hip.lib()
    L.hbhip_blend_set_ass_images.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    arr, keep = hbrt.ass_image_array(am.build("pair")[2])
    assert L.hbhip_blend_set_ass_images(None, C.cast(arr, C.c_void_p), 2, 0, 0) == -3
    L.hbhip_blend_debug_overlay_count.argtypes = [C.c_void_p]
    assert L.hbhip_blend_debug_overlay_count(None) == -3
    assert C.sizeof(hbrt.AssImage) == 32
    F = hip.filters()
    F.hb_blend_hip_set_ass_images.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    assert F.hb_blend_hip_set_ass_images(None, None, C.cast(arr, C.c_void_p), 2, None) == -3
    if L.hbhip_device_count() > 0:
        return
    h = C.c_void_p()
    assert L.hbhip_ctx_create(0, C.byref(h)) == -1 and not h.value
    frame = am.frame(96, 64)
    with pytest.raises(RuntimeError):
        hbrt.blend_run_ass(F, "hb_blend_hip", frame, [am.build("pair")[2]])
