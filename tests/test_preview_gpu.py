"""GPU: hb_get_preview's list as one device-resident run - hbrt.preview_run, so filter objects -> adapters -> C ABI ->
rgb32_pack_kernel.  The list is the job's picture filters, the display rescale and `format=bgra`, built and initialised the
way the hook of INTEGRATION.md 2b has hb_get_preview do it (hbh_preview_open).  Expected for each list: tests/rgb32_model.py
applied to the composition of the oracle's helpers for the same stages, at tolerance 0.

The registered objects are CPU stand-ins that do nothing (no CPU filter of the reference is linked here): the swap puts the
drop-ins in, and where a drop-in declines, the stand-in of its id comes back - enough to see WHICH object an entry ends on.

The PAR 4:3 case: hb.c:926 makes the display width 64 * 4 / 3 = 85, an odd size, which the RGB step declines like the odd
height below (swscale leaves its unscaled path there); the even 84 x 36 rescale comes from PAR 21:16, and both are here."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip, synth
import oracle_lib as ol
import oracle_stream as os_
import rgb32_model as rm

pytestmark = pytest.mark.gpu
W, H = 96, 54
KEY = "hip-rgb-step"
SCALE = "width=64:height=36:crop-top=0:crop-bottom=0:crop-left=0:crop-right=0"
PAD = "width=80:height=48:color=0x336699:x=8:y=6"
GRAY = "cb=0:cr=0:size=1:high=0"
NAMES = {"decomb": "Decomb", "crop_scale": "Crop and Scale", "pad": "Pad", "rotate": "Rotate", "grayscale": "Grayscale",
         "format": "Format"}


@pytest.fixture()
def cpu_objects(built):
    """the ids' registered filters: CPU stand-ins whose init() succeeds and that are never run"""
    hip.filters()
    F = hbrt.FILTER_ID
    rt = hbrt.runtime()
    keep = {}
    for name, shown in NAMES.items():
        addr, keep[name] = hbrt.filter_stub(F[name], shown)
        rt.hbhip_rt_register_filter(F[name], addr)
    yield F
    for name in keep:
        rt.hbhip_rt_register_filter(F[name], None)


@pytest.fixture(scope="module")
def pictures():
    """a progressive and an interlaced 96 x 54 picture: made once, only read"""
    out = {"progressive": synth.stream("progressive", W, H, 1)[0], "interlaced": synth.stream("interlaced", W, H, 1)[0]}
    for fr in out.values():
        for p in fr:
            p.flags.writeable = False
    return out


def rescaled(fr, par):
    """hb.c:917-933: the display rescale of a frame for a pixel aspect"""
    h, w = fr[0].shape
    sw, sh = (w * par[0] // par[1], h) if par[0] >= par[1] else (w, h * par[1] // par[0])
    return ol.orc_cropscale_frame(fr, sw, sh)


def one_run(entries, n_dropins):
    names = [n for n, _ in entries]
    assert names[0] == "HIP upload adapter" and names[-1] == "HIP download adapter", names
    assert names.count("HIP upload adapter") == 1 and names.count("HIP download adapter") == 1, names
    assert len(names) == n_dropins + 2 and all("HIP" in n for n in names), names          # no CPU filter
    assert names[-2] == "Format (HIP)"
    assert entries[-2][1].get(KEY) == "1" and entries[-1][1].get(KEY) == "1"


@pytest.mark.parametrize("par,size", [((1, 1), (64, 36)), ((21, 16), (84, 36))])
def test_crop_scale_and_the_display_rescale(cpu_objects, pictures, par, size):
    fr = pictures["progressive"]
    entries, got = hbrt.preview_run([(cpu_objects["crop_scale"], SCALE)], fr, par=par)
    one_run(entries, 3)                                                   # crop/scale, the rescale, format
    want = rm.pack(rescaled(ol.orc_cropscale_frame(fr, 64, 36), par), 1, False, "bgra")
    assert got.shape == (size[1], size[0], 4)
    np.testing.assert_array_equal(got, want)


def test_decomb_crop_scale_pad(cpu_objects, pictures):
    fr = pictures["interlaced"]
    F = cpu_objects
    entries, got = hbrt.preview_run([(F["decomb"], "mode=7"), (F["crop_scale"], SCALE), (F["pad"], PAD)], fr)
    one_run(entries, 5)
    mid = os_.decomb_stream([fr], dict(mode=7), flags=0x10)
    assert len(mid) == 1
    mid = ol.orc_pad_frame(ol.orc_cropscale_frame(mid[0]["planes"], 64, 36), 80, 48, 8, 6, rgb=0x336699)
    want = rm.pack(rescaled(mid, (1, 1)), 1, False, "bgra")
    assert got.shape == (48, 80, 4)
    np.testing.assert_array_equal(got, want)


def test_rotate_grayscale(cpu_objects, pictures):
    fr = pictures["progressive"]
    F = cpu_objects
    entries, got = hbrt.preview_run([(F["rotate"], "angle=90:hflip=0"), (F["grayscale"], GRAY)], fr)
    one_run(entries, 4)
    mid = ol.orc_grayscale_frame(ol.orc_rotate_frame(fr, 90, 0))
    want = rm.pack(rescaled(mid, (1, 1)), 1, False, "bgra")
    assert got.shape == (W, H, 4)                                        # 54 wide, 96 high
    np.testing.assert_array_equal(got, want)
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all() and (got[..., 3] == 255).all()


def test_rgba_gives_the_other_order(cpu_objects, pictures):
    fr = pictures["progressive"]
    entries, got = hbrt.preview_run([(cpu_objects["crop_scale"], SCALE)], fr, pix_fmt="rgba")
    one_run(entries, 3)
    assert entries[-1][1]["format"] == "rgba"
    mid = rescaled(ol.orc_cropscale_frame(fr, 64, 36), (1, 1))
    np.testing.assert_array_equal(got, rm.pack(mid, 1, False, "rgba"))
    np.testing.assert_array_equal(got[..., [2, 1, 0, 3]], rm.pack(mid, 1, False, "bgra"))


@pytest.mark.parametrize("scale,par", [("width=64:height=35", (1, 1)), (SCALE, (4, 3))], ids=["odd-height", "odd-width"])
def test_an_odd_size_keeps_the_cpu_format(cpu_objects, pictures, monkeypatch, scale, par):
    """96 x 54 -> 64 x 35, and 64 x 36 shown at PAR 4:3 (85 wide): the Format entry ends on its CPU object, no key is left
    anywhere, and the frames leave the device in front of it.  Not run: the CPU objects here are stand-ins - which is also
    why crop/scale gets its opt-in swscale branch (HBHIP_SWSCALE=1): by default it hands an odd size to its CPU object
    (INTEGRATION 6), and a stand-in that scales nothing would leave the entries behind it an even 96 x 54."""
    monkeypatch.setenv("HBHIP_SWSCALE", "1")
    entries, got = hbrt.preview_run([(cpu_objects["crop_scale"], scale)], pictures["progressive"], par=par, run=False)
    assert got is None
    names = [n for n, _ in entries]
    assert names == ["HIP upload adapter", "Crop and Scale (HIP)", "Crop and Scale (HIP)", "HIP download adapter", "Format"], entries
    assert entries[-1][1] == {"format": "bgra"} and "format" not in entries[-2][1], entries
    assert not any(KEY in s for _, s in entries), entries
