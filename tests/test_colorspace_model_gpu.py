"""GPU: the colorspace HIP drop-in on lattice frames (tests/colour_model.py), bit-exact to the oracle over the whole
frame - the corners of the Y'CbCr cube included, where the PQ EOTF reaches its pole and +-inf / NaN are pinned to the
clip limits - and within the float64 model's tolerances directly, in 4:4:4 and 4:2:0 at 8 / 10 / 12 bits."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import colour_model as cm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

YSTEP = {8: 1, 10: 4, 12: 16}            # 256 Y codes per frame (the top code always), x a 33 x 33 chroma lattice
LAYOUTS = {"444": ("1x1", (0, 0)), "420": ("2x2", (1, 1))}
LATTICE = [(c, d) for c in cm.CASES for d in c[5]]


def frame(depth, layout):
    return cm.lattice_frame(depth, ystep=YSTEP[depth], sub=LAYOUTS[layout][1])


def held(got, case, depth, layout, fr):
    """bit-exact to the oracle, and within the model's tolerances"""
    _, src, _, dst, kw, _ = case
    sub = LAYOUTS[layout][1]
    want = ol.orc_colorspace_frame(fr, ol.colorspace_params(src, dst, **kw), depth=depth, subw=sub[0], subh=sub[1])
    for c in range(3):
        np.testing.assert_array_equal(got[c], want[c], err_msg=f"{case[0]} {depth} bits {layout}: plane {c} vs oracle")
    _, fails = cm.judge(cm.Conversion(src, dst, depth, **kw).convert(fr, *sub), got, hdr_source=src[1] in (16, 18))
    assert not fails, f"{case[0]} {depth} bits {layout}: " + "; ".join(fails)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case,depth", LATTICE, ids=[f"{c[0]}-{d}" for c, d in LATTICE])
def test_drop_in_on_the_lattice(built, case, depth, layout):
    cid, src, settings, dst, kw, _ = case
    fr = frame(depth, layout)
    hbrt.set_source_color(*src)
    try:
        out = hbrt.run_stream(hip.filters(), [("hb_filter_colorspace_hip", settings)], [fr],
                              pix_fmt=hbrt.PIX_FMT[(LAYOUTS[layout][0], depth)])
    finally:
        hbrt.set_source_color()
    assert len(out) == 1
    held(out[0].planes, case, depth, layout, fr)


BATCHED = {8: cm.CASES[0], 10: next(c for c in cm.CASES if c[0] == "pq_709_hable"),
           12: next(c for c in cm.CASES if c[0] == "hlg_pq")}


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_batched_path_on_the_lattice(built, depth):
    """hbhip_filter_process_dev (one launch for the batch), as test_many_frames_per_launch drives it"""
    import torch
    case = BATCHED[depth]
    _, src, _, dst, kw, _ = case
    frames = [frame(depth, "420")] * 3
    h, w = frames[0][0].shape
    npdt, tdt = (np.uint8, torch.uint8) if depth == 8 else (np.int16, torch.int16)
    ctx = hip.Ctx(0)
    flt = hip.colorspace_device_filter(ctx, w, h, src, dst, depth=depth, **kw)
    try:
        dev_in = [[torch.from_numpy(np.ascontiguousarray(p).view(npdt)).cuda() for p in f] for f in frames]
        outs = [[torch.zeros(p.shape, dtype=tdt, device="cuda") for p in f] for f in frames]
        torch.cuda.synchronize()
        arr_in = (hip.DevFrame * len(frames))(*[hip.dev_frame(f) for f in dev_in])
        arr_out = (hip.DevFrame * len(frames))(*[hip.dev_frame(o) for o in outs])
        assert flt.process_dev(arr_in, 0, arr_out) == len(frames)
        ctx.sync()
        got = [[p.cpu().numpy().view(np.uint8 if depth == 8 else np.uint16) for p in o] for o in outs]
    finally:
        flt.close()
        ctx.close()
    for g in got:
        held(g, case, depth, "420", frames[0])
