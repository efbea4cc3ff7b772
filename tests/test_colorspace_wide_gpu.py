"""GPU: the colorspace HIP drop-in on constant-luminance (bt2020c, chroma-derived-c), chroma-derived-nc and ICtCp
streams and targets.  oracle/colorspace_oracle.c refuses these ids, so the new paths have no bit-for-bit pin: they are
held to the float64 model (tests/colour_model_wide.py) within colour_model.judge's tolerances, and the filter's two
entry points (the drop-in, one frame a launch; process_dev, 16 a launch) to each other bit for bit.  The caps of every
lattice case are asserted from the model alone in tests/test_colour_model_wide_cpu.py."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import colour_model as cm
import colour_model_wide as cw

pytestmark = pytest.mark.gpu
UP, DOWN = ("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")


def drop_in(src, settings, frames, depth, layout="420", more=()):
    hbrt.set_source_color(*src)
    try:
        return hbrt.run_stream(hip.filters(), [("hb_filter_colorspace_hip", settings)] + list(more), frames,
                               pix_fmt=hbrt.PIX_FMT[(cw.LAYOUTS[layout][0], depth)])
    finally:
        hbrt.set_source_color()


def judged(res, got, src, what):
    st, fails = cm.judge(res, got, hdr_source=cw.hdr_source(src))
    print(what, {k: st[k] for k in ("max_in", "max_ill_excess", "max_out", "ill", "excluded")})
    assert not fails, f"{what}: " + "; ".join(fails)


@pytest.mark.parametrize("case,depth,layout", cw.LATTICE, ids=[f"{c[0]}-{d}-{lay}" for c, d, lay in cw.LATTICE])
def test_drop_in_on_the_lattice(built, case, depth, layout):
    cid, src, settings, _, _, _ = case
    out = drop_in(src, settings, [cw.frame(depth, layout)], depth, layout)
    assert len(out) == 1
    judged(cw.result(case, depth, layout), out[0].planes, src, f"{cid} {depth} bits {layout}")


@pytest.mark.parametrize("layout", ["444", "420"])
def test_chroma_derived_c_is_bt2020c(built, layout):
    """matrix id 13 on BT.2020 primaries is id 10, on either side: bit for bit"""
    fr = cw.frame(10, layout)
    for a, b, settings in [(cw.CDC, cw.CLSDR, ("matrix=bt2020nc",) * 2),
                           (cw.NC, cw.NC, ("matrix=chroma-derived-c", "matrix=bt2020c"))]:
        one, two = drop_in(a, settings[0], [fr], 10, layout), drop_in(b, settings[1], [fr], 10, layout)
        for c in range(3):
            np.testing.assert_array_equal(one[0].planes[c], two[0].planes[c], err_msg=f"{settings} plane {c}")


@pytest.mark.parametrize("src,settings", [(cw.PQ_NC, "transfer=bt709:matrix=ictcp"),               # SDR destination transfer
                                          (cm.BT709, "matrix=ictcp"),                              # BT.709 primaries
                                          (cm.BT709, "matrix=chroma-derived-c"),
                                          ((9, 1, 14, 1), "matrix=bt2020nc"),                      # ICtCp source, transfer bt709
                                          ((10, 1, 1, 1), "matrix=chroma-derived-nc")],            # no chromaticities (ST 428 XYZ)
                         ids=["ictcp_sdr", "ictcp_709", "cdc_709", "ictcp_source_709", "cdnc_xyz"])
def test_still_declined(built, src, settings):
    hbrt.set_source_color(*src)
    try:
        with pytest.raises(RuntimeError):
            hbrt.Chain(hip.filters(), [("hb_filter_colorspace_hip", settings)], 320, 180, pix_fmt=hbrt.PIX_FMT[("2x2", 10)])
    finally:
        hbrt.set_source_color()


@pytest.mark.parametrize("cid", ["pqictcp_709_hable", "cl_nc"])
def test_batched_path_equals_the_drop_in(built, cid):
    """hbhip_filter_process_dev on 19 frames (one launch of 16 and a rest) against the single-frame drop-in, bit for
    bit: the determinism pin that stands in for the oracle these ids do not have"""
    import torch
    _, src, settings, dst, kw, _ = cw.BY_ID[cid]
    w, h, n = cw.BATCHED
    frames = cw.batched_stream()
    ctx = hip.Ctx(0)
    flt = hip.colorspace_device_filter(ctx, w, h, src, dst, depth=10, **kw)
    try:
        dev_in = [[torch.from_numpy(np.ascontiguousarray(p).view(np.int16)).cuda() for p in f] for f in frames]
        outs = [[torch.zeros(p.shape, dtype=torch.int16, device="cuda") for p in f] for f in frames]
        torch.cuda.synchronize()
        arr_in = (hip.DevFrame * n)(*[hip.dev_frame(f) for f in dev_in])
        arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
        assert flt.process_dev(arr_in, 0, arr_out) == n
        ctx.sync()
        got = [[p.cpu().numpy().view(np.uint16) for p in o] for o in outs]
    finally:
        flt.close()
        ctx.close()
    single = drop_in(src, settings, frames, 10)
    assert len(single) == n
    for t in range(n):
        for c in range(3):
            np.testing.assert_array_equal(got[t][c], single[t].planes[c], err_msg=f"{cid} frame {t} plane {c}")
    if cid == cw.BATCHED_JUDGED[0]:
        t = cw.BATCHED_JUDGED[1]
        judged(cw.Conversion(src, dst, 10, **kw).convert(frames[t], 1, 1), got[t], src, f"{cid} batched frame {t}")


def test_inside_a_device_resident_run(built):
    """[colorspace (ICtCp -> BT.709, hable), crop_scale, lapsharp] between upload and download equals the list on the
    host path and the list run stage by stage"""
    _, src, settings, _, _, _ = cw.BY_ID["pqictcp_709_hable"]
    rest = [("hb_filter_crop_scale_hip", "width=480:height=270"),
            ("hb_filter_lapsharp_hip", "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap")]
    frames = cw.batched_stream()[:6]
    fmt = hbrt.PIX_FMT[("2x2", 10)]
    host = drop_in(src, settings, frames, 10, more=rest)
    hbrt.set_source_color(*src)
    try:
        dev = hbrt.run_stream(hip.filters(), [UP, ("hb_filter_colorspace_hip", settings)] + rest + [DOWN], frames, pix_fmt=fmt)
    finally:
        hbrt.set_source_color()
    staged = [o.planes for o in drop_in(src, settings, frames, 10)]
    for stage in rest:
        staged = [o.planes for o in hbrt.run_stream(hip.filters(), [stage], staged, pix_fmt=fmt)]
    assert len(dev) == len(host) == len(staged) == len(frames)
    for t in range(len(frames)):
        assert (dev[t].start, dev[t].stop) == (host[t].start, host[t].stop)
        for c in range(3):
            np.testing.assert_array_equal(dev[t].planes[c], host[t].planes[c], err_msg=f"frame {t} plane {c} vs the host path")
            np.testing.assert_array_equal(dev[t].planes[c], staged[t][c], err_msg=f"frame {t} plane {c} vs stage by stage")


def test_the_new_id_reaches_the_stage_downstream(built):
    """init->color_matrix carries the new id on: a second colorspace stage converts FROM ICtCp, exactly as when it is
    told so as the source's colour (had it seen bt2020nc it would have nothing to do and pass ICtCp through)"""
    fr = cw.edge_frame(10, 62, 34)
    both = drop_in(cw.PQ_NC, "matrix=ictcp", [fr], 10, more=[("hb_filter_colorspace_hip", "matrix=bt2020nc")])
    first = drop_in(cw.PQ_NC, "matrix=ictcp", [fr], 10)
    second = drop_in(cw.PQ_ICTCP, "matrix=bt2020nc", [first[0].planes], 10)
    for c in range(3):
        np.testing.assert_array_equal(both[0].planes[c], second[0].planes[c], err_msg=f"plane {c}")
    assert not np.array_equal(both[0].planes[1], first[0].planes[1])


@pytest.mark.parametrize("cid,depth,w,h", cw.EDGES, ids=[f"{c}-{d}-{w}x{h}" for c, d, w, h in cw.EDGES])
def test_edges(built, cid, depth, w, h):
    """one full tile with a one-column and a one-row remainder, and the smallest frame create admits, 4:2:0"""
    _, src, settings, dst, kw, _ = cw.BY_ID[cid]
    fr = cw.edge_frame(depth, w, h)
    out = drop_in(src, settings, [fr], depth)
    judged(cw.Conversion(src, dst, depth, **kw).convert(fr, 1, 1), out[0].planes, src, f"{cid} {depth} bits {w}x{h}")
