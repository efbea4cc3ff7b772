"""CPU: the deinterlacer oracles on full-range content (tests/deint_cases.py), tolerance 0.

  * the contents reach what they are made for (deint_cases.reach, every count >= REACH_FLOOR for every shape and depth);
  * oracle/decomb_oracle.c's decomb restatement against the reference's own hb_filter_decomb, where clamps bind, the
    diagonal search sees every cascade and the 12-bit blend indexes the first and last entry of the crop table;
  * the FFmpeg-yadif restatement (orc_yadif_ff_plane, spatial check on, send_frame) against the reference's decomb mode 1
    on rows 3 <= y <= h - 4: away from the top and bottom rows the two are the same arithmetic (decomb.hip runs both
    through one code path that differs in `vertical_edge` only) - the one pin to reference C that the yadif restatement,
    whose own source is not in the reference tree, can have.
The last two skip where oracle/_ref is not built."""
import numpy as np
import pytest

from handbrake_amd import hbrt
import deint_cases as dc
import oracle_lib as ol
import oracle_stream as os_

needs_ref = pytest.mark.skipif(ol.ref() is None, reason="oracle/_ref/libhbref.so not built (no /root/reference)")
TFF, BFF = 0x0008, 0x0000


@pytest.mark.parametrize("depth", dc.DEPTHS)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_reach(w, h, depth):
    total, per = dc.reach_of_shape(w, h, depth)
    for name in dc.CONTENTS:
        print(f"reach {w}x{h} depth {depth} {name}: {per[name]}")
    print(f"reach {w}x{h} depth {depth} total: {total}")
    excused = dc.REACH_EXCEPTIONS.get(((w, h), depth), {})
    for key in dc.REACH_KEYS:
        if key not in excused:
            assert total[key] >= dc.REACH_FLOOR, f"{w}x{h} depth {depth}: {key} reached {total[key]} times"
    maxv = (1 << depth) - 1
    assert dc.blend_extremes(dc.content("cells", w, h, depth)) == ((-2 * maxv) >> 3, (10 * maxv) >> 3)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("h", [4, 5, 6, 7, 9])
def test_ff_oracles_read_inside_the_plane(built, h, dtype):
    """vf_bwdif.c's mirror tests compare rows with the sample size: on a 16-bit plane of six rows or fewer its intra filter
    reaches row -1 and row h (the chroma planes of (70, 10) are five rows).  The restatements define those taps (see
    orc_bwdif_plane); held here by filtering planes that lie inside a larger buffer: what stands in the rows above and
    below the plane must not show in the output."""
    import ctypes as C
    w, guard = 19, 8
    depth = 8 if dtype == np.uint8 else 12
    rng = np.random.RandomState(h)
    planes = [rng.randint(0, 1 << depth, (h, w)).astype(dtype) for _ in range(3)]
    o = ol.oracle()
    o.orc_bwdif_plane.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6
    o.orc_yadif_ff_plane.argtypes = [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 5
    for parity in (0, 1):
        for tff in (0, 1):
            for variant in ("intra", "bwdif", "yadif", "yadif nospatial"):
                outs = []
                for fill in (0, (1 << depth) - 1):
                    bufs = [np.full((h + 2 * guard, w), fill, dtype) for _ in range(3)]
                    for b, p in zip(bufs, planes):
                        b[guard:guard + h] = p
                    at = [b.ctypes.data + guard * b.strides[0] for b in bufs]
                    dst = np.zeros((h, w), dtype)
                    tail = (dst.ctypes.data, dst.strides[0], parity, tff)
                    if variant in ("intra", "bwdif"):
                        o.orc_bwdif_plane(*at, bufs[0].strides[0], w, h, *tail, int(variant == "intra"), dst.itemsize, depth)
                    else:
                        o.orc_yadif_ff_plane(*at, bufs[0].strides[0], w, h, *tail, int(variant != "yadif"), dst.itemsize)
                    outs.append(dst)
                np.testing.assert_array_equal(outs[0], outs[1], err_msg=f"{variant} h {h} parity {parity} tff {tff}")


@needs_ref
@pytest.mark.parametrize("depth", dc.DEPTHS)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_decomb_oracle_matches_reference(built, w, h, depth):
    fmt = hbrt.PIX_FMT_FOR_DEPTH[depth]
    for name in dc.CONTENTS:
        frames = dc.content(name, w, h, depth)
        for flags in (TFF, BFF):
            for mode in dc.DECOMB_MODES:
                got = hbrt.run_stream(ol.ref(), [("hb_filter_decomb", f"mode={mode}")], frames, flags=flags,
                                      combed=dc.COMBED, pix_fmt=fmt)
                want = os_.decomb_stream(frames, dict(mode=mode, depth=depth), flags=flags, combed=dc.COMBED)
                assert len(got) == len(want)
                for t in range(len(want)):
                    what = f"{name} {w}x{h} depth {depth} mode {mode} flags {flags:#x} frame {t}"
                    assert (got[t].start, got[t].stop) == (want[t]["start"], want[t]["stop"]), what
                    for c in range(3):
                        np.testing.assert_array_equal(want[t]["planes"][c], got[t].planes[c], err_msg=f"{what} plane {c}")


@needs_ref
@pytest.mark.parametrize("depth", dc.DEPTHS)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_yadif_oracle_matches_reference_decomb_mode_1(built, w, h, depth):
    fmt = hbrt.PIX_FMT_FOR_DEPTH[depth]
    combed = [2] * dc.N_FRAMES
    compared = 0
    for name in dc.CONTENTS:
        frames = dc.content(name, w, h, depth)
        for flags in (TFF, BFF):
            ref = hbrt.run_stream(ol.ref(), [("hb_filter_decomb", "mode=1")], frames, flags=flags, combed=combed, pix_fmt=fmt)
            ours = os_.yadif_stream(frames, mode=3, flags=flags, combed=combed)
            assert len(ref) == len(ours) == dc.N_FRAMES
            for t in range(dc.N_FRAMES):
                for c in range(3):
                    ph = frames[t][c].shape[0]
                    if ph < 7:
                        continue                                         # no row with rows y +- 3 inside the plane
                    a, b = ours[t]["planes"][c][3:ph - 3], ref[t].planes[c][3:ph - 3]
                    compared += a.size
                    np.testing.assert_array_equal(a, b, err_msg=f"{name} {w}x{h} depth {depth} flags {flags:#x} frame {t} plane {c}")
    assert compared > 0
