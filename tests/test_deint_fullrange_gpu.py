"""GPU parity, tolerance 0: the deinterlacers of csrc/decomb.hip on full-range content (tests/deint_cases.py) against their
oracles - the content on which cropv() / cubic4() and bwdif's clip bind at every depth, the diagonal search (v_perm_b32 +
v_sad_u8 at 8 bits, the scalar slope() at 16) sees every +-1 / +-2 cascade and byte differences of 255, the temporal bound
d +- diff leaves [0, max] and bwdif's filters run on large operands.  tests/test_deint_fullrange_cpu.py holds the oracles to
the reference on the same streams and asserts that the contents reach all of that.

Every drop-in is driven through hbrt.run_stream as in test_decomb_gpu.py / test_yadif_gpu.py / test_bwdif_gpu.py; the modes,
field orders and parities of a (depth, shape, content) run inside one case."""
import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import deint_cases as dc
import oracle_stream as os_

pytestmark = pytest.mark.gpu
TFF, BFF = 0x0008, 0x0000

_WANT = {}


def want_decomb(name, w, h, depth, mode, flags, sub="2x2"):
    """The oracle's stream, computed once for the cases that share it."""
    key = (name, w, h, depth, mode, flags, sub)
    if key not in _WANT:
        _WANT[key] = os_.decomb_stream(dc.content(name, w, h, depth, sub=sub), dict(mode=mode, depth=depth), flags=flags,
                                       combed=dc.COMBED)
    return _WANT[key]


def check(got, want, what):
    assert len(got) == len(want), what
    for t in range(len(want)):
        for c in range(3):
            np.testing.assert_array_equal(got[t].planes[c], want[t]["planes"][c], err_msg=f"{what} frame {t} plane {c}")
        assert (got[t].start, got[t].stop) == (want[t]["start"], want[t]["stop"]), f"{what} frame {t} timestamps"


@pytest.mark.parametrize("name", dc.CONTENTS)
@pytest.mark.parametrize("depth", dc.DEPTHS)
@pytest.mark.parametrize("w,h", dc.SHAPES)
def test_decomb(built, w, h, depth, name):
    frames = dc.content(name, w, h, depth)
    for flags in (TFF, BFF):
        for mode in dc.DECOMB_MODES:
            got = hbrt.run_stream(hip.filters(), [("hb_filter_decomb_hip", f"mode={mode}")], frames, flags=flags,
                                  combed=dc.COMBED, pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[depth])
            check(got, want_decomb(name, w, h, depth, mode, flags), f"{name} {w}x{h} depth {depth} mode {mode} flags {flags:#x}")


@pytest.mark.parametrize("depth", dc.DEPTHS)
def test_decomb_in_a_chain_batch(built, depth):
    """As test_decomb_gpu.py::test_decomb_in_a_chain_batch: inside a fused chain the frames of a batch share one launch of
    decomb_plane4_kernel (grid.z over frames and planes); mode 39 mixes yadif + cubic, blend-only and copied frames in it."""
    import torch
    w, h, n = 322, 182, dc.N_FRAMES
    frames = dc.content("cells", w, h, depth)
    dt = torch.uint8 if depth == 8 else torch.uint16
    for mode in (7, 39):
        want = want_decomb("cells", w, h, depth, mode, TFF)
        ctx = hip.Ctx(0)
        dec = hip.DecombDevice(ctx, w, h, mode=mode, depth=depth)
        stage = hip.DeviceFilter(ctx, dec.h)
        dec.h = None
        chain = hip.Chain(ctx, [stage])
        try:
            dev_in = [[torch.from_numpy(np.array(p)).cuda() for p in f] for f in frames]
            cap = 2 * n + 2
            outs = [[torch.zeros(p.shape, dtype=dt, device="cuda") for p in frames[0]] for _ in range(cap)]
            torch.cuda.synchronize()
            got, t = [], 0
            for b in (n - 2, 2):
                arr_in = (hip.DevFrame * b)(*[hip.dev_frame(dev_in[t + i]) for i in range(b)])
                arr_out = (hip.DevFrame * cap)(*[hip.dev_frame(o) for o in outs])
                k = chain.process_dev(arr_in, arr_out, tag0=t, flags=[TFF] * b, combed=dc.COMBED[t:t + b])
                chain.sync()
                got += [[p.cpu().numpy().copy() for p in outs[i]] for i in range(k)]
                t += b
            arr_out = (hip.DevFrame * cap)(*[hip.dev_frame(o) for o in outs])
            k = chain.flush_dev(arr_out)
            chain.sync()
            got += [[p.cpu().numpy().copy() for p in outs[i]] for i in range(k)]
            assert len(got) == len(want)
            for i in range(len(want)):
                for c in range(3):
                    np.testing.assert_array_equal(got[i][c], want[i]["planes"][c], err_msg=f"mode {mode} frame {i} plane {c}")
        finally:
            chain.close()
            ctx.close()


@pytest.mark.parametrize("name", ["random", "cells"])
@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("w,h", [(36, 40), (260, 68)])
def test_decomb_eedi2_guided_16bit(built, w, h, depth, name):
    """Modes 15 and 31: the guess comes from the 16-bit EEDI2 engine and decomb_row4<uint16_t> bounds it to d +- diff."""
    frames = dc.content(name, w, h, depth)
    for mode in (15, 31):
        for flags in (TFF, BFF):
            got = hbrt.run_stream(hip.filters(), [("hb_filter_decomb_hip", f"mode={mode}")], frames, flags=flags,
                                  pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[depth])
            want = os_.decomb_eedi2_stream(frames, dict(mode=mode, depth=depth), flags=flags)
            check(got, want, f"{name} {w}x{h} depth {depth} mode {mode} flags {flags:#x}")


# (filter, modes, the selective mode): yadif 1 send_frame_nospatial, 3 send_frame, 5 / 7 the same with send_field (bob), + 8
# only frames marked combed; for bwdif the spatial bit means nothing
FF_FILTERS = {"yadif": ("hb_filter_yadif_hip", (1, 3, 5, 7), 15), "bwdif": ("hb_filter_bwdif_hip", (1, 3, 5, 7), 13)}
MIXED = [2, 0, 1, 0, 2]


@pytest.mark.parametrize("name", dc.CONTENTS)
@pytest.mark.parametrize("depth", dc.DEPTHS)
@pytest.mark.parametrize("w,h", dc.SHAPES)
@pytest.mark.parametrize("which", ["yadif", "bwdif"])
def test_yadif_and_bwdif(built, which, w, h, depth, name):
    symbol, modes, selective = FF_FILTERS[which]
    frames = dc.content(name, w, h, depth)
    fmt = hbrt.PIX_FMT_FOR_DEPTH[depth]
    runs = [(m, [2] * dc.N_FRAMES) for m in modes] + [(selective, MIXED)]
    for mode, combed in runs:
        # the field order from the frames' flags, top and bottom first, and forced against them by the parity setting
        for flags, parity in ((TFF, -1), (BFF, -1), (TFF, 1)):
            st = f"mode={mode}" + (f":parity={parity}" if parity >= 0 else "")
            got = hbrt.run_stream(hip.filters(), [(symbol, st)], frames, flags=flags, combed=combed, pix_fmt=fmt)
            want = os_.yadif_stream(frames, mode=mode, parity_opt=parity, flags=flags, combed=combed, bwdif=which == "bwdif",
                                    depth=depth)
            check(got, want, f"{which} {name} {w}x{h} depth {depth} {st} flags {flags:#x}")


@pytest.mark.parametrize("depth", [10, 12])
@pytest.mark.parametrize("h", [8, 10, 12])
def test_bwdif_16bit_chroma_of_six_rows_or_fewer(built, h, depth):
    """Chroma planes of 4, 5 and 6 rows at 16 bits: vf_bwdif.c's intra filter (the first field of a stream, the last of a
    bob stream) sends the +-3 tap of row 0 to row -1 and of row h - 1 to row h there; bwdif_kernel and orc_bwdif_plane take
    row y + 3 / y - 3 instead (tests/test_deint_fullrange_cpu.py holds the oracle to reading inside the plane)."""
    w = 32
    frames = dc.content("random", w, h, depth)
    combed = [2] * dc.N_FRAMES
    for mode in (3, 7):
        for flags in (TFF, BFF):
            got = hbrt.run_stream(hip.filters(), [("hb_filter_bwdif_hip", f"mode={mode}")], frames, flags=flags, combed=combed,
                                  pix_fmt=hbrt.PIX_FMT_FOR_DEPTH[depth])
            want = os_.yadif_stream(frames, mode=mode, flags=flags, combed=combed, bwdif=True, depth=depth)
            check(got, want, f"bwdif random {w}x{h} depth {depth} mode {mode} flags {flags:#x}")


@pytest.mark.parametrize("w,h", [(35, 33), (322, 182)])
@pytest.mark.parametrize("sub", ["2x1", "1x1"])
def test_other_subsamplings_10bit(built, sub, w, h):
    """4:2:2 and 4:4:4 at 10 bits: chroma planes of the full height / size, the per-plane oracles on planes of those sizes."""
    depth = 10
    frames = dc.content("cells", w, h, depth, sub=sub)
    fmt = hbrt.PIX_FMT[(sub, depth)]
    for flags in (TFF, BFF):
        got = hbrt.run_stream(hip.filters(), [("hb_filter_decomb_hip", "mode=7")], frames, flags=flags, combed=dc.COMBED, pix_fmt=fmt)
        check(got, want_decomb("cells", w, h, depth, 7, flags, sub), f"decomb 7 {sub} {w}x{h} flags {flags:#x}")
        combed = [2] * dc.N_FRAMES
        got = hbrt.run_stream(hip.filters(), [("hb_filter_bwdif_hip", "mode=7")], frames, flags=flags, combed=combed, pix_fmt=fmt)
        want = os_.yadif_stream(frames, mode=7, flags=flags, combed=combed, bwdif=True, depth=depth)
        check(got, want, f"bwdif 7 {sub} {w}x{h} flags {flags:#x}")
