"""EEDI2's full-height launches leave rows alone that hold what they would store (csrc/eedi2.hip, the invariant at
Eedi2Engine::enqueue_passes; its premise on the CPU: tests/test_eedi2_copy_rows_cpu.py).  What that can get wrong and
the other scratch-plane tests do not provoke: a slot that ran another parity, or a plane that had a mask, the run
before; rows that end without padding, or in a dword that straddles the width; the other assignment of tmp2p / tmp2p2.
All nine scratch planes at their full stride against the oracle after every run."""
import numpy as np
import pytest

from handbrake_amd import hip, synth
import oracle_lib as ol

pytestmark = pytest.mark.gpu
TFF = 0x0008
MSKP = ol.EEDI2_BUFFERS.index("mskp")


def _assert_scratch(dev, oe, what):
    for b in range(9):
        for c in range(3):
            np.testing.assert_array_equal(dev.eedi_plane(b, c), oe.plane(b, c), err_msg=f"{ol.EEDI2_BUFFERS[b]} plane {c} {what}")


def _upper_chroma_only(frame):
    """`corners` with its chroma edges kept to the upper three eighths of the picture.  The edge mask clears only its
    upper half from run to run (eedi2_template.c:132): a plane with an edge lower down never loses its mask again, and
    no stream could take a slot's chroma from masked to maskless."""
    y, u, v = (p.copy() for p in frame)
    for p in (u, v):
        p[p.shape[0] * 3 // 8:] = 128
    return y, u, v


# luma rows without padding (192: flat reads past a row's end land in the next row); padding, a last dword across the
# width and a chroma width that is no multiple of 4 (130 -> 65, 322 -> 161); the smallest frame the filter takes
@pytest.mark.parametrize("w,h,confined", [(192, 108, True), (192, 108, False), (130, 76, True), (322, 184, True), (16, 16, True)])
def test_reused_slots_change_mask_and_parity(built, w, h, confined):
    """One field per pushed frame (mode 8, pulled at once): a batch of one starts at slot 0 or 1, whichever the last run
    did not end in (EediEngineBase::add_field), so consecutive runs alternate between the engine's slots 0 and 1 - its
    other slots only ever hold the later fields of longer batches - and ten runs put five into each.  The content goes
    corners, corners, interlaced, interlaced, .. and the field order flips every third frame, so each of the two slots
    sees masked -> maskless -> masked chroma and both parities, in turn."""
    n = 10
    corners, inter = synth.stream("corners", w, h, n + 1), synth.stream("interlaced", w, h, n + 1)
    if confined:
        corners = [_upper_chroma_only(f) for f in corners]
    frames = [corners[t] if (t // 2) % 2 == 0 else inter[t] for t in range(n + 1)]
    flags = [TFF if (t // 3) % 2 == 0 else 0 for t in range(n + 1)]
    ctx = hip.Ctx(0)
    dev = hip.DecombDevice(ctx, w, h, mode=8)
    oe = ol.OrcEedi2(w, h)
    masked = []
    try:
        dev.push(frames[0], flags=flags[0])
        for t in range(1, n + 1):
            dev.push(frames[t], flags=flags[t])              # processes frame t - 1
            oe.run(frames[t - 1], 1 if flags[t - 1] & TFF else 0)
            while dev.pull() is not None:
                pass
            _assert_scratch(dev, oe, f"after frame {t - 1}")
            masked.append(bool((oe.plane(MSKP, 1) == 255).any()))
        if confined and w >= 192:                            # (the case this test is about, by the oracle's mask)
            for slot in (0, 1):
                assert masked[slot::2] == [True, False, True, False, True], masked
    finally:
        oe.close()
        dev.close()
        ctx.close()


@pytest.mark.parametrize("postproc", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", [(192, 108), (130, 76)])
def test_both_plane_assignments(built, w, h, postproc):
    """post-processing 1 / 3: the direction map lives in tmp2p2 and the doubled half-height map is not stored; 0 / 2: the
    map in tmp2p, the doubled map in tmp2p2, where it stays.  Both fields of a frame per push, the order flag flipping."""
    n = 4
    frames = synth.stream("corners", w, h, n + 1)
    flags = [TFF if t % 2 == 0 else 0 for t in range(n + 1)]
    ctx = hip.Ctx(0)
    dev = hip.DecombDevice(ctx, w, h, mode=24, postproc=postproc)
    oe = ol.OrcEedi2(w, h, postproc=postproc)
    try:
        dev.push(frames[0], flags=flags[0])
        for t in range(1, n + 1):
            dev.push(frames[t], flags=flags[t])
            first = 1 if flags[t - 1] & TFF else 0
            for tff in (first, 1 - first):
                oe.run(frames[t - 1], tff)
            while dev.pull() is not None:
                pass
            _assert_scratch(dev, oe, f"after frame {t - 1}")
    finally:
        oe.close()
        dev.close()
        ctx.close()


@pytest.mark.parametrize("postproc", [0, 1])
def test_search_distance_32(built, postproc):
    """the unfused half-height path (dstp written by k_filter_map behind k_dir_map4 / k_dir_map_c) in front of the same
    full-height launches, which now read dstp where they read its doubled copy"""
    w, h, n = 322, 184, 4
    frames = synth.stream("random", w, h, n + 1)
    flags = [TFF if t % 2 == 0 else 0 for t in range(n + 1)]
    ctx = hip.Ctx(0)
    dev = hip.DecombDevice(ctx, w, h, mode=8, search=32, postproc=postproc)
    oe = ol.OrcEedi2(w, h, search=32, postproc=postproc)
    try:
        dev.push(frames[0], flags=flags[0])
        for t in range(1, n + 1):
            dev.push(frames[t], flags=flags[t])
            oe.run(frames[t - 1], 1 if flags[t - 1] & TFF else 0)
            while dev.pull() is not None:
                pass
            _assert_scratch(dev, oe, f"after frame {t - 1}")
    finally:
        oe.close()
        dev.close()
        ctx.close()
