"""GPU parity of EEDI2's calc_directions (k_calc_dir_rows / q_calc_dir_rows: the dense row walk and the list form) where
its blocks are cut: field heights whose last block of rows is partial, dense blocks next to the bottom edge, blocks whose
pixels take every step beside pixels that leave some out (the poisoned steps of the dense form), and search distances up
to the LDS halo's limit - every scratch plane against the oracle, at 8 and 10 bits."""
import numpy as np
import pytest

from handbrake_amd import hip, synth
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _parity(model, w, h, n, depth=8, search=None):
    frames = synth.stream(model, w, h, n, depth=depth)
    kw = {} if search is None else {"search": search}
    ctx = hip.Ctx(0)
    dev = hip.DecombDevice(ctx, w, h, mode=24, depth=depth, **kw)
    oe = ol.OrcEedi2(w, h, **kw) if depth == 8 else ol.OrcEedi2_16(w, h, depth, **kw)
    try:
        dev.push(frames[0])
        for t in range(1, n):
            dev.push(frames[t])
            for tff in (1, 0):
                oe.run(frames[t - 1], tff)
            while dev.pull() is not None:
                pass
            for b in range(9):
                for c in range(3):
                    np.testing.assert_array_equal(dev.eedi_plane(b, c), oe.plane(b, c),
                                                  err_msg=f"{ol.EEDI2_BUFFERS[b]} plane {c} after frame {t - 1}")
    finally:
        oe.close()
        dev.close()
        ctx.close()


# field heights (h / 2 luma, h / 4 chroma) that leave every remainder 0 .. 3 of a block of four rows: 180 -> 90 / 45,
# 184 -> 92 / 46, 188 -> 94 / 47, 196 -> 98 / 49.  Noise fills the mask at once, so the last dense block of a plane is
# the one just above the bottom edge rows.
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("h", [180, 184, 188, 196])
def test_partial_last_block_dense(built, depth, h):
    _parity("random", 320, h, 3, depth=depth)


# widths that are not a multiple of the 256-column block (the search range is clipped at the right edge: those pixels
# leave steps out) on content whose mask is dense in some blocks and sparse in others
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("model,w,h,n", [("corners", 600, 188, 4), ("interlaced", 322, 196, 5)])
def test_mixed_step_sets(built, depth, model, w, h, n):
    _parity(model, w, h, n, depth=depth)


# the widest windows the tiled kernels take (CD_HALO - 2 = 30 luma, 15 chroma) and odd ones (chroma halves them)
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("search", [30, 29, 17, 3])
def test_search_distances_dense(built, depth, search):
    _parity("random", 384, 188, 3, depth=depth, search=search)
