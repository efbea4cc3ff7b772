"""GPU parity of the tail of EEDI2's full-height map (fill_gaps_2x twice, the lattice candidates and their resolve pass)
on widths that are not multiples of the kernels' spans: fill_gaps and the candidates take 1024 pixels per workgroup,
the resolve pass 256 pixels per pass of a wave.  Every scratch frame against the oracle after each pushed frame, both
field parities (mode 24 runs tff=1, then tff=0), on content that leaves the mask sparse and content that makes it dense."""
import numpy as np
import pytest

from handbrake_amd import hip, synth
import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model,w,h,n", [("interlaced", 1918, 120, 3), ("corners", 1000, 96, 3), ("random", 4096, 64, 3),
                                         ("random", 1000, 96, 4), ("interlaced", 1918, 120, 6), ("corners", 1918, 96, 4)])
def test_tail_passes_every_scratch_buffer(built, model, w, h, n):
    frames = synth.stream(model, w, h, n)
    ctx = hip.Ctx(0)
    dev = hip.DecombDevice(ctx, w, h, mode=24)
    oe = ol.OrcEedi2(w, h)
    try:
        dev.push(frames[0])                      # first frame only primes the ring
        for t in range(1, n):
            dev.push(frames[t])                  # processes frame t-1: fields tff=1 then tff=0
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
