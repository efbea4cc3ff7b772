"""The NV12 / P010LE compositor cases tests/test_biplanar_cpu.py and tests/test_biplanar_gpu.py share.

Placements are the ones the reference stays inside its buffers on, and inside the two departures of the kernels
(csrc/blend.hip:16-19), by the functions' own index arithmetic:
  same subsampling (YUVA420P overlays, blend8onbi* :606-786): fully inside (odd origin too: chroma goes to (left >> 1) + xx
      >= 0); over the left / top edge by an EVEN amount (x0 = -left, chroma starts at x0 >> 1 = -(left >> 1): index 0 - an
      odd amount gives index -1, the stray write); over the right / bottom edge (ww / hh are clamped to the frame, :628-637).
  4:4:4 overlays (blend_subsample_8onbi* :142-423): fully inside only - `width` is clamped for left == x0 alone (:167), so
      anything over an edge runs past the row.  Odd origins and odd sizes: the overlay starts and ends inside chroma blocks.
Three overlays a case, the second on top of the first."""
import numpy as np

NV12, P010LE = 23, 158
YUVA420P, YUVA444P = 33, 79
DEPTH = {NV12: 8, P010LE: 10}


def frame(pix_fmt, w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if pix_fmt == NV12:
        return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, 2 * cw), dtype=np.uint8))
    return ((rng.integers(0, 1024, (h, w)) << 6).astype(np.uint16), (rng.integers(0, 1024, (ch, 2 * cw)) << 6).astype(np.uint16))


def overlay(x, y, ow, oh, subsampled, seed):
    rng = np.random.default_rng(seed)
    cw, ch = ((ow + 1) // 2, (oh + 1) // 2) if subsampled else (ow, oh)
    a = rng.integers(0, 256, (oh, ow), dtype=np.uint8)
    gx, gy = np.arange(ow)[None, :], np.arange(oh)[:, None]
    a[(gx // 5 + gy // 3) % 4 == 0] = 0                # transparent, opaque and soft areas
    a[(gx // 7 + gy // 4) % 5 == 1] = 255
    return (x, y, (rng.integers(0, 256, (oh, ow), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
                   rng.integers(0, 256, (ch, cw), dtype=np.uint8), a))


def overlays(w, h, overlay_fmt, seed=0):
    if overlay_fmt == YUVA420P:
        return [overlay(7, 5, 24, 12, True, seed + 1),                 # inside, odd origin
                overlay(-4, -2, 30, 16, True, seed + 2),               # over the left / top edge by an even amount, on the first
                overlay(w - 18, h - 9, 26, 14, True, seed + 3)]        # over the right / bottom edge
    return [overlay(7, 5, 24, 13, False, seed + 1),                    # ends at an odd column
            overlay(20, 10, 30, 15, False, seed + 2),                  # on the first; ends at an odd row
            overlay(w - 21, h - 11, 21, 11, False, seed + 3)]          # touches the right / bottom edge


def nine_disjoint(w, h, overlay_fmt, seed=0):
    """more than BL_GROUP = 8 overlays that share no part of the frame: two launches (csrc/blend.hip: build_launches)"""
    sub = overlay_fmt == YUVA420P
    return [overlay(4 + (w // 3) * i, 3 + (h // 3) * j, 30, 20, sub, seed + 10 + 3 * j + i) for j in range(3) for i in range(3)]


SHIFTS = {YUVA420P: (1, 1), YUVA444P: (0, 0)}
CASES = [(pf, of, loc) for pf in (NV12, P010LE) for of in (YUVA420P, YUVA444P) for loc in (1, 2, 3)]
