"""The shapes and contents the BM3D tests share (tests/test_bm3d_cpu.py measures the float32 allowance on exactly what
tests/test_bm3d_gpu.py runs), and the float64 reference of each, computed once."""
import functools

import numpy as np

import bm3d_model as bm
from handbrake_amd import synth

LCW = {"2x2": (1, 1), "2x1": (1, 0), "1x1": (0, 0)}
# the smallest shapes that still exercise each edge
SHAPES = [(16, 16, "1x1"),          # one block per plane
          (17, 19, "1x1"),          # clamped origins off the 4-grid on both axes
          (36, 32, "2x2"),          # chroma 18 x 16: one clamped column, a single block row
          (72, 40, "2x1"),          # 4:2:2
          (200, 120, "2x2")]        # several tiles, tile seams
DEPTHS = [8, 10, 12]
CONTENTS = ["random", "banded", "noisy"]
NOISE_AMP = 6                       # "noisy": uniform noise of +-6 codes (at 8 bits) on the progressive picture


def plane_shapes(w, h, sub):
    lcw, lch = LCW[sub]
    cw, ch = -((-w) >> lcw), -((-h) >> lch)
    return [(h, w), (ch, cw), (ch, cw)]


def _random(w, h, sub, depth, t):
    shapes = plane_shapes(w, h, sub)
    r = synth.lcg_stream(synth.frame_seed(0x3d, t), sum(a * b for a, b in shapes)) >> np.uint32(32 - depth)
    out, at = [], 0
    for a, b in shapes:
        out.append(r[at:at + a * b].reshape(a, b).astype(np.uint8 if depth == 8 else np.uint16))
        at += a * b
    return tuple(out)


@functools.lru_cache(maxsize=None)
def content(kind, w, h, sub, depth, t=0):
    """(frame, noise-free frame or None)"""
    if kind == "random":
        return _random(w, h, sub, depth, t), None
    if kind == "banded":
        return synth.picture("banded", w, h, t, cfg=21, depth=depth, chroma=sub), None
    clean = synth.picture("progressive", w, h, t, cfg=4, depth=depth, chroma=sub)
    shapes = [p.shape for p in clean]
    amp = NOISE_AMP << (depth - 8)
    r = (synth.lcg_stream(synth.frame_seed(0x4e, t), sum(a * b for a, b in shapes)) >> np.uint32(12)).astype(np.int64)
    noisy, at = [], 0
    for p in clean:
        n = r[at:at + p.size].reshape(p.shape) % (2 * amp + 1) - amp
        at += p.size
        noisy.append(np.clip(p.astype(np.int64) + n, 0, (1 << depth) - 1).astype(p.dtype))
    return tuple(noisy), clean


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, sub, depth, sigma, t=0):
    """the float64 model's frame; shared, so leave it unchanged"""
    out = bm.bm3d_frame(content(kind, w, h, sub, depth, t)[0], f"sigma={sigma}", depth)
    for p in out:
        p.setflags(write=False)
    return out


def differences(got, want):
    """per plane: (largest |difference|, share of differing samples)"""
    out = []
    for g, w in zip(got, want):
        d = np.abs(g.astype(np.int64) - w.astype(np.int64))
        out.append((int(d.max()), float((d != 0).mean())))
    return out
