"""Detelecine (pullup) cases: a synthetic stream, its per-picture flags and a settings string each.

tests/golden/make_detelecine_golden.py runs them through the reference's own filter and records the outputs as
tests/golden/detelecine_<name>.npz; tests/test_detelecine_cpu.py holds tests/pullup_model.py to those recordings and
tests/test_detelecine_gpu.py the HIP drop-in to both.
"""
from __future__ import annotations

import os

import numpy as np

from handbrake_amd import hbrt, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIC_FLAG_TOP_FIELD_FIRST = synth.PIC_FLAG_TOP_FIELD_FIRST
PIC_FLAG_PROGRESSIVE_FRAME = synth.PIC_FLAG_PROGRESSIVE_FRAME
PIC_FLAG_REPEAT_FIRST_FIELD = synth.PIC_FLAG_REPEAT_FIRST_FIELD
DURATION = 3003


def cadence(n_src: int, start: int = 3):
    """3:2 pulldown field counts for n_src source frames"""
    return [start if k % 2 == 0 else 5 - start for k in range(n_src)]


def _hard(w=128, h=64, n_src=20, top_first=True, cuts=(), depth=8, chroma="2x2", durations=None):
    return lambda: synth.telecine_stream(w, h, durations or cadence(n_src), cuts=cuts, top_first=top_first,
                                         depth=depth, chroma=chroma)


def _soft(w=128, h=64, n_src=24, depth=8, chroma="2x2"):
    return lambda: synth.telecine_stream(w, h, cadence(n_src), soft=[True] * n_src, depth=depth, chroma=chroma)


def _plain(model, w=128, h=64, n=24, depth=8, chroma="2x2"):
    flag = PIC_FLAG_PROGRESSIVE_FRAME if model == "progressive" else PIC_FLAG_TOP_FIELD_FIRST

    def make():
        frames = [synth.picture(model, w, h, t, cfg=2 if model == "progressive" else 3, depth=depth, chroma=chroma)
                  for t in range(n)]
        return frames, [flag] * n
    return make


# name -> (stream builder, depth, chroma layout, settings)
CASES = {
    "hard_tff":          (_hard(), 8, "2x2", ""),
    "hard_bff":          (_hard(top_first=False), 8, "2x2", ""),
    "soft_rff":          (_soft(), 8, "2x2", ""),
    "broken_cadence":    (_hard(durations=[3, 2, 3, 2, 3, 2, 2, 3, 2, 3, 3, 2, 3, 2, 2, 2, 3, 2, 3, 2], cuts=(6, 13)),
                          8, "2x2", ""),
    "progressive":       (_plain("progressive"), 8, "2x2", ""),
    "interlaced":        (_plain("interlaced"), 8, "2x2", ""),
    "strict_breaks":     (_hard(cuts=(9,)), 8, "2x2", "strict-breaks=1"),
    "plane1":            (_hard(), 8, "2x2", "plane=1:skip-top=2:skip-bottom=2"),
    "parity0":           (_hard(top_first=False), 8, "2x2", "parity=0"),
    "parity1":           (_hard(), 8, "2x2", "parity=1"),
    "skips":             (_hard(w=160, h=96), 8, "2x2", "skip-left=3:skip-right=2:skip-top=6:skip-bottom=5"),
    "width_odd8":        (_hard(w=134), 8, "2x2", ""),
    "hard_10bit":        (_hard(depth=10), 10, "2x2", ""),
    "soft_12bit":        (_soft(depth=12), 12, "2x2", ""),
    "hard_422":          (_hard(chroma="2x1"), 8, "2x1", ""),
    "hard_444_10bit":    (_hard(chroma="1x1", depth=10), 10, "1x1", "plane=2"),
}


def pix_fmt(depth: int, chroma: str) -> int:
    return hbrt.PIX_FMT[(chroma, depth)]


def build(name: str):
    make, depth, chroma, settings = CASES[name]
    frames, flags = make()
    return frames, flags, depth, chroma, settings


def run_chain(lib, symbol: str, settings: str, frames, flags, depth: int, chroma: str):
    """Every picture through one filter object of `lib` (its own flags, 90 kHz times by index), then EOF."""
    h, w = frames[0][0].shape
    out = []
    with hbrt.Chain(lib, [(symbol, settings)], w, h, pix_fmt(depth, chroma)) as ch:
        for i, (fr, fl) in enumerate(zip(frames, flags)):
            ch.push(fr, start=i * DURATION, stop=(i + 1) * DURATION, flags=fl)
            out += ch.drain()
        ch.push_eof()
        out += ch.drain()
    return out


def expected(name: str):
    """What the model makes of a case: list of (planes, (start, stop, flags))."""
    import pullup_model as pm
    frames, flags, depth, chroma, settings = build(name)
    return [(planes, (i * DURATION, (i + 1) * DURATION, flags[i])) for i, planes in pm.run(frames, flags, depth, settings)]


def load_golden(name: str):
    """The reference's outputs recorded for a case: list of (planes, (start, stop, flags))."""
    z = np.load(os.path.join(GOLDEN, f"detelecine_{name}.npz"))
    return [(tuple(z[f"f{t}_p{c}"] for c in range(3)), tuple(int(v) for v in z[f"f{t}_meta"]))
            for t in range(int(z["nframes"]))]


def seeded_stream(seed: int, n: int, w: int, h: int, depth: int = 8, chroma: str = "2x2"):
    """A long telecined stream: 3:2 cadence with random breaks (a source frame of 2 fields where 3 were due or the
    other way round), scene cuts, and runs of soft pulldown (RFF) between runs of hard telecine; about n pictures."""
    rng = np.random.default_rng(seed)
    durations, soft, cuts = [], [], set()
    want, in_soft = 3, False
    while sum(durations) < 2 * n:
        d = want
        if rng.random() < 0.08:
            d = 5 - d                                  # a break in the cadence
        if rng.random() < 0.05:
            cuts.add(len(durations))
        if rng.random() < 0.1:
            in_soft = not in_soft
        durations.append(d)
        soft.append(in_soft)
        want = 5 - want
    frames, flags = synth.telecine_stream(w, h, durations, soft=soft, cuts=cuts, depth=depth, chroma=chroma,
                                          cfg=2 + seed % 5)
    return frames[:n], flags[:n]
