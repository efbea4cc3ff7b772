"""The segment schedule of handbrake_amd/csrc/hqdn3d.hip, restated in plain Python / numpy.

A restatement of the SCHEDULE, not of the kernel: how a chain is cut, what a segment guesses, what it keeps, how the
guess is verified and the segment re-walked.  No lanes, no LDS, no packed loads.  Everything is in the state domain
(samples after LOAD, denoise.c:32-33) and uses one LUT of the oracle (OrcHqdn3d.coef).

  cut rules     Hqdn3dFilter::one_frame, hqdn3d.hip:568-575: the `cut` lambda and the `gh` / `gv` line under it -
                about 64 samples a segment, at most H_SEG = 32 row segments (aligned to 16 samples) or MAX_SEG = 16
                column segments (:97-98)
                Hqdn3dFilter::process_many, :623-630: the same lambda with the targets ceil(n / HB_SEG) and
                ceil(n / VB_SEG) - HB_SEG = 8 row segments (aligned to 16), VB_SEG = 4 column segments (:249)
                both take the cut from the LUMA plane's size and use it on every plane; a segment is live where
                k * len < n (`live`, :121 and :299)
  warm-up       Hqdn3dFilter::warm = 64 (:655), HBHIP_HQDN3D_WARMUP overrides it (Hqdn3dFilter::setup, :542)
  guess         hq_h_rows :126-138: `xb = seg == 0 ? 0 : max(0, x0 - g.warm)`, the state is the sample at xb itself;
                hq_v_cols :313-325: `ys`, the same on the h-filtered column
  verify/repair the loops after the barrier, hq_h_rows :211-227 and hq_v_cols :362-379

Row chains keep their state as the reference does, in 32 bits; column chains go through the reference's uint16 line
buffer (denoise.c:126-165), so their state is truncated to 16 bits before every step.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

CENTRE = 4096
WARM = 64                                  # Hqdn3dFilter::warm
H_SEG, MAX_SEG = 32, 16                    # frame-at-a-time: row / column segments at most
HB_SEG, VB_SEG = 8, 4                      # batched
M32 = 0xffffffff

Seg = namedtuple("Seg", "seg len warm")    # HqSeg: segments per chain, samples per segment, warm-up samples
FORMS = ("row-frame", "row-batch", "col-frame", "col-batch")
EXACT, MET, END, LAST = "exact", "met", "end", "last"


def _cut(n, target, align, most, warm):
    """the `cut` lambda of one_frame / process_many"""
    seg = min(most, max(1, (n + target - 1) // target))
    length = ((n + seg - 1) // seg + align - 1) // align * align
    return Seg(seg, length, warm)


def cut(form, n, warm=WARM):
    """HqSeg of a form for a luma plane n samples wide (row-*) or high (col-*)"""
    if form == "row-frame":
        return _cut(n, 64, 16, H_SEG, warm)
    if form == "col-frame":
        return _cut(n, 64, 1, MAX_SEG, warm)
    if form == "row-batch":
        return _cut(n, (n + HB_SEG - 1) // HB_SEG, 16, HB_SEG, warm)
    if form == "col-batch":
        return _cut(n, (n + VB_SEG - 1) // VB_SEG, 1, VB_SEG, warm)
    raise ValueError(form)


def live_segments(g, n):
    return [k for k in range(g.seg) if k * g.len < n]


def lut_list(coef):
    """an OrcHqdn3d.coef table (ctypes int16[8192]) as a Python list"""
    return [int(v) for v in coef]


def to_state(plane, depth):
    """LOAD (denoise.c:32-33): sample -> 16-bit fixed point"""
    sh = 16 - depth
    return (plane.astype(np.int64) << sh) + (((1 << sh) - 1) >> 1)


def lowpass(prev, cur, lut):
    """denoise.c:96-100 in C's types: int arguments, the sum returned as uint32"""
    return (cur + lut[CENTRE + ((prev - cur) >> 4)]) & M32


def _int(v):
    """(int) of a uint32"""
    return v - (1 << 32) if v & 0x80000000 else v


def serial_chain(samples, lut, quirk=False, trunc16=False):
    """The chain as the reference walks it.  It starts from its first sample; `quirk`: row 0 of a plane starts from
    lowpass(LOAD(0), LOAD(0)) instead (denoise.c:140-146).  trunc16: the state goes through a uint16 (column chains);
    what is returned is then the truncated state, i.e. what the next step sees."""
    mask = 0xffff if trunc16 else M32
    run = samples[0]
    if quirk:
        run = lowpass(run, samples[0], lut)
    out = [run & mask]
    for x in range(1, len(samples)):
        run = lowpass(_int(run & mask), samples[x], lut)
        out.append(run & mask)
    return out


def segmented_chain(samples, lut, g, quirk=False, trunc16=False):
    """The chain as the kernels' schedule walks it.  Returns (stored samples, class of every segment boundary).

    Speculative part, segment k of the live ones, samples [x0, x1):
      k == 0   the chain's own start; nothing to guess.
      k  > 0   start at xb = max(0, x0 - warm) from the state "sample xb itself", walk to x0 keeping nothing, remember
               the state x0 is entered with (`in`), then keep every result and the state after x1 - 1 (`out`).
               Without any warm-up (xb == x0) the guessed state is sample x0 and x0 is the first step.
    Verify / repair, in segment order, `state` = the true state after the segment before:
      in[k] == state   exact: nothing to do, state = out[k]
      otherwise        re-walk from `state`; where the new state equals the stored one BEFORE the segment's last
                       sample, the rest of the segment is right as stored (met, state = out[k]); else every sample is
                       replaced and the state after the last one is handed on.
    Classes: exact / met as above; `end`: the re-walk ran out and handed on a state other than out[k]; `last`: it ran
    out but arrived at out[k] on the last sample - counted apart, it is neither of the two the tests ask shares of."""
    n = len(samples)
    mask = 0xffff if trunc16 else M32
    stored = [None] * n
    s_in, s_out = {}, {}
    live = live_segments(g, n)
    for k in live:
        x0, x1 = k * g.len, min(n, (k + 1) * g.len)
        xb = 0 if k == 0 else max(0, x0 - g.warm)
        run = samples[xb]
        if k == 0:
            if quirk:
                run = lowpass(run, samples[0], lut)
            stored[0] = run & mask
            x = 1
        elif xb == x0:
            x = x0
        else:
            x = xb + 1
        for x in range(x, x1):
            if x == x0:
                s_in[k] = run & mask
            run = lowpass(_int(run & mask), samples[x], lut)
            if x >= x0:
                stored[x] = run & mask
        s_out[k] = run & mask
    classes = []
    state = s_out[0]
    for k in live[1:]:
        x0, x1 = k * g.len, min(n, (k + 1) * g.len)
        if s_in[k] == state:
            classes.append(EXACT)
            state = s_out[k]
            continue
        run, met = state, False
        for x in range(x0, x1):
            run = lowpass(_int(run & mask), samples[x], lut) & mask
            if run == stored[x] and x + 1 < x1:
                met = True
                break
            stored[x] = run
        if met:
            classes.append(MET)
            state = s_out[k]
        else:
            classes.append(LAST if run == s_out[k] else END)
            state = run
    return stored, classes


def h_filter_plane(state_plane, lut):
    """the serial horizontal recurrence of every row (rows side by side in numpy), as int64 of the uint32 states"""
    lut_np = np.asarray(lut, np.int64)
    s = np.asarray(state_plane, np.int64)
    out = np.empty_like(s)
    run = s[:, 0].copy()
    run[0] = (run[0] + lut_np[CENTRE + ((run[0] - s[0, 0]) >> 4)]) & M32            # row 0 quirk
    out[:, 0] = run
    for x in range(1, s.shape[1]):
        prev = np.where(run & 0x80000000, run - (1 << 32), run)
        run = (s[:, x] + lut_np[CENTRE + ((prev - s[:, x]) >> 4)]) & M32
        out[:, x] = run
    return out


def v_filter_plane(h_plane, lut):
    """the serial vertical recurrence of every column of an h-filtered plane, through the reference's uint16 line
    buffer (denoise.c:126-165).  Returns the 32-bit results as SIGNED integers: what the temporal step takes; the next
    row sees their low 16 bits."""
    lut_np = np.asarray(lut, np.int64)
    hp = np.asarray(h_plane, np.int64)
    hs = np.where(hp & 0x80000000, hp - (1 << 32), hp)
    out = np.empty_like(hs)
    out[0] = hs[0]
    for y in range(1, hs.shape[0]):
        prev = out[y - 1] & 0xffff
        out[y] = hs[y] + lut_np[CENTRE + ((prev - hs[y]) >> 4)]
    return out


def chains(form, state_plane, lut):
    """(samples, quirk, trunc16) of every chain of a form on a plane: its rows, or the columns of its serially h-filtered
    plane"""
    if form.startswith("row"):
        return [([int(v) for v in row], y == 0, False) for y, row in enumerate(np.asarray(state_plane))]
    hp = h_filter_plane(state_plane, lut)
    return [([int(v) for v in col], False, True) for col in hp.T]


def plane_classes(form, state_plane, lut, warm):
    """class counts of every segment boundary of a form on one plane, {exact, met, end, last: count}; every chain is
    checked against the serial one on the way"""
    h, w = np.asarray(state_plane).shape
    g = cut(form, w if form.startswith("row") else h, warm)
    count = {EXACT: 0, MET: 0, END: 0, LAST: 0}
    for samples, quirk, t16 in chains(form, state_plane, lut):
        stored, classes = segmented_chain(samples, lut, g, quirk, t16)
        if stored != serial_chain(samples, lut, quirk, t16):
            raise AssertionError(f"{form} warm {warm}: the segmented walk differs from the serial chain")
        for c in classes:
            count[c] += 1
    return count
