"""What the hqdn3d tests share: the content that makes the speculative segments of handbrake_amd/csrc/hqdn3d.hip guess
wrong, and the ctypes harness that drives the filter with device-resident frames (hbhip_filter_process_dev ->
Hqdn3dFilter::process_many).  The content part needs no GPU: tests/test_hqdn3d_segments_cpu.py counts on the very same
frames how many guesses are wrong."""
import numpy as np

from handbrake_amd import synth

STRONG = ("y-spatial=14:cb-spatial=10:cr-spatial=10:y-temporal=9:cb-temporal=6:cr-temporal=6",
          dict(y_spatial=14, cb_spatial=10, cr_spatial=10, y_temporal=9, cb_temporal=6, cr_temporal=6))


def _dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def flat_noisy(w, h, n, amp=1, seed=3, depth=8):
    """Nearly flat pictures: the recurrences forget slowly here (small differences decay slowly), the
    hard case for the speculative segments of csrc/hqdn3d.hip.  depth 10 / 12: the same +- amp noise around the
    levels shifted up, 120 << (depth - 8) for luma, as uint16."""
    rng = np.random.default_rng(seed)
    e, dt = depth - 8, _dtype(depth)
    out = []
    for t in range(n):
        y = ((120 << e) + rng.integers(-amp, amp + 1, (h, w))).astype(dt)
        cb = ((128 << e) + rng.integers(-amp, amp + 1, ((h + 1) // 2, (w + 1) // 2))).astype(dt)
        cr = (((100 + (np.arange((w + 1) // 2)[None, :] // 9)) << e) + rng.integers(0, 1, ((h + 1) // 2, 1))).astype(dt)
        out.append((y, cb, cr))
    return out


def rails(w, h, depth=8):
    """Frames at the ends of the sample range: all 0, all 2^depth - 1, one-sample-wide vertical stripes 0 / max,
    top half 0 and bottom half max - jumps past the LUT's support and the values next to both ends of the 16-bit
    state range - and, fifth, top half max and bottom half 0.  At 12 bits a flat column of 4095 settles past 65535
    (the reference then stores 4096), and the temporal step from such a wrapped state to a row of 0 lands below 0
    (the reference stores 65535).  Four more frames next to the rails, see below."""
    top, dt = (1 << depth) - 1, _dtype(depth)

    def planes(fn):
        return tuple(fn(ph, pw).astype(dt) for ph, pw in ((h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2)))

    def stripes(ph, pw):
        return np.tile((np.arange(pw) & 1) * top, (ph, 1))

    def halves(ph, pw):
        return np.repeat((np.arange(ph) >= ph // 2) * top, pw).reshape(ph, pw)

    # ... and next to the rails.  Random samples within 8 codes of the top, within 8 of 0, and the first over the second.
    # Last, CLIMB: below 12 bits a vertical result passes 65535 only where a column steps down a few codes under the top
    # in the right order (each step ends up to 7 state units past the farther of state and sample): the patch below,
    # tiled, does it at 10 bits with y-spatial = 14 (tests/test_hqdn3d_segments_cpu.py counts the samples).
    rng = np.random.default_rng(depth)
    patch = np.zeros((6, 7), np.int64)
    patch[2, 6], patch[3, 6], patch[4, 6], patch[5, 5], patch[5, 6] = 3, 4, 1, 3, 3

    def climb(ph, pw):
        return top - np.tile(patch, (ph // 6 + 1, pw // 7 + 1))[:ph, :pw]

    def near_top(ph, pw):
        return top - rng.integers(0, 9, (ph, pw))

    def near_zero(ph, pw):
        return rng.integers(0, 9, (ph, pw))

    def top_over_zero(ph, pw):
        return np.where(np.arange(ph)[:, None] < ph // 2, near_top(ph, pw), near_zero(ph, pw))

    return [planes(lambda ph, pw: np.zeros((ph, pw), np.int64)), planes(lambda ph, pw: np.full((ph, pw), top, np.int64)),
            planes(stripes), planes(halves), planes(lambda ph, pw: top - halves(ph, pw)),
            planes(near_top), planes(near_zero), planes(top_over_zero), planes(climb)]


def segment_frames(w, h, depth, n=5):
    """The frames of the segment tests, 4:2:0.  The first five: 2 flat-noisy amp 1, 1 progressive, 1 flat-noisy amp 3,
    1 rails (the stripes); then 1 flat-noisy amp 1, 1 rails (the halves); beyond seven, flat-noisy pictures of
    alternating amplitude 1 / 3."""
    r = rails(w, h, depth)
    fr = (flat_noisy(w, h, 2, depth=depth) + synth.stream("progressive", w, h, 1, depth=depth)
          + flat_noisy(w, h, 1, amp=3, seed=8, depth=depth) + [r[2]]
          + flat_noisy(w, h, 1, seed=11, depth=depth) + [r[3]])
    for k in range(7, n):
        fr += flat_noisy(w, h, 1, amp=1 if k & 1 else 3, seed=20 + k, depth=depth)
    return fr[:n]


# the batched segment test: seven frames as calls of 3, 1, 2 and 1 - a batch, a single frame, the smallest batch and a
# single frame on one temporal state.  BATCHED_FRAMES: the frames that go through the batched kernels.
CALLS = (3, 1, 2, 1)
BATCHED_FRAMES = (0, 1, 2, 4, 5)


def stretch_chroma(frames, lcw, lch):
    """4:2:0 frames with the chroma planes stretched to another subsampling (sample repetition)"""
    out = []
    for y, u, v in frames:
        h, w = y.shape
        ch, cw = -(-h >> lch), -(-w >> lcw)
        u, v = (np.repeat(np.repeat(p, 2 - lch, axis=0), 2 - lcw, axis=1)[:ch, :cw] for p in (u, v))
        out.append((y, np.ascontiguousarray(u), np.ascontiguousarray(v)))
    return out


def expected_launches(calls, par):
    """{profile name: launches} of run_dev(..., pitch_align=16): a call of k frames is cut into runs of HQ_BATCH = 16; a
    run of two frames and more takes the batched kernels (hqdn3d_h, hqdn3d_v, hqdn3d_t), a run of one the frame-at-a-time
    ones (hqdn3d_h, hqdn3d_vt and, for planes without a spatial filter, hqdn3d_t)"""
    runs = [min(16, k - at) for k in calls for at in range(0, k, 16)]
    batches, singles = sum(r > 1 for r in runs), sum(r == 1 for r in runs)
    ys = par.get("y_spatial", 4.0)
    cbs = par.get("cb_spatial", 3.0 * ys / 4.0)
    on = [s != 0 for s in (ys, cbs, par.get("cr_spatial", cbs))]
    want = {"hqdn3d_t": batches + (singles if not all(on) else 0)}
    if any(on):
        want.update(hqdn3d_h=batches + singles, hqdn3d_v=batches, hqdn3d_vt=singles)
    return {k: v for k, v in want.items() if v}


def run_dev(frames, par, depth, calls, lcw=1, lch=1, pitch_align=None, launches=None):
    """hbhip_hqdn3d_create with the oracle's own tables, the frames uploaded once, then one process_dev call per entry
    of `calls` (that many frames each) on one filter, i.e. one temporal state.  Returns the downloaded output frames.

    pitch_align None: contiguous planes.  process_dev hands the caller's frames to process_many() only where every
    plane address and pitch is a multiple of 16 bytes (SimpleFilter::process_dev_batch); other frames are pushed one by
    one through pool pictures, i.e. through the frame-at-a-time kernels whatever the size of the call.
    pitch_align 16: rows padded to that many bytes, so a call of two frames and more does reach the batched kernels;
    the padding of the outputs must come back untouched.  launches: a dict that receives {profile name: launches}."""
    import ctypes as C
    import torch
    from handbrake_amd import hip
    import oracle_lib as ol

    h, w = frames[0][0].shape
    assert sum(calls) == len(frames)
    orc = ol.OrcHqdn3d(w, h, depth=depth, **par)
    dt = torch.uint8 if depth == 8 else torch.int16
    bases = []

    def plane(ph, pw, src=None):
        """a (ph, pw) device plane, zeroed or a copy of src: a view into rows of the pitch asked for"""
        es = 1 if depth == 8 else 2
        pitch = pw if not pitch_align else -(-pw * es // pitch_align) * pitch_align // es
        base = torch.zeros((ph, pitch), dtype=dt, device="cuda")
        if src is not None:
            a = np.ascontiguousarray(src)
            base[:, :pw] = torch.from_numpy(a.view(np.int16) if depth > 8 else a).cuda()
        bases.append((base, pw, src is None))
        return base[:, :pw]

    class HQ(C.Structure):
        _fields_ = [("coef", (C.c_int16 * 8192) * 6)]
    hq = HQ()
    for k in range(6):
        C.memmove(hq.coef[k], orc.coef[k], 8192 * 2)
    ctx = hip.Ctx(0)
    flt = hip._create("hbhip_hqdn3d_create", ctx, [C.c_void_p, C.POINTER(HQ)] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                      ctx.h, C.byref(hq), w, h, depth, lcw, lch)
    try:
        if launches is not None:
            ctx.profile(True)
        dev_in = [[plane(*p.shape, src=p) for p in f] for f in frames]
        outs = [[plane(*p.shape) for p in f] for f in frames]
        torch.cuda.synchronize()
        t = 0
        for b in calls:
            arr_in = (hip.DevFrame * b)(*[hip.dev_frame(dev_in[t + i]) for i in range(b)])
            arr_out = (hip.DevFrame * b)(*[hip.dev_frame(outs[t + i]) for i in range(b)])
            assert flt.process_dev(arr_in, t, arr_out) == b
            t += b
        ctx.sync()
        if launches is not None:
            launches.update({k: v[0] for k, v in ctx.profile_stats().items()})
        for base, pw, is_out in bases:
            assert not is_out or not bool(base[:, pw:].any()), "a kernel wrote into the padding of an output row"
        got = []
        for fo in outs:
            planes = [np.ascontiguousarray(p.cpu().numpy()) for p in fo]
            got.append(tuple(p.view(np.uint16) if depth > 8 else p for p in planes))
        return got
    finally:
        flt.close()
        ctx.close()
