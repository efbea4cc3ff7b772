"""Frames through one device filter in device-resident bursts (one process_dev call each): what the GPU tests of the
one-in / one-out filters share.  Not a conftest: import it."""
import numpy as np

from handbrake_amd import hip


def bursts(make_filter, frames, sizes, pads=(0,), depth=8, out_shape=None, setup=None, out_depth=None, ctx=None,
           out_row_bytes=1):
    """`frames` (tuples of three numpy planes) through make_filter(ctx) in bursts of the given sizes; input i's rows are
    padded by pads[i % len(pads)] samples, so that pitches mix inside a burst.  Returns the output frames as lists of
    numpy planes, or None when setup(flt) - a knob of the filter's, applied once - returns a non-zero code.
    out_shape: the (height, width) of the output luma where it differs from the input's (pad); out_depth: the output's
    depth where it differs (format); ctx: a context of the caller's, left open (its profile, say), else one of its own;
    out_row_bytes: the output rows' pitch is rounded up to a multiple of this (a 40-byte chroma row on a 16-byte pitch)."""
    import torch
    tdt = lambda d: torch.int16 if d > 8 else torch.uint8
    conv = lambda t: t.cpu().numpy().view(np.uint16) if t.dtype == torch.int16 else t.cpu().numpy()
    out_depth = depth if out_depth is None else out_depth
    assert frames[0][0].dtype == (np.uint16 if depth > 8 else np.uint8)
    own = ctx is None
    ctx = hip.Ctx(0) if own else ctx
    flt = make_filter(ctx)
    out = []
    try:
        if setup is not None and setup(flt) != 0:
            return None
        at = 0
        for n in sizes:
            part = frames[at:at + n]
            dev_in, keep = [], []
            for i, f in enumerate(part):
                pad = pads[(at + i) % len(pads)]
                planes = []
                for p in f:
                    p = np.array(p)
                    full = torch.zeros((p.shape[0], p.shape[1] + pad), dtype=tdt(depth), device="cuda")
                    full[:, :p.shape[1]] = torch.from_numpy(p.view(np.int16) if depth > 8 else p).cuda()
                    keep.append(full)
                    planes.append(full[:, :p.shape[1]])
                dev_in.append(planes)
            at += n
            shapes = [p.shape for p in part[0]]
            if out_shape is not None:                                    # the chroma planes grow by the luma's ratio
                shapes = [(s[0] * out_shape[0] // shapes[0][0], s[1] * out_shape[1] // shapes[0][1]) for s in shapes]
            unit = max(1, out_row_bytes // (2 if out_depth > 8 else 1))                     # in samples
            outs = [[torch.full((s[0], -(-s[1] // unit) * unit), 7, dtype=tdt(out_depth), device="cuda")[:, :s[1]] for s in shapes]
                    for _ in part]
            torch.cuda.synchronize()
            arr_in = (hip.DevFrame * n)(*[hip.dev_frame(f) for f in dev_in])
            arr_out = (hip.DevFrame * n)(*[hip.dev_frame(o) for o in outs])
            assert flt.process_dev(arr_in, 0, arr_out) == n
            ctx.sync()
            out += [[conv(p) for p in o] for o in outs]
            for f, d in zip(part, dev_in):                               # out of place: the inputs are untouched
                for c in range(3):
                    np.testing.assert_array_equal(conv(d[c]), f[c])
        return out
    finally:
        flt.close()
        if own:
            ctx.close()
