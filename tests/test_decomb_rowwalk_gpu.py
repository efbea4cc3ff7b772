"""GPU parity, tolerance 0: decomb mode 31 (EEDI2-guided yadif, bob) on device-resident frames against the oracle, at the
sizes where decomb_rowwalk8_kernel (csrc/decomb.hip) changes path.  A thread walks the R = 8 rebuilt rows of a strip of
2 R = 16 rows; strips that touch the first / last three rows of a plane go row by row through decomb_row4.  Heights (luma;
chroma has half): no strip walks (16, 24), one does (4 R + 4 = 36, 4 R + 8 - for one field parity only in chroma -, the strip
behind it cut short), several do (68, 100).  Bob gives both field parities, TFF / BFF both field orders, and the first and
last frames filter against themselves.  The EEDI2 engine takes no picture below 16 x 16 (EediEngineBase::init_slots: the
reference overruns its scratch planes there), so at heights 8 and 12 and at width 4 there is nothing to walk: what is held
there is that the filter still says so when it is created; 16 and 24 rows and 16 / 20 columns are the smallest that run."""
import numpy as np
import pytest

from handbrake_amd import hip, synth
import oracle_stream as os_

pytestmark = pytest.mark.gpu

R = 8                                                                 # decomb.hip: DW_R
TFF, BFF = 0x0008, 0
N = 5


def _frames(content, w, h):
    if content == "checker":
        def plane(pw, ph, t):
            return ((np.add.outer(np.arange(ph), np.arange(pw)) + t) & 1).astype(np.uint8) * 255
        return [(plane(w, h, t), plane(w // 2, h // 2, t // 2), plane(w // 2, h // 2, t)) for t in range(N)]
    return synth.stream(content, w, h, N)


def _refused(w, h):
    return w < 16 or h < 16 or h % 4


def _decomb31(w, h, frames, flags):
    import torch
    ctx = hip.Ctx(0)
    dec = hip.DecombDevice(ctx, w, h, mode=31, postproc=1)
    stage = hip.DeviceFilter(ctx, dec.h)
    dec.h = None
    chain = hip.Chain(ctx, [stage])
    try:
        n = len(frames)
        dev_in = [[torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in f] for f in frames]
        cap = 2 * n + 2
        outs = [[torch.zeros((h, w), dtype=torch.uint8, device="cuda"),
                 torch.zeros((h // 2, w // 2), dtype=torch.uint8, device="cuda"),
                 torch.zeros((h // 2, w // 2), dtype=torch.uint8, device="cuda")] for _ in range(cap)]
        torch.cuda.synchronize()
        arr_in = (hip.DevFrame * n)(*[hip.dev_frame(f) for f in dev_in])
        arr_out = (hip.DevFrame * cap)(*[hip.dev_frame(o) for o in outs])
        k = chain.process_dev(arr_in, arr_out, tag0=0, flags=[flags] * n, combed=[2] * n)
        chain.sync()
        got = [[p.cpu().numpy().copy() for p in outs[i]] for i in range(k)]
        arr_out = (hip.DevFrame * cap)(*[hip.dev_frame(o) for o in outs])
        k = chain.flush_dev(arr_out)
        chain.sync()
        return got + [[p.cpu().numpy().copy() for p in outs[i]] for i in range(k)]
    finally:
        chain.close()
        ctx.close()


@pytest.mark.parametrize("flags", [TFF, BFF], ids=["tff", "bff"])
@pytest.mark.parametrize("w", [4, 16, 20, 36, 260])
@pytest.mark.parametrize("h", [8, 12, 16, 24, 4 * R + 4, 4 * R + 8, 68, 100])
def test_mode31(built, w, h, flags):
    if _refused(w, h):
        ctx = hip.Ctx(0)
        try:
            with pytest.raises(hip.HipError, match="not supported"):
                hip.DecombDevice(ctx, w, h, mode=31, postproc=1)
        finally:
            ctx.close()
        return
    for content in ("interlaced", "random", "checker"):
        frames = _frames(content, w, h)
        want = os_.decomb_eedi2_stream(frames, dict(mode=31, postproc=1), flags=flags)
        got = _decomb31(w, h, frames, flags)
        assert len(got) == len(want) == 2 * N
        for i in range(len(want)):
            for c in range(3):
                np.testing.assert_array_equal(got[i][c], want[i]["planes"][c], err_msg=f"{content} {w}x{h} frame {i} plane {c}")
