"""The ctypes harness of the sharpen-family GPU tests (tests/test_lapsharp_wide_gpu.py, tests/test_sharpen_generic_gpu.py):
lapsharp, unsharp and chroma smooth created through the C API at any depth, one hbhip_filter_process_dev call over
device-resident planes whose rows carry junk behind the width, and the comparison with the oracle at tolerance 0."""
import ctypes as C

import numpy as np

from handbrake_amd import hip
import oracle_lib as ol
import sharpen_cases as sc

JUNK = 0x5A
CREATE = {"lapsharp": "hbhip_lapsharp_create", "unsharp": "hbhip_unsharp_create", "chroma_smooth": "hbhip_chroma_smooth_create"}


class BlurParams(C.Structure):
    _fields_ = [("amount", C.c_int * 3), ("size", C.c_int * 3)]


def lapsharp_params(kernels, strengths):
    return hip.LapsharpParams((C.c_double * 3)(*strengths), (C.c_int * 3)(*[ol.LAPSHARP_KERNELS[k] for k in kernels]))


def blur_params(strengths, sizes):
    """amount = (int)(strength * 65536.0), unsharp.c:258"""
    return BlurParams((C.c_int * 3)(*[int(s * 65536.0) for s in strengths]), (C.c_int * 3)(*sizes))


def device_plane(q, pad=0, offset=0):
    """(the plane's view, its buffer): a byte buffer filled with junk, rows of the plane's bytes rounded up to 64, plus pad,
    starting `offset` bytes in; 16-bit samples are viewed as torch.int16 (values <= 4095 fit)"""
    import torch
    ph, pw = q.shape
    es = q.dtype.itemsize
    pitch = (pw * es + 63) // 64 * 64 + pad
    buf = torch.full((ph * pitch + 64,), JUNK, dtype=torch.uint8, device="cuda")
    v, a = buf[offset:offset + ph * pitch], np.ascontiguousarray(q)
    if es == 2:
        v, a = v.view(torch.int16), a.view(np.int16)
    v = v.view(ph, pitch // es)[:, :pw]
    v.copy_(torch.from_numpy(a))
    return v, buf


def _download(v, buf):
    """(an output plane, whether its buffer holds nothing but junk around the plane's own samples)"""
    b = buf.cpu().numpy()
    ph, pw = v.shape
    es, pitch = v.element_size(), v.stride(0) * v.element_size()
    off = v.data_ptr() - buf.data_ptr()
    rows = b[off:off + ph * pitch].reshape(ph, pitch)
    q = rows[:, :pw * es].copy()
    rows[:, :pw * es] = JUNK
    return (q.view(np.uint16) if es == 2 else q), bool((b == JUNK).all())


def run_dev(flt, params, w, h, depth, frames, lcw=1, lch=1, pad=0, offset=0, launches=None):
    """frames (lists of three planes) through ONE process_dev call of a filter made by CREATE[flt]; offset moves every
    input plane's first byte.  launches: a dict that receives {profile name: launches}."""
    import torch
    ctx = hip.Ctx(0)
    f = hip._create(CREATE[flt], ctx, [C.c_void_p, C.POINTER(type(params))] + [C.c_int] * 5 + [C.POINTER(C.c_void_p)],
                    ctx.h, C.byref(params), w, h, depth, lcw, lch)
    try:
        if launches is not None:
            ctx.profile(True)
        dev_in = [[device_plane(q, pad, offset)[0] for q in fr] for fr in frames]
        outs = [[device_plane(np.zeros_like(q), pad) for q in fr] for fr in frames]
        torch.cuda.synchronize()
        n = len(frames)
        arr_in = (hip.DevFrame * n)(*[hip.dev_frame(fr) for fr in dev_in])
        arr_out = (hip.DevFrame * n)(*[hip.dev_frame([v for v, _ in o]) for o in outs])
        assert f.process_dev(arr_in, 0, arr_out) == n
        ctx.sync()
        if launches is not None:
            launches.update({k: v[0] for k, v in ctx.profile_stats().items()})
        got = []
        for o in outs:
            planes = [_download(v, buf) for v, buf in o]
            assert all(clean for _, clean in planes), f"{flt} {w}x{h} depth {depth}: a kernel wrote outside an output plane's rows"
            got.append([q for q, _ in planes])
        return got
    finally:
        f.close()
        ctx.close()


def run_job(job, launches=None):
    a, b = job.par
    params = lapsharp_params(a, b) if job.filter == "lapsharp" else blur_params(a, b)
    return run_dev(job.filter, params, job.w, job.h, job.depth, job.frames, job.lcw, job.lch, launches=launches, **job.how)


def check_job(job, guard=None, launches=None):
    """the job on the GPU against the oracle, plane by plane; chroma smooth must hand luma back as it came"""
    want = sc.expected(job)
    if guard is not None:
        guard.note(job, want)
    got = run_job(job, launches)
    for t in range(len(want)):
        for c in range(3):
            np.testing.assert_array_equal(got[t][c], want[t][c], err_msg=f"{sc.describe(job)} frame {t} plane {c}")
        if job.filter == "chroma_smooth":
            np.testing.assert_array_equal(got[t][0], job.frames[t][0], err_msg=f"{sc.describe(job)} frame {t}: luma")


def check_jobs(jobs, exempt=False):
    guard = sc.Guard()
    for job in jobs:
        check_job(job, guard)
    guard.finish(exempt)
