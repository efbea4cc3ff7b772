"""yuv420p -> p010le in numpy: the definition the widening merges (bi_widen_merge_kernel, csrc/biplanar.hip), the C ABI
around them (hbhip_frame_download_widen, hbhip_frame_export_surface_widen) and the jobs that end in `format=p010le` behind
an 8-bit 4:2:0 run are held to, at tolerance 0.  Shares no code with csrc/.

What is restated (from memory: libswscale lies outside the reference tree and no FFmpeg is at hand, so parity is UNPINNED,
as for all of DESIGN 4.6.7): yuv420p -> p010le is one of libswscale's unscaled special cases, planar8ToP01xleWrapper in
swscale_unscaled.c, not the scaler.  Its loops read every sample t of the three planes and write the 16-bit little-endian word

    t | (t << 8)

the byte twice: 0 -> 0, 255 -> 65535, and the low six bits - which P010 leaves unspecified - are NOT zero.  Range is not
looked at.  Plane 0 is Y, width x height; plane 1 is Cb Cr interleaved, Cb first.

One departure, on purpose: the wrapper's chroma loop runs width / 2 times (rounded DOWN), so for an odd width it leaves the
last Cb Cr pair of every chroma row unwritten - whatever the destination held.  There is no value to reproduce there; the
model and the kernel write that pair like every other, from the ceil(width / 2)-th chroma sample, which is the geometry of
the existing merges and of hb_frame_buffer_init's P010LE buffer: ceil(width / 2) pairs x ceil(height / 2) rows."""
import numpy as np


def widen(plane):
    """every 8-bit sample t as the word t | t << 8"""
    t = np.asarray(plane)
    assert t.dtype == np.uint8
    t = t.astype(np.uint16)
    return t | (t << 8)


def chroma_shape(width, height):
    return (height + 1) // 2, (width + 1) // 2


def merge(planes):
    """(Y, Cb, Cr) uint8 of a 4:2:0 picture -> (Y, CbCr) uint16: P010LE's two planes, rows of samples without padding"""
    y, cb, cr = planes
    h, w = y.shape
    assert cb.shape == cr.shape == chroma_shape(w, h)
    c = np.empty((cb.shape[0], 2 * cb.shape[1]), dtype=np.uint16)
    c[:, 0::2] = widen(cb)
    c[:, 1::2] = widen(cr)
    return widen(y), c


def place(buf, offset, pitch, planes):
    """the merged picture's bytes into the byte block `buf`: plane p from offset[p], rows pitch[p] apart; the samples' bytes
    only (2 * width, 4 * ceil(width / 2) a row), everything else of `buf` stays.  Returns buf."""
    for p, a in enumerate(merge(planes)):
        raw = np.ascontiguousarray(a.astype("<u2")).view(np.uint8)       # little endian: the low byte first
        idx = offset[p] + np.arange(raw.shape[0])[:, None] * pitch[p] + np.arange(raw.shape[1])[None, :]
        buf[idx] = raw
    return buf
