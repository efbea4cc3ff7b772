"""Device surfaces in numpy: an NV12 / P010LE picture as a block of bytes with two plane offsets and two pitches, and the
repack to and from planar 4:2:0 by the formats' definition - the oracle of bi_surface_split_kernel / bi_surface_merge_kernel
(csrc/biplanar.hip) and of the C ABI around them (include/hbhip.h, "device surfaces").

  Y[y][x]   = sample x of row y of plane 0
  Cb[y][x]  = sample 2x of row y of plane 1,  Cr[y][x] = sample 2x + 1
  depth 10  : samples are 16-bit little endian with their ten bits in the high end; planar = sample >> 6, and a merge
              writes sample << 6 (low six bits zero)

A Layout says where the planes lie: offsets and pitches in bytes, the rows each plane is allocated for.  merge() writes
[0, align16(row bytes)) of each of the height / ceil(height / 2) sample rows - the samples, and behind them what the caller
passes as the planar rows' own continuation (the frame's row padding) - and nothing else."""
import numpy as np


def align(n, a):
    return -(-n // a) * a


class Layout:
    def __init__(self, width, height, depth, pitch, offset, rows, size):
        self.width, self.height, self.depth = width, height, depth
        self.bps = 2 if depth > 8 else 1
        self.dtype = np.uint16 if depth > 8 else np.uint8
        self.cw, self.ch = (width + 1) // 2, (height + 1) // 2
        self.row_bytes = (width * self.bps, 2 * self.cw * self.bps)
        self.sample_rows = (height, self.ch)
        self.pitch, self.offset, self.rows, self.size = tuple(pitch), tuple(offset), tuple(rows), size

    def written(self):
        """mask over the block's bytes: what an export may write, [0, align16(row bytes)) of every sample row"""
        m = np.zeros(self.size, dtype=bool)
        for p in range(2):
            at = self.offset[p] + np.arange(self.sample_rows[p])[:, None] * self.pitch[p] + np.arange(align(self.row_bytes[p], 16))[None, :]
            m[at.ravel()] = True
        return m


def pooled(width, height, depth, pitch_align, rows_align, lead=0, tail=0):
    """what hbhip_surface_alloc lays out: pitch = the row rounded up to pitch_align, plane 1 at pitch * align(height,
    rows_align), half as many rows behind it; `lead` / `tail` bytes in front and behind (a larger allocation around it)"""
    bps = 2 if depth > 8 else 1
    cw = (width + 1) // 2
    pitch = (align(width * bps, pitch_align), align(2 * cw * bps, pitch_align))
    rows0 = align(height, rows_align)
    rows = (rows0, (rows0 + 1) // 2)
    offset = (lead, lead + pitch[0] * rows0)
    return Layout(width, height, depth, pitch, offset, rows, offset[1] + pitch[1] * rows[1] + tail)


def plane_rows(buf, lay, p, whole_pitch=False):
    """rows of plane p as a 2-D array of samples: the samples alone, or (whole_pitch) everything the pitch holds"""
    n = lay.pitch[p] if whole_pitch else lay.row_bytes[p]
    rows = lay.sample_rows[p]
    idx = lay.offset[p] + np.arange(rows)[:, None] * lay.pitch[p] + np.arange(n)[None, :]
    return np.ascontiguousarray(buf[idx]).view(lay.dtype)


def split(buf, lay, whole_pitch=False):
    """surface -> planar (Y, Cb, Cr)"""
    sh = 6 if lay.depth == 10 else 0
    y = plane_rows(buf, lay, 0, whole_pitch)
    c = plane_rows(buf, lay, 1, whole_pitch)
    return (y >> sh, np.ascontiguousarray(c[:, 0::2]) >> sh, np.ascontiguousarray(c[:, 1::2]) >> sh)


def merge(buf, lay, planes):
    """planar (Y, Cb, Cr) of the picture's size -> the samples of `buf`, in place; everything else of `buf` stays"""
    sh = 6 if lay.depth == 10 else 0
    y, cb, cr = (np.asarray(a, dtype=lay.dtype) for a in planes)
    assert y.shape == (lay.height, lay.width) and cb.shape == cr.shape == (lay.ch, lay.cw)
    c = np.empty((lay.ch, 2 * lay.cw), dtype=lay.dtype)
    c[:, 0::2] = cb << sh
    c[:, 1::2] = cr << sh
    for p, a in enumerate((y << sh, c)):
        raw = np.ascontiguousarray(a).view(np.uint8)
        idx = lay.offset[p] + np.arange(a.shape[0])[:, None] * lay.pitch[p] + np.arange(raw.shape[1])[None, :]
        buf[idx] = raw
    return buf
