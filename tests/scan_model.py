"""The title scan's per-pixel work restated: hb_detect_comb (libhb/hb.c:1088-1167) and the black-border walk of
libhb/scan.c (:456-509, :986-1052), in two forms that must agree on every case (tests/test_scan_cpu.py):

  literal_*   the reference's loops as written, one Python function per C function, each citing its lines;
  reduced_*   what the kernels of handbrake_amd/csrc/scan.hip compute: sum / min / max of the clamped samples per row and
              per column, the device-side walk over them, per-plane combing counts added up on the host.

Parity of the GPU code is pinned by THIS restatement of about 120 lines of integer C, not by the reference compiled in
place.  Pictures are (Y, Cb, Cr) uint8 arrays, 4:2:0.  A result is the tuple
(top, bottom, left, right, recorded, (cc0, cc1, cc2), average_cc, combed)."""
import numpy as np

DEFAULT_PARAMS = (10, 30, 9, 10, 30, 9)          # scan.c:973


# ---------------------------------------------------------------- literal
def clampBlack(x):
    """scan.c:450-454"""
    return 16 if x < 16 else x


def absdiff(x, y):
    """scan.c:445-448"""
    return y - x if x < y else x - y


def row_all_dark(luma, row):
    """scan.c:456-482"""
    width = len(luma[0])
    avg = 0
    for i in range(width):
        avg += clampBlack(luma[row][i])
    avg //= width
    if avg >= 32:
        return 0
    for i in range(width):
        if absdiff(avg, clampBlack(luma[row][i])) > 16:
            return 0
    return 1


def column_all_dark(luma, top, bottom, col):
    """scan.c:484-509"""
    height = len(luma) - top - bottom
    avg = 0
    for i in range(height):
        avg += clampBlack(luma[top + i][col])
    avg //= height
    if avg >= 32:
        return 0
    for i in range(height):
        if absdiff(avg, clampBlack(luma[top + i][col])) > 16:
            return 0
    return 1


def literal_crop(y_plane):
    """scan.c:986-1052: (top, bottom, left, right, recorded)"""
    luma = y_plane.tolist()
    height, width = len(luma), len(luma[0])
    h4, w4 = height // 4, width // 4
    border = height // 100
    top = border
    while top < h4:
        if not row_all_dark(luma, top):
            break
        top += 1
    if top <= border:
        top = 0
        while top < border:
            if not row_all_dark(luma, top):
                break
            top += 1
        if top >= border:
            top = 0
    bottom = border
    while bottom < h4:
        if not row_all_dark(luma, height - 1 - bottom):
            break
        bottom += 1
    if bottom <= border:
        bottom = 0
        while bottom < border:
            if not row_all_dark(luma, height - 1 - bottom):
                break
            bottom += 1
        if bottom >= border:
            bottom = 0
    left = 0
    while left < w4:
        if not column_all_dark(luma, top, bottom, left):
            break
        left += 1
    right = 0
    while right < w4:
        if not column_all_dark(luma, top, bottom, width - 1 - right):
            break
        right += 1
    recorded = int(top < h4 and bottom < h4 and left < w4 and right < w4)
    return top, bottom, left, right, recorded


def literal_detect_comb(planes, flags, color_equal, color_diff, threshold, prog_equal, prog_diff, prog_threshold):
    """hb.c:1088-1167: ((cc0, cc1, cc2), average_cc, combed)"""
    cc = [0, 0, 0]
    cc_1 = cc_2 = 0                                     # never reset between planes
    if flags & 16:
        color_diff, color_equal, threshold = prog_diff, prog_equal, prog_threshold
    for k in range(3):
        data = planes[k].tolist()
        height, width = len(data), len(data[0])
        for j in range(width):
            n = 0
            while n < height - 4:
                s1, s2, s3, s4 = data[n][j], data[n + 1][j], data[n + 2][j], data[n + 3][j]
                if abs(s1 - s3) < color_equal and abs(s1 - s2) > color_diff:
                    cc_1 += 1
                if abs(s2 - s4) < color_equal and abs(s2 - s3) > color_diff:
                    cc_2 += 1
                n += 2
        cc[k] = int((cc_1 + cc_2) * 1000.0 / (width * height))
    average_cc = (2 * cc[0] + (cc[1] // 2) + (cc[2] // 2)) // 3
    return tuple(cc), average_cc, int(average_cc > threshold)


def literal_scan(planes, flags=0, params=DEFAULT_PARAMS):
    return literal_crop(planes[0]) + literal_detect_comb(planes, flags, *params)


# ---------------------------------------------------------------- reduced
def _stats(c, axis):
    """sum, min, max of clamped samples along `axis`"""
    return c.sum(axis=axis, dtype=np.int64), c.min(axis=axis).astype(np.int64), c.max(axis=axis).astype(np.int64)


def _dark(stats, n):
    s, mn, mx = stats
    avg = s // n
    return (avg < 32) & (mx - avg <= 16) & (avg - mn <= 16)


def _first_not_dark(dark, lo, hi):
    """the first index of [lo, hi) that is not dark, else hi"""
    idx = np.flatnonzero(~dark[lo:hi])
    return lo + int(idx[0]) if idx.size else hi


def _walk_rows(dark, h4, border):
    t = _first_not_dark(dark, border, h4)
    if t <= border:
        t = _first_not_dark(dark, 0, border)
        if t >= border:
            t = 0
    return t


def reduced_crop(y_plane):
    height, width = y_plane.shape
    h4, w4, border = height // 4, width // 4, height // 100
    c = np.maximum(y_plane, 16).astype(np.int32)
    # rows [0, h4) from the top, then [0, h4) from the bottom upwards: the rows the walk can reach and no others
    dark_top = _dark(_stats(c[:h4], 1), width)
    dark_bottom = _dark(_stats(c[::-1][:h4], 1), width)
    top, bottom = _walk_rows(dark_top, h4, border), _walk_rows(dark_bottom, h4, border)
    body = c[top:height - bottom]
    n = height - top - bottom
    left = _first_not_dark(_dark(_stats(body[:, :w4], 0), n), 0, w4)
    right = _first_not_dark(_dark(_stats(body[:, ::-1][:, :w4], 0), n), 0, w4)
    return top, bottom, left, right, int(top < h4 and bottom < h4 and left < w4 and right < w4)


def comb_counts(plane, equal, diff):
    """one plane's own (cc_1, cc_2)"""
    p = plane.astype(np.int32)
    h = p.shape[0]
    n = np.arange(0, max(h - 4, 0), 2)
    if n.size == 0:
        return 0, 0
    s1, s2, s3, s4 = p[n], p[n + 1], p[n + 2], p[n + 3]
    c1 = (np.abs(s1 - s3) < equal) & (np.abs(s1 - s2) > diff)
    c2 = (np.abs(s2 - s4) < equal) & (np.abs(s2 - s3) > diff)
    return int(c1.sum()), int(c2.sum())


def scores_from_counts(counts, shapes, threshold, carry=True):
    """the host's part: counts = three (cc_1, cc_2), shapes = three (height, width).  carry=False: what the scores
    would be if the reference reset its counters per plane (it does not) - for building cases only."""
    cc, cc_1, cc_2 = [], 0, 0
    for (a, b), (h, w) in zip(counts, shapes):
        cc_1, cc_2 = (cc_1 + a, cc_2 + b) if carry else (a, b)
        cc.append(int((cc_1 + cc_2) * 1000.0 / (w * h)))
    average_cc = (2 * cc[0] + (cc[1] // 2) + (cc[2] // 2)) // 3
    return tuple(cc), average_cc, int(average_cc > threshold)


def reduced_detect_comb(planes, flags=0, params=DEFAULT_PARAMS, carry=True):
    equal, diff, threshold = params[3:6] if flags & 16 else params[0:3]
    counts = [comb_counts(p, equal, diff) for p in planes]
    return scores_from_counts(counts, [p.shape for p in planes], threshold, carry)


def reduced_scan(planes, flags=0, params=DEFAULT_PARAMS):
    return reduced_crop(planes[0]) + reduced_detect_comb(planes, flags, params)
