"""Independent numpy model of FFmpeg's `deblock` filter as libhb's deblock.c configures it.

FFmpeg's source is not in the reference tree, so this restates it: the loop order is certain, the tap divisors
(WEAK_DIV / STRONG_DIV) and the strong filter's fifth skip test are recalled - csrc/deblock.hip keeps the same two tables.

Two forms of the plane filter:
  * deblock_plane_raster - a literal transcription of FFmpeg's filter_frame loop, one edge at a time (slow: small sizes);
  * deblock_plane        - per block row: the horizontal edge across all columns at once, then the vertical edges of the
                           block row's rows (all at once where windows cannot overlap, left to right where they can).
And the settings resolution: deblock.c's doubles -> "%g" -> float option -> (int)(option * max).
"""
from __future__ import annotations

import numpy as np

WEAK_DIV = (8, 2, 2, 8)            # A += d/8, B += d/2, C -= d/2, D -= d/8      (d = C - B)
STRONG_DIV = (8, 4, 2, 2, 4, 8)    # A += d/8, B += d/4, C += d/2, D -= d/2, E -= d/4, F -= d/8   (d = D - C)
DEFAULT_ALPHA, DEFAULT_BGD = 0.098, 0.05   # FFmpeg's defaults for what deblock.c leaves unset


class Declined(Exception):
    pass


def _option(v: float) -> np.float32:
    """a double as hb_dict hands it on ("%g") and as FFmpeg parses it back into a float option"""
    return np.float32(float("%g" % v))


def thresholds(thresh, depth: int):
    """(ath, bth, gth, dth) for deblock.c's integer `thresh` (None / <= 0: FFmpeg's defaults)"""
    maxv = np.float32((1 << depth) - 1)
    if thresh is not None and thresh > 0:
        a = thresh * 0.010
        alpha, bgd = _option(a), _option(a / 2)
        if alpha > 1 or bgd > 1:
            raise Declined(f"thresh {thresh} past the options' range")
    else:
        alpha, bgd = np.float32(DEFAULT_ALPHA), np.float32(DEFAULT_BGD)
    ath, bth = int(np.float32(alpha * maxv)), int(np.float32(bgd * maxv))
    return ath, bth, bth, bth


def plane_ok(size: int, b: int, strong: bool) -> bool:
    if size <= b:
        return True
    r = size % b
    return r not in ((1, 2) if strong else (1,))


def resolve(settings: str, depth: int, plane_sizes=()):
    """deblock.c's settings string -> dict(strong, block, thr); Declined for what the drop-in declines"""
    kv = dict(p.split("=", 1) for p in settings.split(":") if p)
    strength = kv.get("strength")
    if strength is None:
        strong = True
    elif strength in ("weak", "strong"):
        strong = strength == "strong"
    else:
        raise Declined(f"unknown strength {strength!r}")
    b = int(kv.get("blocksize", 8))
    if not 4 <= b <= 512:
        raise Declined(f"blocksize {b}")
    thr = thresholds(int(kv["thresh"]) if "thresh" in kv else None, depth)
    for w, h in plane_sizes:
        if not (plane_ok(w, b, strong) and plane_ok(h, b, strong)):
            raise Declined(f"plane {w}x{h}, block {b}")
    return dict(strong=strong, block=b, thr=thr)


def _div(d, n):
    """C int division: truncates towards zero"""
    return np.sign(d) * (np.abs(d) // n)


def edge(win, strong: bool, thr, maxv: int):
    """filter windows win[..., taps] (int64) across their middle; returns (new windows, fired mask)"""
    ath, bth, gth, dth = thr
    v = [win[..., k] for k in range(win.shape[-1])]
    if strong:
        d = v[3] - v[2]
        fire = (np.abs(d) < ath) & (np.abs(v[2] - v[1]) < bth) & (np.abs(v[3] - v[4]) < gth) & \
               (np.abs(v[1] - v[0]) < dth) & (np.abs(v[4] - v[5]) < dth)
        sign = (1, 1, 1, -1, -1, -1)
        new = [v[k] + sign[k] * _div(d, STRONG_DIV[k]) for k in range(6)]
    else:
        d = v[2] - v[1]
        fire = (np.abs(d) < ath) & (np.abs(v[1] - v[0]) < bth) & (np.abs(v[2] - v[3]) < gth)
        sign = (1, 1, -1, -1)
        new = [v[k] + sign[k] * _div(d, WEAK_DIV[k]) for k in range(4)]
    new = np.clip(np.stack(new, axis=-1), 0, maxv)
    return np.where(fire[..., None], new, win), fire


def deblock_plane_raster(plane, b: int, strong: bool, thr, depth: int, stats=None):
    """FFmpeg's filter_frame loop, literally"""
    out = plane.astype(np.int64).copy()
    h, w = out.shape
    L = 3 if strong else 2
    maxv = (1 << depth) - 1
    fired = [0, 0]

    def one(idx):
        new, f = edge(out[idx][None, :], strong, thr, maxv)
        out[idx] = new[0]
        fired[0] += int(f[0])
        fired[1] += 1

    def vert_edge(x, y0, n):
        for r in range(y0, y0 + n):
            one((r, slice(x - L, x + L)))

    def horz_edge(y, x0, n):
        for c in range(x0, x0 + n):
            one((slice(y - L, y + L), c))

    for x in range(b, w, b):
        vert_edge(x, 0, min(b, h))
    for y in range(b, h, b):
        horz_edge(y, 0, min(b, w))
        for x in range(b, w, b):
            horz_edge(y, x, min(b, w - x))
            vert_edge(x, y, min(b, h - y))
    if stats is not None:
        stats["fired"], stats["edges"] = stats.get("fired", 0) + fired[0], stats.get("edges", 0) + fired[1]
    return out.astype(plane.dtype)


def deblock_plane(plane, b: int, strong: bool, thr, depth: int, stats=None):
    """per block row: its horizontal edge over all columns, then the vertical edges of its rows"""
    out = plane.astype(np.int64).copy()
    h, w = out.shape
    L = 3 if strong else 2
    maxv = (1 << depth) - 1
    xs = np.arange(b, w, b)
    overlap = 2 * L > b
    fired = edges = 0
    for y in range(0, h, b):
        if y > 0:
            new, f = edge(out[y - L:y + L, :].T, strong, thr, maxv)
            out[y - L:y + L, :] = new.T
            fired, edges = fired + int(f.sum()), edges + f.size
        rows = slice(y, min(y + b, h))
        if len(xs) == 0:
            continue
        if overlap:
            for x in xs:
                new, f = edge(out[rows, x - L:x + L], strong, thr, maxv)
                out[rows, x - L:x + L] = new
                fired, edges = fired + int(f.sum()), edges + f.size
        else:
            cols = xs[:, None] + np.arange(-L, L)[None, :]
            new, f = edge(out[rows][:, cols], strong, thr, maxv)
            sub = out[rows]
            sub[:, cols] = new
            out[rows] = sub
            fired, edges = fired + int(f.sum()), edges + f.size
    if stats is not None:
        stats["fired"], stats["edges"] = stats.get("fired", 0) + fired, stats.get("edges", 0) + edges
    return out.astype(plane.dtype)


def deblock_frame(planes, settings: str, depth: int, stats=None):
    """a whole frame through the model (the drop-in's settings string); Declined as the drop-in declines"""
    p = resolve(settings, depth, [pl.shape[::-1] for pl in planes])
    return tuple(deblock_plane(pl, p["block"], p["strong"], p["thr"], depth, stats) for pl in planes)


PRESETS = {"ultralight": "strength=weak:thresh=20", "light": "strength=weak:thresh=50",
           "medium": "strength=strong:thresh=20", "strong": "strength=strong:thresh=50",
           "stronger": "strength=strong:thresh=75", "verystrong": "strength=strong:thresh=100"}
TUNES = {"small": "blocksize=4", "medium": "", "large": "blocksize=16"}


def settings_for(preset: str, tune: str = "medium") -> str:
    return ":".join(s for s in (PRESETS[preset], TUNES[tune]) if s)
