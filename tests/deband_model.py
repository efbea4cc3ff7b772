"""Independent numpy model of FFmpeg's `deband` filter as libhb's deband.c configures it.

FFmpeg's source is not in the reference tree, so this restates it: deband.c's keys and defaults are certain, FFmpeg's
option ranges, offset table and per-sample rule are recalled - csrc/deband.hip keeps the same in one place too.

The offset table calls libm's own sinf / cosf / floorf through ctypes, one position at a time, and rounds to float32 at
every step: the hash multiplies sinf's result by 43758.5, so numpy's float32 sin (another implementation) would move
offsets.  A 1080p table takes seconds, so tables are cached per (W, H, range, direction).

Two forms of the plane filter:
  * deband_plane_loop - per sample, literally (slow: small planes);
  * deband_plane      - the same with numpy fancy indexing.
And the settings resolution: deband.c's doubles -> "%g" -> the option's range check -> float option -> thresholds.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

# ---- the recalled part, in one place (csrc/deband.hip keeps the same) ------------------------------------------------
HASH_X, HASH_Y, HASH_SCALE = np.float32(12.9898), np.float32(78.233), np.float32(43758.545)
THR_MIN, THR_MAX = 0.00003, 0.5                     # FFmpeg's range of 1thr .. 4thr
DIRECTION = np.float32(2 * math.pi)                 # FFmpeg's default direction, stored as a float
RANGE_MAX = 1 << 30                                 # past this the drop-in declines (INT_MIN has no -range)
DEFAULTS = dict(thr=(0.02, 0.02, 0.02, 0.02), range=16, blur=1)   # deband.c:52-53


def avg4(r0, r1, r2, r3):
    return (r0 + r1 + r2 + r3) // 4


def decide(s, r0, r1, r2, r3, thr, blur):
    """FFmpeg's per-sample rule (works elementwise on arrays and on ints)"""
    avg = avg4(r0, r1, r2, r3)
    if blur:
        return np.where(np.abs(s - avg) < thr, avg, s)
    ok = (np.abs(s - r0) < thr) & (np.abs(s - r1) < thr) & (np.abs(s - r2) < thr) & (np.abs(s - r3) < thr)
    return np.where(ok, avg, s)


class Declined(Exception):
    pass


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _fn in ("sinf", "cosf", "floorf"):
    getattr(_libm, _fn).restype = ctypes.c_float
    getattr(_libm, _fn).argtypes = [ctypes.c_float]
_sinf, _cosf, _floorf = _libm.sinf, _libm.cosf, _libm.floorf
_TABLES: dict = {}


def offsets(W: int, H: int, rng: int = 16, direction=DIRECTION):
    """FFmpeg's (x_pos, y_pos) tables, int64 arrays of shape (H, W)"""
    direction = np.float32(direction)
    key = (W, H, rng, float(direction))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    x = np.arange(W, dtype=np.float32)[None, :]
    y = np.arange(H, dtype=np.float32)[:, None]
    arg = (x * HASH_X + y * HASH_Y).astype(np.float32).ravel()       # float32 products and sum: one rounding each
    sin_arg = np.array([_sinf(float(a)) for a in arg], dtype=np.float32)
    r = (sin_arg * HASH_SCALE).astype(np.float32)
    r = (r - np.array([_floorf(float(v)) for v in r], dtype=np.float32)).astype(np.float32)
    if direction < 0:
        d = np.full_like(r, -direction)
    else:
        d = (r * direction).astype(np.float32)
    if rng < 0:
        dist = np.full(r.shape, -rng, dtype=np.int64)
    else:
        dist = np.trunc((r * np.float32(rng)).astype(np.float32)).astype(np.int64)
    distf = dist.astype(np.float32)                                  # exact: |range| <= 2^30
    cos_d = np.array([_cosf(float(v)) for v in d], dtype=np.float32)
    sin_d = np.array([_sinf(float(v)) for v in d], dtype=np.float32)
    xp = np.trunc((cos_d * distf).astype(np.float32)).astype(np.int64).reshape(H, W)
    yp = np.trunc((sin_d * distf).astype(np.float32)).astype(np.int64).reshape(H, W)
    _TABLES[key] = (xp, yp)
    return xp, yp


def option(v: float) -> float:
    """a double as hb_dict hands it on ("%g") and as FFmpeg parses it back; Declined outside the option's range"""
    d = float("%g" % v)
    if not THR_MIN <= d <= THR_MAX:
        raise Declined(f"threshold {v!r} outside [{THR_MIN}, {THR_MAX}]")
    return d


def threshold(v: float, depth: int) -> int:
    """(int)(((1 << depth) - 1) * (float)option): a float product, truncated"""
    return int(np.float32((1 << depth) - 1) * np.float32(option(v)))


def resolve(settings: str, depth: int):
    """deband.c's settings string -> dict(thr=(3 ints), range, blur); Declined for what the drop-in declines"""
    kv = dict(p.split("=", 1) for p in settings.split(":") if p)
    thr = [float(kv.get(f"{i + 1}thr", DEFAULTS["thr"][i])) for i in range(4)]
    rng = int(float(kv.get("range", DEFAULTS["range"])))
    blur = int(float(kv.get("blur", DEFAULTS["blur"])))
    ints = [threshold(t, depth) for t in thr][:3]                    # (4thr is range-checked too; no alpha plane here)
    if blur not in (0, 1):
        raise Declined(f"blur {blur}")
    if abs(rng) > RANGE_MAX:
        raise Declined(f"range {rng}")
    return dict(thr=tuple(ints), range=rng, blur=blur)


def deband_plane(plane, xp, yp, thr: int, blur: int):
    """one plane; xp / yp: the luma table (its top-left corner serves the chroma planes)"""
    h, w = plane.shape
    src = plane.astype(np.int64)
    dx, dy = xp[:h, :w], yp[:h, :w]
    y = np.arange(h)[:, None]
    x = np.arange(w)[None, :]
    ya, yb = np.clip(y + dy, 0, h - 1), np.clip(y - dy, 0, h - 1)
    xa, xb = np.clip(x + dx, 0, w - 1), np.clip(x - dx, 0, w - 1)
    out = decide(src, src[ya, xa], src[yb, xa], src[yb, xb], src[ya, xb], thr, blur)
    return out.astype(plane.dtype)


def deband_plane_loop(plane, xp, yp, thr: int, blur: int):
    """the same, one sample at a time as FFmpeg's loop goes"""
    h, w = plane.shape
    src = plane.astype(np.int64)
    out = np.empty_like(plane)
    clip = lambda v, hi: 0 if v < 0 else (hi if v > hi else v)
    for y in range(h):
        for x in range(w):
            dx, dy = int(xp[y, x]), int(yp[y, x])
            r0 = int(src[clip(y + dy, h - 1), clip(x + dx, w - 1)])
            r1 = int(src[clip(y - dy, h - 1), clip(x + dx, w - 1)])
            r2 = int(src[clip(y - dy, h - 1), clip(x - dx, w - 1)])
            r3 = int(src[clip(y + dy, h - 1), clip(x - dx, w - 1)])
            s = int(src[y, x])
            a = (r0 + r1 + r2 + r3) // 4
            if blur:
                out[y, x] = a if abs(s - a) < thr else s
            else:
                out[y, x] = a if all(abs(s - r) < thr for r in (r0, r1, r2, r3)) else s
    return out


def deband_frame(planes, settings: str, depth: int):
    """a whole frame through the model (the drop-in's settings string); Declined as the drop-in declines"""
    p = resolve(settings, depth)
    H, W = planes[0].shape
    xp, yp = offsets(W, H, p["range"])
    return tuple(deband_plane(pl, xp, yp, p["thr"][c], p["blur"]) for c, pl in enumerate(planes))
