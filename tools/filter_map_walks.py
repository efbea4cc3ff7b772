#!/usr/bin/env python3
"""A host-side model of k_filter_map's walks (no GPU): what the pass meets on a field, and what a wave pays for the walk
loop under different ways of dealing the candidate pixels to lanes.

usage: filter_map_walks.py [--contents interlaced,corners,random] [--size 1920x1080] [--rows 4,8,16]
                           [--buckets "1|2+;1|2|3+;1|2|3-4|5+"] [--out profiles/filter_map_walks.json]

The input of the pass comes from the CPU oracle (tests/oracle_lib.py) run up to the pass in front of filter_map
(`npasses=8`) on the luma plane of the third field of `synth.stream(content, w, h, 3)` - two fields before it settle the
edge mask.  A candidate is a pixel on the mask (mskp == 255) that carries a direction (map != 255) off the plane's border;
it walks |((map - 128) >> 2) >> 2| + 1 steps (two fm_steps each), the clipping at the row ends ignored.  Schedules:
  now      a thread owns a dword, a wave a 256-pixel row of a 256 x 4 tile: for each of the four byte positions the wave
           pays the longest walk of its 64 lanes at that position
  raster   the candidates of a 256 x R tile on one list, a lane per entry, 64 consecutive entries a wave
  buckets  one list per class of walk lengths (e.g. "1|2|3+"), waves never mix classes
  sorted   one list sorted by length
  ideal    lane-steps / 64
The figure is wave-steps (the sum over waves of their longest lane) per field: what the vector pipe executes in the walk
loop.  It prices steps only - not the lists, not the set-up of a walk, not the staging."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE_W = 256


def filter_map_input(content, w, h, frames=None):
    """(mask, map) of the luma plane in front of filter_map, third field of the stream (or of `frames`)"""
    from handbrake_amd import synth
    import oracle_lib as ol
    if frames is None:
        frames = synth.stream(content, w, h, 3)
    oe = ol.OrcEedi2(w, h)
    try:
        oe.run(frames[0], 1)
        oe.run(frames[0], 0)
        oe.run(frames[1], 1, npasses=8)
        msk, dmap = oe.plane(1, 0)[:, :w], oe.plane(2, 0)[:, :w]
    finally:
        oe.close()
    return msk, dmap


def walk_steps(msk, dmap):
    """per pixel: steps of its walk, 0 where the pixel is no candidate"""
    h, w = msk.shape
    cand = (msk == 255) & (dmap != 255)
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    steps = np.abs(((dmap.astype(np.int32) - 128) >> 2) >> 2) + 1
    return np.where(cand, steps, 0)


def chunks_cost(lengths):
    """wave-steps of a list dealt to lanes 64 consecutive entries a wave"""
    n = len(lengths)
    if n == 0:
        return 0
    pad = (-n) % 64
    a = np.concatenate([lengths, np.zeros(pad, dtype=lengths.dtype)]).reshape(-1, 64)
    return int(a.max(axis=1).sum())


def parse_buckets(spec):
    """"1|2|3-4|5+" -> [(1, 1), (2, 2), (3, 4), (5, 99)]"""
    out = []
    for part in spec.split("|"):
        if part.endswith("+"):
            out.append((int(part[:-1]), 99))
        elif "-" in part:
            lo, hi = part.split("-")
            out.append((int(lo), int(hi)))
        else:
            out.append((int(part), int(part)))
    return out


def cost_now(steps):
    h, w = steps.shape
    total = 0
    for x0 in range(0, w, TILE_W):
        t = steps[:, x0:x0 + TILE_W]
        pad = (-t.shape[1]) % 4
        if pad:
            t = np.pad(t, ((0, 0), (0, pad)))
        total += int(t.reshape(h, -1, 4).max(axis=1).sum())        # per row (a wave) and byte position: the longest lane
    return total


def cost_tiles(steps, rows, how, buckets=None):
    h, w = steps.shape
    total = 0
    for y0 in range(0, h, rows):
        for x0 in range(0, w, TILE_W):
            t = steps[y0:y0 + rows, x0:x0 + TILE_W].ravel()
            t = t[t > 0]
            if how == "raster":
                total += chunks_cost(t)
            elif how == "sorted":
                total += chunks_cost(np.sort(t))
            else:
                for lo, hi in buckets:
                    total += chunks_cost(t[(t >= lo) & (t <= hi)])
    return total


def model(content, w, h, rows_set, bucket_specs):
    msk, dmap = filter_map_input(content, w, h)
    steps = walk_steps(msk, dmap)
    c = steps[steps > 0]
    hist = {int(k): int(v) for k, v in zip(*np.unique(c, return_counts=True))}
    out = {"field": [int(steps.shape[1]), int(steps.shape[0])], "candidates": int(c.size),
           "candidate_density": round(float(c.size) / steps.size, 4),
           "mean_steps_per_candidate": round(float(c.mean()), 3) if c.size else 0.0,
           "steps_histogram": hist, "lane_steps": int(c.sum()), "ideal": int(-(-int(c.sum()) // 64)),
           "now_dword_walk_256x4": cost_now(steps), "tiles": {}}
    for rows in rows_set:
        t = {"raster": cost_tiles(steps, rows, "raster"), "sorted": cost_tiles(steps, rows, "sorted")}
        for spec in bucket_specs:
            t["buckets " + spec] = cost_tiles(steps, rows, "buckets", parse_buckets(spec))
        out["tiles"]["256x%d" % rows] = t
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--contents", default="interlaced,corners,random")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--rows", default="4,8,16")
    ap.add_argument("--buckets", default="1|2+;1|2|3+;1|2|3-4|5+")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_map_walks.json"))
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    rows_set = [int(v) for v in args.rows.split(",")]
    specs = [s for s in args.buckets.split(";") if s]
    res = {"what": "tools/filter_map_walks.py: wave-steps of k_filter_map's walk loop per field (luma, third field of "
                   "synth.stream(content, %d, %d, 3)) under each schedule; a model on the CPU oracle's planes, steps only - "
                   "nothing here is a GPU measurement" % (w, h),
           "contents": {}}
    for content in args.contents.split(","):
        res["contents"][content] = model(content, w, h, rows_set, specs)
        m = res["contents"][content]
        print("%-10s density %.3f  mean steps %.2f  now %d  ideal %d" % (content, m["candidate_density"],
              m["mean_steps_per_candidate"], m["now_dword_walk_256x4"], m["ideal"]))
        for name, t in m["tiles"].items():
            print("   %-7s " % name + "  ".join("%s %d" % kv for kv in t.items()))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
