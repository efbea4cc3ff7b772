"""The preview JPEG (csrc/jpeg.hip) on 1080p and 2160p pictures: each launch by the context's kernel timer, a push + pull by
a host clock (timer off), and what it replaces on the same machine - the picture's download, and Pillow's encode of it where
Pillow on libjpeg-turbo is installed (the file is then compared too).  DESIGN.md §4.19.1 quotes its output.

    python tools/jpeg_measure.py [rounds] [out.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                   # noqa: E402
from handbrake_amd import hip                                        # noqa: E402
import jpeg_model as jm                                              # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    ctx = hip.Ctx(0)
    try:
        from PIL import features
        have_pil = bool(features.check("libjpeg_turbo"))
    except Exception:
        have_pil = False
    out = {"device": ctx.name(), "rounds": n, "pillow": have_pil, "cases": []}
    for (w, h) in ((1920, 1080), (3840, 2160)):
        for content in ("formula", "noise", "flat"):
            planes = jm.content(content, w, h)
            fr = hip.Frame(ctx, w, h)
            fr.upload([np.ascontiguousarray(p) for p in planes])
            enc = hip.JpegDevice(ctx, w, h)
            for _ in range(3):
                enc.push(fr)
                data = enc.pull()
            ctx.sync()
            walls = []
            for _ in range(n):
                t0 = time.perf_counter()
                enc.push(fr)
                data = enc.pull()
                walls.append(time.perf_counter() - t0)
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(n):
                enc.push(fr)
                data = enc.pull()
            ctx.sync()
            stats = {k: round(v[1] / v[0] * 1000.0, 2) for k, v in ctx.profile_stats().items() if k.startswith("jpeg")}
            ctx.profile(False)
            downs = []
            for _ in range(n):
                t0 = time.perf_counter()
                host = fr.download()
                downs.append(time.perf_counter() - t0)
            encode_ms = None
            if have_pil:
                times = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    ref = jm.pillow_encode(host, 90)
                    times.append(time.perf_counter() - t0)
                encode_ms = round(float(np.median(times)) * 1000, 3)
                assert ref == data, "the file differs from Pillow's"
            case = {"size": [w, h], "content": content, "file_bytes": len(data), "kernels_us": stats,
                    "kernels_sum_us": round(sum(stats.values()), 2),
                    "push_pull_ms": {"median": round(float(np.median(walls)) * 1000, 4), "min": round(min(walls) * 1000, 4)},
                    "download_ms": {"median": round(float(np.median(downs)) * 1000, 4), "min": round(min(downs) * 1000, 4)},
                    "pillow_encode_ms": encode_ms}
            print(json.dumps(case), flush=True)
            out["cases"].append(case)
            enc.close()
            fr.close()
    ctx.close()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
