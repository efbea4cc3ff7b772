"""Writes tests/golden/preview_jpeg.npz: what Pillow (libjpeg-turbo, default DCT) writes for the pictures of
tests/jpeg_model.py - the file itself up to 48 x 32, its length and SHA-256 beyond, and the same for one 1920 x 1080 formula
picture.  With it the GPU tests need no Pillow; tests/test_preview_jpeg_cpu.py re-derives every entry where Pillow is there.

    python tests/golden/make_preview_jpeg.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_model as jm                                            # noqa: E402


def entries():
    """{name: array}: "file/<key>" uint8, or "length/<key>" int64 and "sha256/<key>" uint8[32]"""
    out = {}
    todo = [(w, h, c, q) for (w, h, c, q) in jm.cases()] + [jm.BIG + ("formula", 90)]
    for (w, h, c, q) in todo:
        data = jm.pillow_encode(jm.content(c, w, h), q)
        k = jm.key(w, h, c, q)
        if w <= jm.GOLDEN_BYTES_MAX[0] and h <= jm.GOLDEN_BYTES_MAX[1]:
            out["file/" + k] = np.frombuffer(data, np.uint8)
        else:
            out["length/" + k] = np.int64(len(data))
            out["sha256/" + k] = np.frombuffer(hashlib.sha256(data).digest(), np.uint8)
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "preview_jpeg.npz")
    np.savez_compressed(path, **entries())
    print(path, os.path.getsize(path), "bytes")
