#!/usr/bin/env python3
"""Record tests/golden/detelecine_*.npz from a library that exports the reference's `hb_filter_detelecine`.

The reference's detelecine.c is not among the wrappers oracle/ builds, so the library is named on the command line.
Built from the reference's unmodified source, outside this repository, e.g.:

    printf '#include "wrap_common.h"\\n#include "detelecine.c"\\n' > wrap_detelecine.c
    gcc -std=gnu99 -O3 -fPIC -fvisibility=default -ffp-contract=off -w -I$REPO/include -I$REPO/handbrake_amd/libhb \\
        -I$REPO/oracle/ref_wrap -I$REPO/oracle/shim -I$REF/libhb -c wrap_detelecine.c -o wrap_detelecine.o
    gcc -shared -o libdetelecine_ref.so wrap_detelecine.o -L$REPO/handbrake_amd -lhbrt -lm -lpthread \\
        -Wl,-rpath,$REPO/handbrake_amd -Wl,--no-undefined

    python tests/golden/make_detelecine_golden.py --ref-lib /path/to/libdetelecine_ref.so [case names ...]

Each case of tests/detelecine_cases.py goes through the object with its per-picture flags; the planes of every output
frame and its (start, stop, flags) are stored as make_golden.py stores them.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from handbrake_amd import hbrt  # noqa: E402
import detelecine_cases as dc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-lib", required=True, help="library exporting the reference's hb_filter_detelecine")
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    hbrt.runtime()
    lib = C.CDLL(os.path.abspath(a.ref_lib), mode=C.RTLD_GLOBAL)
    for name in dc.CASES:
        if a.cases and name not in a.cases:
            continue
        frames, flags, depth, chroma, settings = dc.build(name)
        out = dc.run_chain(lib, "hb_filter_detelecine", settings, frames, flags, depth, chroma)
        arrs = {}
        for t, fr in enumerate(out):
            for c in range(3):
                arrs[f"f{t}_p{c}"] = fr.planes[c]
            arrs[f"f{t}_meta"] = np.array([fr.start, fr.stop, fr.flags], dtype=np.int64)
        path = os.path.join(HERE, f"detelecine_{name}.npz")
        np.savez_compressed(path, nframes=np.array(len(out)), **arrs)
        print(f"{name}: {len(frames)} in, {len(out)} out -> {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
