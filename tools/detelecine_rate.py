"""Rates of the HIP detelecine drop-in on a 1080i hard-telecined (3:2) stream.

  * detelecine alone, host buffers in and out (hb_filter_detelecine_hip: upload, metrics, decision, weave, download);
  * [detelecine, decomb, nlmeans, lapsharp] through the plugin surface (upload / download adapters around the run,
    device frames between the stages), against the same list without detelecine; serial and with a thread per filter.

Input frames per second (what the source delivers) and output frames per second.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python tools/detelecine_rate.py`.  usage: detelecine_rate.py [ninputs]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from handbrake_amd import hbrt, hip, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
TFF = synth.PIC_FLAG_TOP_FIELD_FIRST
LAP = "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap"
UP, DOWN = ("hb_filter_hip_upload", ""), ("hb_filter_hip_download", "")
DT = ("hb_filter_detelecine_hip", "")
LIST = [("hb_filter_decomb_hip", "mode=7"), ("hb_filter_nlmeans_hip", hip.NLMEANS_MEDIUM), ("hb_filter_lapsharp_hip", LAP)]

# 3:2 over 16 source frames = 20 pictures, cycled (a cycle boundary is a cadence break, as a cut would be)
pics, flags = synth.telecine_stream(1920, 1080, [3, 2] * 8)
assert all(f == TFF for f in flags)
seq = [pics[i % len(pics)] for i in range(n)]

CASES = [
    ("detelecine alone, host buffers", [DT]),
    ("[detelecine, decomb 7, nlmeans, lapsharp] plugin surface", [UP, DT] + LIST + [DOWN]),
    ("[decomb 7, nlmeans, lapsharp] plugin surface", [UP] + LIST + [DOWN]),
]
for threaded in (False, True):
    hbrt.set_threaded(threaded)
    for name, chain in CASES:
        if threaded and len(chain) == 1:
            continue
        hbrt.run_stream(hip.filters(), chain, seq[:8], flags=TFF)          # warm-up (allocations, code objects)
        t0 = time.perf_counter()
        out = hbrt.run_stream(hip.filters(), chain, seq, flags=TFF)
        dt = time.perf_counter() - t0
        print(f"{name + ('  [threaded]' if threaded else ''):72s} in {n / dt:8.1f} fps   out {len(out) / dt:8.1f} fps"
              f"   ({dt * 1e3 / n:.3f} ms per input, {len(out)} outputs)", flush=True)
hbrt.set_threaded(False)
