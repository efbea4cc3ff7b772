#!/usr/bin/env python3
"""PCIe-inclusive rate of bench.py's list with and without Deband: [decomb 31, vfr, deband, nlmeans, 2160p scale,
lapsharp] against [decomb 31, vfr, nlmeans, 2160p scale, lapsharp], through the plugin surface with host frames in and
out (handbrake_amd/hostpath.run), each pass in a child process of its own the way bench.py spawns its PCIe pass, the
two alternated.  usage: deband_rate.py [rounds] [frames] [deband settings]"""
import json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = "1thr=0.02:2thr=0.02:3thr=0.02:4thr=0.02:range=16:blur=1"      # param.c's `default` preset


def child(with_deband, frames, settings):
    sys.path.insert(0, ROOT)
    from handbrake_amd import hostpath
    chain = hostpath.chain_for("chain", (3840, 2160))
    if with_deband:
        at = [i for i, c in enumerate(chain) if c[0] == "hb_filter_nlmeans_hip"][0]
        chain.insert(at, ("hb_filter_deband_hip", settings))
    res = hostpath.run("chain", 1920, 1080, (3840, 2160), n_in=frames, chain=chain)
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2] == "1", int(sys.argv[3]), sys.argv[4])
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    settings = sys.argv[3] if len(sys.argv) > 3 else DEFAULT
    rates = {0: [], 1: []}
    for r in range(rounds):
        for wd in ((0, 1) if r % 2 == 0 else (1, 0)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(wd), str(frames), settings],
                               cwd=ROOT, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                print(json.dumps({"deband": wd, "error": (p.stderr or "no output")[-600:]}), flush=True)
                return 1
            res = json.loads(lines[-1])
            rates[wd].append(res["value"])
            print(json.dumps({"deband": wd, "value": res["value"], "busy": res.get("stage_thread_busy_fraction")}), flush=True)
    best = {k: max(v) for k, v in rates.items()}
    print(json.dumps({"without": rates[0], "with": rates[1], "best_without": best[0], "best_with": best[1],
                      "ratio": round(best[1] / best[0], 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
