"""Registers, scratch, LDS and code size of every colorspace_kernel instantiation, at compile time (no GPU): compiles
handbrake_amd/csrc/colorspace.hip, or the copy given, for gfx950 with -Rpass-analysis=kernel-resource-usage and reads
the kernel symbols' sizes from the code object.  Run it on two checkouts and compare: an instantiation that is not
meant to change has every figure equal.

    python tools/colorspace_resources.py [path/to/colorspace.hip]             -> JSON
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READELF = os.environ.get("READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
KEYS = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
        "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}


def short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    name = name.replace("unsigned char", "u8").replace("unsigned short", "u16")
    return name.replace(", CsPlanWide>", ", wide>").replace(", CsPlan>", ">")


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "handbrake_amd", "csrc", "colorspace.hip")
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "colorspace.co")
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-O3", "-std=c++17",
                            "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "handbrake_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                            "-c", src, "-o", co], capture_output=True, text=True, check=True)
        out, cur = {}, None
        for line in p.stderr.splitlines():
            m = re.search(r"remark:\s+(.*?): (.*) \[-Rpass", line)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2).strip()
            if k == "Function Name":
                cur = out.setdefault(short(v), {})
            elif cur is not None and k in KEYS:
                cur[KEYS[k]] = int(v)
        for line in subprocess.run([READELF, "-sW", co], capture_output=True, text=True, check=True).stdout.splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and short(f[7]) in out:
                out[short(f[7])]["code_bytes"] = int(f[2])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
