#!/usr/bin/env python3
"""bench.py — filtered frames/sec of the libhb video-filter hot path on MI355X.

Default workload = the chain BASELINE.json's `metric` names ("1080p YUV420p NLMeans+decomb
chain"), in the form BASELINE configs[3] spells out:

    decomb (mode 31: yadif+blend+cubic+EEDI2, bob) -> NLMeans medium -> crop/scale Lanczos
    1920x1080 -> 3840x2160 -> lapsharp (medium: 0.2, isolap)

on 1920x1080 YUV420P 8-bit interlaced synthetic frames.  A "step" = one pass of the chain over
one batch of BATCH consecutive input frames of a stream that is already resident in HBM; every
input frame leaves as two 3840x2160 output frames (bob).  The frames go through the product C ABI
(hbhip_chain_process_dev: the run of HIP filters fused the way hb_avfilter_combine fuses a run of
libavfilter filters) exactly as they would in production: every EEDI2 pass taking the fields of a batch
in one launch, pictures handed from stage to stage by pointer.  `value` counts OUTPUT
frames.  Nothing of the oracle or of any CPU path runs inside the timed region.

Other workloads (--workload): nlmeans = configs[1], decomb_eedi2 = configs[2] (add
--comb-detect for the comb-detect + selective-decomb pair), chain2160 = the per-GPU stream of
configs[4] (3840x2160 interlaced in, same chain without the then-identity scaler, work.c:1467-1473).

Multi-GPU (--gpus N under torch.distributed.run): every rank filters its own independent stream
on its own GPU (frames shard by stream); no data-path collective; RCCL only reduces
{frames, seconds}: value = total output frames of all ranks / max-over-ranks time.  scaling = weak.

A plain run sets up, warms up, times the steps, writes --dump-outputs if asked and prints the line: the headline
(`value`, `ms_per_step`, ...) and what follows from the timed steps alone (input_fps, the chain's algorithmic HBM rate,
host_enqueue_ms_per_step_timed_region).  Everything else runs after the timed region and only with --full:
  roofline       dominant kernel of the workload (largest share of GPU time): algorithmic bytes per
                 launch / its mean launch time.  Launch times come from a pass right after the timed
                 region in which the same launches are bracketed by HIP events on the stream they run
                 on; `kernels` lists the rest.  `roofline.valu` prices the kernel's vector instructions with its own mix,
                 `roofline.issue_floors` carries the committed vector / scalar / LDS / HBM floors of that kernel
                 (tools/kernel_bounds.py on the newest counter passes under profiles/ - evidence, not a measurement of this run).
                 `roofline.measured_peak` is the on-box copy ceiling, `config.eedi2_mask_density` the share of each plane
                 EEDI2 works on, `host_enqueue_ms_per_step` the host's time for a step into an empty queue.
  cpu_baseline   the reference's own C filters (oracle/_ref, threaded by its own taskset.c as libhb
                 does) on this box's host cores, bounded sample; the scaler leg is our restatement
                 (zimg is not buildable here) and is labelled as such.
  pcie_inclusive the same chain through the hb_filter_object_t surface with host hb_buffer_t in and
                 out (upload adapter ... download adapter) — PCIe included.  Never `value`.

--dump-outputs DIR writes the frames the last timed step handed back, plane by plane, as DIR/<plane>.npy (float32,
frames x rows x columns, or a seeded sample of each frame when the whole would pass 64 MB - see dump_outputs()).  The
inputs are the same from run to run for the same arguments, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s
LAPSHARP = "y-strength=0.2:y-kernel=isolap:cb-strength=0.2:cb-kernel=isolap"     # param.c:932-935

WORKLOADS = {
    "chain": dict(w=1920, h=1080, model="interlaced", batch=16, scale=(3840, 2160), cfg=3,
                  text="BASELINE configs[3]: decomb(31, EEDI2 bob) -> nlmeans medium -> cropscale lanczos "
                       "1920x1080 -> 3840x2160 -> lapsharp, 1080i YUV420P 8-bit in, inputs resident in HBM"),
    "chain2160": dict(w=3840, h=2160, model="interlaced", batch=4, scale=None, cfg=4,
                      text="BASELINE configs[4], one stream per GPU: decomb(31, EEDI2 bob) -> nlmeans medium -> "
                           "lapsharp on 3840x2160 interlaced YUV420P 8-bit (identity crop/scale dropped, "
                           "work.c:1467-1473), inputs resident in HBM"),
    "decomb_eedi2": dict(w=1920, h=1080, model="interlaced", batch=16, scale=None, cfg=3,
                         text="BASELINE configs[2]: decomb EEDI2 bob (mode 31) 1920x1080 interlaced"),
    "nlmeans": dict(w=1920, h=1080, model="progressive", batch=32, scale=None, cfg=2,
                    text="BASELINE configs[1]: nlmeans medium (patch 7, range 3, 2 frames) 1920x1080 YUV420P "
                         "8-bit, inputs resident in HBM"),
}


DUMP_BUDGET = 64 << 20     # bytes: every file --dump-outputs writes, all ranks together


def dump_outputs(path, planes, budget=DUMP_BUDGET):
    """--dump-outputs: `planes` maps a name to the list of (rows x columns) device tensors of one plane, one per output frame
    of the last timed step.  Each name becomes <path>/<name>.npy in float32: frames x rows x columns when everything fits in
    `budget`, else frames x k - the same k positions of every frame, drawn without replacement by a generator seeded with the
    name (sorted flat indices into the plane), k in proportion to the plane's size.  Runs after the timed region."""
    import zlib
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    total = sum(len(ts) * ts[0].numel() for ts in planes.values() if ts)
    room = max(budget - 256 * len(planes), 0) // 4                       # float32 values, less the .npy headers
    for name, ts in planes.items():
        if not ts:
            continue
        full = torch.stack([t.contiguous() for t in ts])
        if total > room:
            n = ts[0].numel()
            k = max(1, n * room // total)
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            idx = torch.from_numpy(np.sort(rng.choice(n, size=k, replace=False))).to(full.device)
            full = full.reshape(len(ts), n)[:, idx]
        np.save(os.path.join(path, name + ".npy"), full.cpu().numpy().astype(np.float32))


def frame_bytes(w, h):
    return w * h * 3 // 2


def algorithmic_bytes(kernel, w, h, out_w, out_h, frames_per_launch=1):
    """ALGORITHMIC bytes one launch of `kernel` moves: planes it must read +
    planes it must write once each, 8-bit 4:2:0.  half = one field-sized 3-plane picture."""
    full, half, out = frame_bytes(w, h), frame_bytes(w, h) // 2, frame_bytes(out_w, out_h)
    t = {
        "nlmeans_plane_n7": 3 * full * frames_per_launch,            # read 2 frames + write 1
        "nlmeans_plane_n5": 3 * full * frames_per_launch, "nlmeans_plane_n3": 3 * full * frames_per_launch,
        "nlmeans_plane_n9": 3 * full * frames_per_launch,
        "decomb_plane": 5 * full,                                     # prev, cur, next, EEDI2 guess -> out
        "cropscale_lanczos_fused": full + out,
        "lapsharp_3x3": 2 * out, "lapsharp_5x5": 2 * out,
        "copy_planes": full,                                          # the chain's copy-in: one input frame read + written per TWO output frames
        "eedi2_mask_passes": 3.5 * half,                              # field rows + the old mask's lower half -> srcp + new mask (all fields of a batch per launch)
        "eedi2_mask_repair": 4,                                       # one workgroup that reads the chain's error word and returns (MaskChain)
        "eedi2_calc_directions": 3 * half,                            # mskp + srcp -> tmpp
        "eedi2_filter_dir_map": 3 * half, "eedi2_expand_dir_map": 3 * half, "eedi2_filter_map": 3 * half,
        "eedi2_filter_expand_dir_map": 3 * half,                      # the two passes in one launch: mskp + map -> map

        "eedi2_mark_directions_2x": 3 * half + 4 * full,              # 3 line doublings + tmp2p
        "eedi2_filter_dir_map_2x": 3 * full, "eedi2_expand_dir_map_2x": 3 * full, "eedi2_filter_expand_dir_map_2x": 3 * full,
        "eedi2_filter_expand_dir_map_2x_post": 6 * full,              # msk2p + map -> map + filtered map; dst2p read and (rarely) written
        "eedi2_fill_gaps_2x": 3 * full,
        "eedi2_lattice_candidates": 3 * full + 4 * full,              # tmp2p, dst2p, tmp2p2 -> u32 candidates
        "eedi2_lattice_resolve": 4 * full + 2 * full,
        "eedi2_post_process": 4 * full,
        "comb_detect": 3 * w * h + w * h, "comb_mask_passes": 2 * w * h, "comb_block_score": w * h,
    }
    return t.get(kernel)


def cpu_quota():
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            return max(1, int(int(q) / int(per)))
    except Exception:
        pass
    return None


def cpu_baseline_nlmeans(frames_np):
    """Reference NLMeans on the host cores (rank 0, N=1 only). ~10-30 s of CPU work."""
    from handbrake_amd import hbrt, hip
    import oracle_lib as ol
    settings = hip.NLMEANS_MEDIUM
    ref = ol.ref()
    if ref is not None:
        ncpu = min(os.cpu_count() or 1, 128)
        rule = lambda c: c // 2 if c >= 32 else (c // 4) * 3 if c >= 16 else max(c, 1)   # nlmeans.c:361-373
        candidates = [rule(ncpu)]
        # a container CPU quota (cgroup cpu.max) below the visible core count throttles an
        # over-subscribed run: also time the thread count the quota supports and keep the better
        quota = cpu_quota()
        if quota and quota < ncpu and quota not in candidates:
            candidates.append(quota)
        best = None
        for threads in candidates:
            st = settings + f":threads={threads}"
            n = max(2 * threads + 2, 24)
            seq = [frames_np[i % len(frames_np)] for i in range(n)]
            t0 = time.perf_counter()
            out = hbrt.run_stream(ref, [("hb_filter_nlmeans", st)], seq)
            dt = time.perf_counter() - t0
            if dt < 5.0:   # too short to be meaningful: repeat with a sample of about 8 s
                k = int(min(8.0 / max(dt, 1e-3), 64)) + 1
                seq = seq * k
                t0 = time.perf_counter()
                out = hbrt.run_stream(ref, [("hb_filter_nlmeans", st)], seq)
                dt = time.perf_counter() - t0
            rec = (len(out) / dt, threads, len(out), dt)
            if best is None or rec[0] > best[0]:
                best = rec
        fps, threads, nout, dt = best
        return {"value": round(fps, 3), "unit": "frames/s", "cores": threads,
                "kind": "reference",
                "sample": f"{nout} frames 1920x1080 YUV420P through the reference hb_filter_nlmeans "
                          f"init/work/close (libhb/nlmeans.c compiled in place, taskset threads={threads}"
                          f"{' = best of ' + str(candidates) if len(candidates) > 1 else ''}, "
                          f"{'cpu quota ' + str(quota) + ' CPUs, ' if quota else ''}SSE2 integral), {dt:.1f}s wall"}
    # port: single-thread restatement, a few frames
    n = 3
    t0 = time.perf_counter()
    for t in range(n):
        for c in range(3):
            ol.orc_nlmeans_plane([frames_np[t][c], frames_np[t + 1][c]])
    dt = time.perf_counter() - t0
    return {"value": round(n / dt, 3), "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{n} frames 1920x1080 YUV420P, oracle/nlmeans_oracle.c single thread, {dt:.1f}s wall"}


def cpu_baseline_chain(workload, frames_np, scale):
    """The reference's own filter objects (oracle/_ref) for the chain workloads on the host cores, stage by stage.
    EEDI2 runs on 3 plane threads whatever the core count (decomb.c:386-394), ~0.5 s per 1080p field.  libhb runs
    every filter on a thread of its own with fifos between them (work.c:2527-2600), so a job's frame rate is that of
    its slowest stage: `value` is that rate - an upper bound for the CPU, the stages then compete for the same cores -
    and `serial_value` what one gets running the stages one after the other."""
    from handbrake_amd import hbrt, hip
    import oracle_lib as ol
    import oracle_stream as os_
    ref = ol.ref()
    if ref is None:
        return None
    quota = cpu_quota()
    threads = min(os.cpu_count() or 1, quota or 1 << 30)
    nlm = hip.NLMEANS_MEDIUM + f":threads={threads}"
    # BASELINE.md §3 plans 64 timed frames after 8 warm-up, median of 3.  Kept within about a minute of CPU time here:
    # 32 timed output frames (16 input; 2160p input: 4) after a warm-up pass of 2 input frames, and the median of 3 passes
    # for the stage that sets the rate (decomb: EEDI2 takes ~0.25 s per 1080p field on its 3 plane threads); the other
    # stages, 4 - 20 x faster, are timed once over the same frames.  Stated in `sample`.
    n_in = 16 if frames_np[0][0].shape[1] <= 1920 else 4
    seq = [frames_np[i % len(frames_np)] for i in range(n_in)]
    stages = []

    def timed(name, fn, note, passes=1):
        times = []
        for _ in range(passes):
            t0 = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t0)
        dt = sorted(times)[len(times) // 2]
        stages.append({"stage": name, "seconds": round(dt, 3), "frames": len(out), "note": note,
                       **({"passes": [round(t, 3) for t in times], "statistic": "median"} if passes > 1 else {})})
        return out

    hbrt.run_stream(ref, [("hb_filter_decomb", "mode=31")], seq[:2], flags=8)          # warm-up: pages, thread pools
    out = timed("decomb", lambda: hbrt.run_stream(ref, [("hb_filter_decomb", "mode=31")], seq, flags=8),
                "reference hb_filter_decomb mode=31 (EEDI2 bob, 3 plane threads)", passes=3)
    n_out = len(out)
    frames = [o.planes for o in out]
    if workload != "decomb_eedi2":
        out = timed("nlmeans", lambda: hbrt.run_stream(ref, [("hb_filter_nlmeans", nlm)], frames),
                    f"reference hb_filter_nlmeans medium (taskset threads={threads})")
        frames = [o.planes for o in out]
        if scale:
            frames = timed("crop_scale", lambda: os_.cropscale_stream(frames, dict(width=scale[0], height=scale[1])),
                           f"crop/scale Lanczos to {scale[0]}x{scale[1]}: OUR restatement of zimg's fixed-point resize "
                           "(oracle/alias_oracle.c, one thread) - the reference's scaler is zimg, not buildable here")
        out = timed("lapsharp", lambda: hbrt.run_stream(ref, [("hb_filter_lapsharp", LAPSHARP)], frames),
                    "reference hb_filter_lapsharp (mt_frame_filter threaded)")
        assert len(out) == n_out
    for st in stages:
        st["output_fps"] = round(n_out / st["seconds"], 3)
    slowest = max(stages, key=lambda st: st["seconds"])
    total = sum(st["seconds"] for st in stages)
    return {"value": round(n_out / slowest["seconds"], 3), "unit": "output frames/s", "cores": threads, "kind": "reference",
            "stages": stages, "slowest_stage": slowest["stage"], "serial_value": round(n_out / total, 3),
            "sample": f"{len(seq)} input / {n_out} output frames after a 2-frame warm-up pass, decomb = median of 3 passes "
                      f"(BASELINE.md §3 plans 64 frames / 8 warm-up / median of 3: halved to bound the line's run time); value = "
                      f"rate of the slowest stage ({slowest['stage']}), as libhb's thread-per-filter pipeline delivers it; stages "
                      f"timed one after the other: {total:.1f}s per pass"}


def measured_hbm_peak(device_index):
    """On-box ceiling: a float4 copy kernel of the library's own (hbhip_ctx_copy_bandwidth, csrc/hbhip_core.hip) over
    two 1 GiB buffers - 2 GiB of traffic per pass, well past the 256 MB Infinity Cache -, HIP-event timed, best of 5.  (The
    guide's 6.29 TB/s is measured the same way; torch.Tensor.copy_, which rounds 1-4 used here, goes through the runtime's
    blit kernel and reads ~15 % lower.)"""
    from handbrake_amd import hip
    ctx = hip.Ctx(device_index)
    try:
        fn = hip.lib().hbhip_ctx_copy_bandwidth
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
        fn.restype = C.c_int
        out = C.c_double()
        rc = fn(ctx.h, 1 << 30, 5, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"hbhip_ctx_copy_bandwidth failed ({rc})")
        return round(out.value, 1)
    finally:
        ctx.close()


def pcie_inclusive(workload, w, h, scale, cfg, device, content="interlaced"):
    """The chain through the hb_filter_object_t surface, host hb_buffer_t in and out (H2D + D2H on the path), in a
    process of its own (handbrake_amd/hostpath.py says why): one thread per filter with libhb's bounded fifos between
    them (filter_loop, work.c:2527-2600)."""
    import subprocess
    cmd = [sys.executable, "-m", "handbrake_amd.hostpath", "--workload", workload, "--width", str(w), "--height", str(h),
           "--scale", "none" if not scale else "%dx%d" % tuple(scale), "--cfg", str(cfg), "--device", str(device),
           "--content", content]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if not lines:
        return {"error": (r.stderr or "no output")[-400:], "n_out": 0, "seconds": 0.0}
    return json.loads(lines[-1])


def run_nlmeans(args, world, rank, local_rank):
    """configs[1]: NLMeans medium alone, BATCH frames per launch through hbhip_filter_process_dev."""
    import torch
    import torch.distributed as dist
    from handbrake_amd import hip, shard, synth

    wl = WORKLOADS["nlmeans"]
    W, H = wl["w"], wl["h"]
    B = args.batch or wl["batch"]
    frames_np = synth.stream("progressive", W, H, B + 1, cfg=2 + 16 * rank, depth=args.depth)
    dev_in = [[torch.from_numpy(p).cuda() for p in fr] for fr in frames_np]
    dev_out = [[torch.empty_like(p) for p in dev_in[0]] for _ in range(B)]
    torch.cuda.synchronize()

    ctx = hip.Ctx(local_rank)
    flt = hip.nlmeans_device_filter(ctx, hip.NLMEANS_MEDIUM, W, H, batch=B, depth=args.depth)
    in_arr = (hip.DevFrame * B)(*[hip.dev_frame(dev_in[1 + i]) for i in range(B)])
    out_arr = (hip.DevFrame * B)(*[hip.dev_frame(f) for f in dev_out])
    flt.push_dev(hip.dev_frame(dev_in[0]), 0)       # prime the 1-frame look-ahead

    def step(i):
        n = flt.process_dev(in_arr, 1 + i * B, out_arr)
        assert n == B, f"step produced {n} frames, expected {B}"

    def fence():
        ctx.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for i in range(args.warmup):
        step(i)
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    ctx.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        pre = f"rank{rank}_" if world > 1 else ""
        dump_outputs(args.dump_outputs, {pre + p: [f[c] for f in dev_out] for c, p in enumerate(("y", "cb", "cr"))},
                     DUMP_BUDGET // world)
    if world > 1:
        dist.barrier()
    if args.full:
        # the kernel's launch time: the same steps once more with every launch bracketed by HIP events on its stream (kept
        # out of the timed region: an event record costs the queue ~4.5 us)
        ctx.profile(True)
        ctx.profile_reset()
        for i in range(args.steps):
            step(args.warmup + args.steps + i)
        ctx.sync()
        stats = ctx.profile_stats()
        ctx.profile(False)

    frames_local = float(args.steps * B)
    frames_total, dt_max = shard.reduce_throughput(frames_local, dt, device="cuda")
    if rank == 0:
        out = {
            "metric": "filtered frames/sec, 1080p YUV420p NLMeans (medium) alone [the NLMeans+decomb chain is the default workload]",
            "value": round(frames_total / dt_max, 2), "unit": "frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt_max / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8 (f32 weights)" if args.depth == 8 else f"u16, {args.depth}-bit samples (f32 weights)",
            "data": "synthetic",
            "config": {"workload": wl["text"], "frames_per_step": B, "width": W, "height": H,
                       "parallelism": f"{world} independent stream(s), one per GPU", "device": ctx.name()},
        }
        if args.full:
            kname, (launches, total_ms) = max(stats.items(), key=lambda kv: kv[1][1])
            avg_s = total_ms / launches / 1e3
            frames_per_launch = frames_local / launches
            algo_bytes = 3 * frame_bytes(W, H) * frames_per_launch * (2 if args.depth > 8 else 1)
            achieved = algo_bytes / avg_s / 1e9
            traffic, valu_insts = pmc_record(kname, B)
            out["roofline"] = {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 2),
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                               "traffic": traffic, "launch_us": round(avg_s * 1e6, 2), "launches": launches,
                               "algorithmic_bytes_per_launch": int(algo_bytes),
                               "note": "NLMeans is VALU-bound (about 320 integer/float lane-ops per pixel); "
                                       "'valu' prices the same launch against the measured vector-ALU issue rate"}
            if valu_insts:
                out["roofline"]["valu"] = valu_roofline(valu_insts, avg_s, "nlmeans_plane_n7")
            if world == 1 and not args.no_cpu_baseline and args.depth == 8:
                out["cpu_baseline"] = cpu_baseline_nlmeans(frames_np)
        print(json.dumps(out), flush=True)
    flt.close()
    ctx.close()


def pmc_record(kname, units_per_launch):
    """HBM bytes and VALU instructions per launch from the committed PMC passes (profiles/pmc_traffic.json), scaled from
    the launch shape they were collected on (`units_per_launch` fields / frames) to this run's."""
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(pmc):
        try:
            recs = json.load(open(pmc)).get(kname, {})
            rec = recs.get(str(int(round(units_per_launch)))) or (next(iter(recs.values())) if recs else None)
            if rec:
                k = units_per_launch / float(rec.get("units_per_launch") or units_per_launch)
                t, v = rec.get("hbm_bytes_per_launch"), rec.get("valu_insts_per_launch")
                return (None if t is None else t * k), (None if v is None else v * k)
        except Exception:
            pass
    return None, None


# the device function behind a profiler name, for the kernel's own instruction mix (tools/isa_mix.py)
ISA_NAMES = {"eedi2_calc_directions": ("eedi2_isa_mix.json", "k_calc_dir_rows<4>"),
             "eedi2_fill_gaps_2x": ("eedi2_isa_mix.json", "k_fill_gaps_b"),
             "eedi2_lattice_candidates": ("eedi2_isa_mix.json", "k_lattice_cand_q"),
             "eedi2_filter_dir_map_2x": ("eedi2_isa_mix.json", "k_dir_map4"),
             "nlmeans_plane_n7": ("nlmeans_isa_mix.json", "nlmeans_lanes_kernel<7, 3, 36, false>"),
             "cropscale_lanczos_fused": ("alias_isa_mix.json", "scale8_up_kernel<32>")}


def _newest_profile(suffix):
    """the newest committed profiles/<round>_<suffix> (rounds sort by name: r3_ < r4_)"""
    try:
        files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_" + suffix))
        return files[-1] if files else None
    except OSError:
        return None


def issue_floors(kname):
    """The committed per-kernel floors (tools/kernel_bounds.py on the newest counter passes: the time a launch of the
    profiled shape would take if the vector pipe, the scalar unit, the LDS or the memory were its only limit) for the
    kernel behind a profiler name - static evidence carried on the line, not measured by this run; None without it."""
    own = ISA_NAMES.get(kname)
    try:
        files = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_kernel_bounds.json"))
        rec = json.load(open(os.path.join(ROOT, "profiles", files[-1])))
        key = own[1].split("(")[0]
        k, v = next((k, v) for k, v in rec["kernels"].items() if k.startswith(key))
        return {"kernel": k, "profiled_launch_us": v["launch_us"], "valu_us": v["valu_us"], "salu_us": v["salu_us"],
                "lds_us": v["lds_us"], "hbm_us": v["hbm_us"], "bound": v["bound"], "floor_frac": v["floor_frac"],
                "source": "profiles/" + files[-1]}
    except Exception:
        return None


# the guide's nominal vector issue rate: 256 CUs x 4 SIMDs x 2.4 GHz, a wave64 instruction every 2 cycles (MI355X_MICROARCH.md).
# No kernel of this path can reach it: 70 % of NLMeans' instructions are in classes that issue every 4 cycles
# (profiles/r02_valu_rate.json, r6_valu_rate_f16.json) - `frac` prices the kernel's own mix, `frac_of_nominal` this figure.
NOMINAL_VALU = 256 * 4 * 2.4e9 / 2.0


def valu_roofline(valu_insts, avg_s, kname=None):
    """wave64 VALU instructions (SQ_INSTS_VALU of the committed PMC pass) against the issue peak of the kernel's OWN
    instruction mix: its text classified by tools/isa_mix.py into the issue classes tools/valu_rate.hip measured on
    this GPU type (profiles/r02_valu_rate.json).  Without such a file: the NLMeans mix of r02_valu_rate.json."""
    cyc, src = 4.0, "assumed 4 cycles per wave64 instruction (no micro-benchmark result committed)"
    peak = 256 * 4 * 2.4e9 / cyc
    own = ISA_NAMES.get(kname)
    if own and _newest_profile(own[0]):
        own = (_newest_profile(own[0]), own[1])
        try:
            ks = json.load(open(os.path.join(ROOT, "profiles", own[0])))["kernels"]
            rec = next(v for k, v in ks.items() if own[1] in k)
            peak, cyc = rec["peak_ginst_s"] * 1e9, rec["cyc_per_inst"]
            src = (f"static instruction mix of {own[1]} (profiles/{own[0]}: {rec['full']} full-rate, {rec['half']} half-rate, "
                   f"{rec['quarter']} quarter-rate VALU instructions) priced with the per-class issue rates measured by "
                   f"tools/valu_rate.hip (profiles/r02_valu_rate.json)")
            return {"insts_per_launch": int(valu_insts), "achieved_ginst_s": round(valu_insts / avg_s / 1e9, 1),
                    "peak_ginst_s": round(peak / 1e9, 1), "frac": round(valu_insts / avg_s / peak, 4),
                    "nominal_ginst_s": round(NOMINAL_VALU / 1e9, 1), "frac_of_nominal": round(valu_insts / avg_s / NOMINAL_VALU, 4),
                    "cycles_per_wave_inst": cyc, "peak_source": src}
        except Exception:
            pass
    p = os.path.join(ROOT, "profiles", "r02_valu_rate.json")
    if os.path.exists(p):
        try:
            rec = json.load(open(p))
            cyc = float(rec["nlmeans_mix"]["cyc_per_inst"])
            peak = float(rec["nlmeans_mix"]["peak_ginst_s"]) * 1e9
            src = rec["nlmeans_mix"]["note"]
        except Exception:
            pass
    return {"insts_per_launch": int(valu_insts), "achieved_ginst_s": round(valu_insts / avg_s / 1e9, 1),
            "peak_ginst_s": round(peak / 1e9, 1), "frac": round(valu_insts / avg_s / peak, 4),
            "nominal_ginst_s": round(NOMINAL_VALU / 1e9, 1), "frac_of_nominal": round(valu_insts / avg_s / NOMINAL_VALU, 4),
            "cycles_per_wave_inst": cyc, "peak_source": src}


def build_chain(hip, device, W, H, scale, depth=8, split=2, only_decomb=False, comb_detect=False):
    """The chain object of one stream of frames exactly as the bench drives it (tests/test_configs_gpu.py::test_bench_shape
    builds its chain through this function too): decomb (EEDI2 bob) -> NLMeans medium -> Lanczos scale -> lapsharp behind
    one hbhip_chain.  split: 0 every stage on one context (HIP stream); 1 a context per stage - one stream per filter, as
    libhb runs one thread per filter; 2 decomb on the chain's context, the stages behind it on a second (the default:
    DESIGN 4.10.5); 3 decomb + NLMeans (arithmetic-bound) on one, scaler + lapsharp (memory-bound) on a second; 4 decomb /
    NLMeans / scaler + lapsharp.  The first stage always runs on the chain's own context - the caller's stream.  Returns
    (contexts, chain); the chain owns its stages, the caller closes chain then contexts."""
    OW, OH = scale if scale else (W, H)
    ctxs = [hip.Ctx(device)]

    def stage_ctx(stage=0):
        # split 2: decomb stays on the chain's own context - the caller's stream -, the other stages get one more: with
        # EEDI2's two side streams that makes four busy HIP streams, one per hardware queue of the runtime's default four
        # (a fifth shares a queue with one of them, and whatever waits in it holds the other up: DESIGN 4.10)
        if (not split or stage == 0 or (split == 2 and len(ctxs) >= 2) or (split == 3 and stage != 2) or
                (split == 4 and stage == 3)):
            return ctxs[-1]
        ctxs.append(hip.Ctx(device))
        return ctxs[-1]

    c = stage_ctx()
    decomb = hip.DecombDevice(c, W, H, mode=63 if comb_detect else 31, depth=depth)
    stages = [hip.DeviceFilter(c, decomb.h)]
    decomb.h = None                                       # owned by the chain from here on
    if not only_decomb:
        stages.append(hip.nlmeans_device_filter(stage_ctx(1), hip.NLMEANS_MEDIUM, W, H, batch=1, depth=depth))
        if scale:
            stages.append(hip.cropscale_device_filter(stage_ctx(2), W, H, OW, OH, depth=depth))
        stages.append(hip.lapsharp_device_filter(stage_ctx(3), OW, OH, depth=depth))
    return ctxs, hip.Chain(ctxs[0], stages)


CONTENTS = {
    # the survey's interlaced model: bars moving 6 px / field + a diagonal texture; its chroma steps are too
    # small for EEDI2's edge test (eedi2_template.c:122-195), so the chroma planes' masks are empty and every pass behind
    # the mask only copies them - as the reference's passes skip unmasked pixels (:371, :392-393)
    "interlaced": "interlaced",
    # diamonds in luma, saturated discs in chroma, field-shifted: edges and corners in all three planes
    "corners": "corners",
    # uniform random bytes: nearly every pixel is an edge pixel - the worst case for every masked pass
    "random": "random",
}


def mask_density(hip, device, frames_np, W, H, depth):
    """Fraction of set pixels in EEDI2's edge mask (MSKPF, decomb.c:64-68) per plane, measured on the GPU from the
    engine's own scratch plane after the fields of two frames: what decides how much work the passes behind the mask
    have (they skip unmasked pixels, eedi2_template.c:371, :392-393)."""
    import numpy as np
    ctx = hip.Ctx(device)
    dec = hip.DecombDevice(ctx, W, H, mode=31, depth=depth)
    try:
        for fr in frames_np[:3]:
            dec.push(fr)
        while dec.pull() is not None:
            pass
        out = {}
        for c, name in enumerate(("y", "cb", "cr")):
            m = dec.eedi_plane(1, c)
            w = W if c == 0 else (W + 1) // 2
            out[name] = round(float(np.count_nonzero(m[:, :w])) / float(m.shape[0] * w), 4)
        return out
    finally:
        dec.close()
        ctx.close()


def run_chain(args, world, rank, local_rank):
    """The chain workloads through hbhip_chain (device-resident, one or more independent streams per GPU)."""
    import numpy as np
    import torch
    from handbrake_amd import hip, shard, synth

    wl = WORKLOADS[args.workload]
    W, H, scale = wl["w"], wl["h"], wl["scale"]
    OW, OH = scale if scale else (W, H)
    B = args.batch or wl["batch"]
    # a stream of NSRC consecutive frames of the model, walked batch after batch (it starts over after NSRC: a scene cut
    # every NSRC frames) - no two consecutive steps see the same frames
    nsrc = args.stream_frames if args.stream_frames > 0 else (3 * B if W <= 1920 else B)
    depth = args.depth                                                 # 10 / 12 bits: uint16 planes through the same chain
    frames_np = synth.stream(CONTENTS[args.content], W, H, nsrc, cfg=wl["cfg"] + 16 * rank, depth=depth)
    dev_in = [[torch.from_numpy(p.view(np.int16) if depth > 8 else p).cuda() for p in fr] for fr in frames_np]
    nphase = nsrc // math.gcd(nsrc, B)                                 # distinct batches before the walk repeats
    in_arrs = [(hip.DevFrame * B)(*[hip.dev_frame(dev_in[(k * B + i) % nsrc]) for i in range(B)]) for k in range(nphase)]
    flags = [synth.PIC_FLAG_TOP_FIELD_FIRST] * B
    torch.cuda.synchronize()
    only_decomb = args.workload == "decomb_eedi2"

    def planes(w, h):
        dt = torch.uint8 if depth == 8 else torch.int16
        return [torch.empty((h, w), dtype=dt, device="cuda"),
                torch.empty((h // 2, w // 2), dtype=dt, device="cuda"),
                torch.empty((h // 2, w // 2), dtype=dt, device="cuda")]

    class Lane:
        """One independent stream of frames: its own contexts, filter instances, chain and output frames.
        split: every stage on a context (HIP stream) of its own - one stream per filter, as libhb runs one
        thread per filter - so the chain overlaps the stages of consecutive batches."""
        def __init__(self, split):
            self.ctxs, self.chain = build_chain(hip, local_rank, W, H, scale, depth=depth, split=split, only_decomb=only_decomb,
                                                comb_detect=args.comb_detect)
            self.ctx = self.ctxs[0]
            self.comb = hip.CombDetectDevice(self.ctx, W, H) if args.comb_detect else None
            self.cap = 2 * B + 4
            self.out_t = [planes(OW, OH) for _ in range(self.cap)]
            self.out_arr = (hip.DevFrame * self.cap)(*[hip.dev_frame(t) for t in self.out_t])
            self.produced = 0
            self.fed = 0
            self.last = 0                                 # output frames of the latest step: out_t[:last]

        def combed_for(self, i0, n):
            """comb_detect_work (comb_detect.c:1537-1583): frame i is classified from the luma of i-1, i, i+1 (the first
            frame of the stream from itself twice and its successor, verdict forced) - the frames of a batch in three
            launches and one read-back (hbhip_comb_detect_classify_many_dev)."""
            lumas = [dev_in[max(j, 0) % nsrc][0] for j in range(i0 - 1, i0 + n + 1)]
            return self.comb.classify_many([t.data_ptr() for t in lumas], lumas[0].stride(0), force_bits=1 if i0 == 0 else 0)

        def step(self):
            combed = self.combed_for(self.fed, B) if self.comb else [2] * B
            self.last = self.chain.process_dev(in_arrs[(self.fed // B) % nphase], self.out_arr, tag0=self.fed, flags=flags,
                                               combed=combed)
            self.produced += self.last
            self.fed += B

        def sync(self):
            self.chain.sync()

        def close(self):
            self.chain.close()
            if self.comb:
                self.comb.close()
            for c in reversed(self.ctxs):
                c.close()

    lanes = [Lane(args.stage_streams) for _ in range(max(1, args.streams))]
    ctx = lanes[0].ctx

    def sync_all():
        for ln in lanes:
            ln.sync()
        torch.cuda.synchronize()

    def fence():
        sync_all()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()

    for _ in range(args.warmup):
        for ln in lanes:
            ln.step()
    fence()
    start = sum(ln.produced for ln in lanes)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for ln in lanes:
            ln.step()
    t_enq = time.perf_counter() - t0                     # host time to enqueue the timed steps (nothing waited for yet)
    sync_all()
    dt = time.perf_counter() - t0
    if args.dump_outputs:
        dump = {}
        for i, ln in enumerate(lanes):
            pre = (f"rank{rank}_" if world > 1 else "") + (f"stream{i}_" if len(lanes) > 1 else "")
            for c, p in enumerate(("y", "cb", "cr")):
                dump[pre + p] = [ln.out_t[j][c] for j in range(ln.last)]
        dump_outputs(args.dump_outputs, dump, DUMP_BUDGET // world)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    out_frames = sum(ln.produced for ln in lanes) - start
    frames_total, dt_max = shard.reduce_throughput(float(out_frames), dt, device="cuda")
    if args.full:
        # host time to enqueue a step when nothing holds the host back: three steps into an empty queue (in the timed
        # region the host runs ahead of the GPU until a filter's ring of job tables / pictures makes it wait)
        t1 = time.perf_counter()
        for _ in range(3):
            for ln in lanes:
                ln.step()
        t_enq_free = (time.perf_counter() - t1) / 3
        sync_all()

    # per-kernel launch times: same launches, bracketed by HIP events on their stream, right after the timed region
    stats = {}
    if args.full and not args.no_kernel_timer:
        # on one stream (a lane of its own, all stages on one context) so that every launch is timed alone
        pl = Lane(False)
        for _ in range(2):
            pl.step()
        pl.sync()
        pl.ctx.profile(True)
        pl.ctx.profile_reset()
        for _ in range(2):
            pl.step()
        pl.ctx.sync()
        stats = pl.ctx.profile_stats()
        pl.ctx.profile(False)
        pl.close()

    if rank == 0:
        top = sorted(stats.items(), key=lambda kv: -kv[1][1])
        total_ms = sum(ms for _, (_, ms) in top) or 1.0
        kernels = []
        for k, (n, ms) in top[:24]:
            # the profiled pass ran 2 steps = 4 B output frames (= fields); the kernels take the frames / fields of a
            # batch in one launch (EEDI2: HBHIP_EEDI2_FIELDS per launch; a pass that runs twice per field counts half)
            per_field = {"eedi2_fill_gaps_2x": 2, "eedi2_filter_dir_map_2x": 2, "eedi2_expand_dir_map_2x": 2}.get(k, 1)
            fpl = 4 * B * per_field / n
            ab = algorithmic_bytes(k, W, H, OW, OH, frames_per_launch=fpl if k.startswith("nlmeans_plane") else 1)
            ab = int(ab * (1 if k.startswith("nlmeans_plane") else fpl)) if ab else ab
            avg = ms / n / 1e3
            kernels.append({"kernel": k, "launches": n, "frames_per_launch": round(fpl, 2), "avg_us": round(avg * 1e6, 2), "share": round(ms / total_ms, 4),
                            "algorithmic_bytes_per_launch": ab,
                            "frac_of_hbm_peak": None if ab is None else round(ab / avg / 1e9 / HBM_PEAK_GBS, 5)})
        roof = None
        if kernels:
            d = kernels[0]
            ab = d["algorithmic_bytes_per_launch"]
            if ab:
                achieved = ab / (d["avg_us"] * 1e-6) / 1e9
                traffic, valu = pmc_record(d["kernel"], d["frames_per_launch"])
                roof = {"bound": "hbm", "kernel": d["kernel"], "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                        "launch_us": d["avg_us"], "launches": d["launches"], "share_of_gpu_time": d["share"],
                        "algorithmic_bytes_per_launch": ab,
                        "note": "dominant kernel of the chain = largest share of summed kernel time in the event-"
                                "bracketed pass that follows the timed region; its bytes are small against its "
                                "arithmetic (NLMeans: 17 patch comparisons per pixel; calc_directions: a +-24 step search "
                                "per edge pixel), see `valu`; a launch covers `frames_per_launch` frames / fields"}
                if valu:
                    roof["valu"] = valu_roofline(valu, d["avg_us"] * 1e-6, d["kernel"])
                fl = issue_floors(d["kernel"])
                if fl:
                    roof["issue_floors"] = fl
        per_out = {"chain": 62_208_000, "chain2160": 4 * frame_bytes(W, H) + 3 * frame_bytes(W, H) + 2 * frame_bytes(W, H),
                   "decomb_eedi2": 4 * frame_bytes(W, H)}[args.workload]      # SURVEY §8d, per output frame
        line = {
            "metric": "filtered frames/sec, 1080p YUV420p NLMeans+decomb chain" if args.workload == "chain"
                      else "filtered frames/sec (" + args.workload + ")",
            "value": round(frames_total / dt_max, 2), "unit": "output frames/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt_max / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("u8" if depth == 8 else f"u16, {depth}-bit samples") + " (f32 NLMeans weights, 16-bit fixed-point scaler as zimg, sharpen mix = the reference's f64 expression, as one f32 multiply where init proves that equal)",
            "data": "synthetic",
            "config": {"workload": wl["text"] + (" + comb detect in front (selective decomb, mode 63)" if args.comb_detect else ""),
                       "input_frames_per_step": B * len(lanes), "output_frames_per_step": 2 * B * len(lanes),
                       "input": f"{W}x{H}", "output": f"{OW}x{OH}", "streams_per_gpu": len(lanes),
                       "content": args.content, "stream_frames": nsrc,
                       "stage_streams": int(args.stage_streams),
                       "parallelism": f"{world} GPU(s) x {len(lanes)} independent stream(s)", "device": ctx.name()},
            "input_fps": round(frames_total / dt_max / 2, 2),
            **({"host_enqueue_ms_per_step": round(t_enq_free * 1e3, 4)} if args.full else {}),
            "host_enqueue_ms_per_step_timed_region": round(t_enq / args.steps * 1e3, 4),
            "chain_hbm_GBps_algorithmic": round(per_out * frames_total / dt_max / 1e9, 2),
            "chain_frac_of_hbm_peak": round(per_out * frames_total / dt_max / 1e9 / HBM_PEAK_GBS, 5),
            **({"roofline": roof, "kernels": kernels} if args.full else {}),
        }
        if roof is not None and not args.no_kernel_timer:
            try:
                mp = measured_hbm_peak(local_rank)
                roof["measured_peak"] = mp
                roof["frac_of_measured_peak"] = round(roof["achieved"] / mp, 5)
                line["chain_frac_of_measured_peak"] = round(per_out * frames_total / dt_max / 1e9 / mp, 5)
            except Exception as e:
                roof["measured_peak"] = None
                roof["measured_peak_error"] = repr(e)
        if args.full and not args.no_kernel_timer:
            try:
                line["config"]["eedi2_mask_density"] = mask_density(hip, local_rank, frames_np, W, H, depth)
            except Exception as e:
                line["config"]["eedi2_mask_density"] = {"error": repr(e)}
        if args.full:
            if world == 1 and not args.no_cpu_baseline:
                line["cpu_baseline"] = cpu_baseline_chain(args.workload, frames_np, scale)
            else:
                line["cpu_baseline"] = None
    # The same chain through the plugin surface, host frames in and out: on EVERY rank at the same time (each on its
    # own GPU with its own pinned buffers), so that an N-GPU run shows what the host's PCIe root complex and memory
    # give N streams at once - the resident rate above cannot.
    pcie = None
    if args.full and not args.no_pcie:
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        try:
            pcie = pcie_inclusive(args.workload, W, H, scale, wl["cfg"] + 16 * rank, local_rank, CONTENTS[args.content])
        except Exception as e:                                               # never lose the bench line over it
            pcie = {"error": repr(e), "n_out": 0, "seconds": 0.0}
        pcie = shard.reduce_host_path(pcie, device="cuda")
    if rank == 0:
        if pcie is not None:
            line["pcie_inclusive"] = pcie
        print(json.dumps(line), flush=True)
    for ln in lanes:
        ln.close()


def dry_run(args, world, rank):
    """What `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` goes through around the kernels, on
    the CPU with gloo in place of RCCL (tests/test_dist_gloo.py runs it at world sizes 2 and 4): RANK / WORLD_SIZE /
    MASTER_* from the environment, the process group, the barrier + max-over-ranks timing, the stream -> rank sharding,
    the SUM / MAX reduction and ONE line from rank 0.  A "step" here credits the frames a real step would put out and
    sleeps - nothing is filtered, the line says so (`data`), `value` is not a throughput of anything.  It always goes through
    the host path's reduction too (`pcie_inclusive`), which a real run does only with --full: free here, and it keeps that
    plumbing covered."""
    import torch.distributed as dist
    from handbrake_amd import shard
    wl = WORKLOADS[args.workload]
    B = args.batch or wl["batch"]
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
        dist.barrier()
    streams = shard.stream_for_rank(rank, world, world)               # one stream per GPU: rank r owns stream r
    produced = 0
    for _ in range(args.warmup):
        time.sleep(0.001)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 * (1 + rank))                                # ranks finish at different times: MAX is exercised
        produced += (B if args.workload == "nlmeans" else 2 * B) * len(streams)
    dt = time.perf_counter() - t0
    if world > 1:
        dist.barrier()
    frames_total, dt_max = shard.reduce_throughput(float(produced), dt)
    pcie = shard.reduce_host_path({"value": produced / dt, "n_out": produced, "seconds": dt})
    if rank == 0:
        print(json.dumps({
            "metric": "filtered frames/sec, 1080p YUV420p NLMeans+decomb chain" if args.workload == "chain"
                      else "filtered frames/sec (" + args.workload + ")",
            "value": round(frames_total / dt_max, 2), "unit": "output frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt_max / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "none", "data": "dry-run (no GPU, nothing filtered)",
            "config": {"workload": wl["text"], "parallelism": f"{world} rank(s) x 1 stream, gloo", "streams_of_rank0": streams},
            "frames_total": frames_total, "seconds_max": dt_max, "pcie_inclusive": pcie, "roofline": None, "cpu_baseline": None,
        }), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0,
                    help="input frames per step (default: per workload - chain 16, chain2160 4, nlmeans 32)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: per-kernel launch times "
                         "and the roofline, the on-box copy ceiling, EEDI2's mask density, the host's enqueue time, the "
                         "CPU baseline and the PCIe-inclusive pass (about 40 s more; the --no-* switches below trim it)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-pcie", action="store_true", help="with --full: skip the PCIe-inclusive pass of the chain workloads")
    ap.add_argument("--depth", type=int, default=8, choices=[8, 10, 12],
                    help="nlmeans and decomb_eedi2 workloads: sample depth (10 / 12 = 16-bit containers)")
    ap.add_argument("--comb-detect", action="store_true",
                    help="chain workloads: run comb detection in front of the (then selective) decomb, "
                         "as BASELINE configs[2] words it")
    ap.add_argument("--no-kernel-timer", action="store_true",
                    help="with --full, chain workloads: skip the event-bracketed pass after the timed region (roofline = null)")
    ap.add_argument("--stage-streams", type=int, default=None,
                    help="chain workloads: 2 = decomb on one HIP stream, the stages behind it on a second (default at 8 bits; at 10 / 12 "
                         "bits, where it costs 3 %%, the default is 0: the next "
                         "batch's EEDI2 passes beside this batch's NLMeans / scaler / lapsharp; 8 100 -> 8 300 output fps - it was "
                         "-3.5 %% while EEDI2 took 16 fields per launch group); 0 = the whole chain on one stream (EEDI2 itself "
                         "still forks its passes onto side streams); 1 = every filter on a stream of its own (libhb: one thread "
                         "per filter; 7 400), 3 = decomb + NLMeans | scaler + lapsharp (7 900), 4 = decomb | NLMeans | scaler + "
                         "lapsharp (7 300)")
    ap.add_argument("--streams", type=int, default=1,
                    help="chain workloads: independent streams (own HIP stream and filter instances) per GPU")
    ap.add_argument("--workload", default="chain", choices=sorted(WORKLOADS),
                    help="chain = BASELINE's metric, configs[3] (default, the line the driver records); nlmeans = "
                         "configs[1]; decomb_eedi2 = configs[2]; chain2160 = one stream of configs[4]")
    ap.add_argument("--content", default="interlaced", choices=sorted(CONTENTS),
                    help="chain workloads: the synthetic picture model (handbrake_amd/synth.py).  interlaced (default) = the survey's "
                         "model, whose chroma has no EEDI2 edge; corners = edges and corners in all three planes; random = uniform "
                         "noise, every pixel an edge pixel.  The EEDI2 passes skip unmasked pixels as the reference does "
                         "(eedi2_template.c:371, :392-393), so the rate depends on it: config.eedi2_mask_density says how much")
    ap.add_argument("--stream-frames", type=int, default=0,
                    help="chain workloads: length of the synthetic stream the steps walk through (default 3 batches; 2160p: 1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the output frames of the last one as DIR/<plane>.npy (float32, "
                         "at most 64 MB in all: a fixed seeded sample of each frame when the whole is larger)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU, no kernels: the rank plumbing of the multi-GPU launch only (gloo on the CPU) - see "
                         "dry_run(); the line it prints is labelled and is not a measurement")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.dry_run:
        ap.error("--dump-outputs: a dry run computes nothing")
    if args.stage_streams is None:
        args.stage_streams = 2 if args.depth == 8 else 0

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} ranks (WORLD_SIZE={world})")
    if args.dry_run:
        return dry_run(args, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback in the product path)")
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if args.workload == "nlmeans":
        run_nlmeans(args, world, rank, local_rank)
    else:
        run_chain(args, world, rank, local_rank)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
