"""GPU: the comb-detect kernels (csrc/comb_detect.hip) held to the oracle's masks cell by cell, through the test hook
hbhip_comb_detect_debug_mask - the detector's mask, the filtered mask the block score read and, where a launch writes
one to HBM, the intermediate mask, each over its whole height x stride buffer (padding columns and border rows must be
the zeros the oracle has) - and then to its verdict.  The product path of 8-bit pictures (classify_batch: the dword
detector, the fused dword mask passes or one byte pass, the block score) and of deeper ones (the generic detector, the
fused byte passes) on the sizes, content and configurations of tests/comb_cases.py, whose expected masks
tests/test_comb_masks_cpu.py keeps on the kernels' edges and ties to the reference."""
import ctypes as C

import numpy as np
import pytest

from handbrake_amd import hip
import comb_cases as cc
import oracle_lib as ol
from test_comb_masks_cpu import knife_scores, oracle_case, oracle_masks

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -3, -5


@pytest.fixture(scope="module")
def ctx(built):
    c = hip.Ctx(0)
    yield c
    c.close()


def which_masks(par):
    """the masks a configuration has in HBM: 0 always, 1 with a mask filter, 2 where filter mode 0's pass wrote it (the
    fused kernels of filter mode 2 carry theirs in LDS, filter mode 1 has none)"""
    if not par["mode"] & 2:
        return [0]
    return [0, 1, 2] if par.get("filter_mode", 2) == 0 else [0, 1]


def same_masks(cd, want, par, tag, frame=0):
    for which in (0, 1, 2):
        if which not in which_masks(par):
            rc = hip.lib().hbhip_comb_detect_debug_mask(cd.h, frame, which, None, 0, None)
            assert rc == ERR_UNSUPPORTED, (tag, which, rc)
            continue
        got = cd.debug_mask(which, frame)
        assert got.shape == want[which].shape, (tag, which)
        if not np.array_equal(got, want[which]):
            ys, xs = np.nonzero(got != want[which])
            cells = [(int(y), int(x), int(got[y, x]), int(want[which][y, x])) for y, x in zip(ys[:8], xs[:8])]
            raise AssertionError(f"{tag} mask {which}: {len(ys)} cells differ; (row, column, got, want): {cells}")


def run_case(ctx, w, h, cfg, depth=8):
    want = oracle_case(w, h, cfg, depth)
    cd = hip.CombDetectDevice(ctx, w, h, depth=depth, **cfg["par"])
    try:
        for step, (((p, c, n), force), (verdict, masks)) in enumerate(zip(cc.case_lumas(w, h, cfg, depth), want)):
            cd.store(p)
            cd.store(None if c is p else c)                         # the repeated frame: store_ref's luma == NULL
            cd.store(n)
            got = cd.classify(force)
            tag = (w, h, depth, cfg["name"], "step", step)
            same_masks(cd, masks, cfg["par"], tag)
            assert got == verdict, tag
    finally:
        cd.close()


@pytest.mark.parametrize("w", cc.WIDTHS)
def test_masks_cell_for_cell(ctx, w):
    """8 bits, every size x configuration: classify_batch's kernels.  Each case classifies two or three times on one
    instance with different content, which exposes a cell a kernel fails to rewrite."""
    for h in cc.heights_of(w):
        for cfg in cc.CONFIGS:
            run_case(ctx, w, h, cfg)


@pytest.mark.parametrize("w", cc.DEEP_WIDTHS)
@pytest.mark.parametrize("depth", [10, 12])
def test_masks_cell_for_cell_deep(ctx, depth, w):
    """depths 10 and 12: comb_detect_kernel<uint16_t> with the (1 << depth)-entry gamma table, comb_mask_fused_kernel
    (filter mode 2) or comb_mask_pass_kernel (filter mode 1), the block score's byte path"""
    assert {c["par"].get("filter_mode", 2) if c["par"]["mode"] & 2 else None for c in cc.DEEP_CONFIGS} == {2, 1, None}
    for h in cc.DEEP_HEIGHTS:
        for cfg in cc.DEEP_CONFIGS:
            run_case(ctx, w, h, cfg, depth)


def test_hook_refusals(ctx):
    w, h = 67, 21
    cfg = cc.CONFIGS[0]
    cd = hip.CombDetectDevice(ctx, w, h, **cfg["par"])
    try:
        L = hip.lib()
        buf = np.zeros((h, 128), np.uint8)
        st = C.c_int()
        assert L.hbhip_comb_detect_debug_mask(cd.h, 0, 0, buf.ctypes.data, buf.nbytes, C.byref(st)) == ERR_ARG   # nothing classified
        (p, c, n), force = cc.case_lumas(w, h, cfg)[-1]
        for y in (p, c, n):
            cd.store(y)
        cd.classify(force)
        assert L.hbhip_comb_detect_debug_mask(cd.h, 0, 0, buf.ctypes.data, buf.nbytes, C.byref(st)) == 0 and st.value == 128
        for frame, which, nbytes in [(1, 0, buf.nbytes), (-1, 0, buf.nbytes), (0, 3, buf.nbytes), (0, -1, buf.nbytes),
                                     (0, 0, buf.nbytes - 1), (0, 1, 0)]:
            assert L.hbhip_comb_detect_debug_mask(cd.h, frame, which, buf.ctypes.data, nbytes, C.byref(st)) == ERR_ARG
        assert L.hbhip_comb_detect_debug_mask(cd.h, 0, 2, buf.ctypes.data, buf.nbytes, C.byref(st)) == ERR_UNSUPPORTED
        assert L.hbhip_comb_detect_debug_mask(None, 0, 0, buf.ctypes.data, buf.nbytes, C.byref(st)) == ERR_ARG
    finally:
        cd.close()


# ---------------------------------------------------------------------------------------- several frames per launch
def batch_lumas(w, h, n, cfg):
    """n + 2 lumas for n frames; every fourth one repeats its predecessor, so frames 0, 3, 4, 7, 8 .. have no motion
    and (with a motion threshold) an empty mask unless their force bit is set"""
    s = cc.seed_of(w, h, cfg) + 9
    if cfg["first"] == "threshold":
        lumas = cc.comb_threshold(w, h, n + 2, s, 8, cfg["par"]["spatial_thresh"])
    else:
        lumas = cc.comb_field(w, h, n + 2, s)
    for i in range(1, n + 2, 4):
        lumas[i] = lumas[i - 1]
    return lumas


class DevLumas:
    """lumas in HBM, `stride` bytes a row with zero padding (hbhip_dev_alloc / _upload: plain device memory)"""

    def __init__(self, ctx, lumas, stride):
        self.ctx, self.stride, self.ptrs = ctx, stride, []
        for y in lumas:
            buf = np.zeros((y.shape[0], stride), np.uint8)
            buf[:, :y.shape[1]] = y
            p = C.c_void_p()
            hip.check(hip.lib().hbhip_dev_alloc(ctx.h, buf.nbytes, C.byref(p)), ctx.h, "dev_alloc")
            self.ptrs.append(p.value)
            hip.check(hip.lib().hbhip_dev_upload(ctx.h, p.value, buf.ctypes.data, buf.nbytes), ctx.h, "dev_upload")

    def close(self):
        for p in self.ptrs:
            hip.lib().hbhip_dev_free(self.ctx.h, p)
        self.ptrs = []


def oracle_batch(w, h, par, lumas, n, force_bits):
    """the oracle classifying the same triples one by one: [(verdict, masks)]"""
    oc = ol.OrcComb(w, h, **par)
    try:
        out = []
        for i in range(n):
            v = oc.classify(lumas[i], lumas[i + 1], lumas[i + 2], bool((force_bits >> i) & 1))
            out.append((v, oracle_masks(oc, h)))
        return out
    finally:
        oc.close()


BATCH_CONFIGS = [c for c in cc.CONFIGS if not c["par"]["mode"] & 2 or c["par"]["filter_mode"] == 2]


@pytest.mark.parametrize("n,force_bits", [(16, 0x5555), (5, 0x0A)])
@pytest.mark.parametrize("w,h", [(67, 21), (128, 35), (258, 19)])
def test_masks_of_several_frames_per_launch(ctx, w, h, n, force_bits):
    """classify_many_dev: frames along grid.z, every frame's masks and verdict the oracle's; the lumas with padded rows
    and, where the width is a multiple of 4, packed (stride = width)"""
    assert len(BATCH_CONFIGS) >= 12
    for cfg in BATCH_CONFIGS:
        lumas = batch_lumas(w, h, n, cfg)
        want = oracle_batch(w, h, cfg["par"], lumas, n, force_bits)
        if cfg["par"]["motion_thresh"] > 0:
            empty = [not m[0].any() for _, m in want]
            assert any(empty) and not all(empty), cfg["name"]                  # the force bits matter
        for stride in [cc.mask_stride(w) + 64] + ([w] if w % 4 == 0 else []):
            dev = DevLumas(ctx, lumas, stride)
            cd = hip.CombDetectDevice(ctx, w, h, **cfg["par"])
            try:
                got = cd.classify_many(dev.ptrs, stride, force_bits=force_bits)
                for i in range(n):
                    same_masks(cd, want[i][1], cfg["par"], (w, h, n, stride, cfg["name"], "frame", i), frame=i)
                assert got == [v for v, _ in want], (w, h, n, stride, cfg["name"])
                assert hip.lib().hbhip_comb_detect_debug_mask(cd.h, n, 0, None, 0, None) == ERR_ARG
            finally:
                cd.close()
                dev.close()


# ------------------------------------------------------------------------------------------ knife-edge block scores
@pytest.mark.parametrize("k", cc.knife_cases(), ids=lambda k: k["name"])
def test_knife_edge_block_scores(ctx, k):
    """one block's score S from the oracle's mask; block thresholds S - 1, S, 2 * S + 2 give HEAVY, LIGHT, NONE (the
    unscored last block column: NONE, NONE, NONE) - one off in comb_score_kernel's sums or block bounds changes one"""
    lumas, s, thr = knife_scores(k)
    got = []
    for t in thr:
        cd = hip.CombDetectDevice(ctx, k["w"], k["h"], block_thresh=t, **k["par"])
        try:
            for y in lumas:
                cd.store(y)
            got.append(cd.classify(False))
        finally:
            cd.close()
    assert tuple(got) == k["want"], (k["name"], s, thr)


# --------------------------------------------------------------------------------- refusals of classify_many_dev
def many(cd, ptrs, stride, n, force_bits=0):
    L = hip.lib()
    L.hbhip_comb_detect_classify_many_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_int)]
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    out = (C.c_int * max(n, 1))()
    return L.hbhip_comb_detect_classify_many_dev(cd.h, arr, stride, n, force_bits, out), list(out)[:n]


def test_classify_many_refusals(ctx):
    """what classify_many_dev refuses it refuses before it queues anything: a valid call behind each refusal is right"""
    w, h, n = 67, 21, 3
    cfg = next(c for c in cc.CONFIGS if c["name"] == "gamma_f2_16x16")
    lumas = batch_lumas(w, h, n, cfg)
    want = oracle_batch(w, h, cfg["par"], lumas, n, 0b010)
    dev = DevLumas(ctx, lumas, 128)
    ptrs = list(dev.ptrs)
    cd = hip.CombDetectDevice(ctx, w, h, **cfg["par"])

    def valid():
        rc, got = many(cd, ptrs, 128, n, 0b010)
        assert rc == 0 and got == [v for v, _ in want]
        for i in range(n):
            same_masks(cd, want[i][1], cfg["par"], ("after a refusal", i), frame=i)

    try:
        assert many(cd, ptrs, 130, n)[0] == ERR_ARG                             # a stride that is no multiple of 4
        valid()
        assert many(cd, ptrs, 64, n)[0] == ERR_ARG                              # ... or below the width
        assert many(cd, [ptrs[0], ptrs[1] + 1] + ptrs[2:], 128, n)[0] == ERR_ARG    # a misaligned luma
        valid()
        assert many(cd, ptrs[:2] + [None] + ptrs[3:], 128, n)[0] == ERR_ARG
        assert many(cd, [ptrs[i % len(ptrs)] for i in range(19)], 128, 17)[0] == ERR_UNSUPPORTED
        assert many(cd, ptrs, 128, 0)[0] == ERR_UNSUPPORTED
        valid()
    finally:
        cd.close()
    # filter mode 1 is a pass of its own behind a batch of one: no classify_many, and classify() goes on working
    cfg1 = next(c for c in cc.CONFIGS if c["name"] == "gamma_f1_8x8")
    cd = hip.CombDetectDevice(ctx, w, h, **cfg1["par"])
    try:
        assert many(cd, ptrs, 128, n)[0] == ERR_UNSUPPORTED
        (p, c, nx), force = cc.case_lumas(w, h, cfg1)[-1]
        for y in (p, c, nx):
            cd.store(y)
        got = cd.classify(force)
        verdict, masks = oracle_case(w, h, cfg1)[-1]
        same_masks(cd, masks, cfg1["par"], "filter mode 1 after a refusal")
        assert got == verdict
    finally:
        cd.close()
        dev.close()
