"""CPU: the preview JPEG's definition (tests/jpeg_model.py) held to libjpeg, and the kernels' block arithmetic
(handbrake_amd/csrc/jpeg_block.h, run on the host by tools/jpeg_block_check) held to the definition.

The reference is Pillow on libjpeg-turbo with its default, accurate integer DCT; tests/golden/preview_jpeg.npz records what
it writes (tests/golden/make_preview_jpeg.py), so the model is pinned on machines without Pillow too and the fixture is
re-derived where Pillow is present.  Everything is integer: byte for byte, no tolerance.
"""
import ctypes as C
import functools
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from handbrake_amd import hbrt, hip
import jpeg_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "jpeg_block_check")
GOLDEN = os.path.join(ROOT, "tests", "golden", "preview_jpeg.npz")
CASES = jm.cases()
case_ids = [jm.key(*c) for c in CASES]


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def model_file(w, h, content, q):
    """computed once per case and shared"""
    return jm.encode(jm.content(content, w, h), q)


def equals_golden(data, k):
    g = golden()
    if "file/" + k in g:
        return data == g["file/" + k].tobytes()
    return len(data) == int(g["length/" + k]) and hashlib.sha256(data).digest() == g["sha256/" + k].tobytes()


# ---------------------------------------------------------------- the model against libjpeg
@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_model_equals_what_libjpeg_wrote(case):
    """the whole file, byte for byte (by length and digest beyond 48 x 32), against the recorded Pillow output"""
    assert equals_golden(model_file(*case), jm.key(*case))


@pytest.mark.parametrize("case", CASES, ids=case_ids)
def test_model_equals_pillow(case):
    """the same against Pillow itself, where it is installed on libjpeg-turbo: the whole file, byte for byte"""
    features = pytest.importorskip("PIL.features")
    if not features.check("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo")
    w, h, content, q = case
    assert model_file(*case) == jm.pillow_encode(jm.content(content, w, h), q)


def test_the_golden_file_is_what_pillow_writes():
    pytest.importorskip("PIL")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_preview_jpeg", os.path.join(ROOT, "tests", "golden", "make_preview_jpeg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fresh, kept = mod.entries(), golden()
    assert sorted(fresh) == sorted(kept)
    for k in fresh:
        assert np.array_equal(fresh[k], kept[k]), k
    big = jm.key(*jm.BIG, "formula", 90)
    assert "sha256/" + big in kept and "file/" + jm.key(48, 32, "noise", 90) in kept and "length/" + jm.key(130, 70, "noise", 90) in kept


def test_tables_equal_the_segments_of_a_libjpeg_file():
    """DQT and DHT as libjpeg wrote them (the recorded 24 x 18 files at five qualities) against the model's literals"""
    for q in (90,) + jm.QUALITIES_EXTRA:
        data = golden()["file/" + jm.key(24, 18, "smooth", q)].tobytes()
        segs, at = jm.segments(data)
        assert at == jm.HEADER_BYTES
        assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
        dqt = [p for m, p in segs if m == 0xDB]
        for index, base in ((0, jm.LUMA_BASE), (1, jm.CHROMA_BASE)):
            assert dqt[index] == jm.dqt_segment(index, jm.quant_table(base, q))[4:], (q, index)
        dht = [p for m, p in segs if m == 0xC4]
        assert [p[0] for p in dht] == [0x00, 0x10, 0x01, 0x11]
        for p in dht:
            assert p == jm.dht_segment(p[0])[4:], hex(p[0])
        assert data[:jm.HEADER_BYTES] == jm.header(24, 18, q)
    # quality scaling at its ends: every entry 255 at quality 1 where the base is large, 1 at quality 100
    assert max(jm.quant_table(jm.LUMA_BASE, 1)) == 255 and set(jm.quant_table(jm.CHROMA_BASE, 100)) == {1}


# ---------------------------------------------------------------- the kernels' header on the host
@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):                        # built by `make product` (__graft_entry__.build())
        subprocess.run(["make", "-C", ROOT, "tools/jpeg_block_check"], capture_output=True, timeout=600)
    assert os.path.exists(EXE), "tools/jpeg_block_check is not built (make product)"
    return EXE


def host_blocks(exe, planes, q, tmp_path=None):
    h, w = planes[0].shape
    data = b"%d %d %d\n" % (w, h, q) + b"".join(np.ascontiguousarray(p).tobytes() for p in planes)
    if tmp_path is not None:                           # from a file
        path = tmp_path / "picture.bin"
        path.write_bytes(data)
        r = subprocess.run([exe, str(path)], capture_output=True, timeout=300)
    else:                                              # from stdin
        r = subprocess.run([exe], input=data, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.decode().splitlines():
        f = line.split()
        out.append((int(f[0]), bool(int(f[1])), [int(v) for v in f[2:66]], f[66]))
    return out


@pytest.mark.parametrize("content", jm.CONTENTS)
@pytest.mark.parametrize("shape", jm.QUALITY_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_check_equals_the_model(exe, tmp_path, shape, content):
    """coefficient for coefficient and bit string for bit string, dummy blocks included"""
    planes = jm.content(content, *shape)
    for q, path in ((90, None), (1, tmp_path), (100, None)):
        got, want = host_blocks(exe, planes, q, path), jm.coded_blocks(planes, q)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (q, i)
        assert any(b[1] for b in want)                 # both sizes have dummy blocks


def test_host_check_refuses_what_the_encoder_refuses(exe):
    for head in (b"25 18 90\n", b"24 18 0\n", b"24 18 101\n", b"nonsense\n"):
        r = subprocess.run([exe], input=head + bytes(1000), capture_output=True, timeout=60)
        assert r.returncode == 1 and not r.stdout, head
    r = subprocess.run([exe], input=b"24 18 90\n" + bytes(10), capture_output=True, timeout=60)
    assert r.returncode == 2 and not r.stdout          # short input


# ---------------------------------------------------------------- what the contents are there to exercise
def luma_strings(w, h, content, q=90):
    return [b for b in jm.coded_blocks(jm.content(content, w, h), q) if b[0] == 0 and not b[1]]


def zrl_symbols(coefs):
    """the 0xF0 symbols of a block: one for every sixteen zeros in front of a coefficient that is not zero"""
    count, run = 0, 0
    for v in coefs[1:]:
        if v == 0:
            run += 1
        else:
            count, run = count + run // 16, 0
    return count


def test_sparse_has_a_zrl_in_every_luma_block():
    for shape in ((24, 18), (130, 70)):
        w, h = shape
        blocks = luma_strings(*shape, "sparse")
        assert len(blocks) == -(-w // 8) * -(-h // 8)
        # a block that lies wholly inside the picture is the one cosine: 62 zeros in front of the last coefficient of the
        # scan - three runs of sixteen and one of fourteen.  (A block the picture's edge cuts is continued by its last
        # column or row and is no single cosine any more; a corner block may have no run of sixteen at all.)
        whole = [coefs for comp, dummy, coefs, bits in blocks if coefs[63] != 0 and not any(coefs[1:63])]
        assert len(whole) == (w // 8) * (h // 8) and all(zrl_symbols(c) == 3 for c in whole)
        assert sum(zrl_symbols(coefs) for comp, dummy, coefs, bits in blocks) >= len(blocks)      # one a luma block and more


def test_noise_has_stuffed_bytes_and_flat_is_short():
    assert jm.entropy_segment(jm.content("noise", 130, 70), 90).count(b"\xff\x00") >= 16
    for shape in ((48, 32), (130, 70), (640, 360)):    # (the first MCU's DC terms weigh less from six MCUs on)
        blocks = jm.coded_blocks(jm.content("flat", *shape), 90)
        assert sum(len(b[3]) for b in blocks) / len(blocks) < 8, shape


def test_dummy_blocks_in_both_directions():
    def dummies(w, h):
        mw = -(-w // 16)
        out = set()
        for i, b in enumerate(jm.coded_blocks(jm.content("smooth", w, h), 90)):
            if b[1]:
                assert b[0] == 0 and b[3] == "00" + "1010"            # DC difference 0, end of block
                m, k = divmod(i, 6)
                if 2 * (m % mw) + (k & 1) >= -(-w // 8):
                    out.add("right")
                if 2 * (m // mw) + (k >> 1) >= -(-h // 8):
                    out.add("bottom")
        return out
    assert dummies(24, 18) | dummies(34, 10) == {"right", "bottom"}
    assert "right" in dummies(34, 10) and "bottom" in dummies(24, 18)
    assert not dummies(48, 32)


def test_a_block_never_passes_the_slot():
    """the longest string of any case stays below the 1660 bits the kernels' 256-byte slots are sized for"""
    longest = max(len(b[3]) for c in ("noise", "sat") for q in (100,) for b in jm.coded_blocks(jm.content(c, 130, 70), q))
    assert 600 < longest <= 1660


# ---------------------------------------------------------------- the interface without a GPU
def test_header_constants_and_symbols(built):
    text = open(os.path.join(ROOT, "include", "hbhip.h")).read()
    assert int(re.search(r"#define HBHIP_JPEG_INFLIGHT_MAX (\d+)", text).group(1)) == hip.JPEG_INFLIGHT_MAX == 4
    decl = sorted(set(re.findall(r"\b(hbhip_jpeg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert decl == ["hbhip_jpeg_bound", "hbhip_jpeg_create", "hbhip_jpeg_destroy", "hbhip_jpeg_inflight", "hbhip_jpeg_pull",
                    "hbhip_jpeg_push"]
    lib = hip.lib()
    for sym in decl:
        assert hasattr(lib, sym) and sym in hip.ABI_SYMBOLS
    assert hasattr(hip.filters(), "hb_hip_scan_picture_preview") and hasattr(hbrt.runtime(), "hbh_scan_preview_run")


def test_null_handles_are_refused(built):
    lib = hip.lib()
    h, size = C.c_void_p(), C.c_size_t(7)
    buf = (C.c_uint8 * 16)()
    assert lib.hbhip_jpeg_create(None, 64, 48, 90, C.byref(h)) == -3 and not h.value    # HBHIP_ERR_ARG
    assert lib.hbhip_jpeg_push(None, None) == -3
    assert lib.hbhip_jpeg_pull(None, buf, 16, C.byref(size)) == -3
    assert lib.hbhip_jpeg_inflight(None) == 0 and lib.hbhip_jpeg_bound(None) == 0
    lib.hbhip_jpeg_destroy(None)


def test_libhb_helper_declines_without_a_device(built, monkeypatch):
    """non-zero and no buffer: scan.c keeps hb_save_preview (no fallback inside the helper)"""
    F = hip.filters()
    planes = jm.content("smooth", 64, 48)
    if hip.lib().hbhip_device_count() <= 0:
        rc, _, data, left = hbrt.scan_preview_run(F, planes)
        assert rc == 1 and data is None and not left
    monkeypatch.setenv("HBHIP_DISABLE", "1")
    rc, _, data, left = hbrt.scan_preview_run(F, planes)
    assert rc == 1 and data is None and not left
