"""CPU: the title scan's model, interface and libhb side (handbrake_amd/csrc/scan.hip, libhb/scan_hip.c).

The model's literal form - scan.c's and hb.c's loops as written - against its reduced form, which is what the kernels compute,
on every content of tests/scan_cases.py; what those contents are there to exercise; the structures, constants and symbols of
include/hbhip.h against the binding; what the libhb helper answers without a GPU; and scan_hip.c against the reference's real
headers."""
import ctypes as C
import os
import re
import subprocess

import pytest

from handbrake_amd import hbrt, hip
import scan_cases as sc
import scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/libhb"
HEADER = os.path.join(ROOT, "include", "hbhip.h")


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", sorted(sc.CASES))
def test_literal_and_reduced_forms_agree(case, shape):
    planes = sc.CASES[case](*shape)
    assert sm.literal_scan(planes) == sm.reduced_scan(planes)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("case", sorted(sc.COMB_CASES))
def test_forms_agree_under_flags_and_sensitivities(case, shape):
    planes = sc.COMB_CASES[case](*shape)
    for flags, params in sc.FLAG_PARAMS:
        assert sm.literal_detect_comb(planes, flags, *params) == sm.reduced_detect_comb(planes, flags, params), (flags, params)


def test_cases_reach_the_branches_they_are_there_for():
    """at 100 x 240: border = 2, h4 = 60, w4 = 25"""
    w, h = 100, 240
    crop = {name: sm.literal_crop(fn(w, h)[0]) for name, fn in sc.CROP_CASES.items()}
    assert crop["no_border"] == (0, 0, 0, 0, 1)
    assert crop["all_black"] == (60, 60, 25, 25, 0)                  # the walk hits h4 / w4: not recorded
    assert crop["letterbox_line21"] == (30, 40, 0, 0, 1)             # the bright rows inside the border region are passed over
    assert crop["letterbox_plain"] == (30, 40, 0, 0, 1)
    assert crop["border_rows_dark"] == (0, 0, 0, 0, 1)               # top <= border, the untested rows all dark: 0
    assert crop["border_row_bright"] == (1, 1, 0, 0, 1)              # ... one of them not: that row
    assert crop["pillarbox"] == (0, 0, 0, 0, 1)                      # row 0 is part of every column
    assert crop["pillarbox_matte"] == (30, 40, 10, 14, 1)            # the columns start below the matte
    assert crop["average_31_32"] == (30, 48, 0, 0, 1)
    assert crop["below_16"] == (30, 30, 11, 0, 1)
    assert crop["sixteen_seventeen"] == (30, 34, 2, 0, 1)
    # border = 0 (64 x 48): both loops over the border rows are empty
    assert sm.literal_crop(sc.letterbox(64, 48, line21=False)[0]) == (6, 8, 0, 0, 1)
    assert sm.literal_crop(sc.all_black(64, 48)[0]) == (12, 12, 16, 16, 0)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_combing_cases_say_what_they_are_there_for(shape):
    assert sm.literal_scan(sc.interlaced(*shape))[7] == 1
    assert sm.literal_scan(sc.progressive(*shape))[7] == 0
    p = sc.chroma_only_combed(*shape)
    cc, _, combed = sm.literal_detect_comb(p, 0, *sm.DEFAULT_PARAMS)
    assert combed == 1 and cc[0] == 0 and cc[2] == cc[1] > 0         # Cr is flat: its score is Cb's counts, carried over
    assert sm.reduced_detect_comb(p, 0, carry=False)[2] == 0          # ... and without them the verdict would be the other one
    # bit 16 selects the prog_* triple, and only that bit does
    verdicts = [sm.literal_detect_comb(sc.interlaced(*shape), flags, *params)[2] for flags, params in sc.FLAG_PARAMS]
    assert verdicts == [1, 1, 1, 0]


# ---------------------------------------------------------------- the interface
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "hbhip.h"
#define P(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
    P(hbhip_scan_params, color_equal); P(hbhip_scan_params, color_diff); P(hbhip_scan_params, threshold);
    P(hbhip_scan_params, prog_equal); P(hbhip_scan_params, prog_diff); P(hbhip_scan_params, prog_threshold);
    P(hbhip_scan_result, top); P(hbhip_scan_result, bottom); P(hbhip_scan_result, left); P(hbhip_scan_result, right);
    P(hbhip_scan_result, recorded); P(hbhip_scan_result, cc); P(hbhip_scan_result, average_cc); P(hbhip_scan_result, combed);
    printf("sizeof.params %zu\nsizeof.result %zu\n", sizeof(hbhip_scan_params), sizeof(hbhip_scan_result));
    printf("inflight %d\nrecord %d\n", HBHIP_SCAN_INFLIGHT_MAX, HBHIP_SCAN_RECORD_BYTES);
    return 0;
}
"""


def test_structures_and_constants_equal_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=gnu99", f"-I{ROOT}/include", str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for struct, name in ((hip.ScanParams, "hbhip_scan_params"), (hip.ScanResult, "hbhip_scan_result")):
        for field, _ in struct._fields_:
            assert int(got[f"{name}.{field}"]) == getattr(struct, field).offset, (name, field)
    assert int(got["sizeof.params"]) == C.sizeof(hip.ScanParams) and int(got["sizeof.result"]) == C.sizeof(hip.ScanResult)
    assert int(got["inflight"]) == hip.SCAN_INFLIGHT_MAX and int(got["record"]) == hip.SCAN_RECORD_BYTES
    assert tuple(hip.ScanParams(*sm.DEFAULT_PARAMS).__getattribute__(f) for f, _ in hip.ScanParams._fields_) == (10, 30, 9, 10, 30, 9)


def scan_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hbhip_scan_[a-z0-9_]+)\s*\(", text)))


def test_every_scan_symbol_of_the_header_is_exported(built):
    decl = scan_symbols()
    assert decl == ["hbhip_scan_create", "hbhip_scan_destroy", "hbhip_scan_inflight", "hbhip_scan_pull", "hbhip_scan_push"]
    lib = hip.lib()
    for sym in decl:
        assert hasattr(lib, sym), f"{sym} declared in hbhip.h but not exported by libhbhip.so"
        assert sym in hip.ABI_SYMBOLS
    F = hip.filters()
    for sym in ("hb_hip_scan_open", "hb_hip_scan_picture", "hb_hip_scan_close"):
        assert hasattr(F, sym), f"{sym} not exported by libhbhip_filters.so"
    assert hasattr(hbrt.runtime(), "hbh_scan_run")


def test_null_arguments_are_refused_without_a_device(built):
    lib = hip.lib()
    h = C.c_void_p()
    assert lib.hbhip_scan_create(None, 64, 48, C.byref(h)) == -3 and not h.value        # HBHIP_ERR_ARG
    assert lib.hbhip_scan_push(None, None, 0, None) == -3
    assert lib.hbhip_scan_pull(None, C.byref(hip.ScanResult())) == -3
    assert lib.hbhip_scan_inflight(None) == 0
    lib.hbhip_scan_destroy(None)


def test_the_libhb_helper_declines_without_a_gpu_and_when_disabled(built, monkeypatch):
    """non-zero from open: scan.c keeps its CPU loops (no fallback inside the helper)"""
    F = hip.filters()
    planes = sc.no_border(64, 48)
    if hip.lib().hbhip_device_count() == 0:
        assert hbrt.scan_run(F, planes)[0] == 1
    monkeypatch.setenv("HBHIP_DISABLE", "1")
    assert hbrt.scan_run(F, planes)[0] == 1


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference tree")
def test_scan_hip_compiles_against_the_real_libhb_headers():
    """as tests/test_boundary_cpu.py does for the filter objects: every libhb type, field and function scan_hip.c uses exists
    in the reference's own headers with a compatible type"""
    flags = ["-fsyntax-only", "-std=gnu99", "-Wall", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
             "-Werror=int-conversion", "-D__LIBHB__", "-DHBHIP_IN_LIBHB", f"-I{ROOT}/tests/libhb_stubs", f"-I{REF}",
             f"-I{ROOT}/include", f"-I{ROOT}/handbrake_amd/libhb", "-DHBHIP_DEVICE=3", "-DHB_FILTER_HIP_UPLOAD=98",
             "-DHB_FILTER_HIP_DOWNLOAD=99"]
    r = subprocess.run(["gcc"] + flags + [os.path.join(ROOT, "handbrake_amd", "libhb", "scan_hip.c")], capture_output=True, text=True)
    assert r.returncode == 0, "\n".join(ln for ln in r.stderr.splitlines() if "error" in ln)
    assert "warning" not in r.stderr, r.stderr
