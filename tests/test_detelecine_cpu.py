"""CPU: the pullup model (tests/pullup_model.py) reproduces the reference's detelecine filter on every recorded case,
and the HIP drop-in is registered under the reference's id."""
import ctypes as C

import numpy as np
import pytest

import detelecine_cases as dc
import pullup_model as pm
from handbrake_amd import hbrt, hip


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_model_reproduces_the_reference(name):
    want = dc.load_golden(name)
    got = dc.expected(name)
    assert len(got) == len(want), f"{name}: {len(got)} frames, the reference made {len(want)}"
    for t, ((gp, gm), (wp, wm)) in enumerate(zip(got, want)):
        assert gm == wm, f"{name} frame {t}: (start, stop, flags) {gm} != {wm}"
        for c in range(3):
            assert np.array_equal(gp[c], wp[c]), f"{name} frame {t} plane {c} differs"


def test_fixtures_drive_pullup():
    """The recorded streams make pullup drop and weave: a 3:2 stream loses a fifth of its pictures, soft telecine
    none, and the woven frames are not the input pictures"""
    assert len(dc.load_golden("hard_tff")) == 20 and len(dc.build("hard_tff")[0]) == 25
    assert len(dc.load_golden("soft_rff")) == len(dc.build("soft_rff")[0])
    frames = dc.build("hard_tff")[0]
    woven = [p for p, _ in dc.load_golden("hard_tff")]
    assert any(not any(np.array_equal(w[0], f[0]) for f in frames) for w in woven)


def test_model_declines_what_has_no_defined_result():
    with pytest.raises(pm.Declined):
        pm.Pullup([(65, 128), (33, 64), (33, 64)], 8)
    with pytest.raises(pm.Declined):
        pm.Pullup([(66, 128), (33, 64), (33, 64)], 8)          # 4:2:0 with a chroma plane of odd height
    with pytest.raises(pm.Declined):
        pm.Pullup([(64, 128), (32, 64), (32, 64)], 8, "skip-left=10:skip-right=7")


def test_model_first_picture_passes_through():
    frames, flags = dc.build("hard_tff")[:2]
    out = pm.run(frames[:1], flags[:1], 8)
    assert len(out) == 1 and out[0][0] == 0 and out[0][1] is frames[0]


def test_drop_in_registered_under_the_detelecine_id(built):
    F = hip.filters()
    F.hbhip_filter_get.restype = C.c_void_p
    F.hbhip_filter_get.argtypes = [C.c_int]
    addr = C.addressof(C.c_char.in_dll(F, "hb_filter_detelecine_hip"))
    assert C.c_int.in_dll(F, "hb_filter_detelecine_hip").value == 3 == hbrt.FILTER_ID["detelecine"]
    assert F.hbhip_filter_get(3) == addr
