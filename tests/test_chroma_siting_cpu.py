"""The chroma siting rule of crop/scale and colorspace (handbrake_amd/csrc/chroma_siting.h) on the host.  The header's own
text is what runs: tools/chroma_siting_check compiles it for the host and prints what it gives; the expectations are
tests/chroma_siting_model.py's, derived from the geometry.  The last test checks the DIRECTION of the shift without
either statement of the formula: a ramp sampled at the sited positions must come out of the resize as the same ramp."""
import os
import subprocess

import numpy as np
import pytest

import chroma_siting_model as csm
import sited_lib as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "chroma_siting_check")
LAYOUTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
# (src_w, dst_w, src_h, dst_h): ratios 1/2, 1, 2, 3/2 in both directions, and different ratios in x and y
SIZES = [(256, 128, 192, 96), (128, 128, 96, 96), (128, 256, 96, 192), (128, 192, 96, 144),
         (192, 128, 128, 96), (64, 64, 48, 96), (256, 128, 96, 144)]
CASES = [(loc, lay, sz) for loc in csm.LOCATIONS for lay in LAYOUTS for sz in SIZES]


@pytest.fixture(scope="module")
def table():
    """every case through ONE run of the host check: {case: (valid, shift_x, shift_y, h_centred, v_cosited)}"""
    if not os.path.exists(EXE):                        # built by `make product` (__graft_entry__.build())
        subprocess.run(["make", "-C", ROOT, "tools/chroma_siting_check"], capture_output=True, timeout=600)
    assert os.path.exists(EXE), "tools/chroma_siting_check is not built (make product)"
    args = []
    for loc, lay, sz in CASES:
        args += [loc, *LAYOUTS[lay], *sz]
    extra = [(-1, 1, 1, 64, 32, 64, 32), (7, 1, 1, 64, 32, 64, 32)]
    for e in extra:
        args += list(e)
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [l.split() for l in r.stdout.strip().split("\n")]
    assert len(rows) == len(CASES) + len(extra)
    out = {c: (int(v[0]), float(v[1]), float(v[2]), int(v[3]), int(v[4])) for c, v in zip(CASES, rows)}
    out["outside"] = [int(v[0]) for v in rows[len(CASES):]]
    return out


@pytest.mark.parametrize("loc,lay,sz", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_header_gives_the_models_shifts(table, loc, lay, sz):
    valid, sx, sy, hc, vc = table[(loc, lay, sz)]
    lw, lh = LAYOUTS[lay]
    sw, dw, sh, dh = sz
    want = csm.shifts(loc, lw, lh, sw, dw, sh, dh)
    assert valid == 1
    # one rounding in the model, three in the header: a few units of the last place of a number below 1
    assert abs(sx - want[0]) <= 2.0 ** -50 and abs(sy - want[1]) <= 2.0 ** -50, (sx, sy, want)
    left_sx = 0.25 * (1.0 - sw / dw) if lw else 0.0           # the expression crop/scale used before (tests/oracle_lib.py)
    top = 0.25 * (1.0 - sh / dh) if lh else 0.0
    if loc in (0, 1):
        assert sx == left_sx and sy == 0.0                    # bit for bit
    if loc == 2:
        assert sx == 0.0 and sy == 0.0
    if loc in (1, 3, 5):
        assert sx == left_sx
    if loc in (2, 4, 6):
        assert sx == 0.0
    if loc in (3, 4):
        assert sy == top                                      # the same expression in both directions
    if loc in (5, 6):
        assert sy == -top                                     # bottom is the negative of top
    if loc == 3 and lw and lh and sw * dh == sh * dw:
        assert sx == sy
    if lay == "444":
        assert sx == 0.0 and sy == 0.0                        # no siting without subsampling
    assert (bool(hc), bool(vc)) == csm.colour_forms(loc)


def test_locations_outside_the_enum_are_not_valid(table):
    assert table["outside"] == [0, 0]


def test_colour_forms_keep_vertical_bottom_centred():
    assert [csm.colour_forms(l) for l in range(7)] == [(False, False), (False, False), (True, False), (False, True),
                                                       (True, True), (False, False), (True, False)]


# ---- the direction of the shift, without the formula -----------------------------------------------------------------
SLOPE_X, SLOPE_Y, BASE, DEPTH = 40.0, 56.0, 8192.0, 16        # codes per LUMA sample; 16-bit samples


def _ramp(cw, ch, ox, oy):
    """a X + b Y at the luma coordinates of a cw x ch 4:2:0 chroma plane sited (ox, oy)"""
    x = csm.luma_position(np.arange(cw), ox)[None, :]
    y = csm.luma_position(np.arange(ch), oy)[:, None]
    return BASE + SLOPE_X * x + SLOPE_Y * y


def _deviation(loc, sw, sh, dw, dh, shifts_of):
    """largest |resized - ramp at the destination's sited positions| on interior samples, in codes"""
    ox, oy = csm.offsets(loc)
    src = np.rint(_ramp(sw // 2, sh // 2, ox, oy)).astype(np.uint16)
    sx, sy = csm.shifts(shifts_of, 1, 1, sw, dw, sh, dh)
    got = sl.cropscale_plane(src, dw // 2, dh // 2, sx, sy, DEPTH, "double").astype(np.float64)
    # the destination grid shows the same picture: luma coordinate X_d of the destination is X_d * src / dst of the source
    want = BASE + SLOPE_X * (csm.luma_position(np.arange(dw // 2), ox)[None, :] * sw / dw) \
                + SLOPE_Y * (csm.luma_position(np.arange(dh // 2), oy)[:, None] * sh / dh)
    m = 8                                                      # a Lanczos window (three source samples at 2 -> 1) from the edges
    return float(np.abs(got - want)[m:-m, m:-m].max())


@pytest.mark.parametrize("loc", [2, 3, 6])
@pytest.mark.parametrize("size", [(128, 96, 64, 48), (64, 48, 128, 96)], ids=["2to1", "1to2"])
def test_sited_shift_puts_the_ramp_where_the_destination_grid_is(built, loc, size):
    """A chroma ramp 40 X + 56 Y (codes per luma sample, 16-bit samples; luma is constant and left out) sampled at the
    sited positions of the source grid and scaled by orc_cropscale_plane_d under the model's shifts for the location
    must be the ramp at the sited positions of the destination grid; under the left-sited shifts (what crop/scale did
    for every location before) it is not.  Measured here on interior samples, in codes (every value of the ramp is a
    whole number, so the deviations are too) - sited / left-sited:
        2 -> 1 (128 x 96 -> 64 x 48):  location 2: 0 / 20    3: 1 / 28    6: 0 / 48
        1 -> 2 (64 x 48 -> 128 x 96):  location 2: 4 / 13    3: 3 / 17    6: 3 / 27
    The left-sited deviation is the quarter chroma sample per direction that differs: location 2 at 2 -> 1 is 0.25 of a
    source chroma sample of X = 0.25 * 2 * 40 = 20 codes; location 3 the same of Y = 28; location 6 both, with the sign
    of Y turned round.  The sited deviation is not a siting error: at location 2 both statements of the rule give the
    shift 0, and the 4 codes at 1 -> 2 are the Lanczos kernel's ripple on a ramp of 112 codes a sample (it does not
    reproduce a linear function exactly when interpolating), the same 3 to 4 codes at every location.
    Asserted: sited <= 4 codes, left-sited >= 13 codes, and left-sited at least three times the sited deviation (the
    smallest measured ratio is 13 / 4)."""
    sw, sh, dw, dh = size
    sited = _deviation(loc, sw, sh, dw, dh, loc)
    left = _deviation(loc, sw, sh, dw, dh, 1)
    print(f"location {loc} {sw}x{sh} -> {dw}x{dh}: sited {sited:.3f} codes, left-sited {left:.3f} codes")
    assert sited <= 4.0
    assert left >= 13.0 and left >= 3.0 * sited
