"""The speculative segments of handbrake_amd/csrc/hqdn3d.hip, on the CPU: the schedule's own claim (a segmented chain
with verify / repair equals the serial chain for ANY input) on many more cases than the GPU can afford, and the
condition that keeps the GPU tests of tests/test_hqdn3d_gpu.py honest: on the frames they run, with the warm-ups they
force, every kernel form at every depth has to repair segments both ways - re-walks that meet the stored results and
re-walks that run to the segment's end."""
import numpy as np
import pytest

import oracle_lib as ol
import hqdn3d_dev as hd
import hqdn3d_segment_model as m

W, H = 200, 150                     # the smallest shape at which every class occurs in every form (see the GPU tests)
DEPTHS = (8, 10, 12)


def _lut(depth, **par):
    return m.lut_list(ol.OrcHqdn3d(W, H, depth=depth, **par).coef[0])


def test_cut_rules():
    """the four cuts at the shapes of the GPU tests, worked out by hand from Hqdn3dFilter::one_frame / process_many"""
    assert m.cut("row-frame", 200) == (4, 64, 64) and m.live_segments(m.cut("row-frame", 200), 200) == [0, 1, 2, 3]
    assert m.cut("col-frame", 150) == (3, 50, 64)
    assert m.cut("row-batch", 200) == (8, 32, 64) and m.live_segments(m.cut("row-batch", 200), 200) == list(range(7))
    assert m.cut("col-batch", 150) == (4, 38, 64)
    assert m.cut("col-frame", 64).seg == 1 and m.cut("col-frame", 65).seg == 2      # height <= 64: a single segment
    assert m.cut("row-frame", 4096) == (32, 128, 64) and m.cut("col-frame", 2160) == (16, 135, 64)
    assert m.cut("row-batch", 1920, 3) == (8, 240, 3) and m.cut("col-batch", 1080) == (4, 270, 64)
    assert m.cut("row-batch", 18) == (6, 16, 64) and m.live_segments(m.cut("row-batch", 18), 18) == [0, 1]
    assert m.cut("col-batch", 10) == (4, 3, 64) and m.live_segments(m.cut("col-batch", 10), 10) == [0, 1, 2, 3]
    assert m.cut("col-batch", 50) == (4, 13, 64)


def _check(samples, lut, g, quirk, t16, what):
    stored, classes = m.segmented_chain(samples, lut, g, quirk, t16)
    assert stored == m.serial_chain(samples, lut, quirk, t16), what
    assert len(classes) == len(m.live_segments(g, len(samples))) - 1, what
    return classes


@pytest.mark.parametrize("form", m.FORMS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_segmented_walk_equals_the_serial_chain(built, depth, form):
    """Random chains (every jump resets the state), flat-noisy chains (the state forgets slowly or not at all), a chain
    that never forgets, chains shorter than one segment; warm-up 0, 3, 64, 1000; strengths 1, 4, 14; with and without
    the row 0 start.  Column forms truncate the state to 16 bits."""
    t16 = form.startswith("col")
    rng = np.random.default_rng(depth * 16 + m.FORMS.index(form))
    top, base = (1 << depth) - 1, 120 << (depth - 8)
    seen = set()
    for strength in (1, 4, 14):
        lut = _lut(depth, y_spatial=strength)
        for warm in (0, 3, 64, 1000):
            for n in (1, 2, 15, 17, 63, 64, 65, 130, 200, 517, 1100):
                g = m.cut(form, n, warm)
                for kind in ("random", "flat1", "flat3", "ends"):
                    px = {"random": lambda: rng.integers(0, top + 1, n),
                          "flat1": lambda: base + rng.integers(-1, 2, n),
                          "flat3": lambda: base + rng.integers(-3, 4, n),
                          "ends": lambda: rng.choice([0, 1, top - 1, top], n)}[kind]()
                    samples = [int(v) for v in m.to_state(px, depth)]
                    for quirk in ((False,) if t16 else (False, True)):
                        seen.update(_check(samples, lut, g, quirk, t16, f"strength {strength} warm {warm} n {n} {kind}"))
                if n < 16 and form != "col-batch":                                 # (a batched column is cut in 4 from 4 rows on)
                    assert len(m.live_segments(g, n)) == 1                         # shorter than one segment
            # never forgets: constant input, the true state one LUT bin above the one a segment guesses.  The first
            # sample puts the state on the fixed point of bin 1; a segment starts from the sample itself and stays on
            # the fixed point of bin 0 for good: every boundary whose warm-up does not reach the chain's first sample is
            # repaired to the segment's end - the serial walk
            n = 517
            c = int(m.to_state(np.array([base]), depth)[0])
            samples = [c + 24] + [c] * (n - 1)
            serial = m.serial_chain(samples, lut, False, t16)
            assert serial[-1] == serial[-2] and (serial[-1] - c) >> 4 == 1, "no fixed point in bin 1"
            g = m.cut(form, n, warm)
            classes = _check(samples, lut, g, False, t16, f"never forgets: strength {strength} warm {warm}")
            assert len(classes) >= 3
            seen.update(classes)
            assert classes == [m.EXACT if k * g.len <= warm else m.END for k in m.live_segments(g, n)[1:]]
    assert {m.EXACT, m.MET, m.END} <= seen


def _shares(depth, form, warms, par, frames):
    lut = _lut(depth, **par)
    idx = range(5) if form.endswith("frame") else hd.BATCHED_FRAMES
    tot = dict.fromkeys((m.EXACT, m.MET, m.END, m.LAST), 0)
    for i in idx:
        for warm in warms:
            for k, v in m.plane_classes(form, m.to_state(frames[i][0], depth), lut, warm).items():
                tot[k] += v
    return tot


@pytest.fixture(scope="module")
def frames():
    return {d: hd.segment_frames(W, H, d, 7) for d in DEPTHS}


@pytest.mark.parametrize("form", m.FORMS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_gpu_inputs_need_both_kinds_of_repair(built, frames, depth, form):
    """The luma planes the GPU segment tests run at 200 x 150 - the five frames of the drop-in test for the
    frame-at-a-time forms, the frames of the 3- and the 2-frame call of the process_dev test for the batched ones -
    with the warm-ups 0 and 3 together: `met` and `end` each at least 2 % of the form's segment boundaries and at least
    20 of them.  Which content carries it: with the STRONG settings (y-spatial 14) the flat-noisy frames do at every
    depth and in every form.  With the default strength (4) they do at 10 and 12 bits; at 8 bits a column chain on
    them always forgets within a segment (`end` 0 of 4000 frame-at-a-time, 7 of 6000 batched; 1.8 % in batched rows),
    so there the default settings exercise little but `met` - the GPU tests run both settings on the same frames."""
    for name, par in (("strong", hd.STRONG[1]), ("default", {})):
        tot = _shares(depth, form, (0, 3), par, frames[depth])
        n = sum(tot.values())
        print(f"hqdn3d segments {name:7s} depth {depth:2d} {form:9s} boundaries {n}: "
              + "  ".join(f"{k} {100 * v / n:.1f} %" for k, v in tot.items()))
        if name == "default" and depth == 8:
            continue                                        # (printed, not asserted: see above)
        for k in (m.MET, m.END):
            assert tot[k] >= 20 and tot[k] >= 0.02 * n, f"{name} {form} depth {depth}: {k} {tot[k]} of {n}"


@pytest.mark.parametrize("depth", [10, 12])
def test_shipped_warmup_needs_repairs_above_8_bits(built, frames, depth):
    """With the shipped warm-up of 64 the same content needs repairs at 10 and 12 bits, in every form: the GPU tests'
    hook-less case is more than a happy path there.  (At 8 bits and the default strength none is needed.)"""
    for form in m.FORMS:
        tot = _shares(depth, form, (m.WARM,), {}, frames[depth])
        print(f"hqdn3d segments shipped warm-up depth {depth} {form:9s}: " + "  ".join(f"{k} {v}" for k, v in tot.items()))
        assert tot[m.MET] + tot[m.END] + tot[m.LAST] >= 1, form


@pytest.mark.parametrize("depth", DEPTHS)
def test_rails_wrap_the_vertical_result(built, depth):
    """What hqdn3d_tn_kernel relies on, and the condition that the GPU rails test meets it: the vertical result goes to
    the next row through a uint16 and to the temporal step in 32 bits, and the batched form stores the uint16 only.
    On the rails frames (hqdn3d_dev.rails), every plane, default and strong settings:
      - a 32-bit vertical result is never farther than 7 from [0, 65535], so its low 16 bits are within 7 of an end
        where it left the range (the kernel rebuilds within 16);
      - an h-filtered sample always fits 16 bits (what the kernel rebuilds from);
      - results past 65535 do occur: at 12 bits on the flat all-max frame with either setting, at 10 bits on the CLIMB
        frame with the strong settings, at least 20 luma samples each.  (At 8 bits neither setting gets there.)"""
    fr = hd.rails(W, H, depth)
    past = {}
    for name, par in (("default", {}), ("strong", hd.STRONG[1])):
        orc = ol.OrcHqdn3d(W, H, depth=depth, **par)
        for c in range(3):
            lut = m.lut_list(orc.coef[2 * c])
            for t, f in enumerate(fr):
                hp = m.h_filter_plane(m.to_state(f[c], depth), lut)
                assert 0 <= hp.min() and hp.max() <= 0xffff, f"{name} frame {t} plane {c}: h-filtered sample out of 16 bits"
                v = m.v_filter_plane(hp, lut)
                assert -7 <= v.min() and v.max() <= 0xffff + 7, f"{name} frame {t} plane {c}"
                if c == 0:
                    past[name, t] = int((v > 0xffff).sum())
    print(f"hqdn3d rails depth {depth}: luma vertical results past 65535 per (setting, frame): "
          + str({k: n for k, n in past.items() if n}))
    if depth == 12:
        assert past["default", 1] >= 20 and past["strong", 1] >= 20
    if depth == 10:
        assert past["strong", 8] >= 20
