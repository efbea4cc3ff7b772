"""The catalogue of NLMeans kernel forms (tests/nlmeans_forms.py) held against the host planner (hbhip_nlmeans_plan, what
the filter dispatches from): every case takes the form it names, a sweep of the planner finds no form without a case,
and every kernel instantiation is either a case's form or listed as unreachable.  No device is needed: the planner is
host arithmetic on the settings."""
import pytest

from handbrake_amd import hip
import nlmeans_forms as nf


@pytest.mark.parametrize("case", nf.CASES, ids=repr)
def test_a_case_takes_the_form_it_names(built, case):
    launches = nf.plan(case.planes, case.depth)
    assert [nf.form_of(L) for L in launches] == case.forms
    for L in launches:
        bits = 16 if L["wide"] else 8
        assert bits == (8 if case.depth == 8 else 16)
        assert L["planes"] == sum(1 << c for c, p in enumerate(case.planes) if p["strength"] != 0 and p["patch"] == L["patch_size"])
        assert L["max_rh"] == max((p["range"] - 1) // 2 for p in case.planes if p["patch"] == L["patch_size"])
        if L["generic"]:
            assert (L["tile_w"], L["tile_h"]) == (32, 8) and L["cmp_rows"] == 0
            continue
        # the tile: its rows, and the bytes of the two (four with a prefilter) tiles and the table - or, for the pairs,
        # of one tile and the larger of a tile and the stash
        assert (L["tile_w"], L["tile_h"]) == (120, 64)
        assert L["cmp_rows"] == 64 + 2 * (L["patch_size"] // 2 + L["max_rh"])
        tile = 4 * (L["pitch"] * L["cmp_rows"] + 4)
        if L["fast"] == 3:
            assert L["lds_bytes"] == 512 + tile + max(tile, 4 * L["pairs"] * 9 * 256)
        else:
            assert L["lds_bytes"] == 512 + (4 if L["pre"] else 2) * tile
        assert L["lds_bytes"] <= 160 * 1024                    # what a gfx950 workgroup can have


def test_the_case_names_are_distinct():
    names = [c.name for c in nf.CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", nf.STRONG_8BIT, ids=repr)
def test_strong_8bit_cases_are_form_1_for_the_cause_they_name(built, case):
    (L,) = nf.plan(case.planes, case.depth)
    assert L["fast"] == 1 and not L["wide"]
    for c in range(3):
        assert L["diff_cap"][c] >= 0
        if case.name.endswith("ishift"):
            assert L["imul4"][c] != 0 and L["ishift"][c] != 0
        else:
            assert case.name.endswith("nomul") and L["imul4"][c] == 0


def test_both_causes_of_form_1_under_strong_denoising_have_a_case():
    assert sorted(c.name.rsplit("-", 1)[1] for c in nf.STRONG_8BIT) == ["ishift", "nomul"]


def catalogued():
    return {f for c in nf.CASES for f in c.forms}


def test_the_sweep_finds_no_form_without_a_case(built):
    found = nf.sweep()
    missing = {f: found[f] for f in found if f not in catalogued()}
    assert not missing, "forms the planner gives that no case of the catalogue takes: " + \
        "; ".join(f"{nf.name_of(f)} (depth {d}: {nf.settings(p)})" for f, (d, p) in sorted(missing.items()))
    hit = sorted(nf.name_of(f) for f in found if f in nf.UNREACHABLE)
    assert not hit, f"listed as unreachable, but the planner gives them: {hit}"


def test_every_instantiation_is_a_case_or_listed_as_unreachable(built):
    inst = nf.instantiations()
    have = catalogued()
    assert not (have & set(nf.UNREACHABLE))
    unknown = sorted(nf.name_of(f) for f in inst - have - set(nf.UNREACHABLE))
    assert not unknown, f"kernel instantiations without a case in tests/nlmeans_forms.py: {unknown}"
    gone = sorted(nf.name_of(f) for f in (have | set(nf.UNREACHABLE)) - inst)
    assert not gone, f"forms of the catalogue the dispatcher holds no kernel for: {gone}"
    assert all(reason for reason in nf.UNREACHABLE.values())


def test_what_no_build_does(built):
    """the two exclusions that are not instantiations: the form list has no pairs' kernel at patch 9 that IS form 3, and
    no plan of the sweep searches the job table (sweep() asserts job_arith of every launch it plans)"""
    assert set(nf.EXCLUDED) == {"pairs at patch 9", "job table search"}
    assert not [f for f in hip.nlmeans_forms() if f["fast"] == 3 and f["patch_size"] > 7]
    assert all(L["job_arith"] == 1 for c in nf.CASES for L in nf.plan(c.planes, c.depth))


def test_the_planner_declines_what_the_filter_declines(built):
    """HBHIP_ERR_UNSUPPORTED for a plane under 16 pixels and for a reach past the 16-pixel border; neither needs a device"""
    p = nf.plane(6, 7, 3)
    with pytest.raises(hip.HipError):
        nf.plan((p, p, p), 8, w=30, h=32)                          # 4:2:0: chroma 15 x 16
    with pytest.raises(hip.HipError):
        nf.plan((p, p, p), 8, w=15, h=16, lcw=0, lch=0)
    assert len(nf.plan((p, p, p), 8, w=16, h=16, lcw=0, lch=0)) == 1
    q = nf.plane(6, 5, 31)                                         # reach 2 + 15 = 17
    with pytest.raises(hip.HipError):
        nf.plan((q, q, q), 8)
    assert len(nf.plan((nf.plane(6, 5, 29),) * 3, 8)) == 1
