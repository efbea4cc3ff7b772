"""The kernel forms NLMeans can run, and settings that reach each of them.

A frame is filtered by one launch per distinct patch size, and a launch runs one of several dozen kernel instantiations,
chosen by the host planner (hbhip_nlmeans_plan, csrc/nlmeans.hip) from the settings and the bit depth.  This module names
a form by the fields of the plan that select its kernel, lists one case of settings per form the planner can give, and
lists the instantiations it can never give, with the reason.  tests/test_nlmeans_forms_cpu.py holds the list against the
planner (every case takes the form it says; a sweep of the planner finds no form without a case; every instantiation is
in one list or the other); tests/test_nlmeans_forms_gpu.py runs every case against the oracle.

The strengths were found with the planner (the sweep below, printed per form), not worked out by hand: which index form
a plane takes depends on float rounding in weight_fact_table = 16.84 / (patch * strength)^2, strength times
(depth - 8)^2 at 10 / 12 bits."""
import functools
import itertools

from handbrake_amd import hip

TUNED = (3, 5, 7, 9)                    # patch sizes of the lane-sharing kernels; every other size is the generic kernel's
W, H = 250, 134                         # the frame the cases are planned (and run) at, 4:2:0


def plane(strength, patch, rng, origin=1.0, frames=2, prefilter=0):
    """one plane's settings, in the oracle's names (golden_cases.nlm)"""
    return dict(strength=strength, origin_tune=origin, patch=patch, range=rng, nframes=frames, prefilter=prefilter)


def settings(planes):
    """the filter's settings string of three planes"""
    return ":".join(f"{name}-strength={p['strength']}:{name}-origin-tune={p['origin_tune']}:{name}-patch-size={p['patch']}:"
                    f"{name}-range={p['range']}:{name}-frame-count={p['nframes']}:{name}-prefilter={p['prefilter']}"
                    for name, p in zip(("y", "cb", "cr"), planes))


def oracle_params(planes, depth):
    return [dict(p, depth=depth) for p in planes]


# ---- forms -------------------------------------------------------------------------------------------------------------
def lanes(bits, patch, fast, pitch, pre=0, pairs=0, origin_f32=0):
    """nlmeans_lanes_kernel (bits 8) / nlmeans_lanes16_kernel (bits 16) <patch, fast, pitch, pre, ...>"""
    return ("lanes", bits, patch, fast, pitch, pre, pairs, origin_f32)


def generic(bits, pre=0):
    """nlmeans_generic_kernel<uint8_t | uint16_t>; the patch size and the prefilter flag are kernel arguments"""
    return ("generic", bits, pre)


def form_of(launch):
    """the form of a launch of a plan, or of an entry of hip.nlmeans_forms()"""
    bits = 16 if launch["wide"] else 8
    if launch["generic"]:
        return generic(bits, launch["pre"])
    return lanes(bits, launch["patch_size"], launch["fast"], launch["pitch"], launch["pre"], launch["pairs"], launch["origin_f32"])


def plan(planes, depth, w=W, h=H, lcw=1, lch=1):
    return hip.nlmeans_plan(settings(planes), w, h, depth, lcw, lch)


def forms_of(planes, depth, **geo):
    return [form_of(L) for L in plan(planes, depth, **geo)]


def instantiations():
    """every form the dispatcher holds a kernel for (the generic kernels with and without their prefilter argument)"""
    out = set()
    for f in hip.nlmeans_forms():
        out |= {generic(16 if f["wide"] else 8, 0), generic(16 if f["wide"] else 8, 1)} if f["generic"] else {form_of(f)}
    return out


def name_of(form):
    if form[0] == "generic":
        return f"generic{form[1]}" + ("-pre" if form[2] else "")
    _, bits, patch, fast, pitch, pre, pairs, origin_f32 = form
    return f"lanes{bits}-n{patch}-fast{fast}-pitch{pitch}" + ("-pre" if pre else "") + (f"-pairs{pairs}" if pairs else "") + \
        ("-org1" if origin_f32 else "")


# ---- the sweep ---------------------------------------------------------------------------------------------------------
DEPTHS = (8, 10, 12)
PATCHES = tuple(range(1, 18, 2))
RANGES = tuple(range(1, 32, 2))
STRENGTHS = (0.02, 0.05, 0.1, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.6, 0.7, 0.75, 0.85, 1, 1.2, 1.5, 1.75, 2, 2.5, 3, 3.5, 4.5, 6, 7.5, 9,
             12, 15.5, 20, 27, 33, 40)
BORDER = 16                             # the reach limit: patch // 2 + range // 2 <= 16


def index_class(launch, c=0):
    """which index form plane c of a launch allows on its own: 0 gated, 1 clamp, 2 integer multiply-high"""
    if launch["diff_cap"][c] < 0:
        return 0
    return 2 if launch["imul4"][c] != 0 and (launch["wide"] or launch["ishift"][c] == 0) else 1


@functools.lru_cache(maxsize=None)
def sweep():
    """{form: (depth, planes) of the first settings that gave it} over
    depth 8 / 10 / 12 x patch 1..17 x the strength grid (one plane, to learn the index class of every strength), and then,
    for every depth, patch and index class, at the weakest strength of the class (the classes are a property of depth,
    patch and strength alone: index_class() reads them off the plan's per-plane constants): one plane at every range within
    the reach limit x origin-tune 1 / 0.5 x prefilter off / on; two and three planes sharing the patch size at ranges
    that differ (1, 3, 9, 11, 17, 19 and the widest), their index classes, origin-tunes and prefilters mixed."""
    found = {}

    def note(depth, planes):
        for L in plan(planes, depth):
            assert L["job_arith"] == 1
            found.setdefault(form_of(L), (depth, planes))

    off = plane(0, 7, 3)
    for depth, patch in itertools.product(DEPTHS, PATCHES):
        by_class = {}
        for s in STRENGTHS:
            planes = (plane(s, patch, 3), off, off)
            note(depth, planes)
            by_class.setdefault(index_class(plan(planes, depth)[0]), s)
        ranges = [r for r in RANGES if patch // 2 + r // 2 <= BORDER]
        some = sorted({r for r in (1, 3, 9, 11, 17, 19, ranges[-1]) if r in ranges})
        classes = sorted(by_class)
        for k in classes:
            for r, origin, pf in itertools.product(ranges, (1.0, 0.5), (0, 1)):
                note(depth, (plane(by_class[k], patch, r, origin, prefilter=pf), off, off))
        for (ka, kb), (ra, rb), (oa, ob), (pa, pb) in itertools.product(itertools.combinations_with_replacement(classes, 2),
                                                                      itertools.combinations_with_replacement(some, 2),
                                                                      ((1.0, 1.0), (1.0, 0.5)), ((0, 0), (0, 1), (1, 1))):
            a, b = plane(by_class[ka], patch, ra, oa, prefilter=pa), plane(by_class[kb], patch, rb, ob, prefilter=pb)
            note(depth, (a, b, off))
            note(depth, (a, b, plane(by_class[classes[-1]], patch, some[0], 1.0)))
            note(depth, (b, a, plane(by_class[classes[0]], patch, some[-1], 0.5, prefilter=1)))
    return found


# ---- the catalogue -----------------------------------------------------------------------------------------------------
class Case:
    """settings (three planes), a depth, and the forms its launches take, in launch order (ascending patch size)"""
    def __init__(self, depth, planes, forms, note=""):
        self.depth, self.planes, self.forms = depth, tuple(planes), list(forms)
        self.name = f"{depth}bit-" + "+".join(name_of(f) for f in forms) + (f"-{note}" if note else "")

    def __repr__(self):
        return self.name


P = plane


def C(depth, p, *forms, note=""):
    """a case whose three planes have the same settings: one launch, luma and both chroma planes in it"""
    return Case(depth, (p, p, p), forms, note)


# One case per lane-sharing form, every plane of the frame in its one launch.  The range is the widest its tile pitch
# takes (9 / 17 at pitch 36 / 76; the reach limit at pitch 44 / 84; 3 for the pairs), so that the staged tile has the
# most rows the instantiation is sized for; the strength is the middle one of the sweep's strengths that give the
# form's index class at that depth and patch size.
CASES = [
    C(8, P(0.35, 3, 9), lanes(8, 3, 0, 36, 0, 0, 0)),
    C(8, P(0.35, 3, 9, 1.0, prefilter=1), lanes(8, 3, 0, 36, 1, 0, 0)),
    C(8, P(0.35, 3, 31), lanes(8, 3, 0, 44, 0, 0, 0)),
    C(8, P(0.35, 3, 31, 1.0, prefilter=1), lanes(8, 3, 0, 44, 1, 0, 0)),
    C(8, P(1.5, 3, 9), lanes(8, 3, 1, 36, 0, 0, 0)),
    C(8, P(1.5, 3, 9, 1.0, prefilter=1), lanes(8, 3, 1, 36, 1, 0, 0)),
    C(8, P(1.5, 3, 31), lanes(8, 3, 1, 44, 0, 0, 0)),
    C(8, P(1.5, 3, 31, 1.0, prefilter=1), lanes(8, 3, 1, 44, 1, 0, 0)),
    C(8, P(12, 3, 9), lanes(8, 3, 2, 36, 0, 0, 0)),
    C(8, P(12, 3, 9, 1.0, prefilter=1), lanes(8, 3, 2, 36, 1, 0, 0)),
    C(8, P(12, 3, 31), lanes(8, 3, 2, 44, 0, 0, 0)),
    C(8, P(12, 3, 31, 1.0, prefilter=1), lanes(8, 3, 2, 44, 1, 0, 0)),
    C(8, P(12, 3, 3, 0.5), lanes(8, 3, 3, 36, 0, 4, 0)),
    C(8, P(12, 3, 3), lanes(8, 3, 3, 36, 0, 4, 1)),
    C(8, P(0.35, 5, 9), lanes(8, 5, 0, 36, 0, 0, 0)),
    C(8, P(0.35, 5, 9, 1.0, prefilter=1), lanes(8, 5, 0, 36, 1, 0, 0)),
    C(8, P(0.35, 5, 29), lanes(8, 5, 0, 44, 0, 0, 0)),
    C(8, P(0.35, 5, 29, 1.0, prefilter=1), lanes(8, 5, 0, 44, 1, 0, 0)),
    C(8, P(1, 5, 9), lanes(8, 5, 1, 36, 0, 0, 0)),
    C(8, P(1, 5, 9, 1.0, prefilter=1), lanes(8, 5, 1, 36, 1, 0, 0)),
    C(8, P(1, 5, 29), lanes(8, 5, 1, 44, 0, 0, 0)),
    C(8, P(1, 5, 29, 1.0, prefilter=1), lanes(8, 5, 1, 44, 1, 0, 0)),
    C(8, P(6, 5, 9), lanes(8, 5, 2, 36, 0, 0, 0)),
    C(8, P(6, 5, 9, 1.0, prefilter=1), lanes(8, 5, 2, 36, 1, 0, 0)),
    C(8, P(6, 5, 29), lanes(8, 5, 2, 44, 0, 0, 0)),
    C(8, P(6, 5, 29, 1.0, prefilter=1), lanes(8, 5, 2, 44, 1, 0, 0)),
    C(8, P(6, 5, 3, 0.5), lanes(8, 5, 3, 36, 0, 4, 0)),
    C(8, P(6, 5, 3), lanes(8, 5, 3, 36, 0, 4, 1)),
    C(8, P(0.25, 7, 9), lanes(8, 7, 0, 36, 0, 0, 0)),
    C(8, P(0.25, 7, 9, 1.0, prefilter=1), lanes(8, 7, 0, 36, 1, 0, 0)),
    C(8, P(0.25, 7, 27), lanes(8, 7, 0, 44, 0, 0, 0)),
    C(8, P(0.25, 7, 27, 1.0, prefilter=1), lanes(8, 7, 0, 44, 1, 0, 0)),
    C(8, P(0.75, 7, 9), lanes(8, 7, 1, 36, 0, 0, 0)),
    C(8, P(0.75, 7, 9, 1.0, prefilter=1), lanes(8, 7, 1, 36, 1, 0, 0)),
    C(8, P(0.75, 7, 27), lanes(8, 7, 1, 44, 0, 0, 0)),
    C(8, P(0.75, 7, 27, 1.0, prefilter=1), lanes(8, 7, 1, 44, 1, 0, 0)),
    C(8, P(4.5, 7, 9), lanes(8, 7, 2, 36, 0, 0, 0)),
    C(8, P(4.5, 7, 9, 1.0, prefilter=1), lanes(8, 7, 2, 36, 1, 0, 0)),
    C(8, P(4.5, 7, 27), lanes(8, 7, 2, 44, 0, 0, 0)),
    C(8, P(4.5, 7, 27, 1.0, prefilter=1), lanes(8, 7, 2, 44, 1, 0, 0)),
    C(8, P(4.5, 7, 3, 0.5), lanes(8, 7, 3, 36, 0, 4, 0)),
    C(8, P(4.5, 7, 3), lanes(8, 7, 3, 36, 0, 4, 1)),
    C(8, P(0.1, 9, 9), lanes(8, 9, 0, 36, 0, 0, 0)),
    C(8, P(0.1, 9, 9, 1.0, prefilter=1), lanes(8, 9, 0, 36, 1, 0, 0)),
    C(8, P(0.1, 9, 25), lanes(8, 9, 0, 44, 0, 0, 0)),
    C(8, P(0.1, 9, 25, 1.0, prefilter=1), lanes(8, 9, 0, 44, 1, 0, 0)),
    C(8, P(0.7, 9, 9), lanes(8, 9, 1, 36, 0, 0, 0)),
    C(8, P(0.7, 9, 9, 1.0, prefilter=1), lanes(8, 9, 1, 36, 1, 0, 0)),
    C(8, P(0.7, 9, 25), lanes(8, 9, 1, 44, 0, 0, 0)),
    C(8, P(0.7, 9, 25, 1.0, prefilter=1), lanes(8, 9, 1, 44, 1, 0, 0)),
    C(8, P(3.5, 9, 9), lanes(8, 9, 2, 36, 0, 0, 0)),
    C(8, P(3.5, 9, 9, 1.0, prefilter=1), lanes(8, 9, 2, 36, 1, 0, 0)),
    C(8, P(3.5, 9, 25), lanes(8, 9, 2, 44, 0, 0, 0)),
    C(8, P(3.5, 9, 25, 1.0, prefilter=1), lanes(8, 9, 2, 44, 1, 0, 0)),
    C(12, P(0.05, 3, 17), lanes(16, 3, 0, 76, 0, 0, 0)),
    C(10, P(0.1, 3, 17, 1.0, prefilter=1), lanes(16, 3, 0, 76, 1, 0, 0)),
    C(12, P(0.05, 3, 31), lanes(16, 3, 0, 84, 0, 0, 0)),
    C(10, P(0.1, 3, 31, 1.0, prefilter=1), lanes(16, 3, 0, 84, 1, 0, 0)),
    C(10, P(0.5, 3, 17), lanes(16, 3, 1, 76, 0, 0, 0)),
    C(12, P(9, 3, 17, 1.0, prefilter=1), lanes(16, 3, 1, 76, 1, 0, 0)),
    C(10, P(0.5, 3, 31), lanes(16, 3, 1, 84, 0, 0, 0)),
    C(12, P(9, 3, 31, 1.0, prefilter=1), lanes(16, 3, 1, 84, 1, 0, 0)),
    C(12, P(0.85, 3, 17), lanes(16, 3, 2, 76, 0, 0, 0)),
    C(10, P(2.5, 3, 17, 1.0, prefilter=1), lanes(16, 3, 2, 76, 1, 0, 0)),
    C(12, P(0.85, 3, 31), lanes(16, 3, 2, 84, 0, 0, 0)),
    C(10, P(2.5, 3, 31, 1.0, prefilter=1), lanes(16, 3, 2, 84, 1, 0, 0)),
    C(10, P(2.5, 3, 3), lanes(16, 3, 3, 76, 0, 3, 0)),
    C(10, P(0.05, 5, 17), lanes(16, 5, 0, 76, 0, 0, 0)),
    C(12, P(0.02, 5, 17, 1.0, prefilter=1), lanes(16, 5, 0, 76, 1, 0, 0)),
    C(10, P(0.05, 5, 29), lanes(16, 5, 0, 84, 0, 0, 0)),
    C(12, P(0.02, 5, 29, 1.0, prefilter=1), lanes(16, 5, 0, 84, 1, 0, 0)),
    C(12, P(7.5, 5, 17), lanes(16, 5, 1, 76, 0, 0, 0)),
    C(10, P(7.5, 5, 17, 1.0, prefilter=1), lanes(16, 5, 1, 76, 1, 0, 0)),
    C(12, P(7.5, 5, 29), lanes(16, 5, 1, 84, 0, 0, 0)),
    C(10, P(7.5, 5, 29, 1.0, prefilter=1), lanes(16, 5, 1, 84, 1, 0, 0)),
    C(10, P(1.75, 5, 17), lanes(16, 5, 2, 76, 0, 0, 0)),
    C(12, P(0.75, 5, 17, 1.0, prefilter=1), lanes(16, 5, 2, 76, 1, 0, 0)),
    C(10, P(1.75, 5, 29), lanes(16, 5, 2, 84, 0, 0, 0)),
    C(12, P(0.75, 5, 29, 1.0, prefilter=1), lanes(16, 5, 2, 84, 1, 0, 0)),
    C(12, P(0.75, 5, 3), lanes(16, 5, 3, 76, 0, 3, 0)),
    C(10, P(0.05, 7, 17), lanes(16, 7, 0, 76, 0, 0, 0)),
    C(10, P(0.05, 7, 17, 1.0, prefilter=1), lanes(16, 7, 0, 76, 1, 0, 0)),
    C(10, P(0.05, 7, 27), lanes(16, 7, 0, 84, 0, 0, 0)),
    C(10, P(0.05, 7, 27, 1.0, prefilter=1), lanes(16, 7, 0, 84, 1, 0, 0)),
    C(10, P(20, 7, 17), lanes(16, 7, 1, 76, 0, 0, 0)),
    C(12, P(7.5, 7, 17, 1.0, prefilter=1), lanes(16, 7, 1, 76, 1, 0, 0)),
    C(10, P(20, 7, 27), lanes(16, 7, 1, 84, 0, 0, 0)),
    C(12, P(7.5, 7, 27, 1.0, prefilter=1), lanes(16, 7, 1, 84, 1, 0, 0)),
    C(12, P(0.6, 7, 17), lanes(16, 7, 2, 76, 0, 0, 0)),
    C(10, P(1.5, 7, 17, 1.0, prefilter=1), lanes(16, 7, 2, 76, 1, 0, 0)),
    C(12, P(0.6, 7, 27), lanes(16, 7, 2, 84, 0, 0, 0)),
    C(10, P(1.5, 7, 27, 1.0, prefilter=1), lanes(16, 7, 2, 84, 1, 0, 0)),
    C(10, P(1.5, 7, 3), lanes(16, 7, 3, 76, 0, 3, 0)),
    C(10, P(0.05, 9, 17), lanes(16, 9, 0, 76, 0, 0, 0)),
    C(10, P(0.05, 9, 17, 1.0, prefilter=1), lanes(16, 9, 0, 76, 1, 0, 0)),
    C(10, P(0.05, 9, 25), lanes(16, 9, 0, 84, 0, 0, 0)),
    C(10, P(0.05, 9, 25, 1.0, prefilter=1), lanes(16, 9, 0, 84, 1, 0, 0)),
    C(12, P(6, 9, 17), lanes(16, 9, 1, 76, 0, 0, 0)),
    C(10, P(15.5, 9, 17, 1.0, prefilter=1), lanes(16, 9, 1, 76, 1, 0, 0)),
    C(12, P(6, 9, 25), lanes(16, 9, 1, 84, 0, 0, 0)),
    C(10, P(15.5, 9, 25, 1.0, prefilter=1), lanes(16, 9, 1, 84, 1, 0, 0)),
    C(10, P(1, 9, 17), lanes(16, 9, 2, 76, 0, 0, 0)),
    C(12, P(0.5, 9, 17, 1.0, prefilter=1), lanes(16, 9, 2, 76, 1, 0, 0)),
    C(10, P(1, 9, 25), lanes(16, 9, 2, 84, 0, 0, 0)),
    C(12, P(0.5, 9, 25, 1.0, prefilter=1), lanes(16, 9, 2, 84, 1, 0, 0)),
]

# nlmeans_generic_kernel: the patch size and the prefilter flag are arguments, the sample type the only instantiation
CASES += [
    C(8, P(6, 11, 5), generic(8)),
    C(8, P(5, 13, 3, 0.8, prefilter=2), generic(8, 1)),
    C(10, P(3, 15, 3), generic(16)),
    C(12, P(2, 1, 7, 0.9, prefilter=1), generic(16, 1)),
]

# Strong denoising at 8 bits (patch x strength of roughly 185 and up): the table's factor is so small that its integer
# multiplier needs a shift (ishift != 0), which the 8-bit kernels do not have, or that no multiplier reproduces the
# float index (imul4 == 0).  Either way the plane takes the float clamp form: the same kernels as the form-1 cases
# above, reached the other way.  (test_nlmeans_forms_cpu.py holds each case to the cause its note names.)
STRONG_8BIT = [
    C(8, P(27, 7, 27, 0.7), lanes(8, 7, 1, 44), note="ishift"),
    C(8, P(33, 9, 9, prefilter=1), lanes(8, 9, 1, 36, 1), note="nomul"),
]
CASES += STRONG_8BIT

# Instantiations no settings reach, and why.  Everything hip.nlmeans_forms() lists is either a form of a case above or
# in here.
UNREACHABLE = {}
for _n in (3, 5, 7):
    for _org in (0, 1):
        UNREACHABLE[lanes(8, _n, 3, 44, 0, 4, _org)] = \
            "the pairs run only when every plane of the launch searches 3 x 3, and a half-range of 1 never takes the wide pitch"
for _f in (lanes(8, 9, 2, 36, 0, 0, 1), lanes(8, 9, 2, 44, 0, 0, 1), lanes(16, 9, 2, 76, 0, 3, 0)):
    UNREACHABLE[_f] = ("what the pairs' kernel comes to at patch 9, where it falls back to form 2 (the pairs' sharing stops at "
                      "patch 7, by a static_assert): the planner gives patch 9 the plain form-2 kernel")

# What the source could do but no build does: not instantiations, so hip.nlmeans_forms() cannot list them.
# test_nlmeans_forms_cpu.py holds each to what the planner and the form list say.
EXCLUDED = {
    "pairs at patch 9": "FAST 3 with N = 9 fails the kernels' static_assert (a lane's window would reach past its neighbour)",
    "job table search": "the binary search for a tile's job runs only where NLM_JOB_ARITH is 0; every plan has job_arith 1",
}
