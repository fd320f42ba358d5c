"""CPU test of the one routing of the 8-bit NV12 warps (warp_route, csrc/vstab_warp_request.hpp; DESIGN.md, "Warp routing"), through the
vstabx_warp_route hook: request -> (kernel family, argument block, kernel mode tag).  The rows were written from the three routing sites the
function replaced -- the ladders of vstab_warp_nv12_rs_ex and vstab_warp_nv12_pinhole and the 8-bit half of the pipeline's launch_warp --,
one at least per branch of each, and from the argument checks for what has no route.  profiles/warp_request_routes.txt holds the kernels
both versions launched for every servable row."""
import ctypes

import pytest

# the request: map modes, lens, resampler, the entry point's border mode (none; its own kernels; an option beside a resampler), border, format
IDEAL, FISH, RECTD, RECTD0 = 0, 1, 2, 3
DEFAULT, CUBIC, LANCZOS4 = 0, 2, 4
NONE, OWN, OPTION = 0, 1, 2
CONSTANT, REPLICATE, REFLECT, REFLECT_101 = 0, 1, 2, 4
BGR8, NV12, PLANAR = 0, 1, 2
# the route: family, argument block, mode tag (csrc/vstab_map.hpp, MapMode)
NO_ROUTE, K_FUSED, K_PLANAR, K_BORDER, K_CUBIC, K_LANCZOS4, K_KEEP = range(7)
WARP_ARGS, CUBIC_ARGS, BORDER_ARGS, KEEP_ARGS = range(4)
RS0, RS1, RS5, FISHD_RECT, FISHD_FISH, RS_FISHD, RECTD_RECT, RECTD_FISH = 6, 7, 8, 9, 10, 11, 12, 13
RS_TAG = {0: RS0, 1: RS1, 5: RS5}
BORDERS, MODES = (CONSTANT, REPLICATE, REFLECT, REFLECT_101), range(6)


def req(mode, lens=IDEAL, rs=0, resample=DEFAULT, entry=NONE, border=CONSTANT, fmt=BGR8, keep=0, qmap=0):
    return (mode, lens, rs, resample, entry, border, fmt, keep, qmap)


ROWS = []
# ---- vstab_warp_nv12_rs_ex's ladder (the border mode is an option) --------------------------------------------------------------------
# 1. no rotation, dist: vstab_warp_nv12_dist_ex's tail -- the resampler's kernels over CubicArgs, k_warp_border under a non-constant
#    border, else the bilinear kernels of vstab_warp_nv12_dist
for mode, tag in ((1, FISHD_RECT), (2, FISHD_FISH)):
    for b in BORDERS:
        ROWS += [(req(mode, FISH, 0, CUBIC, OPTION, b), (K_CUBIC, CUBIC_ARGS, tag)), (req(mode, FISH, 0, LANCZOS4, OPTION, b, PLANAR), (K_LANCZOS4, CUBIC_ARGS, tag))]
    for b in BORDERS[1:]:
        ROWS += [(req(mode, FISH, 0, DEFAULT, OPTION, b), (K_BORDER, BORDER_ARGS, tag)), (req(mode, FISH, 0, DEFAULT, OPTION, b, PLANAR), (K_BORDER, BORDER_ARGS, tag))]
    ROWS += [(req(mode, FISH, 0, DEFAULT, OPTION, CONSTANT), (K_FUSED, WARP_ARGS, tag)), (req(mode, FISH, 0, DEFAULT, OPTION, CONSTANT, PLANAR), (K_PLANAR, WARP_ARGS, tag))]
# 2. the default resampler, no dist: no rotation and the constant border is vstab_warp_nv12_ex, everything else vstab_warp_nv12_border
for mode in MODES:
    ROWS += [(req(mode, entry=OPTION), (K_FUSED, WARP_ARGS, mode)), (req(mode, entry=OPTION, fmt=PLANAR), (K_PLANAR, WARP_ARGS, mode))]
    ROWS += [(req(mode, entry=OPTION, border=b), (K_BORDER, BORDER_ARGS, mode)) for b in BORDERS[1:]]
for mode in (0, 1, 5):
    ROWS += [(req(mode, rs=1, entry=OPTION, border=b), (K_BORDER, BORDER_ARGS, RS_TAG[mode])) for b in BORDERS]   # the constant border too
    ROWS += [(req(mode, rs=1, entry=OPTION, fmt=PLANAR), (K_BORDER, BORDER_ARGS, RS_TAG[mode]))]
# 3. no rotation under a resampler: vstab_warp_nv12_cubic / _lanczos4, with a border mode their _border forms (the same kernels' family)
for mode in MODES:
    for b in BORDERS:
        ROWS += [(req(mode, resample=CUBIC, entry=OPTION, border=b), (K_CUBIC, CUBIC_ARGS, mode)),
                 (req(mode, resample=LANCZOS4, entry=OPTION, border=b, fmt=PLANAR), (K_LANCZOS4, CUBIC_ARGS, mode))]
# 4. new ground: a rotation per row under the resamplers (BorderArgs), and under every resampler through a calibrated lens (map mode 1)
for b in BORDERS:
    ROWS += [(req(1, FISH, 1, DEFAULT, OPTION, b), (K_BORDER, BORDER_ARGS, RS_FISHD)),                     # rotation with dist under INTER_LINEAR
             (req(1, FISH, 1, CUBIC, OPTION, b, PLANAR), (K_CUBIC, BORDER_ARGS, RS_FISHD)), (req(1, FISH, 1, LANCZOS4, OPTION, b), (K_LANCZOS4, BORDER_ARGS, RS_FISHD))]
    for mode in (0, 1, 5):
        ROWS += [(req(mode, IDEAL, 1, CUBIC, OPTION, b), (K_CUBIC, BORDER_ARGS, RS_TAG[mode])), (req(mode, IDEAL, 1, LANCZOS4, OPTION, b, PLANAR), (K_LANCZOS4, BORDER_ARGS, RS_TAG[mode]))]

# ---- vstab_warp_nv12_pinhole's ladder (the border mode is an option; map modes 3 and 4, no rotation per row) ---------------------------
for mode, tag in ((3, RECTD_RECT), (4, RECTD_FISH)):
    # all five coefficients zero: what served the ideal pinhole before -- the _rs_ex ladder without rotation and dist, copied
    ROWS += [(req(mode, RECTD0, entry=OPTION), (K_FUSED, WARP_ARGS, mode)), (req(mode, RECTD0, entry=OPTION, fmt=PLANAR), (K_PLANAR, WARP_ARGS, mode))]
    for b in BORDERS:
        if b != CONSTANT:
            ROWS += [(req(mode, RECTD0, entry=OPTION, border=b), (K_BORDER, BORDER_ARGS, mode)), (req(mode, RECTD0, entry=OPTION, border=b, fmt=PLANAR), (K_BORDER, BORDER_ARGS, mode))]
        ROWS += [(req(mode, RECTD0, 0, CUBIC, OPTION, b), (K_CUBIC, CUBIC_ARGS, mode)), (req(mode, RECTD0, 0, LANCZOS4, OPTION, b, PLANAR), (K_LANCZOS4, CUBIC_ARGS, mode))]
        # coefficients: the kernels that take a BorderArgs, the constant border included
        ROWS += [(req(mode, RECTD, 0, DEFAULT, OPTION, b), (K_BORDER, BORDER_ARGS, tag)), (req(mode, RECTD, 0, DEFAULT, OPTION, b, PLANAR), (K_BORDER, BORDER_ARGS, tag)),
                 (req(mode, RECTD, 0, CUBIC, OPTION, b), (K_CUBIC, BORDER_ARGS, tag)), (req(mode, RECTD, 0, LANCZOS4, OPTION, b, PLANAR), (K_LANCZOS4, BORDER_ARGS, tag))]

# ---- the pipeline's launch_warp, 8-bit half: the stateless entry point each branch called ---------------------------------------------
for mode in MODES:
    rs_modes = (0, 1) if mode in RS_TAG else (0,)
    for rs in rs_modes:
        tag = RS_TAG[mode] if rs else mode
        # a keep pull (vstab_warp_nv12_keep), with the frame's read-out rotation where it has one
        ROWS += [(req(mode, rs=rs, keep=1), (K_KEEP, KEEP_ARGS, tag)), (req(mode, rs=rs, fmt=PLANAR, keep=1), (K_KEEP, KEEP_ARGS, tag))]
        # a border mode without a resampler (vstab_warp_nv12_border: k_warp_border, under the constant border too where it is asked by name)
        ROWS += [(req(mode, rs=rs, entry=OWN, border=b), (K_BORDER, BORDER_ARGS, tag)) for b in BORDERS]
        # the plain handle: vstab_warp_nv12_ex, or vstab_warp_nv12_rs for a frame with a read-out rotation; all three formats
        ROWS += [(req(mode, rs=rs), (K_FUSED, WARP_ARGS, tag)), (req(mode, rs=rs, fmt=NV12), (K_FUSED, WARP_ARGS, tag)), (req(mode, rs=rs, fmt=PLANAR), (K_PLANAR, WARP_ARGS, tag))]
    # a cubic or Lanczos handle: the plain entry point, or under a border mode its _border form
    ROWS += [(req(mode, resample=CUBIC), (K_CUBIC, CUBIC_ARGS, mode)), (req(mode, resample=LANCZOS4, fmt=PLANAR), (K_LANCZOS4, CUBIC_ARGS, mode))]
    ROWS += [(req(mode, resample=CUBIC, entry=OWN, border=b, fmt=PLANAR), (K_CUBIC, CUBIC_ARGS, mode)) for b in BORDERS]
    ROWS += [(req(mode, resample=LANCZOS4, entry=OWN, border=b), (K_LANCZOS4, CUBIC_ARGS, mode)) for b in BORDERS]
# cached (vstab_warp_nv12_mapped, a calibrated handle's too: the lens is in the map written down): the CACHED kernels, under MAP_CREATEMAP_CL
ROWS += [(req(0, qmap=1), (K_FUSED, WARP_ARGS, 0)), (req(0, qmap=1, fmt=NV12), (K_FUSED, WARP_ARGS, 0)), (req(1, qmap=1), (K_FUSED, WARP_ARGS, 0))]
# vstab_warp_nv12_dist (no border mode of its own)
ROWS += [(req(1, FISH), (K_FUSED, WARP_ARGS, FISHD_RECT)), (req(2, FISH, fmt=PLANAR), (K_PLANAR, WARP_ARGS, FISHD_FISH))]
# (a calibrated handle: vstab_warp_nv12_dist_ex, rows 1; with PER_ROW and a read-out rotation vstab_warp_nv12_rs_ex, rows 4; a pinhole handle:
#  vstab_warp_nv12_pinhole's rows)

# ---- no route -------------------------------------------------------------------------------------------------------------------------
NO = (NO_ROUTE, WARP_ARGS, 0)
NO_ROWS = [
    # a rotation per row with map modes 2, 3 and 4, whatever the entry point
    req(2, rs=1), req(3, rs=1), req(4, rs=1), req(2, rs=1, entry=OWN, border=REFLECT), req(3, rs=1, resample=CUBIC, entry=OPTION), req(4, rs=1, keep=1),
    req(2, FISH, 1, CUBIC, OPTION), req(3, RECTD, 1, DEFAULT, OPTION), req(4, RECTD0, 1, DEFAULT, OPTION),
    # the quantised map: no chroma positions, one rotation, the constant border built in, INTER_LINEAR
    req(0, qmap=1, fmt=PLANAR), req(0, rs=1, qmap=1), req(0, entry=OWN, border=REPLICATE, qmap=1), req(0, resample=CUBIC, qmap=1), req(1, FISH, qmap=1),
    # a lens on a map mode it does not belong to
    req(0, FISH), req(5, FISH), req(3, FISH, entry=OPTION), req(4, FISH, resample=CUBIC, entry=OPTION), req(0, RECTD, entry=OPTION), req(1, RECTD, entry=OPTION),
    req(2, RECTD0, entry=OPTION), req(5, RECTD, resample=LANCZOS4, entry=OPTION),
    # NV12 through BGR: the bilinear entry points alone
    req(0, resample=CUBIC, fmt=NV12), req(0, resample=LANCZOS4, fmt=NV12), req(1, FISH, fmt=NV12), req(0, entry=OWN, fmt=NV12), req(0, entry=OPTION, fmt=NV12),
    req(0, keep=1, fmt=NV12), req(3, RECTD, entry=OPTION, fmt=NV12),
    # keep edges: INTER_LINEAR through an ideal lens, the constant border, the map evaluated
    req(0, resample=CUBIC, keep=1), req(0, entry=OWN, border=REFLECT_101, keep=1), req(1, FISH, keep=1), req(3, RECTD, entry=OPTION, keep=1), req(0, keep=1, qmap=1),
    # an entry point without a border mode has the constant border
    req(0, border=REPLICATE), req(0, resample=CUBIC, border=REFLECT), req(1, FISH, border=REFLECT_101),
    # unknown values
    req(-1), req(6), req(7, rs=1), req(0, resample=1), req(0, resample=3, entry=OPTION), req(0, entry=OWN, border=3), req(0, entry=OPTION, border=5), req(0, fmt=3),
    req(0, fmt=-1),
]


@pytest.fixture(scope="module")
def route(vs):
    fn = vs.lib.vstabx_warp_route
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)]

    def call(request):
        out = (ctypes.c_int * 3)(-1, -1, -1)
        assert fn(*request, out) == 0
        return tuple(out)
    return call


def test_every_route_without_a_device(route):
    assert len({r for r, _ in ROWS}) == len(ROWS)                        # no request twice
    for request, expected in ROWS:
        assert route(request) == expected, (request, route(request), expected)


def test_the_table_reaches_every_family_block_and_tag():
    routes = {r for _, r in ROWS}
    assert {f for f, _, _ in routes} == {K_FUSED, K_PLANAR, K_BORDER, K_CUBIC, K_LANCZOS4, K_KEEP}
    assert {(f, b) for f, b, _ in routes} == {(K_FUSED, WARP_ARGS), (K_PLANAR, WARP_ARGS), (K_BORDER, BORDER_ARGS), (K_CUBIC, CUBIC_ARGS), (K_CUBIC, BORDER_ARGS),
                                              (K_LANCZOS4, CUBIC_ARGS), (K_LANCZOS4, BORDER_ARGS), (K_KEEP, KEEP_ARGS)}
    assert {t for _, _, t in routes} == set(range(14))
    # the argument block follows from the tag under a resampler: one rotation through an ideal or a fisheye lens is CubicArgs, the rest BorderArgs
    for f, b, t in routes:
        if f in (K_CUBIC, K_LANCZOS4):
            assert (b == CUBIC_ARGS) == (t <= 5 or t in (FISHD_RECT, FISHD_FISH)), (f, b, t)


def test_what_has_no_route(route):
    assert len(set(NO_ROWS)) == len(NO_ROWS) and not set(NO_ROWS) & {r for r, _ in ROWS}
    for request in NO_ROWS:
        assert route(request) == NO, (request, route(request))


def test_the_hook_refuses_a_null_output(vs, route):
    assert vs.lib.vstabx_warp_route(0, 0, 0, 0, 0, 0, 0, 0, 0, None) == vs.ERR_INVALID
    assert vs.lib.vstab_last_error() == b"vstabx_warp_route: bad argument"
