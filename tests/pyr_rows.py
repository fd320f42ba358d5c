"""The interior body of k_pyr_down (csrc/vstab_pyramid.hip: pyr_down_rows, PYR_ROWS) restated for the tests, on top of pyr_paths: a thread of
an interior workgroup owns the group of 4 outputs g in the R = PYR_ROWS rows of ONE row group, loads 2R + 3 source rows once each and sums
each horizontally once.  The edge workgroups, k_pack_pyr and k_pyr_down_x2 are pyr_paths' own and unchanged.  No GPU here.

THE GRID.  rows_grid = pyr_paths.pyr_grid with nb_int = nbx x div_up(dh, 4 R): an interior workgroup is 64 groups x 4 row groups (a wave is
64 groups of one row group).  decode: every (block, thread) as pyr_down_dispatch<false, R> does -> the (g, y) of the live edge threads and
the (g, row group) of the live interior threads.

A ROW GROUP.  row_group(rg, sh): output rows y0 = R rg .. y0 + R - 1, of which those < dh are stored; source row j of 2R + 3 is
ry = 2 y0 - 2 + j, read at max(min(|ry|, 2 sh - 2 - |ry|), 0) -- one reflection, then the clamp for rows that only dropped outputs tap.

THE PATHS, per live interior thread (ROWS_PATHS):
    rows_fast            all R rows stored and all 2R + 3 source rows inside the image: no row index changes
    rows_top             the row group of output row 0 (source rows -2, -1 reflected)
    rows_bottom_odd      the row group of the last output row, sh odd (source rows sh, sh + 1 reflected)
    rows_bottom_even     the same, sh even (source row sh reflected)
    rows_partial_group   dh % R != 0: the last row group stores fewer than R rows; the rows it drops read clamped indices
    rows_many_y          (per launch) div_up(dh, 4 R) >= 2: more than one workgroup of row groups
    rows_none            (per launch) no interior workgroup: unaligned planes, sw < 20 or sh < 4 -- the edge paths of pyr_paths alone

THE CASES.  ROWS_CASES: pyr_paths.Call("down", ...) with `what` from ROWS_PATHS; test_pyr_rows_cpu.py asserts that each reaches what it
names and that the table reaches every name."""
import collections

import numpy as np

import pyr_paths as pp

R = 4                                     # PYR_ROWS of csrc/vstab_pyramid.hip (test_pyr_rows_cpu.py reads it from the source)
NS = 2 * R + 3

ROWS_PATHS = frozenset("rows_fast rows_top rows_bottom_odd rows_bottom_even rows_partial_group rows_many_y rows_none".split())


def rows_grid(sw, dw, dh, wide):
    G = pp.pyr_grid(sw, dw, dh, wide)
    return G._replace(nb_int=G.nbx * pp.div_up(dh, 4 * R))


def decode(G, dh):
    """-> (g, y) of the live edge threads (pyr_paths' decode: unchanged) and (g, row group) of the live interior threads."""
    eg, ey, _, _ = pp.decode_grid(G._replace(nb_int=0), dh)
    b = np.arange(G.nb_int)
    by = b // max(G.nbx, 1)
    bx = b - by * G.nbx
    t = np.arange(256)
    g = (G.g_lo + bx[:, None] * 64 + (t & 63)[None, :]).ravel()
    rg = (by[:, None] * 4 + (t >> 6)[None, :]).ravel()
    live = (g < G.g_hi) & (R * rg < dh)
    return eg, ey, g[live], rg[live]


RowGroup = collections.namedtuple("RowGroup", "y0 stored ry read used reflected")


def row_group(rg, sh):
    """stored: the output rows written.  ry / read: the 2R + 3 source row indices before and after folding and clamping.  used: which of them
    a stored output taps.  reflected: the used ones whose index changed."""
    dh = (sh + 1) // 2
    y0 = R * rg
    stored = [y for y in range(y0, y0 + R) if y < dh]
    ry = [2 * y0 - 2 + j for j in range(NS)]
    read = [max(min(abs(i), 2 * sh - 2 - abs(i)), 0) for i in ry]
    used = [any(2 * (y - y0) <= j <= 2 * (y - y0) + 4 for y in stored) for j in range(NS)]
    return RowGroup(y0, stored, ry, read, used, [i for i, f, u in zip(ry, read, used) if u and i != f])


def group_paths(rg, sh):
    """The names a thread of row group rg takes."""
    dh = (sh + 1) // 2
    G = row_group(rg, sh)
    names = set()
    if len(G.stored) == R and all(0 <= i < sh for i in G.ry):
        names.add("rows_fast")
    if G.y0 == 0:
        names.add("rows_top")
    if dh - 1 in G.stored:
        names.add("rows_bottom_odd" if sh % 2 else "rows_bottom_even")
    if len(G.stored) < R:
        names.add("rows_partial_group")
    return names


def rows_host(c):
    H = pp.down_host(c.sw, c.sh, c.src, c.dst)
    H["grid"] = rows_grid(c.sw, H["dw"], H["dh"], H["vec_ok"] and H["near"])
    return H


def rows_paths(c):
    """-> Counter: path name -> interior threads that take it (1 for the names of the whole launch)."""
    H = rows_host(c)
    G, dh = H["grid"], H["dh"]
    P = collections.Counter()
    _, _, ig, irg = decode(G, dh)
    for rg, n in zip(*np.unique(irg, return_counts=True)):
        for name in group_paths(int(rg), c.sh):
            P[name] += int(n)
    if ig.size == 0:
        P["rows_none"] = 1
    elif pp.div_up(dh, 4 * R) >= 2:
        P["rows_many_y"] = 1
    return +P


def failing(c, mutant):
    """Whether case c must fail on a build with `mutant`: "bottom" -- the reflection of source rows >= sh broken (any stored output of an
    interior thread taps one); "round" -- the + 128 of the vertical pass dropped (any interior thread at all: on content where some sum's
    low byte is >= 128, which every plane of tests' content has)."""
    H = rows_host(c)
    _, _, ig, irg = decode(H["grid"], H["dh"])
    if mutant == "round":
        return ig.size > 0
    assert mutant == "bottom"
    return any(i >= c.sh for rg in np.unique(irg) for i in row_group(int(rg), c.sh).reflected)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _case(sw, sh, src=None, dst=None, what=()):
    dw = (sw + 1) // 2
    return pp.Call("down", sw, sh, src or (0, pp.al(sw, 4)), dst or (0, pp.al(dw, 4)), what=tuple(what))


def trailing_edge_groups(sw):
    """Edge groups behind the last interior group of a row of an aligned image."""
    dw = (sw + 1) // 2
    G = pp.pyr_grid(sw, dw, 1, True)
    return G.n_groups - G.g_hi


def _cases():
    cases = []
    # the smallest interior images: 20 wide (one interior group, g = 1), heights 2 R k + 1 .. 2 R k + 2 R for k = 0, 1 -- every residue of
    # dh mod R with an odd and an even bottom, one row group (top and bottom at once) and two.  sh < 4 is not `near`: no interior workgroup.
    for sh in range(1, 4 * R + 1):
        dh = (sh + 1) // 2
        if sh < 4:
            what = ("rows_none",)
        else:
            what = ("rows_top", "rows_bottom_odd" if sh % 2 else "rows_bottom_even") + (("rows_partial_group",) if dh % R else ())
        cases.append(_case(20, sh, what=what))
    # three row groups, from sh = 4 R + 1 on: the middle one is the first rows_fast (its source rows 2 R - 2 .. 4 R); up to 6 R
    for sh in range(4 * R + 1, 6 * R + 1):
        dh = (sh + 1) // 2
        what = ("rows_top", "rows_fast", "rows_bottom_odd" if sh % 2 else "rows_bottom_even") + (("rows_partial_group",) if dh % R else ())
        cases.append(_case(20, sh, what=what))
    # widths: 64 interior groups (one workgroup a row group, full) and 65 (two); then one, two trailing edge groups behind the last interior
    # group (44: dw = 22, a partial last group; 49 with a pitch of 52) -- three cannot happen: ceil(sw / 8) - ((sw - 12) / 8 + 1) <= 2
    cases.append(_case(524, 4 * R + 3, what=("rows_fast", "rows_bottom_odd")))
    cases.append(_case(532, 4 * R + 3, what=("rows_fast", "rows_bottom_odd")))
    cases.append(_case(532, 5, what=("rows_top", "rows_bottom_odd", "rows_partial_group")))
    cases.append(_case(44, 4 * R + 4, what=("rows_fast", "rows_bottom_even")))
    cases.append(_case(49, 4 * R + 4, what=("rows_fast", "rows_bottom_even")))
    cases.append(_case(48, 2 * R + 1, what=("rows_partial_group",)))
    # alignment: the source or the destination 1 .. 3 bytes past alignment, or an odd pitch: the byte path, no interior workgroup
    for off in (1, 2, 3):
        cases.append(_case(44, 4 * R + 3, src=(off, 44), what=("rows_none",)))
        cases.append(_case(44, 4 * R + 3, dst=(off, 24), what=("rows_none",)))
    cases.append(_case(44, 4 * R + 3, src=(0, 47), what=("rows_none",)))
    cases.append(_case(44, 4 * R + 3, dst=(0, 25), what=("rows_none",)))
    # pitches wider than the rows on both planes, bases a multiple of 4 that is no multiple of 16
    cases.append(_case(44, 4 * R + 3, src=(8, 60), dst=(4, 28), what=("rows_fast", "rows_top", "rows_bottom_odd", "rows_partial_group")))
    cases.append(_case(72, 6 * R, src=(0, 128), dst=(0, 64), what=("rows_fast", "rows_bottom_even")))
    # tall: many workgroups of row groups (24 x 260: dh = 130 = 8 x 16 + 2), and a height one workgroup of row groups holds exactly
    cases.append(_case(24, 260, what=("rows_many_y", "rows_fast", "rows_partial_group")))
    cases.append(_case(24, 8 * R * 4 + 1, what=("rows_many_y", "rows_bottom_odd")))
    cases.append(_case(24, 8 * R * 4, what=("rows_fast", "rows_bottom_even")))
    return cases


ROWS_CASES = _cases()
