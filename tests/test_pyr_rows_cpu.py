"""The model of k_pyr_down's interior body (tests/pyr_rows.py) checked without a device: edge and interior work together produce every
(group, row) exactly once, no interior thread reads a row outside the image, the taps of every stored output are the reflection the
definition asks for, the case table reaches every named path and each case the paths it names, and the model's R is the source's."""
import collections
import os
import re

import numpy as np
import pytest

import pyr_paths as pp
import pyr_rows as pr


def _check(sw, sh, wide, tag, groups):
    dw, dh = (sw + 1) // 2, (sh + 1) // 2
    G = pr.rows_grid(sw, dw, dh, wide)
    eg, ey, ig, irg = pr.decode(G, dh)
    assert ((ig >= 1) & (8 * ig + 12 <= sw) & (4 * ig + 4 <= dw)).all(), tag
    if not wide:
        assert ig.size == 0 and G.nb_int == 0, tag
    # every (group, row) once: the edge threads' own, and the rows each interior thread stores
    count = np.zeros((dh, G.n_groups), np.int32)
    np.add.at(count, (ey, eg), 1)
    for rg in np.unique(irg).tolist():
        rows = groups[rg].stored
        assert rows and rows[0] == pr.R * rg, tag
        count[np.ix_(rows, ig[irg == rg])] += 1
    assert (count == 1).all(), (tag, np.argwhere(count != 1)[:4].tolist())
    # the grid is as small as the decode allows, and every group that could be interior is
    assert G.nb_edge == pp.div_up(eg.size, 256) and G.nb_int == G.nbx * pp.div_up(dh, 4 * pr.R), tag
    if wide:
        could = sum(1 for k in range(1, G.n_groups) if 8 * k + 12 <= sw and 4 * k + 4 <= dw)
        assert ig.size == could * pp.div_up(dh, pr.R), tag
        assert pr.trailing_edge_groups(sw) in (1, 2) or could == 0, tag


def test_edge_and_interior_work_produce_every_group_and_row_once_and_read_inside_the_image():
    """sw 1..600 x sh 1..40, planes aligned or not: `wide` is what launch_pyr_down derives (vec_ok && sw >= 16 && sh >= 4) -- it is never
    set for an image that is not `near`, whose taps one reflection does not bring back."""
    for sh in range(1, 41):
        dh = (sh + 1) // 2
        groups = [pr.row_group(rg, sh) for rg in range(pp.div_up(dh, pr.R))]
        if sh >= 4:
            for G in groups:
                assert all(0 <= i < sh for i in G.read), (sh, G)                      # dropped rows included
                for i, f, u in zip(G.ry, G.read, G.used):
                    if u:                                                             # a tap of a stored output: the definition's fold, one reflection
                        assert f == pp.fold101(i, sh) and pp.folds(i, sh) <= 1, (sh, G.y0, i, f)
                assert all(i < 0 or i >= sh for i in G.reflected), (sh, G)
            assert sorted(y for G in groups for y in G.stored) == list(range(dh)), sh
        for sw in range(1, 601):
            for aligned in (False, True):
                _check(sw, sh, aligned and sw >= 16 and sh >= 4, (sw, sh, aligned), groups)


def test_the_cases_reach_every_path_and_each_the_paths_it_names():
    cases = pr.ROWS_CASES
    assert len({c.id for c in cases}) == len(cases), "two cases are the same call"
    reached = collections.defaultdict(list)
    for c in cases:
        got = pr.rows_paths(c)
        assert set(got) <= pr.ROWS_PATHS, (c.id, sorted(got))
        assert c.what and set(c.what) <= set(got), (c.id, "names", c.what, "reaches", sorted(got))
        assert ("rows_none" in got) == (len(got) == 1 and got["rows_none"] == 1), c.id
        if "rows_none" in got and (c.sw >= 20 and c.sh >= 4):
            assert pp.down_paths(c.sw, c.sh, c.src, c.dst).get("edge_all_bytes", 0) > 0, (c.id, "the byte path")
        for n in got:
            reached[n].append(c.id)
        print(f"  {c.id:34s} {' '.join(f'{n}={v}' for n, v in sorted(got.items()))}")
    for n in sorted(pr.ROWS_PATHS):
        print(f"  {n:20s} {len(reached[n]):3d}  {' '.join(reached[n][:6])}{' ...' if len(reached[n]) > 6 else ''}")
    assert set(reached) == set(pr.ROWS_PATHS), ("never reached", sorted(pr.ROWS_PATHS - set(reached)))


def test_the_shapes_the_case_table_leans_on():
    R = pr.R
    # 20 x 4 is the first image with an interior thread; every residue of dh mod R over the heights 2 R k + 1 .. 2 R k + 2 R, k = 0, 1
    assert pr.rows_paths(pr._case(19, 4)) == {"rows_none": 1} and "rows_top" in pr.rows_paths(pr._case(20, 4))
    heights = [c.sh for c in pr.ROWS_CASES if c.sw == 20 and c.src == (0, 20)]
    assert set(range(1, 4 * R + 1)) <= set(heights)
    assert {((sh + 1) // 2) % R for sh in heights if 4 <= sh <= 2 * R} == set(range(R)) - {1} | {0}     # (dh = 1 is sh <= 2: not near)
    assert {((sh + 1) // 2) % R for sh in heights if 2 * R < sh <= 4 * R} == set(range(R))
    # one, two and three row groups; the middle one of three is the first fast one (source rows 2 R - 2 .. 4 R)
    for sh, n, fast in ((2 * R, 1, False), (2 * R + 1, 2, False), (4 * R, 2, False), (4 * R + 1, 3, True), (4 * R + 2, 3, True)):
        got = pr.rows_paths(pr._case(20, sh))
        assert pp.div_up((sh + 1) // 2, R) == n and ("rows_fast" in got) == fast, (sh, got)
    # 64 and 65 interior groups a row; one and two edge groups behind the last interior one, never three
    assert pp.pyr_grid(524, 262, 1, True).g_hi - 1 == 64 and pp.pyr_grid(532, 266, 1, True).nbx == 2
    assert (pr.trailing_edge_groups(44), pr.trailing_edge_groups(49)) == (1, 2)
    assert {pr.trailing_edge_groups(sw) for sw in range(20, 2000)} == {1, 2}
    # the largest 16-bit half of the vertical pass: 255 * 256 + 128, below 2^16; the sum of three horizontal sums below it too
    assert 255 * 16 * 16 + 128 == 65408 < 1 << 16 and 3 * 255 * 16 < 1 << 16


def test_the_models_r_is_the_sources():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "video-annotator_amd", "csrc", "vstab_pyramid.hip")).read()
    assert re.search(r"#define VSTAB_PYR_ROWS (\d+)\n", src).group(1) == str(pr.R)
    assert "pyr_down_dispatch<false, PYR_ROWS>" in src and "pyr_grid(sw, dw, dh, vec_ok && near, PYR_ROWS)" in src
    assert "div_up(dh, 4 * rows)" in src


@pytest.mark.parametrize("mutant", ("bottom", "round"))
def test_the_model_names_cases_a_broken_build_must_fail_and_cases_it_must_pass(mutant):
    bad = [c.id for c in pr.ROWS_CASES if pr.failing(c, mutant)]
    assert 0 < len(bad) < len(pr.ROWS_CASES), (mutant, len(bad))
