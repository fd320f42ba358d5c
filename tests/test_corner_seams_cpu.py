"""CPU half of the tests of k_corners_fused's ownership seams (tests/corner_seams.py): the frames put the image border on every position
of the kernel's three ownerships, and hold tiles of the interior path and of the border path in one launch.  No GPU here."""
import numpy as np

import corner_seams as S


def test_sizes_cover_the_remainders_and_stay_small():
    sizes = S.sizes()
    assert len(set(sizes)) == len(sizes) == len(S.W_REM) * len(S.H_REM) + len(S.TINY) + 1      # 67 x 33 counts once
    assert {(w % S.TW, h % S.TH) for w, h in sizes} >= {(a, b) for a in S.W_REM for b in S.H_REM}
    assert all(3 <= w <= 640 and 3 <= h <= 360 for w, h in sizes)
    assert set(S.TINY) <= set(sizes) and S.BIG in sizes and S.RINGED in sizes
    assert all(S.tiles(w, h) in ((1, 1), (2, 2)) for w, h in S.TINY) and S.tiles(67, 33) == (2, 2)


def test_borders_fall_on_every_ownership_position():
    """the last column (row) of the image in its prod group of 4 (5), its box group of 3, its lane (its row of the wave's 8); the first
    column and row always sit at prod position 2 and box position 1 (the regions start 2 and 1 pixels before the tile)"""
    cols, rows = zip(*(S.border_positions(w, h) for w, h in S.sizes()))
    assert {c[0] for c in cols} == set(range(S.PROD_W)) and {c[1] for c in cols} == set(range(S.BOX))
    assert {r[0] for r in rows} == set(range(S.PROD_H)) and {r[1] for r in rows} == set(range(S.BOX))
    assert {0, 1, 2, 3, 4, 62} <= {c[2] for c in cols}                      # lanes at both ends of the wave
    assert {r[2] for r in rows} >= {0, 1, 2, 3, 5}                           # (row 29 of a tile is row 5 of the last wave's 7)
    assert S.border_positions(321, 125) == ((2, 1, 0), (2, 1, 0))
    assert S.border_positions(67, 33) == ((0, 0, 2), (3, 2, 1))


def test_which_tiles_take_the_interior_path():
    """a tile is interior when its 72 x 38 source bytes from (ox - 4, oy - 3) lie inside the image: never in the first tile column or row,
    and only with 68 columns and 35 rows of image from the tile's origin on"""
    m = S.interior_map(*S.BIG)
    assert m.shape == (5, 6)
    assert m.astype(int).tolist() == [[0] * 6, [0, 1, 1, 1, 0, 0], [0, 1, 1, 1, 0, 0], [0] * 6, [0] * 6]
    assert not S.interior_map(*S.BIG, aligned=False).any()                     # an unaligned view: every tile takes the border path
    # the exact edges of the test: 68 columns from ox = 64, 35 rows from oy = 31
    assert S.interior(1, 1, 132, 66) and not S.interior(1, 1, 131, 66) and not S.interior(1, 1, 132, 65)
    assert not S.interior(0, 1, 640, 360) and not S.interior(1, 0, 640, 360) and S.interior(1, 1, 640, 360)
    assert S.interior_map(640, 360).sum() == 8 * 10 and S.interior_map(640, 360).shape == (12, 10)
    # frames with tiles of both paths in one launch, and frames without an interior tile
    both = [(w, h) for w, h in S.sizes() if S.interior_map(w, h).any()]
    assert all(not S.interior_map(w, h).all() for w, h in both)
    assert len(both) >= 5 and S.BIG in both and {S.interior_map(w, h).sum() for w, h in both} >= {1, 2, 3, 4, 6}
    assert not any(S.interior_map(w, h).any() for w, h in S.TINY)
    # an interior tile next to the right border's tile and above the bottom border's tile, so a seam between the two paths runs both ways
    assert S.tiles(*S.RINGED) == (3, 3)
    assert S.interior_map(*S.RINGED).astype(int).tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]


def test_frames_are_seeded_and_hold_what_they_claim():
    for kind in ("noise", "rects"):
        a, b = S.frame(kind, 133, 67), S.frame.__wrapped__(kind, 133, 67)
        assert a.shape == (67, 133) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert len(np.unique(S.frame("noise", 321, 125))) == 256
    r = S.frame("rects", 321, 125)
    assert {30, 200, 225} <= set(np.unique(r).tolist()) and ((r >= 124) & (r < 132)).mean() > 0.3
    # noise: over a hundred survivors in every whole tile, under the slots; rectangles leave a few survivors per tile
    n, k = S.model("noise", *S.BIG), S.model("rects", *S.BIG)
    assert 100 < n.hi[:4, :5].min() and n.hi.max() <= 256 and k.lo.max() < 100 and k.n > 0
    print("noise 321 x 125: survivors per tile", n.lo.ravel().tolist(), "spilled", n.spilled_range())
