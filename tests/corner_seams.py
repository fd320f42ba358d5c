"""Frames for the ownership seams inside a tile of k_corners_fused (csrc/vstab_corners_fused.hip), and the kernel's ownership restated.  No GPU here.

Inside a 64 x 31 tile at (ox, oy) the kernel hands out work three ways:

    prod   derivative products on 68 x 35 pixels from image (ox - 2, oy - 2): a thread owns 4 columns x 5 rows;
    box    eigenvalues on 66 x 33 pixels from image (ox - 1, oy - 1): a thread owns 3 x 3;
    nms    the 64 x 31 outputs: a lane owns a column, a wave 8 rows.

A tile whose 72 x 38 source bytes from image (ox - 4, oy - 3) lie inside an image of dword-aligned rows takes a path of its own (no
reflection, no sign flips, no image-bounds tests).  The frames below put the image's right and bottom border, and with them the mirrored
pixels behind it, on every position of the three ownerships, and hold tiles of both paths in one launch."""
import functools

import numpy as np

import corner_tiles as C

TW, TH = C.TW, C.TH
PROD_W, PROD_H, BOX = 4, 5, 3          # prod: columns x rows per thread; box: 3 x 3
NMS_ROWS = 8
SRC_W, SRC_H, SRC_X0, SRC_Y0 = 72, 38, -4, -3

W_REM, H_REM = (1, 2, 3, 4, 5, 63), (1, 2, 3, 4, 30)     # w mod 64, h mod 31 (4 is added to the heights: the fifth row of a prod thread)
TINY = ((3, 3), (4, 5), (16, 4), (67, 33))
BIG = (321, 125)
RINGED = (133, 67)                       # 3 x 3 tiles: one interior tile ringed by eight border tiles


def sizes():
    """(w, h): every remainder of the width with every remainder of the height, one to four tiles wide and one to three high (the
    larger ones hold tiles of the interior path); the frames smaller than a tile; 321 x 125; 133 x 67"""
    out = []
    for i, rw in enumerate(W_REM):
        for j, rh in enumerate(H_REM):
            kx, ky = 1 + (i + 2 * j) % 4, 1 + (i + j) % 3
            out.append((TW * kx + rw if rw != 63 else TW * (kx - 1) + rw, TH * ky + rh if rh != 30 else TH * (ky - 1) + rh))
    return list(dict.fromkeys(out + list(TINY) + [BIG, RINGED]))      # (67 x 33 is both a remainder pair and a tiny frame)


def tiles(w, h):
    return -(-w // TW), -(-h // TH)


def interior(tx, ty, w, h, aligned=True):
    """the kernel's test (tile_interior over SourceTile3) RESTATED: the source bytes of tile (tx, ty) lie inside the image, and the rows are dword aligned.
    Nothing here reads the kernel's choice, and both paths give the same bits, so a kernel that takes the border path more often than this
    says passes every test; a tile that wrongly takes the interior path reads outside the image or skips a sign flip, and that the GPU
    comparisons of test_corner_seams_gpu.py catch (eigenvalues and keys of the tiles next to every border)."""
    ox, oy = tx * TW, ty * TH
    return bool(aligned and ox + SRC_X0 >= 0 and ox + SRC_X0 + SRC_W <= w and oy + SRC_Y0 >= 0 and oy + SRC_Y0 + SRC_H <= h)


def interior_map(w, h, aligned=True):
    nx, ny = tiles(w, h)
    return np.array([[interior(tx, ty, w, h, aligned) for tx in range(nx)] for ty in range(ny)], bool).reshape(ny, nx)


def border_positions(w, h):
    """where the image's last column and row fall in the last tile column's / row's ownerships:
    (prod column in its group of 4, box column in its group of 3, lane), (prod row in its group of 5, box row in its group of 3, row in the wave)"""
    nx, ny = tiles(w, h)
    lx, ly = w - 1 - (nx - 1) * TW, h - 1 - (ny - 1) * TH
    return ((lx + 2) % PROD_W, (lx + 1) % BOX, lx), ((ly + 2) % PROD_H, (ly + 1) % BOX, ly % NMS_ROWS)


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    """`noise`: every byte value, seeded by the size (a tile holds around 130 survivors); `rects`: noise of eight
    levels under bright and dark rectangles, whose corners set the threshold (few survivors per tile)"""
    rng = np.random.default_rng(1000 * w + h)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    img = rng.integers(124, 132, (h, w), dtype=np.uint8)
    for _ in range(max(2, w * h // 1500)):
        rw, rh = int(rng.integers(2, max(3, min(w, 40)))), int(rng.integers(2, max(3, min(h, 24))))
        x, y = int(rng.integers(0, max(1, w - rw + 1))), int(rng.integers(0, max(1, h - rh + 1)))
        img[y:y + rh, x:x + rw] = rng.choice([225, 30, 200])
    return img


@functools.lru_cache(maxsize=None)
def model(kind, w, h):
    """the tile model of a frame, computed once per process and shared"""
    return C.Model(frame(kind, w, h))
