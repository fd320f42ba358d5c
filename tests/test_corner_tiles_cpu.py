"""CPU half of the corner detector's path tests (tests/corner_tiles.py): every set reaches the tile states, k_filter_keys workgroups, seams
and key-buffer fills it is named for -- exact counts throughout -- and the hooks refuse bad arguments without a device."""
import ctypes
import importlib

import numpy as np
import pytest

import corner_tiles as C
import oracle


PLATEAU_CELL = 1239      # survivors of the plateau cell "P", wherever it lies


def test_model_agrees_with_the_oracle_detector():
    """The model's candidates are the oracle's: with no minimum distance and no limit, goodFeaturesToTrack returns every candidate, value
    descending and ties by later raster position -- the model's keys, descending."""
    for name in ("tile_257", "grid_5x3", "timing", "ramp_4", "cut_129x63", "stripes_diagonal"):
        m = C.model(name)
        xy = oracle.good_features(m.img, 0, m.quality, 0.0)
        idx = (m.keys[::-1] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.array_equal(xy, np.stack([idx % m.w, idx // m.w], 1).astype(np.float32)), name


@pytest.mark.parametrize("n,state", [(255, "keys"), (256, "full"), (257, "spills"), (258, "spills")])
def test_single_tiles_around_the_slot_count(n, state):
    for name in (f"tile_{n}", f"inset_{n}"):
        m = C.model(name)
        assert (m.w, m.h, m.n_tiles) == (C.TW, C.TH, 1)
        assert m.n == n and m.lo[0, 0] == n and m.hi[0, 0] == n and m.state(0) == state, name
        assert m.spilled_range() == ((1, 1) if n > C.SLOTS else (0, 0))
    # the numbered cells count the same wherever they lie in a frame
    m = C.Model(C.cells_frame([[0, n, 0], [n, 0, n], [0, n, n]]))
    assert m.lo.tolist() == m.hi.tolist() == [[0, n, 0], [n, 0, n], [0, n, n]]


def test_sixteen_full_tiles_fill_kept_exactly():
    m = C.model("full_16")
    wg = m.workgroups()
    assert m.n_tiles == 16 and len(wg) == 1 and int(m.full.sum()) == 16 and m.spilled_range() == (0, 0)
    assert wg[0]["kept"] == (C.FK_TILES * C.SLOTS,) * 2 == (4096, 4096) and m.n == 4096


def test_tile_mixes():
    m = C.model("mixed_wave")
    assert [m.state(t) for t in range(8)] == ["keys", "spills", "spills", "keys", "keys", "keys", "full", "keys"]
    assert m.lo.ravel().tolist() == [255, 257, PLATEAU_CELL, 255, 255, 255, 256, 255]
    assert m.workgroups()[0]["mixed_waves"] == [0] and not m.timing.any()
    m = C.model("spill_last")
    assert m.n_tiles == 6 and [m.state(t) for t in range(6)] == ["keys"] * 5 + ["spills"] and m.workgroups()[0]["mixed_waves"] == [1]
    counts = [C.model(f"grid_{tx}x{ty}").n_tiles for tx, ty in C.GRIDS]
    assert counts == [1, 2, 3, 15, 16, 17, 18, 35, 35]
    assert {c % 4 for c in counts} == {0, 1, 2, 3} and {1, 15, 16, 17} <= set(counts)
    for tx, ty in C.GRIDS:
        m = C.model(f"grid_{tx}x{ty}")
        assert (m.w, m.h) == (tx * C.TW, ty * C.TH) and not m.timing.any()
        # every tile holds what its cell says (P: a plateau)
        for y in range(ty):
            for x in range(tx):
                c = C.GRID_CELLS[(x * 5 + y * 3) % 6]
                assert m.lo[y, x] == (PLATEAU_CELL if c == "P" else c), (tx, ty, x, y)
    # a workgroup whose 16 tiles wrap over tile rows, with spilled and keyed tiles in one wave
    for tx, ty, rows, mixed in ((3, 6, [0, 1, 2, 3, 4, 5], [[0, 1, 2, 3], [0]]), (5, 3, [0, 1, 2], [[0, 1, 2]]),
                                (5, 7, [0, 1, 2, 3], [[0, 1, 2], [0, 1, 2, 3], []]), (7, 5, [0, 1, 2], [[0, 1, 2, 3], [0, 1, 2, 3], [0]])):
        wg = C.model(f"grid_{tx}x{ty}").workgroups()
        assert wg[0]["rows"] == rows and [g["mixed_waves"] for g in wg] == mixed
    assert [len(w["tiles"]) for w in C.model("grid_7x5").workgroups()] == [16, 16, 3]
    assert [len(w["tiles"]) for w in C.model("grid_17x1").workgroups()] == [16, 1]


def test_plateau_tiles_cut_by_the_image_edges():
    assert {w % C.TW for w, _ in C.CUTS} == {1, 2, 63} and {h % C.TH for _, h in C.CUTS} == {1, 2, 30}
    spilled = {}
    for w, h in C.CUTS:
        m = C.model(f"cut_{w}x{h}")
        assert m.n == (w - 4) * (h - 4) and not m.timing.any()
        spilled[(w, h)] = m.spilled_range()[0]
        # the last tile column / row: w mod 64 (h mod 31) columns (rows) of which the image's last is no candidate, its last but one
        # lies on the plateau's rim
        cols, rows = w % C.TW, h % C.TH
        assert (m.lo[:, -1] > 0).all() == (cols > 2) and (m.lo[-1, :] > 0).all() == (rows > 2)
        assert m.state(0) == "spills"
    assert spilled == {(65, 32): 1, (66, 33): 1, (127, 61): 4, (129, 63): 4, (191, 92): 9, (194, 95): 9}
    # the cut tiles that spill: 63 columns or 30 rows of plateau
    assert C.model("cut_127x61").lo.tolist() == [[1798, 1769], [1736, 1708]]


def test_timing_frame_has_tiles_that_spill_or_not():
    m = C.model("timing")
    assert int(m.timing.sum()) == 7 and m.spilled_range() == (0, 7)
    assert m.timing.tolist() == [[False] * 5, [False] * 5, [True, False, False, True, False], [True, True, True, True, True]]
    # two of them keep keys under the final threshold too
    assert m.lo[2:].tolist() == [[0, 0, 0, 0, 0], [0, 4, 0, 4, 0]] and m.n == 89
    assert (m.hi[m.timing] > 400).all()


def test_ramps_reach_negative_eigenvalues_and_one_negative_tile_maximum():
    neg = {}
    for k in range(len(C.RAMPS)):
        m = C.model(f"ramp_{k}")
        neg[k] = (int((m.eig[2:-2, 2:-2] < 0).sum()), int(m.negative_max.sum()))
    assert neg == {0: (0, 0), 1: (0, 0), 2: (159, 0), 3: (483, 0), 4: (9358, 1), 5: (0, 0), 6: (0, 0)}
    # the search found one: the middle tile of 0.5 x + 0.25 y + 10 at 150 x 70 has a negative maximum, so its lower bound is -inf and all
    # 1984 pixels of its plateau survive unless another tile has published a maximum by then; none passes the final threshold
    m = C.model("ramp_4")
    assert m.negative_max.tolist() == [[False] * 3, [False, True, False], [False] * 3]
    assert (m.lo[1, 1], m.hi[1, 1]) == (0, C.TW * C.TH) and m.state(4) == "timing" and m.frame_max > 0
    assert np.unique(m.eig[C.TH - 1:2 * C.TH + 1, C.TW - 1:2 * C.TW + 1]).tolist() == [float(np.float32(-2.0 ** -40))]   # -9.09e-13, one plateau
    # the pure ramps along one axis are exactly zero everywhere: a frame maximum of 0, threshold 0, no candidate
    for k in (0, 1):
        m = C.model(f"ramp_{k}")
        assert m.frame_max == 0 and m.n == 0 and not m.eig.any()
    # plateaus of rounding noise fill tiles past their slots
    assert C.model("ramp_5").spilled_range() == (1, 1) and C.model("ramp_6").spilled_range() == (4, 4)


def test_stripes():
    assert C.model("stripes_vertical").n == 0 and C.model("stripes_horizontal").n == 0
    m = C.model("stripes_diagonal")
    assert m.n == 282 and m.spilled_range() == (0, 2)


def test_frames_at_the_key_capacity():
    assert C.Model(C.checker(570, 464)).n == 260360
    for which, n in (("2^18", 1 << 18), ("2^18+1", (1 << 18) + 1)):
        g = C.cap_frame(which)
        assert g.shape == (468, 570) and C.Model(g).n == n, which
    assert int((C.cap_frame("2^18") != C.cap_frame("2^18+1")).sum()) == 23     # one frame but for 23 pixels at the rim of the flat patch
    assert C.KEY_CAP == 1 << 18 and C.SPEC_CAP == 1 << 15


def test_pipeline_clips_lie_where_they_claim():
    """Candidates per frame against SPEC_CAP and the key capacity, and corners against the 150 below which a handle makes every frame a key
    frame (no planned key frame, no speculative detection): the 320 x 180 checkerboard is such a clip."""
    for which, size, n, corners in (("under_spec_cap", (640, 360), 21010, 200), ("middle_320", (320, 180), 55616, 78), ("middle", (480, 270), 126616, 171),
                                    ("at_spec_cap", (640, 360), 1 << 15, 200), ("over_spec_cap", (640, 360), (1 << 15) + 1, 200)):
        got_size, frames = C.pipeline_clip(which)
        # (odd frames: the checkerboard moved by a pixel; the detected frames -- 0 and 20, or all of middle_320's -- are counted here)
        assert got_size == size and len(frames) == 25 and all(np.array_equal(f, frames[k % 2]) for k, f in enumerate(frames))
        assert not np.array_equal(frames[0], frames[1])
        g = np.ascontiguousarray(frames[0][:size[1]])
        assert C.Model(g).n == n and len(oracle.good_features(g)) == corners, which
    # the odd frames (phase 1): the checkerboards count the same, the banded frames do not -- "at" is over SPEC_CAP there, so the SPEC_CAP
    # cases of the GPU test hold because the planned key frame's detection reads frame 20; a change of that parity shows here first
    for which, n in (("middle_320", 55616), ("middle", 126616), ("under_spec_cap", 27984), ("at_spec_cap", 40048), ("over_spec_cap", 40050)):
        (w, h), frames = C.pipeline_clip(which)
        assert C.Model(frames[1][:h]).n == n, which
        assert np.array_equal(frames[20], frames[0])
    (w, h), frames = C.pipeline_clip("large")
    assert (w, h, len(frames)) == (640, 480, 8)
    assert [C.Model(f[:h]).n for f in frames[:3]] == [302736] * 3 and max(C.Model(f[:h]).n for f in frames[3:]) < 6000
    assert 21010 < C.SPEC_CAP < 55616 < 126616 < C.KEY_CAP < 302736


def test_hooks_refuse_bad_arguments_without_a_device():
    """vstabx_corners_fused checks everything before it touches the device; vstabx_detector_counters refuses null."""
    vs = importlib.import_module("video-annotator_amd")

    class Fake:   # a "device" plane: only its pointer and pitch reach the library, which refuses before using them
        def __init__(self, ptr, pitch, shape):
            self.ptr, self.pitch, self.shape = ptr, pitch, shape

        def data_ptr(self):
            return self.ptr

        def stride(self, d):
            return self.pitch

    def refused(gray, **kw):
        with pytest.raises(vs.VstabError) as e:
            vs.corners_fused(gray, stream=ctypes.c_void_p(), **kw)
        assert e.value.status == vs.ERR_INVALID and "vstabx_corners_fused: " in str(e.value), str(e.value)

    ok = Fake(4096, 640, (360, 640))
    refused(Fake(0, 640, (360, 640)))                     # null image
    refused(Fake(4096, 639, (360, 640)))                  # pitch below the width
    refused(ok, w=2)
    refused(ok, h=2)
    refused(ok, w=0)
    refused(ok, h=-1)
    refused(Fake(4096, 1 << 20, (4096, 640)))             # a plane of 4 GiB
    refused(Fake(4096, 1 << 16, (1 << 15, 1 << 16)))      # 2^31 pixels
    for q in (0.0, -0.01, 1.5, float("nan")):
        refused(ok, quality=q)
    for cap in (0, -1, (1 << 24) + 1):
        refused(ok, cap=cap)
    for canary in (0, -1, (1 << 16) + 1):
        refused(ok, canary=canary)
    L, c = vs.lib, ctypes
    keys, counts, tiles = (c.c_uint64 * 80)(), (c.c_uint * 2)(), (c.c_uint * 72)()
    for args in ((None, counts, tiles), (keys, None, tiles), (keys, counts, None)):
        assert L.vstabx_corners_fused(4096, 640, 640, 360, 0.01, 16, 64, *args, None) == vs.ERR_INVALID
    assert L.vstabx_detector_counters(None, (c.c_long * 3)()) == vs.ERR_INVALID
    assert L.vstabx_detector_counters(4096, None) == vs.ERR_INVALID
