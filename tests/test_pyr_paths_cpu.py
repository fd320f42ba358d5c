"""The pyramid's model (tests/pyr_paths.py) checked without a device: the case tables reach every named path of k_pyr_down, k_pyr_down_x2 and
k_pack_pyr, and each case the paths it is there for; the modelled grids and tiles produce every output exactly once and read nothing they did
not write; the oracle's pyrDown equals the closed-form definition (and scipy's `mirror`) from 1 x 1 on; and every refusal of the three
launchers, by its exact text, with the planes at exactly 4 GiB and one pitch step under."""
import collections
import re
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import oracle
import pyr_paths as pp

P = 4096                       # a non-null dummy address, 16-byte aligned; refused calls never dereference it
G4 = 1 << 32


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(pp.TABLES))
def test_the_cases_reach_every_path_and_each_the_paths_it_names(kind):
    cases, names = pp.TABLES[kind]
    assert len({c.id for c in cases}) == len(cases), "two cases are the same call"
    reached = collections.defaultdict(list)
    print(f"\n{kind}: {len(cases)} cases")
    for c in cases:
        got = pp.paths(c)
        extra = set(got) - names - {"copy_edge_clipped"}
        assert not extra, (c.id, extra)
        assert c.what and set(c.what) <= set(got), (c.id, "names", c.what, "reaches", sorted(got))
        assert got.get("copy_edge_clipped", 0) == 0, c.id
        for n in got:
            reached[n].append(c.id)
        print(f"  {c.id:48s} {' '.join(f'{n}={v}' for n, v in sorted(got.items()))}")
    print(f"{kind}: path -> cases that reach it")
    for n in sorted(names):
        ids = reached.get(n, [])
        print(f"  {n:28s} {len(ids):3d}  {' '.join(ids[:6])}{' ...' if len(ids) > 6 else ''}")
    assert set(reached) == set(names), ("never reached", sorted(names - set(reached)))


def test_the_thresholds_the_issue_states():
    """The facts the case tables lean on, from the model: the first interior tile of the two-level kernel, the first width with two interior
    workgroups a row, when a stored output's tap folds twice, and that k_pack_pyr's edge copy never clips."""
    for sw, sh in ((139, 83), (140, 82), (140, 83)):
        c = pp._x2(sw, sh, (0, pp.al(sw, 4)), (0, pp.al((sw + 1) // 2, 4)), (0, 36))
        H, tiles = pp.x2_tiles(c)
        assert [(T.bx, T.by) for T in tiles if T.interior] == ([(1, 1)] if (sw, sh) == (140, 83) else []), (sw, sh)
    assert pp.pyr_grid(531, 266, 3, True).nbx == 1 and pp.pyr_grid(532, 266, 3, True).nbx == 2
    for sw in range(1, 30):
        for sh in range(1, 12):
            assert (sum(pp.multi_fold_taps(sw, sh)) > 0) == (sw <= 2 or sh <= 2), (sw, sh)
    for w in range(16, 200, 8):
        assert pp.pack_paths(pp._pack(w, 6)).get("copy_edge_clipped", 0) == 0, w
    # every cause that denies uv_vec has a case where it is the only one
    alone = {tuple(pp.pack_host(c)["uv_causes"]) for c in pp.PACK_CASES if pp.pack_ok(c)}
    assert {("chroma_base",), ("chroma_pitch",), ("width",), ("ring_base",), ()} <= alone, alone
    # interior groups of the fused copy: none at 16 wide, the first at 24 and 32
    assert [pp.pyr_grid(w, w // 2, 2, True).g_hi - 1 for w in (16, 24, 32, 40)] == [0, 1, 2, 3]


# ---- the grid is a partition -----------------------------------------------------------------------------------------------------------
def _check_grid(sw, dw, dh, wide, tag):
    G = pp.pyr_grid(sw, dw, dh, wide)
    eg, ey, ig, iy = pp.decode_grid(G, dh)
    assert ((ig >= 1) & (8 * ig + 12 <= sw) & (4 * ig + 4 <= dw)).all(), tag
    if not wide:
        assert ig.size == 0, tag
    g, y = np.concatenate([eg, ig]), np.concatenate([ey, iy])
    assert g.size == G.n_groups * dh and (g >= 0).all() and (g < G.n_groups).all() and (y >= 0).all(), tag
    assert np.unique(y * G.n_groups + g).size == g.size, (tag, "a group is produced twice")
    # and no edge workgroup is all idle, no interior one either: the grid is as small as the decode allows
    assert G.nb_edge == pp.div_up(eg.size, 256), tag
    # every group that could be interior is, when wide
    if wide:
        could = sum(1 for k in range(1, G.n_groups) if 8 * k + 12 <= sw and 4 * k + 4 <= dw)
        assert ig.size == could * dh, tag


def test_the_grid_of_k_pyr_down_produces_every_group_once():
    for sw in range(1, 601):
        dw = (sw + 1) // 2
        for dh in range(1, 10):
            for wide in (False, True):
                _check_grid(sw, dw, dh, wide, (sw, dh, wide))
    for kind in ("down", "pack"):
        for c in pp.TABLES[kind][0]:
            H = pp.down_host(c.sw, c.sh, c.src, c.dst) if kind == "down" else pp.pack_host(c)
            wide = (H["vec_ok"] and H["near"]) if kind == "down" else True
            if kind == "pack" and not H["ok"]:
                continue
            _check_grid(c.sw, H["dw"], H["dh"], wide, c.id)


def _check_tiles(c):
    H, tiles = pp.x2_tiles(c)
    mid = np.zeros((H["mh"], H["mw"]), np.int32)
    out = np.zeros((H["dh"], H["dw"]), np.int32)
    for T in tiles:
        for y, x, n, kind in T.mid:
            assert 0 <= y < H["mh"] and 0 <= x and x + n <= H["mw"] and n >= 1, (c.id, T.bx, T.by, "first-level store outside the level")
            assert kind != "dword" or (H["vec_ok"] and x % 4 == 0), c.id
            mid[y, x:x + n] += 1
        for y, x, n, kind in T.out:
            assert 0 <= y < H["dh"] and 0 <= x and x + n <= H["dw"], (c.id, T.bx, T.by, "second-level store outside the level")
            assert kind != "dword" or (H["dst_vec_ok"] and x % 4 == 0), c.id
            out[y, x:x + n] += 1
        for rows, cols in T.reads:
            assert rows.min() >= 0 and rows.max() < pp.P2_MH and cols.min() >= 0 and cols.max() < pp.P2_MW, (c.id, T.bx, T.by, rows, cols, "read outside the region")
            assert T.written[np.ix_(rows, cols)].all(), (c.id, T.bx, T.by, rows, cols, "read of a region byte no thread wrote")
        if T.interior:
            assert T.written.all() and not T.reads
            x0, y0 = 16 * T.bx, 10 * T.by
            assert 2 * (2 * x0 - 4) - 4 >= 0 and 2 * (2 * y0 - 2) - 2 >= 0, "an interior tile's loads start inside the source"
            assert 2 * (2 * x0 - 4 + 4 * 9) - 4 + 16 <= H["sw"] and 2 * (2 * y0 - 2 + 22) + 2 < H["sh"], "and end inside it"
    assert (mid == 1).all(), (c.id, "first level", np.argwhere(mid != 1)[:4].tolist())
    assert (out == 1).all(), (c.id, "second level", np.argwhere(out != 1)[:4].tolist())


def test_the_tiles_of_k_pyr_down_x2_cover_both_levels_once_and_read_what_they_wrote():
    n = 0
    for c in pp.X2_CASES:
        if pp.x2_ok(c.sw, c.sh):
            _check_tiles(c)
            n += 1
    assert n >= 20
    # a sweep over small sizes, aligned and not (the planes' pitches rounded up to 4)
    for sw in list(range(15, 80)) + [135, 139, 140, 141, 144]:
        for sh in ((15, 18, 43) if sw < 80 else (83, 84)):
            mw = (sw + 1) // 2
            for off in (0, 1):
                _check_tiles(pp._x2(sw, sh, (off, pp.al(sw, 4)), (0, pp.al(mw, 4)), (0, pp.al((mw + 1) // 2, 4))))


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def test_the_oracle_is_the_closed_form_definition_from_1x1_on():
    k = np.array([1, 4, 6, 4, 1])
    n_scipy = 0
    for h in range(1, 13):
        for w in range(1, 13):
            for kind in ("random", "extreme"):
                img = pp.content(kind, 31 * h + w, w, h)
                exp = pp.pyr_down_ref(img)
                assert exp.shape == ((h + 1) // 2, (w + 1) // 2)
                assert np.array_equal(oracle.pyr_down(img), exp), (w, h, kind)
                try:       # scipy's mirror folds once or not at all, by version: ask it, and count what it answered
                    acc = ndi.correlate1d(ndi.correlate1d(img.astype(np.int64), k, axis=0, mode="mirror"), k, axis=1, mode="mirror")
                except (RuntimeError, ValueError):
                    continue
                if min(w, h) >= 3:    # (a filter longer than the mirrored image: scipy's answer is its own below that)
                    assert np.array_equal(((acc + 128) >> 8)[::2, ::2].astype(np.uint8), exp), (w, h, kind)
                    n_scipy += 1
    assert n_scipy >= 2 * 10 * 10
    for w, h in ((44, 9), (144, 84), (32, 6)):      # the 0 / 255 content reaches the largest sum there is: 255 * 256 (+ 128) -> 255
        assert pp.pyr_down_ref(pp.content("extreme", 7 * w + h, w, h))[0, 0] == 255
    flat = np.full((7, 9), 255, np.uint8)
    assert (pp.pyr_down_ref(flat) == 255).all() and (pp.pyr_down_ref(np.zeros((1, 1), np.uint8)) == 0).all()
    # the closed-form fold against the loop it replaces
    for n in range(1, 9):
        for i in range(-20, 30):
            j = i
            while n > 1 and (j < 0 or j >= n):
                j = -j if j < 0 else 2 * n - 2 - j
            assert pp.fold101(i, n) == (0 if n == 1 else j), (i, n)


# ---- the model restates the sources ------------------------------------------------------------------------------------------------------------
def test_the_constants_and_messages_are_the_sources_own():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "video-annotator_amd", "csrc", "vstab_pyramid.hip")).read()
    assert re.search(r"constexpr int P2_TW = (\d+), P2_TH = (\d+);", src).groups() == (str(pp.P2_TW), str(pp.P2_TH))
    assert "P2_MG = (2 * P2_TW + 5 + 3) / 4, P2_MW = 4 * P2_MG" in src and "P2_MH = 2 * P2_TH + 3" in src
    assert "bool pyr_down_x2_ok(int sw, int sh) { return (sw + 1) / 2 >= 8 && (sh + 1) / 2 >= 8; }" in src
    stateless = open(os.path.join(root, "video-annotator_amd", "csrc", "vstab_stateless.cpp")).read()
    for m in (pp.MSG_DOWN_4G, pp.MSG_X2_4G, pp.MSG_X2_SMALL, pp.MSG_PACK):
        assert src.count('"' + m + '"') == 1, m
    for m in (pp.MSG_DOWN_ARG, pp.MSG_X2_ARG):
        assert stateless.count('"' + m + '"') == 1, m


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
_DOWN = dict(src=P, pitch_src=64, width=64, height=32, dst=P, pitch_dst=32, stream=None)
_X2 = dict(src=P, pitch_src=64, width=64, height=32, mid=P, pitch_mid=32, dst=P, pitch_dst=16, stream=None)
# (arguments that differ from a good call, message).  Two faults at once: the earlier check's message wins.
DOWN_ROWS = [(d, pp.MSG_DOWN_ARG) for d in (
    dict(src=None), dict(dst=None), dict(width=0), dict(width=-1), dict(height=0), dict(height=-5), dict(pitch_src=63), dict(pitch_dst=31),
    dict(width=63, pitch_src=62), dict(width=63, pitch_src=63, pitch_dst=31), dict(src=None, pitch_src=G4), dict(pitch_dst=31, pitch_src=G4 // 32))] + [
    (d, pp.MSG_DOWN_4G) for d in (
        dict(pitch_src=G4 // 32),                     # the source plane is exactly 2^32 bytes
        dict(pitch_dst=G4 // 16),                     # the level is
        dict(pitch_src=G4), dict(pitch_src=G4 // 32 + 1), dict(pitch_src=G4 // 32, pitch_dst=G4 // 16),
        dict(height=31, pitch_dst=G4 // 16),          # an odd height: dh = 16 rows
        dict(width=1, height=1, pitch_src=G4), dict(width=1, height=1, pitch_src=1, pitch_dst=G4))]
X2_ROWS = [(d, pp.MSG_X2_ARG) for d in (
    dict(src=None), dict(mid=None), dict(dst=None), dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(pitch_src=63), dict(pitch_mid=31),
    dict(pitch_dst=15), dict(width=61, pitch_mid=30), dict(width=61, pitch_dst=15), dict(mid=None, pitch_src=G4), dict(width=8, pitch_dst=1))] + [
    (d, pp.MSG_X2_4G) for d in (
        dict(pitch_src=G4 // 32), dict(pitch_mid=G4 // 16), dict(pitch_dst=G4 // 8), dict(pitch_src=G4), dict(height=29, pitch_dst=G4 // 8),
        dict(pitch_src=G4 // 32, pitch_mid=G4 // 16, pitch_dst=G4 // 8))] + [
    # under 15 x 15 the entry point runs launch_pyr_down twice: that launcher's message, for the first launch (src -> mid) or the second (mid -> dst)
    (d, pp.MSG_DOWN_4G) for d in (
        dict(width=14, height=16, pitch_src=G4 // 16), dict(width=14, height=16, pitch_mid=G4 // 8), dict(width=14, height=16, pitch_dst=G4 // 4),
        dict(width=64, height=14, pitch_src=G4 // 14 + 1), dict(width=1, height=1, pitch_dst=G4))]


def _planes(d, names):
    return [(0, d["pitch_" + n]) for n in names]


def test_vstab_pyr_down_refuses_by_name_without_a_device(vs):
    L = vs.lib
    for bad, text in DOWN_ROWS:
        a = dict(_DOWN, **bad)
        assert L.vstab_pyr_down(*a.values()) == vs.ERR_INVALID, bad
        assert L.vstab_last_error() == text.encode(), bad
        if a["src"] and a["dst"]:
            assert pp.down_refusal(a["width"], a["height"], *_planes(a, ("src", "dst"))) == (pp.ERR_INVALID, text), bad


def test_vstab_pyr_down_x2_refuses_by_name_without_a_device(vs):
    L = vs.lib
    for bad, text in X2_ROWS:
        a = dict(_X2, **bad)
        assert L.vstab_pyr_down_x2(*a.values()) == vs.ERR_INVALID, bad
        assert L.vstab_last_error() == text.encode(), bad
        if a["src"] and a["mid"] and a["dst"]:
            assert pp.x2_refusal(a["width"], a["height"], *_planes(a, ("src", "mid", "dst"))) == (pp.ERR_INVALID, text), bad


def test_the_launchers_own_checks_at_4_gib_and_one_pitch_step_under(vs):
    """vstabx_pyr_down_check: what launch_pyr_down / launch_pyr_down_x2 refuse, asked without a launch.  Each plane at exactly 2^32 bytes is
    refused, at one byte of pitch less it is not -- and the largest source the 4 GiB tests of test_pyr_paths_gpu.py run is accepted."""
    chk = vs.lib.vstabx_pyr_down_check
    w, h = 64, 32                                    # levels of 32 x 16 and 16 x 8
    for two, text in ((0, pp.MSG_DOWN_4G), (1, pp.MSG_X2_4G)):
        good = dict(pitch_src=64, pitch_mid=32, pitch_dst=16 if two else 32)
        rows = dict(pitch_src=h, pitch_mid=h // 2, pitch_dst=h // 4 if two else h // 2)
        assert chk(good["pitch_src"], w, h, good["pitch_mid"], good["pitch_dst"], two) == vs.OK
        for name in (("pitch_src", "pitch_mid", "pitch_dst") if two else ("pitch_src", "pitch_dst")):
            at = dict(good, **{name: G4 // rows[name]})
            assert chk(at["pitch_src"], w, h, at["pitch_mid"], at["pitch_dst"], two) == vs.ERR_INVALID, (two, name)
            assert vs.lib.vstab_last_error() == text.encode(), (two, name)
            under = dict(good, **{name: G4 // rows[name] - 1})
            assert chk(under["pitch_src"], w, h, under["pitch_mid"], under["pitch_dst"], two) == vs.OK, (two, name)
        assert pp.BIG_PITCH % 4 == 0 and pp.BIG_PITCH * pp.BIG_H < G4 <= (pp.BIG_PITCH + 4) * pp.BIG_H
        assert chk(pp.BIG_PITCH, pp.BIG_W, pp.BIG_H, 72, 36 if two else 72, two) == vs.OK
        assert chk(pp.BIG_PITCH + 4, pp.BIG_W, pp.BIG_H, 72, 36 if two else 72, two) == vs.ERR_INVALID
    assert chk(64, 14, 14, 32, 16, 1) == vs.ERR_INVALID and vs.lib.vstab_last_error() == pp.MSG_X2_SMALL.encode()
    assert chk(G4, 14, 14, 32, 16, 1) == vs.ERR_INVALID and vs.lib.vstab_last_error() == pp.MSG_X2_SMALL.encode()   # the size is looked at first


def _pack_args(c, base=P):
    """The Call's planes at fake addresses with its base offsets: (y, pitch_y, uv, pitch_uv, w, h, ring, dst, dpitch)."""
    return (base + c.src[0], c.src[1], 2 * base + c.uv[0], c.uv[1], c.sw, c.sh, 3 * base + c.ring, 4 * base + c.dst[0], c.dst[1])


def test_pack_pyr_ok_is_the_models_and_its_launcher_refuses_by_name_without_a_device(vs):
    """The hook's answer for every case (-1 = pack_pyr_ok is false) and launch_pack_pyr's own refusal; only refused cases are asked here: an
    accepted one would launch."""
    n = 0
    for c in pp.PACK_CASES:
        if pp.pack_ok(c):
            continue
        assert vs.pack_pyr(*_pack_args(c), stream=0) == -1, c.id
        assert vs.pack_pyr(*_pack_args(c), launch_anyway=True, stream=0) == vs.ERR_INVALID, c.id
        assert vs.lib.vstab_last_error() == pp.MSG_PACK.encode(), c.id
        n += 1
    assert n >= 5
    # the 32-bit products of k_pack_pyr: every plane it indexes, at exactly 2^32 bytes
    good = pp._pack(32, 8)
    for over in (dict(src=(0, G4 // 8)), dict(uv=(0, G4 // 4)), dict(dst=(0, G4 // 4)), dict(src=(0, 1 << 24)), dict(uv=(0, 1 << 24))):
        c = pp.dataclasses.replace(good, **over)
        assert not pp.pack_ok(c), over
        assert vs.pack_pyr(*_pack_args(c), stream=0) == -1, over
    assert pp.pack_ok(pp.dataclasses.replace(good, dst=(0, G4 // 4 - 4)))


def test_the_binding_checks_caller_planes_without_a_device(vs):
    import torch
    img = torch.zeros((6, 20), dtype=torch.uint8)
    for out in (torch.zeros((3, 10), dtype=torch.int8), torch.zeros((3, 11), dtype=torch.uint8), torch.zeros((3, 20), dtype=torch.uint8)[:, ::2],
                torch.zeros((10, 3), dtype=torch.uint8).t(), torch.zeros((3, 10, 1), dtype=torch.uint8), np.zeros((3, 10), np.uint8)):
        with pytest.raises(ValueError, match="pyr_down: out must be"):
            vs.pyr_down(img, out=out)
    with pytest.raises(ValueError, match=r"pyr_down_x2 \(dst\): out must be"):
        vs.pyr_down_x2(img, out=(torch.zeros((3, 10), dtype=torch.uint8), torch.zeros((2, 6), dtype=torch.uint8)))
    with pytest.raises(ValueError, match=r"pyr_down_x2 \(mid\): out must be"):
        vs.pyr_down_x2(img, out=(torch.zeros((3, 9), dtype=torch.uint8), torch.zeros((2, 5), dtype=torch.uint8)))
