"""The cost-weighted XCD bands of the fused 8-bit warp (vstab_warp_bands.hpp: weighted_bands, band_costs, BandCache), run as the
library's own code through the vstabx_weighted_bands / vstabx_band_costs / vstabx_band_cache_run hooks.  For every output size of the
dense sweep (1..300 rows x every number of tile columns a width of 1..300 gives) and the shapes of test_shapes_gpu.py, with uniform,
modelled, random, all-zero and one-huge-row cost vectors: band_y[0] == 0, band_y[8] == dh, non-decreasing multiples of the half-tile
height; split_y - band_y a multiple of the tall height and tile_schedule's tail rule per band; grid == 8 max(share); and the kernels'
block -> tile prologue (layouts.block_tiles) covers every tile exactly once with no live workgroup below the image.  A uniform vector
gives exactly layouts.tile_schedule."""
import ctypes

import numpy as np
import pytest

import dead_tiles as D
import layouts
import oracle
from test_shapes_gpu import SHAPES, STATELESS_OUTPUTS, warp_output

_u32p, _ip, _fp = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def L(vs):
    lib = vs.lib
    lib.vstabx_weighted_bands.restype = ctypes.c_int
    lib.vstabx_weighted_bands.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double, _u32p, ctypes.c_int, _ip]
    lib.vstabx_band_costs.restype = ctypes.c_int
    lib.vstabx_band_costs.argtypes = [_fp, ctypes.c_int] + [ctypes.c_int] * 5 + [_u32p, ctypes.c_int]
    lib.vstabx_band_cache_run.restype = ctypes.c_int
    lib.vstabx_band_cache_run.argtypes = [_fp, ctypes.c_int] + [ctypes.c_int] * 7 + [ctypes.c_double, _ip, ctypes.POINTER(ctypes.c_long)]
    return lib


def _sched(out):
    return dict(band_y=[int(v) for v in out[:9]], split_y=[int(v) for v in out[9:17]], tiles_x=int(out[17]), grid=int(out[18]))


def weighted(L, dw, dh, rwb, lds_kb, tail, cost):
    out = np.zeros(19, np.int32)
    c = None if cost is None else np.ascontiguousarray(cost, np.uint32)
    st = L.vstabx_weighted_bands(dw, dh, rwb, lds_kb, float(tail), None if c is None else c.ctypes.data_as(_u32p), 0 if c is None else len(c),
                                 out.ctypes.data_as(_ip))
    assert st == 0
    return _sched(out)


def model_costs(L, params, sw, sh, dw, dh, ts, nan_behind=False):
    n = -(-dh // ts)
    cost = np.zeros(n, np.uint32)
    p = np.ascontiguousarray(params, np.float32)
    assert L.vstabx_band_costs(p.ctypes.data_as(_fp), int(nan_behind), sw, sh, dw, dh, ts, cost.ctypes.data_as(_u32p), n) == 0
    return cost


def check(s, dw, dh, rwb, lds_kb, tail):
    th, ts = 4 * rwb, 2 * rwb
    half_rows, tx = -(-dh // ts), -(-dw // 64)
    b, sp = s["band_y"], s["split_y"]
    assert s["tiles_x"] == tx and b[0] == 0 and b[8] == dh and all(x <= y for x, y in zip(b, b[1:]))
    assert all(v % ts == 0 or v == dh for v in b)
    slots = layouts.SLOTS_PER_WG_PER_CU * max(1, min(8, layouts.LDS_BUDGET_KB // lds_kb))
    shares = []
    for k in range(8):
        rows = b[k + 1] - b[k]
        tall_max = rows // th
        tall = tall_max - min(tall_max, layouts._lround(tail * slots / tx))
        assert sp[k] == b[k] + tall * th and (sp[k] - b[k]) % th == 0, (k, s)
        shares.append(tall * tx + -(-(b[k + 1] - sp[k]) // ts) * tx)
    assert s["grid"] == 8 * max(shares)
    live, idle = layouts.block_tiles(dict(s, shares=shares), rwb)
    assert len(live) + idle == s["grid"]
    blk, x0, ys, rows = (np.array(v, np.int64) for v in zip(*live))
    assert (ys < dh).all() and (ys >= 0).all() and (x0 < dw).all() and (x0 % 64 == 0).all() and (ys % ts == 0).all()
    k = blk & 7
    lo, hi = np.array(b)[k], np.array(b)[k + 1]
    assert (ys >= lo).all() and (ys < hi).all()
    tall = rows == th
    assert (ys[tall] + rows[tall] <= hi[tall]).all()
    cover = np.zeros((half_rows, tx), np.int64)
    for n in (1, 2):
        sel = rows >= n * ts
        np.add.at(cover, (ys[sel] // ts + n - 1, x0[sel] // 64), 1)
    assert cover.min() == 1 and cover.max() == 1, (dw, dh, rwb, lds_kb, tail, int((cover != 1).sum()))


def cost_vectors(L, dw, dh, ts, rng):
    """uniform, the model's (a GoPro-wide source of the output's size seen through a camera centred on the output), random (zeros among
    them), all-zero, one huge row."""
    n = -(-dh // ts)
    sw, sh = max(2, dw), max(2, dh)
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, sw, sh)
    Ko = np.eye(3)
    Ko[0, 0] = Ko[1, 1] = 0.45 * K[0, 0]
    Ko[0, 2], Ko[1, 2] = (dw - 1) / 2, (dh - 1) / 2
    huge = np.ones(n, np.uint32)
    huge[int(rng.integers(0, n))] = 4_000_000_000
    return {"uniform": np.full(n, 7, np.uint32), "model": model_costs(L, oracle.map_params(K, Ko, oracle.rodrigues((0.02, -0.05, 0.01))), sw, sh, dw, dh, ts),
            "random": (rng.integers(0, 1000, n) * rng.integers(0, 2, n)).astype(np.uint32), "zero": np.zeros(n, np.uint32), "huge": huge}


def launch_choices(dw, dh):
    return {layouts.fused_launch(dw, dh), (4, 20, 0.5), (8, 40, 0.5), (4, 20, 0.25), (8, 40, 1.0)}


def run_all(L, dw, dh, rng):
    for rwb, lds_kb, tail in launch_choices(dw, dh):
        even = layouts.tile_schedule(dw, dh, rwb, lds_kb, tail)
        for kind, cost in cost_vectors(L, dw, dh, 2 * rwb, rng).items():
            s = weighted(L, dw, dh, rwb, lds_kb, tail, cost)
            check(s, dw, dh, rwb, lds_kb, tail)
            if kind in ("uniform", "zero"):
                assert all(s[key] == even[key] for key in ("band_y", "split_y", "tiles_x", "grid")), (kind, dw, dh, rwb, tail)
        assert weighted(L, dw, dh, rwb, lds_kb, tail, None)["band_y"] == even["band_y"]          # the hook's even bands are the model's
        short = weighted(L, dw, dh, rwb, lds_kb, tail, np.ones(-(-dh // (2 * rwb)) + 1, np.uint32))  # a vector of the wrong length: even bands
        assert short["band_y"] == even["band_y"] and short["grid"] == even["grid"]


def test_dense_sweep(L):
    """Heights 1..300 at every number of tile columns widths 1..300 give (the schedule depends on the width only through it), the launcher's
    own choice of tile shape and tail and every other tail in use."""
    rng = np.random.default_rng(1)
    for dh in range(1, 301):
        for dw in (1, 64, 65, 129, 193, 257, 300):
            run_all(L, dw, dh, rng)


def _all_outputs():
    out = [(dw, dh) for name in SHAPES for dw, dh in [warp_output(name)]]
    return out + [(w, h) for name, (w, h, _) in SHAPES.items()] + list(STATELESS_OUTPUTS) + [(3524, 1999), (3072, 1024)]


@pytest.mark.parametrize("dw,dh", _all_outputs())
def test_gpu_shapes(L, dw, dh):
    run_all(L, dw, dh, np.random.default_rng(dw + dh))


def test_headline_bands_follow_the_cost(L):
    """4K headline: the model's vector is low in the first and last rows (dead tiles) and highest in the middle; the weighted bands give
    the outer XCDs more rows than the inner ones, and every band's cost is within one row's cost of an eighth of the total."""
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, 3840, 2160)
    Ko, (cw, ch) = oracle.get_output_camera(K, 3840, 2160)
    p = oracle.map_params(K, Ko, np.eye(3))
    cost = model_costs(L, p, 3840, 2160, cw, ch, 16).astype(np.int64)
    assert cost[:8].max() < 0.7 * cost[55:70].min() and cost[-8:].max() < 0.7 * cost[55:70].min()
    s = weighted(L, cw, ch, 8, 40, 0.5, cost)
    check(s, cw, ch, 8, 40, 0.5)
    rows = np.diff(s["band_y"])
    assert rows[0] > rows[3] and rows[7] > rows[4]
    per_band = [cost[a // 16:-(-b // 16)].sum() for a, b in zip(s["band_y"], s["band_y"][1:])]
    assert max(per_band) - cost.sum() / 8 <= cost.max(), (per_band, cost.sum() / 8)
    # the host's dead / live guess (it only steers placement) against the kernel's rule: never fewer dead tiles in a row than the rule finds
    ruled = D.rule(p, cw, ch, 3840, 2160, 16).sum(axis=1)
    assert (cost[ruled == 56] == 56 * 135).all() and (cost[ruled == 0] >= 56 * 220).all() and ruled.sum() > 2000


def test_cache_hits_within_the_angle_and_recomputes_beyond(L):
    """The same launch again hits; a rotation 1 degree away hits and gets the cached bands; 4 degrees away misses and gets its own; other
    sizes or another mode never share an entry; a long bounded shake ends up all hits."""
    w, h = 3840, 2160
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, w, h)
    Ko, (cw, ch) = oracle.get_output_camera(K, w, h)

    def run(rvecs, mode=5):
        ps = np.ascontiguousarray(np.stack([oracle.map_params(K, Ko, oracle.rodrigues(r)) for r in rvecs]), np.float32)
        out, counts = np.zeros((len(rvecs), 19), np.int32), (ctypes.c_long * 3)()
        assert L.vstabx_band_cache_run(ps.ctypes.data_as(_fp), len(rvecs), w, h, cw, ch, mode, 8, 40, 0.5, out.ctypes.data_as(_ip), counts) == 0
        return out, list(counts)

    d = np.deg2rad
    out, counts = run([(0, 0, 0), (0, 0, 0), (d(1.0), 0, 0), (d(4.0), 0, 0), (d(4.5), 0, 0), (0, 0, 0)])
    assert counts == [4, 2, 2]
    assert (out[1] == out[0]).all() and (out[2] == out[0]).all() and (out[4] == out[3]).all() and (out[5] == out[0]).all()
    assert (out[3] != out[0]).any()                                   # 4 degrees of pitch move the bands
    for o in out:
        check(_sched(o), cw, ch, 8, 40, 0.5)
    rng = np.random.default_rng(3)
    shake = rng.normal(0.0, d(1.0), (400, 3)).clip(-d(2.5), d(2.5))
    _, counts = run(list(shake) + list(shake))
    assert counts[1] <= 32 and counts[0] >= 800 - 32 and counts[0] + counts[1] == 800, counts
