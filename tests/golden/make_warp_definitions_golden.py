"""Generates tests/golden/warp_definitions_kat.npz, recorded answers of the numpy warp definition and of the tile model themselves
(tests/warp_def.py, tests/warp_tiles.py):
python tests/golden/make_warp_definitions_golden.py

The committed file was produced at commit e40f3ec ("Test definitions: one numpy detector, one numpy tracker"), the last one at which the
warp was defined in seven layers (cubic_def, lanczos4_def, border_def, resample_border_def, keep_def, distort_resample_def, rs_resample_def)
and its tiles in five (cubic_tiles, lanczos4_tiles, border_tiles, resample_border_tiles, keep_tiles).  There the tests held those layers
against each other; the answers here are what the OLDER layer of each pair gave on the inputs of those tests -- cubic_def.remap_cubic and
lanczos4_def.remap_lanczos4 under resample_border_def's CONSTANT, border_def.remap_border(CONSTANT) under keep_def.remap_keep -- and what the
five tile models gave, computed by this file's cases through a thin adapter with warp_def's and warp_tiles' signatures.  Run through the
single definition and the single model there are now it must reproduce the file bit for bit (test_warp_definitions_kat_cpu.py), and the
tests that used to compare two layers compare the one definition with the file.

  constant_c<cn>_*     src (13 x 17), mapx, mapy (11 x 15), border and the constant-border cubic and lanczos4 remaps
                       (test_resample_border_cpu.py::test_constant_equals_constant_definitions)
  keep_c<cn>_*         src (23 x 31), mapx, mapy, prev (17 x 29) and the constant-border bilinear remap with borders 0 and 255
                       (test_keep_cpu.py::test_written_samples_are_the_constant_border_warp_and_kept_ones_are_prev)
  edges_n<n>_a<axis>_* src (n x n), mapx, mapy, prev and the constant-border bilinear remap (test_keep_cpu.py::test_the_rule_at_the_edges)
  states_<case>_<resampler>_<rule>   tile_states of a case as (3 planes, states) counts: planes in PLANES' order, states in RECORDED[rule]'s --
                       the state names the model of that rule's kernels had at that commit --, a least_over of None as -1.  The cases: every
                       TILE_SETS entry under its kernel's rule (k_warp_border's also under `clamp`, BORDER_CONSTANT), and the named shapes of
                       test_distort_resample_cpu.py, test_rs_resample_cpu.py and test_pinhole_cpu.py under every kernel they are run with.

The file holds inputs and recorded results of this project's own test definitions only.  Fixtures are data only; their purpose is that an
edit of the definition or of the model shows: the committed tests assert "at least" counts, the GPU tests rely on these inputs reaching the
states, and nothing else anchors the model.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import warp_def as wd  # noqa: E402
import warp_tiles as wt  # noqa: E402

PLANES = ("bgr", "luma", "chroma")
_BOXED = ("none", "staged", "gathered", "at_budget", "over_by_one", "least_over", "odd_w", "even_w", "partial_staged")
RECORDED = {"touching": _BOXED, "every": wt.BORDER_STATES, "clamp": wt.BORDER_STATES, "written": wt.KEEP_STATES}
EXACT = [("cubic", "every"), ("cubic", "touching"), ("lanczos4", "every"), ("lanczos4", "touching")]      # the cubic and Lanczos kernels
DIST_EX = [("linear", "every")] + EXACT                  # vstab_warp_nv12_dist_ex: linear + CONSTANT is the probing kernels'
PINHOLE = [("linear", "clamp")] + DIST_EX                # vstab_warp_nv12_pinhole: k_warp_border under BORDER_CONSTANT too


def edge_positions(n):
    """X = -1, 0, n - 2, n - 1 with and without a fraction, NaN, +-3e9, inf"""
    return np.array([-1.0, -0.5, -1 / 64, 0.0, 0.25, n - 2.0, n - 1.5, n - 1.0 - 1 / 32, n - 1.0, n - 0.5, np.nan, 3e9, -3e9, np.inf], np.float32)


def random_keep_case(rng, cn, sw=31, sh=23, dw=29, dh=17):
    src = rng.integers(0, 256, (sh, sw, cn) if cn > 1 else (sh, sw), dtype=np.uint8)
    prev = rng.integers(0, 256, (dh, dw, cn) if cn > 1 else (dh, dw), dtype=np.uint8)
    mx = rng.uniform(-0.4 * sw, 1.4 * sw, (dh, dw)).astype(np.float32)
    my = rng.uniform(-0.4 * sh, 1.4 * sh, (dh, dw)).astype(np.float32)
    mx[0, :5] = [np.nan, np.inf, -1e30, 32768.0, 3e9]
    my[1, :3] = [np.nan, -3e9, 3e9]
    return src, mx, my, prev


def definition_answers():
    out = {}
    rng = np.random.default_rng(12)
    for cn in (1, 2, 3):
        src = rng.integers(0, 256, (13, 17, cn) if cn > 1 else (13, 17), dtype=np.uint8)
        mx = rng.uniform(-20, 40, (11, 15)).astype(np.float32)
        my = rng.uniform(-15, 30, (11, 15)).astype(np.float32)
        bd = np.array((7, 200, 33)[:cn], np.int32)
        out.update({f"constant_c{cn}_src": src, f"constant_c{cn}_mapx": mx, f"constant_c{cn}_mapy": my, f"constant_c{cn}_border": bd})
        for r in ("cubic", "lanczos4"):
            out[f"constant_c{cn}_{r}"] = wd.remap(src, mx, my, r, wd.CONSTANT, bd)
    rng = np.random.default_rng(6)
    for cn in (1, 2, 3):
        src, mx, my, prev = random_keep_case(rng, cn)
        out.update({f"keep_c{cn}_src": src, f"keep_c{cn}_mapx": mx, f"keep_c{cn}_mapy": my, f"keep_c{cn}_prev": prev})
        for border in (0, 255):
            out[f"keep_c{cn}_border{border}"] = wd.remap(src, mx, my, "linear", wd.CONSTANT, border)
    for n in (2, 5, 64):
        src = np.arange(n * n, dtype=np.uint8).reshape(n, n)
        pos = edge_positions(n)
        inside = np.zeros(len(pos), np.float32)
        for axis, (mx, my) in enumerate(((pos[None], inside[None]), (inside[None], pos[None]))):
            k = f"edges_n{n}_a{axis}_"
            out.update({k + "src": src, k + "mapx": mx, k + "mapy": my, k + "prev": np.full((1, len(pos)), 200, np.uint8),
                        k + "constant": wd.remap(src, mx, my, "linear", wd.CONSTANT, 0)})
    return out


def state_cases():
    """-> (case name, mapx, mapy, sw, sh, [(resampler, rule)]) of every recorded tile_states"""
    from test_distort_resample_cpu import shape_maps as fisheye_maps
    from test_lens_gpu import ROTS
    from test_pinhole_cpu import shape_maps as pinhole_maps
    for kernel in sorted(wt.TILE_SETS):
        resampler, border_mode = wt.KERNELS[kernel]
        rules = [wt.kernel_rule(resampler, border_mode)] + (["clamp"] if kernel == "border" else [])
        for name in sorted(wt.TILE_SETS[kernel]):
            params, sw, sh, dw, dh, mode = wt.set_params(kernel, name)
            yield (f"set_{kernel}_{name}", *wd.maps(params, dw, dh, mode), sw, sh, [(resampler, rule) for rule in rules])
    for lens, shape_maps, modes, kernels in (("fisheye", fisheye_maps, (1, 2), DIST_EX), ("pinhole", pinhole_maps, (3, 4), PINHOLE)):
        for mode in modes:
            for (w, h, dw, dh), rot in (((640, 360, 333, 201), 1), ((1024, 576, 200, 72), 1), ((2048, 1152, 256, 128), 1), ((128, 72, 130, 70), 3)):
                yield (f"{lens}_{w}x{h}_m{mode}", *shape_maps(w, h, dw, dh, mode, ROTS[rot]), w, h, kernels)
    yield ("pinhole_3072x1728_m3", *pinhole_maps(3072, 1728, 256, 128, 3, ROTS[1]), 3072, 1728, PINHOLE)
    sw, sh, dw, dh, fi, fo = wd.ZOOMED_OUT
    p, rb = wd.case_params(sw, sh, dw, dh, fi, fo)
    for mode in (0, 1):
        yield (f"rs_zoomed_out_m{mode}", *wd.maps(p, dw, dh, mode, rb), sw, sh, EXACT)
    sw, sh, dw, dh, fi, fo = wd.GATHERS
    p, rb = wd.case_params(sw, sh, dw, dh, fi, fo, wd.GATHERS_R0, wd.GATHERS_R_BOTTOM)
    yield ("rs_gathers", *wd.maps(p, dw, dh, 1, rb), sw, sh, EXACT)
    p, rb = wd.case_params(64, 36, 65, 37, 30.0, 30.0, r0=(0.0, 0.0, 0.0), r_bottom=(0.0, 0.0, 0.0))
    p[4], p[5] = 32.0, 16.0
    yield ("rs_axis_pixel", *wd.maps(p, 65, 37, 0, rb), 64, 36, EXACT)


def stored(states, rule):
    """what the file holds of a tile_states dictionary: the recorded states of the rule, plane by plane"""
    return np.array([[-1 if states[p][k] is None else states[p][k] for k in RECORDED[rule]] for p in PLANES], np.int32)


def state_answers():
    out = {}
    for name, mx, my, sw, sh, kernels in state_cases():
        for resampler, rule in kernels:
            out[f"states_{name}_{resampler}_{rule}"] = stored(wt.tile_states(mx, my, sw, sh, resampler, rule), rule)
    return out


def build():
    return {**definition_answers(), **state_answers()}


def load():
    return np.load(os.path.join(HERE, "warp_definitions_kat.npz"))


def main(path=os.path.join(HERE, "warp_definitions_kat.npz")):
    out = build()
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
