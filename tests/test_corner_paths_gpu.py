"""GPU half of the corner detector's path tests: the raw output of k_corners_fused + k_filter_keys (test hook vstabx_corners_fused), the
public operators and the pipeline against the tile model of tests/corner_tiles.py and the oracle.  What each set reaches is asserted
without a GPU in test_corner_tiles_cpu.py.  Every comparison is exact."""
import numpy as np
import pytest

import corner_tiles as C
import oracle

pytestmark = pytest.mark.gpu

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
PARAMS = ((4000, 0.01, 0.0), (200, 0.01, 30.0))     # every candidate in order (as far as 4000 go); the pipeline's: the tie order on plateaus


def dev(img, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img)).to(cuda)


def unaligned_view(img, cuda):
    """the image as a pitched device view whose base is not 4-byte aligned and whose pitch is odd: the kernels' byte-wise loads"""
    import torch
    h, w = img.shape
    pitch = w + 5
    buf = torch.full((pitch * h + 8,), 77, dtype=torch.uint8, device=cuda)
    v = buf[1:1 + pitch * h].view(h, pitch)[:, :w]
    v.copy_(torch.from_numpy(np.ascontiguousarray(img)).to(cuda))
    assert v.data_ptr() % 4 != 0 and v.stride(0) == pitch
    return v


def check_raw(vs, m, gray, cap=None):
    """one run of the hook against the model m; returns (sorted keys, per-tile counts, tiles that spilled)"""
    cap = m.n + 7 if cap is None else cap
    keys, kept, spilled, tiles = vs.corners_fused(gray, m.quality, cap=cap, canary=64)
    print(f"{m.w} x {m.h}: kept {kept} (model {m.n}), spilled {spilled} (model {m.spilled_range()}), tile counts {tiles.ravel().tolist()[:12]}")
    assert kept == m.n
    n = min(kept, cap)
    assert (keys[n:] == FILL).all()                                  # nothing written past the keys: the tail of the buffer and the canary
    got = np.sort(keys[:n])
    if cap >= m.n:
        assert np.array_equal(got, m.keys)
    else:
        assert len(np.unique(got)) == n and np.isin(got, m.keys).all()   # distinct members of the candidate set
    assert tiles.shape == m.lo.shape and (tiles >= m.lo).all() and (tiles <= m.hi).all()
    lo, hi = m.spilled_range()
    assert lo <= spilled <= hi and spilled == int((tiles > C.SLOTS).sum())
    return got, tiles, spilled


def check_operators(vs, m, gray):
    for mc, q, md in PARAMS:
        exp = oracle.good_features(m.img, mc, q, md)
        for det in (vs.DETECTOR_AUTO, vs.DETECTOR_TWO_PASS):
            info = {}
            got = vs.good_features(gray, mc, q, md, detector=det, info=info)
            assert np.array_equal(got, exp), (mc, md, det)
            assert info["detector_used"] == (vs.DETECTOR_TWO_PASS if det == vs.DETECTOR_TWO_PASS else vs.DETECTOR_FUSED)


@pytest.mark.parametrize("name", list(C.SETS))
def test_raw_output_and_operators(vs, cuda, name):
    """Keys, keys kept, per-tile counts and tiles that spilled against the model (lo == hi pins a count; spilled tiles are pinned where no
    tile is `timing`), then both public detectors against the oracle."""
    m = C.model(name)
    g = dev(m.img, cuda)
    check_raw(vs, m, g)
    check_operators(vs, m, g)


def test_timing_tiles_three_runs_one_key_set(vs, cuda):
    """The frame whose tiles spill or not by timing, and the ramp whose middle tile has a negative maximum: whatever the tiles did, the keys
    are the model's, run after run."""
    for name in ("timing", "ramp_4"):
        m = C.model(name)
        assert m.timing.any()
        g = dev(m.img, cuda)
        runs = [check_raw(vs, m, g) for _ in range(3)]
        assert all(np.array_equal(r[0], runs[0][0]) for r in runs)
        print(name, "tiles that spilled per run:", [r[2] for r in runs])


@pytest.mark.parametrize("name", ["grid_5x3", "full_16", "cut_129x63"])
def test_unaligned_pitched_views(vs, cuda, name):
    """vec_ok = 0: a base that is not 4-byte aligned, an odd pitch"""
    m = C.model(name)
    assert m.spills.any() or m.full.all()
    v = unaligned_view(m.img, cuda)
    check_raw(vs, m, v)
    check_operators(vs, m, v)


@pytest.mark.parametrize("name", ["full_16", "grid_5x3", "cut_129x63"])
def test_key_buffer_cap(vs, cuda, name):
    """A key buffer of exactly n, n - 1 and 1 keys: the count is the whole n every time, the keys that fit are distinct candidates, and
    nothing is written behind the buffer.  full_16 appends per workgroup only; cut_129x63 per wave only (every tile spills); grid_5x3 both."""
    m = C.model(name)
    assert {"full_16": not m.spills.any(), "grid_5x3": m.spills.any() and m.keyed.any(), "cut_129x63": int(m.lo[m.keyed].sum()) == 0}[name]
    g = dev(m.img, cuda)
    for cap in (m.n, m.n - 1, 1):
        check_raw(vs, m, g, cap=cap)


def test_public_operator_at_the_key_capacity(vs, cuda):
    """Exactly 2^18 candidates fit the key buffer of a fresh Detector: the fused detector's corners.  One more: the two-pass detector's."""
    for which, used in (("2^18", vs.DETECTOR_FUSED), ("2^18+1", vs.DETECTOR_TWO_PASS)):
        img = C.cap_frame(which)
        g = dev(img, cuda)
        for mc, q, md in PARAMS:
            info = {}
            got = vs.good_features(g, mc, q, md, detector=vs.DETECTOR_AUTO, info=info)
            assert info["detector_used"] == used, which
            assert np.array_equal(got, oracle.good_features(img, mc, q, md)), (which, mc)
        m = C.Model(img)
        assert m.n == C.KEY_CAP + (which != "2^18")
        check_raw(vs, m, g, cap=C.KEY_CAP)


def test_min_eig_bits(vs, cuda):
    """vstab_min_eig on rounding-noise eigenvalues (ramps: negative and positive zeros' neighbours), stripes and the patch frames"""
    names = [f"ramp_{k}" for k in range(len(C.RAMPS))] + ["stripes_vertical", "stripes_horizontal", "stripes_diagonal", "tile_257", "grid_5x3", "grid_3x6",
                                                         "cut_66x33", "timing"]
    for name in names:
        m = C.model(name)
        for g in (dev(m.img, cuda), unaligned_view(m.img, cuda)):
            got = vs.min_eig(g).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), m.eig.view(np.uint32)), name


@pytest.mark.parametrize("which", ["under_spec_cap", "at_spec_cap", "over_spec_cap", "middle_320", "middle", "large"])
def test_pipeline_around_the_caps(vs, cuda, monkeypatch, which):
    """A handle on clips whose key frames hold fewer candidates than Detector::SPEC_CAP, exactly as many, one more, far more, and more than
    the key capacity: decisions, counts, rotations and every output frame are the oracle state machine's (the check of test_pipeline_gpu.py),
    and the handle's counters say which way the detections went."""
    import test_pipeline_gpu as P
    seen = {}
    run_product = P.run_product

    def spy(*a, **kw):
        seen["stab"], outs = run_product(*a, **kw)
        return seen["stab"], outs

    monkeypatch.setattr(P, "run_product", spy)
    (w, h), frames = C.pipeline_clip(which)
    K = oracle.get_preset_camera(4, w, h)
    log = P._check_against_oracle_state_machine(vs, cuda, frames, K, w, h, 2, 9)
    stab = seen["stab"]
    c, prof = stab.detector_counters(), stab.profile()
    selections = prof["corner_selections_by_caller"] + prof["corner_selections_by_helper"]
    keys = [k for k, l in enumerate(log) if l["key"]]
    print(which, "key frames", keys, "counters", c, "selections", selections)
    if which == "large":
        # the seed detection found more than 2^18 candidates: it overflowed the fused detector, and the two-pass detector grew the capacity
        # to their count; the key frames among the textured frames behind it are detected by the fused detector as ever
        assert c["fused_overflows"] == 1 and c["key_capacity"] == 302736 and c["spec_over_cap"] == 0
        assert keys == [4, 5, 6]
        return
    assert c["fused_overflows"] == 0 and c["key_capacity"] == C.KEY_CAP
    if which == "middle_320":
        assert keys == list(range(24)) and selections == 0 and c["spec_over_cap"] == 0      # 78 corners: every frame a key frame, never planned
        return
    assert keys == [20] and selections == 1                                              # the counter's key frame, detected ahead of time
    assert c["spec_over_cap"] == (0 if which in ("under_spec_cap", "at_spec_cap") else 1)
