"""GPU tests of the LK tracker's multi-pair launches (k_lk_track with fi > 0) and chained launches, through the test hook
vstabx_lk_segments: the records of every pair of every slot against the oracle chained over the surviving slots (tests/lk_segments.py),
under several segmentations; the chain statuses; pitched / unaligned frames; 1 to 257 slots; a 4K bench-shaped launch; and k_pack_pyr
(the ring copy and pyramid level 1 in one launch) against oracle.pack_nv12 / oracle.pyr_down."""
import numpy as np
import pytest

import lk_segments as M
import oracle

pytestmark = pytest.mark.gpu


def _dev(frames, cuda):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(f)).to(cuda) for f in frames]


def _segmentations(K):
    return [[8], [1] * 8, [3, 5]] if K == 8 else [[8, 8, 2]]


def check_records(exp, hrec, drec, what):
    """status bytes as the oracle's; x / y bits of status 1 as the oracle's; status 2 / 3 at (0, 0); both tags = the pair's sequence
    number (the hook's tracker numbers pairs 1, 2, ...); host copy == device copy."""
    K, n = exp["status"].shape
    assert hrec.shape == (K, n, 4)
    assert np.array_equal(hrec, drec), (what, "host and device records differ")
    seq = np.arange(1, K + 1, dtype=np.uint32)[:, None]
    assert np.array_equal(hrec[..., 1], np.broadcast_to(seq, (K, n))), what
    assert np.array_equal(hrec[..., 3] >> 2, np.broadcast_to(seq, (K, n))), what
    st = hrec[..., 3] & 3
    bad = np.argwhere(st != exp["status"])
    assert bad.size == 0, (what, "status", bad[:5], st[tuple(bad[0])], exp["status"][tuple(bad[0])])
    one = exp["status"] == 1
    xy = hrec[..., [0, 2]]
    ebits = exp["xy"].view(np.uint32)
    bad = np.argwhere(one[..., None] & (xy != ebits))
    assert bad.size == 0, (what, "x / y bits", bad[:5], xy.view(np.float32)[tuple(bad[0][:2])], exp["xy"][tuple(bad[0][:2])])
    dead = (exp["status"] == 2) | (exp["status"] == 3)
    assert not (dead[..., None] & (xy != 0)).any(), what


def run_set(vs, cuda, name, n=None):
    frames, pts, _ = M.make_set(name, n)
    K = len(frames) - 1
    exp = M.expected(frames, pts, [K])
    df = _dev(frames, cuda)
    recs = []
    for segs in _segmentations(K):
        hrec, drec, _ = vs.lk_segments(df, pts, segs)
        check_records(exp, hrec, drec, (name, segs))
        recs.append(hrec)
    for r in recs[1:]:   # segment invariance: status-0 positions included
        assert np.array_equal(r, recs[0]), name
    return frames, df, pts, exp, recs[0]


@pytest.mark.parametrize("name", list(M.SETS))
def test_sets_under_every_segmentation(vs, cuda, name):
    """Every scripted set (tests/lk_segments.py: steady, jumping, coarse-blind, drifting across the border, going flat, leaving by
    the last step; 1- to 4-level pyramids, 333 x 181) as one launch of 8, eight chained launches of 1 and [3, 5] (the 18-pair set as
    [8, 8, 2]): the records of every pair equal the oracle's and each other; and equal vstab_pyr_lk run pair by pair (Tracker::track,
    one pair per launch) on the slots still alive, status-0 positions included."""
    frames, df, pts, exp, rec = run_set(vs, cuda, name)
    for k in range(len(frames) - 1):
        alive = np.flatnonzero(~np.isnan(exp["start"][k, :, 0]))
        if not alive.size:
            continue
        nxt, st = vs.pyr_lk(df[k], df[k + 1], exp["start"][k, alive])
        assert np.array_equal(st, rec[k, alive, 3] & 3), (name, k)
        assert np.array_equal(nxt.view(np.uint32), rec[k][alive][:, [0, 2]]), (name, k)


def test_chain_statuses(vs, cuda):
    """A chained launch handed a wrong parent tag reports status 3 for every pair of every slot; a launch chained behind a status-3
    record keeps reporting 3.  The launches before it are untouched."""
    frames, pts, _ = M.make_set("drift_240")
    df = _dev(frames, cuda)
    for segs, bad in (([3, 5], 1), ([2, 3, 3], 1), ([1] * 8, 7), ([4, 2, 2], 2)):
        exp = M.expected(frames, pts, segs, bad_parent=bad)
        hrec, drec, _ = vs.lk_segments(df, pts, segs, bad_parent=bad)
        check_records(exp, hrec, drec, (segs, bad))
        first = sum(segs[:bad])
        assert (hrec[first:, :, 3] & 3 == 3).all() and (hrec[:first, :, 3] & 3 != 3).all()


def test_pitched_unaligned_frames_and_slot_counts(vs, cuda):
    """Level-0 frames as views with pitch > width and a base 3 bytes past an aligned one (every pyramid kernel takes its byte paths)
    give the records of contiguous frames; 1, 200 and 257 slots (257: more workgroups than the pipeline's 200 and than one record
    buffer of init() holds)."""
    import torch
    for name in ("steady_640", "drift_y_333"):
        frames, pts, _ = M.make_set(name)
        K = len(frames) - 1
        exp = M.expected(frames, pts, [K])
        h, w = frames[0].shape
        views = []
        for f in frames:
            big = torch.zeros((h + 2, w + 45), dtype=torch.uint8, device=cuda)
            big[1:h + 1, 3:w + 3] = torch.from_numpy(f).to(cuda)
            views.append(big[1:h + 1, 3:w + 3])
        for segs in ([8], [3, 5]):
            hrec, drec, _ = vs.lk_segments(views, pts, segs)
            check_records(exp, hrec, drec, (name, "pitched", segs))
    frames, _, _ = M.make_set("jump_640")
    df = _dev(frames, cuda)
    for n in (1, 257):
        pts = M.start_points(frames[0], n, seed=3)
        exp = M.expected(frames, pts, [8])
        for segs in ([8], [3, 5]):
            hrec, drec, _ = vs.lk_segments(df, pts, segs)
            check_records(exp, hrec, drec, ("jump_640", n, segs))


def test_bench_shaped_launch(vs, cuda):
    """The bench's shape: 3840 x 2160, nine frames of bench.shaky_ring, 200 oracle corners of the first, one launch of 8 pairs."""
    import torch
    import bench
    w, h = 3840, 2160
    K = oracle.get_preset_camera(oracle.GOPRO_H4B_WIDE169_MEASURED, w, h)
    ring, _ = bench.shaky_ring(torch, cuda, w, h, K, 9, seed=2)
    df = [f[:h] for f in ring]
    frames = [f.cpu().numpy() for f in df]
    pts = oracle.good_features(frames[0], 200, 0.01, 30.0)
    assert pts.shape[0] == 200
    exp = M.expected(frames, pts, [8])
    hrec, drec, _ = vs.lk_segments(df, pts, [8])
    check_records(exp, hrec, drec, "4K")
    assert (exp["status"][-1] == 1).sum() >= 150


@pytest.mark.parametrize("case", ["w640_uv_vec", "w640_uv_pitch", "w264_uv_offset"])
def test_pack_pyr(vs, cuda, case):
    """k_pack_pyr as the pipeline's ingest uses it (a frame upstream recycles): the ring equals oracle.pack_nv12 of the luma and
    chroma views, the canary bytes behind the packed frame are untouched, level 1 equals oracle.pyr_down, the levels above it equal
    the pyramid the plain path builds, and tracking from the ring's luma gives the records of the plain path.  Widths with w % 16 of
    0 and 8; chroma aligned (16-byte copy path), with a pitch that is not a multiple of 16, and 3 bytes past an aligned base (byte
    path); the last case's rings 8 bytes past a 16-byte boundary."""
    import torch
    name = "drift_240" if case.startswith("w264") else "steady_640"
    frames, pts, _ = M.make_set(name)
    if case.startswith("w264"):
        frames = [np.ascontiguousarray(np.pad(f, ((0, 0), (0, 24)), mode="reflect")) for f in frames]
    h, w = frames[0].shape
    K = len(frames) - 1
    rng = np.random.default_rng(5)
    uvs = [rng.integers(0, 256, (h // 2, w), dtype=np.uint8) for _ in frames]
    uv_pitch, uv_off, ring_off = {"w640_uv_vec": (w, 0, 0), "w640_uv_pitch": (w + 20, 0, 0), "w264_uv_offset": (w + 16, 3, 8)}[case]
    ys, uvd, rings, ring_bufs = [], [], [], []
    nbytes = w * h * 3 // 2
    for f, u in zip(frames, uvs):
        ybig = torch.zeros((h, w + 64), dtype=torch.uint8, device=cuda)
        ybig[:, :w] = torch.from_numpy(f).to(cuda)
        ys.append(ybig[:, :w])
        ubig = torch.zeros((h // 2 * uv_pitch + uv_off + 64,), dtype=torch.uint8, device=cuda)
        uview = ubig[uv_off:uv_off + h // 2 * uv_pitch].view(h // 2, uv_pitch)[:, :w]
        uview.copy_(torch.from_numpy(u).to(cuda))
        uvd.append(uview)
        rb = torch.full((nbytes + ring_off + 256,), 0xA5, dtype=torch.uint8, device=cuda)
        ring_bufs.append(rb)
        rings.append(rb[ring_off:])
    hrec, drec, pyr = vs.lk_segments(ys, pts, [K], uv=uvd, rings=rings, want_pyr=True)
    plain_h, plain_d, plain_pyr = vs.lk_segments(_dev(frames, cuda), pts, [K], want_pyr=True)
    assert np.array_equal(hrec, plain_h) and np.array_equal(drec, plain_d), case
    check_records(M.expected(frames, pts, [K]), hrec, drec, case)
    assert np.array_equal(pyr, plain_pyr), case
    l1 = (w + 1) // 2 * ((h + 1) // 2)
    for i, (f, u) in enumerate(zip(frames, uvs)):
        rb = ring_bufs[i].cpu().numpy()
        assert np.array_equal(rb[ring_off:ring_off + nbytes].reshape(h * 3 // 2, w), oracle.pack_nv12(f, u)), (case, i)
        assert (rb[ring_off + nbytes:] == 0xA5).all() and (rb[:ring_off] == 0xA5).all(), (case, i, "canary")
        assert np.array_equal(pyr[i, :l1].reshape((h + 1) // 2, (w + 1) // 2), oracle.pyr_down(f)), (case, i)
