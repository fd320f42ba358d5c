"""The pyramid kernels on every case of tests/pyr_paths.py: the source placed with the case's base offset and pitch among junk bytes, every output
in a fenced plane (pyr_paths.Fenced) with the case's layout, all bytes equal to pyr_down_ref -- the second level to pyr_down_ref of the first --
and every fence byte intact.  Which case reaches which path is asserted in test_pyr_paths_cpu.py; a test id here is the case's id there.

  k_pyr_down     through vstab_pyr_down (vs.pyr_down with a caller's plane)
  k_pyr_down_x2  through vstab_pyr_down_x2, its fallback to two k_pyr_down launches included
  k_pack_pyr     through the hook vstabx_pack_pyr: ring == oracle.pack_nv12, level 1 == the reference, the hook's answer == the model's
                 pack_pyr_ok; refused planes are VSTAB_ERR_INVALID by launch_pack_pyr's own message and nothing is written
  two planes just under 4 GiB, one per kernel: a 144 x 84 source with the largest pitch the launchers accept, so that its last rows start
  just under 2^32 -- the 32-bit row products of both kernels at their limit.

Every table runs on random bytes and on 0 / 255 content (sums up to 255 * 256 + 128 in the dot products and the byte extraction)."""
import functools

import numpy as np
import pytest

import oracle
import pyr_paths as pp

pytestmark = pytest.mark.gpu

KINDS = ("random", "extreme")
SWEEP = [c for c in pp.DOWN_CASES if c.sw <= 24 and c.sh <= 6 and c.src == (0, c.sw) and c.dst == (0, (c.sw + 1) // 2)]
NAMED_DOWN = [c for c in pp.DOWN_CASES if c not in SWEEP]
assert len(SWEEP) == 24 * 6 and len(NAMED_DOWN) >= 30


@functools.lru_cache(maxsize=None)
def _levels(kind, w, h):
    """-> (image, its first level, its second level) by the definition; computed once, read-only."""
    img = pp.content(kind, 7 * w + h, w, h)
    e1 = pp.pyr_down_ref(img)
    e2 = pp.pyr_down_ref(e1)
    for a in (img, e1, e2):
        a.setflags(write=False)
    return img, e1, e2


def _same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {exp.size} bytes differ, the first at (row, column) {bad[0].tolist()}: "
                             f"{int(got[tuple(bad[0])])} for {int(exp[tuple(bad[0])])}")


def _down(vs, cuda, c, kind):
    img, e1, _ = _levels(kind, c.sw, c.sh)
    buf, v = pp.place(img, cuda, *c.src)
    assert v.data_ptr() % 16 == c.src[0] and v.stride(0) == c.src[1]
    out = pp.Fenced(e1.shape[0], e1.shape[1], cuda, *c.dst)
    r = vs.pyr_down(v, out=out.view())
    assert r.data_ptr() == out.ptr and out.ptr % 16 == c.dst[0] and r.stride(0) == c.dst[1]
    _same(out.host(), e1, (c.id, kind))
    _same(v.cpu().numpy(), img, (c.id, kind, "the source"))


def _x2(vs, cuda, c, kind):
    img, e1, e2 = _levels(kind, c.sw, c.sh)
    buf, v = pp.place(img, cuda, *c.src)
    mid = pp.Fenced(e1.shape[0], e1.shape[1], cuda, *c.mid)
    dst = pp.Fenced(e2.shape[0], e2.shape[1], cuda, *c.dst)
    m, d = vs.pyr_down_x2(v, out=(mid.view(), dst.view()))
    assert (m.data_ptr(), d.data_ptr()) == (mid.ptr, dst.ptr) and mid.ptr % 16 == c.mid[0] and dst.ptr % 16 == c.dst[0]
    _same(mid.host(), e1, (c.id, kind, "first level"))
    _same(dst.host(), e2, (c.id, kind, "second level"))
    _same(v.cpu().numpy(), img, (c.id, kind, "the source"))


@pytest.mark.parametrize("kind", KINDS)
def test_pyr_down_every_size_1_to_24_by_1_to_6(vs, cuda, kind):
    """The dense sweep of DOWN_CASES: widths 1 .. 4 (taps that leave the image twice), the far / near thresholds, every residue of dw."""
    for c in SWEEP:
        _down(vs, cuda, c, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", NAMED_DOWN, ids=lambda c: c.id)
def test_pyr_down_layouts_and_grids(vs, cuda, c, kind):
    _down(vs, cuda, c, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", pp.X2_CASES, ids=lambda c: c.id)
def test_pyr_down_x2_tiles_and_layouts(vs, cuda, c, kind):
    _x2(vs, cuda, c, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", pp.PACK_CASES, ids=lambda c: c.id)
def test_pack_pyr_copy_and_level_1(vs, cuda, c, kind):
    import torch
    w, h = c.sw, c.sh
    y, e1, _ = _levels(kind, w, h)
    uv = pp.content(kind, 3 * w + h + 1, w, max(h // 2, 1))[: h // 2]
    ybuf, yv = pp.place(y, cuda, *c.src)
    ubuf, uvv = pp.place(uv, cuda, *c.uv, seed=1) if h >= 2 else (None, yv)
    ring = pp.Fenced(h * 3 // 2, w, cuda, off=c.ring)
    l1 = pp.Fenced(e1.shape[0], e1.shape[1], cuda, *c.dst)
    args = (yv.data_ptr(), c.src[1], uvv.data_ptr(), c.uv[1], w, h, ring.ptr, l1.ptr, c.dst[1])
    st = vs.pack_pyr(*args)
    assert (st != -1) == pp.pack_ok(c), (c.id, st, "pack_pyr_ok differs from the model")
    if not pp.pack_ok(c):
        assert vs.pack_pyr(*args, launch_anyway=True) == vs.ERR_INVALID and vs.lib.vstab_last_error() == pp.MSG_PACK.encode(), c.id
        torch.cuda.synchronize()
        assert ring.untouched() and l1.untouched(), (c.id, "a refused call wrote something")
        return
    assert st == vs.OK, (c.id, st, vs.lib.vstab_last_error())
    _same(ring.host(), oracle.pack_nv12(y, uv), (c.id, kind, "ring"))
    _same(l1.host(), e1, (c.id, kind, "level 1"))
    _same(yv.cpu().numpy(), y, (c.id, kind, "the luma source"))


def _release():
    """Give a large buffer back to the device before the next one is allocated (the caller has dropped its references)."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("two", (False, True), ids=("k_pyr_down", "k_pyr_down_x2"))
def test_a_source_plane_just_under_4_gib(vs, cuda, two):
    """144 x 84 with pitch BIG_PITCH, the largest multiple of 4 with pitch * 84 < 2^32: the products row * pitch of both kernels' address
    arithmetic at the largest values the launchers let through (row 83 starts within one pitch of 2^32).  Only the rows are written; the
    outputs are fenced and 4-aligned, so the interior groups and the interior tile run."""
    import torch
    w, h, pitch = pp.BIG_W, pp.BIG_H, pp.BIG_PITCH
    assert pitch * h < pp.G4 <= (pitch + 4) * h and pitch * (h - 1) > pp.G4 - 2 * pitch
    img, e1, e2 = _levels("random", w, h)
    buf = torch.empty((pitch * (h - 1) + w + 64,), dtype=torch.uint8, device=cuda)
    try:
        assert buf.data_ptr() % 16 == 0
        v = torch.as_strided(buf, (h, w), (pitch, 1), 0)
        v.copy_(torch.from_numpy(np.array(img)))
        if two:
            mid, dst = pp.Fenced(e1.shape[0], e1.shape[1], cuda, 0, 76), pp.Fenced(e2.shape[0], e2.shape[1], cuda, 0, 40)
            vs.pyr_down_x2(v, out=(mid.view(), dst.view()))
            _same(mid.host(), e1, "first level")
            _same(dst.host(), e2, "second level")
        else:
            out = pp.Fenced(e1.shape[0], e1.shape[1], cuda, 0, 76)
            vs.pyr_down(v, out=out.view())
            _same(out.host(), e1, "level")
        _same(v.cpu().numpy(), img, "the source")
    finally:
        del buf
        v = None
        _release()


def test_without_out_the_binding_allocates_dense_levels_as_before(vs, cuda):
    img, e1, e2 = _levels("random", 70, 43)
    _, v = pp.place(img, cuda)
    a = vs.pyr_down(v)
    m, d = vs.pyr_down_x2(v)
    assert a.is_contiguous() and m.is_contiguous() and d.is_contiguous()
    _same(a.cpu().numpy(), e1, "pyr_down")
    _same(m.cpu().numpy(), e1, "pyr_down_x2 mid")
    _same(d.cpu().numpy(), e2, "pyr_down_x2 dst")


def test_a_refused_two_level_call_writes_nothing(vs, cuda):
    """Under 15 x 15 vstab_pyr_down_x2 is two k_pyr_down launches.  A second level of 4 GiB (4 rows of pitch 2^30; nothing of it is touched) is
    refused with launch_pyr_down's message before the FIRST launch: the first level, a real fenced plane here, stays as it was."""
    import torch
    img, e1, e2 = _levels("random", 14, 16)
    _, v = pp.place(img, cuda)
    mid, dst = pp.Fenced(e1.shape[0], e1.shape[1], cuda), pp.Fenced(e2.shape[0], e2.shape[1], cuda)
    st = vs.lib.vstab_pyr_down_x2(v.data_ptr(), v.stride(0), 14, 16, mid.ptr, mid.pitch, dst.ptr, pp.G4 // e2.shape[0], vs._stream())
    assert st == vs.ERR_INVALID and vs.lib.vstab_last_error() == pp.MSG_DOWN_4G.encode()
    torch.cuda.synchronize()
    assert mid.untouched() and dst.untouched()
    m, d = vs.pyr_down_x2(v, out=(mid.view(), dst.view()))      # and the same planes with their own pitch are written
    _same(mid.host(), e1, "first level")
    _same(dst.host(), e2, "second level")
