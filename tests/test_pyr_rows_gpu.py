"""k_pyr_down's interior body on every case of tests/pyr_rows.py: the source placed with the case's base offset and pitch among junk bytes,
the level in a fenced plane (pyr_paths.Fenced) with the case's layout, every byte equal to pyr_paths.pyr_down_ref and every fence byte
intact.  Which case reaches which path is asserted in test_pyr_rows_cpu.py; a test id here is the case's id there.

Content: random bytes; 0 / 255 bytes (pyr_paths.content's "extreme"); and 255 everywhere, where every 16-bit half of the vertical pass holds
255 * 256 + 128 = 65408 -- the largest value there is, one bit below a carry into the neighbouring half."""
import functools

import numpy as np
import pytest

import pyr_paths as pp
import pyr_rows as pr

pytestmark = pytest.mark.gpu

KINDS = ("random", "extreme", "white")


@functools.lru_cache(maxsize=None)
def _level(kind, w, h):
    """-> (image, its first level by the definition); computed once, read-only."""
    img = np.full((h, w), 255, np.uint8) if kind == "white" else pp.content(kind, 11 * w + h, w, h)
    e1 = pp.pyr_down_ref(img)
    if kind == "white":
        assert (e1 == 255).all()
    img.setflags(write=False)
    e1.setflags(write=False)
    return img, e1


def _down(vs, cuda, c, kind):
    img, e1 = _level(kind, c.sw, c.sh)
    buf, v = pp.place(img, cuda, *c.src)
    assert v.data_ptr() % 16 == c.src[0] and v.stride(0) == c.src[1]
    out = pp.Fenced(e1.shape[0], e1.shape[1], cuda, *c.dst)
    r = vs.pyr_down(v, out=out.view())
    assert r.data_ptr() == out.ptr and out.ptr % 16 == c.dst[0] and r.stride(0) == c.dst[1]
    got = out.host()
    if not np.array_equal(got, e1):
        bad = np.argwhere(got != e1)
        raise AssertionError(f"{c.id} {kind}: {len(bad)} of {e1.size} bytes differ, the first at (row, column) {bad[0].tolist()}: "
                             f"{int(got[tuple(bad[0])])} for {int(e1[tuple(bad[0])])}; rows that differ: {sorted(set(bad[:, 0].tolist()))[:12]}")
    assert np.array_equal(v.cpu().numpy(), img), (c.id, kind, "the source changed")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", pr.ROWS_CASES, ids=lambda c: c.id)
def test_pyr_down_row_groups(vs, cuda, c, kind):
    _down(vs, cuda, c, kind)
