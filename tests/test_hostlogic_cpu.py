"""CPU tests of the pipeline's host-side bookkeeping with hand-made buffers, through the library's vstabx_* test hooks
(video-annotator_amd/csrc/vstab_hostlogic.hpp): the parser of the tracker's result records (what Tracker::track_wait runs on
the records k_lk_track writes into mapped host memory) and the DMA-BUF import cache (resolve_dmabuf).  No device needed -- these
are the parts of the pipeline's host code that the sanitizer build (tools/run_sanitized_tests.sh) could not reach otherwise."""
import ctypes

import numpy as np
import pytest

OK, NOT_READY, BAD_CHAIN, COUNT_MISMATCH = 0, 1, -1, -2


@pytest.fixture(scope="module")
def hooks(vs):
    L = vs.lib
    u32p, f32p, u8p, ip = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int)
    L.vstabx_parse_records.restype = ctypes.c_int
    L.vstabx_parse_records.argtypes = [u32p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, f32p, u8p, ip, ip]
    L.vstabx_dmabuf_cache_sim.restype = ctypes.c_int
    L.vstabx_dmabuf_cache_sim.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_longlong, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_ulonglong)]
    return L


def records(points, statuses, seq):
    """n records as k_lk_track's make_record lays them out: {x bits, seq, y bits, seq << 2 | status}."""
    rec = np.zeros((len(statuses), 4), np.uint32)
    rec[:, 0] = np.asarray(points, np.float32)[:, 0].view(np.uint32)
    rec[:, 2] = np.asarray(points, np.float32)[:, 1].view(np.uint32)
    rec[:, 1] = seq
    rec[:, 3] = (np.uint64(seq) << np.uint64(2)).astype(np.uint32) | np.asarray(statuses, np.uint32)
    return rec


def parse(hooks, rec, seq, expect_n):
    n = len(rec)
    rec = np.ascontiguousarray(rec, np.uint32)
    xy, st = np.full(2 * n + 2, np.nan, np.float32), np.full(n + 1, 255, np.uint8)
    n_out, nxt = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = hooks.vstabx_parse_records(rec.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, seq, expect_n, xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    st.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), ctypes.byref(n_out), ctypes.byref(nxt))
    return rc, xy[:2 * n_out.value].reshape(-1, 2), st[:n_out.value], nxt.value


def test_record_parser_compacts_the_point_list(hooks):
    """Status 1 / 0 entries are this frame's point list in slot order (FrameSourceWarp.cpp:261-268 filters on status afterwards),
    status 2 ("lost in an earlier frame of the chain") is skipped, and the count must be the number of points that went in."""
    rng = np.random.default_rng(1)
    for seq in (1, 7, 0x3fffffff, 0x40000001, 0xfffffffe):          # the status word keeps 30 bits of the tag: wrap-around included
        n = 200
        pts = rng.uniform(-50, 4000, (n, 2)).astype(np.float32)
        st = rng.choice([0, 1, 1, 1, 2], n)
        rec = records(pts, st, seq)
        live = st != 2
        rc, xy, out_st, nxt = parse(hooks, rec, seq, int(live.sum()))
        assert rc == OK and nxt == n
        assert np.array_equal(xy.view(np.uint32), pts[live].view(np.uint32)) and np.array_equal(out_st, st[live])
        # the bookkeeping check: another expectation is an error, never a silently shorter list
        assert parse(hooks, rec, seq, int(live.sum()) + 1)[0] == COUNT_MISMATCH
    assert parse(hooks, np.zeros((0, 4), np.uint32), 5, 0)[0] == OK


def test_record_parser_never_pairs_a_new_tag_with_stale_data(hooks):
    """A record is valid only when BOTH of its 8-byte granules carry the launch's tag: a record of an older launch, a record whose
    second half has not landed yet (nothing promises that the 16-byte store arrives as one write) and a never-written record
    (tag 0) all read as "not ready", at the right index, with everything before them decoded."""
    pts = np.arange(20, dtype=np.float32).reshape(10, 2)
    seq = 41
    for torn_at in (0, 3, 9):
        for kind in ("old launch", "first half only", "second half only", "never written"):
            rec = records(pts, np.ones(10, int), seq)
            if kind == "old launch":
                rec[torn_at] = records(pts[torn_at:torn_at + 1] + 100, [1], seq - 1)[0]
            elif kind == "first half only":
                rec[torn_at, 3] = ((seq - 1) << 2) | 1            # {x, seq} new, {y, tag} still the previous launch's
            elif kind == "second half only":
                rec[torn_at, 1] = seq - 1
            else:
                rec[torn_at] = 0
            rc, xy, st, nxt = parse(hooks, rec, seq, 10)
            assert rc == NOT_READY and nxt == torn_at, (torn_at, kind)
            assert np.array_equal(xy, pts[:torn_at]) and len(st) == torn_at
    # a chained slot whose parent record carried another tag reports status 3: an error, not a lost feature
    rec = records(pts, [1, 1, 3, 1, 1, 1, 1, 1, 1, 1], seq)
    assert parse(hooks, rec, seq, 10)[0] == BAD_CHAIN


def sim(hooks, ids, cap, window, sizes=None, fail_id=-1):
    ids = np.ascontiguousarray(ids, np.uint64)
    counts = (ctypes.c_long * 6)()
    bases = np.zeros(len(ids), np.uint64)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.uintp)
    fails = hooks.vstabx_dmabuf_cache_sim(ids.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)),
                                          None if sz is None else sz.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), len(ids), cap, window, fail_id, counts,
                                          bases.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
    imports, evictions, cached, destroys, peak, destroys_after_clear = counts
    return dict(fails=fails, imports=imports, evictions=evictions, cached=cached, destroys=destroys, peak=peak, destroys_total=destroys_after_clear, bases=bases)


def test_dmabuf_cache_imports_each_object_once_and_returns_its_own_mapping(hooks):
    pool = np.arange(100, 140)                        # a decoder's pool of 40 surfaces, handed round and round
    r = sim(hooks, np.tile(pool, 10), cap=256, window=20)
    assert (r["imports"], r["evictions"], r["cached"], r["fails"]) == (40, 0, 40, 0)
    assert np.array_equal(r["bases"], np.tile(pool, 10) * 4096)          # every lookup got the mapping of ITS object
    assert r["destroys_total"] == 40                                     # all released with the handle
    # same inode, another size = another object (a descriptor number reused for a differently sized surface)
    r = sim(hooks, [7, 7, 7, 7], cap=4, window=0, sizes=[4096, 8192, 4096, 8192])
    assert (r["imports"], r["cached"]) == (2, 2)


def test_dmabuf_cache_evicts_least_recently_used_but_never_inside_the_window(hooks):
    """More objects than the cache holds: the least recently used one is unmapped and imported again when its turn comes -- unless it
    was used within the last `window` lookups (a frame of the look-ahead window may still be read in place): then the cache grows."""
    pool = np.arange(1, 31)                           # 30 objects, cap 4, frames live for 20 lookups
    seq = np.tile(pool, 5)
    r = sim(hooks, seq, cap=4, window=20)
    assert r["fails"] == 0 and np.array_equal(r["bases"], seq * 4096)
    assert r["peak"] == 22 and r["cached"] == 22      # settles at window + 2 objects, not at 4 and not at 30
    assert r["imports"] == len(seq) and r["evictions"] == r["imports"] - r["cached"] == r["destroys"]
    assert r["destroys_total"] == r["imports"]        # nothing mapped is ever forgotten
    # a window of 0 (nothing in flight) keeps exactly `cap` objects; a hot object survives while cold ones rotate
    seq = np.array([1, 2, 3, 4] + [1, 5, 1, 6, 1, 7, 1, 8] * 3)
    r = sim(hooks, seq, cap=4, window=0)
    assert r["peak"] == 4 and np.array_equal(r["bases"], seq * 4096)
    assert r["imports"] == 4 + 4 * 3 and r["evictions"] == r["imports"] - 4      # object 1 was imported once
    # a failing import is reported, caches nothing, and the next attempt imports again
    r = sim(hooks, [1, 2, 9, 9, 3], cap=8, window=0, fail_id=9)
    assert (r["fails"], r["imports"], r["cached"]) == (2, 3, 3) and list(r["bases"][[2, 3]]) == [2 ** 64 - 1] * 2
