"""The refusals of the pipeline object that are made before anything touches a device or a handle, as tables: every check of vstab_create
from the null-argument check down to read_ahead (status, the whole vstab_last_error() text, the handle pointer left null; calls that break
two checks at once pin the order: the earlier check's message wins), and the null-argument refusals of the pull entry points, of
vstab_set_border_mode / _ex and of the profile / info getters.  Handles that are "not null" here are a dummy address that a refused call
never dereferences, so the tables run without a GPU."""
import ctypes
import math

import pytest

P = 4096  # a non-null dummy address
ABI = 0x56534206
CUBIC, LANCZOS4 = 2, 4

C = "vstab_create: "
ABI_TEXT = (C + "vstab_config.abi_version is %d, this library is version " + str(ABI) +
            ": initialise the struct with vstab_config_default() of THIS library (include/vstab.h)")
INTERPOLATION = C + "interpolation must be INTER_LINEAR (1, the only mode the reference passes) or INTER_NEAREST (0)"
NEAREST = C + "INTER_NEAREST exists for the reference's own map (lens_mode 0, 8-bit pixels)"
RESAMPLE = C + "resample must be VSTAB_RESAMPLE_DEFAULT (0), VSTAB_RESAMPLE_CUBIC (2) or VSTAB_RESAMPLE_LANCZOS4 (4)"
NEEDS = C + "VSTAB_RESAMPLE_%s needs interpolation = INTER_LINEAR (1) and 8-bit pixels"
SCALE = C + "scale and zoom must be positive"
READ_AHEAD = C + "read_ahead must be 0 (the default, 12) or 1 .. 16"

# vstab_config fields that differ from vstab_config_default() -> the whole message, in the order of vstab_create's checks; rows that
# break two checks carry the message of the earlier one
CREATE_ROWS = [
    (dict(abi_version=0), ABI_TEXT % 0),
    (dict(abi_version=ABI - 1), ABI_TEXT % (ABI - 1)),
    (dict(abi_version=ABI + 1, smooth_radius=-1), ABI_TEXT % (ABI + 1)),
    (dict(smooth_radius=-1), C + "bad smooth_radius"),
    (dict(smooth_radius=10001), C + "bad smooth_radius"),
    (dict(smooth_radius=10001, interpolation=2), C + "bad smooth_radius"),
    (dict(interpolation=2), INTERPOLATION),
    (dict(interpolation=-1), INTERPOLATION),
    (dict(interpolation=4, resample=1), INTERPOLATION),
    (dict(interpolation=0, lens_mode=1), NEAREST),
    (dict(interpolation=0, pixel_depth=10), NEAREST),
    (dict(interpolation=0, lens_mode=2), NEAREST),
    (dict(interpolation=0, pixel_depth=10, resample=3), NEAREST),
    (dict(resample=1), RESAMPLE),
    (dict(resample=3), RESAMPLE),
    (dict(resample=5), RESAMPLE),
    (dict(resample=-1), RESAMPLE),
    (dict(resample=1, scale=0.0), RESAMPLE),
    (dict(resample=CUBIC, interpolation=0), NEEDS % "CUBIC"),
    (dict(resample=CUBIC, pixel_depth=10), NEEDS % "CUBIC"),
    (dict(resample=CUBIC, pixel_depth=10, zoom=0.0), NEEDS % "CUBIC"),
    (dict(resample=LANCZOS4, interpolation=0), NEEDS % "LANCZOS4"),
    (dict(resample=LANCZOS4, pixel_depth=10), NEEDS % "LANCZOS4"),
    (dict(resample=LANCZOS4, pixel_depth=10, smoother=9), NEEDS % "LANCZOS4"),
    (dict(scale=0.0), SCALE),
    (dict(scale=-1.0), SCALE),
    (dict(scale=math.nan), SCALE),
    (dict(zoom=0.0), SCALE),
    (dict(zoom=-0.5), SCALE),
    (dict(zoom=math.nan), SCALE),
    (dict(zoom=0.0, smoother=4), SCALE),
    (dict(smoother=-1), C + "unknown smoother"),
    (dict(smoother=4), C + "unknown smoother"),
    (dict(smoother=4, lens_mode=2), C + "unknown smoother"),
    (dict(lens_mode=2), C + "lens_mode must be 0 or 1"),
    (dict(lens_mode=-1), C + "lens_mode must be 0 or 1"),
    (dict(lens_mode=2, pixel_depth=9), C + "lens_mode must be 0 or 1"),
    (dict(pixel_depth=9), C + "pixel_depth must be 8 or 10"),
    (dict(pixel_depth=12), C + "pixel_depth must be 8 or 10"),
    (dict(pixel_depth=-8), C + "pixel_depth must be 8 or 10"),
    (dict(pixel_depth=16, blend=2), C + "pixel_depth must be 8 or 10"),
    (dict(blend=2), C + "unknown blend"),
    (dict(blend=-1), C + "unknown blend"),
    (dict(blend=2, map_precision=2), C + "unknown blend"),
    (dict(map_precision=2), C + "unknown map_precision"),
    (dict(map_precision=-1), C + "unknown map_precision"),
    (dict(map_precision=2, read_ahead=17), C + "unknown map_precision"),
    (dict(read_ahead=-1), READ_AHEAD),
    (dict(read_ahead=17), READ_AHEAD),
    (dict(read_ahead=-1, pixel_depth=10, lens_mode=1, tracking=0), READ_AHEAD),
]


@pytest.fixture(scope="module")
def source(vs):
    """A vstab_source whose callbacks are never called: every call of this file is refused before upstream is asked for a frame."""
    called = []
    cb = vs.PULL_FN(lambda user, out: called.append(1) or vs.EOF)
    yield vs.Source(cb, cb, None)
    assert not called


def test_the_library_is_the_version_the_table_was_written_for(vs):
    assert vs.lib.vstab_abi_version() == ABI


@pytest.mark.parametrize("row", range(len(CREATE_ROWS)))
def test_create_refuses_a_bad_config_before_its_first_device_call(vs, source, row):
    bad, text = CREATE_ROWS[row]
    cfg = vs.default_config(**bad)
    h = ctypes.c_void_p()
    got = vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(source), ctypes.byref(h))
    assert got == vs.ERR_INVALID, (bad, got, vs.lib.vstab_last_error())
    assert vs.lib.vstab_last_error() == text.encode(), bad
    assert h.value is None, bad


def test_create_refuses_null_arguments_first(vs, source):
    L = vs.lib
    cb = source.pull
    bad_cfg = vs.default_config(abi_version=0, smooth_radius=-1)      # its own refusals come after the null check
    for good in (vs.default_config(), bad_cfg):
        h = ctypes.c_void_p()
        for cfg, src, out in ((None, ctypes.byref(source), ctypes.byref(h)), (ctypes.byref(good), None, ctypes.byref(h)),
                              (ctypes.byref(good), ctypes.byref(source), None),
                              (ctypes.byref(good), ctypes.byref(vs.Source(vs.PULL_FN(), cb, None)), ctypes.byref(h)),
                              (ctypes.byref(good), ctypes.byref(vs.Source(cb, vs.PULL_FN(), None)), ctypes.byref(h))):
            assert L.vstab_create(cfg, src, out) == vs.ERR_INVALID
            assert L.vstab_last_error() == b"vstab_create: null argument"
            assert h.value is None


# entry point, arguments, message: refused on the arguments alone (a non-null handle is the dummy address, never dereferenced)
PULL_NULL = "vstab_pull_frame: null argument"
NULL_ROWS = [
    ("vstab_pull_frame", (None, P, 64), PULL_NULL),
    ("vstab_pull_frame", (P, None, 64), PULL_NULL),
    ("vstab_pull_frame", (None, None, 0), PULL_NULL),
    ("vstab_peek_frame", (None, P, 64), PULL_NULL),
    ("vstab_peek_frame", (P, None, 64), PULL_NULL),
    ("vstab_pull_frame_bgr16", (None, P, 64), PULL_NULL),
    ("vstab_pull_frame_bgr16", (P, None, 64), PULL_NULL),
    ("vstab_pull_frame_nv12", (None, P, 64, P, 64), PULL_NULL),
    ("vstab_pull_frame_nv12", (P, None, 64, P, 64), PULL_NULL),
    ("vstab_pull_frame_nv12", (P, P, 64, None, 64), PULL_NULL),
    ("vstab_pull_frame_nv12_planar", (None, P, 64, P, 64), PULL_NULL),
    ("vstab_pull_frame_nv12_planar", (P, None, 64, P, 64), PULL_NULL),
    ("vstab_pull_frame_nv12_planar", (P, P, 64, None, 64), PULL_NULL),
    ("vstab_pull_frame_p010_planar", (None, P, 64, P, 64), PULL_NULL),
    ("vstab_pull_frame_p010_planar", (P, None, 64, P, 64), PULL_NULL),
    ("vstab_pull_frame_p010_planar", (P, P, 64, None, 64), PULL_NULL),
    ("vstab_pull_frame_p010", (None, P, 64, P, 64), "vstab_pull_frame_p010: null argument"),
    ("vstab_pull_frame_p010", (P, None, 64, P, 64), "vstab_pull_frame_p010: null argument"),
    ("vstab_pull_frame_p010", (P, P, 64, None, 64), "vstab_pull_frame_p010: null argument"),
    ("vstab_pull_frame_host", (None, P, 64), "vstab_pull_frame_host: bad argument"),
    ("vstab_pull_frame_host", (P, None, 64), "vstab_pull_frame_host: bad argument"),
    ("vstab_set_border_mode", (None, 0), "vstab_set_border_mode: null handle"),
    ("vstab_set_border_mode", (None, 3), "vstab_set_border_mode: null handle"),
    ("vstab_set_border_mode_ex", (None, 0), "vstab_set_border_mode_ex: null handle"),
    ("vstab_set_border_mode_ex", (None, 3), "vstab_set_border_mode_ex: null handle"),
    ("vstab_get_output_info", (None, None, None, None, None), "null handle"),
    ("vstab_enable_profiling", (None, 1), "null handle"),
]


@pytest.mark.parametrize("row", range(len(NULL_ROWS)))
def test_entry_points_refuse_null_arguments_before_touching_a_handle(vs, row):
    fn, args, text = NULL_ROWS[row]
    got = getattr(vs.lib, fn)(*args)
    assert got == vs.ERR_INVALID, (fn, args, got, vs.lib.vstab_last_error())
    assert vs.lib.vstab_last_error() == text.encode(), (fn, args)


def test_get_profile_refuses_null_arguments(vs):
    prof = vs.Profile()
    for args in ((None, ctypes.byref(prof)), (P, None), (None, None)):
        assert vs.lib.vstab_get_profile(*args) == vs.ERR_INVALID
        assert vs.lib.vstab_last_error() == b"vstab_get_profile: null argument"


def test_pull_frames_refuses_bad_arguments_and_reports_no_frame_done(vs):
    L = vs.lib
    dst, pitch = (ctypes.c_void_p * 2)(P, P), (ctypes.c_size_t * 2)(64, 64)
    good = dict(h=P, n=1, dst=dst, pitch_dst=pitch, n_dst=2, first=0)
    for bad in (dict(h=None), dict(dst=None), dict(pitch_dst=None), dict(n=-1), dict(n_dst=0), dict(n_dst=-2), dict(first=-1), dict(h=None, n=-1)):
        done = ctypes.c_int(7)
        assert L.vstab_pull_frames(*dict(good, **bad).values(), ctypes.byref(done)) == vs.ERR_INVALID, bad
        assert L.vstab_last_error() == b"vstab_pull_frames: bad argument", bad
        assert done.value == 0, bad
        assert L.vstab_pull_frames(*dict(good, **bad).values(), None) == vs.ERR_INVALID, bad   # n_done is optional
    done = ctypes.c_int(7)
    assert L.vstab_pull_frames(*dict(good, n=0).values(), ctypes.byref(done)) == vs.OK         # no frame asked for: the handle is not touched
    assert done.value == 0
