"""The refusals of the pull entry points and of vstab_set_border_mode / _ex that need a live handle: status and the whole
vstab_last_error() text, and what the refusal did to the stream.  A format refusal comes before any frame is dequeued: the same handle
next delivers the frame the oracle expects as its first, and every frame after it.  A frame the chosen warp cannot serve (a read-out
rotation on a CUBIC, LANCZOS4 or INTER_NEAREST handle; INTER_NEAREST pulled as NV12) is consumed by its refusal: the next pull delivers
the following frame.  Every refusal is provoked through the C API's argument paths; nothing here launches a kernel with bad arguments.
Small handles (640 x 360, tracking off: every frame is warped with the identity rotation, IEEE map arithmetic)."""
import ctypes

import numpy as np
import pytest

import expect
import oracle
import synth
import warp_def as wd

pytestmark = pytest.mark.gpu

W, H, N = 640, 360, 5
P = "vstab_pull_frame: "
SERVED = "8-bit BGR or plane-wise NV12 frames (vstab_pull_frame / _frames / _host / vstab_peek_frame / vstab_pull_frame_nv12_planar), not NV12 through BGR"
DEPTH = P + "a pixel_depth 10 handle emits through vstab_pull_frame_bgr16, an 8-bit handle through the others"
CUBIC_FMT = P + "VSTAB_RESAMPLE_CUBIC emits " + SERVED
LANCZOS4_FMT = P + "VSTAB_RESAMPLE_LANCZOS4 emits " + SERVED
BORDER_FMT = P + "a border mode other than VSTAB_BORDER_CONSTANT emits " + SERVED
NEAREST = "INTER_NEAREST emits 8-bit BGR frames without a read-out rotation"
READOUT = "VSTAB_RESAMPLE_%s warps frames without a read-out rotation (vstab_frame.readout_rotation)"
MODE = "%s: border_mode must be VSTAB_BORDER_CONSTANT (0), _REPLICATE (1), _REFLECT (2) or _REFLECT_101 (4)"
SET = ("vstab_set_border_mode: border modes other than VSTAB_BORDER_CONSTANT are served for 8-bit pixels with INTER_LINEAR (interpolation 1) "
       "and resample VSTAB_RESAMPLE_DEFAULT")
SET_EX = "vstab_set_border_mode_ex: border modes other than VSTAB_BORDER_CONSTANT are served for 8-bit pixels with INTER_LINEAR, INTER_CUBIC or INTER_LANCZOS4"
BASE = dict(smooth_radius=1, tracking=0, map_precision=expect.IEEE)


@pytest.fixture(scope="module")
def clip():
    K = oracle.get_preset_camera(4, W, H)
    Ko, (cw, ch) = oracle.get_output_camera(K, W, H)
    frames, _ = synth.shaky_clip(3, K, W, H, N, sigma=0.004)
    return K, Ko, cw, ch, frames


def wide_frames(frames):
    return [f.astype(np.uint16) << 8 for f in frames]


def handle(vs, cuda, frames, kind, **kw):
    import torch
    if kind == "p010":
        dev = [torch.from_numpy(x.view(np.int16)).to(cuda) for x in wide_frames(frames)]
        return vs.Stabilizer(dev, total=len(frames), bit_depth=10, pixel_depth=10, **dict(BASE, **kw))
    cfg = dict(linear={}, cubic=dict(resample=vs.RESAMPLE_CUBIC), lanczos4=dict(resample=vs.RESAMPLE_LANCZOS4), nearest=dict(interpolation=0))[kind]
    return vs.Stabilizer([torch.from_numpy(f).to(cuda) for f in frames], total=len(frames), **dict(BASE, **cfg, **kw))


def expected(clip, kind, k, border_mode=0):
    """Output for input frame k of a handle of this kind (tracking off: the identity rotation)."""
    K, Ko, cw, ch, frames = clip
    p = oracle.map_params(K, Ko, np.eye(3))
    if kind == "p010":
        w = wide_frames(frames)[k]
        return expect.warp_p010(w[:H], w[H:], p, cw, ch, None, 0, expect.IEEE)
    if kind == "cubic":
        return wd.bgr(frames[k], *wd.maps(p, cw, ch, 0), "cubic")
    if kind == "lanczos4":
        return wd.bgr(frames[k], *wd.maps(p, cw, ch, 0), "lanczos4")
    if border_mode:
        return wd.bgr(frames[k], *wd.maps(p, cw, ch, 0), "linear", border_mode)
    return expect.warp(frames[k], p, cw, ch, expect.IEEE, nearest=kind == "nearest")


def raw_pull(vs, cuda, h, how, cw, ch):
    """One call of the entry point `how` on the raw handle with good output buffers -> status."""
    import torch
    L = vs.lib
    wide = how in ("bgr16", "p010", "p010_planar")
    dt, bps = (torch.int16, 2) if wide else (torch.uint8, 1)
    if how in ("pull", "peek", "bgr16", "frames", "host"):
        o = torch.zeros((ch, cw, 3), dtype=dt, device=cuda)
        if how == "frames":
            done = ctypes.c_int(7)
            st = L.vstab_pull_frames(h, 1, (ctypes.c_void_p * 1)(o.data_ptr()), (ctypes.c_size_t * 1)(o.stride(0)), 1, 0, ctypes.byref(done))
            assert done.value == 0
            return st
        if how == "host":
            out = np.zeros((ch, cw, 3), np.uint8)
            return L.vstab_pull_frame_host(h, out.ctypes.data, out.strides[0])
        fn = dict(pull=L.vstab_pull_frame, peek=L.vstab_peek_frame, bgr16=L.vstab_pull_frame_bgr16)[how]
        return fn(h, o.data_ptr(), o.stride(0) * bps)
    y = torch.zeros((ch, cw), dtype=dt, device=cuda)
    uv = torch.zeros(((ch + 1) // 2, 2 * ((cw + 1) // 2)), dtype=dt, device=cuda)
    fn = dict(nv12=L.vstab_pull_frame_nv12, nv12_planar=L.vstab_pull_frame_nv12_planar, p010=L.vstab_pull_frame_p010,
              p010_planar=L.vstab_pull_frame_p010_planar)[how]
    return fn(h, y.data_ptr(), y.stride(0) * bps, uv.data_ptr(), uv.stride(0) * bps)


def refused(vs, st, status, text, what):
    assert st == status, (what, st, vs.lib.vstab_last_error())
    assert vs.lib.vstab_last_error() == text.encode(), what


def deliver(vs, cuda, stab, kind, cw, ch):
    import torch
    if kind == "p010":
        o = torch.empty((ch, cw, 3), dtype=torch.int16, device=cuda)
        return o.cpu().numpy().view(np.uint16) if stab.pull_bgr16_into(o) else None
    o = stab.pull()
    return None if o is None else o.cpu().numpy()


def rest_of_the_stream(vs, cuda, stab, clip, kind, first, border_mode=0):
    """The handle delivers input frames first .. N - 1, each as the oracle expects it, then the end of the stream."""
    _, _, cw, ch, _ = clip
    for k in range(first, N):
        o = deliver(vs, cuda, stab, kind, cw, ch)
        assert o is not None, (kind, k)
        assert np.array_equal(o, expected(clip, kind, k, border_mode)), (kind, k)
    assert deliver(vs, cuda, stab, kind, cw, ch) is None
    stab.close()


def test_depth_and_format_mismatch_is_refused_before_a_frame_is_dequeued(vs, cuda, clip):
    _, _, cw, ch, frames = clip
    stab = handle(vs, cuda, frames, "linear")
    for how in ("bgr16", "p010", "p010_planar"):
        refused(vs, raw_pull(vs, cuda, stab._h, how, cw, ch), vs.ERR_INVALID, DEPTH, how)
    rest_of_the_stream(vs, cuda, stab, clip, "linear", 1)
    stab = handle(vs, cuda, frames, "p010")
    for how in ("pull", "frames", "host", "peek", "nv12", "nv12_planar"):
        refused(vs, raw_pull(vs, cuda, stab._h, how, cw, ch), vs.ERR_INVALID, DEPTH, how)
    rest_of_the_stream(vs, cuda, stab, clip, "p010", 1)


@pytest.mark.parametrize("kind,border_mode,text", [("cubic", 0, CUBIC_FMT), ("lanczos4", 0, LANCZOS4_FMT), ("linear", 4, BORDER_FMT), ("linear", 1, BORDER_FMT),
                                                   ("cubic", 2, CUBIC_FMT), ("lanczos4", 4, LANCZOS4_FMT)],
                         ids=["cubic", "lanczos4", "reflect_101", "replicate", "cubic-reflect", "lanczos4-reflect_101"])
def test_resampler_and_border_handles_refuse_every_format_but_bgr8_and_planar_nv12(vs, cuda, clip, kind, border_mode, text):
    """NV12 through BGR gets the handle's own message (the resampler's before the border mode's); the 10-bit formats are refused by the
    depth check, which comes first.  BGR8 and plane-wise NV12 are the formats served: the stream that follows is pulled as BGR8."""
    _, _, cw, ch, frames = clip
    stab = handle(vs, cuda, frames, kind, **(dict(border_mode=border_mode) if border_mode else {}))
    refused(vs, raw_pull(vs, cuda, stab._h, "nv12", cw, ch), vs.ERR_INVALID, text, (kind, "nv12"))
    for how in ("bgr16", "p010", "p010_planar"):
        refused(vs, raw_pull(vs, cuda, stab._h, how, cw, ch), vs.ERR_INVALID, DEPTH, (kind, how))
    refused(vs, raw_pull(vs, cuda, stab._h, "nv12", cw, ch), vs.ERR_INVALID, text, (kind, "nv12 again"))
    if kind == "linear":
        rest_of_the_stream(vs, cuda, stab, clip, kind, 1, border_mode)
    else:   # (the border frames of the cubic and Lanczos warps have tests of their own: here the mode goes back to the constant border)
        assert vs.lib.vstab_set_border_mode_ex(stab._h, vs.BORDER_CONSTANT) == vs.OK
        rest_of_the_stream(vs, cuda, stab, clip, kind, 1)


@pytest.mark.parametrize("kind", ["linear", "cubic", "lanczos4", "nearest", "p010"])
def test_set_border_mode_refusals_leave_the_mode_as_it_was(vs, cuda, clip, kind):
    _, _, cw, ch, frames = clip
    L = vs.lib
    stab = handle(vs, cuda, frames, kind)
    for fn in ("vstab_set_border_mode", "vstab_set_border_mode_ex"):
        for bad in (3, 5, -1, 8, 16):   # an invalid mode is refused first, whatever the handle
            refused(vs, getattr(L, fn)(stab._h, bad), vs.ERR_INVALID, MODE % fn, (kind, fn, bad))
    for bm in (vs.BORDER_REPLICATE, vs.BORDER_REFLECT, vs.BORDER_REFLECT_101):
        if kind == "linear":
            assert L.vstab_set_border_mode(stab._h, bm) == vs.OK and L.vstab_set_border_mode_ex(stab._h, bm) == vs.OK
            continue
        refused(vs, L.vstab_set_border_mode(stab._h, bm), vs.ERR_UNSUPPORTED, SET, (kind, bm))
        if kind in ("cubic", "lanczos4"):   # _ex differs in its last term: it serves the resamplers
            assert L.vstab_set_border_mode_ex(stab._h, bm) == vs.OK
            assert L.vstab_set_border_mode_ex(stab._h, vs.BORDER_CONSTANT) == vs.OK
        else:
            refused(vs, L.vstab_set_border_mode_ex(stab._h, bm), vs.ERR_UNSUPPORTED, SET_EX, (kind, bm))
    assert L.vstab_set_border_mode(stab._h, vs.BORDER_CONSTANT) == vs.OK and L.vstab_set_border_mode_ex(stab._h, vs.BORDER_CONSTANT) == vs.OK
    if kind == "linear":
        assert L.vstab_set_border_mode(stab._h, vs.BORDER_REFLECT) == vs.OK
        refused(vs, L.vstab_set_border_mode(stab._h, 3), vs.ERR_INVALID, MODE % "vstab_set_border_mode", "mode kept")
        rest_of_the_stream(vs, cuda, stab, clip, kind, 1, vs.BORDER_REFLECT)   # the refused call changed nothing
    else:
        rest_of_the_stream(vs, cuda, stab, clip, kind, 1)                      # the constant border throughout


@pytest.mark.parametrize("how", ["nv12", "nv12_planar"])
def test_nearest_pulled_as_nv12_consumes_the_frame(vs, cuda, clip, how):
    _, _, cw, ch, frames = clip
    stab = handle(vs, cuda, frames, "nearest")
    refused(vs, raw_pull(vs, cuda, stab._h, how, cw, ch), vs.ERR_INVALID, NEAREST, how)
    rest_of_the_stream(vs, cuda, stab, clip, "nearest", 2)


@pytest.mark.parametrize("kind,text", [("cubic", READOUT % "CUBIC"), ("lanczos4", READOUT % "LANCZOS4"), ("nearest", NEAREST)], ids=["cubic", "lanczos4", "nearest"])
def test_a_readout_rotation_these_warps_cannot_serve_consumes_its_frame(vs, cuda, clip, kind, text):
    """Input frames 1 and 3 carry a vstab_frame.readout_rotation: their pulls are refused and take the frames with them; frames 2 and 4
    are delivered as the oracle expects them."""
    import torch
    _, _, cw, ch, frames = clip
    dev = [torch.from_numpy(f).to(cuda) for f in frames]
    ro = np.ascontiguousarray(oracle.rodrigues((0.002, -0.003, 0.001)), np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    state = {"i": 0}

    def fill(out, advance):
        i = state["i"]
        if i >= N:
            return vs.EOF
        t, o = dev[i], out.contents
        o.y, o.uv = t.data_ptr(), t.data_ptr() + H * t.stride(0)
        o.pitch_y = o.pitch_uv = t.stride(0)
        o.width, o.height, o.mem, o.pts, o.hold, o.bit_depth = W, H, 0, i, 1 << 30, 8
        o.readout_rotation = ro.ctypes.data_as(dp) if i in (1, 3) else None
        if advance:
            state["i"] += 1
        return 0
    pull, peek = vs.PULL_FN(lambda u, o: fill(o, True)), vs.PULL_FN(lambda u, o: fill(o, False))
    src = vs.Source(pull, peek, None)
    extra = dict(cubic=dict(resample=vs.RESAMPLE_CUBIC), lanczos4=dict(resample=vs.RESAMPLE_LANCZOS4), nearest=dict(interpolation=0))[kind]
    cfg = vs.default_config(**dict(BASE, **extra))
    h = ctypes.c_void_p()
    assert vs.lib.vstab_create(ctypes.byref(cfg), ctypes.byref(src), ctypes.byref(h)) == vs.OK, vs.lib.vstab_last_error()
    try:
        for k in range(1, N):
            o = torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda)
            st = vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0))
            if k in (1, 3):
                refused(vs, st, vs.ERR_INVALID, text, (kind, k))
            else:
                assert st == vs.OK, (kind, k, vs.lib.vstab_last_error())
                assert np.array_equal(o.cpu().numpy(), expected(clip, kind, k)), (kind, k)
        o = torch.zeros((ch, cw, 3), dtype=torch.uint8, device=cuda)
        assert vs.lib.vstab_pull_frame(h, o.data_ptr(), o.stride(0)) == vs.EOF
    finally:
        vs.lib.vstab_destroy(h)
