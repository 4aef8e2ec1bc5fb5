"""Temporal accumulation on the GPU (csrc/rtx_temporal.hip through rtx_temporal* and rtx_render_temporal*).

The kernel: against the float64 model of temporal_model.py on a synthetic pair of frames where every term decides
something, then the static camera's running mean, the first frame, the pixels that are not live, poisoned history,
determinism, the device entry between guard words, frame shapes and the argument errors.  The pipeline: a camera path
equals the three public calls chained by hand, bit for bit.  The geometry: a reprojected frame must come closer to the
moved camera's render than the frame it came from.  Quality: the accumulated frame against a 256-pass mean.
"""
import ctypes
import os

import numpy as np
import pytest

import conftest as C
import rtxpy
import temporal_model as TM
from rtxpy import abi

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (17, 33), (300, 2), (3, 70)]
SCENE_FILES = {"scene1": "scene1.json", "scene2": "scene2.json", "scene3": "scene3.json", "scenetest": "scenetest.json",
               "scene5_standin": "scene5_standin.json"}
PIPELINE = [("scene3", 128, 72, "ambient"), ("scene3", 128, 72, "path"), ("scene5_standin", 64, 40, "ambient"),
            ("scene5_standin", 64, 40, "path")]
TOL = 2e-5  # the upsampler test's bound and its reason: a fast exp's argument scaling, about e 2^-23 of a weight


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def render_params(gi, **kw):
    """ambient, or -g path -n 1"""
    return rtxpy.params_from_args(["-g", "path", "-n", "1"] if gi == "path" else [], **kw)


class World:
    """scenes and contexts, each made once and shared"""

    def __init__(self):
        self.scenes, self.ctx = {}, {}
        self.plain = None

    def scene(self, name):
        if name not in self.scenes:
            if "standin" in name:
                import standins
                standins.ensure_scene(name.split("_standin")[0])
            self.scenes[name] = rtxpy.Scene.load(os.path.join(C.SCENES, SCENE_FILES[name]), base_dir=C.GOLDEN)
        return self.scenes[name]

    def renderer(self, name):
        if name not in self.ctx:
            r = rtxpy.Renderer(0)
            r.upload(self.scene(name))
            self.ctx[name] = r
        return self.ctx[name], self.scene(name)

    def plain_ctx(self):
        """a context with no scene: the accumulation needs none"""
        if self.plain is None:
            self.plain = rtxpy.Renderer(0)
        return self.plain

    def close(self):
        for r in list(self.ctx.values()) + ([self.plain] if self.plain else []):
            r.close()
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture(scope="module")
def synth():
    return TM.synthetic()


def run(r, s, variance=True, conf=True, **kw):
    """rtx_temporal on a synthetic() dict"""
    return r.temporal(s["cur_frame"], s["c"], s["Vc"] if variance else None, s["f"], s["prev_frame"], s["hc"],
                      s["Vh"] if variance else None, s["L"], s["g"], conf=conf, **kw)


@pytest.fixture(scope="module")
def device_out(world, synth):
    return run(world.plain_ctx(), synth, **TM.SIGMAS)


def errors(got, ref, s, max_history=32):
    """(rgb in M, conf, len in max_history, var in the largest finite variance): the largest differences from the model"""
    M, VM = TM.finite_max(s["c"], s["hc"]), TM.finite_max(s["Vc"], s["Vh"])
    rgb, var, length, conf = got
    e = [np.abs(rgb.astype(np.float64) - ref["rgb"]).max() / M, np.abs(conf.astype(np.float64) - ref["conf"]).max(),
         np.abs(length.astype(np.float64) - ref["len"]).max() / max_history]
    if var is not None:
        e.append(np.abs(var.astype(np.float64) - ref["var"]).max() / VM)
    return e


def within(e):
    return e[0] <= TOL and e[1] <= TOL and e[2] <= TOL and (len(e) < 4 or e[3] <= 2 * TOL)


# ---- 1. the kernel against the model ----
def test_temporal_matches_the_model(synth, device_out):
    """|d rgb| <= 2e-5 M, |d conf| <= 2e-5, |d len| <= 2e-5 max_history, |d V| <= 4e-5 of the largest finite variance
    (M the largest finite |c| or |hc|).  Measured on an MI355X: 1.03e-7 M, 7.3e-8, 7.0e-8 max_history and 5.8e-8 of
    the largest variance."""
    ref = TM.model_of(synth)
    live = ref["len"] > 0
    fin = np.isfinite(synth["c"]).all(-1)
    assert ref["margin"] > 1e-3
    e = errors(device_out, ref, synth)
    print(f"max |d rgb| = {e[0]:.3e} M, |d conf| = {e[1]:.3e}, |d len| = {e[2]:.3e} max_history, |d V| = {e[3]:.3e} Vmax")
    rgb, var, length, conf = device_out
    assert np.isfinite(rgb[fin]).all() and np.isfinite(var).all() and np.isfinite(length).all() and np.isfinite(conf).all()
    assert conf.min() >= 0 and conf.max() <= 1 + TOL and length[live].min() >= 1 and length.max() <= 32
    assert within(e), e
    # it is neither the current frame nor the history copied: either would not pass
    M = TM.finite_max(synth["c"], synth["hc"])
    assert np.abs(ref["rgb"] - synth["c"]).max() > 100 * TOL * M


def test_the_counters_are_the_models(world, synth, device_out):
    ref = TM.model_of(synth)
    run(world.plain_ctx(), synth, **TM.SIGMAS)
    st = world.plain_ctx().temporal_stats()
    live, hist = int((ref["len"] > 0).sum()), int((ref["conf"] > 0).sum() - (synth["f"]["z"] == 0).sum())
    assert (st.pixels, st.live_pixels, st.history_pixels, st.reset_pixels) == (37 * 29, live, hist, live - hist)
    assert st.temporal_ms > 0 and st.frames == 0 and st.render_ms == 0


def test_an_infinite_sigma_switches_its_term_off(world, synth):
    for term in ("normal", "albedo", "plane"):
        sig = dict(TM.SIGMAS, **{"sigma_" + term: float("inf")})
        e = errors(run(world.plain_ctx(), synth, **sig), TM.model_of(synth, without=term), synth)
        assert within(e), (term, e)


def test_without_the_material_match(world, synth):
    ref = TM.model_of(synth, match_material=False)
    e = errors(run(world.plain_ctx(), synth, match_material=0, **TM.SIGMAS), ref, synth)
    assert within(e), e
    assert np.abs(ref["rgb"] - TM.model_of(synth)["rgb"]).max() > 1e-2


def test_without_variance_the_rest_is_the_same(world, synth, device_out):
    rgb, var, length, conf = run(world.plain_ctx(), synth, variance=False, **TM.SIGMAS)
    ref = TM.temporal(synth["cur_frame"], synth["c"], None, synth["f"], synth["prev_frame"], synth["hc"], None, synth["L"],
                      synth["g"])
    assert var is None and within(errors((rgb, None, length, conf), ref, synth))
    assert not np.array_equal(bits(conf), bits(device_out[3]))  # a history pixel of bad variance alone is usable here


@pytest.mark.parametrize("w,h", SHAPES)
def test_frame_shapes(world, w, h):
    """one pixel, one past a tile each way, a strip each way: against the model"""
    s = TM.shape_pair(w, h)
    ref = TM.model_of(s)
    assert ref["margin"] > 1e-4
    e = errors(run(world.plain_ctx(), s, **TM.SIGMAS), ref, s)
    assert within(e), (w, h, e)
    if w * h > 1:
        assert (ref["conf"] > 0.5).any() and (ref["len"] == 1).any()


# ---- 2. properties ----
def static_pair(synth, k):
    """identical frames and records, every history length k"""
    return dict(synth, cur_frame=synth["prev_frame"], f=synth["g"], L=np.full((29, 37), k, np.float32))


@pytest.mark.parametrize("k", [1, 2, 31, 32])
def test_a_static_camera_is_the_running_mean(world, synth, k):
    """h + (c - h) / (k + 1) within 4 2^-24 M and length k + 1; at k = 32 the length stays max_history (measured: at
    most 0.88 2^-24 M)"""
    s = static_pair(synth, k)
    rgb, var, length, conf = run(world.plain_ctx(), s)
    ok = (s["f"]["z"] != 0) & np.isfinite(s["hc"]).all(-1) & np.isfinite(s["Vh"]).all(-1)
    n = min(k, 31)
    c, hc = s["c"].astype(np.float64), s["hc"].astype(np.float64)
    with np.errstate(invalid="ignore"):  # the history's NaN and inf, outside `ok`
        want = hc + (c - hc) / (n + 1)
    M = TM.finite_max(s["c"], s["hc"])
    err = np.abs(rgb[ok] - want[ok]).max() / M
    print(f"k = {k}: max |d rgb| = {err * 2 ** 24:.2f} 2^-24 M")
    assert err <= 4 * 2.0 ** -24
    assert np.all(length[ok] == n + 1) and np.all(conf[ok] == 1.0)
    a = 1.0 / (n + 1)
    vwant = (1 - a) ** 2 * s["Vh"].astype(np.float64) + a * a * s["Vc"]
    assert np.abs(var[ok] - vwant[ok]).max() <= 8 * 2.0 ** -24 * TM.finite_max(s["Vc"], s["Vh"])


def test_max_history_one_returns_the_current_frame(world, synth):
    rgb, var, length, conf = run(world.plain_ctx(), synth, max_history=1, **TM.SIGMAS)
    live = TM.model_of(synth)["len"] > 0
    M = TM.finite_max(synth["c"], synth["hc"])
    assert np.abs(rgb[live] - synth["c"][live]).max() <= 2.0 ** -23 * M
    assert np.all(length[live] == 1) and np.all(length[~live] == 0)
    assert np.abs(var[live] - synth["Vc"][live]).max() <= 2.0 ** -23 * TM.finite_max(synth["Vc"])


def test_no_history_returns_the_current_frames_bits(world, synth):
    r = world.plain_ctx()
    rgb, var, length, conf = r.temporal(synth["cur_frame"], synth["c"], synth["Vc"], synth["f"])
    hit = synth["f"]["z"] != 0
    assert np.array_equal(bits(rgb), bits(synth["c"])) and np.array_equal(bits(var), bits(synth["Vc"]))
    assert np.all(length[hit] == 1) and np.all(conf[hit] == 0) and np.all(length[~hit] == 0) and np.all(conf[~hit] == 1)
    st = r.temporal_stats()
    assert (st.live_pixels, st.history_pixels, st.reset_pixels) == (int(hit.sum()), 0, int(hit.sum()))
    rgb2, var2, length2, conf2 = r.temporal(synth["cur_frame"], synth["c"], None, synth["f"], conf=False)
    assert var2 is None and conf2 is None and np.array_equal(bits(rgb2), bits(synth["c"])) and np.array_equal(length2, length)


def test_pixels_that_are_not_live_keep_their_bits(world, synth):
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in synth.items()}
    hit = s["f"]["z"] != 0
    assert hit[3, 4] and hit[10, 20] and hit[15, 6] and hit[22, 30] and not hit.all()
    s["c"][3, 4] = (np.nan, 0.25, -0.0)
    s["c"][10, 20, 2] = -np.inf
    s["Vc"][15, 6, 1] = -1e-6
    s["Vc"][22, 30, 0] = np.nan
    dead = ~hit
    for y, x in ((3, 4), (10, 20), (15, 6), (22, 30)):
        dead[y, x] = True
    rgb, var, length, conf = run(world.plain_ctx(), s, **TM.SIGMAS)
    assert np.array_equal(bits(rgb)[dead], bits(s["c"])[dead]) and np.array_equal(bits(var)[dead], bits(s["Vc"])[dead])
    assert np.all(length[dead] == 0) and np.all(conf[dead & ~hit] == 1) and np.all(conf[dead & hit] == 0)
    assert within(errors((np.where(dead[..., None], 0, rgb), np.where(dead[..., None], 0, var), length, conf),
                         {k: (np.where(dead[..., None], 0, v) if k in ("rgb", "var") else v) for k, v in TM.model_of(s).items()}, s))
    # a negative variance alone does not matter without variance buffers
    rgb, _, length, _ = run(world.plain_ctx(), s, variance=False, **TM.SIGMAS)
    assert length[15, 6] >= 1 and length[3, 4] == 0


def test_poisoned_history_poisons_no_output(world, synth, device_out):
    """the synthetic history holds a NaN and an inf in its colour and in its variance"""
    rgb, var, length, conf = device_out
    assert np.isfinite(rgb).all() and np.isfinite(var).all() and np.isfinite(length).all() and np.isfinite(conf).all()
    s = static_pair(synth, 5)
    s["L"][7, 7], s["L"][8, 8], s["L"][9, 9] = np.nan, np.inf, 0.5
    rgb, var, length, conf = run(world.plain_ctx(), s)
    assert np.isfinite(rgb).all() and np.isfinite(var).all() and np.isfinite(length).all() and np.isfinite(conf).all()
    for y, x in ((7, 7), (8, 8), (9, 9), (5, 9), (20, 30), (12, 12), (8, 25)):
        assert s["f"]["z"][y, x] != 0
        assert conf[y, x] == 0 and length[y, x] == 1 and np.array_equal(bits(rgb[y, x]), bits(s["c"][y, x])), (y, x)


def test_two_runs_give_the_same_bits(world, synth, device_out):
    again = run(world.plain_ctx(), synth, **TM.SIGMAS)
    for a, b in zip(again, device_out):
        assert np.array_equal(bits(a), bits(b))


# ---- 3. the device entry ----
def guarded(arrays, guard=64):
    """the arrays as device buffers of float32 words, each with `guard` words of 7.5 before and after it"""
    import torch
    bufs = []
    for a in arrays:
        words = np.ascontiguousarray(a).view(np.float32).reshape(-1)
        t = torch.full((words.size + 2 * guard,), 7.5, dtype=torch.float32, device="cuda")
        t[guard:guard + words.size] = torch.from_numpy(words.copy()).cuda()
        bufs.append(t)
    return bufs


@pytest.mark.parametrize("variance,conf", [(True, True), (True, False), (False, True), (False, False)])
def test_device_entry_equals_the_host_entry_and_stays_in_bounds(world, synth, variance, conf):
    import torch
    s, n, guard = synth, 37 * 29, 64
    r = world.plain_ctx()
    want = run(r, s, variance=variance, conf=conf, **TM.SIGMAS)
    for stream in (None, torch.cuda.Stream()):
        ins = guarded([s["c"], s["Vc"], s["f"], s["hc"], s["Vh"], s["L"], s["g"]])
        outs = guarded([np.zeros(3 * n, np.float32), np.zeros(3 * n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)])
        before = [b.cpu().numpy().copy() for b in ins]
        torch.cuda.synchronize()
        p = [b.data_ptr() + 4 * guard for b in ins + outs]
        assert all(q % 16 == 0 for q in p)
        c, vc, f, hc, vh, L, g, o_rgb, o_var, o_len, o_conf = p
        r.temporal_device(s["cur_frame"], c, vc if variance else None, f, s["prev_frame"], hc, vh if variance else None, L, g,
                          o_rgb, o_var if variance else None, o_len, o_conf if conf else None,
                          stream=stream.cuda_stream if stream else None, **TM.SIGMAS)
        for b, a in zip(ins, before):
            assert np.array_equal(b.cpu().numpy().view(np.uint32), a.view(np.uint32))  # inputs and their guards untouched
        for b, words, x in zip(outs, (3 * n, 3 * n, n, n), want):
            host = b.cpu().numpy()
            assert np.all(host[:guard] == 7.5) and np.all(host[guard + words:] == 7.5)
            if x is None:
                assert np.all(host == np.where((np.arange(host.size) >= guard) & (np.arange(host.size) < guard + words), 0, 7.5))
            else:
                assert np.array_equal(bits(host[guard:guard + words]), bits(x).ravel())
    # in place over the current frame, as the pipeline runs it
    if variance:
        r.temporal_device(s["cur_frame"], c, vc, f, s["prev_frame"], hc, vh, L, g, c, vc, o_len, None, **TM.SIGMAS)
        assert np.array_equal(bits(ins[0].cpu().numpy()[guard:guard + 3 * n]), bits(want[0]).ravel())
        assert np.array_equal(bits(ins[1].cpu().numpy()[guard:guard + 3 * n]), bits(want[1]).ravel())
    # a feature pointer off the 16-byte grid, an output over the history
    for bad in ({2: f + 4}, {6: g + 4}, {7: hc}, {9: L}, {7: g + 48}, {10: vh + 4 * n}):
        a = [c, vc, f, hc, vh, L, g, o_rgb, o_var, o_len, o_conf]
        for k, v in bad.items():
            a[k] = v
        with pytest.raises(rtxpy.RtxError) as e:
            r.temporal_device(s["cur_frame"], a[0], a[1], a[2], s["prev_frame"], *a[3:])
        assert e.value.code == abi.RTX_ERR_ARG, bad


# ---- 4. argument errors ----
def test_argument_errors(world, synth):
    s = synth
    r = world.plain_ctx()
    lib = r.lib
    nan = float("nan")
    for bad in ({"max_history": 0}, {"max_history": 65537}, {"sigma_normal": 0.0}, {"sigma_albedo": -1.0}, {"sigma_plane": nan},
                {"sigma_normal": nan}):
        with pytest.raises(rtxpy.RtxError) as e:
            run(r, s, **bad)
        assert e.value.code == abi.RTX_ERR_ARG, bad
    run(r, s, max_history=65536, sigma_plane=float("inf"))  # both allowed
    tp = rtxpy.temporal_params()
    out = [np.full((29, 37, 3), 3.0, np.float32), np.full((29, 37, 3), 3.0, np.float32), np.full((29, 37), 3.0, np.float32),
           np.full((29, 37), 3.0, np.float32)]
    ptr = lambda a: a.ctypes.data  # noqa: E731
    good = [ctypes.byref(tp), ctypes.byref(s["cur_frame"]), ptr(s["c"]), ptr(s["Vc"]), ptr(s["f"]), ctypes.byref(s["prev_frame"]),
            ptr(s["hc"]), ptr(s["Vh"]), ptr(s["L"]), ptr(s["g"])] + [ptr(o) for o in out]

    def refused(a):
        assert lib.rtx_temporal(r._ctx, *a) == abi.RTX_ERR_ARG
        assert lib.rtx_temporal_device(r._ctx, *a, None) == abi.RTX_ERR_ARG

    def without(*ks):
        a = list(good)
        for k in ks:
            a[k] = None
        return a

    for k in (0, 1, 2, 4, 10, 12):  # params, the current frame, its colour and records, out_rgb, out_length
        refused(without(k))
    for ks in ((3,), (11,), (7,), (3, 11), (3, 7), (7, 11)):  # mixed-null variance pointers
        refused(without(*ks))
    for ks in ((5,), (6,), (8,), (9,), (5, 6, 8), (6, 8, 9), (5, 6, 8, 9)):  # mixed-null history pointers (the last: Vh stays)
        refused(without(*ks))
    assert lib.rtx_temporal(r._ctx, *without(3, 7, 11, 13)) == abi.RTX_OK  # no variance, no confidence
    for o in out:
        o[...] = 3.0
    other = abi.Frame.from_buffer_copy(s["prev_frame"])
    other.width, other.height = 29, 37
    a = list(good)
    a[5] = ctypes.byref(other)
    refused(a)
    singular = abi.Frame.from_buffer_copy(s["prev_frame"])
    for i in range(3):
        singular.step_y[i] = 2 * singular.step_x[i]
    a[5] = ctypes.byref(singular)
    refused(a)
    for w, h in ((0, 29), (37, 0), (1 << 16, 1 << 15)):  # w h = 0, and 2^31 pixels: above RTX_RAYS_MAX
        cur, prev = abi.Frame.from_buffer_copy(s["cur_frame"]), abi.Frame.from_buffer_copy(s["prev_frame"])
        cur.width = prev.width = w
        cur.height = prev.height = h
        a = list(good)
        a[1], a[5] = ctypes.byref(cur), ctypes.byref(prev)
        refused(a)
    a = list(good)
    a[10] = ptr(s["hc"])  # an output over the history
    refused(a)
    assert all(np.all(o == 3.0) for o in out)
    # the context still works
    rgb, _, _, _ = run(r, s)
    assert np.isfinite(rgb).all()


def test_pipeline_argument_errors(world):
    r, scene = world.renderer("scene3")
    frame, p = scene.frame(64, 40), render_params("ambient")
    for bad in ({"max_history": 0}, {"max_history": 65537}, {"sigma_plane": 0.0}, {"sigma_normal": float("nan")}, {"passes": 0}):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_temporal(frame, p, **bad)
        assert e.value.code == abi.RTX_ERR_ARG, bad
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_temporal(frame, rtxpy.params_from_args([], tile_offset=1, tile_stride=2))
    assert e.value.code == abi.RTX_ERR_ARG
    with pytest.raises(rtxpy.RtxError) as e:
        world.plain_ctx().render_temporal(frame, p)
    assert e.value.code == abi.RTX_ERR_STATE
    lib, pp, tp = r.lib, rtxpy.pass_params(), rtxpy.temporal_params()
    f, q, a, t = ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), ctypes.byref(tp)
    for args in ((None, q, a, t), (f, None, a, t), (f, q, None, t), (f, q, a, None)):
        assert lib.rtx_render_temporal(r._ctx, *args, None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_render_temporal_device(r._ctx, f, q, a, t, ctypes.c_void_p(4), None, None, None, None) == abi.RTX_ERR_ARG
    r.temporal_reset()
    assert lib.rtx_render_temporal(r._ctx, f, q, a, t, None, None, None, None) == abi.RTX_OK  # no output at all
    assert r.temporal_stats().frames == 1
    r.temporal_reset()


# ---- 5. the pipeline ----
def shift_of(scene, frame, z, pixels):
    """the move along the camera's x axis that shifts a point at the median hit distance by `pixels`"""
    cam = scene.desc.camera
    step = float(np.linalg.norm(TM.vec(frame.step_x)))
    return pixels * step * float(np.median(z[z != 0])) / cam.focal_length * TM.vec(cam.vectors[0])


def path_frames(r, scene, w, h, n, pixels):
    """n frames of a sideways dolly of `pixels` of image shift per frame"""
    base = scene.frame(w, h)
    move = shift_of(scene, base, r.features(base)["z"], pixels)
    return [scene.frame(w, h, camera=scene.camera(move=tuple(k * move))) for k in range(n)]


@pytest.mark.parametrize("name,w,h,gi", PIPELINE)
def test_render_temporal_is_its_pieces(world, name, w, h, gi):
    """three frames of a moved-camera path: rgb, z, variance and length are those of render_passes, features and
    temporal chained by hand, bit for bit, and the statistics add up; then a reset, a re-upload and a size change each
    start over"""
    r, scene = world.renderer(name)
    frames = path_frames(r, scene, w, h, 3, 2.5)
    passes = 2 if gi == "path" else 1
    r.temporal_reset()
    hist, prev = (None, None, None, None), None
    first = None
    for k, frame in enumerate(frames):
        p = render_params(gi, seed=1000 + 10 * k)
        rgb, z, var = r.render_passes(frame, p, passes)
        ps = r.pass_stats()
        f = r.features(frame)
        want = r.temporal(frame, rgb, var, f, prev, *hist, conf=True)
        ts = r.temporal_stats()
        got = r.render_temporal(frame, p, passes)
        st, ps2, rs = r.temporal_stats(), r.pass_stats(), r.stats()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(z)), k
        assert np.array_equal(bits(got[2]), bits(want[1])) and np.array_equal(bits(got[3]), bits(want[2])), k
        hit = int((z != 0).sum())
        assert (st.frames, st.pixels) == (k + 1, w * h)
        assert (st.live_pixels, st.history_pixels, st.reset_pixels) == (ts.live_pixels, ts.history_pixels, ts.reset_pixels)
        assert st.live_pixels == st.history_pixels + st.reset_pixels <= hit
        assert st.history_pixels == int((want[3] > 0).sum() - (z == 0).sum())
        assert (st.history_pixels == 0) == (k == 0)
        assert (st.closest_rays, st.shadow_rays) == (ps.closest_rays, ps.shadow_rays) == (ps2.closest_rays, ps2.shadow_rays)
        assert ps2.passes_run == passes and rs.closest_rays > 0
        assert st.render_ms > 0 and st.features_ms > 0 and st.temporal_ms > 0
        if gi == "path":
            assert (want[1] > 0).any()
        if k == 0:
            first = (p, want)
        hist, prev = (want[0], want[1], want[2], f), frame
    assert (hist[2] > 1.5).any() and (hist[2] == 1).any()  # history was found, and lost
    # each of these forgets the history: the first frame again, bit for bit
    small = scene.frame(w // 2, h // 2)
    for forget in (r.temporal_reset, lambda: r.upload(scene), lambda: r.render_temporal(small, first[0], passes)):
        forget()
        got = r.render_temporal(frames[0], first[0], passes)
        assert r.temporal_stats().frames == 1 and r.temporal_stats().history_pixels == 0
        assert np.array_equal(bits(got[0]), bits(first[1][0])) and np.all(got[3] <= 1)
    got = r.render_temporal(frames[0], render_params(gi, seed=5), passes)  # and the next call finds it
    assert r.temporal_stats().frames == 2 and (got[3] == 2).any()
    r.temporal_reset()


def test_render_temporal_on_device_buffers(world):
    import torch
    name, w, h, gi = PIPELINE[0]
    r, scene = world.renderer(name)
    frames = path_frames(r, scene, w, h, 2, 2.5)
    n, guard = w * h, 64
    for stream in (None, torch.cuda.Stream()):
        r.temporal_reset()
        want = [r.render_temporal(fr, render_params(gi, seed=7 + k)) for k, fr in enumerate(frames)][1]
        r.temporal_reset()
        r.render_temporal_device(frames[0], render_params(gi, seed=7), None, None, None, None)
        bufs = guarded([np.zeros(3 * n, np.float32), np.zeros(n, np.float32), np.zeros(3 * n, np.float32), np.zeros(n, np.float32)])
        torch.cuda.synchronize()
        r.render_temporal_device(frames[1], render_params(gi, seed=8), *[b.data_ptr() + 4 * guard for b in bufs],
                                 stream=stream.cuda_stream if stream else None)
        for b, words, x in zip(bufs, (3 * n, n, 3 * n, n), want):
            host = b.cpu().numpy()
            assert np.array_equal(bits(host[guard:guard + words]), bits(x).ravel())
            assert np.all(host[:guard] == 7.5) and np.all(host[guard + words:] == 7.5)
    r.temporal_reset()


@pytest.mark.parametrize("name,w,h,gi", PIPELINE)
def test_a_static_camera_accumulates_the_cumulative_mean(world, name, w, h, gi):
    """K = 6 distinct seeds: rgb within K 4 2^-24 M of the float64 mean of the six separate frames, length K"""
    r, scene = world.renderer(name)
    frame, K = scene.frame(w, h), 6
    r.temporal_reset()
    singles = []
    for k in range(K):
        p = render_params(gi, seed=300 + 7 * k)
        singles.append(r.render(frame, p)[0].astype(np.float64))
        rgb, z, var, length = r.render_temporal(frame, p)
    mean = np.mean(singles, axis=0)
    M = max(float(np.abs(s).max()) for s in singles)
    hit = z != 0
    err = np.abs(rgb - mean)[hit].max() / M
    print(f"{name} {gi}: max |rgb - mean of {K}| = {err * 2 ** 24:.2f} 2^-24 M")
    assert err <= K * 4 * 2.0 ** -24
    assert np.all(length[hit] == K) and np.all(length[~hit] == 0)
    assert r.temporal_stats().frames == K and r.temporal_stats().history_pixels == int(hit.sum())
    r.temporal_reset()


# ---- 6. the geometry on a real render ----
def mse(a, b, mask):
    return float(((a[mask].astype(np.float64) - b[mask]) ** 2).mean())


@pytest.mark.parametrize("name", ["scene3", "scene2"])
def test_a_reprojected_frame_is_closer_to_the_moved_cameras_render(world, name):
    """constant RNG, ambient, 128x72, the camera moved sideways by 3.5 pixels of image shift.  Frame A is the history
    with L = 65535 under max_history 65536, so out is A fetched at the reprojected position: over the pixels with
    conf > 0.99 it must be closer to B's own render than A is, pixel for pixel"""
    r, scene = world.renderer(name)
    w, h = 128, 72
    fa, fb = path_frames(r, scene, w, h, 2, 3.5)
    p = render_params("ambient", rng=abi.RTX_RNG_CONST)
    A, zA = r.render(fa, p)
    B, zB = r.render(fb, p)
    ga, gb = r.features(fa), r.features(fb)
    u, _, _ = rtxpy.frame_project(fa, gb["position"])
    hit = zB != 0
    shift = np.abs(u - np.mgrid[0:h, 0:w][1])[hit]
    assert np.median(shift) >= 3.0, np.median(shift)
    out, _, length, conf = r.temporal(fb, B, None, gb, fa, A, None, np.full((h, w), 65535, np.float32), ga, max_history=65536)
    sure = hit & (conf > 0.99)
    m_out, m_a = mse(out, B, sure), mse(A, B, sure)
    print(f"{name}: median shift {np.median(shift):.2f} px, {int(sure.sum())} of {int(hit.sum())} hit pixels above 0.99, "
          f"mse reprojected {m_out:.4e}, unmoved {m_a:.4e} (ratio {m_out / m_a:.4f})")
    assert sure.sum() >= hit.sum() / 4
    assert np.all(length[sure] > 0.99 * 65535)  # n = sum w L is at least conf L
    assert m_out < m_a


# ---- 7. quality ----
def quality_static(world, name, w, h, frames=8):
    r, scene = world.renderer(name)
    frame = scene.frame(w, h)
    ref, z, _ = r.render_passes(frame, render_params("path", seed=90000), 256)
    hit = z != 0
    r.temporal_reset()
    for k in range(frames):
        p = render_params("path", seed=500 + 11 * k)
        rgb = r.render_temporal(frame, p)[0]
    single = r.render(frame, p)[0]
    r.temporal_reset()
    return mse(rgb, ref, hit), mse(single, ref, hit)


def quality_dolly(world, name, w=128, h=72, frames=8):
    """the last frame of an 8-frame sideways dolly of 1.5 px per frame, accumulated and alone, against its own 256-pass
    mean: (mse temporal, mse single, mean conf-free length)"""
    r, scene = world.renderer(name)
    path = path_frames(r, scene, w, h, frames, 1.5)
    ref, z, _ = r.render_passes(path[-1], render_params("path", seed=90000), 256)
    hit = z != 0
    r.temporal_reset()
    for k, frame in enumerate(path):
        p = render_params("path", seed=700 + 13 * k)
        rgb, _, _, length = r.render_temporal(frame, p)
    single = r.render(path[-1], p)[0]
    r.temporal_reset()
    m = mse(rgb, ref, hit), mse(single, ref, hit)
    print(f"{name} {w}x{h}: dolly of {frames} frames, mse temporal {m[0]:.5e}, single {m[1]:.5e} (ratio {m[0] / m[1]:.4f}), "
          f"mean length {length[hit].mean():.2f}")
    return m


@pytest.mark.parametrize("name", ["scene3", "scene2"])
def test_a_static_camera_beats_the_single_frame(world, name):
    """-g path -n 1, 8 frames of distinct seeds against a 256-pass mean of the same frame: the mean of independent
    frames guarantees it (expected ratio: about 1/8; measured: scene2 0.169, scene3 0.628, whose single frame is
    already within 7e-12 of the mean)"""
    m = quality_static(world, name, 128, 72)
    print(f"{name}: static camera, 8 frames, mse temporal {m[0]:.5e}, single {m[1]:.5e} (ratio {m[0] / m[1]:.4f})")
    assert m[0] < m[1], m


@pytest.mark.parametrize("name", ["scene2"])
def test_a_dolly_beats_the_single_frame(world, name):
    """the scenes whose measured ratio is below 0.8 (scene2: 0.439, mean history length 4.6).  The run is
    deterministic; the margin guards later changes of the defaults"""
    m = quality_dolly(world, name)
    assert m[0] < m[1], m


@pytest.mark.parametrize("name", ["scene1", "scene3", "scenetest"])
def test_quality_of_the_dolly_not_asserted(world, name):
    """printed for DESIGN §7.9 (measured: scenetest 0.861; scene1 16.8 and scene3 211, losses: at -g path -n 1 their
    single frames are within 5e-10 and 4e-12 of the 256-pass mean, less than what the bilinear fetch of a shaded,
    textured history and the lag of the highlights cost, 9e-9 and 9e-10)"""
    m = quality_dolly(world, name)
    assert all(np.isfinite(m))
