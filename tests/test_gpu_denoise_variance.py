"""The variance-guided denoiser on the GPU (csrc/rtx_denoise_variance.hip through rtx_denoise_variance*).

The filter level by level against the float64 model of denoise_variance_model.py on the synthetic frame
of denoise_model.py and a variance with which every term of the weight decides something
(test_denoise_variance_model.py checks that), then the pixels that are not live, infinite sigmas, a zero
variance, freedom from the frame's scale, determinism, the device entry, frame shapes, steps beyond the
frame, the argument errors and the stats.  Quality: the mean of 4 one-sample path-traced passes, filtered
with the shipped defaults, against a 1024-spp frame.  Composition: the mean and variance of an adaptive
render, whose tiles received different numbers of passes, against the model.
"""
import ctypes
import os

import numpy as np
import pytest

import conftest as C
import denoise_variance_model as VM
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

W, H = 37, 29
LIVE = W * H - 30 - 2 - 3  # misses; the NaN and the inf colour; the NaN, the negative and the inf variance
BOUND = 2e-5               # of M (colour) and of the level input's largest finite V (variance), as rtx_denoise's test
PATH1 = ["-g", "path", "-n", "1"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def finite_vmax(V, live):
    return float(V[live].max())


class World:
    """scenes and contexts, each made once and shared (no test changes a shared array)"""

    def __init__(self):
        self.scenes, self.ctx, self.frames = {}, {}, {}
        self.plain = None

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = rtxpy.Scene.load(os.path.join(C.SCENES, name + ".json"), base_dir=C.GOLDEN)
        return self.scenes[name]

    def renderer(self, name):
        if name not in self.ctx:
            r = rtxpy.Renderer(0)
            r.upload(self.scene(name))
            self.ctx[name] = r
        return self.ctx[name]

    def filter_ctx(self):
        """a context with no scene: the filter needs none"""
        if self.plain is None:
            self.plain = rtxpy.Renderer(0)
        return self.plain

    def quality_frames(self, name, w, h):
        """(mean, z, variance of 4 one-sample passes, the 1024-spp frame, features), rendered once"""
        key = (name, w, h)
        if key not in self.frames:
            scene, r = self.scene(name), self.renderer(name)
            frame = scene.frame(w, h)
            mean, z, var = r.render_passes(frame, rtxpy.params_from_args(PATH1, seed=11), passes=4)
            ref, _ = r.render(frame, rtxpy.params_from_args(["-g", "path", "-n", "1024"], seed=2024))
            self.frames[key] = (mean, z, var, ref, r.features(frame))
        return self.frames[key]

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
    rgb, feat = VM.synthetic()
    return rgb, VM.synthetic_variance(rgb), feat


@pytest.fixture(scope="module")
def levels(world, synth):
    """the device's (rgb, variance) after k = 0..5 iterations of the synthetic frame (0: the input)"""
    rgb, var, feat = synth
    r = world.filter_ctx()
    return [(rgb, var)] + [r.denoise_variance(rgb, var, feat, iterations=k, **VM.SIGMAS) for k in range(1, 6)]


def gaps(out, ref, src, feat, label=""):
    """(colour gap / M, variance gap / Vmax, colour move / M, variance move / Vmax) of a device level `out` against the
    model's `ref` for the level input `src`, over the live pixels"""
    live = VM.live_mask(src[0], src[1], feat)
    M, VX = VM.finite_max(src[0]), finite_vmax(src[1], live)
    g = (np.abs(out[0][live].astype(np.float64) - ref[0][live]).max() / M,
         np.abs(out[1][live].astype(np.float64) - ref[1][live]).max() / VX,
         np.abs(ref[0][live] - src[0][live]).max() / M, np.abs(ref[1][live] - src[1][live]).max() / VX)
    print(f"{label}: colour gap {g[0]:.3e} M, variance gap {g[1]:.3e} Vmax, moves {g[2]:.3e} M, {g[3]:.3e} Vmax")
    return g


# ---- 1. the filter against the model, level by level ----
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_filter_level_matches_the_model(synth, levels, k):
    """k iterations on the device against one model level (k - 1) of the device's k - 1 iterations: colour within
    2e-5 M, variance within 2e-5 of the level input's largest finite V (the existing filter's bound: a fast exp's
    argument scaling, about e 2^-23 of a weight, twice that in w^2; measured gaps in DESIGN §7.5), and the level
    moves both by more than twice the bound"""
    feat = synth[2]
    src, out = levels[k - 1], levels[k]
    live = VM.live_mask(src[0], src[1], feat)
    assert live.sum() == LIVE
    ref = VM.level(src[0], src[1], feat, k - 1)
    gc, gv, mc, mv = gaps(out, ref, src, feat, f"level {k - 1}")
    assert np.isfinite(out[0][live]).all() and np.isfinite(out[1][live]).all() and (out[1][live] >= 0).all()
    assert gc <= BOUND and gv <= BOUND, (gc, gv)
    assert mc > 2 * BOUND and mv > 2 * BOUND, (mc, mv)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_pixels_that_are_not_live_keep_their_bits(world, synth, k):
    """misses, the NaN and the inf colour, and the pixels rtx_denoise would filter whose variance has a NaN, a
    negative or an infinite component: colour and variance bits untouched"""
    rgb, var, feat = synth
    live = VM.live_mask(rgb, var, feat)
    assert not live[8, 25] and not live[17, 9] and not live[22, 33] and feat["z"][8, 25] != 0 and np.isfinite(rgb[8, 25]).all()
    out = world.filter_ctx().denoise_variance(rgb, var, feat, iterations=k, **VM.SIGMAS)
    assert np.array_equal(bits(out[0])[~live], bits(rgb)[~live])
    assert np.array_equal(bits(out[1])[~live], bits(var)[~live])
    assert not np.array_equal(bits(out[0])[live], bits(rgb)[live])


def test_an_infinite_sigma_switches_its_term_off(world, synth):
    rgb, var, feat = synth
    for term in VM.TERMS:
        sig = dict(VM.SIGMAS, **{"sigma_" + term: float("inf")})
        out = world.filter_ctx().denoise_variance(rgb, var, feat, iterations=1, **sig)
        gc, gv, _, _ = gaps(out, VM.level(rgb, var, feat, 0, without=term), (rgb, var), feat, "without " + term)
        assert gc <= BOUND and gv <= BOUND, term


@pytest.mark.parametrize("k", [1, 3])
def test_a_zero_variance_returns_the_colours_bits(world, synth, k):
    rgb, _, feat = synth
    out = world.filter_ctx().denoise_variance(rgb, np.zeros_like(rgb), feat, iterations=k, **VM.SIGMAS)
    assert np.array_equal(bits(out[0]), bits(rgb))
    assert not bits(out[1]).any()


@pytest.mark.parametrize("e", [-12, 10])
def test_the_filter_does_not_depend_on_the_frames_scale(world, synth, levels, e):
    """(s c, s^2 V) for s a power of two returns (s c', s^2 V'): every operation on a colour or a variance scales
    exactly and e does not change.  Expected bit for bit; 4 float ulps allowed."""
    rgb, var, feat = synth
    s = np.float32(2.0 ** e)
    live = VM.live_mask(rgb, var, feat)
    out = world.filter_ctx().denoise_variance(rgb * s, var * s * s, feat, iterations=3, **VM.SIGMAS)
    worst = 0
    for got, want in ((out[0], levels[3][0] * s), (out[1], levels[3][1] * s * s)):
        d = np.abs(bits(got)[live].astype(np.int64) - bits(want)[live].astype(np.int64)).max()
        worst = max(worst, int(d))
    print(f"scale 2^{e}: largest difference {worst} ulps")
    assert worst <= 4


def test_two_runs_give_the_same_bits_and_the_stats(world, synth, levels):
    rgb, var, feat = synth
    r = world.filter_ctx()
    again = r.denoise_variance(rgb, var, feat, iterations=5, **VM.SIGMAS)
    assert np.array_equal(bits(again[0]), bits(levels[5][0])) and np.array_equal(bits(again[1]), bits(levels[5][1]))
    st = r.denoise_stats()
    assert (st.pixels, st.hit_pixels, st.iterations) == (W * H, W * H - 30, 5) and st.filter_ms > 0
    r.denoise_variance(rgb, var, feat, iterations=2, **VM.SIGMAS)
    assert r.denoise_stats().iterations == 2


@pytest.mark.parametrize("k", [1, 4])
def test_device_entry_equals_the_host_entry(world, synth, levels, k):
    import torch
    rgb, var, feat = synth
    d_rgb, d_var = torch.from_numpy(rgb.copy()).cuda(), torch.from_numpy(var.copy()).cuda()
    d_feat = torch.from_numpy(feat.view(np.float32).reshape(-1, 12).copy()).cuda()
    torch.cuda.synchronize()
    world.filter_ctx().denoise_variance_device(W, H, d_feat.data_ptr(), d_rgb.data_ptr(), d_var.data_ptr(), iterations=k, **VM.SIGMAS)
    assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(levels[k][0]))
    assert np.array_equal(bits(d_var.cpu().numpy()), bits(levels[k][1]))


@pytest.mark.parametrize("w,h", [(16, 16), (1, 1), (300, 2), (17, 33)])
def test_frame_shapes(world, w, h):
    """frames of one tile, one pixel, a strip and one past a tile each way, against the model's first two levels"""
    rng = np.random.default_rng(w * 1000 + h)
    feat = np.zeros((h, w), abi.FEATURE_DTYPE)
    feat["z"] = 3 + 0.02 * rng.random((h, w))
    feat["position"] = rng.random((h, w, 3)) * 0.02 + np.array([0, 0, 1]) * feat["z"][..., None]
    feat["normal"] = (0, 0, -1)
    feat["albedo"] = 0.5
    rgb = rng.random((h, w, 3), np.float32)
    var = (0.05 + 0.1 * rng.random((h, w, 3), np.float32)) ** 2
    r = world.filter_ctx()
    one = r.denoise_variance(rgb, var, feat, iterations=1, **VM.SIGMAS)
    two = r.denoise_variance(rgb, var, feat, iterations=2, **VM.SIGMAS)
    for out, src, k in ((one, (rgb, var), 0), (two, one, 1)):
        gc, gv, _, _ = gaps(out, VM.level(src[0], src[1], feat, k), src, feat, f"{w}x{h} level {k}")
        assert gc <= BOUND and gv <= BOUND
    if w * h > 1:
        assert not np.array_equal(one[0], rgb) and not np.array_equal(one[1], var)
    else:
        # the centre tap alone: c' = c, V' = w^2 V / w^2
        assert np.array_equal(bits(one[0]), bits(rgb)) and np.abs(one[1] / var - 1).max() <= 1e-6


def test_eight_iterations_step_past_the_frame(world, synth, levels):
    """steps 32, 64 and 128 on a 37 x 29 frame: at 32 a few columns still have a tap inside, beyond that every tap
    but the centre's is outside and the level is the identity"""
    rgb, var, feat = synth
    r = world.filter_ctx()
    six = r.denoise_variance(rgb, var, feat, iterations=6, **VM.SIGMAS)
    out = r.denoise_variance(rgb, var, feat, iterations=8, **VM.SIGMAS)
    gc, gv, _, _ = gaps(six, VM.level(levels[5][0], levels[5][1], feat, 5), levels[5], feat, "level 5")
    assert gc <= BOUND and gv <= BOUND
    gc, gv, _, _ = gaps(out, VM.level(six[0], six[1], feat, 6), six, feat, "levels 6 and 7 against level 6")
    assert gc <= BOUND and gv <= BOUND


def test_argument_errors_leave_both_buffers_alone(world, synth):
    import torch
    rgb, var, feat = synth
    r = world.filter_ctx()
    lib = r.lib
    for bad in ({"iterations": 0}, {"iterations": 9}, {"sigma_color": 0.0}, {"sigma_color": -2.0}, {"sigma_color": float("nan")},
                {"sigma_normal": -1.0}, {"sigma_albedo": float("nan")}, {"sigma_plane": 0.0}):
        with pytest.raises(rtxpy.RtxError) as e:
            r.denoise_variance(rgb, var, feat, **bad)
        assert e.value.code == abi.RTX_ERR_ARG, bad
    p = r.denoise_variance_params()
    out, ov = rgb.copy(), var.copy()
    P, F, R, V = ctypes.byref(p), feat.ctypes.data, out.ctypes.data, ov.ctypes.data
    fn = lib.rtx_denoise_variance
    for args in ((W, H, None, F, R, V), (W, H, P, None, R, V), (W, H, P, F, None, V), (W, H, P, F, R, None),
                 (0, H, P, F, R, V), (W, 0, P, F, R, V), (1 << 16, 1 << 15, P, F, R, V)):  # 2^31 pixels: above RTX_RAYS_MAX
        assert fn(r._ctx, *args) == abi.RTX_ERR_ARG, args[:2]
    bad = r.denoise_variance_params(iterations=9)
    assert fn(r._ctx, W, H, ctypes.byref(bad), F, R, V) == abi.RTX_ERR_ARG
    assert np.array_equal(bits(out), bits(rgb)) and np.array_equal(bits(ov), bits(var))
    # the device entry: null buffers, a feature buffer off its 16 bytes, rgb or variance off their 4
    d_rgb, d_var = torch.from_numpy(rgb.copy()).cuda(), torch.from_numpy(var.copy()).cuda()
    d_feat = torch.from_numpy(np.concatenate([feat.view(np.float32).reshape(-1), np.zeros(4, np.float32)])).cuda()
    torch.cuda.synchronize()
    f, c, v = d_feat.data_ptr(), d_rgb.data_ptr(), d_var.data_ptr()
    fd = lib.rtx_denoise_variance_device
    for args in ((None, c, v), (f, None, v), (f, c, None), (f + 4, c, v), (f, c + 2, v), (f, c, v + 1)):
        assert fd(r._ctx, W, H, P, *args, None) == abi.RTX_ERR_ARG, args
    assert fd(r._ctx, W, H, None, f, c, v, None) == abi.RTX_ERR_ARG
    assert fd(r._ctx, W, H, ctypes.byref(bad), f, c, v, None) == abi.RTX_ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(rgb)) and np.array_equal(bits(d_var.cpu().numpy()), bits(var))
    with pytest.raises(ValueError):
        r.denoise_variance(rgb, var[:-1], feat)


# ---- 2. quality ----
SCENE3_RATIO = 1.0271  # measured on the device with the shipped defaults (sigma_color 3, 1 level)


def mse_over_hits(x, ref, hit):
    return float(((x[hit].astype(np.float64) - ref[hit]) ** 2).mean())


@pytest.mark.parametrize("name,w,h", [("scene1", 128, 128), ("scene3", 128, 72)])
def test_filtered_mean_of_4_passes_against_1024spp(world, name, w, h):
    """render_passes(-g path -n 1, passes=4, seed=11) filtered with the shipped defaults, against render(-n 1024,
    seed=2024): the ratio of the mean squared errors over hit pixels, filtered / unfiltered.  scene1 must improve.
    scene3's ratio is asserted against the value measured on the device (SCENE3_RATIO) times 1.1: the run is
    deterministic and the margin covers float-rounding drift across compiler versions only.  Measured: 0.8999 on
    scene1 and 1.0271 on scene3, which this filter does NOT improve (no sigma_color in 0.5..4 with 1..3 levels did:
    1.027..1.033), beside rtx_denoise's 0.9970 and 0.4539 on the same means.  95-99 % of these
    frames' squared error sits in 1 % of the pixels, so large gains are not to be had here."""
    mean, z, var, ref, feat = world.quality_frames(name, w, h)
    r = world.renderer(name)
    out, ov = r.denoise_variance(mean, var, feat)
    plain = r.denoise(mean, feat)
    hit = z != 0
    assert hit.any() and np.isfinite(mean).all() and np.isfinite(out).all() and np.isfinite(ov).all() and (ov >= 0).all()
    m0, m1, m2 = (mse_over_hits(x, ref, hit) for x in (mean, out, plain))
    print(f"{name} {w}x{h}: mse of the mean {m0:.5e}, variance-guided {m1:.5e} (ratio {m1 / m0:.4f}), "
          f"rtx_denoise {m2:.5e} (ratio {m2 / m0:.4f})")
    assert np.array_equal(bits(out)[~hit], bits(mean)[~hit]) and np.array_equal(bits(ov)[~hit], bits(var)[~hit])
    assert not np.array_equal(bits(out), bits(mean))
    if name == "scene1":
        assert m1 < m0, (m1, m0)
    else:
        assert m1 <= SCENE3_RATIO * 1.1 * m0, (m1 / m0, SCENE3_RATIO)


# ---- 3. composition with adaptive passes ----
def test_an_adaptive_renders_mean_and_variance_need_nothing_special(world):
    """tiles of one frame that received different numbers of passes: one level on the device's own outputs equals
    the model within the bounds above"""
    scene, r = world.scene("scene1"), world.renderer("scene1")
    frame = scene.frame(64, 64)
    mean, z, var, n_t = r.render_adaptive(frame, rtxpy.params_from_args(PATH1, seed=11), 16, float(np.float32(0.01)), jitter=True)
    assert n_t.min() < n_t.max()
    feat = r.features(frame)
    src = (mean, var)
    live = VM.live_mask(mean, var, feat)
    assert live.sum() == (z != 0).sum() > 0
    sig = {"sigma_" + t: abi.DENOISE_VARIANCE_DEFAULTS["sigma_" + t] for t in VM.TERMS}
    out = r.denoise_variance(mean, var, feat, iterations=1, **sig)
    gc, gv, mc, mv = gaps(out, VM.level(mean, var, feat, 0, sig), src, feat, "adaptive scene1 64x64")
    assert gc <= BOUND and gv <= BOUND
    assert mc > 2 * BOUND and mv > 2 * BOUND
    assert np.array_equal(bits(out[0])[~live], bits(mean)[~live]) and np.array_equal(bits(out[1])[~live], bits(var)[~live])
