"""Multi-pass rendering on the GPU (csrc/rtx_passes.hip through rtx_render_passes*).

A pass is a render: the mean and the variance of the mean against float64 Welford over the frames Renderer.render
gives for rtx_pass_frame(k) and seed + k, to one float rounding.  Then determinism, the device entry with guard
words, null outputs, frame shapes, anti-aliasing against a supersampled reference, the stopping rule against the
test's own error, statistics and the argument errors.
"""
import ctypes
import os

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

SEED = 11
PATH = ["-g", "path", "-n", "1"]
MODES = {
    "plain": {},
    "jitter": {"jitter": True},
    "lens": {"aperture": 0.2, "focus": 4.0},
    "jitter+lens": {"jitter": True, "aperture": 0.2, "focus": 4.0},
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def path_params(**kw):
    return rtxpy.params_from_args(PATH, **{"seed": SEED, **kw})


class World:
    """scenes, contexts and single renders, each made once and shared (no test changes a shared array)"""

    def __init__(self):
        self.scenes, self.ctx, self.singles = {}, {}, {}

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

    def single(self, name, w, h, mode, k):
        """pass k on its own: Renderer.render of rtx_pass_frame(k) with seed + k -> (rgb, z, closest, shadow rays)"""
        key = (name, w, h, mode, k)
        if key not in self.singles:
            r = self.renderer(name)
            fk = rtxpy.pass_frame(self.scene(name).frame(w, h), k, passes=k + 1, **MODES[mode])
            rgb, z = r.render(fk, path_params(seed=SEED + k))
            st = r.stats()
            self.singles[key] = (rgb, z, st.closest_rays, st.shadow_rays)
        return self.singles[key]

    def close(self):
        for r in self.ctx.values():
            r.close()
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def welford(frames):
    """float64 Welford over the frames, in order: (mean, m2)"""
    mean = np.zeros(frames[0].shape, np.float64)
    m2 = np.zeros(frames[0].shape, np.float64)
    for k, x in enumerate(frames):
        x = x.astype(np.float64)
        d = x - mean
        mean = mean + d / (k + 1)
        m2 = m2 + d * (x - mean)
    return mean, m2


def error_of(mean, m2, n):
    """E = sqrt(sum var_mean) / sum |mean| over the pixels with a finite mean, in float64"""
    if n < 2:
        return 0.0
    ok = np.isfinite(mean).all(axis=-1)
    den = np.abs(mean[ok]).sum()
    return float(np.sqrt((m2[ok] / (n * (n - 1))).sum()) / den) if den else 0.0


def within_ulps(got, want64, ulps=2):
    want = want64.astype(np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64))


def check_against_renders(world, name, w, h, mode, K):
    """render_passes against float64 Welford over the K single renders.  The device's state is double and takes
    the same operations, so its mean and m2 carry about K 2^-53 relative error and the outputs are one float
    rounding of them: 2 float ulps bound both (derived, not measured)."""
    frames = [world.single(name, w, h, mode, k) for k in range(K)]
    rgb, z, var = world.renderer(name).render_passes(world.scene(name).frame(w, h), path_params(), K, **MODES[mode])
    st = world.renderer(name).pass_stats()
    mean, m2 = welford([f[0] for f in frames])
    assert st.passes_run == K
    assert np.array_equal(bits(z), bits(frames[0][1]))
    assert within_ulps(rgb, mean)
    if K == 1:
        assert np.array_equal(bits(rgb), bits(frames[0][0]))
        assert not var.any() and st.error == 0.0
    else:
        assert within_ulps(var, m2 / (K - 1) / K)
        assert var.any()
        e = error_of(mean, m2, K)
        assert abs(st.error - e) <= 1e-9 * e
    assert st.closest_rays == sum(f[2] for f in frames) and st.shadow_rays == sum(f[3] for f in frames)
    return rgb, z, var


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,w,h", [("scene1", 64, 64), ("scenetest", 64, 36)])
def test_a_pass_is_a_render(world, name, w, h, mode, K):
    check_against_renders(world, name, w, h, mode, K)


def test_the_modes_differ(world):
    """jitter moves the samples and the lens moves the origin: the passes after the first are other frames"""
    k1 = {m: world.single("scene1", 64, 64, m, 1)[0] for m in MODES}
    for a in MODES:
        for b in MODES:
            if a < b:
                assert not np.array_equal(bits(k1[a]), bits(k1[b])), (a, b)
    k0 = [world.single("scene1", 64, 64, m, 0)[0] for m in ("plain", "jitter")]
    assert np.array_equal(bits(k0[0]), bits(k0[1]))  # pass 0 with a pinhole is the frame itself


@pytest.mark.parametrize("w,h", [(1, 1), (17, 33), (300, 2)])
def test_shapes(world, w, h):
    """the grid tail, fewer pixels than a block, more than one block: K = 3 with jitter and a lens"""
    check_against_renders(world, "scene1", w, h, "jitter+lens", 3)


def test_two_runs_give_the_same_bits(world):
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(64, 64)
    for kw in ({}, {"target_error": 2.5e-3, "min_passes": 2}):
        a = r.render_passes(frame, path_params(), 6, jitter=True, **kw)
        na = r.pass_stats()
        b = r.render_passes(frame, path_params(), 6, jitter=True, **kw)
        nb = r.pass_stats()
        assert (na.passes_run, na.error) == (nb.passes_run, nb.error) and na.passes_run >= 2 and na.error > 0
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y))


def test_device_entry_equals_the_host_entry_and_stays_in_bounds(world):
    import torch
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(37, 29)
    n, guard = 37 * 29, 64
    want = r.render_passes(frame, path_params(), 3, jitter=True, aperture=0.2, focus=4.0)
    bufs = [torch.full((words + guard,), 7.5, dtype=torch.float32, device="cuda") for words in (3 * n, n, 3 * n)]
    torch.cuda.synchronize()
    r.render_passes_device(frame, path_params(), 3, *[b.data_ptr() for b in bufs], jitter=True, aperture=0.2, focus=4.0)
    for b, words, w in zip(bufs, (3 * n, n, 3 * n), want):
        host = b.cpu().numpy()
        assert np.array_equal(bits(host[:words]), bits(w).ravel())
        assert np.all(host[words:] == 7.5)  # the guard words right after the buffer
    # a stream of the caller's
    s = torch.cuda.Stream()
    d = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_passes_device(frame, path_params(), 3, d.data_ptr(), None, None, stream=s.cuda_stream, jitter=True, aperture=0.2,
                           focus=4.0)
    assert np.array_equal(bits(d.cpu().numpy()), bits(want[0]).ravel())
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_passes_device(frame, path_params(), 3, d.data_ptr() + 4, None, None)
    assert e.value.code == abi.RTX_ERR_ARG


def test_null_outputs(world):
    r, frame = world.renderer("scene1"), world.scene("scene1").frame(37, 29)
    want = r.render_passes(frame, path_params(), 3, jitter=True)
    pp, p = rtxpy.pass_params(passes=3, jitter=True), path_params()
    for keep in range(3):
        out = [np.full(w.shape, 7.5, np.float32) for w in want]
        ptr = [o.ctypes.data if i == keep else None for i, o in enumerate(out)]
        assert r.lib.rtx_render_passes(r._ctx, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), *ptr) == abi.RTX_OK
        assert np.array_equal(bits(out[keep]), bits(want[keep]))
    assert r.lib.rtx_render_passes(r._ctx, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), None, None, None) == abi.RTX_OK
    assert r.pass_stats().passes_run == 3


def supersampled(frame, s):
    """the s x s supersampled frame whose samples tile the pixels' footprints: column c samples corner + (c+1)
    step_x but row r samples corner + r step_y, so pixel (c, r) covers corner + (c+1 +- 1/2) step_x + (r +- 1/2)
    step_y, and the fine frame's corner moves by +(1/2 - 1/(2s)) step_x and -(1/2 - 1/(2s)) step_y"""
    f = abi.Frame.from_buffer_copy(bytes(frame))
    c, sx, sy = (np.array(list(getattr(frame, k)), np.float64) for k in ("corner", "step_x", "step_y"))
    o = 0.5 - 1.0 / (2 * s)
    f.width, f.height = frame.width * s, frame.height * s
    f.corner = abi.F3(*(c + o * sx - o * sy).astype(np.float32))
    f.step_x = abi.F3(*(sx / s).astype(np.float32))
    f.step_y = abi.F3(*(sy / s).astype(np.float32))
    return f


@pytest.mark.parametrize("name,w,h", [("scene1", 64, 64), ("scene3", 64, 36), ("scenetest", 64, 36)])
def test_anti_aliasing(world, name, w, h):
    """noise-free frames (ambient GI, constant RNG): the mean of 16 jittered passes has at most a quarter of the
    one-ray frame's squared error against the 8 x 8 supersampled box reference.  The CPU oracle alone gives
    0.030 / 0.053 / 0.085 and the device 0.0302 / 0.0531 / 0.0849; 0.25 leaves 3x for the device's float differences at
    edges."""
    r, frame = world.renderer(name), world.scene(name).frame(w, h)
    p = rtxpy.default_params(rng=abi.RTX_RNG_CONST)
    fine, _ = r.render(supersampled(frame, 8), p)
    ref = fine.astype(np.float64).reshape(h, 8, w, 8, 3).mean(axis=(1, 3))
    one, _ = r.render(frame, p)
    aa, _, _ = r.render_passes(frame, p, 16, jitter=True)
    e = lambda x: float(((x.astype(np.float64) - ref) ** 2).mean())  # noqa: E731
    ratio = e(aa) / e(one)
    print(f"anti-aliasing {name} {w}x{h}: e(16 jittered passes) / e(one ray) = {ratio:.4f} (e(one ray) = {e(one):.4g})")
    assert e(one) > 0 and ratio <= 0.25


def test_stopping_rule(world):
    """the error after every pass in float64 from the single renders; a target between two consecutive values
    stops exactly where the test's own error first falls to it"""
    r, frame, K = world.renderer("scene1"), world.scene("scene1").frame(64, 64), 12
    frames = [world.single("scene1", 64, 64, "plain", k)[0] for k in range(K)]
    E = [error_of(*welford(frames[:n]), n) for n in range(1, K + 1)]  # E[n-1]: after n passes
    print("E after 1..12 passes:", " ".join(f"{e:.6g}" for e in E))
    pair = next(i for i in range(3, K - 1) if abs(E[i] - E[i + 1]) >= 0.01 * max(E[i], E[i + 1]))
    target = float(np.float32(np.sqrt(E[pair] * E[pair + 1])))
    for min_passes in (2, 9):
        want_n = next((n for n in range(min_passes, K + 1) if E[n - 1] <= target), K)
        assert want_n < K  # the rule stops this run early
        rgb, z, var = r.render_passes(frame, path_params(), K, target_error=target, min_passes=min_passes)
        st = r.pass_stats()
        assert st.passes_run == want_n, (st.passes_run, want_n, min_passes)
        assert abs(st.error - E[want_n - 1]) <= 1e-9 * E[want_n - 1]
        plain = r.render_passes(frame, path_params(), want_n)
        for x, y in zip((rgb, z, var), plain):
            assert np.array_equal(bits(x), bits(y))
    r.render_passes(frame, path_params(), K, target_error=1e30, min_passes=3)
    assert r.pass_stats().passes_run == 3
    r.render_passes(frame, path_params(), K, target_error=0.0, min_passes=3)
    st = r.pass_stats()
    assert st.passes_run == K and abs(st.error - E[K - 1]) <= 1e-9 * E[K - 1]


def test_statistics_and_errors(world):
    r, scene = world.renderer("scene1"), world.scene("scene1")
    frame = scene.frame(64, 64)
    before, zb = r.render(frame, path_params())
    r.render_passes(frame, path_params(), 4, jitter=True)
    st, last = r.pass_stats(), r.stats()
    singles = [world.single("scene1", 64, 64, "jitter", k) for k in range(4)]
    assert st.passes_run == 4 and st.closest_rays == sum(s[2] for s in singles) and st.shadow_rays == sum(s[3] for s in singles)
    assert st.render_ms > 0 and st.accum_ms > 0 and st.error > 0
    assert (last.closest_rays, last.shadow_rays) == singles[3][2:]  # rtx_get_stats describes the last pass
    for bad in (dict(tile_stride=2), dict(tile_stride=2, tile_offset=1), dict(tile_stride=0)):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_passes(frame, path_params(**bad), 2)
        assert e.value.code == abi.RTX_ERR_ARG
    for bad in (dict(passes=0), dict(passes=2, aperture=-1.0), dict(passes=2, target_error=0.1, min_passes=3)):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_passes(frame, path_params(), **bad)
        assert e.value.code == abi.RTX_ERR_ARG
    empty = abi.Frame.from_buffer_copy(bytes(frame))
    empty.width = 0
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_passes(empty, path_params(), 2)
    assert e.value.code == abi.RTX_ERR_ARG
    fresh = rtxpy.Renderer(0)
    try:
        with pytest.raises(rtxpy.RtxError) as e:
            fresh.render_passes(frame, path_params(), 2)
        assert e.value.code == abi.RTX_ERR_STATE
    finally:
        fresh.close()
    # the context is left unharmed: the same frame as before, and the statistics of the refused calls' predecessor
    after, za = r.render(frame, path_params())
    assert np.array_equal(bits(after), bits(before)) and np.array_equal(bits(za), bits(zb))
    assert r.pass_stats().passes_run == 4
