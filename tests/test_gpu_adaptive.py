"""Adaptive passes on the GPU (rtx_render_adaptive*, csrc/rtx_adaptive.hip).

The target tau is the error the existing rtx_render_passes reports after 8 full passes of the same settings, so it
comes from code this file does not test.  The model: with the device's per-tile pass counts n_t and passes run R,
pass k re-rendered by render_tiles on {t : n_t > k} and folded by float64 Welford over each tile's first n_t
frames.  The device's state is double and takes the same operations, so rgb and variance are one float rounding of
it (2 float ulps, the bound of test_gpu_passes); z is pass 0's; the ray counts are the re-renders' sum.  Then every
decision is replayed in float64: a tile that went on was over the threshold, one that stopped was at or under it
(a comparison whose sides differ by less than 1e-9 relative is not judged: the device's fixed summation order
differs from numpy's by about 1e-14).
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
MODES = {"plain": {}, "jitter": {"jitter": True}}
SCENES = {"scene1": "scene1.json", "scene5_standin": "scene5_standin.json"}
PASSES, MIN_PASSES = 24, 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def path_params(**kw):
    return rtxpy.params_from_args(PATH, **{"seed": SEED, **kw})


def within_ulps(got, want64, ulps=2):
    want = want64.astype(np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)).astype(np.float64))


class World:
    def __init__(self):
        self.scenes, self.ctx, self.runs = {}, {}, {}

    def renderer(self, name):
        if name not in self.ctx:
            if "standin" in name:
                import standins
                standins.ensure_scene(name.split("_standin")[0])
            self.scenes[name] = rtxpy.Scene.load(os.path.join(C.SCENES, SCENES[name]), base_dir=C.GOLDEN)
            r = rtxpy.Renderer(0)
            r.upload(self.scenes[name])
            self.ctx[name] = r
        return self.ctx[name], self.scenes[name]

    def tau(self, name, w, h, mode):
        """the error rtx_render_passes reports after 8 full passes"""
        r, scene = self.renderer(name)
        r.render_passes(scene.frame(w, h), path_params(), 8, **MODES[mode])
        return float(np.float32(r.pass_stats().error))

    def run(self, name, w, h, mode, passes=PASSES, min_passes=MIN_PASSES):
        """one adaptive run and its model, made once: nothing changes the arrays"""
        key = (name, w, h, mode, passes, min_passes)
        if key not in self.runs:
            r, scene = self.renderer(name)
            tau = self.tau(name, w, h, mode) or 1e-3  # a frame without noise: any target stops it at min_passes
            out = r.render_adaptive(scene.frame(w, h), path_params(), passes, tau, min_passes=min_passes, **MODES[mode])
            st = r.adaptive_stats()
            self.runs[key] = (tau, out, st, model(r, scene.frame(w, h), mode, passes, out[3], st.passes_run))
        return self.runs[key]

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


def model(r, frame, mode, passes, n_t, R):
    """float64 Welford over render_tiles' frames of {t : n_t > k}, k < R.  Returns mean, m2 (h, w, 3), pass 0's z, the
    re-renders' ray counts, and after every pass j = 1..R the per-tile V_t and S_t (index j - 1)."""
    w, h = frame.width, frame.height
    ty, tx = n_t.shape
    n_px = np.kron(n_t, np.ones((8, 8), np.uint32))[:h, :w]  # each pixel's tile's count
    tile_of = np.kron(np.arange(ty * tx).reshape(ty, tx), np.ones((8, 8), np.int64))[:h, :w]
    mean, m2 = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    z0, closest, shadow, V, S = None, 0, 0, [], []
    for k in range(R):
        tiles = np.flatnonzero(n_t.ravel() > k).astype(np.uint32)
        fk = rtxpy.pass_frame(frame, k, passes=passes, **MODES[mode])
        rgb, z = r.render_tiles(fk, path_params(seed=SEED + k), tiles)
        st = r.stats()
        closest, shadow = closest + st.closest_rays, shadow + st.shadow_rays
        if k == 0:
            z0 = z
        act = n_px > k
        x = rgb.astype(np.float64)[act]
        d = x - mean[act]
        mean[act] += d / (k + 1)
        m2[act] += d * (x - mean[act])
        n_now = np.minimum(n_px, k + 1).astype(np.float64)[..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            var = np.where(n_now > 1, m2 / (n_now * (n_now - 1)), 0.0)
        ok = np.isfinite(mean).all(axis=-1)
        V.append(np.bincount(tile_of[ok], var[ok].sum(axis=-1), ty * tx))
        S.append(np.bincount(tile_of[ok], np.abs(mean[ok]).sum(axis=-1), ty * tx))
    n = n_px.astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(n > 1, m2 / (n * (n - 1)), 0.0)
    return dict(mean=mean, var=var, z=z0, closest=closest, shadow=shadow, V=V, S=S)


def check_against_model(run, passes, min_passes):
    tau, (rgb, z, var, n_t), st, m = run
    R, T = st.passes_run, n_t.size
    print(f"tau {tau:.6g}: R {R}, sum n_t {int(n_t.sum())} of {R * T}, counts {np.bincount(n_t.ravel())[min(min_passes, R):]}")
    assert st.tiles == T and st.tile_passes == int(n_t.sum())
    assert min(min_passes, R) <= n_t.min() and n_t.max() == R and R <= passes
    assert within_ulps(rgb, m["mean"]) and within_ulps(var, m["var"])
    assert np.array_equal(bits(z), bits(m["z"]))
    assert (st.closest_rays, st.shadow_rays) == (m["closest"], m["shadow"])
    V, A = m["V"][R - 1].sum(), m["S"][R - 1].sum()
    want = np.sqrt(V) / A if A else 0.0
    assert abs(st.error - want) <= 1e-9 * want
    # the rule, replayed for every tile after j = min_passes .. R passes
    judged = unjudged = 0
    n = n_t.ravel()
    for j in range(min_passes, R + 1):
        lhs, rhs = m["V"][j - 1] * T, (tau * tau) * m["S"][j - 1].sum() ** 2
        close = np.abs(lhs - rhs) < 1e-9 * np.maximum(np.abs(lhs), rhs)
        went_on, stopped = n > j, (n == j) & (j < passes)  # after the last pass of `passes` nothing is decided
        unjudged += int((close & (went_on | stopped)).sum())
        judged += int((went_on | stopped).sum())
        assert np.all(lhs[went_on & ~close] > rhs), j
        assert np.all(lhs[stopped & ~close] <= rhs), j
    assert unjudged <= 0.01 * judged
    return judged


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name,w,h", [("scene1", 64, 64), ("scene5_standin", 64, 40)])
def test_adaptive_is_its_model_and_spends_its_passes_unevenly(world, name, w, h, mode):
    run = world.run(name, w, h, mode)
    tau, (rgb, z, var, n_t), st, m = run
    assert tau > 0
    judged = check_against_model(run, PASSES, MIN_PASSES)
    R, T = st.passes_run, n_t.size
    # what keeps the checks above from passing on a run that decided nothing
    assert judged > 0 and n_t.min() < n_t.max() and int(n_t.sum()) < R * T
    r, scene = world.renderer(name)
    r.render_passes(scene.frame(w, h), path_params(), R, **MODES[mode])
    full = r.pass_stats()
    assert full.passes_run == R and st.shadow_rays < full.shadow_rays


@pytest.mark.parametrize("w,h", [(17, 33), (1, 1)])
def test_shapes(world, w, h):
    """tiles cut by both edges, and one pixel"""
    check_against_model(world.run("scene1", w, h, "jitter"), PASSES, MIN_PASSES)


def test_two_runs_give_the_same_bits_and_counts(world):
    r, scene = world.renderer("scene1")
    tau, a, sa, _ = world.run("scene1", 64, 64, "jitter")
    b = r.render_adaptive(scene.frame(64, 64), path_params(), PASSES, tau, min_passes=MIN_PASSES, jitter=True)
    sb = r.adaptive_stats()
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert (sa.passes_run, sa.tile_passes, sa.error, sa.closest_rays, sa.shadow_rays) == \
        (sb.passes_run, sb.tile_passes, sb.error, sb.closest_rays, sb.shadow_rays)
    assert sb.render_ms > 0 and sb.fold_ms > 0


def test_every_pass_for_every_tile_is_render_passes(world):
    """passes == min_passes: no tile stops early, and the mean and variance are render_passes' with no target"""
    r, scene = world.renderer("scene1")
    frame = scene.frame(37, 29)
    rgb, z, var, n_t = r.render_adaptive(frame, path_params(), 5, 1e-6, min_passes=5, jitter=True)
    st = r.adaptive_stats()
    assert np.all(n_t == 5) and n_t.shape == (4, 5) and st.passes_run == 5 and st.tile_passes == 100
    want = r.render_passes(frame, path_params(), 5, jitter=True)
    ps = r.pass_stats()
    assert within_ulps(rgb, want[0].astype(np.float64)) and within_ulps(var, want[2].astype(np.float64))
    assert np.array_equal(bits(z), bits(want[1]))
    assert (st.closest_rays, st.shadow_rays) == (ps.closest_rays, ps.shadow_rays)
    assert abs(st.error - ps.error) <= 1e-9 * ps.error
    # a target nothing misses: every tile stops at min_passes
    r.render_adaptive(frame, path_params(), 9, 1e30, min_passes=2, jitter=True)
    assert r.adaptive_stats().passes_run == 2 and r.adaptive_stats().tile_passes == 40


def test_null_outputs(world):
    r, scene = world.renderer("scene1")
    frame, p = scene.frame(37, 29), path_params()
    tau = world.tau("scene1", 37, 29, "jitter")
    want = r.render_adaptive(frame, p, 12, tau, min_passes=3, jitter=True)
    pp = rtxpy.pass_params(passes=12, jitter=True, target_error=tau, min_passes=3)
    f, q, o = ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp)
    for keep in range(4):
        out = [np.full(x.shape, 0x7FE5C3E1, np.uint32).view(x.dtype) for x in want]
        ptr = [x.ctypes.data if i == keep else None for i, x in enumerate(out)]
        assert r.lib.rtx_render_adaptive(r._ctx, f, q, o, *ptr) == abi.RTX_OK
        assert np.array_equal(bits(out[keep]), bits(want[keep]))
    assert r.lib.rtx_render_adaptive(r._ctx, f, q, o, None, None, None, None) == abi.RTX_OK
    assert r.adaptive_stats().tile_passes == int(want[3].sum())


def test_device_entry_equals_the_host_entry_and_stays_in_bounds(world):
    import torch
    r, scene = world.renderer("scene1")
    frame, n, T, guard = scene.frame(37, 29), 37 * 29, 20, 64
    tau = world.tau("scene1", 37, 29, "jitter")
    want = r.render_adaptive(frame, path_params(), 12, tau, min_passes=3, jitter=True)
    sizes = (3 * n, n, 3 * n, T)
    for stream in (None, torch.cuda.Stream()):
        bufs = [torch.full((words + guard,), 7.5, dtype=torch.float32, device="cuda") for words in sizes]
        torch.cuda.synchronize()
        r.render_adaptive_device(frame, path_params(), 12, tau, *[b.data_ptr() for b in bufs], min_passes=3, jitter=True,
                                 stream=stream.cuda_stream if stream else None)
        for b, words, x in zip(bufs, sizes, want):
            host = b.cpu().numpy()
            assert np.array_equal(bits(host[:words]), bits(x).ravel())
            assert np.all(host[words:] == 7.5)  # the guard words right after the buffer
    d = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_adaptive_device(frame, path_params(), 12, tau, d.data_ptr(), None, None, None, min_passes=3, jitter=True)
    assert np.array_equal(bits(d.cpu().numpy()), bits(want[0]).ravel())
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_adaptive_device(frame, path_params(), 12, tau, d.data_ptr() + 4, None, None, None, min_passes=3)
    assert e.value.code == abi.RTX_ERR_ARG


def test_argument_errors(world):
    r, scene = world.renderer("scene1")
    frame = scene.frame(64, 64)
    before = r.render(frame, path_params())
    r.render_adaptive(frame, path_params(), 4, 1e30)
    kept = r.adaptive_stats()
    for bad in (dict(target_error=0.0), dict(target_error=-1e-3), dict(target_error=float("nan")), dict(passes=0),
                dict(passes=1), dict(min_passes=1), dict(min_passes=5), dict(aperture=-1.0), dict(aperture=0.1, focus=0.0)):
        kw = {"passes": 4, "target_error": 0.01, **bad}
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_adaptive(frame, path_params(), kw.pop("passes"), kw.pop("target_error"), **kw)
        assert e.value.code == abi.RTX_ERR_ARG, bad
    for shard in (dict(tile_stride=2), dict(tile_stride=2, tile_offset=1), dict(tile_stride=0)):
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_adaptive(frame, path_params(**shard), 4, 0.01)
        assert e.value.code == abi.RTX_ERR_ARG
    pp = rtxpy.pass_params(passes=4, flags=2, target_error=0.01)
    p = path_params()
    assert r.lib.rtx_render_adaptive(r._ctx, ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), None, None, None,
                                     None) == abi.RTX_ERR_ARG  # an unknown pass flag
    empty = abi.Frame.from_buffer_copy(bytes(frame))
    empty.width = 0
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_adaptive(empty, path_params(), 4, 0.01)
    assert e.value.code == abi.RTX_ERR_ARG
    fresh = rtxpy.Renderer(0)
    try:
        with pytest.raises(rtxpy.RtxError) as e:
            fresh.render_adaptive(frame, path_params(), 4, 0.01)
        assert e.value.code == abi.RTX_ERR_STATE
    finally:
        fresh.close()
    after = r.render(frame, path_params())  # the context is unharmed, and the refused calls left the statistics
    assert np.array_equal(bits(after[0]), bits(before[0])) and np.array_equal(bits(after[1]), bits(before[1]))
    st = r.adaptive_stats()
    assert (st.passes_run, st.tile_passes) == (kept.passes_run, kept.tile_passes) == (2, 128)
