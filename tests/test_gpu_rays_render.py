"""Renders of a caller's rays on the GPU (rtx_render_rays*, rtx_ray_features*, the k_trace<.., RAYS> instances).

A frame's own rays render to rtx_render's image bit for bit; a batch that mixes three cameras gives every pixel its own
camera's pixel; a pixel depends on its own record alone (holes, a NaN direction, a permutation under the constant
RNG); z is the ray queries' t and the feature records are the frame features'; shards, the device entry with guard
words and a stream, and the next plain render's chunk sizing left alone.
"""
import os

import numpy as np
import pytest

import conftest as C
import rays_frames
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FE5C3E1  # a quiet NaN with a payload: no render writes these bits
# objects tested one by one; the 8-wide tree with a transparent mesh; reflective and transparent materials (kr, kt)
SCENES = {"scene1": "scene1.json", "scene5_standin": "scene5_standin.json", "scenetest2": "scenetest2.json"}
PARAMS = {"ambient": [], "path1": ["-g", "path", "-n", "1"], "path2": ["-g", "path", "-n", "2"]}
FRAMES = [(17, 33), (1, 1), (64, 64), (300, 2)]
# per-ray sums; the wave-level counters (tests/test_gpu_build.py: shadow_wave_steps, shadow_leaf_rounds,
# shadow_uniform_steps, shadow_wave_walks) follow which shade points share a k_shadow wave
COUNTERS = ("closest_rays", "shadow_rays", "node_visits", "tri_tests", "sphere_tests", "shadow_box_tests",
            "shadow_tri_tests", "shade_points", "far_closest_rays")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def params(mode, **kw):
    return rtxpy.params_from_args(PARAMS[mode], **{"seed": 5, **kw})


class World:
    def __init__(self):
        self.scenes, self.ctx, self.full = {}, {}, {}

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

    def whole(self, name, mode, w, h):
        """Renderer.render of the scene's own frame, once; nothing changes it"""
        key = (name, mode, w, h)
        if key not in self.full:
            r, scene = self.renderer(name)
            self.full[key] = r.render(scene.frame(w, h), params(mode))
        return self.full[key]

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


def frame_rays(r, frame):
    """the frame's own rays (rtx_frame_rays_device) as a device tensor of 8 words per ray"""
    import torch
    buf = torch.zeros((frame.width * frame.height, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.frame_rays_device(frame, buf.data_ptr())
    return buf


def records(buf):
    return buf.cpu().numpy().view(abi.RAY_DTYPE).reshape(-1)


def render_rays_device(r, w, h, buf, p, fill=0.0):
    import torch
    rgb = torch.full((h * w * 3,), fill, dtype=torch.float32, device="cuda")
    z = torch.full((h * w,), fill, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_rays_device(w, h, buf.data_ptr(), p, rgb.data_ptr(), z.data_ptr())
    return rgb.cpu().numpy().reshape(h, w, 3), z.cpu().numpy().reshape(h, w)


# ---------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("mode", sorted(PARAMS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_frames_own_rays_render_to_the_frames_image(world, name, mode, w, h):
    r, scene = world.renderer(name)
    frame = scene.frame(w, h)
    got = render_rays_device(r, w, h, frame_rays(r, frame), params(mode))
    assert same(got, world.whole(name, mode, w, h))
    # the host entry takes the same path
    assert same(r.render_rays(records(frame_rays(r, frame)), params=params(mode), shape=(h, w)), world.whole(name, mode, w, h))


@pytest.mark.parametrize("mode", sorted(PARAMS))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_identity_of_the_counting_instances(world, name, mode):
    r, scene = world.renderer(name)
    w, h = 17, 33
    frame, p = scene.frame(w, h), params(mode, count_traversal=1)
    a = r.render(frame, p)
    sa = r.stats()
    b = render_rays_device(r, w, h, frame_rays(r, frame), p)
    sb = r.stats()
    assert same(a, b) and same(a, world.whole(name, mode, w, h))
    for f in COUNTERS:
        assert getattr(sa, f) == getattr(sb, f), (f, getattr(sa, f), getattr(sb, f))
    assert sa.closest_rays > 0 and sa.node_visits + sa.sphere_tests > 0


@pytest.mark.parametrize("pack", [0, 1])
@pytest.mark.parametrize("mode", ["path1", "path2"])
def test_identity_with_and_without_the_packed_walk(world, mode, pack):
    r, scene = world.renderer("scene5_standin")
    full = [world.whole("scene5_standin", mode, w, h) for w, h in ((17, 33), (64, 64))]
    r.set_option(abi.RTX_OPT_TRACE_PACK, pack)
    try:
        for (w, h), want in zip(((17, 33), (64, 64)), full):
            frame = scene.frame(w, h)
            for count in (0, 1):
                assert same(render_rays_device(r, w, h, frame_rays(r, frame), params(mode, count_traversal=count)), want)
    finally:
        r.set_option(abi.RTX_OPT_TRACE_PACK, 1)


@pytest.mark.parametrize("option,value", [(abi.RTX_OPT_CHUNK_TILES, 3), (abi.RTX_OPT_SP_PER_TILE, 1)])
@pytest.mark.parametrize("name", ["scene1", "scene5_standin"])
def test_identity_in_small_chunks_and_through_the_overflow_retry(world, name, option, value):
    """chunks of 3 tiles, and chunks sized for one shade point per tile, which overflow and halve (576 tiles, as
    test_gpu_tiles.py)"""
    r, scene = world.renderer(name)
    w, h = 256, 144
    want = world.whole(name, "path1", w, h)  # rendered before the option is set
    frame = scene.frame(w, h)
    rays = frame_rays(r, frame)
    r.set_option(option, value)
    try:
        got = render_rays_device(r, w, h, rays, params("path1"))
        chunks = r.stats().chunks
    finally:
        r.set_option(option, 0)
    assert chunks == 576 // 3 if option == abi.RTX_OPT_CHUNK_TILES else chunks > 1
    assert same(got, want)


# ---------------------------------------------------------------------------------------------- 2. mixed cameras
def far_frame(name, dist, w, h):
    """rays_frames.far_frame at another size: from `dist` scene radii out (DESIGN §2.1's far-origin cases)"""
    lo, hi = (np.array(v, np.float64) for v in rays_frames.BOUNDS[name])
    c, e = 0.5 * (lo + hi), hi - lo
    g = [[c[0] + sx * 0.6 * e[0], c[1] + sy * 0.6 * e[1], c[2]] for sx, sy in ((-1, -1), (1, -1), (-1, 1))]
    return rays_frames.grid_frame(c - [0.0, 0.0, dist * 0.5 * e.max()], *g, w=w, h=h)


def resized(fr, w, h):
    """the frame that looks at fr's target grid with w x h pixels (a camera moved and turned: rays_frames' inside frame)"""
    c, sx, sy = (np.array(v[:], np.float64) for v in (fr.corner, fr.step_x, fr.step_y))
    p00 = c + sx
    return rays_frames.grid_frame(fr.origin[:], p00, p00 + fr.width * sx, p00 + fr.height * sy, w=w, h=h)


@pytest.mark.parametrize("dist", [60.0, 2000.0])
@pytest.mark.parametrize("mode", ["ambient", "path1"])
@pytest.mark.parametrize("name,bounds", [("scene1", "scene1"), ("scene5_standin", "scene5")])
def test_three_cameras_in_one_batch(world, name, bounds, mode, dist):
    """pixel i takes camera i mod 3's ray: it is that camera's own pixel i, since the RNG keys on (seed, pixel index)
    alone; lanes of one wave then start from three origins, one of them far"""
    r, scene = world.renderer(name)
    w, h = 33, 17
    cams = [scene.frame(w, h), resized(rays_frames.handmade_frames(bounds)[0], w, h), far_frame(bounds, dist, w, h)]
    p = params(mode)
    own = [r.render(f, p) for f in cams]
    recs = [records(frame_rays(r, f)) for f in cams]
    pick = np.arange(w * h) % 3
    batch = recs[0].copy()
    for k in (1, 2):
        batch[pick == k] = recs[k][pick == k]
    rgb, z = r.render_rays(batch, params=p, shape=(h, w))
    for k in range(3):
        m = (pick == k).reshape(h, w)
        assert np.array_equal(bits(rgb)[m], bits(own[k][0])[m]), k
        assert np.array_equal(bits(z)[m], bits(own[k][1])[m]), k
    assert np.any(own[0][1] != 0) and np.any(own[1][1] != 0)  # the cameras see the scene


# ---------------------------------------------------------------------------------------------- 3. independence, holes
@pytest.fixture(scope="module")
def panorama(world):
    """a 64 x 32 panorama batch of scene5's stand-in from its camera, and its path render"""
    r, scene = world.renderer("scene5_standin")
    frame = scene.frame(64, 32)
    rec = r.projection_rays(frame, rtxpy.projection("panorama"))
    p = params("path1")
    rgb, z = r.render_rays(rec, params=p)
    return r, rec, p, rgb, z, r.stats().closest_rays


@pytest.mark.parametrize("tmax", [0.0, -1.0, -np.inf])
def test_holes_leave_the_other_pixels_alone(panorama, tmax):
    r, rec, p, rgb, z, closest = panorama
    hole = np.random.default_rng(11).random(rec.shape) < 0.5
    holed = rec.copy()
    holed["tmax"][hole] = tmax
    got = r.render_rays(holed, params=p)
    st = r.stats()
    assert np.array_equal(bits(got[0])[~hole], bits(rgb)[~hole]) and np.array_equal(bits(got[1])[~hole], bits(z)[~hole])
    assert not np.any(bits(got[0])[hole]) and not np.any(bits(got[1])[hole])
    assert 0 < st.closest_rays <= closest - np.count_nonzero(hole)


def test_a_batch_of_holes_renders_zeros(panorama):
    r, rec, p = panorama[:3]
    holed = rec.copy()
    holed["tmax"] = 0.0
    got = r.render_rays(holed, params=p)
    st = r.stats()
    assert not np.any(bits(got[0])) and not np.any(bits(got[1]))
    assert (st.closest_rays, st.shadow_rays, st.shade_points) == (0, 0, 0)


def test_a_permuted_batch_gives_the_permuted_image_under_the_constant_rng(panorama):
    r, rec, p = panorama[:3]
    pc = params("path1", rng=abi.RTX_RNG_CONST)
    a = r.render_rays(rec, params=pc)
    perm = np.random.default_rng(3).permutation(rec.size)
    b = r.render_rays(rec.reshape(-1)[perm].reshape(rec.shape), params=pc)
    assert np.array_equal(bits(b[0]).reshape(-1, 3), bits(a[0]).reshape(-1, 3)[perm])
    assert np.array_equal(bits(b[1]).reshape(-1), bits(a[1]).reshape(-1)[perm])
    assert np.any(a[0] != 0)


def test_a_nan_direction_is_a_traced_miss(panorama):
    r, rec, p, rgb, z, closest = panorama
    y, x = np.argwhere(z != 0)[len(np.argwhere(z != 0)) // 2]
    bad = rec.copy()
    bad["dir"][y, x, 1] = np.nan
    got = r.render_rays(bad, params=p)
    keep = np.ones(z.shape, bool)
    keep[y, x] = False
    assert not np.any(bits(got[0])[y, x]) and bits(got[1])[y, x] == 0
    assert np.array_equal(bits(got[0])[keep], bits(rgb)[keep]) and np.array_equal(bits(got[1])[keep], bits(z)[keep])
    assert r.stats().closest_rays >= 64 * 32 - np.count_nonzero(rec["tmax"] <= 0)  # the ray is traced and counted


# ---------------------------------------------------------------------------------------------- 4. z and features
@pytest.mark.parametrize("kind,fields", [("panorama", {}), ("fisheye", {"fov": 2.0 * np.pi}), ("ortho", {"extent": 12.0})])
@pytest.mark.parametrize("name", ["scene5_standin", "scenetest2"])
def test_z_is_the_ray_queries_t_and_the_features_z(world, name, kind, fields):
    r, scene = world.renderer(name)
    frame = scene.frame(48, 40)
    rec = r.projection_rays(frame, rtxpy.projection(kind, **fields))
    rgb, z = r.render_rays(rec, params=params("ambient"))
    flat = rec.reshape(-1)
    hits = r.trace_rays(flat["origin"], flat["dir"], tmax=flat["tmax"])
    assert np.array_equal(bits(z).reshape(-1), bits(hits["t"]))
    feat = r.ray_features(rec)
    assert np.array_equal(bits(feat["z"]), bits(z))
    hole = rec["tmax"] <= 0
    assert np.all(feat["object"][hole] == -1) and np.all(feat["material"][hole] == -1) and not np.any(feat["z"][hole])
    assert np.any(z != 0) and (kind != "fisheye" or np.any(hole))
    a, b = r.denoise(rgb, feat), r.denoise(rgb, feat)
    assert np.array_equal(bits(a), bits(b)) and np.all(np.isfinite(a))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_ray_features_of_a_frames_own_rays_are_the_frame_features(world, name):
    import torch
    r, scene = world.renderer(name)
    frame = scene.frame(37, 29)
    want = r.features(frame)
    rays = frame_rays(r, frame)
    assert r.ray_features(records(rays), shape=(29, 37)).tobytes() == want.tobytes()
    out = torch.zeros((37 * 29, 12), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.ray_features_device(37, 29, rays.data_ptr(), out.data_ptr())
    assert out.cpu().numpy().tobytes() == want.tobytes()


def test_a_batch_without_a_shape_is_padded_with_holes(world):
    r, scene = world.renderer("scene1")
    frame = scene.frame(37, 29)
    rec = records(frame_rays(r, frame))[:1030]  # more than one row of 1024
    p = params("ambient")
    rgb, z = r.render_rays(rec["origin"], rec["dir"], params=p)
    assert rgb.shape == (1030, 3) and z.shape == (1030,)
    # pixel i's key is (seed, i) in the padded 1024-wide layout as in the frame's: the frame's first 1030 pixels
    want = world.whole("scene1", "ambient", 37, 29)
    assert np.array_equal(bits(rgb), bits(want[0]).reshape(-1, 3)[:1030]) and np.array_equal(bits(z), bits(want[1]).reshape(-1)[:1030])


# ---------------------------------------------------------------------------------------------- 5. shards, device entry
def test_two_shards_make_the_whole(world):
    import torch
    r, scene = world.renderer("scene5_standin")
    w, h = 37, 29
    rays = frame_rays(r, scene.frame(w, h))
    sent = float(np.array([SENTINEL], np.uint32).view(np.float32)[0])
    rgb = torch.full((h * w * 3,), sent, dtype=torch.float32, device="cuda")
    z = torch.full((h * w,), sent, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for off in (0, 1):
        r.render_rays_device(w, h, rays.data_ptr(), params("path1", tile_offset=off, tile_stride=2), rgb.data_ptr(), z.data_ptr())
        if off == 0:
            assert np.count_nonzero(bits(z.cpu().numpy()) == SENTINEL) > 0  # the other shard's pixels are untouched
    want = world.whole("scene5_standin", "path1", w, h)
    assert same((rgb.cpu().numpy().reshape(h, w, 3), z.cpu().numpy().reshape(h, w)), want)
    # the host entry keeps the caller's values outside its shard too
    rec = records(rays)
    hr, hz = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    lib, ctx = r.lib, r._ctx
    import ctypes
    for off in (0, 1):
        p = params("path1", tile_offset=off, tile_stride=2)
        assert lib.rtx_render_rays(ctx, w, h, rec.ctypes.data, ctypes.byref(p), hr.ctypes.data, hz.ctypes.data) == 0
    assert same((hr, hz), want)
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_rays(rec, params=params("path1", tile_offset=2, tile_stride=2), shape=(h, w))
    assert e.value.code == abi.RTX_ERR_ARG
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_rays(rec, params=params("path1", max_bounces=1 << 20), shape=(h, w))
    assert e.value.code == abi.RTX_ERR_ARG


def test_device_entry_with_guard_words_a_stream_and_null_outputs(world):
    import torch
    r, scene = world.renderer("scene1")
    w, h, guard = 37, 29, 64
    n = w * h
    frame, p = scene.frame(w, h), params("path1")
    want = world.whole("scene1", "path1", w, h)
    rays = frame_rays(r, frame)
    sent = float(np.array([SENTINEL], np.uint32).view(np.float32)[0])
    for stream in (None, torch.cuda.Stream()):
        bufs = [torch.full((guard + words + guard,), sent, dtype=torch.float32, device="cuda") for words in (3 * n, n)]
        torch.cuda.synchronize()
        r.render_rays_device(w, h, rays.data_ptr(), p, bufs[0].data_ptr() + 4 * guard, bufs[1].data_ptr() + 4 * guard,
                             stream=stream.cuda_stream if stream else None)
        host = [b.cpu().numpy() for b in bufs]
        for b, words in zip(host, (3 * n, n)):
            assert np.all(bits(b[:guard]) == SENTINEL) and np.all(bits(b[guard + words:]) == SENTINEL)
        assert same((host[0][guard:guard + 3 * n].reshape(h, w, 3), host[1][guard:guard + n].reshape(h, w)), want)
    # either output may be left out
    z = torch.zeros((n,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_rays_device(w, h, rays.data_ptr(), p, None, z.data_ptr())
    assert np.array_equal(bits(z.cpu().numpy().reshape(h, w)), bits(want[1]))
    r.render_rays_device(w, h, rays.data_ptr(), p, None, None)
    with pytest.raises(rtxpy.RtxError) as e:  # a ray buffer that is not 16-byte aligned
        r.render_rays_device(w, h, rays.data_ptr() + 4, p, None, z.data_ptr())
    assert e.value.code == abi.RTX_ERR_ARG


def test_a_ray_render_leaves_the_next_renders_chunk_sizing_alone(world):
    """a plain render after a ray render is the plain render before it, chunk count included, and two ray renders
    give the same bits"""
    r, scene = world.renderer("scene1")
    frame, p = scene.frame(64, 64), params("path1")
    a = r.render(frame, p)
    sa = r.stats()
    rays = frame_rays(r, frame)
    x = render_rays_device(r, 64, 64, rays, p)
    y = render_rays_device(r, 64, 64, rays, p)
    b = r.render(frame, p)
    sb = r.stats()
    assert same(a, b) and same(x, y) and same(a, x)
    assert (sa.chunks, sa.closest_rays, sa.shadow_rays, sa.shade_points) == (sb.chunks, sb.closest_rays, sb.shadow_rays, sb.shade_points)


def test_errors_before_an_upload():
    r = rtxpy.Renderer(0)
    try:
        rec = np.zeros(64, abi.RAY_DTYPE)
        with pytest.raises(rtxpy.RtxError) as e:
            r.render_rays(rec, params=params("ambient"), shape=(8, 8))
        assert e.value.code == abi.RTX_ERR_STATE
        with pytest.raises(rtxpy.RtxError) as e:
            r.ray_features(rec, shape=(8, 8))
        assert e.value.code == abi.RTX_ERR_STATE
    finally:
        r.close()
