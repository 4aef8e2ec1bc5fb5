"""k_trace's packed GI walk (rtx.h RTX_OPT_TRACE_PACK, rtx_trace.hip gi_batch_packed): a tile's path-GI
rays are taken in segments, every ray up to its visit of the root, then the rays that go on into the
8-wide tree packed 64 to a wave, then the hits in the rays' own order.  A ray makes the visits and tests
it made before and the shade points leave in the same order, so with the option on and off the frames,
the ray and shade-point counts and the closest-hit counters are the same, with no tolerance:

 - the bench scene at 64x36, its walker share running from a few per cent (the wall) to all (the mesh):
   tile totals below 64, off a multiple of 64 and across a partial last segment, every segment size,
   and the one-sample batches of deeper bounces through its transparent mesh;
 - partial tiles; a mesh no GI ray reaches (empty queues) and a camera inside a closed mesh (every ray
   walks);
 - the rotated tree frame (scene6), far origins, the BVH2 walk and a scene without a tree (which keep
   the batch-by-batch path), two chunks, a tile list, two passes, an adaptive render, a loopback group
   of two; and the same frame twice from one context.
"""
import json

import numpy as np
import pytest

import conftest as C
import rtxpy
import standins
from rtxpy import abi
from test_gpu_configs import load
from test_gpu_frame import far_shade_point_scene

pytestmark = pytest.mark.gpu

FIELDS = ("closest_rays", "shadow_rays", "shade_points", "node_visits", "tri_tests", "sphere_tests", "plane_tests")


def path_params(spp, bounces=None, seed=1):
    args = ["-g", "path", "-n", str(spp)] + (["-b", str(bounces)] if bounces is not None else [])
    p = rtxpy.params_from_args(args, seed=seed)
    p.rng = abi.RTX_RNG_COUNTER
    return p


def counting(params, count):
    p = rtxpy.default_params(**{f: getattr(params, f) for f, _ in abi.Params._fields_})
    p.count_traversal = count
    return p


def render_pack(r, frame, params, packs=(1, 0), render=None):
    """{(pack, count): (arrays' bytes, stats)} from an uploaded renderer or group"""
    render = render or (lambda p: r.render(frame, p))
    out = {}
    for pack in packs:
        r.set_option(abi.RTX_OPT_TRACE_PACK, pack)
        for count in (0, 1):
            arrays = render(counting(params, count))
            out[(pack, count)] = (tuple(np.asarray(a).tobytes() for a in arrays), r.stats())
    r.set_option(abi.RTX_OPT_TRACE_PACK, 1)
    return out


def check_equal(out):
    """every packed render against the unpacked one of the same kernel: bytes and counters.  Returns the
    counting render's stats with the option on."""
    for (pack, count), (arrays, s) in out.items():
        arrays0, s0 = out[(0, count)]
        assert arrays == arrays0, (pack, count)
        diff = {f: (getattr(s, f), getattr(s0, f)) for f in FIELDS if getattr(s, f) != getattr(s0, f)}
        assert not diff, (pack, count, diff)
    assert out[(1, 0)][0] == out[(1, 1)][0]
    s = out[(1, 1)][1]
    assert s.closest_rays > 0 and s.shade_points > 0
    return s


def trace_counts(s):
    """k_trace's own node visits and triangle tests (the totals hold k_shadow's too)"""
    return s.node_visits - s.shadow_node_visits, s.tri_tests - s.shadow_tri_tests


W8 = ((abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8),)  # a small scene builds the 8-wide tree only when asked to


def opened(scene, opts=(), make=lambda: rtxpy.Renderer(0)):
    r = make()
    try:
        for o, v in opts:
            r.set_option(o, v)
        r.upload(scene)
    except Exception:
        r.close()
        raise
    return r


@pytest.fixture(scope="module")
def bench():
    scene = load("scene5")
    r = opened(scene)
    yield r, scene
    r.close()


@pytest.mark.parametrize("spp", [1, 2, 63, 64, 65, 100])
def test_gpu_trace_pack_on_the_bench_scene(bench, spp):
    """a full tile's GI rays: 64 spp; 1 and 2 stay below a batch or two, 63 and 65 end off a multiple of 64,
    65 and 100 end in a partial segment (4160 and 6400 rays in segments of 4096)"""
    r, scene = bench
    s = check_equal(render_pack(r, scene.frame(64, 36), path_params(spp)))
    visits, tris = trace_counts(s)
    print("spp", spp, "closest", s.closest_rays, "visits", visits, "triangle tests", tris)
    assert s.trace_walk == abi.RTX_WALK_W8 and visits > s.closest_rays and tris > 0


def test_gpu_trace_pack_at_every_segment_size(bench):
    r, scene = bench
    check_equal(render_pack(r, scene.frame(64, 36), path_params(65), packs=(512, 1024, 2048, 4096, 1, 0)))


def test_gpu_trace_pack_through_deeper_bounces(bench):
    """the transparent mesh at 10 bounces: task batches whose hits take one GI sample each"""
    r, scene = bench
    frame = scene.frame(64, 36)
    s = check_equal(render_pack(r, frame, path_params(2, bounces=10)))
    r.set_option(abi.RTX_OPT_TRACE_PACK, 0)
    r.render(frame, path_params(2, bounces=1))
    assert s.closest_rays > r.stats().closest_rays  # the deeper bounces were there
    r.set_option(abi.RTX_OPT_TRACE_PACK, 1)


def test_gpu_trace_pack_on_partial_tiles(bench):
    r, scene = bench
    check_equal(render_pack(r, scene.frame(20, 12), path_params(5)))


def test_gpu_trace_pack_repeats(bench):
    r, scene = bench
    frame, p = scene.frame(64, 36), path_params(7)
    a = render_pack(r, frame, p, packs=(1,))
    b = render_pack(r, frame, p, packs=(1,))
    for k in a:
        assert a[k][0] == b[k][0]
        assert all(getattr(a[k][1], f) == getattr(b[k][1], f) for f in FIELDS)


def room_scene(tmp_path, tris, position, scale, camera):
    """a floor and a back wall, one mesh and a sphere light"""
    (tmp_path / "meshes").mkdir(exist_ok=True)
    standins.write_stl(str(tmp_path / "meshes" / "m.stl"), tris)
    mat = {"ks": [0.0, 0.0, 0.0], "ka": [0.5, 0.5, 0.5], "kr": [0.0, 0.0, 0.0], "kt": [0.0, 0.0, 0.0], "ke": [0.0, 0.0, 0.0],
           "shininess": 0.0, "refractive_index": 1.0}
    d = {"AmbientLight": [0.1, 0.1, 0.1],
         "Camera": dict({"vector_x": [1.0, 0.0, 0.0], "vector_y": [0.0, -0.15, -1.0], "fov": 80, "focal_length": 1.0}, **camera),
         "Materials": [dict(mat, id=0, texture={"type": "uniform", "color": [0.7, 0.7, 0.7]}),
                       dict(mat, id=1, texture={"type": "uniform", "color": [0.8, 0.3, 0.2]}),
                       dict(mat, id=2, ke=[1.0, 1.0, 1.0], texture={"type": "uniform", "color": [0.0, 0.0, 0.0]})],
         "Objects": [
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 0.0, -1.0], "normal": [0.0, 0.0, 1.0]}},
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 5.0, 0.0], "normal": [0.0, -1.0, 0.0]}},
             {"type": "Mesh", "parameters": {"material": 1, "filename": "meshes/m.stl", "position": position, "rotation": [0.0, 0.0, 0.0],
                                             "scale": scale}},
             {"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.0003, "position": [-5.0, 0.0, 2.5], "radius": 0.4, "lights": 8}}]}
    return rtxpy.Scene.parse(json.dumps(d), name="room", base_dir=str(tmp_path))


def test_gpu_trace_pack_with_empty_queues(tmp_path):
    """a mesh under the floor: a GI ray meets a plane before the mesh's box, so no walk leaves the root"""
    v, f = standins.icosphere(2)
    scene = room_scene(tmp_path, v[f].astype(np.float32), [0.0, 2.0, -30.0], 1.0, {"position": [0.0, -3.5, 1.0]})
    r = opened(scene, W8)
    try:
        s = check_equal(render_pack(r, scene.frame(64, 36), path_params(64)))
    finally:
        r.close()
    visits, tris = trace_counts(s)
    print("closest", s.closest_rays, "visits", visits, "triangle tests", tris)
    assert s.trace_walk == abi.RTX_WALK_W8 and tris == 0 and 0 < visits <= s.closest_rays


def test_gpu_trace_pack_with_every_ray_walking(tmp_path):
    """the camera inside a closed mesh whose faces look inwards: every primary hit takes its GI samples, and
    each of them starts inside the root's box and meets the mesh again"""
    v, f = standins.icosphere(3)
    tris = v[f[:, ::-1]].astype(np.float32)
    scene = room_scene(tmp_path, tris, [0.0, 0.0, 1.0], 1.5, {"position": [0.0, 0.0, 1.0]})
    frame, p = scene.frame(64, 36), path_params(64)
    r = opened(scene, W8)
    try:
        s = check_equal(render_pack(r, frame, p))
    finally:
        r.close()
    gi = s.closest_rays - frame.width * frame.height
    visits, tris = trace_counts(s)
    print("closest", s.closest_rays, "GI rays", gi, "visits", visits, "triangle tests", tris)
    assert s.trace_walk == abi.RTX_WALK_W8 and gi == 64 * frame.width * frame.height and visits >= 2 * gi and tris >= gi


def test_gpu_trace_pack_on_the_rotated_frame():
    scene = load("scene6")
    r = opened(scene)
    try:
        s = check_equal(render_pack(r, scene.frame(32, 24), path_params(16)))
    finally:
        r.close()
    assert s.tree_rotated == 1 and s.trace_walk == abi.RTX_WALK_W8 and trace_counts(s)[1] > 0


def test_gpu_trace_pack_with_far_origins(tmp_path):
    scene = far_shade_point_scene(tmp_path, 16)
    r = opened(scene, W8)
    try:
        s = check_equal(render_pack(r, scene.frame(64, 36), path_params(8)))
    finally:
        r.close()
    print("far closest rays", s.far_closest_rays)
    assert s.trace_walk == abi.RTX_WALK_W8 and s.far_closest_rays > 0


@pytest.mark.parametrize("name,opts", [("scene5", ((abi.RTX_OPT_TRACE_WALK, abi.RTX_WALK_BVH2),)), ("scene3", ())], ids=["bvh2", "no-tree"])
def test_gpu_trace_pack_leaves_the_other_walks_alone(name, opts):
    scene = load(name)
    r = opened(scene, opts)
    try:
        s = check_equal(render_pack(r, scene.frame(32, 24), path_params(8)))
    finally:
        r.close()
    assert s.trace_walk == abi.RTX_WALK_BVH2


def test_gpu_trace_pack_in_two_chunks(bench):
    r, scene = bench
    frame = scene.frame(64, 36)
    r.set_option(abi.RTX_OPT_CHUNK_TILES, 20)
    try:
        out = render_pack(r, frame, path_params(9))
    finally:
        r.set_option(abi.RTX_OPT_CHUNK_TILES, 0)
    assert check_equal(out).chunks == 2
    whole = render_pack(r, frame, path_params(9), packs=(1,))
    assert whole[(1, 0)][0] == out[(1, 0)][0]


def test_gpu_trace_pack_on_a_tile_list(bench):
    r, scene = bench
    frame = scene.frame(64, 36)
    tiles = np.array([0, 3, 9, 17, 18, 31, 39], np.uint32)
    check_equal(render_pack(r, frame, path_params(9), render=lambda p: r.render_tiles(frame, p, tiles)))


def test_gpu_trace_pack_in_a_two_pass_render(bench):
    r, scene = bench
    frame = scene.frame(64, 36)
    check_equal(render_pack(r, frame, path_params(5), render=lambda p: r.render_passes(frame, p, 2, jitter=True)))


def test_gpu_trace_pack_in_an_adaptive_render(bench):
    r, scene = bench
    frame = scene.frame(64, 36)
    out = render_pack(r, frame, path_params(3), render=lambda p: r.render_adaptive(frame, p, 4, 0.02))
    check_equal(out)
    assert r.adaptive_stats().passes_run >= 2


def test_gpu_trace_pack_on_a_loopback_group_of_two(bench):
    single, scene = bench
    frame = scene.frame(64, 36)
    g = opened(scene, make=lambda: rtxpy.Group([0], loopback=2))
    try:
        out = render_pack(g, frame, path_params(9))
    finally:
        g.close()
    assert check_equal(out).devices == 2
    one = render_pack(single, frame, path_params(9), packs=(1,))
    assert one[(1, 0)][0] == out[(1, 0)][0]
