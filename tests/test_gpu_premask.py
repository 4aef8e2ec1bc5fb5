"""The per-point masks formed ahead of k_shadow (rtx.h RTX_OPT_SHADOW_PREMASK, rtx_shadow_premask.h
k_point_masks): where k_shadow would form a shade point's cone, plane and listed-object masks with a
whole wave (point_masks), a kernel of its own forms them first, one point per lane, through the same
functions, and k_shadow reads one word per point.  The masks are the same, so with the option on and
off

 - the image, the depth buffer and the ray counts are equal bit for bit, from the product and from
   the counting kernels;
 - every counter of rtx_stats, rtx_point_stats and rtx_dark_stats is equal (all fields but the
   times, which are measurements): equal shadow_cone_clear, shadow_point_clear, shadow_plane_skipped,
   shadow_lin_skipped, shadow_plane_tests and dark counts show the masks agree point by point in
   their effect (the lane-slot frame, which the option does not touch, leaves out the three counters
   of what a packet's waves do together: PER_PACKET below);
 - rtx_premask_stats tells whether the pass ran: for every shade point, or (more than 8 emitters,
   lane-slot packets, every cull off) for none.
"""
import json
import os
import shutil

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi
from test_gpu_configs import load
from test_gpu_cull import three_emitter_scene
from test_gpu_frame import far_camera_scene, far_shade_point_scene
from test_gpu_pointclear import handmade_scene

pytestmark = pytest.mark.gpu

COUNTERS = [f for f, _ in abi.Stats._fields_ if not f.endswith("_ms") and not f.startswith("pad")] \
    + [f for f, _ in abi.PointStats._fields_] + [f for f, _ in abi.DarkStats._fields_]


def bench_params(spp=64, seed=1):
    p = rtxpy.params_from_args(["-g", "path", "-n", str(spp)], seed=seed)
    p.rng = abi.RTX_RNG_COUNTER
    return p


def render_premask(scene, frame, params, opts=(), late=(), make=lambda: rtxpy.Renderer(0)):
    """the frame with the option on and off from the product and the counting kernels:
    {(premask, count): (rgb, z, stats)}.  opts: options set before the upload, late: after it"""
    out = {}
    r = make()
    try:
        for o, v in opts:
            r.set_option(o, v)
        r.upload(scene)
        for o, v in late:
            r.set_option(o, v)
        for pre in (1, 0):
            r.set_option(abi.RTX_OPT_SHADOW_PREMASK, pre)
            for count in (0, 1):
                p = rtxpy.default_params(**{f: getattr(params, f) for f, _ in abi.Params._fields_})
                p.count_traversal = count
                rgb, z = r.render(frame, p)
                out[(pre, count)] = (rgb, z, r.stats())
    finally:
        r.close()
    return out


# what the waves of a packet do together: with one point per packet (the wave-uniform layout) these
# depend on the point alone; on the lane slots they depend on which points share a packet, that is on
# the order k_trace's waves emitted the records in (ties of the Morton sort), which differs from
# render to render with no option changed (measured: four renders of that frame in a row gave
# 261804 / 261672 / 261479 / 261651 wave steps, the same box and triangle tests and wave walks)
PER_PACKET = ("shadow_wave_steps", "shadow_leaf_rounds", "shadow_uniform_steps")


def check_equal(out, ran, skip=()):
    """on equals off: frames bit for bit, every counter (but `skip`); the pass ran for every point
    (ran) or none"""
    for count in (0, 1):
        (rgb, z, s), (rgb0, z0, s0) = out[(1, count)], out[(0, count)]
        assert rgb.tobytes() == rgb0.tobytes() and z.tobytes() == z0.tobytes(), count
        diff = {f: (getattr(s, f), getattr(s0, f)) for f in COUNTERS if f not in skip and getattr(s, f) != getattr(s0, f)}
        assert not diff, (count, diff)
        assert s0.premask_points == 0
        assert s.premask_points == (s.shade_points if ran else 0), (count, s.premask_points, s.shade_points)
    # the product and the counting kernels render the same frame
    assert out[(1, 0)][0].tobytes() == out[(1, 1)][0].tobytes()
    s = out[(1, 1)][2]
    assert s.shade_points > 0 and s.shadow_rays > 0
    return s


def test_gpu_premask_on_the_bench_scene():
    """scene5 with the dragon stand-in at bench.py's settings, a smaller frame: the 8-wide walk, one
    emitter, two planes; most points are all-clear"""
    scene = load("scene5")
    s = check_equal(render_premask(scene, scene.frame(160, 90), bench_params()), ran=True)
    print("scene5 cone_clear", s.shadow_cone_clear, "point_clear", s.shadow_point_clear, "planes skipped", s.shadow_plane_skipped,
          "dark", s.shadow_dark_rays, "of", s.shadow_rays)
    assert s.shadow_walk == abi.RTX_WALK_W8
    assert s.shadow_cone_clear > 0 and s.shadow_point_clear > 0 and s.shadow_plane_skipped > 0 and s.shadow_dark_rays > 0
    assert 0 < s.shadow_wave_walks  # and some packets still walk


@pytest.mark.parametrize("name", ["s1_path2", "s2_blinn_lin", "s3_path2", "s3_none_b3"])
def test_gpu_premask_on_the_golden_configs(name):
    scene, frame, params, _ = C.load_config(name)
    s = check_equal(render_premask(scene, frame, params, late=[(abi.RTX_OPT_SHADOW_SLOT, 64)]), ran=True)  # one point per packet
    print(name, "walk", abi.WALK_NAMES[s.shadow_walk], "planes skipped", s.shadow_plane_skipped, "objects skipped", s.shadow_lin_skipped,
          "all-clear rays", s.shadow_point_clear)


def test_gpu_premask_with_three_emitters(tmp_path):
    """two sphere lights and a triangle light, out of the 8-wide tree (listed records): packets inside
    one emitter's samples and packets straddling two"""
    scene = three_emitter_scene(tmp_path)
    s = check_equal(render_premask(scene, scene.frame(160, 90), bench_params(2, 3)), ran=True)
    print("three emitters: cone_clear", s.shadow_cone_clear, "all-clear rays", s.shadow_point_clear, "objects skipped", s.shadow_lin_skipped)
    assert s.shadow_cone_clear > 0 and s.shadow_point_clear > 0 and s.shadow_lin_skipped > 0


@pytest.mark.parametrize("frame_opt", [abi.RTX_FRAME_AUTO, abi.RTX_FRAME_WORLD])
def test_gpu_premask_on_the_handmade_scene(tmp_path, frame_opt):
    """tilted and transparent planes, a light 1e-3 short of a wall, a triangle light; objects tested
    one by one (no tree): planes, records and the emitter-is-the-record case"""
    scene = handmade_scene(tmp_path)
    out = render_premask(scene, scene.frame(160, 90), bench_params(2, 7), opts=[(abi.RTX_OPT_TREE_FRAME, frame_opt)])
    s = check_equal(out, ran=True)
    print("handmade frame", frame_opt, "planes skipped", s.shadow_plane_skipped, "run", s.shadow_plane_tests, "objects skipped",
          s.shadow_lin_skipped)
    assert s.shadow_plane_skipped > 0 and s.shadow_plane_tests > 0 and s.shadow_lin_skipped > 0


def test_gpu_premask_without_a_tree():
    """scene3: RTX_WALK_LINEAR, six planes per point, masks without a cone cull"""
    scene = load("scene3")
    s = check_equal(render_premask(scene, scene.frame(160, 90), bench_params(2), late=[(abi.RTX_OPT_SHADOW_SLOT, 64)]), ran=True)
    print("scene3 planes skipped", s.shadow_plane_skipped, "run", s.shadow_plane_tests)
    assert s.shadow_walk == abi.RTX_WALK_LINEAR and s.shadow_plane_skipped > 0


@pytest.mark.parametrize("walk", [abi.RTX_WALK_W8, abi.RTX_WALK_BVH2])
def test_gpu_premask_under_both_walks(walk):
    """the bench scene under the 8-wide and the threaded walk (the second has no cone cull: plane
    masks only)"""
    scene = load("scene5")
    out = render_premask(scene, scene.frame(96, 54), bench_params(8), opts=[(abi.RTX_OPT_SHADOW_WALK, walk)])
    s = check_equal(out, ran=True)
    assert s.shadow_walk == walk and s.shadow_plane_skipped > 0
    assert (s.shadow_cone_clear > 0) == (walk == abi.RTX_WALK_W8)


def test_gpu_premask_far_camera(tmp_path):
    """a camera 60 scene radii out, one point per packet"""
    scene = far_camera_scene(tmp_path, 60.0)
    out = render_premask(scene, scene.frame(96, 96), rtxpy.params_from_args([], seed=1), late=[(abi.RTX_OPT_SHADOW_SLOT, 64)])
    s = check_equal(out, ran=True)
    assert s.far_closest_rays >= 96 * 96


@pytest.mark.parametrize("walk", [abi.RTX_WALK_W8, abi.RTX_WALK_BVH2])
def test_gpu_premask_far_shade_points(tmp_path, walk):
    """shade points beyond RTX_FRAME_FAR radii take no mask (their word is 0): their rays are walked
    from the light end as before"""
    scene = far_shade_point_scene(tmp_path, 64)
    params = rtxpy.params_from_args(["-l", "none"], rng=abi.RTX_RNG_CONST)
    s = check_equal(render_premask(scene, scene.frame(96, 96), params, opts=[(abi.RTX_OPT_SHADOW_WALK, walk)]), ran=True)
    assert s.far_shadow_rays > 0 and s.shadow_walk == walk


def test_gpu_premask_in_two_chunks():
    """the array is indexed by the chunk's record index: the same frame in one chunk and in two"""
    scene = load("scene5")
    frame = scene.frame(160, 96)
    tiles = (frame.width // 8) * (frame.height // 8)
    one = render_premask(scene, frame, bench_params(4))
    two = render_premask(scene, frame, bench_params(4), late=[(abi.RTX_OPT_CHUNK_TILES, tiles // 2)])
    s1, s2 = check_equal(one, ran=True), check_equal(two, ran=True)
    assert (s1.chunks, s2.chunks) == (1, 2)
    assert one[(1, 0)][0].tobytes() == two[(1, 0)][0].tobytes() and one[(1, 0)][1].tobytes() == two[(1, 0)][1].tobytes()
    assert s1.shadow_point_clear == s2.shadow_point_clear and s1.shadow_cone_clear == s2.shadow_cone_clear


def test_gpu_premask_in_a_loopback_group():
    """two shards on one device through the device group's render call"""
    scene = load("scene5")
    frame = scene.frame(160, 90)
    single = render_premask(scene, frame, bench_params(4))
    group = render_premask(scene, frame, bench_params(4), make=lambda: rtxpy.Group([0], loopback=2))
    s = check_equal(group, ran=True)
    assert s.devices == 2
    assert group[(1, 0)][0].tobytes() == single[(1, 0)][0].tobytes()
    s1 = single[(1, 1)][2]
    assert (s.shadow_cone_clear, s.shadow_point_clear, s.shadow_plane_skipped) == (s1.shadow_cone_clear, s1.shadow_point_clear,
                                                                                 s1.shadow_plane_skipped)


def edit_bench_scene(tmp_path, name, edit):
    """the bench scene (dragon stand-in) with its object list edited"""
    load("scene5")  # writes the dragon stand-in
    with open(os.path.join(C.SCENES, "scene5_standin.json")) as fh:
        d = json.load(fh)
    os.makedirs(tmp_path / "meshes", exist_ok=True)
    shutil.copy(os.path.join(C.GOLDEN, "meshes", "dragon_standin.stl"), tmp_path / "meshes" / "dragon_standin.stl")
    edit(d)
    return rtxpy.Scene.parse(json.dumps(d), name=name, base_dir=str(tmp_path))


def test_gpu_premask_falls_back_beyond_eight_emitters(tmp_path):
    """nine emitters of 64 lights: a byte per mask cannot hold them, the pass is not launched and
    k_shadow forms the masks itself; the frame is the same"""
    def edit(d):
        for i in range(8):
            d["Objects"].append({"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.0003, "lights": 64, "radius": 0.2,
                                                                  "position": [-5.0 + 1.4 * i, -3.5 + 0.3 * (i % 3), 1.0 + 0.25 * i]}})
    scene = edit_bench_scene(tmp_path, "nine", edit)
    assert scene.desc.num_emitters == 9
    s = check_equal(render_premask(scene, scene.frame(96, 54), bench_params(2, 3)), ran=False)
    assert s.shadow_plane_skipped > 0  # the masks are there all the same


@pytest.mark.parametrize("cull,point", [(0, 1), (1, 0)])
def test_gpu_premask_with_the_culls_off(cull, point):
    """RTX_OPT_SHADOW_CULL 0 turns every mask off (no pass); RTX_OPT_SHADOW_POINT 0 leaves the cone
    mask (the pass forms it alone)"""
    scene = load("scene5")
    late = [(abi.RTX_OPT_SHADOW_CULL, cull), (abi.RTX_OPT_SHADOW_POINT, point)]
    s = check_equal(render_premask(scene, scene.frame(160, 90), bench_params(4), late=late), ran=bool(cull))
    assert (s.shadow_plane_skipped, s.shadow_lin_skipped, s.shadow_point_clear) == (0, 0, 0)
    assert (s.shadow_cone_clear > 0) == bool(cull)


def test_gpu_premask_leaves_the_lane_slots_alone(tmp_path):
    """100 lights: points share packets in 4-lane slots (the lane-slot kernels, which take no
    per-point mask): no pass, same frame"""
    def edit(d):
        for o in d["Objects"]:
            if "lights" in o["parameters"]:
                o["parameters"]["lights"] = 100
    scene = edit_bench_scene(tmp_path, "hundred", edit)
    s = check_equal(render_premask(scene, scene.frame(160, 90), bench_params(2, 3)), ran=False, skip=PER_PACKET)
    assert s.shadow_rays == 100 * s.shade_points  # every shade point samples the one emitter


def test_gpu_premask_option_rejects_bad_values():
    r = rtxpy.Renderer(0)
    try:
        for bad in (-1, 2):
            with pytest.raises(rtxpy.RtxError) as e:
                r.set_option(abi.RTX_OPT_SHADOW_PREMASK, bad)
            assert e.value.code == abi.RTX_ERR_ARG
    finally:
        r.close()
