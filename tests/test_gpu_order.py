"""k_shadow's sample order (rtx.h RTX_OPT_SHADOW_ORDER, rtx_shadow.hip order_begin): a shade point that
walks the tree takes one emitter's light samples (more than 64, at most 1024) in the order of a key of
their light points' position across the cone, the dark ones left out, and adds their terms in index
order as before.

 1. the order itself (RTX_KAT_ORDER): a permutation of the samples that are not dark, buckets
    non-decreasing, indices increasing inside a bucket; the device's buckets are the numpy
    restatement's of the device's key values;
 2. the frames, the ray counts and every per-ray counter are the same with the option on and off,
    with no tolerance, from the product and the counting kernels; only what depends on which rays
    share a packet may move (PACKING);
 3. on the bench scene the ordered packets take fewer wave steps.
"""
import json
import os

import numpy as np
import pytest

import conftest as C
import order_model as M
import rtxpy
from rtxpy import abi
from test_gpu_configs import load
from test_gpu_cull import three_emitter_scene
from test_gpu_dark import dark_side_scene
from test_gpu_frame import far_shade_point_scene
from test_gpu_premask import bench_params, edit_bench_scene

pytestmark = pytest.mark.gpu

# what depends on which rays share a packet, by construction
PACKING = ("shadow_wave_steps", "shadow_leaf_rounds", "shadow_uniform_steps", "shadow_wave_walks")
ORDER = tuple(f for f, _ in abi.OrderStats._fields_)
COUNTERS = [f for f, _ in abi.Stats._fields_ if not f.endswith("_ms") and not f.startswith("pad")] \
    + [f for f, _ in abi.PointStats._fields_] + [f for f, _ in abi.DarkStats._fields_]
# the simulator's figure for the key (16 buckets toward the box centre, bench scene, 3000
# points): 18.8 % fewer wave steps over the walking points.  The small frame's point mix differs: half
SIM_DROP = 0.188


def render_order(scene, frame, params, opts=(), late=(), make=lambda: rtxpy.Renderer(0)):
    """the frame with the option on and off from the product and the counting kernels:
    {(order, count): (rgb, z, stats)}.  opts: options set before the upload, late: after it"""
    out = {}
    r = make()
    try:
        for o, v in opts:
            r.set_option(o, v)
        r.upload(scene)
        for o, v in late:
            r.set_option(o, v)
        for order in (1, 0):
            r.set_option(abi.RTX_OPT_SHADOW_ORDER, order)
            for count in (0, 1):
                p = rtxpy.default_params(**{f: getattr(params, f) for f, _ in abi.Params._fields_})
                p.count_traversal = count
                rgb, z = r.render(frame, p)
                out[(order, count)] = (rgb, z, r.stats())
    finally:
        r.close()
    return out


def check_equal(out, ordered=True):
    """on equals off: frames bit for bit, every counter but PACKING; points were ordered (or none)"""
    for count in (0, 1):
        (rgb, z, s), (rgb0, z0, s0) = out[(1, count)], out[(0, count)]
        assert rgb.tobytes() == rgb0.tobytes() and z.tobytes() == z0.tobytes(), count
        diff = {f: (getattr(s, f), getattr(s0, f)) for f in COUNTERS if f not in PACKING and getattr(s, f) != getattr(s0, f)}
        assert not diff, (count, diff)
        assert (s0.shadow_ordered_points, s0.shadow_ordered_rays) == (0, 0)
        if not count:
            assert (s.shadow_ordered_points, s.shadow_ordered_rays) == (0, 0)
    assert out[(1, 0)][0].tobytes() == out[(1, 1)][0].tobytes()
    s, s0 = out[(1, 1)][2], out[(0, 1)][2]
    assert s.shade_points > 0 and s.shadow_rays > 0
    print("ordered points", s.shadow_ordered_points, "rays", s.shadow_ordered_rays, "of", s.shadow_rays, "wave steps", s.shadow_wave_steps,
          "against", s0.shadow_wave_steps, "leaf rounds", s.shadow_leaf_rounds, "against", s0.shadow_leaf_rounds, "walks",
          s.shadow_wave_walks, "against", s0.shadow_wave_walks)
    if ordered:
        assert s.shadow_ordered_points > 0
        assert 0 < s.shadow_ordered_rays <= s.shadow_rays
    else:
        assert (s.shadow_ordered_points, s.shadow_ordered_rays) == (0, 0)
        for f in PACKING:  # nothing ordered: nothing moves
            assert getattr(s, f) == getattr(s0, f), f
    return s, s0


def test_gpu_order_on_the_bench_scene():
    """scene5 with the dragon stand-in at bench.py's settings, a smaller frame: 300 lights, so four
    full packets and one of 44; the ordered packets take fewer wave steps"""
    scene = load("scene5")
    s, s0 = check_equal(render_order(scene, scene.frame(160, 90), bench_params()))
    assert s.shadow_walk == abi.RTX_WALK_W8
    drop = 1.0 - s.shadow_wave_steps / s0.shadow_wave_steps
    print("wave steps drop", round(drop, 4), "bar", SIM_DROP / 2)
    assert drop >= SIM_DROP / 2
    assert s.shadow_leaf_rounds < s0.shadow_leaf_rounds


def lights_scene(tmp_path, lights):
    def edit(d):
        for o in d["Objects"]:
            if "lights" in o["parameters"]:
                o["parameters"]["lights"] = lights
    return edit_bench_scene(tmp_path, f"lights{lights}", edit)


@pytest.mark.parametrize("lights", [64, 65, 128, 1024, 1025])
def test_gpu_order_by_emitter_size(tmp_path, lights):
    """65: the smallest run that is ordered (a packet and one sample); 64: one packet, no order;
    1024: the cap; 1025: over it, nothing ordered"""
    scene = lights_scene(tmp_path, lights)
    ordered = 64 < lights <= M.CAP
    # 64-lane packets whatever the count (65 lights would share packets between points: the lane slots)
    check_equal(render_order(scene, scene.frame(64, 36), bench_params(2, 3), late=[(abi.RTX_OPT_SHADOW_SLOT, 64)]), ordered=ordered)


def test_gpu_order_with_three_emitters(tmp_path):
    """two sphere lights and a triangle light (300 + 64 + 64 samples): the first emitter's packets
    inside its samples are ordered, the straddling packets and the short runs take the index order"""
    scene = three_emitter_scene(tmp_path)
    check_equal(render_order(scene, scene.frame(160, 90), bench_params(2, 3)))


def test_gpu_order_with_a_triangle_light(tmp_path):
    """the bench scene's light as a triangle of 200 samples"""
    def edit(d):
        for o in d["Objects"]:
            if "lights" in o["parameters"]:
                p = o["parameters"]
                c = p["position"]
                o["type"] = "Triangle"
                o["parameters"] = {"material": p["material"], "epsilon": 0.0001, "lights": 200,
                                   "vertex_1": [c[0] - 0.5, c[1], c[2] - 0.3], "vertex_2": [c[0] + 0.5, c[1], c[2] - 0.3],
                                   "vertex_3": [c[0], c[1] + 0.2, c[2] + 0.5]}
    scene = edit_bench_scene(tmp_path, "trilight", edit)
    check_equal(render_order(scene, scene.frame(96, 54), bench_params(2, 5), late=[(abi.RTX_OPT_SHADOW_SLOT, 64)]))


@pytest.mark.parametrize("frame_opt", [abi.RTX_FRAME_AUTO, abi.RTX_FRAME_WORLD])
@pytest.mark.parametrize("material", ["pane", "even"])
def test_gpu_order_on_a_scene_lit_from_one_side(material, frame_opt):
    """dark_side.json: 128 samples; "pane": a transparent occluder between the light and the objects,
    "even": shininess 2 (light from behind still shines); both tree frames, the 8-wide walk.

    The "pane" cases found a flaw in the counting kernels: the 8-wide walk defers transparent leaves
    and tests them in rounds the wave's lanes start together, and the tests were counted where they
    ran, so a ray an opaque leaf blocked had counted as much of its queue as its packet mates had let
    it test (shadow_sphere_tests 463554 on against 463487 off).  They count where the leaf is queued
    now (w8_iter): what the ray's own walk calls for, per-ray work as rtx.h says."""
    scene = dark_side_scene(material)
    out = render_order(scene, scene.frame(96, 54), bench_params(2, 7),
                       opts=[(abi.RTX_OPT_TREE_FRAME, frame_opt), (abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8)])
    s, _ = check_equal(out)
    assert s.shadow_dark_rays > 0


def test_gpu_order_through_two_transparent_materials():
    """two panes of different kt stacked between the light and the objects: a ray's transmittance
    is a product in walk order, which the order of the samples does not touch"""
    with open(os.path.join(C.SCENES, "dark_side.json")) as fh:
        d = json.load(fh)
    d["Materials"].append(dict(d["Materials"][2], kt=[0.9, 0.5, 0.3], id=len(d["Materials"])))
    d["Materials"][2]["kt"] = [0.4, 0.8, 0.6]
    d["Objects"].append({"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.00025, "position": [-3.5, 1.5, 1.2], "radius": 0.9}})
    d["Objects"].append({"type": "Sphere", "parameters": {"material": len(d["Materials"]) - 1, "epsilon": 0.00025,
                                                          "position": [-2.6, 1.2, 1.1], "radius": 0.7}})
    scene = rtxpy.Scene.parse(json.dumps(d), name="two_panes", base_dir=C.GOLDEN)
    out = render_order(scene, scene.frame(96, 54), bench_params(2, 7), opts=[(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8)])
    check_equal(out)


def test_gpu_order_under_the_threaded_walk():
    scene = load("scene5")
    out = render_order(scene, scene.frame(96, 54), bench_params(8), opts=[(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_BVH2)])
    s, _ = check_equal(out)
    assert s.shadow_walk == abi.RTX_WALK_BVH2


def test_gpu_order_without_the_cone_cull():
    """RTX_OPT_SHADOW_CULL 0: no masks, no all-clear points, no dark samples: every point walks and
    is ordered, but the far ones on the floor (whole points of 300 rays, which keep the index order)"""
    scene = load("scene5")
    s, _ = check_equal(render_order(scene, scene.frame(96, 54), bench_params(8), late=[(abi.RTX_OPT_SHADOW_CULL, 0)]))
    assert s.shadow_cone_clear == 0 and s.shadow_dark_rays == 0
    assert s.shadow_ordered_rays == 300 * s.shadow_ordered_points
    rest = s.shadow_rays - s.shadow_ordered_rays
    print("not ordered", rest, "rays; far rays that reached the walk", s.far_shadow_rays)
    assert rest % 300 == 0 and s.far_shadow_rays > 0 and s.shadow_ordered_rays >= 0.85 * s.shadow_rays


def test_gpu_order_without_the_dark_samples():
    scene = load("scene5")
    s, _ = check_equal(render_order(scene, scene.frame(96, 54), bench_params(8), late=[(abi.RTX_OPT_SHADOW_DARK, 0)]))
    assert s.shadow_dark_rays == 0 and s.shadow_cone_clear > 0


@pytest.mark.parametrize("walk", [abi.RTX_WALK_W8, abi.RTX_WALK_BVH2])
def test_gpu_order_far_shade_points(tmp_path, walk):
    """shade points beyond RTX_FRAME_FAR radii keep the index order (their rays walk from the light end)"""
    scene = far_shade_point_scene(tmp_path, 128)
    params = rtxpy.params_from_args(["-l", "none"], rng=abi.RTX_RNG_COUNTER)
    s, _ = check_equal(render_order(scene, scene.frame(96, 96), params, opts=[(abi.RTX_OPT_SHADOW_WALK, walk)]))
    assert s.far_shadow_rays > 0 and s.shadow_walk == walk


def test_gpu_order_in_two_chunks():
    scene = load("scene5")
    frame = scene.frame(160, 96)
    tiles = (frame.width // 8) * (frame.height // 8)
    one = render_order(scene, frame, bench_params(4))
    two = render_order(scene, frame, bench_params(4), late=[(abi.RTX_OPT_CHUNK_TILES, tiles // 2)])
    (s1, _), (s2, _) = check_equal(one), check_equal(two)
    assert (s1.chunks, s2.chunks) == (1, 2)
    assert one[(1, 0)][0].tobytes() == two[(1, 0)][0].tobytes() and one[(1, 0)][1].tobytes() == two[(1, 0)][1].tobytes()
    assert (s1.shadow_ordered_points, s1.shadow_ordered_rays) == (s2.shadow_ordered_points, s2.shadow_ordered_rays)


def test_gpu_order_in_a_loopback_group():
    """two shards on one device through the device group's render call"""
    scene = load("scene5")
    frame = scene.frame(160, 90)
    single = render_order(scene, frame, bench_params(4))
    group = render_order(scene, frame, bench_params(4), make=lambda: rtxpy.Group([0], loopback=2))
    s, _ = check_equal(group)
    assert s.devices == 2
    assert group[(1, 0)][0].tobytes() == single[(1, 0)][0].tobytes()
    s1 = single[(1, 1)][2]
    assert (s.shadow_ordered_points, s.shadow_ordered_rays) == (s1.shadow_ordered_points, s1.shadow_ordered_rays)


# ---- the order itself ----
def order_records(seed, n, nl, etype, on_axis=False, dark=1):
    """KAT_ORDER records: a shade point below and beside an emitter, its normal random (so a good part
    of the samples is dark), the box centre off the axis, or on it (the key's other direction)"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, abi.KAT_IN[abi.KAT_ORDER]), np.float32)
    x[:, 0:3] = rng.uniform(-3, 3, (n, 3))
    nrm = rng.normal(size=(n, 3))
    x[:, 3:6] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    view = rng.normal(size=(n, 3))
    x[:, 6:9] = view / np.linalg.norm(view, axis=1, keepdims=True)
    x[:, 9:12] = rng.uniform(0.1, 1, (n, 3))   # kd
    x[:, 12:15] = rng.uniform(0.1, 1, (n, 3))  # ks
    x[:, 15] = 5.0
    x[:, 16] = etype
    c = rng.uniform(-1, 1, (n, 3)) + [0, 0, 8]
    if etype == 0:
        x[:, 17:20] = c
        x[:, 29] = rng.uniform(0.2, 1.5, n)
    else:
        x[:, 17:20] = c + rng.uniform(-1, 1, (n, 3))
        x[:, 20:23] = c + rng.uniform(-1, 1, (n, 3))
        x[:, 23:26] = c + rng.uniform(-1, 1, (n, 3))
    x[:, 26] = nl
    x[:, 27] = rng.integers(0, 1 << 24, n)
    x[:, 28] = rng.integers(0, 1 << 24, n)
    x[:, 30:33] = rng.uniform(-2, 2, (n, 3)) + [0, 0, 3]
    if on_axis:  # the centre on the line from the point to the emitter sphere's centre
        ec = x[:, 17:20] if etype == 0 else (x[:, 17:20] + x[:, 20:23] + x[:, 23:26]) / 3
        x[:, 30:33] = x[:, 0:3] + 0.5 * (ec - x[:, 0:3])
    x[:, 33] = abi.RTX_PHONG
    x[:, 34] = abi.RTX_ATT_SQR
    x[:, 35] = 1.0
    x[:, 36] = dark
    return x


@pytest.mark.parametrize("etype", [0, 1])
@pytest.mark.parametrize("nl", [65, 300, 1024])
def test_gpu_order_is_a_stable_sort_of_the_lit_samples(etype, nl):
    x = np.concatenate([order_records(3 + nl, 6, nl, etype), order_records(5 + nl, 3, nl, etype, on_axis=True),
                        order_records(7 + nl, 2, nl, etype, dark=0)])
    y = rtxpy.gpu_kat(abi.KAT_ORDER, x)
    ndark = 0
    for i in range(len(x)):
        n_ord, npk = int(y[i, 0]), int(y[i, 1])
        order, buckets, key = y[i, 4:4 + M.CAP].astype(np.int64), y[i, 4 + M.CAP:4 + 2 * M.CAP].astype(np.int64), y[i, 4 + 2 * M.CAP:4 + 3 * M.CAP]
        assert npk == (nl + 63) // 64
        assert (order[n_ord:] == -1).all() and (buckets[nl:] == M.BUCKETS).all()
        M.check_order(order[:n_ord], buckets, nl)
        lit = buckets[:nl] < M.BUCKETS
        assert np.array_equal(buckets[:nl][lit], M.bucket(key[:nl][lit]))
        assert np.isfinite(key[:nl]).all()
        if x[i, 36] == 0:
            assert lit.all() and n_ord == nl
        ndark += int((~lit).sum())
        # the key spreads the samples: the light points cover the emitter, so more than two buckets are in use
        assert len(set(buckets[:nl][lit].tolist())) >= 3 or lit.sum() < 16
    print("etype", etype, "nl", nl, "dark samples", ndark, "of", nl * len(x))
    assert ndark > 0


def test_gpu_order_leaves_short_and_long_runs_alone():
    for nl in (1, 64, 1025):
        y = rtxpy.gpu_kat(abi.KAT_ORDER, order_records(11, 2, nl, 0))
        assert (y[:, 0:2] == 0).all() and (y[:, 4:4 + M.CAP] == -1).all()
