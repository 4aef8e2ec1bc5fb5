"""RTX_OPT_SHADOW_CLEARLANE (rtx.h; rtx_shadow_clearlane.h k_clear_count / k_clear_scan / k_clear_scatter and
k_shadow_clear): the all-clear shade points that lie on no emitter are split off the processing order and
shaded one per lane, their samples in sequence, summed in the order of k_shadow's 64-lane reduction.

Every case renders the frame four times: option on and off, product and counting kernels.  A counting render
never takes the new path, so it is the old code whatever the option says.  The four frames' bytes (rgb and
z) and ray totals must be the same; the new kernel must have taken no point where the option is off or the
render counts; and, so that a silent fallback cannot pass, on a scene of one emitter it must have taken
exactly shadow_point_clear / nl points, the all-clear points k_shadow counts with the option off (there a
point on the emitter samples nothing and is not all-clear), on the others more than 0.
"""
import json

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi
from test_gpu_configs import load
from test_gpu_cull import three_emitter_scene
from test_gpu_frame import far_shade_point_scene
from test_gpu_spec import spec_scene

pytestmark = pytest.mark.gpu

CL = abi.RTX_OPT_SHADOW_CLEARLANE
SLOT64 = ((abi.RTX_OPT_SHADOW_SLOT, 64),)
W8 = ((abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8),)


def bench_params(spp=2, seed=5, rng=abi.RTX_RNG_COUNTER):
    p = rtxpy.params_from_args(["-g", "path", "-n", str(spp)], seed=seed)
    p.rng = rng
    return p


def copy_params(p, **over):
    q = rtxpy.default_params(**{f: getattr(p, f) for f, _ in abi.Params._fields_})
    for k, v in over.items():
        setattr(q, k, v)
    return q


def renders(scene, frame, params, opts=(), late=(), make=lambda: rtxpy.Renderer(0), tiles=None):
    """{(clearlane, count): (rgb bytes, z bytes, stats)}; opts: options set before the upload, late: after it"""
    out = {}
    r = make()
    try:
        for o, v in opts:
            r.set_option(o, v)
        r.upload(scene)
        for o, v in late:
            r.set_option(o, v)
        for cl in (1, 0):
            r.set_option(CL, cl)
            for count in (0, 1):
                p = copy_params(params, count_traversal=count)
                rgb, z = r.render(frame, p) if tiles is None else r.render_tiles(frame, p, tiles)
                out[(cl, count)] = (rgb.tobytes(), z.tobytes(), r.stats())
    finally:
        r.close()
    return out


def check(out, nl=None, none=False):
    """the four frames and ray totals are one; what the kernel took (see the module's text).  nl: the lights of
    a single-emitter scene; none: the path must not have run.  Returns (product stats with the option on, counting
    stats with it off)."""
    rgb0, z0, s0 = out[(0, 0)]
    for k, (rgb, z, s) in out.items():
        assert rgb == rgb0 and z == z0, k
        assert (s.closest_rays, s.shadow_rays, s.shade_points) == (s0.closest_rays, s0.shadow_rays, s0.shade_points), k
        if k != (1, 0):
            assert (s.clear_points, s.clear_rays) == (0, 0), k
    on, cnt = out[(1, 0)][2], out[(0, 1)][2]
    assert on.shade_points > 0 and on.shadow_rays > 0
    print("clear points", on.clear_points, "rays", on.clear_rays, "of", on.shadow_rays, "shade points", on.shade_points,
          "all-clear rays (counting, option off)", cnt.shadow_point_clear)
    if none:
        assert (on.clear_points, on.clear_rays) == (0, 0)
    elif nl:
        assert on.clear_points > 0 and on.clear_points * nl == cnt.shadow_point_clear
        assert on.clear_rays == on.clear_points * nl
    else:
        assert on.clear_points > 0 and 0 < on.clear_rays <= cnt.shadow_point_clear
    return on, cnt


def edit_spec_scene(name, edit, ks=0.3, shin=5.0, lights=65):
    """test_gpu_spec's spec_scene (a floor and a back wall of material 0, an opaque teapot, one sphere emitter of
    `lights` lights up on the left), its description handed to `edit` before it is parsed"""
    mat = {"ka": [0.5, 0.5, 0.5], "kr": [0.0, 0.0, 0.0], "kt": [0.0, 0.0, 0.0], "ke": [0.0, 0.0, 0.0], "refractive_index": 1.0}
    d = {"AmbientLight": [0.1, 0.1, 0.1],
         "Camera": {"position": [0.0, -3.5, 1.0], "vector_x": [1.0, 0.0, 0.0], "vector_y": [0.0, -0.15, -1.0], "fov": 80, "focal_length": 1.0},
         "Materials": [
             dict(mat, id=0, ks=[ks, ks, ks], shininess=shin, texture={"type": "uniform", "color": [0.7, 0.7, 0.7]}),
             dict(mat, id=1, ks=[0.4, 0.4, 0.4], shininess=5.0, texture={"type": "uniform", "color": [0.8, 0.3, 0.2]}),
             dict(mat, id=2, ks=[0.0, 0.0, 0.0], ka=[0.0, 0.0, 0.0], ke=[1.0, 1.0, 1.0], shininess=0.0,
                  texture={"type": "uniform", "color": [0.0, 0.0, 0.0]})],
         "Objects": [
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 0.0, -1.0], "normal": [0.0, 0.0, 1.0]}},
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 5.0, 0.0], "normal": [0.0, -1.0, 0.0]}},
             {"type": "Mesh", "parameters": {"material": 1, "filename": "meshes/utah_teapot_lowpoly.stl", "position": [0.8, 2.5, -1.0],
                                             "rotation": [0.0, 0.0, 0.0], "scale": 0.04}},
             light([-5.0, 0.0, 2.5], lights)]}
    edit(d)
    return rtxpy.Scene.parse(json.dumps(d), name=name, base_dir=C.GOLDEN)


def light(pos, lights, radius=0.4):
    return {"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.0003, "position": list(pos), "radius": radius, "lights": lights}}


# ---- the option itself ----
def test_gpu_clearlane_option_values_and_default():
    scene = spec_scene(0.3, 5.0, 65, True)
    r = rtxpy.Renderer(0)
    try:
        r.set_option(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8)
        r.upload(scene)
        r.set_option(*SLOT64[0])
        for bad in (-1, 2, 64):
            with pytest.raises(Exception):
                r.set_option(CL, bad)
        r.render(scene.frame(48, 27), bench_params())
        assert r.stats().clear_points > 0  # on by default, and a refused value left it on
        r.set_option(CL, 0)
        r.render(scene.frame(48, 27), bench_params())
        assert r.stats().clear_points == 0
    finally:
        r.close()


# ---- frames ----
def test_gpu_clearlane_on_the_bench_scene():
    """scene5 with the dragon stand-in at bench.py's settings but 4 samples, a small frame: one emitter of 300 lights"""
    scene = load("scene5")
    on, cnt = check(renders(scene, scene.frame(96, 54), bench_params(4, 1)), nl=300)
    assert cnt.shadow_walk == abi.RTX_WALK_W8 and cnt.shadow_wave_walks > 0  # and the rest list still walks
    assert on.clear_points < on.shade_points


@pytest.mark.parametrize("lights", [64, 65, 300, 1024, 1025])
def test_gpu_clearlane_at_every_packet_count(lights):
    """one packet, a packet and one sample, 4.7 packets, 16 whole ones, 16 and one sample"""
    scene = spec_scene(0.3, 5.0, lights, True)
    on, cnt = check(renders(scene, scene.frame(96, 54), bench_params(), opts=W8, late=SLOT64), nl=lights)
    assert cnt.shadow_wave_walks > 0


def test_gpu_clearlane_two_emitters_whose_ranges_straddle_packets():
    """65 + 300 lights: emitter 1's samples begin at index 65, so every packet but the first holds index
    ranges of its own, and packet 1 holds samples of both (k_shadow hands it to light_sample)"""
    scene = edit_spec_scene("two", lambda d: d["Objects"].append(light([4.0, -1.0, 3.0], 300)))
    assert scene.desc.num_emitters == 2
    check(renders(scene, scene.frame(96, 54), bench_params(), opts=W8))


def test_gpu_clearlane_with_a_triangle_light(tmp_path):
    """the bench scene with a second sphere light and a triangle light, 428 samples a point"""
    scene = three_emitter_scene(tmp_path)
    check(renders(scene, scene.frame(96, 54), bench_params(2, 3)))


def test_gpu_clearlane_leaves_points_on_an_emitter_behind():
    """a second emitter in front of the camera: the points on it sample the other emitter alone, so their
    sample ranges are not the common ones; all-clear or not, they stay with k_shadow"""
    scene = edit_spec_scene("seen", lambda d: d["Objects"].append(light([-0.6, 1.5, 0.2], 300, 0.5)))
    on, cnt = check(renders(scene, scene.frame(96, 54), bench_params(), opts=W8))
    # a point on the emitter of 300 lights has 65 samples, one on the emitter of 65 (a GI ray found it) has 300, every
    # other point 365: the rays short of 365 a point tell that at least short / 300 points lie on an emitter
    short = on.shade_points * 365 - on.shadow_rays
    print("rays short of 365 a point", short)
    assert short > 0
    assert on.clear_rays == on.clear_points * 365 and on.clear_points <= on.shade_points - (short + 299) // 300


def test_gpu_clearlane_shininess_0_and_5_side_by_side():
    """the floor of shininess 0 and the wall of shininess 5 meet along an edge, and the Morton order runs across
    it: waves whose 64 points are all of shininess 0, all of 5, and both (those take the generic loop)"""
    def edit(d):
        wall = dict(d["Materials"][0], id=3, shininess=5.0)
        d["Materials"].append(wall)
        d["Objects"][1]["parameters"]["material"] = 3
    scene = edit_spec_scene("floorwall", edit, ks=0.3, shin=0.0, lights=300)
    for spec in (1, 0):
        check(renders(scene, scene.frame(96, 54), bench_params(), opts=W8, late=((abi.RTX_OPT_SHADOW_SPEC, spec),)), nl=300)


@pytest.mark.parametrize("att", [abi.RTX_ATT_NONE, abi.RTX_ATT_LIN, abi.RTX_ATT_SQR], ids=["none", "lin", "sqr"])
@pytest.mark.parametrize("refl", [abi.RTX_PHONG, abi.RTX_BLINN], ids=["phong", "blinn"])
def test_gpu_clearlane_under_every_shading_model(refl, att):
    scene = spec_scene(0.3, 5.0, 65, False)
    p = copy_params(bench_params(), reflection=refl, attenuation=att)
    check(renders(scene, scene.frame(96, 54), p, opts=W8, late=SLOT64), nl=65)


@pytest.mark.parametrize("rng", [abi.RTX_RNG_CONST, abi.RTX_RNG_COUNTER, abi.RTX_RNG_STRAT], ids=["const", "counter", "strat"])
def test_gpu_clearlane_under_every_rng(rng):
    scene = spec_scene(0.3, 5.0, 300, True)
    check(renders(scene, scene.frame(96, 54), bench_params(rng=rng), opts=W8), nl=300)


def test_gpu_clearlane_leaves_far_points_behind(tmp_path):
    """shade points beyond RTX_FRAME_FAR scene radii take no mask: they are in the rest list"""
    scene = far_shade_point_scene(tmp_path, 64)
    params = rtxpy.params_from_args(["-l", "none"], rng=abi.RTX_RNG_CONST)
    on, cnt = check(renders(scene, scene.frame(96, 96), params, opts=W8), nl=64)
    assert cnt.far_shadow_rays > 0 and on.clear_rays + cnt.far_shadow_rays <= on.shadow_rays


def test_gpu_clearlane_in_two_chunks():
    scene = spec_scene(0.3, 5.0, 65, True)
    frame = scene.frame(96, 54)
    tiles = ((96 + 7) // 8) * ((54 + 7) // 8)
    one = renders(scene, frame, bench_params(), opts=W8, late=SLOT64)
    two = renders(scene, frame, bench_params(), opts=W8, late=SLOT64 + ((abi.RTX_OPT_CHUNK_TILES, (tiles + 1) // 2),))
    (a, _), (b, _) = check(one, nl=65), check(two, nl=65)
    assert (a.chunks, b.chunks) == (1, 2) and a.clear_points == b.clear_points
    assert one[(1, 0)][:2] == two[(1, 0)][:2]


def test_gpu_clearlane_with_the_sort_off():
    """emission order: the identity stands in for the sorted order"""
    scene = spec_scene(0.3, 5.0, 65, True)
    frame = scene.frame(96, 54)
    srt = renders(scene, frame, bench_params(), opts=W8, late=SLOT64)
    raw = renders(scene, frame, bench_params(), opts=W8, late=SLOT64 + ((abi.RTX_OPT_SPSORT, 0),))
    (a, _), (b, _) = check(srt, nl=65), check(raw, nl=65)
    assert a.clear_points == b.clear_points and srt[(1, 0)][:2] == raw[(1, 0)][:2]


def test_gpu_clearlane_on_a_tile_list():
    scene = spec_scene(0.3, 5.0, 65, True)
    frame = scene.frame(96, 54)
    tiles = np.arange(0, 12 * 7, 3, dtype=np.uint32)
    check(renders(scene, frame, bench_params(), opts=W8, late=SLOT64, tiles=tiles), nl=65)


def test_gpu_clearlane_on_a_loopback_group_of_two():
    scene = spec_scene(0.3, 5.0, 65, True)
    frame = scene.frame(96, 54)
    one = renders(scene, frame, bench_params(), opts=W8, late=SLOT64)
    grp = renders(scene, frame, bench_params(), opts=W8, late=SLOT64, make=lambda: rtxpy.Group([0], loopback=2))
    (a, _), (g, _) = check(one, nl=65), check(grp, nl=65)
    assert g.devices == 2 and g.clear_points == a.clear_points
    assert one[(1, 0)][:2] == grp[(1, 0)][:2]


@pytest.mark.parametrize("late", [((abi.RTX_OPT_SHADOW_PREMASK, 0),), ((abi.RTX_OPT_SHADOW_POINT, 0),)], ids=["premask-off", "point-off"])
def test_gpu_clearlane_needs_the_premask_and_the_point_masks(late):
    scene = spec_scene(0.3, 5.0, 65, True)
    check(renders(scene, scene.frame(96, 54), bench_params(), opts=W8, late=SLOT64 + late), none=True)


def test_gpu_clearlane_leaves_the_lane_slots_alone():
    """100 lights: 4-lane slots, several points to a packet; the kernel takes none"""
    scene = spec_scene(0.3, 5.0, 100, True)
    check(renders(scene, scene.frame(96, 54), bench_params(), opts=W8), none=True)


# ---- the clear list's length ----
def floor_scene(lights):
    """a camera looking down at a floor lit by one sphere emitter off to one side, a plain sphere off to the other
    (the two span the bounded objects' box, so the floor below is not far from it): with no GI and no reflection
    every pixel is one shade point on the floor, and every one is all-clear"""
    mat = {"ka": [0.5, 0.5, 0.5], "kr": [0.0, 0.0, 0.0], "kt": [0.0, 0.0, 0.0], "ke": [0.0, 0.0, 0.0], "refractive_index": 1.0}
    d = {"AmbientLight": [0.1, 0.1, 0.1],
         "Camera": {"position": [0.0, 0.0, 2.0], "vector_x": [1.0, 0.0, 0.0], "vector_y": [0.0, -1.0, 0.0], "fov": 40, "focal_length": 1.0},
         "Materials": [
             dict(mat, id=0, ks=[0.3, 0.3, 0.3], shininess=5.0, texture={"type": "uniform", "color": [0.7, 0.7, 0.7]}),
             dict(mat, id=1, ks=[0.0, 0.0, 0.0], ka=[0.0, 0.0, 0.0], ke=[1.0, 1.0, 1.0], shininess=0.0,
                  texture={"type": "uniform", "color": [0.0, 0.0, 0.0]})],
         "Objects": [
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 0.0, -1.0], "normal": [0.0, 0.0, 1.0]}},
             {"type": "Sphere", "parameters": {"material": 0, "epsilon": 0.0003, "position": [6.0, 0.0, 2.5], "radius": 0.4}},
             {"type": "Sphere", "parameters": {"material": 1, "epsilon": 0.0003, "position": [-6.0, 0.0, 2.5], "radius": 0.4, "lights": lights}}]}
    return rtxpy.Scene.parse(json.dumps(d), name="floor", base_dir=C.GOLDEN)


@pytest.mark.parametrize("w,h", [(1, 1), (9, 7), (8, 8), (13, 5), (15, 9), (31, 17)], ids=["1", "63", "64", "65", "135", "527"])
def test_gpu_clearlane_list_lengths(w, h):
    """a wave's first lane alone, a wave one lane short, a whole wave, a wave and one lane, two waves and seven
    lanes, two workgroups and fifteen lanes"""
    scene = floor_scene(65)
    params = rtxpy.params_from_args(["-g", "none"], seed=3)
    params.rng = abi.RTX_RNG_COUNTER
    on, _ = check(renders(scene, scene.frame(w, h), params, late=SLOT64), nl=65)
    assert on.shade_points == w * h and on.clear_points == w * h
