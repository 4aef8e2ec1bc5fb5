"""k_shadow's per-point masks (rtx.h RTX_OPT_SHADOW_POINT, rtx_shadow.hip point_masks / clear_run):
a shade point with 64 light samples or more decides once, per emitter, that no ray from it to the
emitter can meet a plane (plane_clear) or an object tested one by one (the cone test against the
records' bounding spheres, rtx_upload.cpp build_lsph); its packets skip those tests, and a point clear
of the tree, the planes and the records runs its packets without any shadow query.

 1. soundness: over seeded cases, no (point, light, plane / record) has its clear bit set together
    with a blocking sample; the samples are k_shadow's own (sample_ray) and the blocking test is
    both the kernel's per-ray function and a float32 numpy restatement of hit_plane;
 2. the frames are the same bit for bit with the option on, off and with every cull off;
 3. on the bench scene most cone-clear rays belong to all-clear points.
"""
import json

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi
from test_gpu_configs import load
from test_gpu_cull import three_emitter_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
EPS = np.array([1e-4, 2.5e-4, 1e-3], f32)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def dot32(a, b):
    """rtx_math.h dot3 in float32, its operation order"""
    a, b = a.astype(f32), b.astype(f32)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def hit_plane_blocks(n, dd, o, d, eps, dist):
    """hit_plane (object.c:473-488) && t < dist, float32 with IEEE division"""
    a = dot32(n, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (dd.astype(f32) - dot32(n, o)) / a
    return (np.abs(a) >= eps) & (t > eps) & (t < dist)


def light_fields(rng, centre, size, tri):
    """v0 v1 v2 r of a light about `centre`: a sphere of radius `size`, or a triangle within it"""
    n = len(centre)
    v = np.zeros((n, 10))
    v[:, 0:3] = centre
    v[:, 9] = size
    for k in range(3):
        corner = centre + unit(rng.normal(size=(n, 3))) * size[:, None] * rng.uniform(0.3, 1.0, (n, 1))
        v[:, 3 * k:3 * k + 3] = np.where(tri[:, None], corner, v[:, 3 * k:3 * k + 3])
    return v


def plane_cases(seed, n):
    """points on, just off and away from a plane of any orientation and normal length, at
    coordinates up to 1e4, with sphere and triangle lights clear of, grazing, touching and
    straddling the plane on either side; returns the records, the lights' geometric height over
    the plane in light sizes, and the point's signed geometric height"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(0, 5, n)  # |coordinates| up to 1e4
    nu = unit(rng.normal(size=(n, 3)))
    axis = rng.random(n) < 0.15
    nu[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * rng.choice([-1.0, 1.0], (axis.sum(), 1))
    nlen = np.where(rng.random(n) < 0.5, 1.0, 10.0 ** rng.uniform(-1, 1, n))  # non-unit normals
    q0 = rng.uniform(-1, 1, (n, 3)) * scale[:, None]
    t1 = unit(np.cross(nu, rng.normal(size=(n, 3))))
    t2 = np.cross(nu, t1)
    reach = scale * 10.0 ** rng.uniform(-1.5, 0.5, n)  # the scene's extent about q0
    # the point: on the plane, a hair off it (either side), or well off it (either side)
    kind = rng.integers(0, 5, n)
    hp = np.select([kind == 0, kind <= 2, kind >= 3],
                   [0.0, 10.0 ** rng.uniform(-7, -2, n) * np.maximum(reach, 1e-3), reach * rng.uniform(0.02, 1.0, n)])
    hp = hp * rng.choice([-1.0, 1.0], n)
    p = q0 + t1 * (rng.uniform(-1, 1, n) * reach)[:, None] + t2 * (rng.uniform(-1, 1, n) * reach)[:, None] + nu * hp[:, None]
    # the light: size, and its centre's height over the plane in sizes
    size = reach * 10.0 ** rng.uniform(-2.5, -0.3, n)
    rel = rng.choice([0.0, 0.5, 0.999, 1.0, 1.001, 1.01, 1.5, 3.0, 30.0], n) * rng.choice([-1.0, 1.0], n)
    lc = q0 + t1 * (rng.uniform(-1, 1, n) * reach)[:, None] + t2 * (rng.uniform(-1, 1, n) * reach)[:, None] + nu * (rel * size)[:, None]
    tri = rng.random(n) < 0.3
    x = np.zeros((n, 21))
    x[:, 0:3] = p
    x[:, 3] = tri
    x[:, 4:14] = light_fields(rng, lc, size, tri)
    x[:, 14:17] = nu * nlen[:, None]
    x[:, 18] = rng.choice(EPS, n)
    x[:, 19:21] = rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)
    x = x.astype(f32)
    # dd from the float32 normal and plane point, as a scene file's plane has it
    x[:, 17] = (x[:, 14:17].astype(np.float64) * q0.astype(f32)).sum(1).astype(f32)
    return x, rel, hp, tri


def test_gpu_plane_clear_is_sound():
    x, rel, hp, tri = plane_cases(11, 6000)
    y = rtxpy.gpu_kat(abi.KAT_PLANE_CLEAR, x)
    clear, blocks = y[:, 0] > 0, y[:, 1] > 0
    ref = hit_plane_blocks(x[:, 14:17], x[:, 17], x[:, 0:3], y[:, 2:5], x[:, 18], y[:, 5])
    print("plane cases", len(x), "clear", int(clear.sum()), "blocking", int(blocks.sum()), "restated blocking", int(ref.sum()),
          "clear on the plane", int((clear & (hp == 0)).sum()), "clear with a triangle light", int((clear & tri).sum()))
    assert not (clear & blocks).any()
    assert not (clear & ref).any()
    # a sphere light that touches or straddles the plane is never clear
    assert not clear[~tri & (np.abs(rel) <= 1.0)].any()
    # the plane between point and light: never clear (points more than two epsilons off the plane;
    # nearer ones count as on it: t <= eps), and those rays do cross it
    between = (np.sign(hp) == -np.sign(rel)) & (np.abs(rel) >= 1.01) & (np.abs(hp) > 2.0 * x[:, 18])
    assert between.sum() > 300 and not clear[between].any()
    assert blocks[between & ~tri].mean() > 0.5
    # the predicate is not vacuous: points on the plane, beside it and triangle lights do clear
    assert (clear & (hp == 0)).sum() > 100
    assert (clear & (np.sign(hp) == np.sign(rel)) & (np.abs(hp) > 2.0 * x[:, 18])).sum() > 100
    assert (clear & tri).sum() > 50
    assert (clear & (np.abs(x[:, 0:3]).max(1) > 1e3)).sum() > 20


def test_gpu_plane_clear_near_the_light():
    """the bench scene's case: a point on a plane the light hangs 0.5 and 3.5 above, epsilon 1e-4"""
    rng = np.random.default_rng(5)
    n = 2000
    x = np.zeros((n, 21), f32)
    d = 10.0 ** rng.uniform(-1, 2.5, n)  # the point's distance from the light's foot, 0.1 .. 300
    ang = rng.uniform(0, 2 * np.pi, n)
    x[:, 0], x[:, 1] = d * np.cos(ang), d * np.sin(ang)
    x[:, 2] = rng.choice([0.0, 1e-7, -1e-7, 3e-6, -3e-6], n)
    x[:, 6] = rng.choice([0.5, 3.5], n) + 0.25  # sphere light of radius 0.25 about (0, 0, h + r)
    x[:, 13] = 0.25
    x[:, 16] = 1.0
    x[:, 18] = 1e-4
    x[:, 19:21] = rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)
    y = rtxpy.gpu_kat(abi.KAT_PLANE_CLEAR, x)
    clear, blocks = y[:, 0] > 0, y[:, 1] > 0
    assert not (clear & blocks).any()
    assert not (clear & hit_plane_blocks(x[:, 14:17], x[:, 17], x[:, 0:3], y[:, 2:5], x[:, 18], y[:, 5])).any()
    near = (x[:, 2] == 0) & (d < 20)
    assert clear[near].all()  # on the plane within tens of units: |s| = 0 <= eps a_min


def test_gpu_record_clear_is_sound():
    """the listed records: spheres and triangles about the cone from the point around the light,
    inside it, outside it and across its edge"""
    rng = np.random.default_rng(23)
    n = 6000
    scale = 10.0 ** rng.integers(0, 4, n)
    p = rng.uniform(-1, 1, (n, 3)) * scale[:, None]
    ax = unit(rng.normal(size=(n, 3)))
    L = scale * 10.0 ** rng.uniform(-1, 0.5, n)
    size = L * 10.0 ** rng.uniform(-2, -0.4, n)
    lc = p + ax * L[:, None]
    tri = rng.random(n) < 0.3
    # the record: at distance t along the axis and e off it, e about the cone's radius there
    t = L * rng.choice([-0.2, 0.1, 0.5, 0.9, 1.0, 1.3], n) * rng.uniform(0.8, 1.2, n)
    rr = L * 10.0 ** rng.uniform(-2.5, -0.5, n)
    cone_r = np.abs(t) * size / L
    e = (cone_r + rr) * rng.choice([0.0, 0.5, 0.99, 1.0, 1.001, 1.01, 1.1, 2.0, 10.0], n)
    side = unit(np.cross(ax, rng.normal(size=(n, 3))))
    rc = p + ax * t[:, None] + side * e[:, None]
    rtri = rng.random(n) < 0.4
    x = np.zeros((n, 28))
    x[:, 0:3] = p
    x[:, 3] = tri
    x[:, 4:14] = light_fields(rng, lc, size, tri)
    x[:, 14] = rtri
    x[:, 15:25] = light_fields(rng, rc, rr, rtri)
    x[:, 25] = rng.choice(EPS, n)
    x[:, 26:28] = rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)
    y = rtxpy.gpu_kat(abi.KAT_LIN_CLEAR, x.astype(f32))
    clear, blocks = y[:, 0] > 0, y[:, 1] > 0
    print("record cases", n, "clear", int(clear.sum()), "blocking", int(blocks.sum()))
    assert not (clear & blocks).any()
    assert clear.sum() > 500 and blocks.sum() > 300
    assert (clear & rtri).sum() > 100 and (clear & tri).sum() > 100


# ---- frames ----
def render_modes(scene, frame, params, slot=0, frame_opt=abi.RTX_FRAME_AUTO):
    """the frame with the masks on, off (the cone cull still on) and with every cull off, from the
    product and the counting kernels"""
    out = {}
    r = rtxpy.Renderer(0)
    try:
        r.set_option(abi.RTX_OPT_TREE_FRAME, frame_opt)
        r.upload(scene)
        r.set_option(abi.RTX_OPT_SHADOW_SLOT, slot)
        for mode, (cull, point) in {"on": (1, 1), "off": (1, 0), "nocull": (0, 1)}.items():
            r.set_option(abi.RTX_OPT_SHADOW_CULL, cull)
            r.set_option(abi.RTX_OPT_SHADOW_POINT, point)
            for count in (0, 1):
                p = rtxpy.default_params(**{f: getattr(params, f) for f, _ in abi.Params._fields_})
                p.count_traversal = count
                rgb, z = r.render(frame, p)
                out[(mode, count)] = (rgb, z, r.stats())
    finally:
        r.close()
    return out


def check_same(out):
    rgb0, z0, s0 = out[("nocull", 0)]
    for key, (rgb, z, s) in out.items():
        assert np.array_equal(rgb, rgb0) and np.array_equal(z, z0), key
        assert (s.closest_rays, s.shadow_rays, s.shade_points) == (s0.closest_rays, s0.shadow_rays, s0.shade_points), key
    for mode in ("off", "nocull"):  # option 0 (or every cull off): nothing is skipped
        s = out[(mode, 1)][2]
        assert (s.shadow_plane_skipped, s.shadow_lin_skipped, s.shadow_point_clear) == (0, 0, 0), mode
    on, off = out[("on", 1)][2], out[("off", 1)][2]
    # the plane tests run and those skipped are the tests the option-0 frame runs
    assert on.shadow_plane_tests + on.shadow_plane_skipped == off.shadow_plane_tests
    assert on.shadow_cone_clear == off.shadow_cone_clear
    return on


@pytest.fixture(scope="module")
def bench_frame():
    scene = load("scene5")
    frame = scene.frame(320, 180)
    params = rtxpy.params_from_args(["-g", "path", "-n", "4"], seed=1)
    params.rng = abi.RTX_RNG_COUNTER
    return render_modes(scene, frame, params)


def test_gpu_point_masks_are_invisible_on_the_bench_scene(bench_frame):
    on = check_same(bench_frame)
    print("scene5 plane tests skipped", on.shadow_plane_skipped, "of", on.shadow_plane_skipped + on.shadow_plane_tests)


def test_gpu_point_masks_clear_most_of_the_bench_scene(bench_frame):
    """the light clears the two planes by 3.5 and 0.5 units and epsilon is 1e-4, so the near-plane
    rule holds for floor and wall points out to tens of units: at least half the cone-clear rays
    belong to all-clear points"""
    on = bench_frame[("on", 1)][2]
    print("scene5 point_clear", on.shadow_point_clear, "cone_clear", on.shadow_cone_clear, "ratio",
          round(on.shadow_point_clear / max(1, on.shadow_cone_clear), 4), "shadow rays", on.shadow_rays)
    assert on.shadow_plane_skipped > 0
    assert 0 < on.shadow_point_clear <= on.shadow_cone_clear
    assert on.shadow_point_clear >= 0.5 * on.shadow_cone_clear


@pytest.mark.parametrize("name", ["s1_path2", "s2_blinn_lin", "s3_path2", "s3_none_b3"])
def test_gpu_point_masks_are_invisible_on_the_golden_configs(name):
    scene, frame, params, _ = C.load_config(name)
    on = check_same(render_modes(scene, frame, params, slot=64))  # 64-lane packets: one point per packet
    print(name, "planes skipped", on.shadow_plane_skipped, "objects skipped", on.shadow_lin_skipped, "all-clear rays",
          on.shadow_point_clear, "of", on.shadow_rays)


def test_gpu_point_masks_with_three_emitters(tmp_path):
    scene = three_emitter_scene(tmp_path)
    frame = scene.frame(160, 90)
    params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=3)
    params.rng = abi.RTX_RNG_COUNTER
    on = check_same(render_modes(scene, frame, params))
    print("three emitters: all-clear rays", on.shadow_point_clear, "objects skipped", on.shadow_lin_skipped)
    assert on.shadow_point_clear > 0 and on.shadow_lin_skipped > 0


def handmade_scene(tmp_path):
    """a tilted floor, a transparent tilted pane, a back wall a sphere light comes within 1e-3 of,
    a triangle light above, and a light behind the pane (and behind the floor's far end) from part
    of the frame; few objects, so they are tested one by one (RTX_WALK_LINEAR), and 256 lights, so a
    point's samples fill 64-lane packets of their own"""
    def mat(i, color, kt=(0.0, 0.0, 0.0), ke=(0.0, 0.0, 0.0), ks=(0.3, 0.3, 0.3)):
        return {"id": i, "ks": list(ks), "ka": [0.5, 0.5, 0.5], "kr": [0.0, 0.0, 0.0], "kt": list(kt), "ke": list(ke),
                "shininess": 8.0, "refractive_index": 1.0, "texture": {"type": "uniform", "color": list(color)}}

    def plane(m, pos, nrm):
        return {"type": "Plane", "parameters": {"material": m, "epsilon": 0.00025, "position": pos, "normal": nrm}}

    def sphere(m, pos, r, lights=None):
        o = {"type": "Sphere", "parameters": {"material": m, "epsilon": 0.00025, "position": pos, "radius": r}}
        if lights:
            o["parameters"]["lights"] = lights
        return o

    wall_q, wall_n = np.array([0.0, 9.0, 0.0]), np.array([0.1, 1.0, 0.05])
    wall_u = wall_n / np.linalg.norm(wall_n)
    near_wall = [float(v) for v in wall_q - 0.801 * wall_u + 3.0 * unit(np.cross(wall_u, [1.0, 0.0, 0.0]))]
    d = {"AmbientLight": [0.1, 0.1, 0.1],
         "Camera": {"position": [0.0, -6.0, 1.5], "vector_x": [1.0, 0.0, 0.0], "vector_y": [0.0, 1.0, -0.1], "fov": 80,
                    "focal_length": 1.0},
         "Materials": [mat(0, (0.7, 0.7, 0.7)), mat(1, (0.2, 0.5, 0.8)), mat(2, (0.9, 0.9, 0.9), kt=(0.6, 0.8, 0.7)),
                       mat(3, (0.0, 0.0, 0.0), ke=(1.0, 1.0, 1.0), ks=(0.0, 0.0, 0.0)), mat(4, (0.8, 0.3, 0.2))],
         "Objects": [plane(0, [0.0, 0.0, -1.0], [0.05, -0.12, 1.0]),          # the tilted floor
                     plane(1, [float(v) for v in wall_q], [float(v) for v in wall_n]),  # the back wall
                     plane(2, [2.5, 0.0, 0.0], [1.0, 0.2, 0.1]),              # a transparent pane
                     sphere(4, [-1.5, 2.0, 0.0], 1.0),
                     sphere(4, [1.0, 4.0, -0.2], 0.7),
                     sphere(3, near_wall, 0.8, lights=96),                    # its surface 1e-3 short of the back wall
                     sphere(3, [5.0, 1.0, 1.0], 0.3, lights=96),              # behind the pane from the left
                     {"type": "Triangle", "parameters": {"material": 3, "epsilon": 0.0001, "lights": 64,
                                                         "vertex_1": [-3.0, 0.0, 4.0], "vertex_2": [-2.0, 0.0, 4.0],
                                                         "vertex_3": [-2.5, 1.0, 4.2]}}]}
    path = tmp_path / "handmade.json"
    path.write_text(json.dumps(d))
    return rtxpy.Scene.load(str(path), base_dir=str(tmp_path))


@pytest.mark.parametrize("frame_opt", [abi.RTX_FRAME_AUTO, abi.RTX_FRAME_WORLD])
def test_gpu_point_masks_on_a_handmade_scene(tmp_path, frame_opt):
    scene = handmade_scene(tmp_path)
    frame = scene.frame(160, 90)
    params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=7)
    params.rng = abi.RTX_RNG_COUNTER
    out = render_modes(scene, frame, params, frame_opt=frame_opt)
    on = check_same(out)
    print("handmade frame", frame_opt, "planes skipped", on.shadow_plane_skipped, "run", on.shadow_plane_tests,
          "objects skipped", on.shadow_lin_skipped, "all-clear rays", on.shadow_point_clear, "of", on.shadow_rays)
    assert on.shadow_plane_skipped > 0 and on.shadow_plane_tests > 0 and on.shadow_lin_skipped > 0
