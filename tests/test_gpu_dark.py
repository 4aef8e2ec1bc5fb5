"""k_shadow's dark samples (rtx.h RTX_OPT_SHADOW_DARK, rtx_shadow.hip dark_terms / sample_dark): a
light sample whose diffuse and specular factors are both 0 adds +-0 to its shade point whether or
not its shadow ray is blocked and whatever transmittance it gathers, so the wave-uniform path
answers it without a shadow query (where shadow rays walk a tree and the cone cull has not
already cleared the packet).

 1. the predicate: over seeded cases, whenever it holds, shade_terms is +-0 in every channel for the
    sample's li and for li times a transmittance (the kernel's own functions, RTX_KAT_DARK); the
    cases' make-up is checked on the CPU by a numpy restatement first;
 2. the frames are the same bit for bit with the option on and off, product and counting kernels;
 3. the counters are non-zero where an object is lit from one side, zero with the option off or
    where the scene's transmittances forbid it.
"""
import json
import os

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

f32 = np.float32
SHININESS = np.array([0.0, 1.0, 2.0, 5.0, 4.5, -1.0], f32)
EDGE = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-7, -1e-7], f32)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def dot32(a, b):
    """rtx_math.h dot3 in float32, its operation order"""
    a, b = a.astype(f32), b.astype(f32)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def dark_cases(seed, n):
    """KAT_DARK records: n3 view3 kd3 ks3 shin ldir3 ldist li3 att att_offset refl kt3.  A third are
    `edge` cases with the normal on the z axis, so that a = ldir.n is exactly ldir's z (+-0, +-1e-30,
    +-1e-7) and the specular multiplier is exactly +-0 or +- tiny: Phong with ldir = (+-1, 0, a) and the
    view direction (t, 1, 0), sm = +-t; Blinn with view.z = a + t, sm = -(t / |view - ldir|)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 26), f32)
    nrm = unit(rng.normal(size=(n, 3)))
    ldir = unit(rng.normal(size=(n, 3)))
    behind = rng.random(n) < 0.65  # most lights behind the surface
    a = (ldir * nrm).sum(1)
    ldir = np.where(((a > 0) & behind)[:, None], ldir - 2 * a[:, None] * nrm, ldir)
    view = unit(rng.normal(size=(n, 3)))
    refl = rng.integers(0, 2, n)
    edge = rng.random(n) < 0.33
    ne = int(edge.sum())
    ea = np.where(rng.random(ne) < 0.7, rng.choice(EDGE, ne), rng.uniform(-1, 1, ne).astype(f32)).astype(f32)
    et = rng.choice(EDGE, ne)
    lxy = unit(rng.normal(size=(ne, 2))) * rng.choice([-1.0, 1.0], (ne, 1))
    nrm[edge] = [0.0, 0.0, 1.0]
    phong = (refl[edge] == abi.RTX_PHONG)[:, None]
    ldir[edge] = np.where(phong, np.stack([np.sign(lxy[:, 0]), np.zeros(ne), ea], 1), np.stack([lxy[:, 0], lxy[:, 1], ea], 1))
    phong_view = np.stack([et, np.ones(ne), np.zeros(ne)], 1)
    blinn_view = np.stack([rng.uniform(-1, 1, ne), rng.uniform(-1, 1, ne), (ea + et).astype(f32)], 1)
    view[edge] = np.where(phong, phong_view, blinn_view)
    x[:, 0:3] = nrm
    x[:, 3:6] = view
    x[:, 6:9] = np.where((rng.random(n) < 0.2)[:, None], 0.0, rng.uniform(0.05, 1.0, (n, 3)))  # kd
    x[:, 9:12] = np.where((rng.random(n) < 0.3)[:, None], 0.0, rng.uniform(0.05, 1.0, (n, 3)))  # ks
    x[:, 12] = rng.choice(SHININESS, n)
    x[:, 13:16] = ldir
    x[:, 16] = rng.uniform(0.5, 20.0, n)
    zero_len = rng.random(n) < 0.05  # ldist = 0: the direction is 0 * inf
    x[zero_len, 13:16] = np.nan
    x[zero_len, 16] = 0.0
    x[:, 17:20] = rng.uniform(0.01, 3.0, (n, 3))  # li
    bad_li = rng.random(n) < 0.03
    x[bad_li, 17] = rng.choice(np.array([np.inf, np.nan], f32), int(bad_li.sum()))
    x[:, 20] = rng.integers(0, 3, n)  # RTX_ATT_NONE / LIN / SQR
    x[:, 21] = rng.choice(np.array([1.0, 0.0], f32), n, p=[0.8, 0.2])
    x[:, 22] = refl
    x[:, 23:26] = rng.choice(np.array([0.0, 0.32, 0.95, 1.0], f32), (n, 3))
    big_kt = rng.random(n) < 0.03
    x[big_kt, 24] = 1.5
    return x, edge


def restate(x):
    """the predicate's meaning, from the reference's formulas (render.c:199-228) in float32: the
    factors pd and pw, and `dark` = both terms are surely 0 and nothing in them is infinite"""
    n, view, kd, ks, shin, ldir, ldist = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12], x[:, 13:16], x[:, 16]
    li, att, off, refl, kt = x[:, 17:20], x[:, 20], x[:, 21], x[:, 22], x[:, 23:26]
    with np.errstate(all="ignore"):
        a = dot32(ldir, n)
        pd = np.where(a > 0, a, f32(0))  # fmaxf(0, a): a NaN gives 0
        h = view - ldir
        hn = h * (f32(1) / np.sqrt(dot32(h, h)))[:, None]
        sm = np.where(refl == abi.RTX_BLINN, -dot32(n, hn), -dot32(n * (f32(2) * a)[:, None] - ldir, view))
        odd = (np.rint(shin) == shin) & (np.rint(shin / 2) != shin / 2)
        whole = np.rint(shin) == shin
        # powf(sm, shin) clamped at 0: sm < 0 gives a value above 0 only for an even power, sm = 0 gives
        # 0 for a power above 0, a NaN gives 0
        pw_zero = np.where(shin == 0, False, np.isnan(sm) | ((sm < 0) & (odd | ~whole)) | ((sm == 0) & (shin > 0)))
        attf = np.select([att == abi.RTX_ATT_LIN, att == abi.RTX_ATT_SQR], [f32(1) / (off + ldist), f32(1) / (off + ldist * ldist)], f32(1))
        ok = np.isfinite(li).all(1) & (np.abs(kt) <= 1).all(1) & np.isfinite(attf)
        pw_inf = (sm == 0) & (shin < 0)
        dark = ok & ((pd == 0) | (kd == 0).all(1)) & (pw_zero | ((ks == 0).all(1) & ~pw_inf))
        # an even power: light from behind still shines (sm well away from 0, whose square underflows)
        leak = (a < 0) & (sm < -1e-6) & (shin == 2) & (ks > 0).all(1) & ok
    return dark, leak, a, sm


def test_dark_cases_are_not_vacuous():
    """the generator on the CPU: a quarter of the cases and more are dark by the restatement, the
    even-shininess leak and every edge value are there"""
    x, edge = dark_cases(41, 10000)
    dark, leak, a, sm = restate(x)
    print("cases", len(x), "dark", int(dark.sum()), "leak", int(leak.sum()), "edge", int(edge.sum()))
    assert dark.mean() >= 0.25
    assert leak.sum() >= 100
    for v in EDGE:
        same = (a[edge] == v) & (np.signbit(a[edge]) == np.signbit(v))
        assert same.sum() >= 20, v
    assert ((sm[edge] == 0) & np.signbit(sm[edge])).sum() >= 20 and ((sm[edge] == 0) & ~np.signbit(sm[edge])).sum() >= 20
    assert ((np.abs(sm[edge]) > 0) & (np.abs(sm[edge]) < 1e-20)).sum() >= 50
    for s in SHININESS:
        assert (x[:, 12] == s).sum() >= 1000
    for col, lo in ((6, 1000), (9, 1000)):
        assert (x[:, col:col + 3] == 0).all(1).sum() >= lo  # kd = 0, ks = 0
    assert (x[:, 16] == 0).sum() >= 200 and np.isnan(x[x[:, 16] == 0, 13]).all()
    for att in (abi.RTX_ATT_NONE, abi.RTX_ATT_LIN, abi.RTX_ATT_SQR):
        for refl in (abi.RTX_PHONG, abi.RTX_BLINN):
            assert ((x[:, 20] == att) & (x[:, 22] == refl)).sum() >= 1000


@pytest.mark.gpu
def test_gpu_dark_samples_shade_to_zero():
    x, edge = dark_cases(41, 10000)
    want, leak, a, sm = restate(x)
    y = rtxpy.gpu_kat(abi.KAT_DARK, x)
    dark = y[:, 0] > 0
    print("cases", len(x), "dark on the device", int(dark.sum()), "by the restatement", int(want.sum()), "both", int((dark & want).sum()),
          "leak cases", int(leak.sum()))
    # whenever the predicate holds, all six terms are +-0 (a NaN fails the comparison too)
    assert (y[dark, 1:7] == 0).all()
    # not vacuous: a quarter of the cases, edge cases among them
    assert dark.mean() >= 0.25
    assert (dark & edge).sum() >= 300
    # an even power of a negative specular multiplier is above 0: never dark, and the term is there
    assert leak.sum() >= 100 and not dark[leak].any()
    assert (y[leak, 1:4] > 0).all()
    # an infinite or NaN emitter, a transmittance above 1: the scene's flag is off
    flag_off = ~np.isfinite(x[:, 17:20]).all(1) | (np.abs(x[:, 23:26]) > 1).any(1)
    assert flag_off.sum() >= 300 and not dark[flag_off].any()
    # the device and the restatement agree away from powf's underflow and the exact zeros of sm
    # (the device forms sm with its own rounding; its sign is only sure well away from 0)
    sure = ~edge & (np.abs(sm) > 1e-6) & (np.abs(a) > 1e-6)
    assert sure.sum() >= 4000 and (dark[sure] == want[sure]).all()


# ---- frames ----
def render_dark(scene, frame, params, slot=0, frame_opt=abi.RTX_FRAME_AUTO, walk=abi.RTX_WALK_AUTO, variants=(None,)):
    """the frame with the option on and off from the product and the counting kernels, for each
    (reflection, attenuation) variant: {(variant, dark, count): (rgb, z, stats)}"""
    out = {}
    r = rtxpy.Renderer(0)
    try:
        r.set_option(abi.RTX_OPT_TREE_FRAME, frame_opt)
        r.set_option(abi.RTX_OPT_SHADOW_WALK, walk)
        r.upload(scene)
        r.set_option(abi.RTX_OPT_SHADOW_SLOT, slot)
        for v in variants:
            for dark in (1, 0):
                r.set_option(abi.RTX_OPT_SHADOW_DARK, dark)
                for count in (0, 1):
                    p = rtxpy.default_params(**{f: getattr(params, f) for f, _ in abi.Params._fields_})
                    if v is not None:
                        p.reflection, p.attenuation = v
                    p.count_traversal = count
                    rgb, z = r.render(frame, p)
                    out[(v, dark, count)] = (rgb, z, r.stats())
    finally:
        r.close()
    return out


def check_same(out):
    """every render of a variant equals its option-0 product frame; returns the summed dark
    counters of the option-1 counting renders"""
    rays = packets = 0
    for (v, dark, count), (rgb, z, s) in out.items():
        rgb0, z0, s0 = out[(v, 0, 0)]
        key = (v, dark, count)
        assert np.array_equal(rgb, rgb0) and np.array_equal(z, z0), key
        assert (s.closest_rays, s.shadow_rays, s.shade_points) == (s0.closest_rays, s0.shadow_rays, s0.shade_points), key
        if not (dark and count):
            assert (s.shadow_dark_rays, s.shadow_dark_packet_rays) == (0, 0), key
        else:
            assert s.shadow_dark_packet_rays <= s.shadow_dark_rays <= s.shadow_rays, key
            off = out[(v, 0, 1)][2]
            # the plane tests are counted for dark rays too; the cone cull's count does not move
            assert (s.shadow_plane_tests, s.shadow_cone_clear) == (off.shadow_plane_tests, off.shadow_cone_clear), key
            rays += s.shadow_dark_rays
            packets += s.shadow_dark_packet_rays
    return rays, packets


@pytest.mark.gpu
def test_gpu_dark_is_invisible_on_the_bench_scene():
    from test_gpu_configs import load
    scene = load("scene5")
    frame = scene.frame(160, 90)
    params = rtxpy.params_from_args(["-g", "path", "-n", "64"], seed=1)
    params.rng = abi.RTX_RNG_COUNTER
    out = render_dark(scene, frame, params)
    rays, packets = check_same(out)
    on, off = out[(None, 1, 1)][2], out[(None, 0, 1)][2]
    print("scene5 dark rays", rays, "in dark packets", packets, "of", on.shadow_rays, "wave walks", on.shadow_wave_walks, "against",
          off.shadow_wave_walks, "wave steps", on.shadow_wave_steps, "against", off.shadow_wave_steps)
    # the dragon's far side is lit from one side: whole packets go dark and their walks go
    assert rays > 0 and packets > 0
    assert on.shadow_wave_walks < off.shadow_wave_walks and on.shadow_wave_steps < off.shadow_wave_steps


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s1_path2", "s2_blinn_lin", "s3_path2", "s3_none_b3"])
def test_gpu_dark_is_invisible_on_the_golden_configs(name):
    scene, frame, params, _ = C.load_config(name)
    rays, packets = check_same(render_dark(scene, frame, params, slot=64))  # 64-lane packets: one point per packet
    print(name, "dark rays", rays, "in dark packets", packets)


MATERIALS = {"even": {"ks": [0.4, 0.4, 0.4], "shininess": 2.0}, "odd": {"ks": [0.4, 0.4, 0.4], "shininess": 5.0},
             "matte": {"ks": [0.0, 0.0, 0.0], "shininess": 5.0}, "pane": {"ks": [0.4, 0.4, 0.4], "shininess": 5.0}}
VARIANTS = tuple((refl, att) for refl in (abi.RTX_PHONG, abi.RTX_BLINN) for att in (abi.RTX_ATT_NONE, abi.RTX_ATT_LIN, abi.RTX_ATT_SQR))


def dark_side_scene(material, kt=None):
    """tests/golden/scenes/dark_side.json: a sphere, a small mesh and a small matte sphere on a
    floor, lit from the left by one sphere light of 128 samples; `material` sets the first two
    objects' ks and shininess (the matte sphere's far side is dark under any of them), "pane" also
    hangs a transparent sphere between the light and them (kt: its transmittance)"""
    with open(os.path.join(C.SCENES, "dark_side.json")) as fh:
        d = json.load(fh)
    d["Materials"][1].update(MATERIALS[material])
    if material == "pane":
        d["Objects"].append({"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.00025, "position": [-3.5, 1.5, 1.2], "radius": 0.9}})
    if kt is not None:
        d["Materials"][2]["kt"] = list(kt)
    return rtxpy.Scene.parse(json.dumps(d), name="dark_side", base_dir=C.GOLDEN)


@pytest.mark.gpu
@pytest.mark.parametrize("frame_opt", [abi.RTX_FRAME_AUTO, abi.RTX_FRAME_WORLD])
@pytest.mark.parametrize("material", list(MATERIALS))
def test_gpu_dark_on_a_scene_lit_from_one_side(material, frame_opt):
    """Phong and Blinn, the three attenuations, the threaded and the 8-wide walk, both tree frames"""
    scene = dark_side_scene(material)
    frame = scene.frame(96, 54)
    params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=7)
    params.rng = abi.RTX_RNG_COUNTER
    for walk in (abi.RTX_WALK_AUTO, abi.RTX_WALK_W8):
        out = render_dark(scene, frame, params, frame_opt=frame_opt, walk=walk, variants=VARIANTS)
        rays, packets = check_same(out)
        print(material, "frame", frame_opt, "walk", abi.WALK_NAMES[out[(VARIANTS[0], 1, 1)][2].shadow_walk], "dark rays", rays,
              "in dark packets", packets)
        assert rays > 0 and packets > 0


@pytest.mark.gpu
def test_gpu_dark_keeps_the_even_power_leak():
    """shininess 2 leaves fewer dark samples than shininess 5 on the same frame, and the frames differ"""
    frames = {}
    for material in ("even", "odd"):
        scene = dark_side_scene(material)
        params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=7)
        params.rng = abi.RTX_RNG_COUNTER
        out = render_dark(scene, scene.frame(96, 54), params)
        frames[material] = (check_same(out)[0], out[(None, 1, 0)][0])
    print("dark rays: shininess 2", frames["even"][0], "shininess 5", frames["odd"][0])
    assert 0 < frames["even"][0] < frames["odd"][0]
    assert not np.array_equal(frames["even"][1], frames["odd"][1])


@pytest.mark.gpu
def test_gpu_dark_is_off_for_a_transmittance_above_one():
    """kt > 1 could let a product grow: the scene's flag is off, nothing is dark, and the frames
    are those of option 0"""
    scene = dark_side_scene("pane", kt=(0.6, 1.5, 0.7))
    params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=7)
    params.rng = abi.RTX_RNG_COUNTER
    out = render_dark(scene, scene.frame(96, 54), params)
    assert check_same(out) == (0, 0)
    assert out[(None, 1, 1)][2].shadow_wave_walks == out[(None, 0, 1)][2].shadow_wave_walks


@pytest.mark.gpu
def test_gpu_dark_leaves_the_lane_slot_path_alone(tmp_path):
    """three emitters of 16 lights: 48 samples per point, so the points share packets (the
    lane-slot kernels, which do not evaluate the predicate): same frames, nothing counted"""
    from test_gpu_cull import three_emitter_scene
    scene = three_emitter_scene(tmp_path)
    with open(tmp_path / "three.json") as fh:
        d = json.load(fh)
    for o in d["Objects"]:
        if "lights" in o["parameters"]:
            o["parameters"]["lights"] = 16
    scene = rtxpy.Scene.parse(json.dumps(d), name="three16", base_dir=str(tmp_path))
    frame = scene.frame(160, 90)
    params = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=3)
    params.rng = abi.RTX_RNG_COUNTER
    assert check_same(render_dark(scene, frame, params)) == (0, 0)
