"""k_shadow's shininess-0 forms (rtx.h RTX_OPT_SHADOW_SPEC, rtx_shadow.hip shade_terms_s0 /
dark_terms_s0): powf(x, 0) is 1 for every x, so a wave-uniform shade point whose material has
shininess 0 takes its samples' specular term as ks li without evaluating the specular factor.

 1. the forms themselves (RTX_KAT_SPEC0) against shade_terms / dark_terms with shin = +-0
    (RTX_KAT_DARK), the output words compared as integers: seeded records and the edges (a
    negative, zero, NaN and infinite specular multiplier, an infinite or NaN emitter channel, an
    infinite attenuation factor, ks of +-0 and denormals, kd = 0, pd = 0);
 2. the frames, the ray counts and every counter are the same with the option on and off: plane
    materials with and without ks and shininess, Phong and Blinn, the three attenuations, emitters
    of 64, 65 and 300 lights in 64-lane packets (the wave-uniform path) and of 8 and 65 lights in
    lane slots, the other k_shadow options on and off, both walks, a two-chunk render and a
    loopback group of 2.
"""
import ctypes
import json

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

f32 = np.float32


# ---- the KAT ----
def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def spec_records(seed, n):
    """KAT_DARK / KAT_SPEC0 records (n3 view3 kd3 ks3 shin ldir3 ldist li3 att att_offset refl kt3) with
    shin = +-0, half of them with the light behind the surface"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 26), f32)
    nrm = unit(rng.normal(size=(n, 3)))
    ldir = unit(rng.normal(size=(n, 3)))
    a = (ldir * nrm).sum(1)
    behind = rng.random(n) < 0.5
    ldir = np.where(((a > 0) & behind)[:, None], ldir - 2 * a[:, None] * nrm, ldir)
    x[:, 0:3] = nrm
    x[:, 3:6] = unit(rng.normal(size=(n, 3)))
    x[:, 6:9] = np.where((rng.random(n) < 0.2)[:, None], 0.0, rng.uniform(0.05, 1.0, (n, 3)))  # kd
    x[:, 9:12] = np.where((rng.random(n) < 0.4)[:, None], 0.0, rng.uniform(0.05, 1.0, (n, 3)))  # ks
    x[:, 12] = rng.choice(np.array([0.0, -0.0], f32), n)
    x[:, 13:16] = ldir
    x[:, 16] = rng.uniform(0.5, 20.0, n)
    x[:, 17:20] = rng.uniform(0.01, 3.0, (n, 3))  # li
    x[:, 20] = rng.integers(0, 3, n)  # RTX_ATT_NONE / LIN / SQR
    x[:, 21] = rng.choice(np.array([1.0, 0.0], f32), n, p=[0.8, 0.2])
    x[:, 22] = rng.integers(0, 2, n)  # RTX_PHONG / RTX_BLINN
    x[:, 23:26] = rng.choice(np.array([0.0, 0.32, 0.95, 1.0], f32), (n, 3))
    return x


def spec_edges():
    """the edges, each under Phong and Blinn and the three attenuations, shin +0 and -0.  The normal is
    the z axis, so a = ldir.n is ldir's z; Phong's specular multiplier for the view direction v is
    -((2 a n - ldir) . v)."""
    base = np.zeros(26, f32)
    base[0:3] = [0, 0, 1]
    base[3:6] = [0.6, 0.0, -0.8]
    base[6:9] = [0.7, 0.5, 0.3]
    base[9:12] = [0.3, 0.2, 0.4]
    base[13:16] = [0.6, 0.0, 0.8]
    base[16] = 4.0
    base[17:20] = [1.5, 0.7, 2.0]
    base[21] = 1.0
    base[23:26] = [0.5, 1.0, 0.0]
    rows = {}

    def put(name, **cols):
        r = base.copy()
        for k, v in cols.items():
            lo, hi = {"n": (0, 3), "view": (3, 6), "kd": (6, 9), "ks": (9, 12), "ldir": (13, 16), "ldist": (16, 17), "li": (17, 20),
                      "off": (21, 22)}[k]
            r[lo:hi] = v
        rows[name] = r

    put("sm_negative", view=[-0.6, 0.0, 0.8])   # the view direction along the mirrored light: sm = -1
    put("sm_positive", view=[0.6, 0.0, -0.8])
    put("sm_zero", view=[0.0, 1.0, 0.0])          # across both: sm = +-0
    put("sm_nan", view=[np.nan, 0.0, 1.0])
    put("sm_inf", view=[3e38, 0.0, -3e38])        # the dot product overflows
    put("sm_neg_inf", view=[-3e38, 0.0, 3e38])
    put("li_inf", li=[np.inf, 0.7, 2.0])
    put("li_neg_inf", li=[1.5, -np.inf, 2.0])
    put("li_nan", li=[1.5, 0.7, np.nan])
    put("attf_inf", ldist=0.0, off=0.0)           # 1 / (0 + 0) under lin and sqr
    put("ks_zero", ks=[0.0, 0.0, 0.0])
    put("ks_neg_zero", ks=[-0.0, -0.0, -0.0])
    put("ks_mixed_zero", ks=[0.0, -0.0, 0.3])
    put("ks_denormal", ks=[1e-40, -1e-42, 1e-45])
    put("ks_zero_li_inf", ks=[0.0, -0.0, 0.0], li=[np.inf, 0.7, 2.0])  # 0 * inf: a NaN, never dark
    put("kd_zero", kd=[0.0, 0.0, 0.0])
    put("kd_ks_zero", kd=[0.0, 0.0, 0.0], ks=[0.0, 0.0, 0.0])
    put("pd_zero", ldir=[1.0, 0.0, 0.0])          # a light in the surface's plane: a = +0
    put("pd_neg_zero", ldir=[1.0, 0.0, -0.0])
    put("pd_behind", ldir=[0.6, 0.0, -0.8])
    put("pd_behind_ks_zero", ldir=[0.6, 0.0, -0.8], ks=[0.0, 0.0, 0.0])
    put("pd_nan", ldir=[np.nan, np.nan, np.nan], ldist=0.0)
    put("pd_zero_kd_ks_denormal", ldir=[1.0, 0.0, 0.0], kd=[1e-40, 1e-40, 1e-40], ks=[1e-40, 0.0, 0.0])
    names, out = [], []
    for name, r in rows.items():
        for refl in (abi.RTX_PHONG, abi.RTX_BLINN):
            for att in (abi.RTX_ATT_NONE, abi.RTX_ATT_LIN, abi.RTX_ATT_SQR):
                for shin in (0.0, -0.0):
                    q = r.copy()
                    q[12], q[20], q[22] = shin, att, refl
                    names.append((name, refl, att, shin))
                    out.append(q)
    return names, np.array(out, f32)


@pytest.mark.gpu
def test_gpu_spec0_forms_match_the_generic_ones_bit_for_bit():
    names, edges = spec_edges()
    x = np.concatenate([edges, spec_records(73, 4000)])
    want = rtxpy.gpu_kat(abi.KAT_DARK, x).view(np.uint32)
    got = rtxpy.gpu_kat(abi.KAT_SPEC0, x).view(np.uint32)
    bad = np.flatnonzero((want != got).any(1))
    print("records", len(x), "edges", len(edges), "dark", int((want[:, 0] != 0).sum()), "NaN terms", int(np.isnan(want.view(f32)[:, 1:]).any(1).sum()),
          "differing", len(bad), [names[i] if i < len(names) else int(i) for i in bad[:8]])
    assert len(bad) == 0
    # not vacuous: dark and lit records, NaN and infinite terms, and terms that hold ks li
    y = want.view(f32)
    dark = y[:, 0] > 0
    assert 200 <= dark.sum() <= len(x) - 2000
    assert np.isnan(y[:, 1:4]).any(1).sum() >= 20 and np.isinf(y[:, 1:4]).any(1).sum() >= 6
    behind = ((x[:, 13:16] * x[:, 0:3]).sum(1) < -1e-3) & np.isfinite(x).all(1) & (x[:, 9:12] > 0.01).all(1) & (x[:, 20] == abi.RTX_ATT_NONE)
    assert behind.sum() >= 300 and (y[behind, 1:4] == x[behind, 9:12] * x[behind, 17:20]).all()  # pd = 0: the term is ks li


# ---- frames ----
PLANE_MATERIALS = [(0.0, 0.0), (0.3, 0.0), (0.0, 5.0), (0.3, 5.0), (-0.0, 0.0)]
VARIANTS = tuple((refl, att) for refl in (abi.RTX_PHONG, abi.RTX_BLINN) for att in (abi.RTX_ATT_NONE, abi.RTX_ATT_LIN, abi.RTX_ATT_SQR))
# what depends on which samples share a wave.  On the lane-slot launches (fewer than 64 lanes a slot) two identical
# renders do not repeat them (65 lights at the automatic 4-lane slots, option off both times: wave steps 116111 and
# 116084, walks 11333 and 11332), so there they are left out; wave-uniform launches repeat them exactly
PACKING = ("shadow_wave_steps", "shadow_leaf_rounds", "shadow_uniform_steps", "shadow_wave_walks")
SLOT64 = ((abi.RTX_OPT_SHADOW_SLOT, 64),)  # one point per 64-lane packet whatever the light count (the automatic choice for 64 and 300)
COUNTERS = [f for f, t in abi.Stats._fields_ if t in (ctypes.c_uint64, ctypes.c_uint32) and not f.startswith("pad")] + \
    [f for s in (abi.PointStats, abi.DarkStats, abi.PremaskStats, abi.OrderStats) for f, _ in s._fields_]


def spec_scene(ks, shin, lights, opaque):
    """a floor and a back wall of one material (ks, shin), a small mesh standing on the floor, transparent
    or opaque, and one sphere emitter of `lights` lights up on the left: the mesh's shadow lies on the
    floor and climbs the wall, so points near it walk the tree and the rest of the planes are clear"""
    mat = {"ka": [0.5, 0.5, 0.5], "kr": [0.0, 0.0, 0.0], "kt": [0.0, 0.0, 0.0], "ke": [0.0, 0.0, 0.0], "refractive_index": 1.0}
    d = {"AmbientLight": [0.1, 0.1, 0.1],
         "Camera": {"position": [0.0, -3.5, 1.0], "vector_x": [1.0, 0.0, 0.0], "vector_y": [0.0, -0.15, -1.0], "fov": 80, "focal_length": 1.0},
         "Materials": [
             dict(mat, id=0, ks=[ks, ks, ks], shininess=shin, texture={"type": "uniform", "color": [0.7, 0.7, 0.7]}),
             dict(mat, id=1, ks=[0.4, 0.4, 0.4], shininess=5.0, kt=[0.0, 0.0, 0.0] if opaque else [0.6, 0.8, 0.7],
                  texture={"type": "uniform", "color": [0.8, 0.3, 0.2]}),
             dict(mat, id=2, ks=[0.0, 0.0, 0.0], ka=[0.0, 0.0, 0.0], ke=[1.0, 1.0, 1.0], shininess=0.0,
                  texture={"type": "uniform", "color": [0.0, 0.0, 0.0]})],
         "Objects": [
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 0.0, -1.0], "normal": [0.0, 0.0, 1.0]}},
             {"type": "Plane", "parameters": {"material": 0, "epsilon": 0.00025, "position": [0.0, 5.0, 0.0], "normal": [0.0, -1.0, 0.0]}},
             {"type": "Mesh", "parameters": {"material": 1, "filename": "meshes/utah_teapot_lowpoly.stl", "position": [0.8, 2.5, -1.0],
                                             "rotation": [0.0, 0.0, 0.0], "scale": 0.04}},
             {"type": "Sphere", "parameters": {"material": 2, "epsilon": 0.0003, "position": [-5.0, 0.0, 2.5], "radius": 0.4, "lights": lights}}]}
    return rtxpy.Scene.parse(json.dumps(d), name="spec", base_dir=C.GOLDEN)


def bench_like_params():
    p = rtxpy.params_from_args(["-g", "path", "-n", "2"], seed=5)
    p.rng = abi.RTX_RNG_COUNTER
    return p


def copy_params(p, **over):
    q = rtxpy.default_params(**{f: getattr(p, f) for f, _ in abi.Params._fields_})
    for k, v in over.items():
        setattr(q, k, v)
    return q


def renders(r, frame, params, variants=(None,)):
    """{(variant, spec, count): (rgb bytes, z bytes, stats)} from an uploaded renderer or group"""
    out = {}
    for v in variants:
        for spec in (0, 1):
            r.set_option(abi.RTX_OPT_SHADOW_SPEC, spec)
            for count in (0, 1):
                p = copy_params(params, count_traversal=count)
                if v is not None:
                    p.reflection, p.attenuation = v
                rgb, z = r.render(frame, p)
                out[(v, spec, count)] = (rgb.tobytes(), z.tobytes(), r.stats())
    return out


def check_equal(out, lane_slots=False):
    """option on against off, no tolerance: the images' bytes among all four renders of a variant, the
    ray counts too, and every counter between the two counting renders (lane_slots: but PACKING).
    Returns a counting render's stats with the option on."""
    last = None
    for (v, spec, count), (rgb, z, s) in out.items():
        rgb0, z0, s0 = out[(v, 0, 0)]
        assert rgb == rgb0 and z == z0, (v, spec, count)
        assert (s.closest_rays, s.shadow_rays, s.shade_points) == (s0.closest_rays, s0.shadow_rays, s0.shade_points), (v, spec, count)
        if spec and count:
            off = out[(v, 0, 1)][2]
            diff = [(f, getattr(s, f), getattr(off, f)) for f in COUNTERS
                    if getattr(s, f) != getattr(off, f) and not (lane_slots and f in PACKING)]
            assert not diff, (v, diff)
            last = s
    return last


def open_renderer(scene, walk=abi.RTX_WALK_AUTO, options=()):
    r = rtxpy.Renderer(0)
    try:
        r.set_option(abi.RTX_OPT_SHADOW_WALK, walk)
        r.upload(scene)
        for o, v in options:
            r.set_option(o, v)
    except Exception:
        r.close()
        raise
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("opaque", [False, True], ids=["transparent", "opaque"])
@pytest.mark.parametrize("ks,shin", PLANE_MATERIALS)
def test_gpu_spec_is_invisible_under_every_shading_model(ks, shin, opaque):
    """the five plane materials, Phong and Blinn, the three attenuations; 65 lights in 64-lane packets: a
    whole packet and a packet of one sample.  The 8-wide walk, the bench frame's: only there (or without a
    tree) is a point ever all-clear, so only there does clear_run run"""
    scene = spec_scene(ks, shin, 65, opaque)
    r = open_renderer(scene, abi.RTX_WALK_W8, SLOT64)
    try:
        s = check_equal(renders(r, scene.frame(96, 54), bench_like_params(), VARIANTS))
    finally:
        r.close()
    print("ks", ks, "shin", shin, "opaque", opaque, "rays", s.shadow_rays, "point-clear", s.shadow_point_clear, "walks", s.shadow_wave_walks,
          "dark", s.shadow_dark_rays)
    # some of the planes' points are all-clear ones (clear_run), and some walk
    assert s.shadow_point_clear > 0 and s.shadow_wave_walks > 0


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [abi.RTX_WALK_AUTO, abi.RTX_WALK_W8], ids=["auto", "w8"])
@pytest.mark.parametrize("lights,slot", [(64, 64), (65, 64), (300, 64), (8, 0), (65, 0)])
def test_gpu_spec_is_invisible_at_every_packet_shape(lights, slot, walk):
    """64, 65 and 300 lights in 64-lane packets: the wave-uniform path (300: ordered runs too); 8 lights,
    and 65 at the automatic slot size (4 lanes, points straddling packets): lane slots, whose points keep the
    generic forms"""
    for ks in (0.0, 0.3):
        scene = spec_scene(ks, 0.0, lights, True)
        r = open_renderer(scene, walk, ((abi.RTX_OPT_SHADOW_SLOT, slot),))
        try:
            s = check_equal(renders(r, scene.frame(96, 54), bench_like_params(), (None, (abi.RTX_BLINN, abi.RTX_ATT_SQR))), lane_slots=not slot)
        finally:
            r.close()
        print("lights", lights, "walk", abi.WALK_NAMES[s.shadow_walk], "ks", ks, "point-clear", s.shadow_point_clear, "ordered points",
              s.shadow_ordered_points, "dark", s.shadow_dark_rays, "walks", s.shadow_wave_walks)
        assert s.shadow_wave_walks > 0
        if slot:
            assert (s.shadow_point_clear > 0) == (walk == abi.RTX_WALK_W8)  # the threaded walk has no cone masks: no all-clear point
        else:
            assert s.shadow_point_clear == 0 and s.shadow_ordered_points == 0
        if lights == 300:
            assert s.shadow_ordered_points > 0


@pytest.mark.gpu
@pytest.mark.parametrize("walk", [abi.RTX_WALK_AUTO, abi.RTX_WALK_W8], ids=["auto", "w8"])
@pytest.mark.parametrize("dark", [1, 0])
@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("point", [1, 0])
def test_gpu_spec_is_invisible_beside_the_other_options(point, order, dark, walk):
    """RTX_OPT_SHADOW_POINT, RTX_OPT_SHADOW_ORDER and RTX_OPT_SHADOW_DARK on and off: every k_shadow instance
    and each of the three call sites with and without its neighbours"""
    for ks, opaque in ((0.0, False), (0.3, True)):
        scene = spec_scene(ks, 0.0, 300, opaque)
        r = open_renderer(scene, walk, ((abi.RTX_OPT_SHADOW_POINT, point), (abi.RTX_OPT_SHADOW_ORDER, order), (abi.RTX_OPT_SHADOW_DARK, dark)))
        try:
            s = check_equal(renders(r, scene.frame(96, 54), bench_like_params()))
        finally:
            r.close()
        print("point", point, "order", order, "dark", dark, "walk", abi.WALK_NAMES[s.shadow_walk], "ks", ks, "point-clear", s.shadow_point_clear,
              "ordered points", s.shadow_ordered_points, "dark rays", s.shadow_dark_rays, "walks", s.shadow_wave_walks)
        assert s.shadow_wave_walks > 0
        assert (s.shadow_point_clear > 0) == (bool(point) and walk == abi.RTX_WALK_W8)
        assert s.shadow_ordered_points == 0 or order
        assert s.shadow_dark_rays == 0 or dark
        if point and order and dark:
            assert s.shadow_ordered_points > 0


@pytest.mark.gpu
def test_gpu_spec_is_invisible_in_a_two_chunk_render():
    scene = spec_scene(0.3, 0.0, 65, False)
    frame = scene.frame(96, 54)
    tiles = ((96 + 7) // 8) * ((54 + 7) // 8)
    r = open_renderer(scene, abi.RTX_WALK_W8, SLOT64 + ((abi.RTX_OPT_CHUNK_TILES, (tiles + 1) // 2),))
    try:
        out = renders(r, frame, bench_like_params())
        s = check_equal(out)
        assert s.chunks == 2
        r.set_option(abi.RTX_OPT_CHUNK_TILES, 0)
        whole = renders(r, frame, bench_like_params())
    finally:
        r.close()
    assert check_equal(whole).chunks == 1
    assert whole[(None, 1, 0)][:2] == out[(None, 1, 0)][:2]


@pytest.mark.gpu
def test_gpu_spec_is_invisible_on_a_loopback_group_of_two():
    scene = spec_scene(0.0, 0.0, 65, False)
    frame = scene.frame(96, 54)
    g = rtxpy.Group([0], loopback=2)
    try:
        g.set_option(abi.RTX_OPT_SHADOW_WALK, abi.RTX_WALK_W8)
        g.upload(scene)
        g.set_option(*SLOT64[0])
        out = renders(g, frame, bench_like_params())
    finally:
        g.close()
    s = check_equal(out)
    assert s.devices == 2 and s.shadow_point_clear > 0
    r = open_renderer(scene, abi.RTX_WALK_W8, SLOT64)
    try:
        one = renders(r, frame, bench_like_params())
    finally:
        r.close()
    assert one[(None, 1, 0)][:2] == out[(None, 1, 0)][:2]
