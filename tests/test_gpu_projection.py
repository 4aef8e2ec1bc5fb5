"""The ray generator of the camera models on the GPU (rtx_projection_rays_device, k_projection_rays) against
tests/projection_model.py, and rtx_render_projection against the two calls it chains.

The kernel evaluates the header's formulas in double and rounds once, like the model: a component may differ by one
float32 ulp where the two doubles straddle a rounding boundary (about 1e-8 per component), so at most 1 in 1000 may
differ at all, and the holes are identical.
"""
import math
import os

import numpy as np
import pytest

import conftest as C
import projection_model as model
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

SIZES = [(64, 32), (33, 17), (1, 1)]
SETTINGS = [("panorama", dict()), ("panorama", dict(fov=math.pi, offset_x=0.25, offset_y=-0.4)),
            ("panorama", dict(fov=1.0)), ("fisheye", dict()), ("fisheye", dict(fov=math.pi)),
            ("fisheye", dict(fov=1.0, offset_x=0.25, offset_y=-0.4)), ("ortho", dict()),
            ("ortho", dict(extent=7.5, offset_x=0.25, offset_y=-0.4))]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def world():
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scenetest2.json"), base_dir=C.GOLDEN)
    r = rtxpy.Renderer(0)
    r.upload(scene)
    yield r, scene
    r.close()
    scene.close()


def moved_frame(scene, w, h):
    """the scene's camera moved and turned about a skew axis"""
    cam = scene.camera(move=(0.5, 0.25, -0.5))
    a = np.array([0.3, 1.0, -0.2])
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(0.4) * K + (1 - math.cos(0.4)) * (K @ K)
    for i in range(3):
        v = R @ np.array(cam.vectors[i][:], np.float64)
        for k in range(3):
            cam.vectors[i][k] = v[k]
    return scene.frame(w, h, cam)


@pytest.mark.parametrize("w,h", SIZES)
def test_device_rays_agree_with_the_float64_model(world, w, h):
    r, scene = world
    differ = total = host_differ = 0
    for frame in (scene.frame(w, h), moved_frame(scene, w, h)):
        for kind, fields in SETTINGS:
            proj = rtxpy.projection(kind, **fields)
            rec = r.projection_rays(frame, proj)
            d, t = model.compare(rec, frame, proj)
            differ, total = differ + d, total + t
            host = np.zeros((h, w), abi.RAY_DTYPE)
            for py in range(h):
                for px in range(w):
                    host[py, px] = rtxpy.projection_ray(frame, proj, px, py)
            host_differ += model.compare(host, frame, proj)[0]
    # both caps: the device against the model, and the host definition against it for these inputs
    assert differ * 1000 <= total and host_differ * 1000 <= total, (differ, host_differ, total)


@pytest.mark.parametrize("kind,fields", [("panorama", {}), ("fisheye", {"fov": 2.0 * math.pi}), ("ortho", {"extent": 10.0})])
@pytest.mark.parametrize("w,h", [(64, 32), (33, 17)])
def test_render_projection_is_the_generator_then_the_ray_render(world, kind, fields, w, h):
    import torch
    r, scene = world
    frame, proj = scene.frame(w, h), rtxpy.projection(kind, **fields)
    p = rtxpy.params_from_args(["-g", "path", "-n", "1"], seed=9)
    a = r.render_projection(frame, proj, p)
    b = r.render_rays(r.projection_rays(frame, proj), params=p)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.any(a[1] != 0)
    rgb = torch.zeros((h * w * 3,), dtype=torch.float32, device="cuda")
    z = torch.zeros((h * w,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.render_projection_device(frame, proj, p, rgb.data_ptr(), z.data_ptr(), stream=torch.cuda.Stream().cuda_stream)
    assert np.array_equal(bits(rgb.cpu().numpy().reshape(h, w, 3)), bits(a[0]))
    assert np.array_equal(bits(z.cpu().numpy().reshape(h, w)), bits(a[1]))


def test_projection_errors_on_a_context(world):
    r, scene = world
    frame = scene.frame(16, 8)
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_projection(frame, rtxpy.projection(kind=5), rtxpy.default_params())
    assert e.value.code == abi.RTX_ERR_ARG
    with pytest.raises(rtxpy.RtxError) as e:
        r.render_projection(frame, rtxpy.projection("fisheye", fov=7.0), rtxpy.default_params())
    assert e.value.code == abi.RTX_ERR_ARG
    fresh = rtxpy.Renderer(0)
    try:
        with pytest.raises(rtxpy.RtxError) as e:
            fresh.render_projection(frame, rtxpy.projection(), rtxpy.default_params())
        assert e.value.code == abi.RTX_ERR_STATE
        assert fresh.projection_rays(frame, rtxpy.projection()).shape == (8, 16)  # the generator needs no scene
    finally:
        fresh.close()


def test_an_orthographic_view_of_a_plane_has_the_closed_form_depth(world):
    """a sanity check of the basis: looking along f at a plane of the scene, z is (d - n . o) / (n . f) for every ray
    that meets the plane first.  The float error of one plane intersection is measured against rtx_trace_rays on the
    same rays, which the render's z must match bit for bit."""
    r, scene = world
    planes = [o for o in scene.objects() if o.type == abi.RTX_PLANE]
    assert planes
    frame = scene.frame(40, 24)
    proj = rtxpy.projection("ortho", extent=2.0)
    rec = r.projection_rays(frame, proj)
    rgb, z = r.render_projection(frame, proj, rtxpy.default_params())
    flat = rec.reshape(-1)
    hits = r.trace_rays(flat["origin"], flat["dir"])
    assert np.array_equal(bits(z).reshape(-1), bits(hits["t"]))
    objs = scene.objects()
    checked = 0
    for i, o in enumerate(objs):
        if o.type != abi.RTX_PLANE:
            continue
        m = hits["object"] == i
        if not m.any():
            continue
        n, d = np.array(o.n[:], np.float64), float(o.d)
        org, dr = flat["origin"][m].astype(np.float64), flat["dir"][m].astype(np.float64)
        # the plane as the scene states it: n . P = d or n . P + d = 0; take the one the hits satisfy
        P = org + dr * hits["t"][m].astype(np.float64)[:, None]
        sign = 1.0 if np.abs(P @ n - d).max() < np.abs(P @ n + d).max() else -1.0
        want = (sign * d - org @ n) / (dr @ n)
        got = hits["t"][m].astype(np.float64)
        # float32 intersection: two 3-term dot products of terms up to `scale`, a difference and a quotient, under
        # 16 roundings of that size in the numerator, carried through the division by n . dir
        scale = np.abs(org).max() + abs(d)
        tol = 16 * np.spacing(np.float32(scale)) / np.abs(dr @ n) + 4 * np.spacing(np.abs(got).astype(np.float32))
        assert np.all(np.abs(got - want) <= tol), float(np.abs(got - want).max())
        checked += int(m.sum())
    assert checked > 0
