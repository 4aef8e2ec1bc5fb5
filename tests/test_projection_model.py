"""rtx_projection_ray, the host definition of the panoramic, fisheye and orthographic cameras (include/rtx.h), against
tests/projection_model.py, a float64 model written from the header's formulas.  Both compute in double, so a
component can differ only where the two doubles straddle a float32 rounding boundary: every component within one
float32 ulp of the model's value rounded to float32, the holes identical.  No device needed."""
import math
import os

import numpy as np
import pytest

import conftest as C
import projection_model as model
import rtxpy
from rtxpy import abi

SHAPES = [(16, 8), (7, 5), (1, 1)]
FOVS = [2.0 * math.pi, math.pi, 1.0]
OFFSETS = [(0.0, 0.0), (0.25, -0.4)]
KINDS = ["panorama", "fisheye", "ortho"]


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def frames(w, h):
    """scene1's frame, and the frame of its camera moved and rotated about a skew axis"""
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    try:
        cam = scene.camera(move=(3.5, -1.25, 0.75))
        R = rotation((0.3, 1.0, -0.2), 0.9)
        for i in range(3):
            v = R @ np.array(cam.vectors[i][:], np.float64)
            for k in range(3):
                cam.vectors[i][k] = v[k]
        return [scene.frame(w, h), scene.frame(w, h, cam)]
    finally:
        scene.close()


def host_rays(frame, proj):
    out = np.zeros((frame.height, frame.width), abi.RAY_DTYPE)
    for py in range(frame.height):
        for px in range(frame.width):
            out[py, px] = rtxpy.projection_ray(frame, proj, px, py)
    return out


def settings(kind):
    """every fov for the angular kinds; for ortho the frame's own width and a given extent"""
    for off in OFFSETS:
        if kind == "ortho":
            for extent in (0.0, 3.0):
                yield dict(extent=extent, offset_x=off[0], offset_y=off[1])
        else:
            for fov in FOVS:
                yield dict(fov=fov, offset_x=off[0], offset_y=off[1])


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_definition_agrees_with_the_float64_model(kind, w, h):
    differ = total = 0
    for frame in frames(w, h):
        for fields in settings(kind):
            proj = rtxpy.projection(kind, **fields)
            rec = host_rays(frame, proj)
            d, t = model.compare(rec, frame, proj)
            differ, total = differ + d, total + t
            live = rec["tmax"] > 0
            if live.any():  # every direction is a unit vector to float rounding
                n = np.linalg.norm(rec["dir"][live].astype(np.float64), axis=-1)
                assert np.all(np.abs(n - 1.0) <= 2e-7), float(np.abs(n - 1.0).max())
    # a mismatch needs a double within a few double ulps of a float32 rounding boundary: about 1e-8 per component
    assert differ * 1000 <= total, (differ, total)


def test_holes_appear_where_the_formulas_put_them():
    """a fisheye of fov 2 pi is a disc of radius 1 in x, y: the corners of a square image are holes; a panorama
    taller than 2:1 at fov 2 pi has hole rows above and below the sphere"""
    frame = frames(16, 16)[0]
    fish = host_rays(frame, rtxpy.projection("fisheye", fov=2 * math.pi))
    assert fish["tmax"][0, 0] == 0 and fish["tmax"][15, 15] == 0 and np.isinf(fish["tmax"][8, 8])
    pano = host_rays(frame, rtxpy.projection("panorama"))
    assert np.all(pano["tmax"][:4] == 0) and np.all(pano["tmax"][12:] == 0) and np.all(np.isinf(pano["tmax"][4:12]))
    assert not np.any(fish["dir"][0, 0]) and not np.any(fish["origin"][0, 0])


def test_panorama_centre_pair_straddles_the_view_direction():
    for frame in frames(16, 8):
        r, dn, f, o = model.basis(frame)
        rec = host_rays(frame, rtxpy.projection("panorama"))
        left, right = rec["dir"][4, 7].astype(np.float64), rec["dir"][3, 8].astype(np.float64)
        # columns 7 and 8 lie half a pixel either side of lambda = 0, rows 3 and 4 either side of phi = 0
        assert left @ r < 0 < right @ r and left @ dn > 0 > right @ dn
        mid = rec["dir"][3:5, 7:9].astype(np.float64).reshape(4, 3).mean(axis=0)
        assert np.allclose(mid / np.linalg.norm(mid), f, atol=1e-6)
        assert np.array_equal(rec["origin"].reshape(-1, 3), np.tile(np.array(frame.origin[:], np.float32), (16 * 8, 1)))


def test_fisheye_centre_ray_is_the_view_direction():
    for frame in frames(7, 5):
        f = model.basis(frame)[2]
        for fov in FOVS:
            rec = host_rays(frame, rtxpy.projection("fisheye", fov=fov))
            assert np.array_equal(rec["dir"][2, 3], f.astype(np.float32))


def test_ortho_rays_are_parallel_and_evenly_spaced():
    for frame in frames(16, 8):
        r, dn, f, o = model.basis(frame)
        for extent in (0.0, 3.0):
            rec = host_rays(frame, rtxpy.projection("ortho", extent=extent))
            d = rec["dir"].reshape(-1, 3)
            assert np.all(d.view(np.uint32) == d[0].view(np.uint32))
            E = extent or 16 * np.linalg.norm(np.array(frame.step_x[:], np.float64))
            step = np.diff(rec["origin"].astype(np.float64), axis=1)
            scale = np.abs(rec["origin"]).max()
            assert np.allclose(step @ r, E / 16, atol=4 * np.spacing(np.float32(scale)))
            assert np.allclose(step @ dn, 0, atol=4 * np.spacing(np.float32(scale)))
            down = np.diff(rec["origin"].astype(np.float64), axis=0)
            assert np.allclose(down @ dn, E / 16, atol=4 * np.spacing(np.float32(scale)))
