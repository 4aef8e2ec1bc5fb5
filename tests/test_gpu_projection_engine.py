"""`engine --projection` (host/main.c) on the GPU: the raw TIFF's rgb and z are Renderer.render_projection's bit for
bit, with --denoise the rgb is Renderer.denoise of that render and the ray features of the projection's rays as
rtx_projection_ray defines them, and the combinations the flag refuses exit with their message."""
import math
import os
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

FLAGS = ["-g", "path", "-n", "2"]
W, H = 64, 32
CASES = {"panorama": (["panorama"], dict(kind="panorama")),
         "fisheye": (["fisheye", "180"], dict(kind="fisheye", fov=float(np.float32(180.0 * (math.pi / 180.0)))))}


def engine(out, extra, ok=True):
    cmd = [rtxpy.ENGINE, os.path.join("scenes", "scene1.json"), out, str(W), str(H)] + FLAGS + ["-f"] + extra
    p = subprocess.run(cmd, cwd=C.GOLDEN, capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def library():
    """the Python pipeline per case: (rgb, z) of render_projection, and its denoised rgb"""
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    r = rtxpy.Renderer(0)
    out = {}
    try:
        r.upload(scene)
        frame = scene.frame(W, H)
        for name, (_, fields) in CASES.items():
            proj = rtxpy.projection(**fields)
            rgb, z = r.render_projection(frame, proj, rtxpy.params_from_args(FLAGS))
            rays = np.zeros((H, W), abi.RAY_DTYPE)
            for py in range(H):
                for px in range(W):
                    rays[py, px] = rtxpy.projection_ray(frame, proj, px, py)
            out[name] = (rgb, z, r.denoise(rgb, r.ray_features(rays)))
    finally:
        r.close()
        scene.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_projection_equals_the_library(tmp_path, library, name):
    plain, den = str(tmp_path / "plain.tif"), str(tmp_path / "den.tif")
    args = ["--projection"] + CASES[name][0]
    assert "Denoising" not in engine(plain, args)
    assert "Denoising" in engine(den, args + ["--denoise"])
    rgb0, z0 = rtxpy.read_tiff_raw(plain)
    rgb1, z1 = rtxpy.read_tiff_raw(den)
    rgb, z, want = library[name]
    u = np.uint32
    assert np.array_equal(rgb0.view(u), rgb.view(u)) and np.array_equal(z0.view(u), z.view(u))
    assert np.array_equal(z1.view(u), z.view(u)) and np.array_equal(rgb1.view(u), want.view(u))
    assert np.any(z != 0) and not np.array_equal(rgb1.view(u), rgb0.view(u))


def test_the_projections_differ_from_the_pinhole_and_from_each_other(tmp_path, library):
    out = str(tmp_path / "pinhole.tif")
    engine(out, [])
    z = rtxpy.read_tiff_raw(out)[1]
    assert not np.array_equal(z, library["panorama"][1]) and not np.array_equal(z, library["fisheye"][1])
    assert not np.array_equal(library["panorama"][1], library["fisheye"][1])


@pytest.mark.parametrize("flags,word", [(["--projection", "panorama", "--gpus", "2"], "one GPU"),
                                        (["--projection", "panorama", "--passes", "4"], "--passes"),
                                        (["--projection", "panorama", "--adaptive", "--target-error", "0.1"], "--passes"),
                                        (["--projection", "fisheye", "180", "--filter", "tent"], "--passes"),
                                        (["--projection", "fisheye", "180", "--upsample", "2"], "--upsample"),
                                        (["--projection", "cylinder"], "panorama, fisheye DEGREES or ortho EXTENT")])
def test_engine_refuses_what_a_projection_does_not_combine_with(tmp_path, flags, word):
    out = tmp_path / "o.tif"
    log = engine(str(out), flags, ok=False)
    assert word in log and "Commencing" not in log and not out.exists()
