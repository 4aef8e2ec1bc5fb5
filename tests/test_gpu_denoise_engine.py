"""`engine --denoise` (host/main.c) on the GPU: the saved rgb is Renderer.denoise of the render and its
features bit for bit, z is the render's, and without the flag the output is the plain render."""
import os
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy

pytestmark = pytest.mark.gpu

FLAGS = ["-g", "path", "-n", "4"]


def engine(out, extra):
    cmd = [rtxpy.ENGINE, os.path.join("scenes", "scene1.json"), out, "64", "64"] + FLAGS + ["-f"] + extra
    p = subprocess.run(cmd, cwd=C.GOLDEN, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_engine_denoise_equals_the_library(tmp_path):
    plain, den = str(tmp_path / "plain.tif"), str(tmp_path / "den.tif")
    assert "Denoising" not in engine(plain, [])
    log = engine(den, ["--denoise"])
    assert "Denoising" in log and "filter levels" in log
    rgb0, z0 = rtxpy.read_tiff_raw(plain)
    rgb1, z1 = rtxpy.read_tiff_raw(den)
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    r = rtxpy.Renderer(0)
    try:
        r.upload(scene)
        frame = scene.frame(64, 64)
        rgb, z = r.render(frame, rtxpy.params_from_args(FLAGS))
        want = r.denoise(rgb, r.features(frame))
    finally:
        r.close()
        scene.close()
    u = np.uint32
    assert np.array_equal(rgb0.view(u), rgb.view(u)) and np.array_equal(z0.view(u), z.view(u))  # as it is today
    assert np.array_equal(z1.view(u), z.view(u))
    assert np.array_equal(rgb1.view(u), want.view(u))
    assert not np.array_equal(rgb1.view(u), rgb0.view(u))


def test_engine_help_names_the_flag():
    p = subprocess.run([rtxpy.ENGINE, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--denoise" in p.stdout
