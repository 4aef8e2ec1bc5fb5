"""`engine --upsample S [--refine T]` (host/main.c) on the GPU: the saved rgb and z are Renderer.render_upsampled's
bit for bit, --denoise filters that frame, and without the flag the output is the plain render."""
import os
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

FLAGS = ["--rng", "const"]
W, H = 64, 40
U = np.uint32


def engine(out, extra):
    cmd = [rtxpy.ENGINE, os.path.join("scenes", "scene3.json"), out, str(W), str(H)] + FLAGS + ["-f"] + extra
    p = subprocess.run(cmd, cwd=C.GOLDEN, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def library():
    """what the library gives for the engine's cases, and the plain render"""
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene3.json"), base_dir=C.GOLDEN)
    r = rtxpy.Renderer(0)
    try:
        r.upload(scene)
        frame, p = scene.frame(W, H), rtxpy.params_from_args([], rng=abi.RTX_RNG_CONST)
        out = {"plain": r.render(frame, p)}
        out["s2"] = r.render_upsampled(frame, p, scale=2)
        out["s2_tiles"] = r.upsample_stats().refined_tiles
        out["s3"] = r.render_upsampled(frame, p, scale=3, refine_threshold=0.25)
        out["s2_denoised"] = r.denoise(out["s2"][0], r.features(frame))
    finally:
        r.close()
        scene.close()
    return out


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U), np.ascontiguousarray(b).view(U))


def test_engine_upsample_equals_the_library(tmp_path, library):
    out = str(tmp_path / "up.tif")
    log = engine(out, ["--upsample", "2"])
    assert f"{library['s2_tiles']} of 40 tiles refined" in log and "Upsampled 32x20 by 2" in log
    rgb, z = rtxpy.read_tiff_raw(out)
    assert same(rgb, library["s2"][0]) and same(z, library["s2"][1])
    assert same(z, library["plain"][1]) and not same(rgb, library["plain"][0])


def test_engine_upsample_three_with_a_threshold_equals_the_library(tmp_path, library):
    out = str(tmp_path / "up3.tif")
    log = engine(out, ["--upsample", "3", "--refine", "0.25"])
    assert "Upsampled 22x14 by 3" in log and "below confidence 0.25" in log
    rgb, z = rtxpy.read_tiff_raw(out)
    assert same(rgb, library["s3"][0]) and same(z, library["s3"][1])


def test_engine_upsample_composes_with_denoise(tmp_path, library):
    out = str(tmp_path / "upd.tif")
    log = engine(out, ["--upsample", "2", "--denoise"])
    assert "Upsampled" in log and "Denoising" in log
    rgb, z = rtxpy.read_tiff_raw(out)
    assert same(rgb, library["s2_denoised"]) and same(z, library["plain"][1])
    assert not same(rgb, library["s2"][0])


def test_the_plain_output_is_unchanged(tmp_path, library):
    out = str(tmp_path / "plain.tif")
    assert "Upsampled" not in engine(out, [])
    rgb, z = rtxpy.read_tiff_raw(out)
    assert same(rgb, library["plain"][0]) and same(z, library["plain"][1])
