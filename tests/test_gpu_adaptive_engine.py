"""`engine --adaptive --target-error E` (host/main.c) on the GPU: the saved raster and z tag are
Renderer.render_adaptive of the same frame bit for bit, --denoise filters the mean with the original frame's
features, and without the flag the output is the plain render."""
import os
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy

pytestmark = pytest.mark.gpu

FLAGS = ["-g", "path", "-n", "1", "--seed", "11"]
TARGET = "0.01"  # about the error 8 jittered passes of this frame reach (0.0096): some tiles meet it at once, edges do not


def engine(out, extra):
    cmd = [rtxpy.ENGINE, os.path.join("scenes", "scene1.json"), out, "64", "64"] + FLAGS + ["-f"] + extra
    p = subprocess.run(cmd, cwd=C.GOLDEN, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    r = rtxpy.Renderer(0)
    r.upload(scene)
    yield r, scene, scene.frame(64, 64), rtxpy.params_from_args(FLAGS[:4], seed=11)
    r.close()
    scene.close()


def test_engine_adaptive_equals_the_library(lib, tmp_path):
    r, scene, frame, params = lib
    cases = {
        "aa": (["--adaptive", "--target-error", TARGET, "--aa"], dict(passes=16, jitter=True)),
        "aa24": (["--adaptive", "--target-error", TARGET, "--aa", "--passes", "24"], dict(passes=24, jitter=True)),
        "plain": (["--target-error", TARGET, "--adaptive"], dict(passes=16)),
    }
    for name, (flags, kw) in cases.items():
        out = str(tmp_path / (name + ".tif"))
        log = engine(out, flags)
        rgb, z, _, n_t = r.render_adaptive(frame, params, target_error=float(np.float32(float(TARGET))), **kw)
        st = r.adaptive_stats()
        assert f"Adaptive passes: {st.passes_run} of {kw['passes']} run, {st.tile_passes} of {st.passes_run * 64} tile passes" in log, log
        assert "Passes:" not in log
        got_rgb, got_z = rtxpy.read_tiff_raw(out)
        assert np.array_equal(bits(got_rgb), bits(rgb)), name
        assert np.array_equal(bits(got_z), bits(z)), name
        if "jitter" in kw:
            assert n_t.min() < n_t.max()  # the frame's tiles meet the target at different passes


def test_engine_adaptive_composes_with_denoise_and_leaves_the_plain_render_alone(lib, tmp_path):
    r, scene, frame, params = lib
    plain, den = str(tmp_path / "plain.tif"), str(tmp_path / "den.tif")
    assert "Adaptive" not in engine(plain, [])
    log = engine(den, ["--adaptive", "--target-error", TARGET, "--aa", "--denoise"])
    assert "Adaptive passes:" in log and "Denoising" in log
    rgb0, z0 = r.render(frame, params)
    got_rgb, got_z = rtxpy.read_tiff_raw(plain)
    assert np.array_equal(bits(got_rgb), bits(rgb0)) and np.array_equal(bits(got_z), bits(z0))  # as it is today
    mean, z, _, _ = r.render_adaptive(frame, params, 16, float(np.float32(float(TARGET))), jitter=True)
    want = r.denoise(mean, r.features(frame))
    got_rgb, got_z = rtxpy.read_tiff_raw(den)
    assert np.array_equal(bits(got_z), bits(z)) and np.array_equal(bits(got_z), bits(z0))
    assert np.array_equal(bits(got_rgb), bits(want))
    assert not np.array_equal(bits(got_rgb), bits(mean))
