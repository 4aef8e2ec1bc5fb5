"""`engine --passes / --aa / --lens / --target-error` (host/main.c) on the GPU: the saved raster and z tag are
Renderer.render_passes of the same frame bit for bit, --denoise filters the mean with the original frame's
features, and without the flags the output is the plain render."""
import os
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy

pytestmark = pytest.mark.gpu

FLAGS = ["-g", "path", "-n", "1", "--seed", "11"]


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


def test_engine_passes_equal_the_library(lib, tmp_path):
    r, scene, frame, params = lib
    focus = float(np.float32(4.0 / float(scene.desc.camera.focal_length)))
    cases = {
        "aa4": (["--passes", "4", "--aa"], dict(passes=4, jitter=True)),
        "aa": (["--aa"], dict(passes=16, jitter=True)),
        "lens": (["--lens", "0.2", "4"], dict(passes=16, aperture=0.2, focus=focus)),
        "target": (["--passes", "8", "--target-error", "1e30"], dict(passes=8, target_error=1e30)),
    }
    for name, (flags, kw) in cases.items():
        out = str(tmp_path / (name + ".tif"))
        log = engine(out, flags)
        rgb, z, _ = r.render_passes(frame, params, **kw)
        st = r.pass_stats()
        assert f"Passes: {st.passes_run} of {kw['passes']} run" in log, log
        got_rgb, got_z = rtxpy.read_tiff_raw(out)
        assert np.array_equal(bits(got_rgb), bits(rgb)), name
        assert np.array_equal(bits(got_z), bits(z)), name
    assert r.pass_stats().passes_run == 2  # the target above stops at the least number of passes


def test_engine_passes_compose_with_denoise_and_leave_the_plain_render_alone(lib, tmp_path):
    r, scene, frame, params = lib
    plain, den = str(tmp_path / "plain.tif"), str(tmp_path / "den.tif")
    assert "Passes:" not in engine(plain, [])
    log = engine(den, ["--passes", "4", "--denoise"])
    assert "Passes: 4 of 4 run" in log and "Denoising" in log
    rgb0, z0 = r.render(frame, params)
    got_rgb, got_z = rtxpy.read_tiff_raw(plain)
    assert np.array_equal(bits(got_rgb), bits(rgb0)) and np.array_equal(bits(got_z), bits(z0))  # as it is today
    mean, z, _ = r.render_passes(frame, params, 4)
    want = r.denoise(mean, r.features(frame))
    got_rgb, got_z = rtxpy.read_tiff_raw(den)
    assert np.array_equal(bits(got_z), bits(z)) and np.array_equal(bits(got_z), bits(z0))
    assert np.array_equal(bits(got_rgb), bits(want))
    assert not np.array_equal(bits(got_rgb), bits(mean))
