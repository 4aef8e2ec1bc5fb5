"""`engine --filter NAME [--filter-radius R] [--filter-alpha A]` (host/main.c) on the GPU: the saved raster and z tag
are Renderer.render_passes_filtered of the same frame bit for bit, --denoise-variance filters the filtered mean with
its variance, and without the flag the output is what it was."""
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


def test_engine_filter_equals_the_library(lib, tmp_path):
    r, scene, frame, params = lib
    focus = float(np.float32(4.0 / float(scene.desc.camera.focal_length)))
    cases = {
        "gaussian": (["--filter", "gaussian"], dict(passes=16)),
        "mitchell4": (["--filter", "mitchell", "--filter-radius", "2", "--passes", "4"], dict(passes=4, filter="mitchell", radius=2.0)),
        "wide": (["--filter", "gaussian", "--filter-radius", "2.5", "--filter-alpha", "0.5", "--passes", "3"],
                 dict(passes=3, radius=2.5, alpha=0.5)),
        "tent lens": (["--filter", "tent", "--lens", "0.2", "4"], dict(passes=16, filter="tent", aperture=0.2, focus=focus)),
        "box target": (["--filter", "box", "--passes", "8", "--target-error", "1e30"],
                       dict(passes=8, filter="box", target_error=1e30)),
    }
    for name, (flags, kw) in cases.items():
        out = str(tmp_path / (name.replace(" ", "_") + ".tif"))
        log = engine(out, flags)
        rgb, z, _ = r.render_passes_filtered(frame, params, jitter=True, **kw)
        st = r.pass_stats()
        assert f"Passes: {st.passes_run} of {kw['passes']} run" in log, log
        got_rgb, got_z = rtxpy.read_tiff_raw(out)
        assert np.array_equal(bits(got_rgb), bits(rgb)), name
        assert np.array_equal(bits(got_z), bits(z)), name
    assert r.pass_stats().passes_run == 2  # the target above stops at the least number of passes


def test_engine_filter_composes_with_denoise_variance_and_leaves_the_other_outputs_alone(lib, tmp_path):
    r, scene, frame, params = lib
    plain, aa, filt, den = (str(tmp_path / n) for n in ("plain.tif", "aa.tif", "filt.tif", "den.tif"))
    assert "Passes:" not in engine(plain, [])
    engine(aa, ["--aa", "--passes", "4"])
    assert "Denoising" not in engine(filt, ["--filter", "mitchell", "--passes", "4"])
    log = engine(den, ["--filter", "mitchell", "--passes", "4", "--denoise-variance"])
    assert "Passes: 4 of 4 run" in log and "Denoising with the variance." in log
    # without the flag: the plain render, and the unfiltered passes, as they were
    rgb0, z0 = r.render(frame, params)
    got_rgb, got_z = rtxpy.read_tiff_raw(plain)
    assert np.array_equal(bits(got_rgb), bits(rgb0)) and np.array_equal(bits(got_z), bits(z0))
    mean_aa, z_aa, _ = r.render_passes(frame, params, 4, jitter=True)
    got_rgb, got_z = rtxpy.read_tiff_raw(aa)
    assert np.array_equal(bits(got_rgb), bits(mean_aa)) and np.array_equal(bits(got_z), bits(z_aa))
    # with it: the filtered mean, then that mean filtered with its variance
    mean, z, var = r.render_passes_filtered(frame, params, 4, filter="mitchell", radius=1.5)
    got_rgb, got_z = rtxpy.read_tiff_raw(filt)
    assert np.array_equal(bits(got_rgb), bits(mean)) and np.array_equal(bits(got_z), bits(z))
    assert not np.array_equal(bits(mean), bits(mean_aa))
    want, _ = r.denoise_variance(mean, var, r.features(frame))
    got_rgb, got_z = rtxpy.read_tiff_raw(den)
    assert np.array_equal(bits(got_z), bits(z))
    assert np.array_equal(bits(got_rgb), bits(want))
    assert not np.array_equal(bits(got_rgb), bits(mean))
