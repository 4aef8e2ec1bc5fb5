"""The feature-guided upsampler's C-ABI (rtx_frame_scaled, rtx_upsample*, rtx_upsample_tiles*, rtx_render_upsampled*,
include/rtx.h) on a CPU-only host: declarations, exports, the struct layouts, the defaults, null contexts, every
argument error of rtx_frame_scaled, the low frame against a float64 restatement of the header's formulas, the
numpy model's own tap rules, and the engine's flags."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy
import upsample_model as UM
from rtxpy import abi

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
INT_FUNCS = ["rtx_frame_scaled", "rtx_upsample", "rtx_upsample_device", "rtx_upsample_tiles", "rtx_upsample_tiles_device",
             "rtx_render_upsampled", "rtx_render_upsampled_device", "rtx_get_upsample_stats"]
SHAPES = [(1, 1), (17, 33), (300, 2), (3, 70)]


def test_header_declares_and_library_exports_the_upsample_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_upsample_params_default\(", text, re.M)
    assert "rtx_upsample_params_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_upsample_params_default")
    assert re.search(r"#define\s+RTX_UPSAMPLE_SCALE_MAX\s+8u\b", text) and abi.RTX_UPSAMPLE_SCALE_MAX == 8
    assert re.search(r"#define\s+RTX_UPSAMPLE_E_MAX\s+32\.f\b", text) and abi.RTX_UPSAMPLE_E_MAX == 32.0


@pytest.mark.parametrize("name,mirror,size", [("rtx_upsample_params", abi.UpsampleParams, 32),
                                              ("rtx_upsample_stats", abi.UpsampleStats, 72)])
def test_upsample_struct_layouts_match_compiled_header(tmp_path, name, mirror, size):
    """every field offset and the size of the ctypes mirror against rtx.h as gcc lays it out"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({name}));']
    for f, _ in mirror._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof({name}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(mirror) == size
    for f, _ in mirror._fields_:
        assert int(got[f]) == getattr(mirror, f).offset, f


def test_upsample_params_default_matches_python_mirror():
    lib = rtxpy.rtx_lib()
    p = abi.UpsampleParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    lib.rtx_upsample_params_default(ctypes.byref(p))
    assert set(abi.UPSAMPLE_DEFAULTS) == {f for f, _ in abi.UpsampleParams._fields_}
    for f, _ in abi.UpsampleParams._fields_:
        assert getattr(p, f) == float(np.float32(abi.UPSAMPLE_DEFAULTS[f])), f
    d = rtxpy.Renderer.denoise_params()  # the feature sigmas are the denoiser's
    assert (p.sigma_normal, p.sigma_albedo, p.sigma_plane) == (d.sigma_normal, d.sigma_albedo, d.sigma_plane)
    q = rtxpy.upsample_params(scale=3, demodulate=1)
    assert (q.scale, q.demodulate, q.match_material, q.refine_threshold) == (3, 1, 1, 0.5)
    with pytest.raises(AttributeError):
        rtxpy.upsample_params(sigma_color=1.0)
    lib.rtx_upsample_params_default(None)  # returns


@pytest.fixture(scope="module")
def base_frame():
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    yield scene.frame
    scene.close()


def test_upsample_entries_on_a_null_context_fail_cleanly(base_frame):
    lib = rtxpy.rtx_lib()
    frame, p, up = base_frame(16, 16), rtxpy.default_params(), rtxpy.upsample_params()
    buf = (ctypes.c_float * (16 * 16 * 12))()
    n = ctypes.c_uint32(7)
    u = ctypes.byref(up)
    assert lib.rtx_upsample(None, 16, 16, u, buf, buf, buf, buf, buf) == abi.RTX_ERR_ARG and b"null" in lib.rtx_last_error()
    assert lib.rtx_upsample_device(None, 16, 16, u, buf, buf, buf, buf, buf, None) == abi.RTX_ERR_ARG
    assert lib.rtx_upsample_tiles(None, 16, 16, buf, 0.5, buf, ctypes.byref(n)) == abi.RTX_ERR_ARG
    assert lib.rtx_upsample_tiles_device(None, 16, 16, buf, 0.5, buf, ctypes.byref(n), None) == abi.RTX_ERR_ARG
    assert lib.rtx_render_upsampled(None, ctypes.byref(frame), ctypes.byref(p), u, buf, buf) == abi.RTX_ERR_ARG
    assert lib.rtx_render_upsampled_device(None, ctypes.byref(frame), ctypes.byref(p), u, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_upsample_stats(None, ctypes.byref(abi.UpsampleStats())) == abi.RTX_ERR_ARG
    assert n.value == 7


def test_frame_scaled_argument_errors(base_frame):
    lib = rtxpy.rtx_lib()
    frame, out = base_frame(17, 33), abi.Frame()
    f, o = ctypes.byref(frame), ctypes.byref(out)
    assert lib.rtx_frame_scaled(None, 2, o) == abi.RTX_ERR_ARG and b"null" in lib.rtx_last_error()
    assert lib.rtx_frame_scaled(f, 2, None) == abi.RTX_ERR_ARG
    for s in (0, 9, 16, 0xFFFFFFFF):
        assert lib.rtx_frame_scaled(f, s, o) == abi.RTX_ERR_ARG and b"scale" in lib.rtx_last_error(), s
    for w, h in ((0, 33), (17, 0), (0, 0)):
        bad = base_frame(17, 33)
        bad.width, bad.height = w, h
        assert lib.rtx_frame_scaled(ctypes.byref(bad), 2, o) == abi.RTX_ERR_ARG and b"empty" in lib.rtx_last_error()
    assert bytes(out) == bytes(abi.Frame())  # a refused call writes nothing
    for s in (1, 8):
        assert lib.rtx_frame_scaled(f, s, o) == abi.RTX_OK


def vec(v):
    return np.array(list(v), np.float32)


@pytest.mark.parametrize("w,h", SHAPES)
def test_frame_scaled_matches_the_float64_restatement(base_frame, w, h):
    """s = 1..8: the sizes, the origin's bits, and every component of corner, step_x and step_y within one float ulp
    of the header's formula in float64 (the library rounds the double value once: half an ulp)"""
    frame = base_frame(w, h)
    c, sx, sy = (vec(v).astype(np.float64) for v in (frame.corner, frame.step_x, frame.step_y))
    for s in range(1, 9):
        low = rtxpy.frame_scaled(frame, s)
        assert (low.width, low.height) == (-(-w // s), -(-h // s))
        assert bytes(vec(low.origin)) == bytes(vec(frame.origin))
        if s == 1:
            assert bytes(low) == bytes(frame)
        for got, want in ((low.corner, c + (1 - s) / 2 * sx + (s - 1) / 2 * sy), (low.step_x, s * sx), (low.step_y, s * sy)):
            got = vec(got)
            assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))), (s, got, want)


@pytest.mark.parametrize("w,h", SHAPES)
def test_a_low_pixel_looks_through_the_centre_of_its_block(base_frame, w, h):
    """with the renderer's plane point corner + row step_y + (col + 1) step_x restated in float64, low pixel (c, r)'s
    point is the mean of the points of the s x s full pixels (c s .., r s ..), the ones past the frame's border
    included; the bound is the rounding of the low frame's nine floats carried through the formula"""
    frame = base_frame(w, h)

    def points(fr, cols, rows):
        c, sx, sy = (vec(v).astype(np.float64) for v in (fr.corner, fr.step_x, fr.step_y))
        return c + rows[:, None, None] * sy + (cols[None, :, None] + 1) * sx

    for s in range(1, 9):
        low = rtxpy.frame_scaled(frame, s)
        lc, lr = np.arange(low.width), np.arange(low.height)
        got = points(low, lc, lr)
        full = points(frame, np.arange(low.width * s), np.arange(low.height * s))
        want = full.reshape(low.height, s, low.width, s, 3).mean(axis=(1, 3))
        half = lambda v: 0.5 * np.spacing(np.abs(vec(v))).astype(np.float64)  # noqa: E731
        bound = half(low.corner) + lr[:, None, None] * half(low.step_y) + (lc[None, :, None] + 1) * half(low.step_x)
        assert np.all(np.abs(got - want) <= bound + 1e-12 * np.abs(want)), (s, np.abs(got - want).max())
        if s > 1 and w > 1:
            assert np.abs(got - full[:low.height, :low.width]).max() > 100 * bound.max()  # it is not the full frame's grid


def test_the_models_taps_follow_the_header():
    """u = (X - (s - 1) / 2) / s: floor and fraction from integers equal the float64 expression, the weights of a
    pixel's considered taps are positive and at least one lies inside the low frame"""
    for s in range(1, 9):
        for n in (1, 2, 3, 17, 70):
            x0, fx = UM.axis_taps(n, s)
            u = (np.arange(n) - (s - 1) / 2) / s
            assert np.array_equal(x0, np.floor(u)) and np.allclose(fx, u - np.floor(u), atol=1e-15)
            L = UM.low_size(n, s)
            in0, in1 = (x0 >= 0) & (x0 < L), (x0 + 1 >= 0) & (x0 + 1 < L) & (fx > 0)
            assert np.all(in0 | in1), (s, n)
            if s == 1:
                assert np.all(fx == 0) and np.array_equal(x0, np.arange(n))


def test_the_models_tile_rule():
    conf = np.ones((17, 33), np.float32)
    assert UM.tiles(conf, 0.5).size == 0 and np.array_equal(UM.tiles(conf, 2), np.arange(15))
    conf[16, 32] = 0.25
    conf[0, 8] = np.nan  # a NaN is not below
    conf[9, 0] = 0.5     # nor is the threshold itself
    assert UM.tiles(conf, 0.5).tolist() == [14] and UM.tiles(conf, 0.25).tolist() == [] and UM.tiles(conf, 0).tolist() == []


def run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def test_engine_help_names_the_upsample_flags():
    p = run([rtxpy.ENGINE, "--help"])
    assert p.returncode == 0
    for flag in ("--upsample", "--refine", "1..8"):
        assert flag in p.stdout, flag


@pytest.mark.parametrize("flags,says", [
    (["--upsample", "2", "--gpus", "2"], "one GPU"),
    (["--upsample", "0"], "1..8"),
    (["--upsample", "9"], "1..8"),
    (["--upsample", "two"], "1..8"),
    (["--upsample"], "1..8"),
    (["--upsample", "2", "--passes", "4"], "does not combine"),
    (["--upsample", "2", "--aa"], "does not combine"),
    (["--upsample", "2", "--lens", "0.1", "5"], "does not combine"),
    (["--upsample", "2", "--filter", "tent"], "does not combine"),
    (["--upsample", "2", "--adaptive", "--target-error", "0.01"], "does not combine"),
    (["--upsample", "2", "--target-error", "0.01"], "does not combine"),
    (["--upsample", "2", "--passes", "2", "--denoise-variance"], "does not combine"),
    (["--refine", "0.25"], "needs --upsample"),
])
def test_engine_refuses_bad_upsample_flags_before_any_device(tmp_path, flags, says):
    out = tmp_path / "o.tif"
    p = run([rtxpy.ENGINE, os.path.join(C.SCENES, "scene1.json"), str(out), "16", "16"] + flags)
    assert p.returncode == 1, p.stdout + p.stderr
    assert says in p.stdout, p.stdout
    assert "Loading scene" not in p.stdout and "Commencing" not in p.stdout
    assert not out.exists()
