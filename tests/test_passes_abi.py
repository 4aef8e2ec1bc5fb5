"""Multi-pass rendering's C-ABI (rtx_pass_frame, rtx_render_passes*, include/rtx.h) on a CPU-only host: declarations,
exports, struct layouts, the defaults, every argument error of rtx_pass_frame, the frames it returns (identity
cases, the sub-pixel offsets, the thin lens) against float64 numpy restatements, and the engine's flags."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy
from rtxpy import abi

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
INT_FUNCS = ["rtx_pass_frame", "rtx_render_passes", "rtx_render_passes_device", "rtx_get_pass_stats"]
STRUCTS = {"rtx_pass_params": abi.PassParams, "rtx_pass_stats": abi.PassStats}
VEC = ("corner", "step_x", "step_y", "origin")


@pytest.fixture(scope="module")
def frame():
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    fr = scene.frame(64, 64)
    scene.close()
    return fr


def bits(fr):
    return bytes(fr)


def vec(fr, name, dtype=np.float64):
    return np.array(list(getattr(fr, name)), np.float32).astype(dtype)


def phi(k, b):
    """the radical inverse of k in base b, in float64"""
    r, f = 0.0, 1.0 / b
    while k:
        r += (k % b) * f
        k //= b
        f /= b
    return r


def test_header_declares_and_library_exports_the_pass_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_pass_params_default\(", text, re.M)
    assert "rtx_pass_params_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_pass_params_default")
    assert re.search(r"RTX_PASS_JITTER\s*=\s*1\b", text) and abi.RTX_PASS_JITTER == 1
    assert re.search(r"#define\s+RTX_PASSES_MAX\s+65536u", text) and abi.RTX_PASSES_MAX == 65536


def test_pass_struct_layouts_match_compiled_header(tmp_path):
    """every field offset and struct size of abi.PassParams / PassStats against rtx.h as gcc lays it out"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in STRUCTS.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_pass_params_default_matches_python_mirror():
    lib = rtxpy.rtx_lib()
    p = abi.PassParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    lib.rtx_pass_params_default(ctypes.byref(p))
    assert set(abi.PASS_DEFAULTS) == {f for f, _ in abi.PassParams._fields_}
    for f, _ in abi.PassParams._fields_:
        assert getattr(p, f) == abi.PASS_DEFAULTS[f], f
    q = rtxpy.pass_params(passes=7, jitter=True, aperture=0.25)
    assert (q.passes, q.flags, q.aperture, q.focus, q.min_passes) == (7, abi.RTX_PASS_JITTER, 0.25, 1.0, 2)
    assert rtxpy.pass_params(flags=1, jitter=False).flags == 0
    lib.rtx_pass_params_default(None)  # returns


BAD = {
    "k == passes": (dict(passes=4), 4),
    "k above passes": (dict(passes=1), 7),
    "no passes": (dict(passes=0), 0),
    "too many passes": (dict(passes=abi.RTX_PASSES_MAX + 1), 0),
    "unknown flag": (dict(passes=2, flags=2), 0),
    "unknown flag beside jitter": (dict(passes=2, flags=abi.RTX_PASS_JITTER | 0x80000000), 0),
    "negative aperture": (dict(passes=2, aperture=-0.1), 0),
    "NaN aperture": (dict(passes=2, aperture=math.nan), 0),
    "zero focus": (dict(passes=2, aperture=0.1, focus=0.0), 0),
    "negative focus": (dict(passes=2, aperture=0.1, focus=-1.0), 0),
    "infinite focus": (dict(passes=2, aperture=0.1, focus=math.inf), 0),
    "NaN focus": (dict(passes=2, aperture=0.1, focus=math.nan), 0),
    "negative target": (dict(passes=2, target_error=-1e-3), 0),
    "NaN target": (dict(passes=2, target_error=math.nan), 0),
    "min_passes below 2": (dict(passes=4, target_error=0.1, min_passes=1), 0),
    "min_passes above passes": (dict(passes=4, target_error=0.1, min_passes=5), 0),
    "a target with one pass": (dict(passes=1, target_error=0.1), 0),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_pass_frame_argument_errors(frame, case):
    params, k = BAD[case]
    with pytest.raises(rtxpy.RtxError) as e:
        rtxpy.pass_frame(frame, k, **params)
    assert e.value.code == abi.RTX_ERR_ARG


def test_pass_frame_null_pointers_and_zero_steps(frame):
    lib = rtxpy.rtx_lib()
    pp, out = rtxpy.pass_params(passes=2), abi.Frame()
    f, p, o = ctypes.byref(frame), ctypes.byref(pp), ctypes.byref(out)
    assert lib.rtx_pass_frame(None, p, 0, o) == abi.RTX_ERR_ARG and b"null" in lib.rtx_last_error()
    assert lib.rtx_pass_frame(f, None, 0, o) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_frame(f, p, 0, None) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_frame(f, p, 0, o) == abi.RTX_OK
    for name in ("step_x", "step_y"):
        flat = abi.Frame.from_buffer_copy(bytes(frame))
        setattr(flat, name, abi.F3(0.0, 0.0, 0.0))
        rtxpy.pass_frame(flat, 1, passes=2, jitter=True)  # a pinhole takes it
        with pytest.raises(rtxpy.RtxError) as e:
            rtxpy.pass_frame(flat, 1, passes=2, aperture=0.1)
        assert e.value.code == abi.RTX_ERR_ARG
    # what a pinhole ignores: focus, and min_passes without a target
    rtxpy.pass_frame(frame, 1, passes=2, focus=-1.0, min_passes=0)


def test_render_passes_on_a_null_context_fails_cleanly(frame):
    lib = rtxpy.rtx_lib()
    p, pp, st = rtxpy.default_params(), rtxpy.pass_params(passes=2), abi.PassStats()
    rgb = (ctypes.c_float * 3)()
    args = (ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp))
    assert lib.rtx_render_passes(None, *args, rgb, None, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_render_passes_device(None, *args, None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_pass_stats(None, ctypes.byref(st)) == abi.RTX_ERR_ARG
    assert lib.rtx_get_pass_stats(None, None) == abi.RTX_ERR_ARG


def test_pass_zero_with_a_pinhole_is_the_input_frame(frame):
    for jitter in (False, True):
        assert bits(rtxpy.pass_frame(frame, 0, passes=64, jitter=jitter)) == bits(frame)
        # a negative zero, an infinity and a NaN keep their bits too
        odd = abi.Frame.from_buffer_copy(bytes(frame))
        odd.corner = abi.F3(-0.0, math.inf, math.nan)
        assert bits(rtxpy.pass_frame(odd, 0, passes=64, jitter=jitter)) == bits(odd)


def test_without_jitter_and_lens_every_pass_is_the_input_frame(frame):
    for k in range(64):
        assert bits(rtxpy.pass_frame(frame, k, passes=64)) == bits(frame)
    assert bits(rtxpy.pass_frame(frame, abi.RTX_PASSES_MAX - 1, passes=abi.RTX_PASSES_MAX)) == bits(frame)


def test_jitter_offsets_are_the_halton_points(frame):
    """out.corner = corner + (phi_2(k) - 1/2) step_x + (phi_3(k) - 1/2) step_y to one float ulp per component;
    the offset recovered from it (step_x and step_y are orthogonal) lies in [-1/2, 1/2), and over k = 0..63 the
    offsets' mean is within 1/32 of 0 on each axis (a base-b radical inverse over b^m points is an exact
    stratification: in base 2 the 64 points are the multiples of 1/64; in base 3 the first 54 are two full sets
    of 27 strata and the last 10 fill ninths and their thirds evenly, short of one full set)"""
    c, sx, sy = vec(frame, "corner"), vec(frame, "step_x"), vec(frame, "step_y")
    assert abs(sx @ sy) <= 1e-12 * np.linalg.norm(sx) * np.linalg.norm(sy)
    offs = [(0.0, 0.0)]
    for k in range(1, 64):
        out = rtxpy.pass_frame(frame, k, passes=64, jitter=True)
        for name in ("step_x", "step_y", "origin"):
            assert bytes(getattr(out, name)) == bytes(getattr(frame, name)), name
        assert (out.width, out.height) == (frame.width, frame.height)
        ox, oy = phi(k, 2) - 0.5, phi(k, 3) - 0.5
        want = c + ox * sx + oy * sy
        got = vec(out, "corner")
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got - want) <= ulp), k
        d = got - c
        rx, ry = (d @ sx) / (sx @ sx), (d @ sy) / (sy @ sy)
        # the recovered offset carries the corner's float rounding over the step's length
        tol = float(np.linalg.norm(ulp)) / min(np.linalg.norm(sx), np.linalg.norm(sy))
        assert abs(rx - ox) <= tol and abs(ry - oy) <= tol, k
        assert -0.5 <= ox < 0.5 and -0.5 <= oy < 0.5
        assert -0.5 - tol <= rx < 0.5 + tol and -0.5 - tol <= ry < 0.5 + tol
        offs.append((rx, ry))
    mean = np.mean(offs, axis=0)
    assert abs(mean[0]) <= 1 / 32 and abs(mean[1]) <= 1 / 32, mean


def test_thin_lens_rays_meet_at_the_pixels_focal_point(frame):
    """aperture 0.3, focus 5: for every k < 32 the line from out.origin through a pixel's sample point (corner +
    (c+1) step_x + r step_y, as k_trace forms it) passes within 1e-4 focus |corner - origin| of pass 0's point
    for that pixel (float32 rounding of the frame's components, about 2e-7 relative, with margin); the lens
    point lies within the aperture and in the lens plane (the origin's components are below 8, so their float
    rounding moves it out of the plane by less than 2.4e-7 * sqrt(3) < 1e-6)"""
    ap, focus = 0.3, 5.0
    o, c = vec(frame, "origin"), vec(frame, "corner")
    nrm = np.cross(vec(frame, "step_x"), vec(frame, "step_y"))
    nrm /= np.linalg.norm(nrm)
    tol = 1e-4 * focus * np.linalg.norm(c - o)
    pixels = [(0, 0), (63, 0), (0, 63), (63, 63), (32, 32)]

    def sample(fr, px, py):
        return vec(fr, "corner") + (px + 1) * vec(fr, "step_x") + py * vec(fr, "step_y")

    f0 = rtxpy.pass_frame(frame, 0, passes=32, aperture=ap, focus=focus)
    assert bytes(f0.origin) == bytes(frame.origin)
    focal = [sample(f0, *p) for p in pixels]
    for p, fp in zip(pixels, focal):  # the plane in focus is the image plane scaled about the origin
        assert np.linalg.norm(fp - (o + focus * (sample(frame, *p) - o))) <= tol
    seen = set()
    for k in range(32):
        fk = rtxpy.pass_frame(frame, k, passes=32, aperture=ap, focus=focus)
        lo = vec(fk, "origin")
        assert np.linalg.norm(lo - o) <= ap * (1 + 1e-6), k
        assert abs((lo - o) @ nrm) <= 1e-6, k
        seen.add(bytes(fk.origin))
        for p, fp in zip(pixels, focal):
            d = sample(fk, *p) - lo
            dist = np.linalg.norm(np.cross(fp - lo, d)) / np.linalg.norm(d)
            assert dist <= tol, (k, p, dist)
    assert len(seen) == 32  # every pass its own lens point
    # the lens point is origin + aperture sqrt(phi_5) (cos, sin)(2 pi phi_7) in the steps' unit vectors
    xh, yh = vec(frame, "step_x") / np.linalg.norm(vec(frame, "step_x")), vec(frame, "step_y") / np.linalg.norm(vec(frame, "step_y"))
    for k in (1, 6, 31):
        r, a = ap * math.sqrt(phi(k, 5)), 2 * math.pi * phi(k, 7)
        want = o + r * (math.cos(a) * xh + math.sin(a) * yh)
        got = vec(rtxpy.pass_frame(frame, k, passes=32, aperture=ap, focus=focus), "origin")
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)), k


def run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def test_engine_help_names_the_pass_flags():
    p = run([rtxpy.ENGINE, "--help"])
    assert p.returncode == 0
    for flag in ("--passes", "--aa", "--lens", "--target-error"):
        assert flag in p.stdout, flag


@pytest.mark.parametrize("flags", [["--passes", "2"], ["--aa"], ["--lens", "0.2", "4"], ["--target-error", "0.01"]])
def test_engine_refuses_passes_on_several_gpus_before_any_device(tmp_path, flags):
    out = tmp_path / "o.tif"
    p = run([rtxpy.ENGINE, os.path.join(C.SCENES, "scene1.json"), str(out), "16", "16"] + flags + ["--gpus", "2"])
    assert p.returncode == 1, p.stdout + p.stderr
    assert "one GPU" in p.stdout and "Loading scene" not in p.stdout and "Commencing" not in p.stdout
    assert not out.exists()
