"""The C-ABI of renders of a caller's rays and of the camera models (rtx_render_rays*, rtx_ray_features*,
rtx_projection*, rtx_render_projection*, include/rtx.h) on a CPU-only host: declarations, exports, rtx_projection's
layout and defaults, and every argument error that needs no device."""
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
INT_FUNCS = ["rtx_render_rays", "rtx_render_rays_device", "rtx_ray_features", "rtx_ray_features_device",
             "rtx_projection_ray", "rtx_projection_rays_device", "rtx_render_projection", "rtx_render_projection_device"]


def test_header_declares_and_library_exports_the_new_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_projection_default\(", text, re.M)
    assert "rtx_projection_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_projection_default")
    # the launchers and loaders behind them stay out of the exported symbols
    for f in ("rtx_launch_projection_rays", "rtx_load_projection", "rtx_ray_features_common"):
        assert not hasattr(lib, f), f


def test_projection_layout_matches_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_projection));',
             'printf("kinds %d %d %d\\n", RTX_PROJ_PANORAMA, RTX_PROJ_FISHEYE, RTX_PROJ_ORTHO);']
    for f, _ in abi.Projection._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_projection, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(l.split(None, 1) for l in out)
    assert int(got["size"]) == ctypes.sizeof(abi.Projection) == 20
    assert got["kinds"].split() == [str(abi.RTX_PROJ_PANORAMA), str(abi.RTX_PROJ_FISHEYE), str(abi.RTX_PROJ_ORTHO)]
    for f, _ in abi.Projection._fields_:
        assert int(got[f]) == getattr(abi.Projection, f).offset, f


def test_projection_default():
    lib = rtxpy.rtx_lib()
    p = abi.Projection(kind=7, fov=1.0, extent=2.0, offset_x=3.0, offset_y=4.0)
    lib.rtx_projection_default(ctypes.byref(p))
    for f, _ in abi.Projection._fields_:
        assert getattr(p, f) == abi.PROJECTION_DEFAULTS[f], f
    assert p.fov == float(np.float32(2.0 * math.pi))
    lib.rtx_projection_default(None)  # a null pointer is ignored
    q = rtxpy.projection("fisheye", fov=2.0)
    assert (q.kind, q.fov, q.extent) == (abi.RTX_PROJ_FISHEYE, 2.0, 0.0)


@pytest.fixture(scope="module")
def frame():
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    fr = scene.frame(16, 8)
    scene.close()
    return fr


def test_null_contexts_and_buffers_fail_cleanly(frame):
    lib = rtxpy.rtx_lib()
    p, proj = rtxpy.default_params(), rtxpy.projection()
    rays = np.zeros(16 * 8, abi.RAY_DTYPE)
    out = np.zeros(16 * 8 * 12, np.float32)
    f, q, j, r, o = ctypes.byref(frame), ctypes.byref(p), ctypes.byref(proj), rays.ctypes.data, out.ctypes.data
    calls = [lambda: lib.rtx_render_rays(None, 16, 8, r, q, o, None),
             lambda: lib.rtx_render_rays_device(None, 16, 8, r, q, o, None, None),
             lambda: lib.rtx_ray_features(None, 16, 8, r, abi.RTX_U32_SAT, o),
             lambda: lib.rtx_ray_features_device(None, 16, 8, r, abi.RTX_U32_SAT, o, None),
             lambda: lib.rtx_projection_rays_device(None, f, j, r, None),
             lambda: lib.rtx_render_projection(None, f, j, q, o, None),
             lambda: lib.rtx_render_projection_device(None, f, j, q, o, None, None),
             # with a null context every other bad argument is refused the same way
             lambda: lib.rtx_render_rays(None, 16, 8, None, q, o, None),
             lambda: lib.rtx_render_rays(None, 0, 8, r, q, o, None),
             lambda: lib.rtx_ray_features(None, 16, 0, r, abi.RTX_U32_SAT, o),
             lambda: lib.rtx_ray_features(None, 16, 8, r, abi.RTX_U32_SAT, None),
             lambda: lib.rtx_render_projection(None, None, j, q, o, None),
             lambda: lib.rtx_render_projection(None, f, None, q, o, None),
             lambda: lib.rtx_render_projection(None, f, j, None, o, None)]
    for call in calls:
        assert call() == abi.RTX_ERR_ARG
        assert b"null" in lib.rtx_last_error()


def ray_rc(frame, proj, px=0, py=0, out=True):
    rec = np.zeros(1, abi.RAY_DTYPE)
    rc = rtxpy.rtx_lib().rtx_projection_ray(ctypes.byref(frame) if frame is not None else None,
                                             ctypes.byref(proj) if proj is not None else None, px, py,
                                             rec.ctypes.data if out else None)
    return rc, rtxpy.rtx_lib().rtx_last_error().decode()


def copy_of(frame, **fields):
    fr = abi.Frame.from_buffer_copy(frame)
    for k, v in fields.items():
        if isinstance(v, (tuple, list)):
            for i in range(3):
                getattr(fr, k)[i] = v[i]
        else:
            setattr(fr, k, v)
    return fr


def test_projection_ray_argument_errors(frame):
    ok = rtxpy.projection()
    assert ray_rc(frame, ok)[0] == abi.RTX_OK
    assert ray_rc(frame, ok, 15, 7)[0] == abi.RTX_OK
    for args, word in [((None, ok), "null"), ((frame, None), "null"), ((frame, ok, 0, 0, False), "null"),
                       ((frame, ok, 16, 0), "outside"), ((frame, ok, 0, 8), "outside"),
                       ((frame, rtxpy.projection(kind=3)), "kind"), ((frame, rtxpy.projection(kind=-1)), "kind"),
                       ((frame, rtxpy.projection("panorama", fov=0.0)), "fov"),
                       ((frame, rtxpy.projection("panorama", fov=-1.0)), "fov"),
                       ((frame, rtxpy.projection("fisheye", fov=6.3)), "fov"),
                       ((frame, rtxpy.projection("fisheye", fov=math.nan)), "fov"),
                       ((frame, rtxpy.projection("ortho", extent=-1.0)), "extent"),
                       ((frame, rtxpy.projection("ortho", extent=math.inf)), "extent"),
                       ((frame, rtxpy.projection("panorama", offset_x=math.nan)), "offset"),
                       ((frame, rtxpy.projection("panorama", offset_y=math.inf)), "offset"),
                       ((copy_of(frame, width=0), ok), "frame"), ((copy_of(frame, height=0), ok), "frame"),
                       ((copy_of(frame, step_x=(0, 0, 0)), ok), "zero length"),
                       ((copy_of(frame, step_y=(0, 0, 0)), ok), "zero length"),
                       ((copy_of(frame, step_y=tuple(frame.step_x)), ok), "perpendicular"),
                       ((copy_of(frame, origin=(math.nan, 0, 0)), ok), "finite")]:
        rc, msg = ray_rc(*args)
        assert rc == abi.RTX_ERR_ARG and word in msg, (word, rc, msg)
    # an origin in the image plane gives no side to look to
    flat = copy_of(frame, corner=(0, 0, 0), step_x=(1, 0, 0), step_y=(0, 1, 0), origin=(3, 2, 0))
    rc, msg = ray_rc(flat, ok)
    assert rc == abi.RTX_ERR_ARG and "image plane" in msg
    assert ray_rc(copy_of(flat, origin=(3, 2, -1)), ok)[0] == abi.RTX_OK
    # fov is not looked at for an orthographic view, extent not for the angular ones
    assert ray_rc(frame, rtxpy.projection("ortho", fov=0.0))[0] == abi.RTX_OK
    assert ray_rc(frame, rtxpy.projection("fisheye", fov=1.0, extent=-5.0))[0] == abi.RTX_OK


def run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def test_engine_help_names_projection():
    p = run([rtxpy.ENGINE, "--help"])
    assert p.returncode == 0 and "--projection" in p.stdout


@pytest.mark.parametrize("flags,word", [(["--projection"], "panorama, fisheye DEGREES or ortho EXTENT"),
                                        (["--projection", "cube"], "panorama, fisheye DEGREES or ortho EXTENT"),
                                        (["--projection", "fisheye"], "panorama, fisheye DEGREES or ortho EXTENT"),
                                        (["--projection", "fisheye", "0"], "(0, 360]"),
                                        (["--projection", "fisheye", "400"], "(0, 360]"),
                                        (["--projection", "ortho", "-2"], "at least 0"),
                                        (["--projection", "panorama", "--gpus", "2"], "one GPU"),
                                        (["--projection", "panorama", "--passes", "4"], "--passes"),
                                        (["--projection", "fisheye", "180", "--aa"], "--passes"),
                                        (["--projection", "ortho", "0", "--upsample", "2"], "--upsample")])
def test_engine_refuses_projection_combinations_before_any_device(tmp_path, flags, word):
    out = tmp_path / "o.tif"
    p = run([rtxpy.ENGINE, os.path.join(C.SCENES, "scene1.json"), str(out), "16", "16"] + flags)
    assert p.returncode == 1, p.stdout + p.stderr
    assert word in p.stdout and "Loading scene" not in p.stdout and "Commencing" not in p.stdout
    assert not out.exists()
