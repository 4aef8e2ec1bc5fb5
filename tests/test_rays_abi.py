"""The ray-query C-ABI (rtx_trace_rays*, include/rtx.h) on a CPU-only host: declarations, exports,
struct layouts, argument errors that need no device, and that the GPU tests' hand-made frames
are not vacuous (the oracle itself hits on them)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rays_frames as RF
import rtxpy
from rtxpy import abi

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
FUNCS = ["rtx_trace_rays", "rtx_trace_rays_device", "rtx_frame_rays_device", "rtx_get_ray_stats"]


def test_header_declares_and_library_exports_the_ray_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f


def test_ray_struct_layouts_match_compiled_header(tmp_path):
    """every field offset and struct size of abi.Ray / Hit / RayStats against rtx.h as gcc lays it out"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    structs = {"rtx_ray": abi.Ray, "rtx_hit": abi.Hit, "rtx_ray_stats": abi.RayStats}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    for flag in ("RTX_RAYS_ANY_HIT", "RTX_RAYS_REORDER", "RTX_RAYS_COUNT", "RTX_RAYS_MAX"):
        lines.append(f'printf("{flag} %llu\\n", (unsigned long long){flag});')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    for flag in ("RTX_RAYS_ANY_HIT", "RTX_RAYS_REORDER", "RTX_RAYS_COUNT", "RTX_RAYS_MAX"):
        assert int(got[flag]) == getattr(abi, flag), flag


def test_ray_and_hit_are_32_bytes():
    assert ctypes.sizeof(abi.Ray) == 32 and ctypes.sizeof(abi.Hit) == 32
    # the numpy views Renderer.trace_rays fills are the same records
    for dt, st in ((abi.RAY_DTYPE, abi.Ray), (abi.HIT_DTYPE, abi.Hit)):
        dt = np.dtype(dt)
        assert dt.itemsize == 32
        for f, _ in st._fields_:
            assert dt.fields[f][1] == getattr(st, f).offset, f


def test_null_context_is_an_argument_error():
    lib = rtxpy.rtx_lib()
    ray, hit, st = abi.Ray(), abi.Hit(), abi.RayStats()
    assert lib.rtx_trace_rays(None, 1, ctypes.byref(ray), ctypes.byref(hit), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays(None, 0, None, None, 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays_device(None, 1, None, None, 0, None) == abi.RTX_ERR_ARG
    assert lib.rtx_frame_rays_device(None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_ray_stats(None, ctypes.byref(st)) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()


@pytest.mark.parametrize("name", sorted(RF.SCENE_FILES))
def test_handmade_frames_are_not_vacuous(name):
    """the oracle hits on at least a quarter of the rays of every hand-made frame test_gpu_rays.py
    judges against it, and the far frame's origin is 60 radii out"""
    from rtxpy import oracle
    scene = RF.load_scene(name)
    frames = RF.frames_of(name, scene)
    lo, hi = (np.array(v) for v in RF.BOUNDS[name])
    for key, fr in frames.items():
        z, obj = oracle.primary(scene, fr)
        assert (z > 0).mean() >= 0.25 and ((z > 0) == (obj >= 0)).all(), (name, key, float((z > 0).mean()))
        o = np.array(fr.origin[:])
        if key.startswith("inside"):
            assert (o > lo).all() and (o < hi).all(), (name, key)
            assert np.linalg.norm(o - np.array(scene.desc.camera.position[:])) > 1.0
        if key == "far60":
            assert np.abs(o - 0.5 * (lo + hi)).max() >= 59.9 * 0.5 * (hi - lo).max()
    scene.close()
