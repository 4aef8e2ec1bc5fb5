"""The shadow-query C-ABI (rtx_trace_shadow_rays, include/rtx.h) on a CPU-only host: declarations,
exports, struct layouts and the argument errors that need no device and no upload."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rtxpy
from rtxpy import abi

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
FUNCS = ["rtx_trace_shadow_rays", "rtx_get_shadow_ray_stats"]
FLAGS = ("RTX_SHADOW_RAYS_SLOTS", "RTX_SHADOW_RAYS_COUNT")


def test_header_declares_and_library_exports_the_shadow_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert "lane i % 64 of the 64-ray packet i / 64" in text  # the tests build waves on purpose


def test_shadow_struct_layouts_match_compiled_header(tmp_path):
    """every field offset and struct size of abi.ShadowRay / ShadowResult / ShadowRayStats against rtx.h as gcc lays it out"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    structs = {"rtx_shadow_ray": abi.ShadowRay, "rtx_shadow_result": abi.ShadowResult, "rtx_shadow_ray_stats": abi.ShadowRayStats}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    for flag in FLAGS:
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
    for flag in FLAGS:
        assert int(got[flag]) == getattr(abi, flag), flag


def test_shadow_ray_is_32_bytes_and_result_16():
    assert ctypes.sizeof(abi.ShadowRay) == 32 and ctypes.sizeof(abi.ShadowResult) == 16
    # the numpy views Renderer.shadow_rays fills are the same records
    for dt, st in ((abi.SHADOW_RAY_DTYPE, abi.ShadowRay), (abi.SHADOW_RESULT_DTYPE, abi.ShadowResult)):
        dt = np.dtype(dt)
        assert dt.itemsize == ctypes.sizeof(st)
        for f, _ in st._fields_:
            assert dt.fields[f][1] == getattr(st, f).offset, f
    assert (abi.RTX_SHADOW_RAYS_SLOTS, abi.RTX_SHADOW_RAYS_COUNT) == (1, 2)


def test_null_context_is_an_argument_error():
    lib = rtxpy.rtx_lib()
    ray, res, st = abi.ShadowRay(), abi.ShadowResult(), abi.ShadowRayStats()
    assert lib.rtx_trace_shadow_rays(None, 1, ctypes.byref(ray), ctypes.byref(res), 0) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_trace_shadow_rays(None, 0, None, None, 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_shadow_rays(None, 1, ctypes.byref(ray), ctypes.byref(res), 4) == abi.RTX_ERR_ARG
    assert lib.rtx_get_shadow_ray_stats(None, ctypes.byref(st)) == abi.RTX_ERR_ARG
    assert lib.rtx_get_shadow_ray_stats(None, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
