"""The denoiser's C-ABI (rtx_frame_features*, rtx_denoise*, include/rtx.h) on a CPU-only host:
declarations, exports, struct layouts, the defaults and the argument errors that need no device."""
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
INT_FUNCS = ["rtx_frame_features_device", "rtx_frame_features", "rtx_denoise_device", "rtx_denoise", "rtx_get_denoise_stats"]
STRUCTS = {"rtx_feature": abi.Feature, "rtx_denoise_params": abi.DenoiseParams, "rtx_denoise_stats": abi.DenoiseStats}


def test_header_declares_and_library_exports_the_denoise_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_denoise_params_default\(", text, re.M)
    assert "rtx_denoise_params_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_denoise_params_default")


def test_denoise_struct_layouts_match_compiled_header(tmp_path):
    """every field offset and struct size of abi.Feature / DenoiseParams / DenoiseStats against rtx.h as gcc lays it out"""
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
    assert int(got["rtx_feature"]) == 48
    for cname, py in STRUCTS.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)


def test_feature_is_48_bytes_and_its_dtype_matches():
    assert ctypes.sizeof(abi.Feature) == 48
    dt = np.dtype(abi.FEATURE_DTYPE)
    assert dt.itemsize == 48
    assert [n for n in dt.names] == [f for f, _ in abi.Feature._fields_]
    for f, _ in abi.Feature._fields_:
        assert dt.fields[f][1] == getattr(abi.Feature, f).offset, f
    # three 16-byte records: {P, z}, {n, material}, {albedo, object}
    assert (abi.Feature.z.offset, abi.Feature.material.offset, abi.Feature.object.offset) == (12, 28, 44)


def test_params_default_matches_python_mirror():
    lib = rtxpy.rtx_lib()
    p = abi.DenoiseParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    lib.rtx_denoise_params_default(ctypes.byref(p))
    assert set(abi.DENOISE_DEFAULTS) == {f for f, _ in abi.DenoiseParams._fields_}
    for f, _ in abi.DenoiseParams._fields_:
        assert getattr(p, f) == (abi.DENOISE_DEFAULTS[f] if f == "iterations" else np.float32(abi.DENOISE_DEFAULTS[f])), f
    assert 1 <= p.iterations <= 8
    q = rtxpy.Renderer.denoise_params(iterations=3, sigma_plane=float("inf"))
    assert (q.iterations, q.sigma_color, q.sigma_plane) == (3, p.sigma_color, float("inf"))
    lib.rtx_denoise_params_default(None)  # returns


def test_null_context_is_an_argument_error():
    lib = rtxpy.rtx_lib()
    fr, feat, st = abi.Frame(), abi.Feature(), abi.DenoiseStats()
    fr.width = fr.height = 1
    p = rtxpy.Renderer.denoise_params()
    rgb = (ctypes.c_float * 3)()
    assert lib.rtx_frame_features(None, ctypes.byref(fr), abi.RTX_U32_SAT, ctypes.byref(feat)) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_frame_features_device(None, ctypes.byref(fr), abi.RTX_U32_SAT, ctypes.byref(feat), None) == abi.RTX_ERR_ARG
    assert lib.rtx_denoise(None, 1, 1, ctypes.byref(p), ctypes.byref(feat), rgb) == abi.RTX_ERR_ARG
    assert lib.rtx_denoise_device(None, 1, 1, ctypes.byref(p), ctypes.byref(feat), rgb, None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_denoise_stats(None, ctypes.byref(st)) == abi.RTX_ERR_ARG
    assert lib.rtx_get_denoise_stats(None, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
