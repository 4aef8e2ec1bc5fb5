"""The variance-guided denoiser's C-ABI (rtx_denoise_variance*, include/rtx.h) and the engine's
--denoise-variance flag on a CPU-only host: declarations, exports, the struct layout, the defaults, the
argument errors that need no device, the help text and the flag's refusal without a multi-pass flag."""
import ctypes
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
HOST = os.path.join(rtxpy.REPO_ROOT, "c-raytracer_amd", "host")
INT_FUNCS = ["rtx_denoise_variance_device", "rtx_denoise_variance"]


def test_header_declares_and_library_exports_the_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_denoise_variance_params_default\(", text, re.M)
    assert "rtx_denoise_variance_params_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_denoise_variance_params_default")
    for hidden in ("rtx_launch_denoise_variance", "rtx_load_denoise_variance"):
        assert not hasattr(lib, hidden), hidden


def test_struct_layout_matches_compiled_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    py, cname = abi.DenoiseVarianceParams, "rtx_denoise_variance_params"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in py._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(py) == 20
    for f, _ in py._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, f


def test_params_default_matches_python_mirror():
    lib = rtxpy.rtx_lib()
    p = abi.DenoiseVarianceParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    lib.rtx_denoise_variance_params_default(ctypes.byref(p))
    D = abi.DENOISE_VARIANCE_DEFAULTS
    assert set(D) == {f for f, _ in abi.DenoiseVarianceParams._fields_}
    for f, _ in abi.DenoiseVarianceParams._fields_:
        assert getattr(p, f) == (D[f] if f == "iterations" else np.float32(D[f])), f
    assert 1 <= p.iterations <= 8 and p.sigma_color > 0
    # the feature sigmas are rtx_denoise's
    for f in ("sigma_normal", "sigma_albedo", "sigma_plane"):
        assert D[f] == abi.DENOISE_DEFAULTS[f], f
    q = rtxpy.Renderer.denoise_variance_params(iterations=3, sigma_color=float("inf"))
    assert (q.iterations, q.sigma_color, q.sigma_plane) == (3, float("inf"), p.sigma_plane)
    with pytest.raises(AttributeError):
        rtxpy.Renderer.denoise_variance_params(sigma=1.0)
    lib.rtx_denoise_variance_params_default(None)  # returns


def test_null_context_and_null_params_are_argument_errors():
    lib = rtxpy.rtx_lib()
    feat = abi.Feature()
    p = rtxpy.Renderer.denoise_variance_params()
    rgb, var = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(4, 5, 6)
    fake = ctypes.c_void_p(16)  # never read: the null checks come first
    assert lib.rtx_denoise_variance(None, 1, 1, ctypes.byref(p), ctypes.byref(feat), rgb, var) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_denoise_variance_device(None, 1, 1, ctypes.byref(p), ctypes.byref(feat), rgb, var, None) == abi.RTX_ERR_ARG
    assert lib.rtx_denoise_variance(fake, 1, 1, None, ctypes.byref(feat), rgb, var) == abi.RTX_ERR_ARG
    assert lib.rtx_denoise_variance_device(fake, 1, 1, None, ctypes.byref(feat), rgb, var, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert list(rgb) == [1, 2, 3] and list(var) == [4, 5, 6]


def test_engine_help_names_the_flag():
    p = subprocess.run([rtxpy.ENGINE, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "[--denoise-variance]" in p.stdout


def test_the_flag_without_a_multipass_flag_is_a_usage_error(tmp_path):
    """exit 1 with its message before the scene is loaded or any device opened"""
    out = str(tmp_path / "o.tif")
    for extra in ([], ["--denoise"], ["-n", "4"]):
        p = subprocess.run([rtxpy.ENGINE, os.path.join("scenes", "scene1.json"), out, "16", "16", "--denoise-variance"] + extra,
                           cwd=C.GOLDEN, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, p.stdout[-2000:]
        assert "--denoise-variance needs a multi-pass flag" in p.stdout
        assert "Loading scene" not in p.stdout and "Commencing" not in p.stdout
        assert not os.path.exists(out)


def test_the_flags_hash_collides_with_no_other_flag():
    """argv_find matches whole-string DJB hashes: every flag the engine and rtx_params_from_argv look for"""
    flags = set()
    for name in ("main.c", "scene.c"):
        flags |= set(re.findall(r'argv_find\(argc, argv, "([^"]+)"', open(os.path.join(HOST, name)).read()))
    assert "--denoise-variance" in flags and "--denoise" in flags and len(flags) > 20
    djb = rtxpy.scene_lib().rtx_hash_djb
    hashes = {f: djb(f.encode()) for f in flags}
    assert len(set(hashes.values())) == len(flags)
    assert [f for f, h in hashes.items() if h == hashes["--denoise-variance"]] == ["--denoise-variance"]
