"""The closest-point C-ABI (rtx_closest_points*, include/rtx.h) on a CPU-only host: declarations, exports, struct
layouts and the argument errors that need no device."""
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
FUNCS = ["rtx_closest_point_object", "rtx_closest_points", "rtx_closest_points_device", "rtx_get_closest_stats",
         "rtx_closest_kat", "rtx_closest_kat_grid"]
FLAGS = ("RTX_CLOSEST_BOUNDED_ONLY", "RTX_CLOSEST_REORDER", "RTX_CLOSEST_COUNT", "RTX_NONE")


def test_header_declares_and_library_exports_the_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f


def test_query_is_16_bytes_and_result_32():
    assert ctypes.sizeof(abi.PointQuery) == 16 and ctypes.sizeof(abi.Closest) == 32
    for dt, st in ((abi.POINT_QUERY_DTYPE, abi.PointQuery), (abi.CLOSEST_DTYPE, abi.Closest)):
        dt = np.dtype(dt)
        assert dt.itemsize == ctypes.sizeof(st)
        for f, _ in st._fields_:
            assert dt.fields[f][1] == getattr(st, f).offset, f


def test_struct_layouts_match_compiled_header(tmp_path):
    """every field offset and struct size of abi.PointQuery / Closest / ClosestStats against rtx.h as gcc lays it out"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    structs = {"rtx_point_query": abi.PointQuery, "rtx_closest": abi.Closest, "rtx_closest_stats": abi.ClosestStats}
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
    assert int(got["rtx_point_query"]) == 16 and int(got["rtx_closest"]) == 32
    for cname, py in structs.items():
        assert int(got[cname]) == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(py, f).offset, (cname, f)
    for flag in FLAGS:
        assert int(got[flag]) == getattr(abi, flag), flag


def test_null_context_is_an_argument_error_whatever_else_is_wrong():
    """the context is looked at first, before any device: a null one fails every form of the call"""
    lib = rtxpy.rtx_lib()
    q, r, st = abi.PointQuery(), abi.Closest(), abi.ClosestStats()
    assert lib.rtx_closest_points(None, 1, ctypes.byref(q), ctypes.byref(r), 0) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_closest_points(None, 0, None, None, 0) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points(None, 1, None, None, 0x80) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points(None, abi.RTX_RAYS_MAX + 1, ctypes.byref(q), ctypes.byref(r), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points_device(None, 1, None, None, 0, None) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points_device(None, 1, 8, 8, 0, None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_closest_stats(None, ctypes.byref(st)) == abi.RTX_ERR_ARG


def test_definition_and_kat_argument_errors():
    lib = rtxpy.rtx_lib()
    o = abi.Object()
    p, cp, d = (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), ctypes.c_float()
    ok = (ctypes.addressof(o), ctypes.addressof(p), ctypes.addressof(d), ctypes.addressof(cp))
    assert lib.rtx_closest_point_object(*ok) == abi.RTX_OK
    for k in range(4):
        args = list(ok)
        args[k] = None
        assert lib.rtx_closest_point_object(*args) == abi.RTX_ERR_ARG, k
    o.type = 7
    assert lib.rtx_closest_point_object(*ok) == abi.RTX_ERR_ARG
    assert b"unknown object type" in lib.rtx_last_error()
    # the known-answer entries check their buffers and indices before they look for a device
    o.type = abi.RTX_SPHERE
    out = (ctypes.c_float * 4)()
    idx = (ctypes.c_uint32 * 1)(1)
    assert lib.rtx_closest_kat(1, ctypes.addressof(o), 1, None, None, ctypes.addressof(out)) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_kat(1, ctypes.addressof(o), 1, ctypes.addressof(idx), ctypes.addressof(p), ctypes.addressof(out)) == abi.RTX_ERR_ARG
    assert b"out of range" in lib.rtx_last_error()
    assert lib.rtx_closest_kat(1, ctypes.addressof(o), 2, None, ctypes.addressof(p), ctypes.addressof(out)) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_kat(1, ctypes.addressof(o), abi.RTX_RAYS_MAX + 1, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_kat_grid(1, None, 1, ctypes.addressof(p), ctypes.addressof(out)) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_kat_grid(1 << 20, ctypes.addressof(o), 1 << 20, ctypes.addressof(p), ctypes.addressof(out)) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_kat(0, None, 0, None, None, None) == abi.RTX_OK
