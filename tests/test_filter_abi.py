"""The pixel reconstruction filters' C-ABI (rtx_pass_filter_weights, rtx_render_passes_filtered*, include/rtx.h) on
a CPU-only host: declarations, exports, the struct layout, the defaults, every argument error of
rtx_pass_filter_weights, the weight tables against a float64 restatement of the header's formulas, the filters'
interior sums, a positive weight sum under every truncation by the frame's border, and the engine's flags."""
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
INT_FUNCS = ["rtx_pass_filter_weights", "rtx_render_passes_filtered", "rtx_render_passes_filtered_device"]
F32 = lambda x: float(np.float32(x))  # noqa: E731


def phi(k, b):
    """the radical inverse of k in base b, as the library sums it"""
    inv = 1.0 / b
    f, r = inv, 0.0
    while k:
        r += (k % b) * f
        k //= b
        f *= inv
    return r


def offset(k, jitter=True):
    return (phi(k, 2) - 0.5, phi(k, 3) - 0.5) if jitter and k else (0.0, 0.0)


def f_model(kind, d, r, a):
    """f(d) as include/rtx.h writes it, in Python floats (IEEE double, the header's operation order)"""
    if kind == "box":
        return 1.0 if -r <= d < r else 0.0
    if kind == "tent":
        return max(0.0, 1.0 - abs(d) / r)
    if kind == "gaussian":
        return math.exp(-a * (d * d)) - math.exp(-a * (r * r)) if abs(d) < r else 0.0
    if abs(d) >= r:
        return 0.0
    x = abs(2.0 * d / r)
    if x < 1.0:
        return ((7.0 * x - 12.0) * x * x + 16.0 / 3.0) / 6.0
    return (((-7.0 / 3.0 * x + 12.0) * x - 20.0) * x + 32.0 / 3.0) / 6.0


def test_header_declares_and_library_exports_the_filter_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_filter_params_default\(", text, re.M)
    assert "rtx_filter_params_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_filter_params_default")
    assert re.search(r"RTX_FILTER_BOX = 0, RTX_FILTER_TENT = 1, RTX_FILTER_GAUSSIAN = 2, RTX_FILTER_MITCHELL = 3", text)
    assert (abi.RTX_FILTER_BOX, abi.RTX_FILTER_TENT, abi.RTX_FILTER_GAUSSIAN, abi.RTX_FILTER_MITCHELL) == (0, 1, 2, 3)
    assert re.search(r"#define\s+RTX_FILTER_TAPS\s+5\b", text) and abi.RTX_FILTER_TAPS == 5


def test_filter_struct_layout_matches_compiled_header(tmp_path):
    """every field offset and the size of abi.FilterParams against rtx.h as gcc lays it out"""
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtx.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rtx_filter_params));']
    for f, _ in abi.FilterParams._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rtx_filter_params, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(abi.FilterParams) == 16
    for f, _ in abi.FilterParams._fields_:
        assert int(got[f]) == getattr(abi.FilterParams, f).offset, f


def test_filter_params_default_matches_python_mirror():
    lib = rtxpy.rtx_lib()
    p = abi.FilterParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    lib.rtx_filter_params_default(ctypes.byref(p))
    assert set(abi.FILTER_DEFAULTS) == {f for f, _ in abi.FilterParams._fields_}
    for f, _ in abi.FilterParams._fields_:
        assert getattr(p, f) == abi.FILTER_DEFAULTS[f], f
    q = rtxpy.filter_params(kind="mitchell", radius=2.0)
    assert (q.kind, q.radius, q.alpha, q.pad_) == (abi.RTX_FILTER_MITCHELL, 2.0, 2.0, 0)
    with pytest.raises(ValueError):
        rtxpy.filter_params(kind="lanczos")
    with pytest.raises(AttributeError):
        rtxpy.filter_params(width=3)
    lib.rtx_filter_params_default(None)  # returns


BAD_FILTER = {
    "unknown kind": dict(kind=4),
    "unknown kind, high bit": dict(kind=0x80000000),
    "box radius below 0.5": dict(kind="box", radius=0.49),
    "box radius above 2.5": dict(kind="box", radius=2.51),
    "tent radius below 1": dict(kind="tent", radius=0.99),
    "tent radius above 2.5": dict(kind="tent", radius=2.6),
    "gaussian radius below 1": dict(kind="gaussian", radius=0.5),
    "gaussian radius above 2.5": dict(kind="gaussian", radius=3.0),
    "mitchell radius below 1": dict(kind="mitchell", radius=0.5),
    "mitchell radius above 2.5": dict(kind="mitchell", radius=math.inf),
    "NaN radius": dict(kind="tent", radius=math.nan),
    "negative radius": dict(kind="box", radius=-1.0),
    "zero alpha": dict(kind="gaussian", alpha=0.0),
    "negative alpha": dict(kind="gaussian", alpha=-2.0),
    "infinite alpha": dict(kind="gaussian", alpha=math.inf),
    "NaN alpha": dict(kind="gaussian", alpha=math.nan),
    "pad": dict(pad_=1),
}
BAD_PASS = {
    "k == passes": (dict(passes=4), 4),
    "no passes": (dict(passes=0), 0),
    "too many passes": (dict(passes=abi.RTX_PASSES_MAX + 1), 0),
    "unknown flag": (dict(passes=2, flags=2), 0),
    "negative aperture": (dict(passes=2, aperture=-0.1), 0),
    "zero focus": (dict(passes=2, aperture=0.1, focus=0.0), 0),
    "NaN target": (dict(passes=2, target_error=math.nan), 0),
    "min_passes above passes": (dict(passes=4, target_error=0.1, min_passes=5), 0),
}


@pytest.mark.parametrize("case", sorted(BAD_FILTER))
def test_filter_weights_refuses_bad_filters(case):
    with pytest.raises(rtxpy.RtxError) as e:
        rtxpy.filter_weights(0, filter=rtxpy.filter_params(**BAD_FILTER[case]), passes=2, jitter=True)
    assert e.value.code == abi.RTX_ERR_ARG


@pytest.mark.parametrize("case", sorted(BAD_PASS))
def test_filter_weights_refuses_bad_pass_parameters(case):
    params, k = BAD_PASS[case]
    with pytest.raises(rtxpy.RtxError) as e:
        rtxpy.filter_weights(k, **params)
    assert e.value.code == abi.RTX_ERR_ARG


def test_filter_weights_null_pointers_and_what_it_ignores():
    lib = rtxpy.rtx_lib()
    pp, fp = rtxpy.pass_params(passes=2), rtxpy.filter_params()
    wx, wy = (ctypes.c_double * 5)(), (ctypes.c_double * 5)()
    p, f = ctypes.byref(pp), ctypes.byref(fp)
    assert lib.rtx_pass_filter_weights(None, f, 0, wx, wy) == abi.RTX_ERR_ARG and b"null" in lib.rtx_last_error()
    assert lib.rtx_pass_filter_weights(p, None, 0, wx, wy) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_filter_weights(p, f, 0, None, wy) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_filter_weights(p, f, 0, wx, None) == abi.RTX_ERR_ARG
    assert lib.rtx_pass_filter_weights(p, f, 0, wx, wy) == abi.RTX_OK
    # alpha is the Gaussian's alone; the range ends are inside
    for kind in ("box", "tent", "mitchell"):
        rtxpy.filter_weights(1, filter=rtxpy.filter_params(kind=kind, alpha=math.nan), passes=2, jitter=True)
    for kind, (lo, hi) in abi.FILTER_RADIUS.items():
        rtxpy.filter_weights(1, filter=kind, radius=lo, passes=2, jitter=True)
        rtxpy.filter_weights(1, filter=kind, radius=hi, passes=2, jitter=True)


def test_filtered_entries_on_a_null_context_fail_cleanly():
    lib = rtxpy.rtx_lib()
    scene = rtxpy.Scene.load(os.path.join(C.SCENES, "scene1.json"), base_dir=C.GOLDEN)
    frame = scene.frame(16, 16)
    scene.close()
    p, pp, fp = rtxpy.default_params(), rtxpy.pass_params(passes=2), rtxpy.filter_params()
    rgb = (ctypes.c_float * (3 * 256))()
    args = (ctypes.byref(frame), ctypes.byref(p), ctypes.byref(pp), ctypes.byref(fp))
    assert lib.rtx_render_passes_filtered(None, *args, rgb, None, None) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_render_passes_filtered_device(None, *args, None, None, None, None) == abi.RTX_ERR_ARG


CASES = [("box", 0.5), ("box", 1.5), ("tent", 1.0), ("tent", 2.5), ("gaussian", 1.5), ("gaussian", 2.25),
         ("mitchell", 2.0), ("mitchell", 1.3)]


@pytest.mark.parametrize("kind,radius", CASES)
def test_weights_match_the_float64_restatement(kind, radius):
    """k = 0 .. 63 with jitter (and k = 5 without): 4 double ulps, exp being the only inexact step"""
    alpha = 3.5 if radius == 2.25 else 2.0
    r, a = F32(radius), F32(alpha)
    for k in list(range(64)) + [None]:
        jitter = k is not None
        kk = 5 if k is None else k
        wx, wy = rtxpy.filter_weights(kk, filter=kind, radius=radius, alpha=alpha, passes=64, jitter=jitter)
        ox, oy = offset(kk, jitter)
        for got, o in ((wx, ox), (wy, oy)):
            want = np.array([f_model(kind, (i - 2) + o, r, a) for i in range(5)])
            assert np.all(np.abs(got - want) <= 4 * np.spacing(np.abs(want))), (k, got, want)
        assert wx.dtype == np.float64 and np.all(np.isfinite(wx)) and np.all(np.isfinite(wy))
        if kind != "mitchell":
            assert np.all(wx >= 0) and np.all(wy >= 0)
        assert wx[2] > 0 and wy[2] > 0  # the tap q = p


def test_box_half_is_the_single_tap():
    for k in range(256):
        for jitter in (False, True):
            wx, wy = rtxpy.filter_weights(k, filter="box", radius=0.5, passes=256, jitter=jitter)
            assert wx.tolist() == [0, 0, 1, 0, 0] and wy.tolist() == [0, 0, 1, 0, 0], k


def test_interior_sums_of_the_partition_of_unity_filters():
    for k in range(64):
        for kind, radius, tol in (("tent", 1.0, 1e-15), ("mitchell", 2.0, 1e-14)):
            wx, wy = rtxpy.filter_weights(k, filter=kind, radius=radius, passes=64, jitter=True)
            assert abs(math.fsum(wx) - 1.0) <= tol and abs(math.fsum(wy) - 1.0) <= tol, (kind, k)


@pytest.mark.parametrize("kind", sorted(abi.FILTER_KINDS))
def test_weight_sums_stay_positive_under_every_border_truncation(kind):
    """W_k(p) > 0: a pixel at or near the frame's border loses 0 - 2 taps on each side of each axis.  Radii
    stepped by 0.05 over the kind's range, k < 4096; the x offsets phi_2 and the y offsets phi_3 both.  The tables
    come from the restatement (checked against the library above) so that the sweep stays quick, and from the
    library at every 64th pass."""
    lo, hi = abi.FILTER_RADIUS[abi.FILTER_KINDS[kind]]
    offs = np.array([offset(k) for k in range(4096)]).T.ravel()  # all x offsets, then all y offsets
    smallest = math.inf
    for radius in np.arange(lo, hi + 1e-9, 0.05):
        r = F32(min(radius, hi))
        w = np.array([[f_model(kind, (i - 2) + o, r, 2.0) for i in range(5)] for o in offs])
        for left in range(3):
            for right in range(3):
                s = w[:, left:5 - right].sum(axis=1)
                smallest = min(smallest, float(s.min()))
                assert s.min() > 0, (kind, r, left, right)
        for k in range(0, 4096, 64):
            wx, wy = rtxpy.filter_weights(k, filter=kind, radius=r, passes=4096, jitter=True)
            for t in (wx, wy):
                assert min(t[left:5 - right].sum() for left in range(3) for right in range(3)) > 0, (kind, r, k)
    print(f"{kind}: the smallest per-axis weight sum over radii, passes and truncations is {smallest:.4g}")
    if kind == "mitchell":
        assert smallest > 0.05  # what include/rtx.h states


def run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=120, **kw)


def test_engine_help_names_the_filter_flags():
    p = run([rtxpy.ENGINE, "--help"])
    assert p.returncode == 0
    for flag in ("--filter", "--filter-radius", "--filter-alpha", "box", "tent", "gaussian", "mitchell"):
        assert flag in p.stdout, flag


@pytest.mark.parametrize("flags,says", [
    (["--filter", "gaussian", "--gpus", "2"], "one GPU"),
    (["--filter", "tent", "--adaptive", "--target-error", "0.01"], "--adaptive"),
    (["--filter", "lanczos"], "box, tent, gaussian, mitchell"),
    (["--filter"], "box, tent, gaussian, mitchell"),
    (["--filter", "tent", "--filter-radius", "0.5"], "radius"),
    (["--filter", "box", "--filter-radius", "3"], "radius"),
    (["--filter", "mitchell", "--filter-radius", "nan"], "radius"),
    (["--filter", "gaussian", "--filter-alpha", "0"], "alpha"),
    (["--filter-radius", "2"], "need --filter"),
])
def test_engine_refuses_bad_filter_flags_before_any_device(tmp_path, flags, says):
    out = tmp_path / "o.tif"
    p = run([rtxpy.ENGINE, os.path.join(C.SCENES, "scene1.json"), str(out), "16", "16"] + flags)
    assert p.returncode == 1, p.stdout + p.stderr
    assert says in p.stdout, p.stdout
    assert "Loading scene" not in p.stdout and "Commencing" not in p.stdout
    assert not out.exists()
