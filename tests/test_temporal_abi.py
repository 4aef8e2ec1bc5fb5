"""The temporal accumulation's C-ABI (rtx_frame_project, rtx_temporal*, rtx_render_temporal*, include/rtx.h) on a
CPU-only host: declarations, exports, the struct layouts, the defaults, null contexts, every argument error of
rtx_frame_project, the projection against the oracle's primary hits (the test an off-by-one or a half-pixel
convention fails), and the numpy model's own power on the synthetic pair of frames."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conftest as C
import rtxpy
import temporal_model as TM
from rtxpy import abi, oracle

HEADER = os.path.join(rtxpy.REPO_ROOT, "include", "rtx.h")
INT_FUNCS = ["rtx_frame_project", "rtx_temporal", "rtx_temporal_device", "rtx_render_temporal", "rtx_render_temporal_device",
             "rtx_temporal_reset", "rtx_get_temporal_stats"]
SHAPES = [(1, 1), (17, 33), (300, 2), (3, 70)]


def test_header_declares_and_library_exports_the_temporal_functions():
    text = open(HEADER).read()
    lib = ctypes.CDLL(rtxpy.LIBRTX)
    for f in INT_FUNCS:
        assert re.search(r"^\s*int\s+%s\(" % f, text, re.M), f
        assert f in abi.RTX_SYMBOLS and hasattr(lib, f), f
    assert re.search(r"^\s*void\s+rtx_temporal_params_default\(", text, re.M)
    assert "rtx_temporal_params_default" in abi.RTX_SYMBOLS and hasattr(lib, "rtx_temporal_params_default")
    assert re.search(r"#define\s+RTX_TEMPORAL_HISTORY_MAX\s+65536u\b", text) and abi.RTX_TEMPORAL_HISTORY_MAX == 65536
    assert re.search(r"#define\s+RTX_TEMPORAL_E_MAX\s+32\.f\b", text) and abi.RTX_TEMPORAL_E_MAX == 32.0


@pytest.mark.parametrize("name,mirror,size", [("rtx_temporal_params", abi.TemporalParams, 24),
                                              ("rtx_temporal_stats", abi.TemporalStats, 80)])
def test_temporal_struct_layouts_match_compiled_header(tmp_path, name, mirror, size):
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


def test_temporal_params_default_matches_python_mirror():
    lib = rtxpy.rtx_lib()
    p = abi.TemporalParams()
    ctypes.memset(ctypes.byref(p), 0xFF, ctypes.sizeof(p))
    lib.rtx_temporal_params_default(ctypes.byref(p))
    assert set(abi.TEMPORAL_DEFAULTS) == {f for f, _ in abi.TemporalParams._fields_}
    for f, _ in abi.TemporalParams._fields_:
        assert getattr(p, f) == float(np.float32(abi.TEMPORAL_DEFAULTS[f])), f
    d = rtxpy.Renderer.denoise_params()  # the feature sigmas are the denoiser's
    assert (p.sigma_normal, p.sigma_albedo, p.sigma_plane) == (d.sigma_normal, d.sigma_albedo, d.sigma_plane)
    q = rtxpy.temporal_params(max_history=8, match_material=0)
    assert (q.max_history, q.match_material, q.sigma_plane) == (8, 0, p.sigma_plane)
    with pytest.raises(AttributeError):
        rtxpy.temporal_params(sigma_color=1.0)
    lib.rtx_temporal_params_default(None)  # returns


class Scenes:
    def __init__(self):
        self.s = {}

    def __call__(self, name):
        if name not in self.s:
            self.s[name] = rtxpy.Scene.load(os.path.join(C.SCENES, name + ".json"), base_dir=C.GOLDEN)
        return self.s[name]

    def close(self):
        for s in self.s.values():
            s.close()


@pytest.fixture(scope="module")
def scenes():
    s = Scenes()
    yield s
    s.close()


def test_temporal_entries_on_a_null_context_fail_cleanly(scenes):
    lib = rtxpy.rtx_lib()
    frame, p, pp, tp = scenes("scene1").frame(16, 16), rtxpy.default_params(), rtxpy.pass_params(), rtxpy.temporal_params()
    buf = (ctypes.c_float * (16 * 16 * 12))()
    out = (ctypes.c_float * (16 * 16 * 12))()
    f, t = ctypes.byref(frame), ctypes.byref(tp)
    assert lib.rtx_temporal(None, t, f, buf, buf, buf, None, None, None, None, None, out, out, out, out) == abi.RTX_ERR_ARG
    assert b"null" in lib.rtx_last_error()
    assert lib.rtx_temporal_device(None, t, f, buf, buf, buf, None, None, None, None, None, out, out, out, out, None) == abi.RTX_ERR_ARG
    assert lib.rtx_render_temporal(None, f, ctypes.byref(p), ctypes.byref(pp), t, out, out, out, out) == abi.RTX_ERR_ARG
    assert lib.rtx_render_temporal_device(None, f, ctypes.byref(p), ctypes.byref(pp), t, None, None, None, None, None) == abi.RTX_ERR_ARG
    assert lib.rtx_temporal_reset(None) == abi.RTX_ERR_ARG
    assert lib.rtx_get_temporal_stats(None, ctypes.byref(abi.TemporalStats())) == abi.RTX_ERR_ARG
    assert not any(out)


def test_frame_project_argument_errors(scenes):
    lib = rtxpy.rtx_lib()
    frame = scenes("scene1").frame(17, 33)
    P = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    u, v, front = ctypes.c_double(7.0), ctypes.c_double(7.0), ctypes.c_int(7)
    a = [ctypes.byref(frame), P, ctypes.byref(u), ctypes.byref(v), ctypes.byref(front)]
    for k in range(5):
        b = list(a)
        b[k] = None
        assert lib.rtx_frame_project(*b) == abi.RTX_ERR_ARG and b"null" in lib.rtx_last_error(), k
    for w, h in ((0, 33), (17, 0), (0, 0)):
        bad = scenes("scene1").frame(17, 33)
        bad.width, bad.height = w, h
        assert lib.rtx_frame_project(ctypes.byref(bad), *a[1:]) == abi.RTX_ERR_ARG and b"empty" in lib.rtx_last_error()
    singular = scenes("scene1").frame(17, 33)
    for i in range(3):
        singular.step_y[i] = 2 * singular.step_x[i]
    assert lib.rtx_frame_project(ctypes.byref(singular), *a[1:]) == abi.RTX_ERR_ARG and b"determinant" in lib.rtx_last_error()
    flat = scenes("scene1").frame(17, 33)  # the image plane through the origin
    for i in range(3):
        flat.corner[i] = flat.origin[i]
    assert lib.rtx_frame_project(ctypes.byref(flat), *a[1:]) == abi.RTX_ERR_ARG
    for val in (float("nan"), float("inf")):
        bad = scenes("scene1").frame(17, 33)
        bad.step_x[1] = val
        assert lib.rtx_frame_project(ctypes.byref(bad), *a[1:]) == abi.RTX_ERR_ARG, val
    u.value, v.value, front.value = 7.0, 7.0, 7
    with pytest.raises(rtxpy.RtxError) as e:
        rtxpy.frame_project(singular, np.zeros((2, 3)))
    assert e.value.code == abi.RTX_ERR_ARG
    assert lib.rtx_frame_project(ctypes.byref(singular), *a[1:]) == abi.RTX_ERR_ARG
    assert (u.value, v.value, front.value) == (7.0, 7.0, 7)  # a refused call writes nothing
    assert lib.rtx_frame_project(*a) == abi.RTX_OK and front.value in (0, 1) and u.value != 7.0


def primary_points(frame, z):
    """RTX_PRIMARY_DIR (csrc/rtx_trace.hip) restated in float32 numpy: the plane point corner + y step_y, then step_x
    added x + 1 times one after the other, the direction normalised by a multiplication with 1 / |d|, and the hit point
    P = d t + origin, every operation rounded to float32"""
    w, h = frame.width, frame.height
    c, sx, sy, o = (np.array(list(v), np.float32) for v in (frame.corner, frame.step_x, frame.step_y, frame.origin))
    pp = np.arange(h, dtype=np.float32)[:, None] * sy[None, :] + c[None, :]
    cols = []
    for _ in range(w):
        pp = pp + sx
        cols.append(pp)
    d = np.stack(cols, axis=1) - o
    mag = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=np.float32)
    d = d * (np.float32(1) / mag)[..., None]
    assert d.dtype == np.float32
    return d * z.astype(np.float32)[..., None] + o


def sideways(scene, w, h, pixels, z):
    """the scene's camera moved along its x axis so that a point at the median hit distance shifts by `pixels`"""
    cam = scene.desc.camera
    fr = scene.frame(w, h)
    step = float(np.linalg.norm(TM.vec(fr.step_x)))
    dx = pixels * step * float(np.median(z[z != 0])) / cam.focal_length
    right = TM.vec(cam.vectors[0])
    return scene.camera(move=tuple(dx * right))


@pytest.mark.parametrize("name", ["scene1", "scene3"])
def test_projection_against_the_oracles_primary_hits(scenes, name):
    """a hit point formed as the renderer forms it projects back onto its own pixel within 0.01 px (measured here:
    at most 3.4e-4 px, on the 300-wide frame; a convention error costs half a pixel or a whole one), the library agrees
    with the model's projection to 1e-9 px, and through a camera moved sideways a point lands on a pixel that sees
    the same object at the point's distance"""
    scene = scenes(name)
    worst, checked = 0.0, 0
    for w, h in SHAPES:
        frame = scene.frame(w, h)
        z, obj = oracle.primary(scene, frame)
        hit = z != 0
        if not hit.any():
            continue
        P = primary_points(frame, z)
        u, v, front = rtxpy.frame_project(frame, P)
        ys, xs = np.mgrid[0:h, 0:w]
        assert front[hit].all()
        err = max(np.abs(u - xs)[hit].max(), np.abs(v - ys)[hit].max())
        worst = max(worst, err)
        print(f"{name} {w}x{h}: {int(hit.sum())} hit pixels, max |u - x|, |v - y| = {err:.3e} px")
        assert err <= 0.01, (w, h, err)
        mu, mv, mf = TM.project(frame, P)
        assert np.array_equal(mf[hit], front[hit])
        assert max(np.abs(mu - u)[hit].max(), np.abs(mv - v)[hit].max()) <= 1e-9
        # the camera moved sideways by 3 pixels of image shift
        cam = sideways(scene, w, h, 3.0, z)
        moved = scene.frame(w, h, camera=cam)
        assert bytes(moved) != bytes(frame) and (moved.width, moved.height) == (w, h)
        z2, obj2 = oracle.primary(scene, moved)
        u2, v2, f2 = rtxpy.frame_project(moved, P)
        with np.errstate(invalid="ignore"):
            fin = hit & f2 & np.isfinite(u2) & np.isfinite(v2)
        u2, v2 = np.where(fin, u2, -9.0), np.where(fin, v2, -9.0)
        xr, yr = np.rint(u2).astype(np.int64), np.rint(v2).astype(np.int64)
        ok = fin & (xr >= 0) & (xr < w) & (yr >= 0) & (yr < h)
        ok[ok] &= obj2[yr[ok], xr[ok]] == obj[ok]
        dist = np.linalg.norm(P.astype(np.float64) - TM.vec(moved.origin), axis=-1)
        if not ok.any():
            continue
        # the rounded pixel's centre is up to half a pixel from the point, which on a slanted surface at these sizes is
        # several per cent of the distance by itself (printed: up to 15 % on scene3 17x33).  So the distance asserted
        # is the moved frame's z at (u', v') itself: the oracle's primary hit of a 1x1 frame whose pixel looks through
        # corner' + v' step_y' + (u' + 1) step_x', which asks more of the projection than the pixel's own z would
        rel = np.abs(z2[yr[ok], xr[ok]] - dist[ok]) / dist[ok]
        idx = np.argwhere(ok)
        idx = idx[::max(1, len(idx) // 120)]
        worst_rel, n_same, n_hidden, beyond = 0.0, 0, 0, 0.0
        c2, sx2, sy2 = TM.vec(moved.corner), TM.vec(moved.step_x), TM.vec(moved.step_y)
        for y, x in idx:
            one = abi.Frame.from_buffer_copy(moved)
            one.width = one.height = 1
            through = c2 + v2[y, x] * sy2 + u2[y, x] * sx2
            for i in range(3):
                one.corner[i] = through[i]
            z1, obj1 = oracle.primary(scene, one)
            if obj1[0, 0] != obj[y, x]:  # past the object's silhouette, or something nearer covers it there
                continue
            d = (float(z1[0, 0]) - dist[y, x]) / dist[y, x]
            beyond = max(beyond, d)
            if d < -0.01:  # a round object's own nearer side hides the point from the moved camera
                n_hidden += 1
                continue
            n_same += 1
            worst_rel = max(worst_rel, abs(d))
        print(f"{name} {w}x{h}: moved camera, {int(ok.sum())} points on a pixel of their object (relative distance error "
              f"at the rounded pixel up to {rel.max():.3e}), {len(idx)} of them traced at (u', v'): {n_hidden} hidden by "
              f"their own object, {n_same} seen at a relative distance error of at most {worst_rel:.3e}")
        # a ray through the point never sees past it, and few points turn away from a camera moved by 3 pixels
        assert beyond <= 0.01 and worst_rel <= 0.01, (w, h, beyond, worst_rel)
        assert n_hidden <= 0.1 * len(idx), (w, h, n_hidden, len(idx))
        checked += n_same
    print(f"{name}: max reprojection error {worst:.3e} px, {checked} moved-camera pixels checked")
    assert checked >= 50


def test_the_default_frame_is_unchanged_and_a_camera_moves_it(scenes):
    scene = scenes("scene1")
    assert bytes(scene.frame(17, 33)) == bytes(scene.frame(17, 33, camera=scene.desc.camera)) == bytes(scene.frame(17, 33, camera=scene.camera()))
    moved = scene.frame(17, 33, camera=scene.camera(move=(0.5, 0.0, 0.0)))
    base = scene.frame(17, 33)
    assert TM.vec(moved.origin)[0] == pytest.approx(TM.vec(base.origin)[0] + 0.5)
    assert bytes(moved.step_x) == bytes(base.step_x) and bytes(moved.step_y) == bytes(base.step_y)
    assert TM.vec(scene.desc.camera.position)[0] == TM.vec(base.origin)[0]  # the scene's own camera stays


# ---- the model's power ----
@pytest.fixture(scope="module")
def synth():
    return TM.synthetic()


def test_the_synthetic_frames_let_every_term_decide(synth):
    """leaving any one term out moves some output by more than 1e-2 of its unit (measured: at least 5.1e-2), and no
    tap sits at the cut nor any (u, v) at an integer, where float and double could disagree"""
    full = TM.model_of(synth)
    M, VM = TM.finite_max(synth["c"], synth["hc"]), TM.finite_max(synth["Vc"], synth["Vh"])
    assert np.isnan(synth["hc"]).sum() == 1 and np.isinf(synth["hc"]).sum() == 1
    assert np.isnan(synth["Vh"]).sum() == 1 and np.isinf(synth["Vh"]).sum() == 1
    assert (synth["L"] == 0).any() and synth["L"].max() == 40
    assert full["margin"] > 1e-3, full["margin"]
    for term in TM.TERMS:
        o = TM.model_of(synth, without=term)
        moved = max(np.abs(o["rgb"] - full["rgb"]).max() / M, np.abs(o["var"] - full["var"]).max() / VM,
                    np.abs(o["len"] - full["len"]).max() / 32, np.abs(o["conf"] - full["conf"]).max())
        print(f"without {term}: {moved:.3e}")
        assert moved > 1e-2, (term, moved)
    assert np.abs(TM.model_of(synth, match_material=False)["rgb"] - TM.model_of(synth, without="material")["rgb"]).max() == 0


def test_the_synthetic_frames_lose_history_both_ways(synth):
    full = TM.model_of(synth)
    live = full["len"] > 0
    u, v = full["u"], full["v"]
    with np.errstate(invalid="ignore"):
        inside = (u > -1) & (u < 37) & (v > -1) & (v < 29)
    left, disoccluded = live & ~inside, live & inside & (full["conf"] == 0)
    print(f"{int(live.sum())} live pixels: {int(left.sum())} left the frame, {int(disoccluded.sum())} inside it have conf 0, "
          f"{int((full['conf'] > 0.99).sum())} above 0.99")
    assert left.sum() >= 20 and disoccluded.sum() >= 5
    assert (full["conf"][left] == 0).all() and (full["len"][left] == 1).all()
    # wall behind the rectangle's old place: the taps are the rectangle's records
    wall = synth["f"]["object"] == 0
    x0, y0 = np.floor(u[disoccluded & wall]).astype(int), np.floor(v[disoccluded & wall]).astype(int)
    assert (synth["g"]["object"][np.clip(y0, 0, 28), np.clip(x0, 0, 36)] != 0).any()
    assert (full["conf"] > 0.99).any() and full["conf"].max() <= 1 + 2.0 ** -22  # the four b are float products
    assert (synth["g"]["object"] == 2).any()  # the column thinner than a pixel is in the history


def test_identical_frames_give_integer_taps(synth):
    fr = synth["prev_frame"]
    o = TM.temporal(fr, synth["c"], synth["Vc"], synth["g"], fr, synth["hc"], synth["Vh"], synth["L"], synth["g"])
    ys, xs = np.mgrid[0:29, 0:37]
    live = o["len"] > 0
    assert np.array_equal(o["u"][live], xs[live]) and np.array_equal(o["v"][live], ys[live])
    assert set(np.unique(o["conf"])) <= {0.0, 1.0}
    ok = live & (synth["L"] >= 1) & np.isfinite(synth["hc"]).all(-1) & np.isfinite(synth["Vh"]).all(-1)
    assert np.array_equal(o["conf"][live] == 1, ok[live])
    k = np.minimum(synth["L"], 31)[ok]
    assert np.array_equal(o["len"][ok], k + 1)
    want = synth["hc"][ok].astype(np.float64) + (synth["c"][ok].astype(np.float64) - synth["hc"][ok]) / (k + 1)[:, None]
    assert np.abs(o["rgb"][ok] - want).max() <= 1e-12
    # the same camera built twice is the same bytes, a projected one would not be integer
    u, v, _ = TM.project(fr, synth["g"]["position"])
    hit = synth["g"]["z"] != 0
    assert 0 < np.abs(u - xs)[hit].max() < 1e-3
