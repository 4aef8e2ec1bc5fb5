"""Scenes and frames of the ray-query tests (test_rays_abi.py on the CPU, test_gpu_rays.py on the GPU).

A frame is an origin plus a grid of target points (include/rtx.h rtx_frame), so any pencil of rays
can be judged by the oracle's primary pass.  Besides each scene's own camera the tests use two
hand-made frames per scene, with the origin inside the bounded objects' box away from the camera
and a target grid spanning the scene, and one frame from 60 scene radii out.
"""
import os

import numpy as np

import conftest as C
import rtxpy

W, H = 128, 72

SCENE_FILES = {"scene1": "scene1.json", "scene4": "scene4.json", "scene5": "scene5_standin.json",
               "scene6": "scene6_standin.json"}

# the bounded objects' boxes (spheres and triangles), rounded outward to 0.1
BOUNDS = {"scene1": ([-4.8, -10.5, 0.5], [5.5, 0.0, 12.0]),
          "scene4": ([-5.3, -8.6, 3.0], [5.3, 0.0, 16.9]),
          "scene5": ([-8.0, -4.5, 2.1], [0.9, -0.1, 5.5]),
          "scene6": ([-1.5, -1.9, -2.1], [1.5, 1.6, 4.1])}


def load_scene(name):
    import standins
    f = SCENE_FILES[name]
    if "standin" in f:
        standins.ensure_scene(name)
    return rtxpy.Scene.load(os.path.join(C.SCENES, f), base_dir=C.GOLDEN)


def grid_frame(origin, p00, p10, p01, w=W, h=H):
    """the frame whose pixel (col, row) aims at p00 + (col / w) (p10 - p00) + (row / h) (p01 - p00):
    the renderer forms a target as corner + row * step_y + (col + 1) * step_x"""
    origin, p00, p10, p01 = (np.asarray(v, np.float64) for v in (origin, p00, p10, p01))
    sx, sy = (p10 - p00) / w, (p01 - p00) / h
    fr = rtxpy.Frame()
    fr.width, fr.height = w, h
    for k in range(3):
        fr.origin[k] = origin[k]
        fr.corner[k] = (p00 - sx)[k]
        fr.step_x[k] = sx[k]
        fr.step_y[k] = sy[k]
    return fr


def handmade_frames(name):
    """two frames from inside the scene's box: A from near its back face looking down -z at a grid
    1.5 boxes wide in x and y on its front face, B from near its -x face looking down +x at a grid
    1.5 boxes wide in y and z on its +x face"""
    lo, hi = (np.array(v, np.float64) for v in BOUNDS[name])
    c, e = 0.5 * (lo + hi), hi - lo
    a0 = c + e * [0.3, -0.2, 0.45]
    ga = [[c[0] + sx * 0.75 * e[0], c[1] + sy * 0.75 * e[1], lo[2]] for sx, sy in ((-1, -1), (1, -1), (-1, 1))]
    b0 = c + e * [-0.45, 0.1, -0.1]
    gb = [[hi[0], c[1] + sy * 0.75 * e[1], c[2] + sz * 0.75 * e[2]] for sz, sy in ((-1, -1), (1, -1), (-1, 1))]
    return [grid_frame(a0, *ga), grid_frame(b0, *gb)]


def far_frame(name="scene5", dist=60.0):
    """from `dist` scene radii (the box's largest half extent) out along -z, aimed at a grid over the
    box's cross-section through its centre"""
    lo, hi = (np.array(v, np.float64) for v in BOUNDS[name])
    c, e = 0.5 * (lo + hi), hi - lo
    rad = 0.5 * e.max()
    g = [[c[0] + sx * 0.6 * e[0], c[1] + sy * 0.6 * e[1], c[2]] for sx, sy in ((-1, -1), (1, -1), (-1, 1))]
    return grid_frame(c - [0.0, 0.0, dist * rad], *g)


def frames_of(name, scene):
    """name -> frame: the scene's own camera, the two hand-made frames, scene5's far frame"""
    fa, fb = handmade_frames(name)
    out = {"camera": scene.frame(W, H), "inside_a": fa, "inside_b": fb}
    if name == "scene5":
        out["far60"] = far_frame(name)
    return out
