"""rtxpy — Python (ctypes) driver for the rtx C-ABI (include/rtx.h, include/rtx_scene.h).

Host plumbing for tests and bench.py.  The product is the C-ABI library
``c-raytracer_amd/lib/librtx.so`` (HIP kernels for gfx950) and the C host glue
``librtxscene.so``; this module only loads them.  There is no CPU fallback:
``Renderer`` raises if librtx.so is missing or no gfx950 device is usable.

The CPU oracle (``oracle/librtx_oracle.so``) is test infrastructure and is
reached only through ``rtxpy.oracle`` by tests/, ``__graft_entry__.smoke()``
and bench.py's cpu_baseline leg.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .abi import (Frame, Params, SceneDesc, Stats, RTX_OK)  # noqa: F401

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_ROOT = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIBRTX = os.environ.get("RTX_LIBRTX") or os.path.join(LIB_DIR, "librtx.so")  # override: build variants
LIBSCENE = os.path.join(LIB_DIR, "librtxscene.so")
ENGINE = os.path.join(LIB_DIR, "engine")

_scene_lib = None
_rtx_lib = None


class RtxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rtx error {code}: {msg}")
        self.code = code


def scene_lib():
    global _scene_lib
    if _scene_lib is None:
        if not os.path.exists(LIBSCENE):
            raise RtxError(abi.RTX_ERR_STATE, f"{LIBSCENE} not built (run __graft_entry__.build())")
        lib = C.CDLL(LIBSCENE)
        abi.declare_scene(lib)
        _scene_lib = lib
    return _scene_lib


def rtx_lib():
    """Load librtx.so (the HIP path).  Raises when it is missing: no fallback."""
    global _rtx_lib
    if _rtx_lib is None:
        if not os.path.exists(LIBRTX):
            raise RtxError(abi.RTX_ERR_STATE, f"{LIBRTX} not built (run __graft_entry__.build())")
        lib = C.CDLL(LIBRTX)
        abi.declare_rtx(lib)
        _rtx_lib = lib
    return _rtx_lib


def _check_scene(rc):
    if rc != RTX_OK:
        raise RtxError(rc, scene_lib().rtx_scene_last_error().decode(errors="replace"))


def _check(rc):
    if rc != RTX_OK:
        raise RtxError(rc, rtx_lib().rtx_last_error().decode(errors="replace"))


class Scene:
    """A loaded scene (owner of the C rtx_scene)."""

    def __init__(self, handle):
        self._h = handle
        self.desc = scene_lib().rtx_scene_desc_of(handle).contents

    @classmethod
    def load(cls, path, scale=None, base_dir=None):
        h = C.c_void_p()
        _check_scene(scene_lib().rtx_scene_load(os.fsencode(path), scale.encode() if scale else None,
                                                os.fsencode(base_dir) if base_dir else None, C.byref(h)))
        return cls(h)

    @classmethod
    def parse(cls, text, name="<memory>", scale=None, base_dir=None):
        data = text.encode() if isinstance(text, str) else text
        h = C.c_void_p()
        _check_scene(scene_lib().rtx_scene_parse(data, len(data), name.encode(), scale.encode() if scale else None,
                                                 os.fsencode(base_dir) if base_dir else None, C.byref(h)))
        return cls(h)

    def frame(self, width, height, camera=None):
        """rtx_frame_setup of the scene's camera, or of `camera` (an abi.Camera: a moved copy of self.desc.camera)"""
        fr = Frame()
        cam = self.desc.camera if camera is None else camera
        _check_scene(scene_lib().rtx_frame_setup(C.byref(cam), width, height, C.byref(fr)))
        return fr

    def camera(self, move=(0.0, 0.0, 0.0)):
        """a copy of the scene's camera, its position moved by `move` in world units (the orientation kept)"""
        cam = abi.Camera.from_buffer_copy(self.desc.camera)
        for i in range(3):
            cam.position[i] += move[i]
        return cam

    @property
    def num_objects(self):
        return self.desc.num_objects

    def objects(self):
        return [self.desc.objects[i] for i in range(self.desc.num_objects)]

    def materials(self):
        return [self.desc.materials[i] for i in range(self.desc.num_materials)]

    def emitters(self):
        return [self.desc.emitters[i] for i in range(self.desc.num_emitters)]

    def close(self):
        if self._h:
            scene_lib().rtx_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_params(**kw):
    """rtx_params_default (render.c:53-60 defaults) plus overrides."""
    p = Params()
    p.max_bounces = 10
    p.min_intensity_sqr = 0.01 * 0.01
    p.reflection = abi.RTX_PHONG
    p.gi = abi.RTX_GI_AMBIENT
    p.samples = 1
    p.attenuation = abi.RTX_ATT_SQR
    p.attenuation_offset = 1.0
    p.rng = abi.RTX_RNG_COUNTER
    p.seed = 1
    p.u32conv = abi.RTX_U32_SAT
    p.tile_offset = 0
    p.tile_stride = 1
    p.count_traversal = 0
    # float32 rounding of .01f*.01f like the C default
    p.min_intensity_sqr = float(np.float32(np.float32(0.01) * np.float32(0.01)))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def params_from_args(args, **kw):
    """render_init (render.c:61-116) over a reference-style argument list."""
    p = default_params(**kw)
    argv = [b"engine"] + [a.encode() for a in args]
    arr = (C.c_char_p * len(argv))(*argv)
    scene_lib().rtx_params_from_argv(len(argv), arr, C.byref(p))
    return p


def hash_djb(s):
    return scene_lib().rtx_hash_djb(s.encode())


def write_tiff(path, rgb, z=None, raw=False):
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    zz = None
    if raw:
        zz = np.ascontiguousarray(z, dtype=np.float32)
    rc = scene_lib().rtx_tiff_write(os.fsencode(path), w, h, rgb.ctypes.data,
                                    zz.ctypes.data if zz is not None else None, 1 if raw else 0)
    if rc != RTX_OK:
        raise RtxError(rc, f"tiff write failed: {path}")


def read_tiff_raw(path):
    """rtx_tiff_read_raw (librtxscene): (rgb (H,W,3), z (H,W)) float32 of a raw TIFF."""
    w, h = C.c_uint32(), C.c_uint32()
    prgb, pz = C.c_void_p(), C.c_void_p()
    rc = scene_lib().rtx_tiff_read_raw(os.fsencode(path), C.byref(w), C.byref(h), C.byref(prgb), C.byref(pz))
    if rc != RTX_OK:
        raise RtxError(rc, f"raw tiff read failed: {path}")
    try:
        n = w.value * h.value
        rgb = np.ctypeslib.as_array((C.c_float * (3 * n)).from_address(prgb.value)).reshape(h.value, w.value, 3).copy()
        z = np.ctypeslib.as_array((C.c_float * n).from_address(pz.value)).reshape(h.value, w.value).copy()
    finally:
        scene_lib().rtx_buffer_free(prgb)
        scene_lib().rtx_buffer_free(pz)
    return rgb, z


def post_from_args(args):
    """rtx_post_from_argv over ["postprocess", "<in>", "<out>"] + args (the reference's argv layout)."""
    from .abi import Post
    argv = [b"postprocess", b"in.tif", b"out.tif"] + [a.encode() for a in args]
    arr = (C.c_char_p * len(argv))(*argv)
    p = Post()
    rc = scene_lib().rtx_post_from_argv(len(argv), arr, C.byref(p))
    if rc != RTX_OK:
        raise RtxError(rc, scene_lib().rtx_scene_last_error().decode())
    return p


def write_stl(path, tris):
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    _check_scene(scene_lib().rtx_stl_write(os.fsencode(path), tris.shape[0], tris.ctypes.data))


def _with_point_stats(s, p, d=None, m=None, o=None, cl=None):
    """the rtx_point_stats (and rtx_dark_stats, rtx_premask_stats, rtx_order_stats, rtx_clearlane_stats) counters as
    attributes of the Stats beside them"""
    for f, _ in abi.PointStats._fields_:
        setattr(s, f, getattr(p, f))
    if d is not None:
        for f, _ in abi.DarkStats._fields_:
            setattr(s, f, getattr(d, f))
    if m is not None:
        for f, _ in abi.PremaskStats._fields_:
            setattr(s, f, getattr(m, f))
    if o is not None:
        for f, _ in abi.OrderStats._fields_:
            setattr(s, f, getattr(o, f))
    if cl is not None:
        for f, _ in abi.ClearlaneStats._fields_:
            setattr(s, f, getattr(cl, f))
    return s


class Renderer:
    """One rtx context on one HIP device (rtx_open .. rtx_close)."""

    def __init__(self, device=0):
        self.lib = rtx_lib()
        self._ctx = C.c_void_p()
        _check(self.lib.rtx_open(device, C.byref(self._ctx)))
        self.device = device

    def set_builder(self, builder):
        """rtx_set_builder: abi.RTX_BUILD_SAH_GPU (default), abi.RTX_BUILD_SAH_HOST, abi.RTX_BUILD_LBVH_GPU or
        abi.RTX_BUILD_PLOC_GPU."""
        _check(self.lib.rtx_set_builder(self._ctx, builder))

    def set_option(self, option, value):
        """rtx_set_option: abi.RTX_OPT_* (shadow walk, BVH leaf size, shade-point sort, k_shadow
        slot and grab sizes); build options take effect at the next upload."""
        _check(self.lib.rtx_set_option(self._ctx, option, int(value)))

    def upload(self, scene):
        _check(self.lib.rtx_upload_scene(self._ctx, C.byref(scene.desc)))

    def render(self, frame, params, rgb=None, z=None):
        w, h = frame.width, frame.height
        if rgb is None:
            rgb = np.zeros((h, w, 3), np.float32)
        if z is None:
            z = np.zeros((h, w), np.float32)
        assert rgb.dtype == np.float32 and rgb.flags.c_contiguous and rgb.size == w * h * 3
        assert z.dtype == np.float32 and z.flags.c_contiguous and z.size == w * h
        _check(self.lib.rtx_render(self._ctx, C.byref(frame), C.byref(params), rgb.ctypes.data, z.ctypes.data))
        return rgb, z

    def render_device(self, frame, params, d_rgb, d_z, stream=None):
        """d_rgb / d_z: device pointers (ints), stream: hipStream_t as int or None."""
        _check(self.lib.rtx_render_device(self._ctx, C.byref(frame), C.byref(params), C.c_void_p(d_rgb),
                                          C.c_void_p(d_z), C.c_void_p(stream) if stream else None))

    def postprocess(self, post, rgb, z):
        """rtx_postprocess on host arrays: returns the postprocessed (H,W,3) float32 copy."""
        out = np.ascontiguousarray(rgb, dtype=np.float32).copy()
        zz = np.ascontiguousarray(z, dtype=np.float32)
        h, w = out.shape[:2]
        _check(self.lib.rtx_postprocess(self._ctx, w, h, C.byref(post), out.ctypes.data, zz.ctypes.data))
        return out

    def postprocess_device(self, post, width, height, d_rgb, d_z, stream=None):
        _check(self.lib.rtx_postprocess_device(self._ctx, width, height, C.byref(post), C.c_void_p(d_rgb),
                                               C.c_void_p(d_z), C.c_void_p(stream) if stream else None))

    def wide_tree(self):
        """the uploaded 8-wide tree (rtx_read_wide_tree): (entries uint32 (n, 16), frame float32 (6,))"""
        n = C.c_uint32(0)
        frame = np.zeros(6, np.float32)
        _check(self.lib.rtx_read_wide_tree(self._ctx, None, 0, C.byref(n), frame.ctypes.data))
        ent = np.zeros((n.value, 16), np.uint32)
        if n.value:
            _check(self.lib.rtx_read_wide_tree(self._ctx, ent.ctypes.data, n.value, C.byref(n), frame.ctypes.data))
        return ent, frame

    def bvh2(self):
        """the uploaded BVH2 (rtx_read_bvh2), a dict: nodes uint32 (nnodes, 16) and prims uint32 (nprims, 16), the
        64-byte DNode / DPrim records of csrc/rtx_device.h as words (view as float32 for the boxes), root_ref,
        qnodes uint32 (nq, 4), the threaded 16-bit copy (nq = 0: the context holds none), qframe float32 (6,)"""
        nn, nb, root, nq = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        qframe = np.zeros(6, np.float32)
        _check(self.lib.rtx_read_bvh2(self._ctx, None, 0, C.byref(nn), C.byref(nb), C.byref(root), None, 0, C.byref(nq),
                                      qframe.ctypes.data))
        rec = np.zeros((nn.value + nb.value, 16), np.uint32)
        qn = np.zeros((nq.value, 4), np.uint32)
        if len(rec) or len(qn):
            _check(self.lib.rtx_read_bvh2(self._ctx, rec.ctypes.data, len(rec), C.byref(nn), C.byref(nb), C.byref(root),
                                          qn.ctypes.data, len(qn), C.byref(nq), qframe.ctypes.data))
        return {"nodes": rec[:nn.value], "prims": rec[nn.value:], "root_ref": root.value, "qnodes": qn, "qframe": qframe}

    def stats(self):
        s = Stats()
        _check(self.lib.rtx_get_stats(self._ctx, C.byref(s)))
        p = abi.PointStats()
        _check(self.lib.rtx_get_point_stats(self._ctx, C.byref(p)))
        d = abi.DarkStats()
        _check(self.lib.rtx_get_dark_stats(self._ctx, C.byref(d)))
        m = abi.PremaskStats()
        _check(self.lib.rtx_get_premask_stats(self._ctx, C.byref(m)))
        o = abi.OrderStats()
        _check(self.lib.rtx_get_order_stats(self._ctx, C.byref(o)))
        cl = abi.ClearlaneStats()
        _check(self.lib.rtx_get_clearlane_stats(self._ctx, C.byref(cl)))
        return _with_point_stats(s, p, d, m, o, cl)

    def trace_rays(self, origins, dirs, tmax=None, any_hit=False, reorder=False, count=False):
        """rtx_trace_rays on host arrays: origins / dirs (n, 3), tmax None (unbounded), a scalar or (n,).
        Returns a dict of numpy arrays: t (n,) float32 (0 on a miss), object / material (n,) int32
        (-1 on a miss), outside (n,) uint32, n (n, 3) float32."""
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        if origins.shape != dirs.shape:
            raise ValueError("origins and dirs differ in shape")
        n = origins.shape[0]
        rays = np.zeros(n, abi.RAY_DTYPE)
        rays["origin"] = origins
        rays["dir"] = dirs
        rays["tmax"] = np.inf if tmax is None else np.asarray(tmax, np.float32)
        hits = np.zeros(n, abi.HIT_DTYPE)
        flags = ((abi.RTX_RAYS_ANY_HIT if any_hit else 0) | (abi.RTX_RAYS_REORDER if reorder else 0)
                 | (abi.RTX_RAYS_COUNT if count else 0))
        _check(self.lib.rtx_trace_rays(self._ctx, n, rays.ctypes.data if n else None, hits.ctypes.data if n else None,
                                       flags))
        return {k: hits[k].copy() for k in ("t", "object", "material", "outside", "n")}

    def trace_rays_device(self, n, d_rays, d_hits, flags=0, stream=None):
        """rtx_trace_rays_device: d_rays / d_hits are device pointers (ints, e.g. a torch tensor's
        data_ptr()) to n rtx_ray / rtx_hit records (8 float32 words each); stream: hipStream_t as int or None."""
        _check(self.lib.rtx_trace_rays_device(self._ctx, n, C.c_void_p(d_rays), C.c_void_p(d_hits), flags,
                                              C.c_void_p(stream) if stream else None))

    def frame_rays_device(self, frame, d_rays, stream=None):
        """rtx_frame_rays_device: the frame's width * height primary rays into the device buffer d_rays"""
        _check(self.lib.rtx_frame_rays_device(self._ctx, C.byref(frame), C.c_void_p(d_rays),
                                              C.c_void_p(stream) if stream else None))

    def ray_stats(self):
        s = abi.RayStats()
        _check(self.lib.rtx_get_ray_stats(self._ctx, C.byref(s)))
        return s

    def closest_points(self, points, max_dist=np.inf, bounded_only=False, reorder=False, count=False):
        """rtx_closest_points on host arrays: points (n, 3), max_dist a scalar or (n,) (inf: unbounded).
        Returns a dict of numpy arrays: dist (n,) float32 (inf on a miss), point (n, 3) float32 (0 on a miss),
        object / material (n,) uint32 (abi.RTX_NONE on a miss)."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        n = points.shape[0]
        q = np.zeros(n, abi.POINT_QUERY_DTYPE)
        q["p"] = points
        q["max_dist"] = np.asarray(max_dist, np.float32)
        res = np.zeros(n, abi.CLOSEST_DTYPE)
        flags = ((abi.RTX_CLOSEST_BOUNDED_ONLY if bounded_only else 0) | (abi.RTX_CLOSEST_REORDER if reorder else 0)
                 | (abi.RTX_CLOSEST_COUNT if count else 0))
        _check(self.lib.rtx_closest_points(self._ctx, n, q.ctypes.data if n else None, res.ctypes.data if n else None,
                                           flags))
        return {k: res[k].copy() for k in ("dist", "point", "object", "material")}

    def closest_points_device(self, n, queries_ptr, results_ptr, flags=0, stream=None):
        """rtx_closest_points_device: queries_ptr / results_ptr are device pointers (ints, e.g. a torch tensor's
        data_ptr()) to n rtx_point_query (4 float32 words) / rtx_closest (8 words) records; stream: hipStream_t
        as int or None."""
        _check(self.lib.rtx_closest_points_device(self._ctx, n, C.c_void_p(queries_ptr), C.c_void_p(results_ptr), flags,
                                                  C.c_void_p(stream) if stream else None))

    def closest_stats(self):
        s = abi.ClosestStats()
        _check(self.lib.rtx_get_closest_stats(self._ctx, C.byref(s)))
        return s

    def shadow_rays(self, origins, dirs, dist, light_object=-1, slots=False, count=False):
        """rtx_trace_shadow_rays on host arrays: origins / dirs (n, 3), dist and light_object a scalar or (n,).
        Ray i runs in lane i % 64 of packet i / 64.  Returns a dict of numpy arrays: blocked (n,) bool,
        transmittance (n, 3) float32 ((0, 0, 0) where blocked)."""
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        if origins.shape != dirs.shape:
            raise ValueError("origins and dirs differ in shape")
        n = origins.shape[0]
        rays = np.zeros(n, abi.SHADOW_RAY_DTYPE)
        rays["origin"] = origins
        rays["dir"] = dirs
        rays["dist"] = np.asarray(dist, np.float32)
        rays["light_object"] = np.asarray(light_object, np.int32)
        res = np.zeros(n, abi.SHADOW_RESULT_DTYPE)
        flags = (abi.RTX_SHADOW_RAYS_SLOTS if slots else 0) | (abi.RTX_SHADOW_RAYS_COUNT if count else 0)
        _check(self.lib.rtx_trace_shadow_rays(self._ctx, n, rays.ctypes.data if n else None, res.ctypes.data if n else None,
                                              flags))
        return {"blocked": res["blocked"] != 0, "transmittance": res["transmittance"].copy()}

    def shadow_ray_stats(self):
        s = abi.ShadowRayStats()
        _check(self.lib.rtx_get_shadow_ray_stats(self._ctx, C.byref(s)))
        return s

    def features(self, frame, u32conv=abi.RTX_U32_SAT):
        """rtx_frame_features: the frame's primary-hit feature records, a structured (h, w) array of
        abi.FEATURE_DTYPE (position, z, normal, material, albedo, object)."""
        out = np.zeros((frame.height, frame.width), abi.FEATURE_DTYPE)
        _check(self.lib.rtx_frame_features(self._ctx, C.byref(frame), u32conv, out.ctypes.data))
        return out

    def features_device(self, frame, d_features, u32conv=abi.RTX_U32_SAT, stream=None):
        """rtx_frame_features_device: d_features is a device pointer (int) to width * height rtx_feature
        records (12 float32 words each); stream: hipStream_t as int or None."""
        _check(self.lib.rtx_frame_features_device(self._ctx, C.byref(frame), u32conv, C.c_void_p(d_features),
                                                  C.c_void_p(stream) if stream else None))

    @staticmethod
    def denoise_params(**params):
        """rtx_denoise_params_default plus overrides (iterations, sigma_color / _normal / _albedo / _plane)"""
        p = abi.DenoiseParams()
        rtx_lib().rtx_denoise_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    def denoise(self, rgb, features, **params):
        """rtx_denoise on host arrays: rgb (h, w, 3) float32, features the (h, w) array of features();
        returns the filtered copy."""
        out = np.ascontiguousarray(rgb, dtype=np.float32).copy()
        feat = np.ascontiguousarray(features, dtype=abi.FEATURE_DTYPE)
        h, w = out.shape[:2]
        if feat.shape != (h, w):
            raise ValueError("features and rgb differ in shape")
        p = self.denoise_params(**params)
        _check(self.lib.rtx_denoise(self._ctx, w, h, C.byref(p), feat.ctypes.data, out.ctypes.data))
        return out

    def denoise_device(self, width, height, d_features, d_rgb, stream=None, **params):
        """rtx_denoise_device: d_features / d_rgb are device pointers (ints); d_rgb is filtered in place."""
        p = self.denoise_params(**params)
        _check(self.lib.rtx_denoise_device(self._ctx, width, height, C.byref(p), C.c_void_p(d_features), C.c_void_p(d_rgb),
                                           C.c_void_p(stream) if stream else None))

    @staticmethod
    def denoise_variance_params(**params):
        """rtx_denoise_variance_params_default plus overrides (iterations, sigma_color in standard deviations,
        sigma_normal / _albedo / _plane)"""
        p = abi.DenoiseVarianceParams()
        rtx_lib().rtx_denoise_variance_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    def denoise_variance(self, rgb, variance, features, **params):
        """rtx_denoise_variance on host arrays: rgb and variance (h, w, 3) float32 (the mean and the variance of the
        mean of render_passes / render_adaptive), features the (h, w) array of features(); returns the filtered
        copies (rgb, variance)."""
        out = np.ascontiguousarray(rgb, dtype=np.float32).copy()
        var = np.ascontiguousarray(variance, dtype=np.float32).copy()
        feat = np.ascontiguousarray(features, dtype=abi.FEATURE_DTYPE)
        h, w = out.shape[:2]
        if feat.shape != (h, w) or var.shape != out.shape:
            raise ValueError("features, variance and rgb differ in shape")
        p = self.denoise_variance_params(**params)
        _check(self.lib.rtx_denoise_variance(self._ctx, w, h, C.byref(p), feat.ctypes.data, out.ctypes.data, var.ctypes.data))
        return out, var

    def denoise_variance_device(self, width, height, d_features, d_rgb, d_variance, stream=None, **params):
        """rtx_denoise_variance_device: d_features / d_rgb / d_variance are device pointers (ints); d_rgb and
        d_variance are filtered in place."""
        p = self.denoise_variance_params(**params)
        _check(self.lib.rtx_denoise_variance_device(self._ctx, width, height, C.byref(p), C.c_void_p(d_features),
                                                    C.c_void_p(d_rgb), C.c_void_p(d_variance),
                                                    C.c_void_p(stream) if stream else None))

    def denoise_stats(self):
        s = abi.DenoiseStats()
        _check(self.lib.rtx_get_denoise_stats(self._ctx, C.byref(s)))
        return s

    def render_passes(self, frame, params, passes, jitter=False, aperture=0.0, focus=1.0, target_error=0.0, min_passes=2):
        """rtx_render_passes on host arrays: the frame rendered `passes` times (seed + k; jitter: each pass at its own
        sub-pixel offset; aperture > 0: a thin lens) and combined on the device.  Returns (rgb (h, w, 3) the mean,
        z (h, w) pass 0's, variance (h, w, 3) of the mean); pass_stats() tells how many passes ran."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        w, h = frame.width, frame.height
        rgb, z, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        _check(self.lib.rtx_render_passes(self._ctx, C.byref(frame), C.byref(params), C.byref(pp), rgb.ctypes.data,
                                          z.ctypes.data, var.ctypes.data))
        return rgb, z, var

    def render_passes_device(self, frame, params, passes, d_rgb, d_z, d_variance, stream=None, jitter=False, aperture=0.0,
                             focus=1.0, target_error=0.0, min_passes=2):
        """rtx_render_passes_device: d_rgb / d_z / d_variance are device pointers (ints, 16-byte aligned) or None;
        stream: hipStream_t as int or None."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        _check(self.lib.rtx_render_passes_device(self._ctx, C.byref(frame), C.byref(params), C.byref(pp),
                                                 C.c_void_p(d_rgb) if d_rgb else None, C.c_void_p(d_z) if d_z else None,
                                                 C.c_void_p(d_variance) if d_variance else None,
                                                 C.c_void_p(stream) if stream else None))

    def pass_stats(self):
        s = abi.PassStats()
        _check(self.lib.rtx_get_pass_stats(self._ctx, C.byref(s)))
        return s

    def render_passes_filtered(self, frame, params, passes, filter="gaussian", radius=None, alpha=None, jitter=True,
                               aperture=0.0, focus=1.0, target_error=0.0, min_passes=2):
        """rtx_render_passes_filtered on host arrays: render_passes with every pass gathered through a pixel
        reconstruction filter (a name of abi.FILTER_KINDS, a kind number or a FilterParams; radius / alpha None: the
        library's defaults).  Returns (rgb, z, variance) as render_passes; pass_stats() describes the call."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        fp = _filter_of(filter, radius, alpha)
        w, h = frame.width, frame.height
        rgb, z, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        _check(self.lib.rtx_render_passes_filtered(self._ctx, C.byref(frame), C.byref(params), C.byref(pp), C.byref(fp),
                                                   rgb.ctypes.data, z.ctypes.data, var.ctypes.data))
        return rgb, z, var

    def render_passes_filtered_device(self, frame, params, passes, d_rgb, d_z, d_variance, stream=None, filter="gaussian",
                                      radius=None, alpha=None, jitter=True, aperture=0.0, focus=1.0, target_error=0.0,
                                      min_passes=2):
        """rtx_render_passes_filtered_device: d_rgb / d_z / d_variance are device pointers (ints, 16-byte aligned) or
        None; stream: hipStream_t as int or None."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        fp = _filter_of(filter, radius, alpha)
        _check(self.lib.rtx_render_passes_filtered_device(self._ctx, C.byref(frame), C.byref(params), C.byref(pp), C.byref(fp),
                                                          C.c_void_p(d_rgb) if d_rgb else None, C.c_void_p(d_z) if d_z else None,
                                                          C.c_void_p(d_variance) if d_variance else None,
                                                          C.c_void_p(stream) if stream else None))

    def render_tiles(self, frame, params, tiles, rgb=None, z=None):
        """rtx_render_tiles on host arrays: the listed 8x8 tiles (row-major indices, strictly increasing) of the
        frame into rgb / z (zeros when not given); every other pixel keeps its value.  Returns (rgb, z)."""
        w, h = frame.width, frame.height
        if rgb is None:
            rgb = np.zeros((h, w, 3), np.float32)
        if z is None:
            z = np.zeros((h, w), np.float32)
        assert rgb.dtype == np.float32 and rgb.flags.c_contiguous and rgb.size == w * h * 3
        assert z.dtype == np.float32 and z.flags.c_contiguous and z.size == w * h
        tiles = np.ascontiguousarray(tiles, dtype=np.uint32).ravel()
        _check(self.lib.rtx_render_tiles(self._ctx, C.byref(frame), C.byref(params), tiles.ctypes.data if tiles.size else None,
                                         tiles.size, rgb.ctypes.data, z.ctypes.data))
        return rgb, z

    def render_tiles_device(self, frame, params, d_tiles, n_tiles, d_rgb, d_z, stream=None):
        """rtx_render_tiles_device: d_tiles (n_tiles uint32 tile indices), d_rgb and d_z are device pointers (ints);
        stream: hipStream_t as int or None."""
        _check(self.lib.rtx_render_tiles_device(self._ctx, C.byref(frame), C.byref(params),
                                                C.c_void_p(d_tiles) if d_tiles else None, n_tiles,
                                                C.c_void_p(d_rgb) if d_rgb else None, C.c_void_p(d_z) if d_z else None,
                                                C.c_void_p(stream) if stream else None))

    def render_adaptive(self, frame, params, passes, target_error, min_passes=2, jitter=False, aperture=0.0, focus=1.0):
        """rtx_render_adaptive on host arrays: multi-pass rendering in which a tile stops receiving passes once its
        share of the error budget target_error is met, `passes` at the most.  Returns (rgb (h, w, 3) the mean, z (h, w)
        pass 0's, variance (h, w, 3) of the mean, tile_passes (tiles_y, tiles_x) uint32); adaptive_stats() tells the
        passes run and the final error."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        w, h = frame.width, frame.height
        rgb, z, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        tp = np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint32)
        _check(self.lib.rtx_render_adaptive(self._ctx, C.byref(frame), C.byref(params), C.byref(pp), rgb.ctypes.data,
                                            z.ctypes.data, var.ctypes.data, tp.ctypes.data))
        return rgb, z, var, tp

    def render_adaptive_device(self, frame, params, passes, target_error, d_rgb, d_z, d_variance, d_tile_passes, stream=None,
                               min_passes=2, jitter=False, aperture=0.0, focus=1.0):
        """rtx_render_adaptive_device: d_rgb / d_z / d_variance / d_tile_passes are device pointers (ints, 16-byte
        aligned) or None; stream: hipStream_t as int or None."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        _check(self.lib.rtx_render_adaptive_device(self._ctx, C.byref(frame), C.byref(params), C.byref(pp),
                                                   *[C.c_void_p(d) if d else None for d in (d_rgb, d_z, d_variance, d_tile_passes)],
                                                   C.c_void_p(stream) if stream else None))

    def adaptive_stats(self):
        s = abi.AdaptiveStats()
        _check(self.lib.rtx_get_adaptive_stats(self._ctx, C.byref(s)))
        return s

    def upsample(self, low_rgb, low_features, features, conf=True, **params):
        """rtx_upsample on host arrays: low_rgb (lh, lw, 3) float32 and low_features (lh, lw) of the low frame,
        features (h, w) of the full frame, with lw = ceil(w / scale) and lh = ceil(h / scale).  Returns (rgb (h, w, 3),
        conf (h, w)); conf=False passes no confidence buffer and returns (rgb, None)."""
        low = np.ascontiguousarray(low_rgb, dtype=np.float32)
        lf = np.ascontiguousarray(low_features, dtype=abi.FEATURE_DTYPE)
        feat = np.ascontiguousarray(features, dtype=abi.FEATURE_DTYPE)
        p = upsample_params(**params)
        h, w = feat.shape
        s = int(p.scale)
        if 1 <= s <= abi.RTX_UPSAMPLE_SCALE_MAX and (lf.shape != (-(-h // s), -(-w // s)) or low.shape != lf.shape + (3,)):
            raise ValueError("the low frame is not ceil(w / scale) x ceil(h / scale)")  # another scale: the library refuses
        rgb = np.zeros((h, w, 3), np.float32)
        cf = np.zeros((h, w), np.float32) if conf else None
        _check(self.lib.rtx_upsample(self._ctx, w, h, C.byref(p), low.ctypes.data, lf.ctypes.data, feat.ctypes.data,
                                     rgb.ctypes.data, cf.ctypes.data if conf else None))
        return rgb, cf

    def upsample_device(self, width, height, d_low_rgb, d_low_features, d_features, d_rgb, d_conf, stream=None, **params):
        """rtx_upsample_device: device pointers (ints; the feature buffers 16-byte aligned), d_conf may be None;
        stream: hipStream_t as int or None."""
        p = upsample_params(**params)
        _check(self.lib.rtx_upsample_device(self._ctx, width, height, C.byref(p), C.c_void_p(d_low_rgb),
                                            C.c_void_p(d_low_features), C.c_void_p(d_features), C.c_void_p(d_rgb),
                                            C.c_void_p(d_conf) if d_conf else None, C.c_void_p(stream) if stream else None))

    def upsample_tiles(self, conf, threshold):
        """rtx_upsample_tiles on a host array: the increasing row-major indices (uint32) of the 8x8 tiles of the (h, w)
        confidence buffer that hold a pixel with conf < threshold, as render_tiles takes them."""
        cf = np.ascontiguousarray(conf, dtype=np.float32)
        h, w = cf.shape
        tiles = np.zeros(((h + 7) // 8) * ((w + 7) // 8), np.uint32)
        n = C.c_uint32(0)
        _check(self.lib.rtx_upsample_tiles(self._ctx, w, h, cf.ctypes.data, float(threshold), tiles.ctypes.data, C.byref(n)))
        return tiles[:n.value].copy()

    def upsample_tiles_device(self, width, height, d_conf, threshold, d_tiles, stream=None):
        """rtx_upsample_tiles_device: d_conf / d_tiles are device pointers (ints); returns the list's length."""
        n = C.c_uint32(0)
        _check(self.lib.rtx_upsample_tiles_device(self._ctx, width, height, C.c_void_p(d_conf), float(threshold),
                                                  C.c_void_p(d_tiles), C.byref(n), C.c_void_p(stream) if stream else None))
        return n.value

    def render_upsampled(self, frame, params, **up):
        """rtx_render_upsampled on host arrays: the frame rendered at 1 / scale of the resolution, upsampled under the
        guidance of the full frame's features, and the tiles of confidence below refine_threshold re-rendered at full
        resolution.  Returns (rgb (h, w, 3), z (h, w)); upsample_stats() tells what was refined."""
        p = upsample_params(**up)
        w, h = frame.width, frame.height
        rgb, z = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
        _check(self.lib.rtx_render_upsampled(self._ctx, C.byref(frame), C.byref(params), C.byref(p), rgb.ctypes.data,
                                             z.ctypes.data))
        return rgb, z

    def render_upsampled_device(self, frame, params, d_rgb, d_z, stream=None, **up):
        """rtx_render_upsampled_device: d_rgb / d_z are device pointers (ints, 16-byte aligned) or None."""
        p = upsample_params(**up)
        _check(self.lib.rtx_render_upsampled_device(self._ctx, C.byref(frame), C.byref(params), C.byref(p),
                                                    C.c_void_p(d_rgb) if d_rgb else None, C.c_void_p(d_z) if d_z else None,
                                                    C.c_void_p(stream) if stream else None))

    def upsample_stats(self):
        s = abi.UpsampleStats()
        _check(self.lib.rtx_get_upsample_stats(self._ctx, C.byref(s)))
        return s

    def temporal(self, frame, rgb, variance, features, prev_frame=None, hist_rgb=None, hist_variance=None, hist_length=None,
                 hist_features=None, conf=True, **params):
        """rtx_temporal on host arrays: the current frame's rgb (h, w, 3), variance (the same shape, or None) and
        features (h, w) accumulated into the history (prev_frame, hist_rgb, hist_variance, hist_length (h, w),
        hist_features; all None: the first frame).  Returns (rgb, variance or None, length, conf); conf=False passes no
        confidence buffer and returns None for it."""
        p = temporal_params(**params)
        w, h = frame.width, frame.height

        def arr(a, dtype, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype)
            if a.shape != shape:
                raise ValueError(f"a buffer of shape {a.shape} where the frame needs {shape}")
            return a

        c, vc = arr(rgb, np.float32, (h, w, 3)), arr(variance, np.float32, (h, w, 3))
        f = arr(features, abi.FEATURE_DTYPE, (h, w))
        hc, vh = arr(hist_rgb, np.float32, (h, w, 3)), arr(hist_variance, np.float32, (h, w, 3))
        hl, g = arr(hist_length, np.float32, (h, w)), arr(hist_features, abi.FEATURE_DTYPE, (h, w))
        out = np.zeros((h, w, 3), np.float32)
        out_var = np.zeros((h, w, 3), np.float32) if vc is not None else None
        out_len = np.zeros((h, w), np.float32)
        cf = np.zeros((h, w), np.float32) if conf else None
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        _check(self.lib.rtx_temporal(self._ctx, C.byref(p), C.byref(frame), ptr(c), ptr(vc), ptr(f),
                                     C.byref(prev_frame) if prev_frame is not None else None, ptr(hc), ptr(vh), ptr(hl), ptr(g),
                                     ptr(out), ptr(out_var), ptr(out_len), ptr(cf)))
        return out, out_var, out_len, cf

    def temporal_device(self, frame, d_rgb, d_variance, d_features, prev_frame, d_hist_rgb, d_hist_variance, d_hist_length,
                        d_hist_features, d_out_rgb, d_out_variance, d_out_length, d_out_conf, stream=None, **params):
        """rtx_temporal_device: device pointers (ints; the feature buffers 16-byte aligned) or None where the header
        allows a NULL; stream: hipStream_t as int or None."""
        p = temporal_params(**params)
        vp = lambda d: C.c_void_p(d) if d else None  # noqa: E731
        _check(self.lib.rtx_temporal_device(self._ctx, C.byref(p), C.byref(frame), vp(d_rgb), vp(d_variance), vp(d_features),
                                            C.byref(prev_frame) if prev_frame is not None else None, vp(d_hist_rgb),
                                            vp(d_hist_variance), vp(d_hist_length), vp(d_hist_features), vp(d_out_rgb),
                                            vp(d_out_variance), vp(d_out_length), vp(d_out_conf), vp(stream)))

    def render_temporal(self, frame, params, passes=1, jitter=False, aperture=0.0, focus=1.0, target_error=0.0, min_passes=2,
                        **temporal):
        """rtx_render_temporal on host arrays: render_passes of the frame, its features, and their accumulation into the
        history this context keeps from its last call (vary params.seed from call to call).  Returns (rgb (h, w, 3),
        z (h, w), variance (h, w, 3), length (h, w)); temporal_stats() describes the call."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        tp = temporal_params(**temporal)
        w, h = frame.width, frame.height
        rgb, z, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        length = np.zeros((h, w), np.float32)
        _check(self.lib.rtx_render_temporal(self._ctx, C.byref(frame), C.byref(params), C.byref(pp), C.byref(tp), rgb.ctypes.data,
                                            z.ctypes.data, var.ctypes.data, length.ctypes.data))
        return rgb, z, var, length

    def render_temporal_device(self, frame, params, d_rgb, d_z, d_variance, d_length, stream=None, passes=1, jitter=False,
                               aperture=0.0, focus=1.0, target_error=0.0, min_passes=2, **temporal):
        """rtx_render_temporal_device: d_rgb / d_z / d_variance / d_length are device pointers (ints, 16-byte aligned)
        or None; stream: hipStream_t as int or None."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        tp = temporal_params(**temporal)
        _check(self.lib.rtx_render_temporal_device(self._ctx, C.byref(frame), C.byref(params), C.byref(pp), C.byref(tp),
                                                   *[C.c_void_p(d) if d else None for d in (d_rgb, d_z, d_variance, d_length)],
                                                   C.c_void_p(stream) if stream else None))

    def temporal_reset(self):
        """rtx_temporal_reset: the next render_temporal is a first frame"""
        _check(self.lib.rtx_temporal_reset(self._ctx))

    def temporal_stats(self):
        s = abi.TemporalStats()
        _check(self.lib.rtx_get_temporal_stats(self._ctx, C.byref(s)))
        return s

    @staticmethod
    def _ray_batch(rays_or_origins, dirs, shape):
        """a render_rays / ray_features batch as (records (h * w,) of abi.RAY_DTYPE, h, w, n): the records as given
        with `shape`, else padded with holes to w = min(8 * ceil(n / 8), 1024), h = ceil(n / w)"""
        if dirs is None:
            rays = np.ascontiguousarray(rays_or_origins, dtype=abi.RAY_DTYPE)
            if shape is None and rays.ndim == 2:
                shape = rays.shape
            rays = rays.reshape(-1)
        else:
            origins = np.asarray(rays_or_origins, np.float32).reshape(-1, 3)
            d = np.asarray(dirs, np.float32).reshape(-1, 3)
            if origins.shape != d.shape:
                raise ValueError("origins and dirs differ in shape")
            rays = np.zeros(len(origins), abi.RAY_DTYPE)
            rays["origin"], rays["dir"], rays["tmax"] = origins, d, np.inf
        n = len(rays)
        if n == 0:
            raise ValueError("an empty ray batch")
        if shape is not None:
            h, w = shape
            if h * w != n:
                raise ValueError(f"shape {shape} does not hold {n} rays")
            return rays, h, w, n
        w = min(8 * ((n + 7) // 8), 1024)
        h = (n + w - 1) // w
        padded = np.zeros(h * w, abi.RAY_DTYPE)  # a hole: tmax 0
        padded[:n] = rays
        return padded, h, w, n

    def render_rays(self, rays_or_origins, dirs=None, params=None, shape=None):
        """rtx_render_rays on host arrays: a frame whose primary rays are the caller's.  rays_or_origins: records of
        abi.RAY_DTYPE (tmax <= 0: a hole), or origins (n, 3) with dirs (n, 3) (unbounded rays).  shape=(h, w): the
        batch is that image, returns (rgb (h, w, 3), z (h, w)); a 2-D record array is its own shape.  Without a
        shape the batch is padded with holes and (rgb (n, 3), z (n,)) of the first n pixels come back."""
        rays, h, w, n = self._ray_batch(rays_or_origins, dirs, shape)
        p = default_params() if params is None else params
        rgb, z = np.zeros((h * w, 3), np.float32), np.zeros(h * w, np.float32)
        _check(self.lib.rtx_render_rays(self._ctx, w, h, rays.ctypes.data, C.byref(p), rgb.ctypes.data, z.ctypes.data))
        if shape is not None or (dirs is None and np.ndim(rays_or_origins) == 2):
            return rgb.reshape(h, w, 3), z.reshape(h, w)
        return rgb[:n].copy(), z[:n].copy()

    def render_rays_device(self, width, height, d_rays, params, d_rgb, d_z, stream=None):
        """rtx_render_rays_device: d_rays a device pointer (int, 16-byte aligned) to width * height rtx_ray records,
        d_rgb / d_z device pointers or None; stream: hipStream_t as int or None."""
        _check(self.lib.rtx_render_rays_device(self._ctx, width, height, C.c_void_p(d_rays), C.byref(params),
                                               C.c_void_p(d_rgb) if d_rgb else None, C.c_void_p(d_z) if d_z else None,
                                               C.c_void_p(stream) if stream else None))

    def ray_features(self, rays_or_origins, dirs=None, u32conv=abi.RTX_U32_SAT, shape=None):
        """rtx_ray_features on host arrays: features() of a ray batch (as render_rays takes it), (h, w) records of
        abi.FEATURE_DTYPE, or the first n of a padded batch"""
        rays, h, w, n = self._ray_batch(rays_or_origins, dirs, shape)
        out = np.zeros(h * w, abi.FEATURE_DTYPE)
        _check(self.lib.rtx_ray_features(self._ctx, w, h, rays.ctypes.data, u32conv, out.ctypes.data))
        if shape is not None or (dirs is None and np.ndim(rays_or_origins) == 2):
            return out.reshape(h, w)
        return out[:n].copy()

    def ray_features_device(self, width, height, d_rays, d_features, u32conv=abi.RTX_U32_SAT, stream=None):
        """rtx_ray_features_device: d_rays / d_features are device pointers (ints, 16-byte aligned)"""
        _check(self.lib.rtx_ray_features_device(self._ctx, width, height, C.c_void_p(d_rays), u32conv, C.c_void_p(d_features),
                                                C.c_void_p(stream) if stream else None))

    def projection_rays_device(self, frame, proj, d_rays, stream=None):
        """rtx_projection_rays_device: the projection's width * height rays into the device buffer d_rays"""
        _check(self.lib.rtx_projection_rays_device(self._ctx, C.byref(frame), C.byref(proj), C.c_void_p(d_rays),
                                                   C.c_void_p(stream) if stream else None))

    def projection_rays(self, frame, proj):
        """the projection's rays as the device forms them, an (h, w) array of abi.RAY_DTYPE (a torch tensor holds them
        on the device; in a process that has not used torch yet, call torch.cuda.init() before the first
        Renderer, as bench.py does: torch ships its own HIP runtime)"""
        import torch
        buf = torch.zeros((frame.height * frame.width, 8), dtype=torch.float32, device=f"cuda:{self.device}")
        torch.cuda.synchronize(self.device)
        self.projection_rays_device(frame, proj, buf.data_ptr())
        return buf.cpu().numpy().view(abi.RAY_DTYPE).reshape(frame.height, frame.width)

    def render_projection(self, frame, proj, params):
        """rtx_render_projection on host arrays: (rgb (h, w, 3), z (h, w)) of the frame through projection(...)"""
        w, h = frame.width, frame.height
        rgb, z = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
        _check(self.lib.rtx_render_projection(self._ctx, C.byref(frame), C.byref(proj), C.byref(params), rgb.ctypes.data,
                                              z.ctypes.data))
        return rgb, z

    def render_projection_device(self, frame, proj, params, d_rgb, d_z, stream=None):
        """rtx_render_projection_device: d_rgb / d_z device pointers (ints) or None"""
        _check(self.lib.rtx_render_projection_device(self._ctx, C.byref(frame), C.byref(proj), C.byref(params),
                                                     C.c_void_p(d_rgb) if d_rgb else None, C.c_void_p(d_z) if d_z else None,
                                                     C.c_void_p(stream) if stream else None))

    def close(self):
        if self._ctx:
            self.lib.rtx_close(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pass_params(jitter=None, **params):
    """rtx_pass_params_default plus overrides (passes, flags, aperture, focus, target_error, min_passes); jitter
    sets or clears RTX_PASS_JITTER in flags"""
    p = abi.PassParams()
    rtx_lib().rtx_pass_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    if jitter is not None:
        p.flags = (p.flags | abi.RTX_PASS_JITTER) if jitter else (p.flags & ~abi.RTX_PASS_JITTER)
    return p


def pass_frame(frame, k, **params):
    """rtx_pass_frame (no device needed): the frame of pass k of `frame` under pass_params(**params)"""
    out = Frame()
    _check(rtx_lib().rtx_pass_frame(C.byref(frame), C.byref(pass_params(**params)), k, C.byref(out)))
    return out


def upsample_params(**params):
    """rtx_upsample_params_default plus overrides (scale, match_material, demodulate, sigma_normal / _albedo / _plane,
    albedo_min, refine_threshold)"""
    p = abi.UpsampleParams()
    rtx_lib().rtx_upsample_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def frame_scaled(frame, scale):
    """rtx_frame_scaled (no device needed): the frame of 1 / scale of the resolution per axis whose pixel (c, r) looks
    through the centre of the scale x scale block of `frame`'s pixels it stands for"""
    out = Frame()
    _check(rtx_lib().rtx_frame_scaled(C.byref(frame), scale, C.byref(out)))
    return out


def temporal_params(**params):
    """rtx_temporal_params_default plus overrides (max_history, match_material, sigma_normal / _albedo / _plane)"""
    p = abi.TemporalParams()
    rtx_lib().rtx_temporal_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def frame_project(frame, points):
    """rtx_frame_project (no device needed) of an (..., 3) array of world points, read as float32: (u, v, in_front)
    arrays of the leading shape, u and v float64 in the frame's pixel coordinates, in_front bool"""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.shape[-1:] != (3,):
        raise ValueError("points must have a last axis of 3")
    flat = pts.reshape(-1, 3)
    u, v = np.zeros(len(flat), np.float64), np.zeros(len(flat), np.float64)
    front = np.zeros(len(flat), bool)
    lib = rtx_lib()
    cu, cv, cf = C.c_double(), C.c_double(), C.c_int()
    fptr = C.POINTER(C.c_float)
    for i in range(len(flat)):
        _check(lib.rtx_frame_project(C.byref(frame), flat[i].ctypes.data_as(fptr), C.byref(cu), C.byref(cv), C.byref(cf)))
        u[i], v[i], front[i] = cu.value, cv.value, bool(cf.value)
    return u.reshape(pts.shape[:-1]), v.reshape(pts.shape[:-1]), front.reshape(pts.shape[:-1])


def projection(kind=None, **fields):
    """rtx_projection_default plus overrides (kind: an abi.RTX_PROJ_* or "panorama" / "fisheye" / "ortho"; fov in
    radians, extent, offset_x, offset_y)"""
    p = abi.Projection()
    rtx_lib().rtx_projection_default(C.byref(p))
    if kind is not None:
        p.kind = abi.PROJ_KINDS[kind] if isinstance(kind, str) else kind
    for k, v in fields.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def projection_ray(frame, proj, px, py):
    """rtx_projection_ray (no device needed): pixel (px, py)'s ray, one record of abi.RAY_DTYPE (tmax 0: a hole)"""
    out = np.zeros(1, abi.RAY_DTYPE)
    _check(rtx_lib().rtx_projection_ray(C.byref(frame), C.byref(proj), px, py, out.ctypes.data))
    return out[0]


def filter_params(**params):
    """rtx_filter_params_default plus overrides (kind: a number or a name of abi.FILTER_KINDS, radius, alpha, pad_).
    A kind other than the default's without a radius takes radius 1.5 as well; the library checks the ranges."""
    p = abi.FilterParams()
    rtx_lib().rtx_filter_params_default(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        if k == "kind" and isinstance(v, str):
            if v not in abi.FILTER_KINDS:
                raise ValueError(f"unknown filter {v!r}: one of {sorted(abi.FILTER_KINDS)}")
            v = abi.FILTER_KINDS[v]
        setattr(p, k, v)
    return p


def _filter_of(filter, radius, alpha):
    """a FilterParams as it is, or filter_params of a kind with the radius and alpha that are not None"""
    if isinstance(filter, abi.FilterParams):
        return filter
    kw = {"kind": filter}
    if radius is not None:
        kw["radius"] = radius
    if alpha is not None:
        kw["alpha"] = alpha
    return filter_params(**kw)


def filter_weights(k, filter="gaussian", radius=None, alpha=None, **params):
    """rtx_pass_filter_weights (no device needed): (wx, wy), each RTX_FILTER_TAPS float64, of pass k under
    pass_params(**params) and the filter (as Renderer.render_passes_filtered takes it)"""
    wx, wy = np.zeros(abi.RTX_FILTER_TAPS, np.float64), np.zeros(abi.RTX_FILTER_TAPS, np.float64)
    fp = _filter_of(filter, radius, alpha)
    _check(rtx_lib().rtx_pass_filter_weights(C.byref(pass_params(**params)), C.byref(fp), k, wx.ctypes.data, wy.ctypes.data))
    return wx, wy


def tree_frame(scene):
    """rtx_tree_frame (no device needed): (rotated, R (3, 3), centre (3,), cost ratio) of the frame
    rtx_upload_scene builds the scene's BVHs in under RTX_FRAME_AUTO"""
    rot = np.zeros(9, np.float32)
    cen = np.zeros(3, np.float32)
    flag = C.c_int()
    ratio = C.c_double()
    _check(rtx_lib().rtx_tree_frame(C.byref(scene.desc), C.byref(flag), rot.ctypes.data, cen.ctypes.data, C.byref(ratio)))
    return bool(flag.value), rot.reshape(3, 3), cen, ratio.value


def gpu_kat(kind, records, params=None):
    records = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, abi.KAT_IN[kind])
    out = np.zeros((records.shape[0], abi.KAT_OUT[kind]), np.float32)
    p = params or default_params()
    _check(rtx_lib().rtx_kat(kind, records.shape[0], records.ctypes.data, out.ctypes.data, C.byref(p)))
    return out


def closest_point_object(scene, object_index, P):
    """rtx_closest_point_object, the definition of the closest-point queries, on the host: (dist, cp (3,) float32) of
    object `object_index` of the scene and the point P"""
    if not 0 <= object_index < scene.desc.num_objects:
        raise IndexError("object index out of range")
    p = np.ascontiguousarray(P, dtype=np.float32).reshape(3)
    dist = C.c_float()
    cp = np.zeros(3, np.float32)
    _check(rtx_lib().rtx_closest_point_object(C.addressof(scene.desc.objects[object_index]), p.ctypes.data, C.byref(dist),
                                              cp.ctypes.data))
    return np.float32(dist.value), cp


def closest_kat(objects, object_index, points):
    """rtx_closest_kat: the device's distance functions on (object, point) pairs, no search.  objects: a numpy
    array of rtx_object records (abi.Object's layout); object_index (n,) or None (pair i = object i); points (n, 3).
    Returns (dist (n,), cp (n, 3))."""
    objects = np.ascontiguousarray(objects)
    assert objects.dtype.itemsize == C.sizeof(abi.Object)
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = points.shape[0]
    idx = None if object_index is None else np.ascontiguousarray(object_index, dtype=np.uint32)
    assert idx is None or idx.shape == (n,)
    out = np.zeros((n, 4), np.float32)
    _check(rtx_lib().rtx_closest_kat(len(objects), objects.ctypes.data, n, None if idx is None else idx.ctypes.data,
                                     points.ctypes.data, out.ctypes.data))
    return out[:, 0].copy(), out[:, 1:].copy()


def closest_kat_grid(objects, points):
    """rtx_closest_kat_grid: dist (n_points, n_objects) float32 of every object to every point, on the device"""
    objects = np.ascontiguousarray(objects)
    assert objects.dtype.itemsize == C.sizeof(abi.Object)
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((points.shape[0], len(objects)), np.float32)
    _check(rtx_lib().rtx_closest_kat_grid(len(objects), objects.ctypes.data, points.shape[0], points.ctypes.data,
                                          out.ctypes.data))
    return out


class Group:
    """Several HIP devices rendering one frame (rtx_group_open .. rtx_group_close): tiles dealt
    round-robin over the devices, gathered to the first one over RCCL.  loopback=n: n shards as
    n contexts on device devices[0] (rtx_group_open_loopback, the test transport).  rccl_self:
    one device whose shard still travels through RCCL, to itself (rtx_group_open_rccl_self)."""

    def __init__(self, devices, loopback=None, rccl_self=False):
        self.lib = rtx_lib()
        self._g = C.c_void_p()
        if rccl_self:
            _check(self.lib.rtx_group_open_rccl_self(int(devices[0]), C.byref(self._g)))
            self.devices = [devices[0]]
        elif loopback:
            _check(self.lib.rtx_group_open_loopback(int(loopback), int(devices[0]), C.byref(self._g)))
            self.devices = [devices[0]] * int(loopback)
        else:
            devs = (C.c_int * len(devices))(*devices)
            _check(self.lib.rtx_group_open(len(devices), devs, C.byref(self._g)))
            self.devices = list(devices)

    def set_builder(self, builder):
        _check(self.lib.rtx_group_set_builder(self._g, builder))

    def set_option(self, option, value):
        _check(self.lib.rtx_group_set_option(self._g, option, int(value)))

    def upload(self, scene):
        _check(self.lib.rtx_group_upload_scene(self._g, C.byref(scene.desc)))

    def render(self, frame, params, rgb=None, z=None):
        """the whole frame on the group's first device's host side; rgb / z: optional preallocated
        float32 (H, W, 3) / (H, W) host arrays (pinned ones make the copy faster)"""
        w, h = frame.width, frame.height
        if rgb is None:
            rgb = np.zeros((h, w, 3), np.float32)
        if z is None:
            z = np.zeros((h, w), np.float32)
        assert rgb.dtype == np.float32 and rgb.flags.c_contiguous and rgb.size == w * h * 3
        assert z.dtype == np.float32 and z.flags.c_contiguous and z.size == w * h
        _check(self.lib.rtx_group_render(self._g, C.byref(frame), C.byref(params), rgb.ctypes.data, z.ctypes.data))
        return rgb, z

    def size(self):
        return self.lib.rtx_group_size(self._g)

    def stats(self):
        s = Stats()
        _check(self.lib.rtx_group_get_stats(self._g, C.byref(s)))
        p = abi.PointStats()
        _check(self.lib.rtx_group_get_point_stats(self._g, C.byref(p)))
        d = abi.DarkStats()
        _check(self.lib.rtx_group_get_dark_stats(self._g, C.byref(d)))
        m = abi.PremaskStats()
        _check(self.lib.rtx_group_get_premask_stats(self._g, C.byref(m)))
        o = abi.OrderStats()
        _check(self.lib.rtx_group_get_order_stats(self._g, C.byref(o)))
        cl = abi.ClearlaneStats()
        _check(self.lib.rtx_group_get_clearlane_stats(self._g, C.byref(cl)))
        return _with_point_stats(s, p, d, m, o, cl)

    def device_stats(self, r):
        s = Stats()
        _check(self.lib.rtx_group_device_stats(self._g, r, C.byref(s)))
        p = abi.PointStats()
        _check(self.lib.rtx_group_device_point_stats(self._g, r, C.byref(p)))
        d = abi.DarkStats()
        _check(self.lib.rtx_group_device_dark_stats(self._g, r, C.byref(d)))
        m = abi.PremaskStats()
        _check(self.lib.rtx_group_device_premask_stats(self._g, r, C.byref(m)))
        o = abi.OrderStats()
        _check(self.lib.rtx_group_device_order_stats(self._g, r, C.byref(o)))
        cl = abi.ClearlaneStats()
        _check(self.lib.rtx_group_device_clearlane_stats(self._g, r, C.byref(cl)))
        return _with_point_stats(s, p, d, m, o, cl)

    def render_passes(self, frame, params, passes, jitter=False, aperture=0.0, focus=1.0, target_error=0.0, min_passes=2):
        """rtx_group_render_passes on host arrays, as Renderer.render_passes: (rgb, z, variance); pass_stats() tells how
        many passes ran, exchange_stats() what travelled between the members."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        w, h = frame.width, frame.height
        rgb, z, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        _check(self.lib.rtx_group_render_passes(self._g, C.byref(frame), C.byref(params), C.byref(pp), rgb.ctypes.data,
                                                z.ctypes.data, var.ctypes.data))
        return rgb, z, var

    def pass_stats(self):
        s = abi.PassStats()
        _check(self.lib.rtx_group_get_pass_stats(self._g, C.byref(s)))
        return s

    def render_adaptive(self, frame, params, passes, target_error, min_passes=2, jitter=False, aperture=0.0, focus=1.0):
        """rtx_group_render_adaptive on host arrays, as Renderer.render_adaptive: (rgb, z, variance, tile_passes), the
        single context's bits for any number of members."""
        pp = pass_params(passes=passes, jitter=jitter, aperture=aperture, focus=focus, target_error=target_error,
                         min_passes=min_passes)
        w, h = frame.width, frame.height
        rgb, z, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        tp = np.zeros(((h + 7) // 8, (w + 7) // 8), np.uint32)
        _check(self.lib.rtx_group_render_adaptive(self._g, C.byref(frame), C.byref(params), C.byref(pp), rgb.ctypes.data,
                                                  z.ctypes.data, var.ctypes.data, tp.ctypes.data))
        return rgb, z, var, tp

    def adaptive_stats(self):
        s = abi.AdaptiveStats()
        _check(self.lib.rtx_group_get_adaptive_stats(self._g, C.byref(s)))
        return s

    def exchange_stats(self):
        """rtx_group_get_exchange_stats: exchanges, bytes, exchange_ms and gather_ms of the last multi-pass render"""
        s = abi.GroupExchangeStats()
        _check(self.lib.rtx_group_get_exchange_stats(self._g, C.byref(s)))
        return s

    def member(self, r):
        """what the runtime reports about member r (rtx_group_member_info): its device, its RCCL
        communicator's count / rank / device, peer access to and from member 0, PCI bus id"""
        m = abi.GroupMember()
        _check(self.lib.rtx_group_member_info(self._g, r, C.byref(m)))
        return {"device": m.device, "comm_count": m.comm_count, "comm_rank": m.comm_rank, "comm_device": m.comm_device,
                "can_access_peer0": m.can_access_peer0, "peer0_can_access": m.peer0_can_access,
                "peer_enabled": m.peer_enabled, "transport": m.transport, "pci_bus_id": m.pci_bus_id.decode()}

    def close(self):
        if self._g:
            self.lib.rtx_group_close(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tile_pack(rgb, z, offset, stride):
    """rtx_tile_pack_host: the shard's (N, 4) float32 tile records {r, g, b, z}."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    z = np.ascontiguousarray(z, dtype=np.float32)
    h, w = z.shape
    lib = rtx_lib()
    n = lib.rtx_tile_pack_count(w, h, offset, stride)
    out = np.zeros((n, 4), np.float32)
    _check(lib.rtx_tile_pack_host(rgb.ctypes.data, z.ctypes.data, w, h, offset, stride, out.ctypes.data))
    return out


def tile_unpack(records, rgb, z, offset, stride):
    """rtx_tile_unpack_host: writes the shard's pixels of records into rgb / z in place."""
    records = np.ascontiguousarray(records, dtype=np.float32)
    assert rgb.dtype == np.float32 and rgb.flags.c_contiguous and z.dtype == np.float32 and z.flags.c_contiguous
    h, w = z.shape
    _check(rtx_lib().rtx_tile_unpack_host(records.ctypes.data, w, h, offset, stride, rgb.ctypes.data, z.ctypes.data))


def pass_pack(rgb, z, variance, offset, stride):
    """rtx_pass_pack_host: the shard's (N, 8) float32 pass records {mean r, g, b, z, var r, g, b, 0}."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    z = np.ascontiguousarray(z, dtype=np.float32)
    variance = np.ascontiguousarray(variance, dtype=np.float32)
    h, w = z.shape
    lib = rtx_lib()
    n = lib.rtx_tile_pack_count(w, h, offset, stride)
    out = np.zeros((n, 8), np.float32)
    _check(lib.rtx_pass_pack_host(rgb.ctypes.data, z.ctypes.data, variance.ctypes.data, w, h, offset, stride, out.ctypes.data))
    return out


def pass_unpack(records, shape, offset, stride, rgb=None, z=None, variance=None):
    """rtx_pass_unpack_host: writes the shard's pixels of records into rgb / z / variance in place, each float32 of a
    frame of shape (h, w) or None."""
    records = np.ascontiguousarray(records, dtype=np.float32)
    h, w = shape
    for a, words in ((rgb, 3), (z, 1), (variance, 3)):
        assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.size == w * h * words)
    _check(rtx_lib().rtx_pass_unpack_host(records.ctypes.data, w, h, offset, stride, *[a.ctypes.data if a is not None else None
                                                                                          for a in (rgb, z, variance)]))
