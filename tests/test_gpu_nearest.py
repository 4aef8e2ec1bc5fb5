"""Closest-point queries (rtx_closest_points*) on the device, bit for bit.

Arithmetic: the device's known-answer entry of the three distance functions equals the host's
rtx_closest_point_object on (object, point) pairs of every fixture scene.  Search: per scene the known-answer
entry gives the distance of every object to every point of the families of nearest_model.py, which depends on no
tree; the query must return the minimum's bits, an object that attains them, that object's closest point and its
material.  A subtree pruned with the answer in it is what these tests exist to find.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import hard_meshes as HM
import nearest_model as NM
import rays_exhaustive as RX
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

U32 = np.uint32
SCENES = tuple(HM.SCENES) + tuple(RX.ROTATION)
NONE = abi.RTX_NONE
# (builder, shadow walk, tree frame, BVH leaf size): the device-collapsed 8-wide tree (the float BVH2 on the scenes too
# small for one); the host-collapsed one, which leaves the emitters out; the float BVH2 with leaves of several primitives
CONFIGS = {"auto": (abi.RTX_BUILD_SAH_GPU, abi.RTX_WALK_AUTO, abi.RTX_FRAME_AUTO, 1),
           "host": (abi.RTX_BUILD_SAH_HOST, abi.RTX_WALK_W8, abi.RTX_FRAME_AUTO, 1),
           "bvh2": (abi.RTX_BUILD_SAH_GPU, abi.RTX_WALK_BVH2, abi.RTX_FRAME_WORLD, 4)}


class Gpu:
    def __init__(self, tmp):
        self.paths = NM.scene_paths(tmp)
        self.res = {}
        self.renderer = rtxpy.Renderer(0)
        self.uploaded = None

    def get(self, name):
        """(scene, records, points, rows of each family, least KAT dist per point over all objects, over the bounded)"""
        if name not in self.res:
            path, load = self.paths[name]
            scene = load(path)
            objs = RX.objects_of(scene)
            fams = NM.search_families(objs)
            rows, at = {}, 0
            for f, v in fams.items():
                rows[f] = slice(at, at + len(v))
                at += len(v)
            P = np.concatenate(list(fams.values()))
            bounded = HM.is_bounded(objs)
            dmin, dmin_b = np.zeros(len(P), np.float32), np.full(len(P), np.inf, np.float32)
            for s in rows.values():
                if s.stop > s.start:
                    D = rtxpy.closest_kat_grid(objs, P[s])
                    dmin[s] = D.min(1)
                    if bounded.any():
                        dmin_b[s] = D[:, bounded].min(1)
            self.res[name] = (scene, objs, P, rows, dmin, dmin_b)
        return self.res[name]

    def upload(self, name, config="auto"):
        r = self.renderer
        if self.uploaded != (name, config):
            builder, walk, frame, leaf = CONFIGS[config]
            r.set_builder(builder)
            r.set_option(abi.RTX_OPT_SHADOW_WALK, walk)
            r.set_option(abi.RTX_OPT_TREE_FRAME, frame)
            r.set_option(abi.RTX_OPT_BVH_LEAF, leaf)
            r.upload(self.get(name)[0])
            self.uploaded = (name, config)
        return r

    def close(self):
        self.renderer.close()
        for s in self.res.values():
            s[0].close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    g = Gpu(tmp_path_factory.mktemp("nearest_gpu"))
    yield g
    g.close()


def raw(r, P, max_dist=np.inf, flags=0):
    """rtx_closest_points on host buffers: the whole rtx_closest records"""
    P = np.asarray(P, np.float32).reshape(-1, 3)
    q = np.zeros(len(P), abi.POINT_QUERY_DTYPE)
    q["p"], q["max_dist"] = P, np.asarray(max_dist, np.float32)
    res = np.full(len(P), 0x7B, np.uint8).repeat(32).view(abi.CLOSEST_DTYPE) if len(P) else np.zeros(0, abi.CLOSEST_DTYPE)
    rc = r.lib.rtx_closest_points(r._ctx, len(P), q.ctypes.data if len(P) else None, res.ctypes.data if len(P) else None, flags)
    assert rc == abi.RTX_OK, (rc, r.lib.rtx_last_error())
    return q, res


def rows_of(bad, rows):
    return {f: int(np.count_nonzero((bad >= s.start) & (bad < s.stop))) for f, s in rows.items() if s.stop > s.start}


def is_miss(res):
    return ((res["dist"] == np.inf) & (res["object"] == NONE) & (res["material"] == NONE) & (res["point"] == 0).all(1)
            & (res["pad"] == 0).all(1))


def check_answers(objs, P, rows, want, res, what):
    """every record of res against the per-object known answers: want = the least dist per point (inf: none)"""
    assert (res["pad"] == 0).all(), what
    bad = np.nonzero(res["dist"].view(U32) != want.view(U32))[0]
    assert not len(bad), (what, "dist differs on", len(bad), rows_of(bad, rows), bad[:6], res["dist"][bad[:6]], want[bad[:6]])
    none = want == np.inf
    assert is_miss(res[none]).all(), what
    hit = np.nonzero(~none)[0]
    obj = res["object"][hit]
    assert (obj < len(objs)).all(), what
    kd, kcp = rtxpy.closest_kat(objs, obj, P[hit])
    ok = kd.view(U32) == want[hit].view(U32)
    assert ok.all(), (what, "the object's own dist is not the minimum on", int((~ok).sum()), hit[~ok][:6])
    ok = (kcp.view(U32) == res["point"][hit].view(U32)).all(1)
    assert ok.all(), (what, "point is not the object's closest point on", int((~ok).sum()), hit[~ok][:6])
    assert (res["material"][hit] == objs["material"][obj].astype(U32)).all(), what


# ---- arithmetic ----
@pytest.mark.parametrize("name", SCENES)
def test_device_functions_equal_the_host_definition(gpu, name):
    _, objs, *_ = gpu.get(name)
    idx, P = NM.pairs_of(objs)
    assert len(idx) >= 700
    d, cp = NM.host(objs, idx, P)
    kd, kcp = rtxpy.closest_kat(objs, idx, P)
    bad = np.nonzero((kd.view(U32) != d.view(U32)) | (kcp.view(U32) != cp.view(U32)).any(1))[0]
    assert not len(bad), (name, len(bad), idx[bad[:6]], P[bad[:6]], kd[bad[:6]], d[bad[:6]])


def test_device_functions_cover_every_type_by_the_thousands(gpu):
    n = {abi.RTX_SPHERE: 0, abi.RTX_TRIANGLE: 0, abi.RTX_PLANE: 0}
    for name in SCENES:
        _, objs, *_ = gpu.get(name)
        idx, _ = NM.pairs_of(objs)
        for t in n:
            n[t] += int((objs["type"][idx] == t).sum())
    assert min(n.values()) >= 2000, n


def test_grid_entry_is_the_pair_entry(gpu):
    _, objs, P, *_ = gpu.get("mixed")
    D = rtxpy.closest_kat_grid(objs, P[:64])
    rs = np.random.RandomState(3)
    p, o = rs.randint(64, size=500), rs.randint(len(objs), size=500)
    kd, _ = rtxpy.closest_kat(objs, o, P[p])
    assert (D[p, o].view(U32) == kd.view(U32)).all()


# ---- search ----
@pytest.mark.parametrize("name", SCENES)
def test_search_equals_brute_force(gpu, name):
    _, objs, P, rows, dmin, dmin_b = gpu.get(name)
    nb = int(HM.is_bounded(objs).sum())
    for f in ("inbox", "far60", "far2000") + (("surface", "ties") if nb else ()):
        assert rows[f].stop - rows[f].start == NM.N_POINTS, (name, f)
    for config in CONFIGS:
        r = gpu.upload(name, config)
        _, res = raw(r, P)
        check_answers(objs, P, rows, dmin, res, (name, config))
        st = r.closest_stats()
        assert st.points == len(P) and st.found == len(P)
        assert st.far_points >= (2 * NM.N_POINTS if nb else 0)
        _, res = raw(r, P, flags=abi.RTX_CLOSEST_BOUNDED_ONLY)
        check_answers(objs, P, rows, dmin_b, res, (name, config, "bounded only"))
        assert r.closest_stats().found == (len(P) if nb else 0)


def test_bounded_only_on_a_scene_of_planes_alone_misses(gpu):
    _, objs, P, rows, dmin, dmin_b = gpu.get("count0")
    assert not HM.is_bounded(objs).any() and len(P) == 3 * NM.N_POINTS
    _, res = raw(gpu.upload("count0"), P, flags=abi.RTX_CLOSEST_BOUNDED_ONLY)
    assert is_miss(res).all()


# ---- edge cases ----
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1025))
def test_batch_sizes(gpu, n):
    _, objs, P, rows, dmin, _ = gpu.get("world")
    pick = np.random.RandomState(n).permutation(len(P))[:n]
    r = gpu.upload("world")
    _, res = raw(r, P[pick])
    assert len(res) == n and (res["dist"].view(U32) == dmin[pick].view(U32)).all()
    assert r.closest_stats().points == n and r.closest_stats().found == n


def test_order_reverse_and_reorder_give_the_same_dist(gpu):
    _, objs, P, rows, dmin, _ = gpu.get("rotated")
    r = gpu.upload("rotated")
    _, rev = raw(r, P[::-1])
    assert (rev["dist"][::-1].view(U32) == dmin.view(U32)).all()
    _, srt = raw(r, P, flags=abi.RTX_CLOSEST_REORDER)
    check_answers(objs, P, rows, dmin, srt, "reorder")
    assert r.closest_stats().sort_ms > 0


def test_host_buffers_equal_a_torch_tensor(gpu):
    import torch
    _, objs, P, rows, dmin, _ = gpu.get("world")
    r = gpu.upload("world")
    n = len(P) - 3
    q, res = raw(r, P[:n])
    d_q = torch.from_numpy(q.view(np.float32).reshape(-1, 4)).cuda()
    d_res = torch.full((n + 2, 8), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.closest_points_device(n, d_q.data_ptr(), d_res.data_ptr(), 0)
    got = d_res.cpu().numpy()
    assert (got[n:] == -7.0).all()
    assert got[:n].tobytes() == res.tobytes()
    out = r.closest_points(P[:n])
    assert out["dist"].tobytes() == res["dist"].tobytes() and out["object"].tobytes() == res["object"].tobytes()
    assert out["point"].tobytes() == res["point"].tobytes() and out["material"].tobytes() == res["material"].tobytes()


def test_max_dist(gpu):
    _, objs, P, rows, dmin, _ = gpu.get("world")
    r = gpu.upload("world")
    s = rows["inbox"]
    p, d = P[s][:512], dmin[s][:512]
    assert (d > 0).all()
    _, res = raw(r, p, max_dist=d)
    assert is_miss(res).all()                                   # the answer's own dist excludes it
    _, res = raw(r, p, max_dist=np.nextafter(d, np.float32(np.inf)))
    assert (res["dist"].view(U32) == d.view(U32)).all()          # the next float above keeps it
    for md in (0.0, -1.0, -np.inf):
        _, res = raw(r, p, max_dist=md)
        assert is_miss(res).all(), md
    for md in (np.nan, np.inf):
        _, res = raw(r, p, max_dist=md)
        assert (res["dist"].view(U32) == d.view(U32)).all(), md
    # a bound between two objects' distances never lets a farther object answer
    _, res = raw(r, p, max_dist=np.float32(2.0) * d)
    assert (res["dist"].view(U32) == d.view(U32)).all()


def test_points_that_are_not_finite_miss(gpu):
    _, objs, P, rows, dmin, _ = gpu.get("mixed")
    r = gpu.upload("mixed")
    p = P[:192].copy()
    p[0::3, 0], p[1::3, 1], p[2::3, 2] = np.nan, np.inf, -np.inf
    p[5] = P[5]
    _, res = raw(r, p)
    keep = np.zeros(len(p), bool)
    keep[5] = True
    assert is_miss(res[~keep]).all() and res["dist"][5].view(U32) == dmin[5].view(U32)
    assert r.closest_stats().found == 1


def test_argument_errors(gpu):
    import torch
    r = gpu.upload("mixed")
    lib, ctx = r.lib, r._ctx
    q, res = abi.PointQuery(), abi.Closest()
    assert lib.rtx_closest_points(ctx, 1, ctypes.byref(q), ctypes.byref(res), 8) == abi.RTX_ERR_ARG
    assert b"flags" in lib.rtx_last_error()
    assert lib.rtx_closest_points(ctx, abi.RTX_RAYS_MAX + 1, ctypes.byref(q), ctypes.byref(res), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points(ctx, 1, None, ctypes.byref(res), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points(ctx, 1, ctypes.byref(q), None, 0) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points_device(ctx, 1, None, None, 0, None) == abi.RTX_ERR_ARG
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert lib.rtx_closest_points_device(ctx, 1, t.data_ptr() + 4, t.data_ptr() + 64, 0, None) == abi.RTX_ERR_ARG
    assert lib.rtx_closest_points_device(ctx, 1, t.data_ptr(), t.data_ptr() + 72, 0, None) == abi.RTX_ERR_ARG
    assert b"aligned" in lib.rtx_last_error()
    assert lib.rtx_closest_points(ctx, 0, None, None, 0) == abi.RTX_OK
    fresh = rtxpy.Renderer(0)
    try:
        assert lib.rtx_closest_points(fresh._ctx, 1, ctypes.byref(q), ctypes.byref(res), 0) == abi.RTX_ERR_STATE
        assert lib.rtx_closest_points(fresh._ctx, 0, None, None, 0) == abi.RTX_ERR_STATE
    finally:
        fresh.close()


def test_a_render_is_the_same_before_and_after_a_query(gpu):
    scene, objs, P, *_ = gpu.get("mixed")
    r = gpu.upload("mixed")
    frame = scene.frame(64, 48)
    params = rtxpy.default_params(rng=abi.RTX_RNG_CONST)
    rgb0, z0 = r.render(frame, params)
    st0 = r.stats()
    raw(r, P, flags=abi.RTX_CLOSEST_REORDER | abi.RTX_CLOSEST_COUNT)
    assert r.stats().closest_rays == st0.closest_rays and r.stats().shadow_rays == st0.shadow_rays
    rgb1, z1 = r.render(frame, params)
    assert rgb0.tobytes() == rgb1.tobytes() and z0.tobytes() == z1.tobytes() and (z0 > 0).any()


# ---- pruning actually happens ----
def test_the_search_prunes(gpu):
    _, objs, P, rows, dmin, _ = gpu.get("world")
    r = gpu.upload("world")
    p = P[rows["surface"]]
    nb = int(HM.is_bounded(objs).sum())
    _, res = raw(r, p, flags=abi.RTX_CLOSEST_COUNT)
    a = r.closest_stats()
    assert (res["dist"].view(U32) == dmin[rows["surface"]].view(U32)).all()
    tests = a.tri_tests + a.sphere_tests
    print("world, on-surface points: %d node visits and %d primitive tests for %d points, %.4f %% of points x bounded objects"
          % (a.node_visits, tests, len(p), 100.0 * tests / (len(p) * nb)))
    assert a.points == len(p) and a.plane_tests == 2 * len(p) and a.node_visits >= len(p)
    assert 0 < tests <= 0.25 * len(p) * nb
    raw(r, p[::-1], flags=abi.RTX_CLOSEST_COUNT)
    b = r.closest_stats()
    assert (a.node_visits, a.tri_tests, a.sphere_tests, a.plane_tests, a.far_points, a.found) == \
           (b.node_visits, b.tri_tests, b.sphere_tests, b.plane_tests, b.far_points, b.found)
    raw(r, p)
    c = r.closest_stats()  # without RTX_CLOSEST_COUNT the traversal counters stay 0
    assert (c.node_visits, c.tri_tests, c.sphere_tests, c.plane_tests) == (0, 0, 0, 0) and c.found == len(p)
