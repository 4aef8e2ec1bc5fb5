"""Ray queries (rtx_trace_rays*, k_rays in csrc/rtx_trace_rays.h) on the GPU.

A frame is an origin plus a grid of targets, so the same pencil of rays can be traced three ways:
by the renderer (its z buffer), by a closest query of rtx_frame_rays_device's rays, and by the
oracle's primary pass.  The query must equal the first bit for bit and the third within the
suite's own z tolerances (conftest.compare_const).
"""
import ctypes

import numpy as np
import pytest

import rays_frames as RF
import rtxpy
from rays_exhaustive import objects_of
from rtxpy import abi

pytestmark = pytest.mark.gpu

W, H, N = RF.W, RF.H, RF.W * RF.H
SENTINEL = 123456.0


def as_hits(t):
    """a torch (n, 8) float32 device tensor of rtx_hit records as a numpy structured array"""
    return t.cpu().numpy().view(abi.HIT_DTYPE).reshape(-1)


class World:
    """scenes, contexts (one per scene and closest-hit walk), frame rays and their closest hits,
    each made once and shared by the tests (none of them changes a shared array)"""

    def __init__(self):
        self.scenes, self.ctx, self.q, self.z = {}, {}, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = RF.load_scene(name)
        return self.scenes[name]

    def frames(self, name):
        return RF.frames_of(name, self.scene(name))

    def renderer(self, name, walk=abi.RTX_WALK_AUTO):
        if (name, walk) not in self.ctx:
            r = rtxpy.Renderer(0)
            r.set_option(abi.RTX_OPT_TRACE_WALK, walk)
            r.upload(self.scene(name))
            self.ctx[name, walk] = r
        return self.ctx[name, walk]

    def query(self, name, key, walk=abi.RTX_WALK_AUTO, renderer=None):
        """(rays (N, 8) float32, hits structured (N,)) of a frame: rtx_frame_rays_device, then a closest query"""
        import torch
        if renderer is None and (name, key, walk) in self.q:
            return self.q[name, key, walk]
        r = renderer or self.renderer(name, walk)
        d_rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
        d_hits = torch.full((N, 8), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # torch filled them on its stream, the context works on its own
        r.frame_rays_device(self.frames(name)[key], d_rays.data_ptr())
        r.trace_rays_device(N, d_rays.data_ptr(), d_hits.data_ptr(), 0)
        out = (d_rays.cpu().numpy(), as_hits(d_hits))
        if renderer is None:
            self.q[name, key, walk] = out
        return out

    def render_z(self, name, key, walk=abi.RTX_WALK_AUTO):
        if (name, key, walk) not in self.z:
            self.z[name, key, walk] = self.renderer(name, walk).render(self.frames(name)[key], rtxpy.default_params())[1]
        return self.z[name, key, walk]

    def close(self):
        for r in self.ctx.values():
            r.close()
        for s in self.scenes.values():
            s.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


# ---- 1. equals the renderer, bit for bit ----
WALKS = [("scene1", abi.RTX_WALK_AUTO), ("scene4", abi.RTX_WALK_AUTO), ("scene5", abi.RTX_WALK_AUTO),
         ("scene6", abi.RTX_WALK_AUTO), ("scene4", abi.RTX_WALK_BVH2), ("scene5", abi.RTX_WALK_BVH2)]


@pytest.mark.parametrize("name,walk", WALKS)
def test_closest_query_equals_render_z(world, name, walk):
    z = world.render_z(name, "camera", walk)
    if name != "scene1":  # (a scene of a few objects may have no 8-wide tree)
        st = world.renderer(name, walk).stats()
        assert st.trace_walk == (abi.RTX_WALK_BVH2 if walk == abi.RTX_WALK_BVH2 else abi.RTX_WALK_W8)
    rays, hits = world.query(name, "camera", walk)
    assert np.isinf(rays[:, 3]).all() and (rays[:, 7] == 0).all()
    assert np.abs(np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(hits["t"].reshape(H, W), z), int((hits["t"].reshape(H, W) != z).sum())
    assert ((hits["t"] > 0) == (hits["object"] >= 0)).all()


@pytest.mark.parametrize("walk", [abi.RTX_WALK_AUTO, abi.RTX_WALK_BVH2])
def test_query_before_any_render_sizes_its_own_overflow_stack(world, walk):
    """scene5's stand-in (BVH2 deeper than the LDS lane stack) queried in a fresh context that has
    never rendered: the HBM overflow stack is the query's own"""
    z = world.render_z("scene5", "camera", walk)
    r = rtxpy.Renderer(0)
    try:
        r.set_option(abi.RTX_OPT_TRACE_WALK, walk)
        r.upload(world.scene("scene5"))
        assert r.stats().bvh_depth + 1 > 9  # RTX_TRACE_LSTK: the deeper entries live in HBM
        _, hits = world.query("scene5", "camera", walk, renderer=r)
    finally:
        r.close()
    assert np.array_equal(hits["t"].reshape(H, W), z)


# ---- 2. against the oracle ----
CASES = [(n, k) for n in sorted(RF.SCENE_FILES) for k in ("camera", "inside_a", "inside_b")] + [("scene5", "far60")]


@pytest.fixture(scope="module")
def oracle_primary(world):
    from rtxpy import oracle
    cache = {}

    def get(name, key):
        if (name, key) not in cache:
            cache[name, key] = oracle.primary(world.scene(name), world.frames(name)[key])
        return cache[name, key]
    return get


@pytest.mark.parametrize("name,key", CASES)
def test_closest_query_against_oracle(world, oracle_primary, name, key):
    ref_z, ref_obj = oracle_primary(name, key)
    _, hits = world.query(name, key)
    t, obj = hits["t"].reshape(H, W), hits["object"].reshape(H, W)
    hit, ref_hit = t > 0, ref_z > 0
    assert ref_hit.mean() >= 0.25
    mism = float((hit != ref_hit).mean())
    both = hit & ref_hit
    rel = np.abs(t - ref_z) / np.maximum(ref_z, 1.0)
    ok = float((rel[both] <= 1e-4).mean())
    same = both & (t.view(np.uint32) == ref_z.view(np.uint32))
    print(name, key, "hit mismatch", mism, "t ok", ok, "bit-equal", float(same.mean()), "max rel", float(rel[both].max()))
    assert mism <= 1e-4 + 1.0 / t.size
    assert ok >= 0.999
    assert same.any() and (obj[same] == ref_obj[same]).all(), int((obj[same] != ref_obj[same]).sum())
    if key == "far60":
        assert (t[hit] > 200).all()


# ---- 3. packet edges ----
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_packet_edges(world, n):
    import torch
    rays, full = world.query("scene4", "camera")
    r = world.renderer("scene4")
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.full((N, 8), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.trace_rays_device(n, d_rays.data_ptr(), d_hits.data_ptr(), 0)
    got = d_hits.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    assert got[:n].tobytes() == full[:n].tobytes()
    assert r.ray_stats().rays == n and r.ray_stats().hits == np.count_nonzero(full["t"][:n])


@pytest.mark.parametrize("queues,grab", [(1, 1), (3, 5), (8, 64)])
def test_packet_queues_and_grabs_give_the_same_hits(world, queues, grab):
    """RTX_OPT_RAYS_QUEUES / RTX_OPT_RAYS_GRAB only change which wave takes a packet: every ray is
    traced once, none past n, for one queue, a count that does not divide the grid, and grabs
    longer than a queue's share"""
    import torch
    rays, full = world.query("scene4", "camera")
    r = world.renderer("scene4")
    d_rays = torch.from_numpy(rays).cuda()
    try:
        r.set_option(abi.RTX_OPT_RAYS_QUEUES, queues)
        r.set_option(abi.RTX_OPT_RAYS_GRAB, grab)
        for n in (N - 7, 64 * 3 + 1):
            d_hits = torch.full((N, 8), SENTINEL, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r.trace_rays_device(n, d_rays.data_ptr(), d_hits.data_ptr(), 0)
            got = d_hits.cpu().numpy()
            assert (got[n:] == SENTINEL).all() and got[:n].tobytes() == full[:n].tobytes()
    finally:
        r.set_option(abi.RTX_OPT_RAYS_QUEUES, 0)
        r.set_option(abi.RTX_OPT_RAYS_GRAB, 0)
    with pytest.raises(rtxpy.RtxError):
        r.set_option(abi.RTX_OPT_RAYS_QUEUES, 9)
    with pytest.raises(rtxpy.RtxError):
        r.set_option(abi.RTX_OPT_RAYS_GRAB, 65)


# ---- 4. mixed origins, order independence, reorder ----
def kat_t(objs, o, d, index):
    """the t bits object `index`'s own device intersector returns for ray (o, d) (rtx_kat), None on a miss"""
    ob = objs[index]
    if ob["type"] == abi.RTX_TRIANGLE:
        kind, rec = abi.KAT_MOLLER, np.concatenate([o, d, ob["p0"], ob["e1"], ob["e2"], [ob["epsilon"]]])
    elif ob["type"] == abi.RTX_SPHERE:
        kind, rec = abi.KAT_SPHERE, np.concatenate([o, d, ob["p0"], [ob["radius"], ob["epsilon"]]])
    else:
        kind, rec = abi.KAT_PLANE, np.concatenate([o, d, ob["n"], [ob["d"], ob["epsilon"]]])
    out = rtxpy.gpu_kat(kind, rec.astype(np.float32))[0]
    return out[1:2].view(np.uint32)[0] if out[0] else None


def test_mixed_origins_order_independence_and_reorder(world):
    import torch
    name, keys = "scene5", ("camera", "inside_a", "inside_b")
    per = [world.query(name, k) for k in keys]
    rays = np.concatenate([p[0] for p in per])
    want = np.concatenate([p[1] for p in per])
    perm = np.random.RandomState(20240611).permutation(len(rays))
    r = world.renderer(name)
    d_rays = torch.from_numpy(rays[perm]).cuda()
    objs = objects_of(world.scene(name))
    for flags in (0, abi.RTX_RAYS_REORDER):
        d_hits = torch.full((len(rays), 8), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.trace_rays_device(len(rays), d_rays.data_ptr(), d_hits.data_ptr(), flags)
        got = as_hits(d_hits)
        st = r.ray_stats()
        assert st.rays == len(rays) and st.hits == np.count_nonzero(want["t"])
        assert (st.sort_ms > 0) == bool(flags) and st.kernel_ms > 0
        assert np.array_equal(got["t"].view(np.uint32), want["t"][perm].view(np.uint32)), flags
        diff = np.nonzero(got["object"] != want["object"][perm])[0]
        print("flags", flags, "object differs on", len(diff), "of", len(rays))
        assert len(diff) <= 64
        for i in diff:  # only exact ties: both objects' own intersectors return the reported t
            o, d = rays[perm][i, 0:3], rays[perm][i, 4:7]
            tb = got["t"][i:i + 1].view(np.uint32)[0]
            assert kat_t(objs, o, d, got["object"][i]) == tb and kat_t(objs, o, d, want["object"][perm][i]) == tb, i
        same = got["object"] == want["object"][perm]
        assert got[same].tobytes() == want[perm][same].tobytes()


# ---- 5. tmax and any-hit ----
@pytest.mark.parametrize("name,walk", [("scene1", abi.RTX_WALK_AUTO), ("scene5", abi.RTX_WALK_AUTO),
                                       ("scene5", abi.RTX_WALK_BVH2)])
def test_tmax_and_any_hit(world, name, walk):
    r = world.renderer(name, walk)
    rays = np.concatenate([world.query(name, k, walk)[0] for k in ("camera", "inside_a")])
    full = np.concatenate([world.query(name, k, walk)[1] for k in ("camera", "inside_a")])
    o, d, tc = rays[:, 0:3], rays[:, 4:7], full["t"]
    hit = tc > 0
    assert 0.25 < hit.mean() and (name != "scene1" or hit.mean() < 1.0)
    again = r.trace_rays(o, d)
    assert all(np.array_equal(again[k], full[k]) for k in again)
    half = r.trace_rays(o, d, tmax=np.where(hit, np.float32(0.5) * tc, np.float32(np.inf)))
    assert (half["t"] == 0).all() and (half["object"] == -1).all() and (half["material"] == -1).all()
    assert (half["outside"] == 0).all() and (half["n"] == 0).all()
    twice = r.trace_rays(o, d, tmax=np.where(hit, np.float32(2) * tc, np.float32(np.inf)))
    assert all(np.array_equal(twice[k], full[k]) for k in twice)
    exact = r.trace_rays(o, d, tmax=np.where(hit, tc, np.float32(np.inf)))  # hits need t < tmax, strictly
    assert (exact["t"] == 0).all()
    rs = np.random.RandomState(7)
    tmax = np.where(hit, tc * rs.uniform(0.2, 3.0, len(tc)), rs.uniform(0.1, 50.0, len(tc))).astype(np.float32)
    for reorder in (False, True):
        any_ = r.trace_rays(o, d, tmax=tmax, any_hit=True, reorder=reorder)
        expect = hit & (tc < tmax)
        assert 0.1 < expect.mean() < 0.9
        assert np.array_equal(any_["t"] > 0, expect), int(((any_["t"] > 0) != expect).sum())
        assert np.array_equal(any_["object"] >= 0, expect)
        assert (any_["t"][expect] >= tc[expect]).all() and (any_["t"][expect] < tmax[expect]).all()
    dn = d.copy()
    dn[::3, 1] = np.nan
    nan = r.trace_rays(o, dn)
    assert (nan["t"][::3] == 0).all() and (nan["object"][::3] == -1).all()
    keep = np.ones(len(tc), bool)
    keep[::3] = False
    assert all(np.array_equal(nan[k][keep], full[k][keep]) for k in nan)


# ---- 6. hit record ----
@pytest.mark.parametrize("name", ["scene1", "scene4"])
def test_hit_record(world, name):
    objs = objects_of(world.scene(name))
    seen = set()
    for key in ("camera", "inside_a", "inside_b"):
        rays, hits = world.query(name, key)
        m = hits["t"] > 0
        o, d, h = rays[m, 0:3], rays[m, 4:7], hits[m]
        ob = objs[h["object"]]
        assert np.array_equal(h["material"], ob["material"])
        b = h["n"][:, 0] * d[:, 0] + h["n"][:, 1] * d[:, 1] + h["n"][:, 2] * d[:, 2]  # dot3's float32 order
        assert b.dtype == np.float32 and np.array_equal(h["outside"], np.signbit(b).astype(np.uint32))
        sph, tri, pln = (ob["type"] == k for k in (abi.RTX_SPHERE, abi.RTX_TRIANGLE, abi.RTX_PLANE))
        p = d[sph] * h["t"][sph, None] + o[sph]
        n_sph = (p - ob["p0"][sph]) * (np.float32(1) / ob["radius"][sph, None])
        assert sph.sum() == 0 or np.abs(h["n"][sph] - n_sph).max() <= 1e-6
        for flat in (tri, pln):
            same = (h["n"][flat] == ob["n"][flat]).all(axis=1)
            flipped = (h["n"][flat] == -ob["n"][flat]).all(axis=1)
            assert (same | flipped).all()
        assert (h["outside"][pln] == 1).all()  # a plane's normal is turned to face the ray
        seen |= {int(k) for k in np.unique(ob["type"])}
        miss = hits[~m]
        assert (miss["object"] == -1).all() and (miss["material"] == -1).all() and (miss["n"] == 0).all()
    assert seen == ({abi.RTX_SPHERE, abi.RTX_PLANE} if name == "scene1" else {abi.RTX_SPHERE, abi.RTX_TRIANGLE, abi.RTX_PLANE})


# ---- 7. errors and isolation ----
def test_errors(world):
    lib = rtxpy.rtx_lib()
    ray, hit = abi.Ray(), abi.Hit()
    r = rtxpy.Renderer(0)
    try:
        assert lib.rtx_trace_rays(r._ctx, 1, ctypes.byref(ray), ctypes.byref(hit), 0) == abi.RTX_ERR_STATE
        with pytest.raises(rtxpy.RtxError) as e:
            r.trace_rays(np.zeros((1, 3)), np.ones((1, 3)))
        assert e.value.code == abi.RTX_ERR_STATE
    finally:
        r.close()
    r = world.renderer("scene1")
    assert lib.rtx_trace_rays(r._ctx, 1, ctypes.byref(ray), ctypes.byref(hit), 8) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays(r._ctx, 1, None, ctypes.byref(hit), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays(r._ctx, 1, ctypes.byref(ray), None, 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays(r._ctx, abi.RTX_RAYS_MAX + 1, ctypes.byref(ray), ctypes.byref(hit), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays_device(r._ctx, 1, None, None, 0, None) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_rays(r._ctx, 0, None, None, 0) == abi.RTX_OK
    assert r.ray_stats().rays == 0


def test_query_between_renders_leaves_the_render_alone(world):
    name = "scene5"
    r = world.renderer(name)
    frame = world.frames(name)["camera"]
    params = rtxpy.default_params()
    rgb0, z0 = r.render(frame, params)
    s0 = r.stats()
    rays = np.concatenate([world.query(name, k)[0] for k in ("camera", "inside_a", "inside_b")])  # a larger grid than the render's
    got = r.trace_rays(rays[:, 0:3], rays[:, 4:7], reorder=True, count=True)
    rs = r.ray_stats()
    assert rs.rays == len(rays) and rs.hits == np.count_nonzero(got["t"]) and rs.node_visits > 0
    assert rs.tri_tests > 0 and rs.plane_tests > 0 and rs.far_rays == 0
    s1 = r.stats()
    assert (s1.closest_rays, s1.shadow_rays, s1.shade_points, s1.kernel_ms) == (s0.closest_rays, s0.shadow_rays, s0.shade_points, s0.kernel_ms)
    rgb1, z1 = r.render(frame, params)
    s2 = r.stats()
    assert np.array_equal(rgb0, rgb1) and np.array_equal(z0, z1)
    assert (s2.closest_rays, s2.shadow_rays, s2.shade_points, s2.chunks) == (s0.closest_rays, s0.shadow_rays, s0.shade_points, s0.chunks)


def test_count_flag_fills_the_far_counter(world):
    rays, hits = world.query("scene5", "far60")
    r = world.renderer("scene5")
    got = r.trace_rays(rays[:, 0:3], rays[:, 4:7], count=True)
    assert np.array_equal(got["t"], hits["t"])
    rs = r.ray_stats()
    assert rs.rays == N and rs.hits == np.count_nonzero(hits["t"]) and rs.far_rays == N and rs.node_visits > 0


# ---- 8. torch path ----
def test_torch_tensors_on_a_side_stream(world):
    import torch
    name = "scene4"
    r = world.renderer(name)
    rays, want = world.query(name, "inside_b")
    host = r.trace_rays(rays[:, 0:3], rays[:, 4:7], tmax=rays[:, 3])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_rays = torch.from_numpy(rays).cuda()
        d_hits = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
        r.trace_rays_device(N, d_rays.data_ptr(), d_hits.data_ptr(), abi.RTX_RAYS_REORDER, s.cuda_stream)
        t = d_hits[:, 0].clone()
    s.synchronize()
    got = as_hits(d_hits)
    assert got.tobytes() == want.tobytes()
    assert all(np.array_equal(host[k], got[k]) for k in host)
    assert np.array_equal(t.cpu().numpy(), want["t"])
