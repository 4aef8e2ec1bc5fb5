"""k_shadow's shadow query, ray by ray, against a brute-force reference.

rtx_trace_shadow_rays runs shadow_query (csrc/rtx_shadow.hip) itself: the planes, the objects tested
one by one, the 8-wide any-hit walk with its octant instances, scalar steps, LDS top levels, lane
stack and spills, deferred transparent-leaf queue and two-leaf rounds, the threaded BVH2 walk, the
fast intersectors, far rays walked from the light end.  For about ten thousand rays per context
(shadow_exhaustive.py: real light packets, incoherent and degenerate rays, rays through a dozen
transparent surfaces, rays from 60 radii, idle lanes, and all of them mixed in one batch) the blocked
flag must equal, and an unblocked ray's transmittance must equal bit for bit, what the device's own
any-hit tests (rtx_kat) say over every candidate object: no tolerance, no excluded ray.  The
transmittances are powers of two, so a test dropped or made twice changes the bits.

The far-sphere exception of DESIGN §7.3 never applies here: the families hold no far ray that grazes
a sphere, and the tests assert that no accepted (far ray, sphere) pair lacks float64's voucher.
"""
import ctypes

import numpy as np
import pytest

import rays_exhaustive as RX
import shadow_exhaustive as SX
import rtxpy
from rtxpy import abi

pytestmark = pytest.mark.gpu

U32 = np.uint32
WALKS = {"w8": abi.RTX_WALK_W8, "bvh2": abi.RTX_WALK_BVH2, "auto": abi.RTX_WALK_AUTO}
BUILDERS = {"sahhost": abi.RTX_BUILD_SAH_HOST, "lbvh": abi.RTX_BUILD_LBVH_GPU, "ploc": abi.RTX_BUILD_PLOC_GPU,
            "sahgpu": abi.RTX_BUILD_SAH_GPU}
BASE = ["%s-%s-%s" % (s, v, w) for s in ("glass", "mixed", "trionly") for v in SX.VARIANTS for w in ("w8", "bvh2")]
CONFIGS = {c: dict(scene=c.split("-")[0], variant=c.split("-")[1], walk=c.split("-")[2]) for c in BASE}
CONFIGS.update({"mixed-world-w8-" + b: dict(scene="mixed", variant="world", walk="w8", builder=v) for b, v in BUILDERS.items()})
CONFIGS.update({"mixed-world-%s-leaf4" % w: dict(scene="mixed", variant="world", walk=w, leaf=4) for w in ("w8", "bvh2")})
CONFIGS["mixed-rotated-w8-frameworld"] = dict(scene="mixed", variant="rotated", walk="w8", frame=abi.RTX_FRAME_WORLD)
CONFIGS.update({"%s-world-w8-lds1" % s: dict(scene=s, variant="world", walk="w8", lds=1) for s in ("glass", "mixed")})
CONFIGS.update({"tiny-%s-%s" % (v, w): dict(scene="tiny", variant=v, walk=w) for v in SX.VARIANTS for w in ("auto", "w8", "bvh2")})


class Gpu:
    def __init__(self, tmp):
        self.paths = SX.write_scenes(tmp)
        self.scenes, self.objs, self.mats, self.fams, self.mix, self.data, self.ctx, self.got = {}, {}, {}, {}, {}, {}, {}, {}

    def scene(self, key):
        if key not in self.scenes:
            self.scenes[key] = RX.load(self.paths[key])
            self.objs[key] = RX.objects_of(self.scenes[key])
            self.mats[key] = SX.Mats(self.scenes[key], self.objs[key])
            self.fams[key] = SX.families(self.objs[key], key[1], key[0])
            self.mix[key] = SX.mixed(self.fams[key])
        return self.scenes[key]

    def rays(self, key, fam):
        self.scene(key)
        return self.mix[key][0] if fam == "mixed" else self.fams[key][fam]

    def get(self, key, fam):
        """a family's expected answers in a scene (the device's own decisions on its candidate pairs)"""
        if (key, fam) not in self.data:
            r = self.rays(key, fam)
            self.data[key, fam] = SX.Data(self.objs[key], self.mats[key], r, rtxpy.gpu_kat)
        return self.data[key, fam]

    def renderer(self, cfg):
        if cfg not in self.ctx:
            c = CONFIGS[cfg]
            r = rtxpy.Renderer(0)
            if "builder" in c:
                r.set_builder(c["builder"])
            r.set_option(abi.RTX_OPT_SHADOW_WALK, WALKS[c["walk"]])
            if "leaf" in c:
                r.set_option(abi.RTX_OPT_BVH_LEAF, c["leaf"])
            if "frame" in c:
                r.set_option(abi.RTX_OPT_TREE_FRAME, c["frame"])
            if "lds" in c:
                r.set_option(abi.RTX_OPT_SHADOW_LDS_STACK, c["lds"])
            r.upload(self.scene(key_of(cfg)))
            self.ctx[cfg] = r
        return self.ctx[cfg]

    def far(self, cfg, o):
        key = key_of(cfg)
        return RX.far_mask(self.scene(key), self.objs[key], o, frame_world=CONFIGS[cfg].get("frame") == abi.RTX_FRAME_WORLD)

    def query(self, cfg, fam, **kw):
        r = self.rays(key_of(cfg), fam)
        return self.renderer(cfg).shadow_rays(r.o, r.d, r.dist, r.light, **kw)

    def plain(self, cfg, fam):
        """a family's plain query (no flags) in a context, made once"""
        if (cfg, fam) not in self.got:
            self.got[cfg, fam] = self.query(cfg, fam)
        return self.got[cfg, fam]

    def close(self):
        for r in self.ctx.values():
            r.close()
        for s in self.scenes.values():
            s.close()


def key_of(cfg):
    return CONFIGS[cfg]["scene"], CONFIGS[cfg]["variant"]


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    g = Gpu(tmp_path_factory.mktemp("shadow_exhaustive_gpu"))
    yield g
    g.close()


def check(D, got, what):
    """exact: the flag on every ray, the transmittance's bits on every unblocked ray, zeros on a blocked one"""
    b, tm = got["blocked"], got["transmittance"]
    wrong = np.nonzero(b != D.blocked)[0]
    assert not len(wrong), (what, "blocked differs on", len(wrong), wrong[:8], D.blocked[wrong[:8]], D.expo[wrong[:8]])
    bits = (tm.view(U32) != D.tm.view(U32)).any(1)
    wrong = np.nonzero(bits)[0]
    assert not len(wrong), (what, "transmittance differs on", len(wrong), wrong[:8], tm[wrong[:8]], D.tm[wrong[:8]])


# ---- 1. exact answers ----
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_shadow_query_equals_brute_force(gpu, cfg):
    c = CONFIGS[cfg]
    key = key_of(cfg)
    r = gpu.renderer(cfg)  # (never rendered: the lane-stack size and the spill area are the query's own)
    st = r.stats()
    want_walk = {"w8": abi.RTX_WALK_W8, "bvh2": abi.RTX_WALK_BVH2, "auto": abi.RTX_WALK_LINEAR}[c["walk"]]
    assert st.shadow_walk == want_walk, (st.shadow_walk, want_walk)
    if "frame" in c:
        assert st.tree_rotated == 0
    w8 = want_walk == abi.RTX_WALK_W8
    rays = exempt = 0
    blocked = []
    top = 0
    for fam in SX.FAMILIES + ("mixed",):
        D = gpu.get(key, fam)
        far = gpu.far(cfg, D.rays.o) & ~D.rays.idle
        if fam == "far60":
            assert far.all()
        elif fam != "mixed":
            assert not far.any()
        ex = D.exempt(far)
        assert ex == 0, (fam, ex)  # no pair that matters falls under the far-sphere exception
        exempt += ex
        check(D, gpu.plain(cfg, fam), (cfg, fam))
        if w8:
            check(D, gpu.query(cfg, fam, slots=True), (cfg, fam, "slots"))
        rays += D.rays.n
        blocked.append(D.blocked)
        top = max(top, int(D.expo.max()))
    # the counting instance on the mixed batch: the same answers, and the spill path known to have run or not
    D = gpu.get(key, "mixed")
    check(D, gpu.query(cfg, "mixed", count=True), (cfg, "mixed", "count"))
    rs = r.shadow_ray_stats()
    assert rs.rays == int((~D.rays.idle).sum()) and rs.blocked == int(D.blocked.sum())
    if w8:
        check(D, gpu.query(cfg, "mixed", count=True, slots=True), (cfg, "mixed", "count slots"))
        assert r.shadow_ray_stats().stack_spills == rs.stack_spills
        if c.get("lds") == 1:
            assert rs.stack_spills > 0
        elif st.wide_depth <= 8 + 1:  # RTX_W8_STACK entries in LDS, one group in a register
            assert rs.stack_spills == 0
        assert rs.box_tests > 0 and rs.tri_tests > 0
        if c["scene"] != "tiny":  # (a tiny scene's tree is a root with leaves)
            assert rs.leaf_rounds > 0 and rs.uniform_steps > 0 and rs.far_rays > 0
        assert (rs.sphere_tests > 0) == (c["scene"] != "trionly")
    elif want_walk == abi.RTX_WALK_BVH2:
        assert rs.box_tests > 0 and rs.tri_tests > 0 and rs.stack_spills == 0 and rs.far_rays > 0
    else:
        assert rs.box_tests == 0 and rs.stack_spills == 0
    print(cfg, "rays", rays, "blocked share %.4f" % float(np.concatenate(blocked).mean()), "max exponent", top, "spills",
          rs.stack_spills, "far-exempt pairs", exempt, "| wide depth", st.wide_depth, "far rays walked", rs.far_rays, "uniform steps",
          rs.uniform_steps, "of", rs.wave_steps)


# ---- 2. batch independence ----
@pytest.mark.parametrize("cfg", BASE)
def test_mixed_batch_returns_each_family_its_bits(gpu, cfg):
    key = key_of(cfg)
    gpu.scene(key)
    perm = gpu.mix[key][1]
    want = {k: np.concatenate([gpu.plain(cfg, f)[k] for f in SX.FAMILIES])[perm] for k in ("blocked", "transmittance")}
    for kw in (dict(), dict(count=True)) + ((dict(slots=True),) if CONFIGS[cfg]["walk"] == "w8" else ()):
        got = gpu.query(cfg, "mixed", **kw)
        assert np.array_equal(got["blocked"], want["blocked"]), (cfg, kw)
        assert np.array_equal(got["transmittance"].view(U32), want["transmittance"].view(U32)), (cfg, kw)
    for f in ("light", "through"):  # the counting instance on whole families too
        got = gpu.query(cfg, f, count=True)
        assert all(np.array_equal(got[k].view(np.uint8), gpu.plain(cfg, f)[k].view(np.uint8)) for k in got), (cfg, f)


# ---- 3. the emitter skip ----
@pytest.mark.parametrize("cfg", BASE + ["tiny-world-auto", "tiny-world-w8", "tiny-world-bvh2"])
def test_light_packets_without_the_emitter_skip(gpu, cfg):
    key = key_of(cfg)
    with_skip = gpu.get(key, "light")
    r = with_skip.rays.without_light()
    D = SX.Data(gpu.objs[key], gpu.mats[key], r, rtxpy.gpu_kat, with_skip.P)
    assert r.target_far.sum() >= 64 and D.blocked[r.target_far].all()  # the emitter itself now blocks them
    assert not with_skip.blocked[r.target_far].all()
    got = gpu.renderer(cfg).shadow_rays(r.o, r.d, r.dist, -1)
    check(D, got, (cfg, "light, no skip"))
    print(cfg, "light family: blocked with the skip", int(with_skip.blocked.sum()), "without", int(D.blocked.sum()), "of", r.n)


# ---- 4. idle lanes, short batches, errors ----
@pytest.mark.parametrize("cfg", ["mixed-world-w8", "mixed-rotated-bvh2", "tiny-world-auto"])
def test_idle_lanes_and_short_batches(gpu, cfg):
    key = key_of(cfg)
    D = gpu.get(key, "idle")
    r = D.rays
    assert r.idle.sum() >= r.n // 4 and (~r.idle).sum() >= r.n // 4
    got = gpu.plain(cfg, "idle")
    assert not got["blocked"][r.idle].any() and (got["transmittance"][r.idle] == 1).all()
    ren = gpu.renderer(cfg)
    for fam in ("idle", "surface"):
        full, fr = gpu.plain(cfg, fam), gpu.rays(key, fam)
        for n in SX.IDLE_SIZES:
            part = ren.shadow_rays(fr.o[:n], fr.d[:n], fr.dist[:n], fr.light[:n])
            assert all(np.array_equal(part[k].view(np.uint8), full[k][:n].view(np.uint8)) for k in part), (cfg, fam, n)
            assert ren.shadow_ray_stats().rays == int((~fr.idle[:n]).sum())


def test_error_codes(gpu):
    lib = rtxpy.rtx_lib()
    ray, res = abi.ShadowRay(), abi.ShadowResult()
    fresh = rtxpy.Renderer(0)
    try:
        assert lib.rtx_trace_shadow_rays(fresh._ctx, 1, ctypes.byref(ray), ctypes.byref(res), 0) == abi.RTX_ERR_STATE
        assert lib.rtx_trace_shadow_rays(fresh._ctx, 0, None, None, 0) == abi.RTX_ERR_STATE
    finally:
        fresh.close()
    r = gpu.renderer("mixed-world-w8")
    assert lib.rtx_trace_shadow_rays(r._ctx, 1, ctypes.byref(ray), ctypes.byref(res), 4) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_shadow_rays(r._ctx, 1, None, ctypes.byref(res), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_shadow_rays(r._ctx, 1, ctypes.byref(ray), None, 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_shadow_rays(r._ctx, abi.RTX_RAYS_MAX + 1, ctypes.byref(ray), ctypes.byref(res), 0) == abi.RTX_ERR_ARG
    assert lib.rtx_trace_shadow_rays(r._ctx, 0, None, None, 0) == abi.RTX_OK
    assert r.shadow_ray_stats().rays == 0
    assert lib.rtx_trace_shadow_rays(r._ctx, 1, ctypes.byref(ray), ctypes.byref(res), 0) == abi.RTX_OK  # dist 0: idle
    assert res.blocked == 0 and list(res.transmittance) == [1.0, 1.0, 1.0] and r.shadow_ray_stats().rays == 0


# ---- 5. the tie to the render ----
COUNTERS = [f for f, t in abi.Stats._fields_ if t in (ctypes.c_uint64, ctypes.c_uint32) and not f.startswith("pad")]


def test_queries_leave_the_render_alone(gpu):
    key = ("mixed", "world")
    scene = gpu.scene(key)
    r = rtxpy.Renderer(0)  # the shipped options: 8-wide walk, culls, point masks and dark samples on
    try:
        r.upload(scene)
        frame, params = scene.frame(24, 16), rtxpy.default_params(count_traversal=1)
        assert params.gi == abi.RTX_GI_AMBIENT
        rgb0, z0 = r.render(frame, params)
        s0 = r.stats()
        assert s0.shadow_walk == abi.RTX_WALK_W8 and s0.shadow_rays > 0
        for fam in ("mixed", "light"):
            fr = gpu.rays(key, fam)
            for kw in (dict(), dict(slots=True, count=True)):
                check(gpu.get(key, fam), r.shadow_rays(fr.o, fr.d, fr.dist, fr.light, **kw), ("after a render", fam, kw))
        s1 = r.stats()
        assert s1.shadow_rays == s0.shadow_rays  # a query is no render
        rgb1, z1 = r.render(frame, params)
        s2 = r.stats()
        assert np.array_equal(rgb0.view(U32), rgb1.view(U32)) and np.array_equal(z0.view(U32), z1.view(U32))
        diff = [f for f in COUNTERS if getattr(s0, f) != getattr(s2, f)]
        assert not diff, diff
    finally:
        r.close()


# ---- 6. the fused triangle test accepts nothing the candidate filter drops ----
@pytest.mark.parametrize("variant", SX.VARIANTS)
def test_filter_loses_no_device_acceptance(gpu, variant):
    """the CPU half shows it for the oracle's exact any-hit test; the device's any_tri is the fused fast form"""
    key = ("mixed", variant)
    gpu.scene(key)
    objs = gpu.objs[key]
    bounded = np.nonzero(objs["type"] != abi.RTX_PLANE)[0]
    lost = pairs = 0
    for fam in SX.FAMILIES:
        D = gpu.get(key, fam)
        r = D.rays
        rows = np.nonzero(~r.idle)[0][:64]
        pr, po = np.repeat(rows, len(bounded)), np.tile(bounded, len(rows))
        hit = RX.any_pairs(rtxpy.gpu_kat, objs, r.o, r.d, r.dist, pr, po)
        accepted = set((pr[hit].astype(np.int64) * len(objs) + po[hit]).tolist())
        lost += len(accepted - set((D.P.pr.astype(np.int64) * len(objs) + D.P.po).tolist()))
        pairs += len(accepted)
    print(key, "device acceptances over every object", pairs, "outside the candidates", lost)
    assert pairs > 0 and lost == 0
