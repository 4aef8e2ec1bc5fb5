/*
 * A scene flattened and its BVHs built (replaces accel_init, accel.c:266-315): materials, planes
 * and emitters into device records, the BVH2 from either builder, the shadow walk's tree.
 * rtx_upload.cpp puts the result on a device.
 */
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "bvh_build.h"
#include "rtx.h"
#include "rtx_device.h"
#include "rtx_frame.h"
#include "rtx_quant.h"
#include "rtx_internal.h"

/* DQNode preorder of the subtree at device ref `ref` (rtx_device.h): the node itself with the
 * box it has in its parent, then its left and right subtrees.  An inner node's link is the
 * index after its subtree (subtree sizes from `size`, filled by thread_sizes); a leaf keeps
 * its device ref. */
static uint32_t thread_sizes(const std::vector<DNode> &recs, uint32_t ref, std::vector<uint32_t> &size)
{
	if (ref & RTX_REF_LEAF)
		return 1;
	const uint32_t i = (ref & RTX_REF_OFF) / (uint32_t)sizeof(DNode);
	const DNode &n = recs[i];
	size[i] = 1 + thread_sizes(recs, n.ref0, size) + thread_sizes(recs, n.ref1, size);
	return size[i];
}


/* one plane pair quantised conservatively (rtx_quant.h) */
static uint32_t quantise(float lo, float hi, float qo, float qs) { return rtx_quantise(lo, hi, qo, qs); }

static void thread_emit(const std::vector<DNode> &recs, const std::vector<uint32_t> &size, const QFrame &F,
			uint32_t ref, const float lo[3], const float hi[3], std::vector<DQNode> &out, uint32_t dep,
			std::vector<uint32_t> &depth)
{
	DQNode t;
	t.x = quantise(lo[0], hi[0], F.qo[0], F.qs[0]);
	t.y = quantise(lo[1], hi[1], F.qo[1], F.qs[1]);
	t.z = quantise(lo[2], hi[2], F.qo[2], F.qs[2]);
	const uint32_t me = (uint32_t)out.size();
	if (ref & RTX_REF_LEAF) {
		t.link = ref;
		out.push_back(t);
		depth.push_back(dep);
		return;
	}
	const uint32_t i = (ref & RTX_REF_OFF) / (uint32_t)sizeof(DNode);
	t.link = (me + size[i]) << 6;
	out.push_back(t);
	depth.push_back(dep);
	const DNode &n = recs[i];
	const float l0[3] = { n.lo0x, n.lo0y, n.lo0z }, h0[3] = { n.hi0x, n.hi0y, n.hi0z };
	const float l1[3] = { n.lo1x, n.lo1y, n.lo1z }, h1[3] = { n.hi1x, n.hi1y, n.hi1z };
	thread_emit(recs, size, F, n.ref0, l0, h0, out, dep + 1, depth);
	thread_emit(recs, size, F, n.ref1, l1, h1, out, dep + 1, depth);
}

/* the quantised threaded BVH and its frame: the bounded objects' box, 65533 steps per axis */
static void thread_bvh(const std::vector<DNode> &inner, uint32_t root_ref, const float lo[3], const float hi[3],
		       std::vector<DQNode> &out, QFrame &F, std::vector<uint32_t> &depth)
{
	out.clear();
	depth.clear();
	float ext_max = 0.f;
	for (int a = 0; a < 3; a++)
		ext_max = std::max(ext_max, hi[a] - lo[a]);
	for (int a = 0; a < 3; a++) {
		F.qo[a] = lo[a];
		const float ext = std::max(hi[a] - lo[a], std::max(ext_max, 1.f) * 1e-6f);
		F.qs[a] = 65533.f / ext;
	}
	if (root_ref == RTX_EMPTY_REF)
		return;
	std::vector<uint32_t> size(inner.size(), 0);
	const uint32_t total = thread_sizes(inner, root_ref, size);
	out.reserve(total);
	thread_emit(inner, size, F, root_ref, lo, hi, out, 0, depth);
}

/* the LDS copy of the threaded BVH's top levels (rtx_device.h RTX_QTOP_CUT): every node
 * shallower than the deepest cut that keeps at most RTX_TOP_MAX records */
static uint32_t thread_top(const std::vector<DQNode> &q, const std::vector<uint32_t> &depth, std::vector<uint32_t> &top)
{
	top.clear();
	if (q.empty())
		return 0;
	std::vector<size_t> hist(66, 0);
	for (uint32_t dj : depth)
		hist[std::min<uint32_t>(dj, 65)]++;
	uint32_t D = 1; /* the top = nodes of depth < D */
	size_t cnt = hist[0];
	while (D < 65 && hist[D] && cnt + hist[D] <= RTX_TOP_MAX) {
		cnt += hist[D];
		D++;
	}
	std::vector<uint32_t> id(q.size(), RTX_NONE);
	uint32_t nt = 0;
	for (size_t j = 0; j < q.size(); j++)
		if (depth[j] < D)
			id[j] = nt++;
	top.assign(5 * (size_t)nt, 0);
	for (size_t j = 0; j < q.size(); j++) {
		if (id[j] == RTX_NONE)
			continue;
		uint32_t *T = &top[4 * (size_t)id[j]];
		T[0] = q[j].x;
		T[1] = q[j].y;
		T[2] = q[j].z;
		const uint32_t link = q[j].link;
		if (link & RTX_REF_LEAF) {
			T[3] = link;
		} else if (depth[j] == D - 1) {
			T[3] = (((uint32_t)j + 1) << 6) | RTX_QTOP_CUT;
			top[4 * (size_t)nt + id[j]] = link >> 6;
		} else {
			/* the node after an above-cut subtree is a sibling's or an ancestor's: in the top */
			const uint32_t e = link >> 6;
			T[3] = (e < q.size() ? id[e] : nt) << 6;
		}
	}
	return nt;
}

/* what the steps of rtx_build_scene hand on to one another */
namespace {
struct SceneBuild {
	const rtx_scene_desc *sc = nullptr;
	std::vector<DMaterial> mats;
	std::vector<DPlane> planes;
	std::vector<uint32_t> bounded; /* the objects the trees hold: spheres and triangles */
	std::vector<DEmitter> emit;
	std::vector<float> lo, hi;     /* the bounded objects' leaf boxes, for the builders */
	float tlo[3], thi[3];          /* their union in the trees' frame */
	BvhConfig cfg;
	bool want_w8 = false;          /* the shadow walk takes the 8-wide tree */
	uint32_t nnodes = 0, root_ref = RTX_EMPTY_REF, depth = 0;
	std::vector<DNode> inner;          /* host copy of the inner-node records (threaded BVH2, host collapse) */
	std::vector<DPrim> prims_dl;       /* device builders: the primitive records read back (host collapse) */
	const DPrim *host_prims = nullptr; /* the primitive records in leaf order on the host */
};
}

static int flatten_materials(const rtx_scene_desc *sc, std::vector<DMaterial> &mats)
{
	if (sc->num_materials > RTX_META_MAT)
		return fail(RTX_ERR_SCENE, "too many materials (%u)", sc->num_materials);
	mats = std::vector<DMaterial>(sc->num_materials);
	for (uint32_t i = 0; i < sc->num_materials; i++) {
		const rtx_material &m = sc->materials[i];
		DMaterial &d = mats[i];
		memset(&d, 0, sizeof(d));
		memcpy(d.ks, m.ks, 12);
		memcpy(d.ka, m.ka, 12);
		memcpy(d.kr, m.kr, 12);
		memcpy(d.kt, m.kt, 12);
		memcpy(d.ke, m.ke, 12);
		d.shininess = m.shininess;
		d.ior = m.refractive_index;
		d.tex = m.texture;
		d.periodic = m.periodic;
		memcpy(d.color, m.color, sizeof(d.color));
		d.scale = m.scale;
		d.mortar = m.mortar_width;
		d.nfs = m.noise_feature_scale;
		d.ns = m.noise_scale;
		d.fs = m.frequency_scale;
		d.flags = (m.emittant ? RTX_MF_EMITTANT : 0) | (m.reflective ? RTX_MF_REFLECTIVE : 0) |
			  (m.transparent ? RTX_MF_TRANSPARENT : 0);
	}
	return RTX_OK;
}

/* the objects into plane records and the list of bounded objects */
static int flatten_objects(SceneBuild &b)
{
	const rtx_scene_desc *sc = b.sc;
	for (uint32_t i = 0; i < sc->num_objects; i++) {
		const rtx_object &o = sc->objects[i];
		if (o.material < 0 || (uint32_t)o.material >= sc->num_materials)
			return fail(RTX_ERR_SCENE, "object %u: material index %d out of range", i, o.material);
		if (o.type == RTX_PLANE) {
			DPlane p;
			memset(&p, 0, sizeof(p));
			memcpy(p.n, o.n, 12);
			p.d = o.d;
			p.eps = o.epsilon;
			p.obj = i;
			p.mat = (uint32_t)o.material;
			p.transparent = (b.mats[o.material].flags & RTX_MF_TRANSPARENT) ? 1u : 0u;
			memcpy(p.kt, b.mats[o.material].kt, 12);
			b.planes.push_back(p);
		} else if (o.type == RTX_SPHERE || o.type == RTX_TRIANGLE) {
			b.bounded.push_back(i);
		} else {
			return fail(RTX_ERR_SCENE, "object %u: unknown type %d", i, o.type);
		}
	}
	return RTX_OK;
}

/* bounded object oi as a record k_shadow tests on its own: an emitter's (which adds its lights),
 * or one of a tiny scene's `lin` list */
static DEmitter object_record(const SceneBuild &b, uint32_t oi)
{
	const rtx_object &o = b.sc->objects[oi];
	DEmitter e;
	memset(&e, 0, sizeof(e));
	e.obj = oi;
	e.type = (uint32_t)o.type;
	memcpy(e.p0, o.p0, 12);
	memcpy(e.p1, o.p1, 12);
	memcpy(e.p2, o.p2, 12);
	e.radius = o.radius;
	memcpy(e.e1, o.e1, 12);
	memcpy(e.e2, o.e2, 12);
	e.eps = o.epsilon;
	e.prim = RTX_NONE;
	e.transparent = (b.mats[o.material].flags & RTX_MF_TRANSPARENT) ? 1u : 0u;
	memcpy(e.kt, b.mats[o.material].kt, 12);
	rtx_world_box(o, e.wlo, e.whi);
	return e;
}

static int emitter_records(SceneBuild &b)
{
	const rtx_scene_desc *sc = b.sc;
	b.emit = std::vector<DEmitter>(sc->num_emitters);
	for (uint32_t i = 0; i < sc->num_emitters; i++) {
		uint32_t oi = sc->emitters[i];
		if (oi >= sc->num_objects)
			return fail(RTX_ERR_SCENE, "emitter %u: object %u out of range", i, oi);
		const rtx_object &o = sc->objects[oi];
		if (o.type == RTX_PLANE)
			return fail(RTX_ERR_SCENE, "Plane cannot be emittant");
		DEmitter &e = b.emit[i];
		e = object_record(b, oi);
		e.num_lights = o.num_lights;
		const rtx_material &m = sc->materials[o.material];
		float inv = 1.f / (float)o.num_lights; /* render.c:175 */
		for (int a = 0; a < 3; a++)
			e.li[a] = m.ke[a] * inv;
	}
	return RTX_OK;
}

/* one 64-byte primitive record (rtx_device.h DPrim) of bounded object oi */
static DPrim make_prim(const SceneBuild &b, uint32_t oi)
{
	const rtx_object &o = b.sc->objects[oi];
	DPrim p;
	memset(&p, 0, sizeof(p));
	uint32_t meta = ((uint32_t)o.type << 24) | (uint32_t)o.material;
	if (b.mats[o.material].flags & RTX_MF_TRANSPARENT)
		meta |= RTX_META_TRANSPARENT;
	memcpy(p.a, o.p0, 12);
	p.a[3] = o.epsilon;
	if (o.type == RTX_SPHERE) {
		p.b[0] = o.radius;
	} else {
		memcpy(p.b, o.e1, 12);
		memcpy(p.c, o.e2, 12);
		memcpy(p.d, o.n, 12);
	}
	memcpy(&p.b[3], &oi, 4);
	memcpy(&p.c[3], &meta, 4);
	return p;
}

static bool is_sphere(const DPrim &p)
{
	uint32_t meta;
	memcpy(&meta, &p.c[3], 4);
	return (meta >> 24) == RTX_SPHERE;
}

static int check_record_count(uint32_t nnodes, uint32_t nb)
{
	if (((uint64_t)nnodes + nb) * sizeof(DNode) > 0xFFFFFFC0ull)
		return fail(RTX_ERR_SCENE, "scene too large: %u BVH nodes + %u primitives exceed 4 GB of records", nnodes, nb);
	return RTX_OK;
}

/* GPU builders (rtx_build.hip): primitives uploaded in input order, records emitted on the device
 * into *recs.  The boxes' and the input records' device copies go with this step. */
static int device_bvh2_records(rtx_ctx *c, SceneBuild &b, PhaseClock &clk, DNode **recs)
{
	const uint32_t nb = (uint32_t)b.bounded.size();
	std::vector<DPrim> prims_in(nb);
	rtx_host_parallel(nb, [&](size_t k0, size_t k1, unsigned) {
		for (size_t k = k0; k < k1; k++)
			prims_in[k] = make_prim(b, b.bounded[k]);
	});
	DevBuf<DPrim> d_in; /* (freed in the order lo, hi, in) */
	DevBuf<float> d_hi, d_lo;
	PHASE(clk, "frame + boxes + records", c->stream);
	int rc;
	if ((rc = upload(d_lo, b.lo, c->stream)) || (rc = upload(d_hi, b.hi, c->stream)) || (rc = upload(d_in, prims_in, c->stream)))
		return rc;
	PHASE(clk, "upload boxes + records", c->stream);
	uint32_t rounds = 0;
	const BvhConfig &cfg = b.cfg;
	hipError_t e = c->builder == RTX_BUILD_PLOC_GPU
			       ? rtx_ploc_build(nb, d_lo, d_hi, d_in, b.tlo, b.thi, cfg.max_leaf, recs, &b.nnodes, &b.root_ref,
						&b.depth, &rounds, c->stream)
		       : c->builder == RTX_BUILD_SAH_GPU
			       ? rtx_sah_build(nb, d_lo, d_hi, d_in, cfg.max_leaf, cfg.bins, cfg.max_depth, cfg.c_trav, cfg.c_isect, recs,
					       &b.nnodes, &b.root_ref, &b.depth, &rounds, c->stream)
			       : rtx_lbvh_build(nb, d_lo, d_hi, d_in, b.tlo, b.thi, cfg.max_leaf, recs, &b.nnodes, &b.root_ref,
						&b.depth, c->stream);
	if (e != hipSuccess)
		return fail(RTX_ERR_HIP, "GPU BVH build failed: %s", hipGetErrorString(e));
	PHASE(clk, "device BVH2 build", c->stream);
	return RTX_OK;
}

/* the 8-wide tree collapsed where the records are (single-primitive leaves), the emitters left out */
static int device_collapse(rtx_ctx *c, const SceneBuild &b, const DNode *recs, PhaseClock &clk, HostScene &hs)
{
	const rtx_scene_desc *sc = b.sc;
	std::vector<uint32_t> skip((sc->num_objects + 31) / 32 + 1, 0u);
	for (uint32_t i = 0; i < sc->num_emitters; i++)
		skip[sc->emitters[i] >> 5] |= 1u << (sc->emitters[i] & 31u);
	DevBuf<uint32_t> d_skip;
	int rc;
	if ((rc = upload(d_skip, skip, c->stream)))
		return rc;
	uint32_t ent = 0, dep = 0, wide = 0, top = 0;
	const hipError_t e = rtx_w8_collapse_device(recs, b.nnodes, (uint32_t)b.bounded.size(), d_skip, sc->num_objects, &hs.dev_w8,
						    &hs.dev_w8s, &hs.dev_w8leaf, &ent, &hs.w8s_entries, &dep, &wide, &top, hs.w8f.qo,
						    hs.w8f.qs, c->stream);
	if (e != hipSuccess)
		return fail(RTX_ERR_HIP, "8-wide BVH collapse on the device failed: %s", hipGetErrorString(e));
	PHASE(clk, "device 8-wide collapse", c->stream);
	if (dep) {
		hs.w8_on_device = true;
		hs.w8depth = dep;
		hs.w8_entries = ent;
		hs.w8_wide = wide;
		hs.w8top = top;
		hs.w8noemit = sc->num_emitters > 0;
	}
	return RTX_OK;
}

/* the emitters' record indices (the 8-wide closest-hit walk tests them apart from the tree), found
 * on the device among the nb primitive records at prims */
static int device_emitter_prims(rtx_ctx *c, SceneBuild &b, const DPrim *prims, PhaseClock &clk)
{
	std::vector<DEmitter> &emit = b.emit;
	std::vector<uint32_t> objs(emit.size()), at(emit.size(), RTX_NONE);
	for (size_t i = 0; i < emit.size(); i++)
		objs[i] = emit[i].obj;
	DevBuf<uint32_t> d_at, d_objs;
	int rc;
	if ((rc = upload(d_objs, objs, c->stream)) || (rc = upload(d_at, at, c->stream)))
		return rc;
	hipError_t e = rtx_launch_find_prims(prims, (uint32_t)b.bounded.size(), d_objs, (uint32_t)objs.size(), d_at, c->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(at.data(), d_at, at.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
		e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess)
		return fail(RTX_ERR_HIP, "emitter record lookup failed: %s", hipGetErrorString(e));
	for (size_t i = 0; i < emit.size(); i++)
		emit[i].prim = at[i];
	PHASE(clk, "emitter records", c->stream);
	return RTX_OK;
}

/* the BVH2 on c's device, which keeps the records (c->d_nodes), and from them whatever else the
 * device can do: the 8-wide collapse and the emitters' record indices */
static int build_on_device(rtx_ctx *c, SceneBuild &b, PhaseClock &clk, HostScene &hs)
{
	const rtx_scene_desc *sc = b.sc;
	const uint32_t nb = (uint32_t)b.bounded.size();
	uint32_t sph = 0;
	for (uint32_t k = 0; k < nb && !sph; k++)
		if (sc->objects[b.bounded[k]].type == RTX_SPHERE)
			sph = RTX_REF_SPH;
	DNode *recs = nullptr;
	int rc = device_bvh2_records(c, b, clk, &recs);
	if (rc)
		return rc;
	c->d_nodes = recs;
	hs.recs_on_device = true;
	if (b.root_ref == RTX_EMPTY_REF) /* nb <= max_leaf: a single leaf */
		b.root_ref = RTX_REF_LEAF | sph | (nb - 1);
	if ((rc = check_record_count(b.nnodes, nb)))
		return rc;
	if (b.want_w8 && b.cfg.max_leaf == 1 && b.nnodes && (rc = device_collapse(c, b, recs, clk, hs)))
		return rc;
	/* the host needs the records only for the host collapse or the threaded BVH2 */
	if (!hs.w8_on_device) {
		b.inner.resize(b.nnodes);
		if (b.nnodes)
			HIP_TRY(hipMemcpy(b.inner.data(), recs, b.nnodes * sizeof(DNode), hipMemcpyDeviceToHost));
		b.prims_dl.resize(nb);
		HIP_TRY(hipMemcpy(b.prims_dl.data(), recs + b.nnodes, (size_t)nb * sizeof(DPrim), hipMemcpyDeviceToHost));
		b.host_prims = b.prims_dl.data();
	}
	if (!b.emit.empty() && (rc = device_emitter_prims(c, b, (const DPrim *)(recs + b.nnodes), clk)))
		return rc;
	return RTX_OK;
}

/* the BVH2 from the host's SAH builder (bvh_build.cpp), its records into hs.recs */
static int build_on_host(SceneBuild &b, HostScene &hs)
{
	const uint32_t nb = (uint32_t)b.bounded.size();
	BvhOutput bvh;
	bvh_build(BvhInput{ nb, b.lo.data(), b.hi.data() }, b.cfg, bvh);
	std::vector<DPrim> prims(nb);
	for (uint32_t k = 0; k < nb; k++)
		prims[k] = make_prim(b, b.bounded[bvh.order[k]]);
	/* nodes and primitives in one array of 64-byte records: the shadow walk addresses both
	 * through one base pointer (record num_nodes + i = primitive i) */
	const uint32_t nnodes = b.nnodes = (uint32_t)bvh.nodes.size();
	int rc = check_record_count(nnodes, nb);
	if (rc)
		return rc;
	/* builder refs (node index | RTX_LEAF_BIT leaf) -> device refs (record byte offset | leaf bits) */
	auto dref = [nnodes, &prims](uint32_t r) -> uint32_t {
		if (r == RTX_EMPTY_REF)
			return r;
		if (r & RTX_LEAF_BIT) {
			const uint32_t first = (r >> 4) & 0x7FFFFFFu, cnt = (r & 15u) + 1;
			uint32_t sph = 0;
			for (uint32_t k = first; k < first + cnt; k++)
				if (is_sphere(prims[k]))
					sph = RTX_REF_SPH;
			return (nnodes + first) * (uint32_t)sizeof(DNode) | RTX_REF_LEAF | sph | (cnt - 1);
		}
		return r * (uint32_t)sizeof(DNode);
	};
	std::vector<DNode> recs(nnodes + (size_t)nb);
	for (uint32_t i = 0; i < nnodes; i++) {
		recs[i] = bvh.nodes[i];
		recs[i].ref0 = dref(recs[i].ref0);
		recs[i].ref1 = dref(recs[i].ref1);
	}
	if (nb)
		memcpy(recs.data() + nnodes, prims.data(), nb * sizeof(DPrim));
	/* the emitters' record indices (the 8-wide closest-hit walk tests them apart from the tree) */
	{
		std::vector<uint32_t> rec_of(b.sc->num_objects, RTX_NONE);
		for (uint32_t k = 0; k < nb; k++)
			rec_of[b.bounded[bvh.order[k]]] = k;
		for (DEmitter &e : b.emit)
			e.prim = rec_of[e.obj];
	}
	b.root_ref = dref(bvh.root_ref);
	b.depth = bvh.depth;
	b.inner.assign(recs.begin(), recs.begin() + nnodes);
	hs.recs = std::move(recs);
	b.host_prims = (const DPrim *)(hs.recs.data() + nnodes);
	return RTX_OK;
}

/* the shadow walk's BVH (RTX_OPT_SHADOW_WALK): the 8-wide compressed tree by default, which
 * walks any depth (collapsed on the device by build_on_device, else here from the host records);
 * the threaded BVH2 for small scenes (its top levels in LDS), for measurement, and when the 8-wide
 * tree cannot be built (over 2^24 entries) */
static void build_shadow_tree(SceneBuild &b, HostScene &hs)
{
	const rtx_scene_desc *sc = b.sc;
	const uint32_t nb = (uint32_t)b.bounded.size();
	if (!hs.w8_on_device && b.want_w8) {
		/* with the host records the emitters are left out of the tree (k_shadow tests them linearly) */
		std::vector<uint32_t> emit_objs;
		for (const DEmitter &e : b.emit)
			emit_objs.push_back(e.obj);
		hs.w8depth = rtx_wide8_build(b.inner, b.nnodes, b.host_prims, b.root_ref, b.tlo, b.thi, emit_objs, hs.tf, hs.frame_pad,
					     hs.w8f, hs.w8noemit, hs.w8, hs.w8leaf);
	}
	if (hs.w8.empty() && !hs.w8_on_device)
		hs.w8depth = 0;
	/* does the 8-wide tree hold spheres?  (the emitters it leaves out do not count) */
	if (hs.w8depth) {
		std::vector<char> is_emit(sc->num_objects, 0);
		for (const DEmitter &e : b.emit)
			is_emit[e.obj] = 1;
		hs.w8sph = false;
		for (uint32_t k = 0; k < nb && !hs.w8sph; k++)
			hs.w8sph = sc->objects[b.bounded[k]].type == RTX_SPHERE && !(hs.w8noemit && is_emit[b.bounded[k]]);
	}
}

/* the walks without an 8-wide tree: a tiny scene's objects as `lin` records, else the threaded BVH2 */
static int build_small_walk(SceneBuild &b, bool linear, HostScene &hs)
{
	const uint32_t nb = (uint32_t)b.bounded.size();
	if (linear) {
		for (uint32_t k = 0; k < nb; k++)
			hs.lin.push_back(object_record(b, b.bounded[k]));
	} else if (!hs.w8depth) {
		std::vector<uint32_t> qdepth;
		thread_bvh(b.inner, nb ? b.root_ref : RTX_EMPTY_REF, b.tlo, b.thi, hs.qnodes, hs.qf, qdepth);
		if (hs.qnodes.size() >= (1u << 26))
			return fail(RTX_ERR_SCENE, "scene too large: %zu threaded BVH nodes (max 2^26)", hs.qnodes.size());
		hs.ntop = thread_top(hs.qnodes, qdepth, hs.qtop);
	}
	return RTX_OK;
}

int rtx_build_scene(rtx_ctx *c, const rtx_scene_desc *sc, HostScene &hs)
{
	if (!sc->num_materials || !sc->materials)
		return fail(RTX_ERR_SCENE, "scene has no materials");
	if (sc->num_objects && !sc->objects)
		return fail(RTX_ERR_ARG, "objects pointer is null");
	if (sc->num_emitters && !sc->emitters)
		return fail(RTX_ERR_ARG, "emitters pointer is null");
	HIP_TRY(hipSetDevice(c->device));
	PhaseClock clk0;
	rtx_free_scene(c);
	PHASE(clk0, "free the old scene", c->stream);
	hs.builder = c->builder;
	hs.device = c->device;

	SceneBuild b;
	b.sc = sc;
	int rc;
	if ((rc = flatten_materials(sc, b.mats)) || (rc = flatten_objects(b)))
		return rc;

	/* leaf boxes (sphere_get_corners / triangle_get_corners), padded so the traversal's
	 * FMA slab test is conservative: in world space for the bounded objects' box (the
	 * shade-point sort's frame), then in the trees' frame (rtx_frame.cpp) for the builders */
	const uint32_t nb = (uint32_t)b.bounded.size();
	b.lo = std::vector<float>(3 * (size_t)nb);
	b.hi = std::vector<float>(3 * (size_t)nb);
	PHASE(clk0, "materials + planes", c->stream);
	rtx_world_boxes(sc, b.bounded, b.lo.data(), b.hi.data(), c->bound_lo, c->bound_hi);
	PHASE(clk0, "world boxes", c->stream);
	PhaseClock clk;
	const auto tf0 = std::chrono::steady_clock::now();
	DTreeFrame &tf = hs.tf;
	hs.frame_ratio = c->opt_frame == RTX_FRAME_AUTO ? rtx_frame_choose(sc, b.bounded, c->bound_lo, c->bound_hi, tf) : 1.0;
	if (c->opt_frame != RTX_FRAME_AUTO)
		rtx_frame_choose(sc, {}, c->bound_lo, c->bound_hi, tf); /* the identity */
	memcpy(b.tlo, c->bound_lo, 12);
	memcpy(b.thi, c->bound_hi, 12);
	/* the objects' centre and radius for the far-origin test (rtx_math.h tf_far), in every frame */
	rtx_frame_far(c->bound_lo, c->bound_hi, tf);
	if (tf.rotated) {
		const double pad = hs.frame_pad = rtx_frame_pad(rtx_frame_radius(c->bound_lo, c->bound_hi, tf));
		rtx_frame_boxes(sc, b.bounded, tf, pad, b.lo.data(), b.hi.data(), b.tlo, b.thi);
	}
	hs.frame_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count();
	b.cfg.max_leaf = c->opt_leaf; /* RTX_OPT_BVH_LEAF (default 1) */

	if ((rc = emitter_records(b)))
		return rc;

	const auto tb0 = std::chrono::steady_clock::now();
	/* RTX_WALK_AUTO: a scene whose threaded BVH2 fits the LDS top records is walked from LDS alone
	 * (scene3, 3 spheres: 102 ms vs 114 ms over the 8-wide tree); larger ones over the 8-wide tree */
	const bool small = (uint64_t)2 * nb <= RTX_TOP_MAX + 1;
	/* a tiny scene (RTX_WALK_LINEAR): k_shadow tests its few bounded objects one by one like the planes
	 * (scene1 / scene3: 3 spheres, one of them the light), no walk */
	const bool linear = nb && (c->opt_walk == RTX_WALK_LINEAR || (c->opt_walk == RTX_WALK_AUTO && nb <= RTX_SHADOW_LINEAR_MAX));
	b.want_w8 = nb && !linear && (c->opt_walk == RTX_WALK_W8 || (c->opt_walk == RTX_WALK_AUTO && !small));
	const bool on_device = c->builder == RTX_BUILD_LBVH_GPU || c->builder == RTX_BUILD_PLOC_GPU || c->builder == RTX_BUILD_SAH_GPU;
	if ((rc = on_device && nb ? build_on_device(c, b, clk, hs) : build_on_host(b, hs)))
		return rc;
	build_shadow_tree(b, hs);
	if ((rc = build_small_walk(b, linear, hs)))
		return rc;
	PHASE(clk, "host trees", c->stream);
	hs.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
	hs.mats = std::move(b.mats);
	hs.planes = std::move(b.planes);
	hs.emit = std::move(b.emit);
	hs.nnodes = b.nnodes;
	hs.nb = nb;
	hs.root_ref = nb ? b.root_ref : RTX_EMPTY_REF;
	hs.depth = b.depth;
	memcpy(hs.bound_lo, c->bound_lo, 12);
	memcpy(hs.bound_hi, c->bound_hi, 12);
	memcpy(hs.ambient, sc->ambient, 12);
	hs.num_emitters = sc->num_emitters;
	return RTX_OK;
}
