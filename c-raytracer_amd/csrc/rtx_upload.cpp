/*
 * A built scene (rtx_scene.cpp) onto a context's device: the records, trees and tables, the
 * 8-wide tree's leaf fill, k_shadow's cull and per-point spheres, and the DScene the kernels take.
 */
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_frame.h"
#include "rtx_quant.h"
#include "rtx_internal.h"

void rtx_free_scene(rtx_ctx *c)
{
	dfree(c->d_nodes);
	dfree(c->d_planes);
	dfree(c->d_mats);
	dfree(c->d_emitters);
	dfree(c->d_lin);
	dfree(c->d_cull);
	dfree(c->d_lsph);
	dfree(c->d_qnodes);
	dfree(c->d_top);
	dfree(c->d_w8);
	dfree(c->d_w8s);
	c->have_scene = false;
	c->sp_tile_seen = 0.0;
	c->sp_tile_key = SpKey{};
}

/* the built scene onto c's device (c->d_nodes already holds the records when the device
 * builder ran on c, or a group copied them to it); device buffers in hs (the 8-wide tree
 * collapsed on the device) change hands to c */
int rtx_upload_built(rtx_ctx *c, HostScene &hs)
{
	DevTree t{ hs.dev_w8, hs.dev_w8s, hs.dev_w8leaf, hs.device };
	hs.dev_w8 = nullptr;
	hs.dev_w8s = nullptr;
	hs.dev_w8leaf = nullptr;
	const int rc = rtx_upload_built(c, hs, &t);
	/* whatever was not handed over goes back to hs, whose destructor frees it */
	hs.dev_w8 = t.w8;
	hs.dev_w8s = t.w8s;
	hs.dev_w8leaf = t.leaf;
	return rc;
}

/* k_shadow's cone cull (DScene.cull, RTX_OPT_SHADOW_CULL): the bounding spheres of the 8-wide
 * tree's second level in world coordinates, from the root entry and its child nodes read back from
 * the device.  Every primitive of the tree lies in one of these boxes (a root slot's children, or
 * the root slot itself when it is a leaf); the spheres are formed in double from the quantised
 * boxes (which contain the primitives' float boxes) and padded for the kernel's float test. */
static int build_cull(rtx_ctx *c, const HostScene &hs, uint32_t num_w8, uint32_t *n_out)
{
	*n_out = 0;
	if (!c->d_w8 || num_w8 < 2)
		return RTX_OK;
	DW8 root, kid[8];
	HIP_TRY(hipMemcpyAsync(&root, c->d_w8, sizeof(DW8), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	const uint32_t base = root.w[2] >> 8, imask = root.w[2] & 0xFFu, vmask = root.w[3] & 0xFFu;
	if (!vmask)
		return RTX_OK;
	if ((uint64_t)base + 8 > num_w8)
		return fail(RTX_ERR_STATE, "8-wide root's children at %u beyond %u entries", base, num_w8);
	HIP_TRY(hipMemcpyAsync(kid, c->d_w8 + base, sizeof(kid), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	std::vector<float4> sph;
	auto add_box = [&](const DW8 &N, int slot) {
		const double org[3] = { (double)(N.w[0] & 0xFFFFu), (double)(N.w[0] >> 16), (double)(N.w[1] & 0xFFFFu) };
		const int ex[3] = { (int)((N.w[1] >> 16) & 15u), (int)((N.w[1] >> 20) & 15u), (int)((N.w[1] >> 24) & 15u) };
		double ctr[3], r2 = 0;
		for (int a = 0; a < 3; a++) {
			const uint32_t lo8 = (N.w[4 + 4 * a + (slot >> 2)] >> (8 * (slot & 3))) & 0xFFu;
			const uint32_t hi8 = (N.w[6 + 4 * a + (slot >> 2)] >> (8 * (slot & 3))) & 0xFFu;
			const double lo = (org[a] + std::ldexp((double)lo8, ex[a])) / (double)hs.w8f.qs[a] + (double)hs.w8f.qo[a];
			const double hi = (org[a] + std::ldexp((double)hi8, ex[a])) / (double)hs.w8f.qs[a] + (double)hs.w8f.qo[a];
			ctr[a] = 0.5 * (lo + hi);
			r2 += 0.25 * (hi - lo) * (hi - lo);
		}
		double w[3], m = 0;
		for (int a = 0; a < 3; a++) /* the frame's x' = R (x - c): x = R^T x' + c */
			w[a] = hs.tf.rotated ? (double)hs.tf.c[a] + hs.tf.r[0][a] * ctr[0] + hs.tf.r[1][a] * ctr[1] + hs.tf.r[2][a] * ctr[2]
					      : ctr[a];
		for (int a = 0; a < 3; a++)
			m = std::max(m, std::fabs(w[a]));
		const double r = std::sqrt(r2);
		sph.push_back(make_float4((float)w[0], (float)w[1], (float)w[2], (float)(r * (1 + 1e-5) + 1e-5 * m + 1e-6)));
	};
	for (int s = 0; s < 8; s++) {
		if (!((vmask >> s) & 1u))
			continue;
		if ((imask >> s) & 1u) {
			const DW8 &K = kid[s];
			for (int s2 = 0; s2 < 8; s2++)
				if ((K.w[3] >> s2) & 1u)
					add_box(K, s2);
		} else {
			add_box(root, s);
		}
	}
	if (sph.empty() || sph.size() > RTX_CULL_MAX)
		return RTX_OK;
	int rc = upload(c->d_cull, sph, c->stream);
	if (rc)
		return rc;
	*n_out = (uint32_t)sph.size();
	return RTX_OK;
}

/* k_shadow's per-point masks (DScene.lsph, RTX_OPT_SHADOW_POINT): the bounding spheres of the
 * records k_shadow tests one by one, in their order (the emitters an 8-wide tree leaves out, or a
 * tiny scene's objects).  More than RTX_CULL_MAX: none (their tests then always run). */
static int build_lsph(rtx_ctx *c, const std::vector<DEmitter> &recs, uint32_t *n_out)
{
	*n_out = 0;
	if (recs.empty() || recs.size() > RTX_CULL_MAX)
		return RTX_OK;
	std::vector<float4> sph(recs.size());
	for (size_t k = 0; k < recs.size(); k++) {
		float s[4];
		rtx_record_sphere(recs[k].type == RTX_SPHERE, recs[k].p0, recs[k].p1, recs[k].p2, recs[k].radius, s);
		sph[k] = make_float4(s[0], s[1], s[2], s[3]);
	}
	int rc = upload(c->d_lsph, sph, c->stream);
	if (rc)
		return rc;
	*n_out = (uint32_t)sph.size();
	return RTX_OK;
}

/* k_shadow's dark samples (DScene.dark_ok, RTX_OPT_SHADOW_DARK): a sample whose terms are 0 may skip
 * its shadow query only if nothing the query gathers could turn 0 into NaN or let a product grow,
 * so every transmittance a shadow ray can meet (the materials' kt, which the plane and emitter
 * records copy) is finite with |kt| <= 1 and every emitter's intensity is finite */
static bool scene_dark_ok(const HostScene &hs)
{
	for (const DMaterial &m : hs.mats)
		for (int k = 0; k < 3; k++)
			if (!(std::fabs(m.kt[k]) <= 1.f))
				return false;
	for (const DPlane &p : hs.planes)
		for (int k = 0; k < 3; k++)
			if (!(std::fabs(p.kt[k]) <= 1.f))
				return false;
	for (const DEmitter &e : hs.emit)
		for (int k = 0; k < 3; k++)
			if (!std::isfinite(e.li[k]) || !(std::fabs(e.kt[k]) <= 1.f))
				return false;
	for (const DEmitter &e : hs.lin)
		for (int k = 0; k < 3; k++)
			if (!(std::fabs(e.kt[k]) <= 1.f))
				return false;
	return true;
}

/* the 8-wide tree onto c's device (taken over from `take`, or uploaded and its scalar-path copies
 * made), and its leaf entries filled from c's primitive records and materials */
static int upload_w8(rtx_ctx *c, const HostScene &hs, DevTree *take, bool have_w8, uint32_t num_w8, PhaseClock &clk)
{
	int rc;
	DevBuf<uint32_t> d_map; /* entry -> primitive index of the 8-wide tree's leaf entries */
	if (hs.w8_on_device) { /* collapsed on the device (or peer-copied to it): the buffers change hands */
		if (!take || take->device != c->device)
			return fail(RTX_ERR_STATE, "8-wide tree on device %d uploaded to device %d", take ? take->device : -1, c->device);
		dfree(c->d_w8);
		dfree(c->d_w8s);
		c->d_w8 = take->w8;
		c->d_w8s = take->w8s;
		d_map.p = take->leaf;
		take->w8 = nullptr;
		take->w8s = nullptr;
		take->leaf = nullptr;
		PHASE(clk, "8-wide tree handover", c->stream);
	} else {
		if ((rc = upload(c->d_w8, hs.w8, c->stream)))
			return rc;
		if ((rc = upload(d_map, hs.w8leaf, c->stream)))
			return rc;
		dfree(c->d_w8s);
		/* the scalar-path node copies (rtx_device.h DW8S) */
		hipError_t e = hipMalloc(&c->d_w8s, std::max<size_t>(num_w8, 1) * sizeof(DW8S));
		if (e == hipSuccess)
			e = rtx_launch_w8_scalar(num_w8, c->d_w8, d_map, c->d_w8s, c->stream);
		if (e != hipSuccess)
			return fail(RTX_ERR_HIP, "8-wide BVH scalar copies failed: %s", hipGetErrorString(e));
	}
	PHASE(clk, "upload host parts", c->stream);
	if (have_w8) { /* the 8-wide tree's leaf entries: copies of their primitive records */
		hipError_t e = rtx_launch_w8_fill((const DPrim *)(c->d_nodes + hs.nnodes), c->d_mats, d_map, num_w8, c->d_w8, c->stream);
		if (e == hipSuccess)
			e = hipStreamSynchronize(c->stream);
		if (e != hipSuccess)
			return fail(RTX_ERR_HIP, "8-wide BVH leaf fill failed: %s", hipGetErrorString(e));
	}
	return RTX_OK;
}

int rtx_upload_built(rtx_ctx *c, const HostScene &hs, DevTree *take)
{
	int rc;
	PhaseClock clk;
	/* a failure below leaves the context without a scene (RTX_ERR_STATE on render), never with a
	 * mix of old and new buffers */
	c->have_scene = false;
	c->sp_tile_seen = 0.0; /* the next render sizes its chunks from the static bound */
	c->sp_tile_key = SpKey{};
	c->tp_valid = false; /* rtx_render_temporal's history is of the scene before */
	HIP_TRY(hipSetDevice(c->device));
	if (!(hs.recs_on_device && c->d_nodes) && (rc = upload(c->d_nodes, hs.recs, c->stream)))
		return rc;
	PHASE(clk, "upload: set device", c->stream);
	if ((rc = upload(c->d_qnodes, hs.qnodes, c->stream)) || (rc = upload(c->d_top, hs.qtop, c->stream)))
		return rc;
	PHASE(clk, "upload threaded BVH2", c->stream);
	if ((rc = upload(c->d_planes, hs.planes, c->stream)))
		return rc;
	PHASE(clk, "upload planes", c->stream);
	if ((rc = upload(c->d_mats, hs.mats, c->stream)) || (rc = upload(c->d_emitters, hs.emit, c->stream)) || (rc = upload(c->d_lin, hs.lin, c->stream)))
		return rc;
	PHASE(clk, "upload scene tables", c->stream);
	const bool have_w8 = hs.w8_on_device || !hs.w8.empty();
	const uint32_t num_w8 = hs.w8_on_device ? hs.w8_entries : (uint32_t)hs.w8.size();
	if ((rc = upload_w8(c, hs, take, have_w8, num_w8, clk)))
		return rc;
	PHASE(clk, "8-wide leaf fill", c->stream);
	uint32_t ncull = 0; /* the cone cull needs the emitters out of the tree (else a light's own leaf meets every cone) */
	if (have_w8 && hs.w8noemit && hs.lin.empty() && (rc = build_cull(c, hs, num_w8, &ncull)))
		return rc;
	uint32_t nlsph = 0; /* the records rtx_launch_shadow lists: the emitters out of the 8-wide tree, else `lin` */
	static const std::vector<DEmitter> none;
	if ((rc = build_lsph(c, have_w8 ? (hs.w8noemit ? hs.emit : none) : hs.lin, &nlsph)))
		return rc;
	memcpy(c->bound_lo, hs.bound_lo, 12);
	memcpy(c->bound_hi, hs.bound_hi, 12);
	DScene &S = c->scene;
	memset(&S, 0, sizeof(S));
	S.nodes = c->d_nodes;
	S.num_nodes = hs.nnodes;
	S.prims = (const DPrim *)(c->d_nodes + hs.nnodes);
	S.planes = c->d_planes;
	S.mats = c->d_mats;
	S.emitters = c->d_emitters;
	S.lin = hs.lin.empty() ? nullptr : c->d_lin;
	S.num_lin = (uint32_t)hs.lin.size();
	S.qnodes = hs.qnodes.empty() ? nullptr : c->d_qnodes;
	S.num_qnodes = (uint32_t)hs.qnodes.size();
	memcpy(S.qo, hs.qf.qo, 12);
	memcpy(S.qs, hs.qf.qs, 12);
	S.top = hs.ntop ? c->d_top : nullptr;
	S.num_top = hs.ntop;
	S.w8 = have_w8 ? c->d_w8 : nullptr;
	S.num_w8 = num_w8;
	S.w8depth = hs.w8depth;
	S.w8top = hs.w8_on_device ? hs.w8top : 0u; /* the device collapse's breadth-first layout only */
	memcpy(S.w8qo, hs.w8f.qo, 12);
	memcpy(S.w8qs, hs.w8f.qs, 12);
	S.w8noemit = hs.w8noemit ? 1u : 0u;
	S.w8sph = hs.w8sph ? 1u : 0u;
	S.w8s = have_w8 ? c->d_w8s : nullptr;
	S.root_ref = hs.root_ref;
	S.num_prims = hs.nb;
	S.num_planes = (uint32_t)hs.planes.size();
	S.num_emitters = hs.num_emitters;
	S.stack_size = std::max<uint32_t>(hs.depth + 1, 4);
	S.tf = hs.tf;
	S.cull = ncull ? (const float *)c->d_cull : nullptr;
	S.num_cull = ncull;
	S.lsph = nlsph ? (const float *)c->d_lsph : nullptr;
	S.num_lsph = nlsph;
	S.dark_ok = scene_dark_ok(hs) ? 1u : 0u;
	c->total_lights = 0;
	for (const DEmitter &e : hs.emit)
		c->total_lights += e.num_lights;
	memcpy(S.ambient, hs.ambient, 12);
	c->have_scene = true;
	c->stats.build_ms = hs.build_ms;
	c->stats.bvh_nodes = hs.nnodes;
	c->stats.bvh_depth = hs.depth;
	c->stats.builder = (uint32_t)hs.builder;
	c->stats.bvh_prims = hs.nb;
	c->stats.shadow_walk = S.lin ? RTX_WALK_LINEAR : S.w8 ? RTX_WALK_W8 : RTX_WALK_BVH2;
	c->stats.tree_rotated = hs.tf.rotated;
	c->stats.frame_cost = hs.frame_ratio;
	c->stats.frame_ms = hs.frame_ms;
	if (S.w8) {
		uint32_t inner_nodes = hs.w8_wide;
		if (!hs.w8_on_device)
			for (const DW8 &e : hs.w8)
				inner_nodes += e.w[3] != 0;
		c->stats.wide_nodes = inner_nodes;
		c->stats.wide_depth = S.w8depth;
		c->stats.wide_entries = S.num_w8;
	} else {
		c->stats.wide_nodes = 0;
		c->stats.wide_depth = 0;
		c->stats.wide_entries = 0;
	}
	return RTX_OK;
}

extern "C" int rtx_upload_scene(rtx_ctx *c, const rtx_scene_desc *sc)
{
	if (!c || !sc)
		return fail(RTX_ERR_ARG, "null argument");
	HostScene hs;
	int rc = rtx_build_scene(c, sc, hs);
	if (rc)
		return rc;
	return rtx_upload_built(c, hs);
}
