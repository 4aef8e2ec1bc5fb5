/*
 * C-ABI of include/rtx.h, the context: last error, defaults, open and close, options and the
 * builder choice, statistics, the known-answer entry, the 8-wide tree read back.
 */
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_kat.h"
#include "rtx_internal.h"

static thread_local char g_err[512] = "";

int rtx_fail(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return code;
}


extern "C" const char *rtx_last_error(void)
{
	return g_err;
}

extern "C" void rtx_params_default(rtx_params *p)
{
	memset(p, 0, sizeof(*p));
	p->max_bounces = 10;
	p->min_intensity_sqr = .01f * .01f;
	p->reflection = RTX_PHONG;
	p->gi = RTX_GI_AMBIENT;
	p->samples = 1;
	p->attenuation = RTX_ATT_SQR;
	p->attenuation_offset = 1.f;
	p->rng = RTX_RNG_COUNTER;
	p->seed = 1;
	p->u32conv = RTX_U32_SAT;
	p->tile_offset = 0;
	p->tile_stride = 1;
	p->count_traversal = 0;
}

extern "C" int rtx_device_count(int *count)
{
	if (!count)
		return fail(RTX_ERR_ARG, "null count");
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	*count = (e == hipSuccess) ? n : 0;
	return RTX_OK;
}

extern "C" void rtx_close(rtx_ctx *c)
{
	if (!c)
		return;
	(void)hipSetDevice(c->device);
	if (c->stream)
		(void)hipStreamSynchronize(c->stream);
	rtx_free_scene(c);
	/* the work buffers, then the events and the stream (rtx_internal.h CtxHandles) */
	delete c;
}

extern "C" int rtx_open(int device, rtx_ctx **out)
{
	if (!out)
		return fail(RTX_ERR_ARG, "null out");
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
		return fail(RTX_ERR_NODEV, "no HIP device available");
	if (device < 0 || device >= n)
		return fail(RTX_ERR_NODEV, "device %d out of range (%d devices)", device, n);
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	if (!strstr(prop.gcnArchName, "gfx950"))
		return fail(RTX_ERR_NODEV, "device %d is %s, this build targets gfx950 only", device, prop.gcnArchName);
	rtx_ctx *c = new rtx_ctx();
	c->device = device;
	c->cus = prop.multiProcessorCount;
	hipError_t e;
	if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess ||
	    (e = hipEventCreate(&c->ev[0])) != hipSuccess || (e = hipEventCreate(&c->ev[1])) != hipSuccess ||
	    (e = hipEventCreate(&c->ev[2])) != hipSuccess || (e = hipEventCreate(&c->ev[3])) != hipSuccess ||
	    (e = hipEventCreate(&c->ev[4])) != hipSuccess ||
	    (e = c->d_ctr.grow(sizeof(unsigned long long) * RTX_C_N)) != hipSuccess) {
		rtx_close(c);
		return fail(RTX_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
	}
	/* one-time device set-up here rather than inside the first upload or render: every code object
	 * of the library loaded on this device (the runtime loads one at its first launch otherwise,
	 * ~30 ms inside the first BVH build), and the runtime's pageable-copy path primed */
	for (hipError_t (*load)(void) : { rtx_load_build, rtx_load_wide8_dev, rtx_load_shadow, rtx_load_trace, rtx_load_sort,
					  rtx_load_post, rtx_load_gather, rtx_load_denoise, rtx_load_denoise_variance, rtx_load_passes,
					  rtx_load_adaptive, rtx_load_filter, rtx_load_upsample, rtx_load_temporal, rtx_load_projection, rtx_load_nearest })
		if ((e = load()) != hipSuccess) {
			rtx_close(c);
			return fail(RTX_ERR_HIP, "loading the device code failed: %s", hipGetErrorString(e));
		}
	{
		std::vector<uint8_t> h((size_t)4 << 20, 0);
		void *d = nullptr;
		e = hipMalloc(&d, h.size());
		if (e == hipSuccess)
			e = hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess)
			e = hipMemcpyAsync(h.data(), d, 64, hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess)
			e = hipStreamSynchronize(c->stream);
		if (d)
			(void)hipFree(d);
		if (e != hipSuccess) {
			rtx_close(c);
			return fail(RTX_ERR_HIP, "context setup failed: %s", hipGetErrorString(e));
		}
	}
	*out = c;
	return RTX_OK;
}

extern "C" int rtx_set_builder(rtx_ctx *c, int builder)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null argument");
	if (builder != RTX_BUILD_SAH_HOST && builder != RTX_BUILD_LBVH_GPU && builder != RTX_BUILD_PLOC_GPU &&
	    builder != RTX_BUILD_SAH_GPU)
		return fail(RTX_ERR_ARG, "unknown BVH builder %d", builder);
	c->builder = builder;
	return RTX_OK;
}

extern "C" int rtx_set_option(rtx_ctx *c, int option, int64_t value)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null argument");
	switch (option) {
	case RTX_OPT_SHADOW_WALK:
		if (value != RTX_WALK_AUTO && value != RTX_WALK_BVH2 && value != RTX_WALK_W8 && value != RTX_WALK_LINEAR)
			return fail(RTX_ERR_ARG, "shadow walk %lld is not AUTO, BVH2, W8 or LINEAR", (long long)value);
		c->opt_walk = (int)value;
		return RTX_OK;
	case RTX_OPT_BVH_LEAF:
		if (value < 1 || value > RTX_MAX_LEAF)
			return fail(RTX_ERR_ARG, "BVH leaf size %lld outside 1..%d", (long long)value, RTX_MAX_LEAF);
		c->opt_leaf = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_SPSORT:
		if (value != 0 && value != 1)
			return fail(RTX_ERR_ARG, "RTX_OPT_SPSORT takes 0 or 1, not %lld", (long long)value);
		c->opt_spsort = value != 0;
		return RTX_OK;
	case RTX_OPT_SHADOW_SLOT:
		if (value < 0 || value > 64 || (value & (value - 1)))
			return fail(RTX_ERR_ARG, "shadow slot %lld is not 0 or a power of two <= 64", (long long)value);
		c->opt_slot = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_LDS_STACK:
		if (value < 1 || value > RTX_W8_STACK)
			return fail(RTX_ERR_ARG, "shadow LDS stack %lld outside 1..%d", (long long)value, RTX_W8_STACK);
		c->opt_lstk = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_TRACE_WALK:
		if (value != RTX_WALK_AUTO && value != RTX_WALK_W8 && value != RTX_WALK_BVH2)
			return fail(RTX_ERR_ARG, "closest-hit walk %lld is not AUTO, W8 or BVH2", (long long)value);
		c->opt_trace_walk = (int)value;
		return RTX_OK;
	case RTX_OPT_TREE_FRAME:
		if (value != RTX_FRAME_AUTO && value != RTX_FRAME_WORLD)
			return fail(RTX_ERR_ARG, "tree frame %lld is not AUTO or WORLD", (long long)value);
		c->opt_frame = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_GRAB:
		if (value < 1 || value > (1 << 24))
			return fail(RTX_ERR_ARG, "shadow grab %lld outside 1..2^24", (long long)value);
		c->opt_grab = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_CHUNK_TILES:
		if (value < 0 || value > 0xFFFFFFFFll)
			return fail(RTX_ERR_ARG, "chunk tiles %lld outside 0..2^32-1", (long long)value);
		c->opt_chunk = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_SP_PER_TILE:
		if (value < 0 || value > (1 << 20))
			return fail(RTX_ERR_ARG, "shade points per tile %lld outside 0..2^20", (long long)value);
		c->opt_sp_tile = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_RAYS_GRAB:
		if (value < 0 || value > 64)
			return fail(RTX_ERR_ARG, "ray-query grab %lld outside 0..64", (long long)value);
		c->opt_rays_grab = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_RAYS_QUEUES:
		if (value < 0 || value > RTX_RQ_MAX_QUEUES)
			return fail(RTX_ERR_ARG, "ray-query queues %lld outside 0..%d", (long long)value, RTX_RQ_MAX_QUEUES);
		c->opt_rays_queues = (uint32_t)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_CULL:
		if (value < 0 || value > 2)
			return fail(RTX_ERR_ARG, "shadow cull %lld is not 0, 1 or 2", (long long)value);
		c->opt_cull = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_POINT:
		if (value < 0 || value > 1)
			return fail(RTX_ERR_ARG, "shadow point masks %lld is not 0 or 1", (long long)value);
		c->opt_point = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_DARK:
		if (value < 0 || value > 1)
			return fail(RTX_ERR_ARG, "shadow dark samples %lld is not 0 or 1", (long long)value);
		c->opt_dark = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_ORDER:
		if (value < 0 || value > 1)
			return fail(RTX_ERR_ARG, "shadow sample order %lld is not 0 or 1", (long long)value);
		c->opt_order = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_SPEC:
		if (value < 0 || value > 1)
			return fail(RTX_ERR_ARG, "shadow specular shortcut %lld is not 0 or 1", (long long)value);
		c->opt_spec = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_CLEARLANE:
		if (value < 0 || value > 1)
			return fail(RTX_ERR_ARG, "shadow clear lanes %lld is not 0 or 1", (long long)value);
		c->opt_clearlane = (int)value;
		return RTX_OK;
	case RTX_OPT_SHADOW_PREMASK:
		if (value < 0 || value > 1)
			return fail(RTX_ERR_ARG, "shadow pre-mask %lld is not 0 or 1", (long long)value);
		c->opt_premask = (int)value;
		return RTX_OK;
	case RTX_OPT_TRACE_PACK:
		if (value != 0 && value != 1 && value != 512 && value != 1024 && value != 2048 && value != 4096)
			return fail(RTX_ERR_ARG, "trace pack %lld is not 0, 1, 512, 1024, 2048 or 4096", (long long)value);
		c->opt_trace_pack = (uint32_t)value;
		return RTX_OK;
	}
	return fail(RTX_ERR_ARG, "unknown option %d", option);
}

extern "C" int rtx_read_wide_tree(rtx_ctx *c, void *entries, uint32_t capacity, uint32_t *count, float frame[6])
{
	if (!c || !count)
		return fail(RTX_ERR_ARG, "null argument");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_read_wide_tree before rtx_upload_scene");
	const DScene &S = c->scene;
	*count = S.w8 ? S.num_w8 : 0u;
	if (frame) {
		memcpy(frame, S.w8qo, 12);
		memcpy(frame + 3, S.w8qs, 12);
	}
	if (entries && S.w8 && capacity) {
		HIP_TRY(hipSetDevice(c->device));
		HIP_TRY(hipMemcpy(entries, S.w8, (size_t)std::min(capacity, S.num_w8) * sizeof(DW8), hipMemcpyDeviceToHost));
	}
	return RTX_OK;
}

extern "C" int rtx_read_bvh2(rtx_ctx *c, void *records, uint32_t record_capacity, uint32_t *num_nodes, uint32_t *num_prims,
			     uint32_t *root_ref, void *qnodes, uint32_t qnode_capacity, uint32_t *num_qnodes, float qframe[6])
{
	if (!c || !num_nodes || !num_prims || !root_ref || !num_qnodes)
		return fail(RTX_ERR_ARG, "null argument");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_read_bvh2 before rtx_upload_scene");
	const DScene &S = c->scene;
	*num_nodes = S.num_nodes;
	*num_prims = S.num_prims;
	*root_ref = S.root_ref;
	*num_qnodes = S.qnodes ? S.num_qnodes : 0u;
	if (qframe) {
		memcpy(qframe, S.qo, 12);
		memcpy(qframe + 3, S.qs, 12);
	}
	const uint64_t nrec = std::min<uint64_t>(record_capacity, (uint64_t)S.num_nodes + S.num_prims);
	const uint32_t nq = std::min(qnode_capacity, *num_qnodes);
	if ((records && nrec) || (qnodes && nq))
		HIP_TRY(hipSetDevice(c->device));
	if (records && nrec)
		HIP_TRY(hipMemcpy(records, S.nodes, (size_t)nrec * sizeof(DNode), hipMemcpyDeviceToHost));
	if (qnodes && nq)
		HIP_TRY(hipMemcpy(qnodes, S.qnodes, (size_t)nq * sizeof(DQNode), hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* the statistics getters: a copy of one of the context's records */
template <class T> static int get_stats(const rtx_ctx *c, T rtx_ctx::*rec, T *out)
{
	if (!c || !out)
		return fail(RTX_ERR_ARG, "null argument");
	*out = c->*rec;
	return RTX_OK;
}

extern "C" int rtx_get_stats(const rtx_ctx *c, rtx_stats *out) { return get_stats(c, &rtx_ctx::stats, out); }
extern "C" int rtx_get_point_stats(const rtx_ctx *c, rtx_point_stats *out) { return get_stats(c, &rtx_ctx::pstats, out); }
extern "C" int rtx_get_dark_stats(const rtx_ctx *c, rtx_dark_stats *out) { return get_stats(c, &rtx_ctx::dstats, out); }
extern "C" int rtx_get_order_stats(const rtx_ctx *c, rtx_order_stats *out) { return get_stats(c, &rtx_ctx::ostats, out); }
extern "C" int rtx_get_premask_stats(const rtx_ctx *c, rtx_premask_stats *out) { return get_stats(c, &rtx_ctx::mstats, out); }
extern "C" int rtx_get_clearlane_stats(const rtx_ctx *c, rtx_clearlane_stats *out) { return get_stats(c, &rtx_ctx::cstats, out); }
extern "C" int rtx_get_ray_stats(const rtx_ctx *c, rtx_ray_stats *out) { return get_stats(c, &rtx_ctx::ray_stats, out); }
extern "C" int rtx_get_shadow_ray_stats(const rtx_ctx *c, rtx_shadow_ray_stats *out)
{
	return get_stats(c, &rtx_ctx::shadow_ray_stats, out);
}
extern "C" int rtx_get_closest_stats(const rtx_ctx *c, rtx_closest_stats *out) { return get_stats(c, &rtx_ctx::closest_stats, out); }
extern "C" int rtx_get_denoise_stats(const rtx_ctx *c, rtx_denoise_stats *out) { return get_stats(c, &rtx_ctx::dn_stats, out); }
extern "C" int rtx_get_pass_stats(const rtx_ctx *c, rtx_pass_stats *out) { return get_stats(c, &rtx_ctx::pass_stats, out); }
extern "C" int rtx_get_adaptive_stats(const rtx_ctx *c, rtx_adaptive_stats *out) { return get_stats(c, &rtx_ctx::ad_stats, out); }
extern "C" int rtx_get_temporal_stats(const rtx_ctx *c, rtx_temporal_stats *out) { return get_stats(c, &rtx_ctx::tp_stats, out); }

extern "C" int rtx_kat(int kind, uint32_t n, const float *in, float *out, const rtx_params *params)
{
	if (kind < 0 || kind >= RTX_KAT_NKINDS)
		return fail(RTX_ERR_ARG, "bad KAT kind %d", kind);
	if (!n)
		return RTX_OK;
	if (!in || !out)
		return fail(RTX_ERR_ARG, "null buffers");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
		return fail(RTX_ERR_NODEV, "no HIP device available");
	const size_t bi = (size_t)n * rtx_kat_in_width[kind] * 4, bo = (size_t)n * rtx_kat_out_width[kind] * 4;
	DevBuf<float> din, dout;
	HIP_TRY(din.grow(bi));
	if (dout.grow(bo) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "KAT output allocation failed");
	hipError_t e = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = kind >= RTX_KAT_FIRST_SHADOW ? rtx_launch_kat_shadow(kind, n, din, dout, nullptr)
						 : rtx_launch_kat(kind, n, din, dout, params ? params->u32conv : RTX_U32_SAT, nullptr);
	if (e == hipSuccess)
		e = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);
	if (e != hipSuccess)
		return fail(RTX_ERR_HIP, "KAT failed: %s", hipGetErrorString(e));
	return RTX_OK;
}
