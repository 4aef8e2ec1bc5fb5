/*
 * C-ABI of include/rtx.h, the queries on caller-supplied batches: closest and any hit
 * (rtx_trace_rays*), shadow rays (rtx_trace_shadow_rays), and a frame's rays (rtx_frame_rays_device).
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"

/* ------------------------------------------------------------------------ */
/* ray queries (include/rtx.h rtx_trace_rays*)                              */
/* ------------------------------------------------------------------------ */
static_assert(sizeof(rtx_ray) == 32 && sizeof(rtx_hit) == 32, "k_rays moves a ray / a hit as two float4");

static int rays_check(rtx_ctx *c, uint64_t n, const void *rays, const void *hits, uint32_t flags)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null context");
	if (flags & ~(uint32_t)(RTX_RAYS_ANY_HIT | RTX_RAYS_REORDER | RTX_RAYS_COUNT))
		return fail(RTX_ERR_ARG, "unknown ray-query flags 0x%x", flags);
	if (n > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "%llu rays above the supported %u per call", (unsigned long long)n, RTX_RAYS_MAX);
	if (n && (!rays || !hits))
		return fail(RTX_ERR_ARG, "null ray / hit buffer");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_trace_rays before rtx_upload_scene");
	return RTX_OK;
}

/* n checked rays on device buffers; touches none of the render's state but grow-only scratch */
int rtx_rays_common(rtx_ctx *c, uint32_t n, const void *d_rays, void *d_hits, uint32_t flags, hipStream_t stream)
{
	rtx_ray_stats rs{};
	if (!n) {
		c->ray_stats = rs;
		return RTX_OK;
	}
	if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u)
		return fail(RTX_ERR_ARG, "ray / hit buffers must be 16-byte aligned");
	DScene S = c->scene; /* the render sets its own copy's walk and stack fields at every render */
	S.trace_w8 = (S.w8 && c->opt_trace_walk != RTX_WALK_BVH2) ? 1u : 0u;
	int per_cu = 0;
	HIP_TRY(rtx_rays_occupancy(S.stack_size, &per_cu));
	if (per_cu <= 0)
		return fail(RTX_ERR_HIP, "ray-query kernel does not fit (LDS %zu B)", rtx_rays_lds_bytes(S.stack_size));
	const uint32_t packets = (uint32_t)(((uint64_t)n + 63) / 64);
	const uint32_t waves = (uint32_t)std::min<uint64_t>((uint64_t)per_cu * c->cus, packets);
	hipError_t e = rtx_ensure_ostk(c, waves); /* for THIS grid */
	if (e != hipSuccess)
		return fail(RTX_ERR_NOMEM, "lane-stack overflow buffer: %s", hipGetErrorString(e));
	S.ostk = c->d_ostk;
	HIP_TRY(rtx_reset_query_counters(c, stream));
	HIP_TRY(hipEventRecord(c->ev[0], stream));
	const uint32_t *perm = nullptr;
	if ((flags & RTX_RAYS_REORDER) && n > 64) { /* one packet has no order to improve */
		size_t tmp = 0;
		HIP_TRY(rtx_raysort_temp_bytes(n, &tmp));
		e = c->d_sortbuf.grow((size_t)n * 4 * sizeof(uint32_t));
		if (e == hipSuccess)
			e = c->d_sorttmp.grow(tmp);
		if (e != hipSuccess)
			return fail(RTX_ERR_NOMEM, "ray sort buffers: %s", hipGetErrorString(e));
		uint32_t *b = c->d_sortbuf;
		const size_t q = n;
		HIP_TRY(rtx_launch_raysort((const float4 *)d_rays, n, c->bound_lo, c->bound_hi, b, b + q, b + 2 * q, b + 3 * q,
					   c->d_sorttmp, c->d_sorttmp.bytes, &perm, stream));
	}
	HIP_TRY(hipEventRecord(c->ev[1], stream));
	/* one queue per XCD's share of the waves (one counter serves ~80 M grabs a second, which bounds a
	 * query of any size: 33 M rays took 6.5 ms with one queue, 1.2 ms with eight); packets per grab:
	 * one, and up to four once a wave has 16 packets or more to take (longer grabs only lengthen the
	 * tail: 2 M permuted rays 0.37 ms at 1, 0.72 ms at 16) */
	const uint32_t grab = c->opt_rays_grab ? c->opt_rays_grab : std::max<uint32_t>(1, std::min<uint32_t>(4, packets / (waves * 16)));
	const uint32_t queues = std::min<uint32_t>(c->opt_rays_queues ? c->opt_rays_queues : RTX_RQ_MAX_QUEUES, waves);
	HIP_TRY(rtx_launch_rays(&S, (const float4 *)d_rays, (float4 *)d_hits, perm, n, queues, grab, c->d_rctr, waves,
				(flags & RTX_RAYS_COUNT) != 0, (flags & RTX_RAYS_ANY_HIT) != 0, stream));
	HIP_TRY(hipEventRecord(c->ev[4], stream));
	unsigned long long ctr[RTX_RQ_STATS];
	HIP_TRY(hipMemcpyAsync(ctr, c->d_rctr, sizeof(ctr), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float so = 0, k = 0;
	HIP_TRY(hipEventElapsedTime(&so, c->ev[0], c->ev[1]));
	HIP_TRY(hipEventElapsedTime(&k, c->ev[1], c->ev[4]));
	rs.rays = n;
	rs.hits = ctr[RTX_RQ_HITS];
	rs.node_visits = ctr[RTX_RQ_NODES];
	rs.tri_tests = ctr[RTX_RQ_TRIS];
	rs.sphere_tests = ctr[RTX_RQ_SPHERES];
	rs.plane_tests = ctr[RTX_RQ_PLANES];
	rs.far_rays = ctr[RTX_RQ_FAR];
	rs.kernel_ms = k;
	rs.sort_ms = perm ? so : 0.0;
	c->ray_stats = rs;
	return RTX_OK;
}

extern "C" int rtx_trace_rays_device(rtx_ctx *c, uint64_t n, const void *d_rays, void *d_hits, uint32_t flags, void *stream)
{
	int rc = rays_check(c, n, d_rays, d_hits, flags);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return rtx_rays_common(c, (uint32_t)n, d_rays, d_hits, flags, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_trace_rays(rtx_ctx *c, uint64_t n, const rtx_ray *rays, rtx_hit *hits, uint32_t flags)
{
	int rc = rays_check(c, n, rays, hits, flags);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	if (n) {
		if (c->d_qrays.grow((size_t)n * sizeof(rtx_ray)) != hipSuccess || c->d_qhits.grow((size_t)n * sizeof(rtx_hit)) != hipSuccess)
			return fail(RTX_ERR_NOMEM, "device copies of %llu rays", (unsigned long long)n);
		HIP_TRY(hipMemcpyAsync(c->d_qrays, rays, (size_t)n * sizeof(rtx_ray), hipMemcpyHostToDevice, c->stream));
	}
	rc = rtx_rays_common(c, (uint32_t)n, c->d_qrays, c->d_qhits, flags, c->stream);
	if (rc)
		return rc;
	if (n)
		HIP_TRY(hipMemcpy(hits, c->d_qhits, (size_t)n * sizeof(rtx_hit), hipMemcpyDeviceToHost));
	return RTX_OK;
}

extern "C" int rtx_frame_rays_device(rtx_ctx *c, const rtx_frame *fr, void *d_rays, void *stream)
{
	if (!c || !fr || !d_rays)
		return fail(RTX_ERR_ARG, "null argument");
	if (!fr->width || !fr->height || (uint64_t)fr->width * fr->height > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad frame %ux%u", fr->width, fr->height);
	if ((uintptr_t)d_rays & 15u)
		return fail(RTX_ERR_ARG, "ray buffer must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	const DFrame F = rtx_dframe(fr);
	hipStream_t st = stream ? (hipStream_t)stream : c->stream;
	HIP_TRY(rtx_launch_frame_rays(&F, (float4 *)d_rays, st));
	HIP_TRY(hipStreamSynchronize(st));
	return RTX_OK;
}

/* ------------------------------------------------------------------------ */
/* shadow queries (include/rtx.h rtx_trace_shadow_rays)                     */
/* ------------------------------------------------------------------------ */
static_assert(sizeof(rtx_shadow_ray) == 32 && sizeof(rtx_shadow_result) == 16, "k_shadow_rays moves a ray as two float4, a result as one");

extern "C" int rtx_trace_shadow_rays(rtx_ctx *c, uint64_t n, const rtx_shadow_ray *rays, rtx_shadow_result *results, uint32_t flags)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null context");
	if (flags & ~(uint32_t)(RTX_SHADOW_RAYS_SLOTS | RTX_SHADOW_RAYS_COUNT))
		return fail(RTX_ERR_ARG, "unknown shadow-query flags 0x%x", flags);
	if (n > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "%llu rays above the supported %u per call", (unsigned long long)n, RTX_RAYS_MAX);
	if (n && (!rays || !results))
		return fail(RTX_ERR_ARG, "null shadow ray / result buffer");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_trace_shadow_rays before rtx_upload_scene");
	rtx_shadow_ray_stats rs{};
	if (!n) {
		c->shadow_ray_stats = rs;
		return RTX_OK;
	}
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t stream = c->stream;
	if (c->d_qrays.grow((size_t)n * sizeof(rtx_shadow_ray)) != hipSuccess ||
	    c->d_qhits.grow((size_t)n * sizeof(rtx_shadow_result)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copies of %llu shadow rays", (unsigned long long)n);
	HIP_TRY(hipMemcpyAsync(c->d_qrays, rays, (size_t)n * sizeof(rtx_shadow_ray), hipMemcpyHostToDevice, stream));
	/* the walk's LDS stack size and spill area as a render sets them (it does so at every render, in
	 * the context's scene; a query may come first, so it sets its own copy) */
	DScene S = c->scene;
	bool alloc;
	const hipError_t e = rtx_ensure_w8spill(c, S, &alloc);
	if (e != hipSuccess)
		return alloc ? fail(RTX_ERR_NOMEM, "lane-stack spill area: %s", hipGetErrorString(e))
			     : fail(RTX_ERR_HIP, "rtx_shadow_grid_lanes failed: %s", hipGetErrorString(e));
	HIP_TRY(rtx_reset_query_counters(c, stream));
	HIP_TRY(hipEventRecord(c->ev[0], stream));
	HIP_TRY(rtx_launch_shadow_rays(&S, c->d_qrays, c->d_qhits, (uint32_t)n, c->d_rctr,
				       (flags & RTX_SHADOW_RAYS_SLOTS) != 0, (flags & RTX_SHADOW_RAYS_COUNT) != 0, (uint32_t)c->cus, stream));
	HIP_TRY(hipEventRecord(c->ev[1], stream));
	unsigned long long ctr[RTX_SQ_N];
	HIP_TRY(hipMemcpyAsync(ctr, c->d_rctr, sizeof(ctr), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(results, c->d_qhits, (size_t)n * sizeof(rtx_shadow_result), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float k = 0;
	HIP_TRY(hipEventElapsedTime(&k, c->ev[0], c->ev[1]));
	rs.rays = ctr[RTX_SQ_RAYS];
	rs.blocked = ctr[RTX_SQ_BLOCKED];
	rs.far_rays = ctr[RTX_SQ_FAR];
	rs.box_tests = ctr[RTX_SQ_BOXES];
	rs.tri_tests = ctr[RTX_SQ_TRIS];
	rs.sphere_tests = ctr[RTX_SQ_SPHERES];
	rs.wave_steps = ctr[RTX_SQ_STEPS];
	rs.uniform_steps = ctr[RTX_SQ_UNIF];
	rs.leaf_rounds = ctr[RTX_SQ_LEAFR];
	rs.stack_spills = ctr[RTX_SQ_SPILL];
	rs.kernel_ms = k;
	c->shadow_ray_stats = rs;
	return RTX_OK;
}
