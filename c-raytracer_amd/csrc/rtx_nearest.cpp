/*
 * C-ABI of include/rtx.h, the closest-point queries: the definition on the host
 * (rtx_closest_point_object), the query on caller-supplied batches (rtx_closest_points*) and the
 * device's known answers of the definition (rtx_closest_kat*).  DESIGN 7.11.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_nearest_math.h"

static_assert(sizeof(rtx_point_query) == 16 && sizeof(rtx_closest) == 32, "k_nearest moves a query as one float4, a result as two");

extern "C" int rtx_closest_point_object(const rtx_object *obj, const float P[3], float *dist, float cp[3])
{
	if (!obj || !P || !dist || !cp)
		return fail(RTX_ERR_ARG, "null argument");
	switch (obj->type) {
	case RTX_SPHERE:
		rtx_nm_sphere(obj->p0, obj->radius, P, dist, cp);
		return RTX_OK;
	case RTX_TRIANGLE:
		rtx_nm_triangle(obj->p0, obj->e1, obj->e2, P, dist, cp);
		return RTX_OK;
	case RTX_PLANE:
		rtx_nm_plane(obj->n, obj->d, P, dist, cp);
		return RTX_OK;
	default:
		return fail(RTX_ERR_ARG, "unknown object type %d", obj->type);
	}
}

static int closest_check(rtx_ctx *c, uint64_t n, const void *queries, const void *results, uint32_t flags)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null context");
	if (flags & ~(uint32_t)(RTX_CLOSEST_BOUNDED_ONLY | RTX_CLOSEST_REORDER | RTX_CLOSEST_COUNT))
		return fail(RTX_ERR_ARG, "unknown closest-point flags 0x%x", flags);
	if (n > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "%llu points above the supported %u per call", (unsigned long long)n, RTX_RAYS_MAX);
	if (n && (!queries || !results))
		return fail(RTX_ERR_ARG, "null query / result buffer");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_closest_points before rtx_upload_scene");
	return RTX_OK;
}

/* n checked queries on device buffers; touches none of the render's state but grow-only scratch */
static int closest_common(rtx_ctx *c, uint32_t n, const void *d_queries, void *d_results, uint32_t flags, hipStream_t stream)
{
	rtx_closest_stats cs{};
	if (!n) {
		c->closest_stats = cs;
		return RTX_OK;
	}
	if (((uintptr_t)d_queries | (uintptr_t)d_results) & 15u)
		return fail(RTX_ERR_ARG, "query / result buffers must be 16-byte aligned");
	DScene S = c->scene;
	int per_cu = 0;
	HIP_TRY(rtx_nearest_occupancy(S.stack_size, &per_cu));
	if (per_cu <= 0)
		return fail(RTX_ERR_HIP, "closest-point kernel does not fit (LDS %zu B)", rtx_nearest_lds_bytes(S.stack_size));
	const uint32_t packets = (uint32_t)(((uint64_t)n + 63) / 64);
	const uint32_t waves = (uint32_t)std::min<uint64_t>((uint64_t)per_cu * c->cus, packets);
	hipError_t e = rtx_ensure_ostk(c, waves); /* for THIS grid */
	if (e != hipSuccess)
		return fail(RTX_ERR_NOMEM, "lane-stack overflow buffer: %s", hipGetErrorString(e));
	S.ostk = c->d_ostk;
	HIP_TRY(rtx_reset_query_counters(c, stream));
	HIP_TRY(hipEventRecord(c->ev[0], stream));
	const uint32_t *perm = nullptr;
	if ((flags & RTX_CLOSEST_REORDER) && n > 64) { /* one packet has no order to improve */
		size_t tmp = 0;
		HIP_TRY(rtx_pointsort_temp_bytes(n, &tmp));
		e = c->d_sortbuf.grow((size_t)n * 4 * sizeof(uint32_t));
		if (e == hipSuccess)
			e = c->d_sorttmp.grow(tmp);
		if (e != hipSuccess)
			return fail(RTX_ERR_NOMEM, "point sort buffers: %s", hipGetErrorString(e));
		uint32_t *b = c->d_sortbuf;
		const size_t q = n;
		HIP_TRY(rtx_launch_pointsort((const float4 *)d_queries, n, c->bound_lo, c->bound_hi, b, b + q, b + 2 * q, b + 3 * q,
					     c->d_sorttmp, c->d_sorttmp.bytes, &perm, stream));
	}
	HIP_TRY(hipEventRecord(c->ev[1], stream));
	/* the bounded objects' largest coordinate magnitude: the scale of the search bound's slack */
	float wmag = 0.f;
	for (int a = 0; a < 3; a++)
		wmag = std::max(wmag, std::max(std::fabs(c->bound_lo[a]), std::fabs(c->bound_hi[a])));
	const uint32_t grab = std::max<uint32_t>(1, std::min<uint32_t>(4, packets / (waves * 16)));
	const uint32_t queues = std::min<uint32_t>(RTX_RQ_MAX_QUEUES, waves);
	HIP_TRY(rtx_launch_nearest(&S, (const float4 *)d_queries, (float4 *)d_results, perm, n, queues, grab, wmag,
				   (flags & RTX_CLOSEST_BOUNDED_ONLY) != 0, c->d_rctr, waves, (flags & RTX_CLOSEST_COUNT) != 0, stream));
	HIP_TRY(hipEventRecord(c->ev[4], stream));
	unsigned long long ctr[RTX_NQ_N];
	HIP_TRY(hipMemcpyAsync(ctr, c->d_rctr, sizeof(ctr), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float so = 0, k = 0;
	HIP_TRY(hipEventElapsedTime(&so, c->ev[0], c->ev[1]));
	HIP_TRY(hipEventElapsedTime(&k, c->ev[1], c->ev[4]));
	cs.points = n;
	cs.found = ctr[RTX_NQ_FOUND];
	cs.node_visits = ctr[RTX_NQ_NODES];
	cs.tri_tests = ctr[RTX_NQ_TRIS];
	cs.sphere_tests = ctr[RTX_NQ_SPHERES];
	cs.plane_tests = ctr[RTX_NQ_PLANES];
	cs.far_points = ctr[RTX_NQ_FAR];
	cs.kernel_ms = k;
	cs.sort_ms = perm ? so : 0.0;
	c->closest_stats = cs;
	return RTX_OK;
}

extern "C" int rtx_closest_points_device(rtx_ctx *c, uint64_t n, const void *d_queries, void *d_results, uint32_t flags, void *stream)
{
	int rc = closest_check(c, n, d_queries, d_results, flags);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return closest_common(c, (uint32_t)n, d_queries, d_results, flags, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_closest_points(rtx_ctx *c, uint64_t n, const rtx_point_query *queries, rtx_closest *results, uint32_t flags)
{
	int rc = closest_check(c, n, queries, results, flags);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	if (n) {
		if (c->d_qrays.grow((size_t)n * sizeof(rtx_point_query)) != hipSuccess ||
		    c->d_qhits.grow((size_t)n * sizeof(rtx_closest)) != hipSuccess)
			return fail(RTX_ERR_NOMEM, "device copies of %llu points", (unsigned long long)n);
		HIP_TRY(hipMemcpyAsync(c->d_qrays, queries, (size_t)n * sizeof(rtx_point_query), hipMemcpyHostToDevice, c->stream));
	}
	rc = closest_common(c, (uint32_t)n, c->d_qrays, c->d_qhits, flags, c->stream);
	if (rc)
		return rc;
	if (n)
		HIP_TRY(hipMemcpy(results, c->d_qhits, (size_t)n * sizeof(rtx_closest), hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* ------------------------------------------------------------------------ */
/* known answers                                                            */
/* ------------------------------------------------------------------------ */
static int kat_device(void)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
		return fail(RTX_ERR_NODEV, "no HIP device available");
	return RTX_OK;
}

extern "C" int rtx_closest_kat(uint32_t n_objects, const rtx_object *objects, uint64_t n, const uint32_t *object_index,
			       const float *points, float *out)
{
	if (n > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "%llu pairs above the supported %u per call", (unsigned long long)n, RTX_RAYS_MAX);
	if (!n)
		return RTX_OK;
	if (!objects || !points || !out)
		return fail(RTX_ERR_ARG, "null buffers");
	if (!object_index && n > n_objects)
		return fail(RTX_ERR_ARG, "%llu pairs of %u objects without an index list", (unsigned long long)n, n_objects);
	for (uint64_t i = 0; object_index && i < n; i++)
		if (object_index[i] >= n_objects)
			return fail(RTX_ERR_ARG, "pair %llu: object %u out of range", (unsigned long long)i, object_index[i]);
	for (uint32_t o = 0; o < n_objects; o++)
		if (objects[o].type != RTX_SPHERE && objects[o].type != RTX_TRIANGLE && objects[o].type != RTX_PLANE)
			return fail(RTX_ERR_ARG, "object %u: unknown type %d", o, objects[o].type);
	int rc = kat_device();
	if (rc)
		return rc;
	DevBuf<rtx_object> dobj;
	DevBuf<uint32_t> didx;
	DevBuf<float> dpts;
	DevBuf<float4> dout;
	if (dobj.grow((size_t)n_objects * sizeof(rtx_object)) != hipSuccess || (object_index && didx.grow(n * sizeof(uint32_t)) != hipSuccess) ||
	    dpts.grow(n * 3 * sizeof(float)) != hipSuccess || dout.grow(n * sizeof(float4)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "KAT buffers");
	hipError_t e = hipMemcpy(dobj, objects, (size_t)n_objects * sizeof(rtx_object), hipMemcpyHostToDevice);
	if (e == hipSuccess && object_index)
		e = hipMemcpy(didx, object_index, n * sizeof(uint32_t), hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = hipMemcpy(dpts, points, n * 3 * sizeof(float), hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = rtx_launch_nearest_kat(dobj, object_index ? didx.p : nullptr, dpts, n, dout, nullptr);
	if (e == hipSuccess)
		e = hipMemcpy(out, dout, n * sizeof(float4), hipMemcpyDeviceToHost);
	if (e != hipSuccess)
		return fail(RTX_ERR_HIP, "KAT failed: %s", hipGetErrorString(e));
	return RTX_OK;
}

extern "C" int rtx_closest_kat_grid(uint32_t n_objects, const rtx_object *objects, uint32_t n_points, const float *points, float *dist)
{
	const uint64_t n = (uint64_t)n_objects * n_points;
	if (n > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "%llu pairs above the supported %u per call", (unsigned long long)n, RTX_RAYS_MAX);
	if (!n)
		return RTX_OK;
	if (!objects || !points || !dist)
		return fail(RTX_ERR_ARG, "null buffers");
	for (uint32_t o = 0; o < n_objects; o++)
		if (objects[o].type != RTX_SPHERE && objects[o].type != RTX_TRIANGLE && objects[o].type != RTX_PLANE)
			return fail(RTX_ERR_ARG, "object %u: unknown type %d", o, objects[o].type);
	int rc = kat_device();
	if (rc)
		return rc;
	DevBuf<rtx_object> dobj;
	DevBuf<float> dpts, dout;
	if (dobj.grow((size_t)n_objects * sizeof(rtx_object)) != hipSuccess || dpts.grow((size_t)n_points * 3 * sizeof(float)) != hipSuccess ||
	    dout.grow(n * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "KAT buffers");
	hipError_t e = hipMemcpy(dobj, objects, (size_t)n_objects * sizeof(rtx_object), hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = hipMemcpy(dpts, points, (size_t)n_points * 3 * sizeof(float), hipMemcpyHostToDevice);
	if (e == hipSuccess)
		e = rtx_launch_nearest_grid(dobj, n_objects, dpts, n_points, dout, nullptr);
	if (e == hipSuccess)
		e = hipMemcpy(dist, dout, n * sizeof(float), hipMemcpyDeviceToHost);
	if (e != hipSuccess)
		return fail(RTX_ERR_HIP, "KAT failed: %s", hipGetErrorString(e));
	return RTX_OK;
}
