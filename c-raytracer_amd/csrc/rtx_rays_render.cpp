/*
 * C-ABI of include/rtx.h, a frame whose primary rays are the caller's: the render of a width x height batch of
 * rtx_ray records (rtx_render_rays*: rtx_render_common with the k_trace instances that read their primary rays) and
 * its feature records (rtx_ray_features*: rtx_frame_features* with the caller's rays in place of the frame's own).
 */
#include <hip/hip_runtime.h>

#include <string.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"

static_assert(sizeof(rtx_ray) == 32, "k_trace loads a primary ray as two float4");

/* what both render entries refuse before anything is launched (the sharding and max_bounces: rtx_render_common) */
static int render_rays_check(rtx_ctx *c, uint32_t w, uint32_t h, const void *rays, const rtx_params *p)
{
	if (!c || !rays || !p)
		return fail(RTX_ERR_ARG, "null argument");
	if (!w || !h || (uint64_t)w * h > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad ray batch %ux%u", w, h);
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_render_rays before rtx_upload_scene");
	return RTX_OK;
}

/* the batch is a width x height image to everything after the primary ray: a frame of that size and no camera */
static rtx_frame rays_frame(uint32_t w, uint32_t h)
{
	rtx_frame fr;
	memset(&fr, 0, sizeof(fr));
	fr.width = w;
	fr.height = h;
	return fr;
}

extern "C" int rtx_render_rays_device(rtx_ctx *c, uint32_t w, uint32_t h, const void *d_rays, const rtx_params *p, void *d_rgb,
				      void *d_z, void *stream)
{
	const int rc = render_rays_check(c, w, h, d_rays, p);
	if (rc)
		return rc;
	if ((uintptr_t)d_rays & 15u)
		return fail(RTX_ERR_ARG, "ray buffer must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	const rtx_frame fr = rays_frame(w, h);
	return rtx_render_common(c, &fr, p, (float *)d_rgb, (float *)d_z, stream ? (hipStream_t)stream : c->stream, nullptr, 0, d_rays);
}

extern "C" int rtx_render_rays(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_ray *rays, const rtx_params *p, float *rgb, float *z)
{
	int rc = render_rays_check(c, w, h, rays, p);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)w * h;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	if (c->d_rr_rays.grow(px * sizeof(rtx_ray)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copy of %zu rays", px);
	HIP_TRY(hipMemcpyAsync(c->d_rr_rays, rays, px * sizeof(rtx_ray), hipMemcpyHostToDevice, c->stream));
	/* pixels of tiles outside this shard keep the caller's values */
	if (p->tile_stride > 1) {
		if (rgb)
			HIP_TRY(hipMemcpyAsync(c->d_rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
		if (z)
			HIP_TRY(hipMemcpyAsync(c->d_z, z, px * 4, hipMemcpyHostToDevice, c->stream));
	}
	const rtx_frame fr = rays_frame(w, h);
	rc = rtx_render_common(c, &fr, p, rgb ? c->d_rgb : nullptr, z ? c->d_z : nullptr, c->stream, nullptr, 0, c->d_rr_rays);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}

static int ray_features_check(rtx_ctx *c, uint32_t w, uint32_t h, const void *rays, int32_t u32conv, const void *features)
{
	if (!c || !rays || !features)
		return fail(RTX_ERR_ARG, "null argument");
	if (!w || !h || (uint64_t)w * h > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad ray batch %ux%u", w, h);
	if (u32conv != RTX_U32_SAT && u32conv != RTX_U32_WRAP)
		return fail(RTX_ERR_ARG, "bad u32conv %d", u32conv);
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_ray_features before rtx_upload_scene");
	return RTX_OK;
}

extern "C" int rtx_ray_features_device(rtx_ctx *c, uint32_t w, uint32_t h, const void *d_rays, int32_t u32conv, void *d_features,
				       void *stream)
{
	const int rc = ray_features_check(c, w, h, d_rays, u32conv, d_features);
	if (rc)
		return rc;
	if ((uintptr_t)d_rays & 15u)
		return fail(RTX_ERR_ARG, "ray buffer must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	return rtx_ray_features_common(c, w, h, d_rays, u32conv, d_features, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_ray_features(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_ray *rays, int32_t u32conv, rtx_feature *features)
{
	int rc = ray_features_check(c, w, h, rays, u32conv, features);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)w * h;
	if (c->d_rr_rays.grow(px * sizeof(rtx_ray)) != hipSuccess || c->d_dn_feat.grow(px * sizeof(rtx_feature)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copies of %zu rays and features", px);
	HIP_TRY(hipMemcpyAsync(c->d_rr_rays, rays, px * sizeof(rtx_ray), hipMemcpyHostToDevice, c->stream));
	rc = rtx_ray_features_common(c, w, h, c->d_rr_rays, u32conv, c->d_dn_feat, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(features, c->d_dn_feat, px * sizeof(rtx_feature), hipMemcpyDeviceToHost));
	return RTX_OK;
}
