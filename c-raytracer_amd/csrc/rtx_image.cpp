/*
 * C-ABI of include/rtx.h, the passes over a finished frame: postprocess (mist, depth of field),
 * the per-pixel feature buffers and the denoiser.
 */
#include <hip/hip_runtime.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"

static int post_common(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_post *pp, float *d_rgb, const float *d_z,
		       hipStream_t stream)
{
	if (!w || !h || (uint64_t)w * h > 0xFFFFFFFFull)
		return fail(RTX_ERR_ARG, "bad postprocess size %ux%u", w, h);
	if (pp->mist && (pp->mist_falloff < RTX_FALLOFF_QUAD || pp->mist_falloff > RTX_FALLOFF_INV_QUAD))
		return fail(RTX_ERR_ARG, "bad mist falloff %d", pp->mist_falloff);
	if (pp->dof < RTX_DOF_NONE || pp->dof > RTX_DOF_CAMERA)
		return fail(RTX_ERR_ARG, "bad dof mode %d", pp->dof);
	const size_t n = (size_t)w * h;
	HIP_TRY(c->d_post_rad.grow(n * sizeof(int)));
	HIP_TRY(c->d_post_pv.grow(n * sizeof(float4)));
	HIP_TRY(c->d_post_scratch.grow(4 * sizeof(unsigned)));
	HIP_TRY(rtx_launch_post(w, h, pp, d_rgb, d_z, c->d_post_rad, c->d_post_pv, c->d_post_scratch, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	return RTX_OK;
}

extern "C" int rtx_postprocess_device(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_post *pp, void *d_rgb,
				      const void *d_z, void *stream)
{
	if (!c || !pp || !d_rgb || !d_z)
		return fail(RTX_ERR_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	return post_common(c, w, h, pp, (float *)d_rgb, (const float *)d_z,
			   stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_postprocess(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_post *pp, float *rgb, const float *z)
{
	if (!c || !pp || !rgb || !z)
		return fail(RTX_ERR_ARG, "null argument");
	if (!w || !h)
		return fail(RTX_ERR_ARG, "bad postprocess size %ux%u", w, h);
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)w * h;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	HIP_TRY(hipMemcpyAsync(c->d_rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->d_z, z, px * 4, hipMemcpyHostToDevice, c->stream));
	int rc = post_common(c, w, h, pp, c->d_rgb, c->d_z, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* ------------------------------------------------------------------------ */
/* denoiser (include/rtx.h rtx_frame_features*, rtx_denoise*)               */
/* ------------------------------------------------------------------------ */
static_assert(sizeof(rtx_feature) == 48, "k_dn_features / k_dn_pack move a feature record as three float4");

static int features_check(rtx_ctx *c, const rtx_frame *fr, int32_t u32conv, const void *features)
{
	if (!c || !fr || !features)
		return fail(RTX_ERR_ARG, "null argument");
	if (!fr->width || !fr->height || (uint64_t)fr->width * fr->height > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad frame %ux%u", fr->width, fr->height);
	if (u32conv != RTX_U32_SAT && u32conv != RTX_U32_WRAP)
		return fail(RTX_ERR_ARG, "bad u32conv %d", u32conv);
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_frame_features before rtx_upload_scene");
	return RTX_OK;
}

/* checked arguments, d_features on the device: n rays (the frame's own, formed here, or with d_rays a caller's), their
 * closest hits, the records */
static int features_body(rtx_ctx *c, const rtx_frame *fr, uint32_t n, const float4 *d_rays, int32_t u32conv, void *d_features,
			 hipStream_t stream)
{
	if ((uintptr_t)d_features & 15u)
		return fail(RTX_ERR_ARG, "feature buffer must be 16-byte aligned");
	if ((!d_rays && c->d_dn_rays.grow((size_t)n * sizeof(rtx_ray)) != hipSuccess) ||
	    c->d_dn_hits.grow((size_t)n * sizeof(rtx_hit)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "rays and hits of %u pixels", n);
	HIP_TRY(hipEventRecord(c->ev0, stream));
	if (!d_rays) {
		const DFrame F = rtx_dframe(fr);
		HIP_TRY(rtx_launch_frame_rays(&F, c->d_dn_rays, stream));
		d_rays = c->d_dn_rays;
	}
	/* the query is the ray queries' own; the caller's rtx_get_ray_stats stays that of their last query */
	const rtx_ray_stats saved = c->ray_stats;
	const int rc = rtx_rays_common(c, n, d_rays, c->d_dn_hits, 0, stream);
	const uint64_t hits = c->ray_stats.hits;
	c->ray_stats = saved;
	if (rc)
		return rc;
	HIP_TRY(rtx_launch_dn_features(n, d_rays, c->d_dn_hits, c->scene.mats, u32conv,
				       (float4 *)d_features, stream));
	HIP_TRY(hipEventRecord(c->ev1, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	c->dn_stats.features_ms = ms;
	c->dn_stats.pixels = n;
	c->dn_stats.hit_pixels = hits;
	return RTX_OK;
}

/* the frame's own rays (the upsampling pipeline's two feature calls too, rtx_upsample.cpp) */
int rtx_features_common(rtx_ctx *c, const rtx_frame *fr, int32_t u32conv, void *d_features, hipStream_t stream)
{
	return features_body(c, fr, fr->width * fr->height, nullptr, u32conv, d_features, stream);
}

/* a caller's rays (rtx_ray_features*, rtx_rays_render.cpp) */
int rtx_ray_features_common(rtx_ctx *c, uint32_t w, uint32_t h, const void *d_rays, int32_t u32conv, void *d_features,
			    hipStream_t stream)
{
	return features_body(c, nullptr, w * h, (const float4 *)d_rays, u32conv, d_features, stream);
}

extern "C" int rtx_frame_features_device(rtx_ctx *c, const rtx_frame *fr, int32_t u32conv, void *d_features, void *stream)
{
	int rc = features_check(c, fr, u32conv, d_features);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return rtx_features_common(c, fr, u32conv, d_features, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_frame_features(rtx_ctx *c, const rtx_frame *fr, int32_t u32conv, rtx_feature *features)
{
	int rc = features_check(c, fr, u32conv, features);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t bytes = (size_t)fr->width * fr->height * sizeof(rtx_feature);
	if (c->d_dn_feat.grow(bytes) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copy of %zu B of features", bytes);
	rc = rtx_features_common(c, fr, u32conv, c->d_dn_feat, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(features, c->d_dn_feat, bytes, hipMemcpyDeviceToHost));
	return RTX_OK;
}

extern "C" void rtx_denoise_params_default(rtx_denoise_params *p)
{
	if (!p)
		return;
	/* chosen on the quality test's frames: raw radiance frames of the golden scenes are of the
	 * order of 1e-4, and beyond one level the blur costs more than the noise it removes at 4 spp */
	p->iterations = 1;
	p->sigma_color = 0.004f;
	p->sigma_normal = 0.05f;
	p->sigma_albedo = 0.1f;
	p->sigma_plane = 0.02f;
}

static int denoise_check(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_params *dp, const void *features, const void *rgb)
{
	if (!c || !dp || !features || !rgb)
		return fail(RTX_ERR_ARG, "null argument");
	if (!w || !h || (uint64_t)w * h > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad denoise size %ux%u", w, h);
	if (dp->iterations < 1 || dp->iterations > 8)
		return fail(RTX_ERR_ARG, "%u denoise iterations outside 1..8", dp->iterations);
	for (float s : { dp->sigma_color, dp->sigma_normal, dp->sigma_albedo, dp->sigma_plane })
		if (!(s > 0.f))
			return fail(RTX_ERR_ARG, "denoise sigma %g is not above 0", (double)s);
	return RTX_OK;
}

/* checked arguments on device buffers */
static int denoise_common(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_params *dp, const void *d_features, void *d_rgb,
			  hipStream_t stream)
{
	if ((uintptr_t)d_features & 15u)
		return fail(RTX_ERR_ARG, "feature buffer must be 16-byte aligned");
	if ((uintptr_t)d_rgb & 3u)
		return fail(RTX_ERR_ARG, "rgb buffer must be 4-byte aligned");
	const size_t n = (size_t)w * h;
	if (c->d_dn_work.grow(5 * n * sizeof(float4)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "denoise work buffers of %zu pixels", n);
	HIP_TRY(c->d_dn_ctr.grow(sizeof(unsigned long long)));
	HIP_TRY(hipMemsetAsync(c->d_dn_ctr, 0, sizeof(unsigned long long), stream));
	HIP_TRY(hipEventRecord(c->ev0, stream));
	HIP_TRY(rtx_launch_denoise(w, h, dp, (const float4 *)d_features, (float *)d_rgb, c->d_dn_work, c->d_dn_ctr, stream));
	HIP_TRY(hipEventRecord(c->ev1, stream));
	unsigned long long hits = 0;
	HIP_TRY(hipMemcpyAsync(&hits, c->d_dn_ctr, sizeof(hits), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	c->dn_stats.filter_ms = ms;
	c->dn_stats.pixels = n;
	c->dn_stats.hit_pixels = hits;
	c->dn_stats.iterations = dp->iterations;
	return RTX_OK;
}

extern "C" int rtx_denoise_device(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_params *dp, const void *d_features,
				  void *d_rgb, void *stream)
{
	int rc = denoise_check(c, w, h, dp, d_features, d_rgb);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return denoise_common(c, w, h, dp, d_features, d_rgb, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_denoise(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_params *dp, const rtx_feature *features, float *rgb)
{
	int rc = denoise_check(c, w, h, dp, features, rgb);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)w * h;
	if (c->d_dn_feat.grow(n * sizeof(rtx_feature)) != hipSuccess || c->d_dn_rgb.grow(n * 3 * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copies of %zu pixels", n);
	HIP_TRY(hipMemcpyAsync(c->d_dn_feat, features, n * sizeof(rtx_feature), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->d_dn_rgb, rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	rc = denoise_common(c, w, h, dp, c->d_dn_feat, c->d_dn_rgb, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(rgb, c->d_dn_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* ------------------------------------------------------------------------ */
/* variance-guided denoiser (include/rtx.h rtx_denoise_variance*)           */
/* ------------------------------------------------------------------------ */
extern "C" void rtx_denoise_variance_params_default(rtx_denoise_variance_params *p)
{
	if (!p)
		return;
	/* chosen by a device sweep over the quality test's frames: sigma_color 1..4 x 1..3 levels, the pair
	 * with the smallest larger ratio of the two frames; the feature sigmas are rtx_denoise's */
	p->iterations = 1;
	p->sigma_color = 3.f;
	p->sigma_normal = 0.05f;
	p->sigma_albedo = 0.1f;
	p->sigma_plane = 0.02f;
}

static int denoise_variance_check(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_variance_params *dp, const void *features,
				  const void *rgb, const void *variance)
{
	if (!c || !dp || !features || !rgb || !variance)
		return fail(RTX_ERR_ARG, "null argument");
	if (!w || !h || (uint64_t)w * h > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad denoise size %ux%u", w, h);
	if (dp->iterations < 1 || dp->iterations > 8)
		return fail(RTX_ERR_ARG, "%u denoise iterations outside 1..8", dp->iterations);
	for (float s : { dp->sigma_color, dp->sigma_normal, dp->sigma_albedo, dp->sigma_plane })
		if (!(s > 0.f))
			return fail(RTX_ERR_ARG, "denoise sigma %g is not above 0", (double)s);
	return RTX_OK;
}

/* checked arguments on device buffers; the records share the scratch rtx_denoise grows */
static int denoise_variance_common(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_variance_params *dp, const void *d_features,
				   void *d_rgb, void *d_variance, hipStream_t stream)
{
	if ((uintptr_t)d_features & 15u)
		return fail(RTX_ERR_ARG, "feature buffer must be 16-byte aligned");
	if (((uintptr_t)d_rgb | (uintptr_t)d_variance) & 3u)
		return fail(RTX_ERR_ARG, "rgb and variance buffers must be 4-byte aligned");
	const size_t n = (size_t)w * h;
	if (c->d_dn_work.grow(7 * n * sizeof(float4)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "denoise work buffers of %zu pixels", n);
	HIP_TRY(c->d_dn_ctr.grow(sizeof(unsigned long long)));
	HIP_TRY(hipMemsetAsync(c->d_dn_ctr, 0, sizeof(unsigned long long), stream));
	HIP_TRY(hipEventRecord(c->ev0, stream));
	HIP_TRY(rtx_launch_denoise_variance(w, h, dp, (const float4 *)d_features, (float *)d_rgb, (float *)d_variance, c->d_dn_work,
					    c->d_dn_ctr, stream));
	HIP_TRY(hipEventRecord(c->ev1, stream));
	unsigned long long hits = 0;
	HIP_TRY(hipMemcpyAsync(&hits, c->d_dn_ctr, sizeof(hits), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	c->dn_stats.filter_ms = ms;
	c->dn_stats.pixels = n;
	c->dn_stats.hit_pixels = hits;
	c->dn_stats.iterations = dp->iterations;
	return RTX_OK;
}

extern "C" int rtx_denoise_variance_device(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_variance_params *dp,
					   const void *d_features, void *d_rgb, void *d_variance, void *stream)
{
	int rc = denoise_variance_check(c, w, h, dp, d_features, d_rgb, d_variance);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return denoise_variance_common(c, w, h, dp, d_features, d_rgb, d_variance, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_denoise_variance(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_denoise_variance_params *dp,
				    const rtx_feature *features, float *rgb, float *variance)
{
	int rc = denoise_variance_check(c, w, h, dp, features, rgb, variance);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)w * h;
	if (c->d_dn_feat.grow(n * sizeof(rtx_feature)) != hipSuccess || c->d_dn_rgb.grow(n * 3 * sizeof(float)) != hipSuccess ||
	    c->d_dn_var.grow(n * 3 * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copies of %zu pixels", n);
	HIP_TRY(hipMemcpyAsync(c->d_dn_feat, features, n * sizeof(rtx_feature), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->d_dn_rgb, rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->d_dn_var, variance, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	rc = denoise_variance_common(c, w, h, dp, c->d_dn_feat, c->d_dn_rgb, c->d_dn_var, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(rgb, c->d_dn_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(variance, c->d_dn_var, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
	return RTX_OK;
}
