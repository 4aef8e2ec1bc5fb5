/*
 * C-ABI of include/rtx.h, feature-guided upsampling with full-resolution tile refinement: the low
 * frame of a frame (host only), the upsampler and the refinement list on caller's buffers (rtx_upsample.hip), and
 * the pipeline that renders the low frame, upsamples it under the guidance of the full frame's feature records and
 * re-renders the tiles of low confidence through the tile-list path.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_tiles.h"

extern "C" void rtx_upsample_params_default(rtx_upsample_params *p)
{
	if (!p)
		return;
	memset(p, 0, sizeof(*p));
	p->scale = 2;
	p->match_material = 1;
	p->demodulate = 0;
	/* the feature sigmas are rtx_denoise's */
	p->sigma_normal = 0.05f;
	p->sigma_albedo = 0.1f;
	p->sigma_plane = 0.02f;
	p->albedo_min = 1.f / 64.f;
	p->refine_threshold = 0.5f;
}

extern "C" int rtx_frame_scaled(const rtx_frame *fr, uint32_t s, rtx_frame *out)
{
	if (!fr || !out)
		return fail(RTX_ERR_ARG, "null argument");
	if (s < 1 || s > RTX_UPSAMPLE_SCALE_MAX)
		return fail(RTX_ERR_ARG, "scale %u outside 1..%u", s, RTX_UPSAMPLE_SCALE_MAX);
	if (!fr->width || !fr->height)
		return fail(RTX_ERR_ARG, "empty frame %ux%u", fr->width, fr->height);
	rtx_frame o = *fr;
	if (s > 1) {
		const double ds = (double)s, cx = (1.0 - ds) / 2.0, cy = (ds - 1.0) / 2.0;
		o.width = (uint32_t)(((uint64_t)fr->width + s - 1) / s);
		o.height = (uint32_t)(((uint64_t)fr->height + s - 1) / s);
		for (int i = 0; i < 3; i++) {
			const double sx = (double)fr->step_x[i], sy = (double)fr->step_y[i];
			o.corner[i] = (float)((double)fr->corner[i] + cx * sx + cy * sy);
			o.step_x[i] = (float)(ds * sx);
			o.step_y[i] = (float)(ds * sy);
		}
	}
	*out = o;
	return RTX_OK;
}

static int up_params_check(const rtx_upsample_params *up)
{
	if (up->scale < 1 || up->scale > RTX_UPSAMPLE_SCALE_MAX)
		return fail(RTX_ERR_ARG, "scale %u outside 1..%u", up->scale, RTX_UPSAMPLE_SCALE_MAX);
	for (float s : { up->sigma_normal, up->sigma_albedo, up->sigma_plane })
		if (!(s > 0.f))
			return fail(RTX_ERR_ARG, "upsample sigma %g is not above 0", (double)s);
	if (!(up->albedo_min > 0.f))
		return fail(RTX_ERR_ARG, "albedo_min %g is not above 0", (double)up->albedo_min);
	return RTX_OK;
}

static int up_size_check(uint32_t w, uint32_t h)
{
	if (!w || !h || (uint64_t)w * h > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad upsample size %ux%u", w, h);
	return RTX_OK;
}

static int upsample_check(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_upsample_params *up, const void *low_rgb, const void *low_feat,
			  const void *feat, const void *rgb)
{
	if (!c || !up || !low_rgb || !low_feat || !feat || !rgb)
		return fail(RTX_ERR_ARG, "null argument");
	const int rc = up_size_check(w, h);
	return rc ? rc : up_params_check(up);
}

static inline uint32_t low_of(uint32_t n, uint32_t s)
{
	return (uint32_t)(((uint64_t)n + s - 1) / s);
}

/* checked arguments on device buffers (16-byte aligned records); the kernel between ev0 and ev1, not synchronised */
static int upsample_enqueue(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_upsample_params *up, const float *d_low_rgb,
			    const float4 *d_low_feat, const float4 *d_feat, float *d_rgb, float *d_conf, hipStream_t stream)
{
	HIP_TRY(hipEventRecord(c->ev0, stream));
	HIP_TRY(rtx_launch_upsample(w, h, up, d_low_rgb, d_low_feat, d_feat, d_rgb, d_conf, stream));
	HIP_TRY(hipEventRecord(c->ev1, stream));
	return RTX_OK;
}

static int upsample_common(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_upsample_params *up, const void *d_low_rgb,
			   const void *d_low_feat, const void *d_feat, void *d_rgb, void *d_conf, hipStream_t stream)
{
	if (((uintptr_t)d_low_feat | (uintptr_t)d_feat) & 15u)
		return fail(RTX_ERR_ARG, "feature buffers must be 16-byte aligned");
	if (((uintptr_t)d_low_rgb | (uintptr_t)d_rgb | (uintptr_t)d_conf) & 3u)
		return fail(RTX_ERR_ARG, "rgb and confidence buffers must be 4-byte aligned");
	int rc = upsample_enqueue(c, w, h, up, (const float *)d_low_rgb, (const float4 *)d_low_feat, (const float4 *)d_feat, (float *)d_rgb,
				  (float *)d_conf, stream);
	if (rc)
		return rc;
	HIP_TRY(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	rtx_upsample_stats us{};
	us.low_width = low_of(w, up->scale);
	us.low_height = low_of(h, up->scale);
	us.upsample_ms = ms;
	c->up_stats = us;
	return RTX_OK;
}

extern "C" int rtx_upsample_device(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_upsample_params *up, const void *d_low_rgb,
				   const void *d_low_feat, const void *d_feat, void *d_rgb, void *d_conf, void *stream)
{
	int rc = upsample_check(c, w, h, up, d_low_rgb, d_low_feat, d_feat, d_rgb);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return upsample_common(c, w, h, up, d_low_rgb, d_low_feat, d_feat, d_rgb, d_conf, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_upsample(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_upsample_params *up, const float *low_rgb,
			    const rtx_feature *low_feat, const rtx_feature *feat, float *rgb, float *conf)
{
	int rc = upsample_check(c, w, h, up, low_rgb, low_feat, feat, rgb);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)w * h, nl = (size_t)low_of(w, up->scale) * low_of(h, up->scale);
	if (c->d_up_low_rgb.grow(nl * 3 * sizeof(float)) != hipSuccess || c->d_up_low_feat.grow(nl * sizeof(rtx_feature)) != hipSuccess ||
	    c->d_up_feat.grow(n * sizeof(rtx_feature)) != hipSuccess || c->d_up_rgb.grow(n * 3 * sizeof(float)) != hipSuccess ||
	    c->d_up_conf.grow(n * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copies of %zu pixels", n);
	HIP_TRY(hipMemcpyAsync(c->d_up_low_rgb, low_rgb, nl * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->d_up_low_feat, low_feat, nl * sizeof(rtx_feature), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(c->d_up_feat, feat, n * sizeof(rtx_feature), hipMemcpyHostToDevice, c->stream));
	rc = upsample_common(c, w, h, up, c->d_up_low_rgb, c->d_up_low_feat, c->d_up_feat, c->d_up_rgb, c->d_up_conf, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(rgb, c->d_up_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
	if (conf)
		HIP_TRY(hipMemcpy(conf, c->d_up_conf, n * sizeof(float), hipMemcpyDeviceToHost));
	return RTX_OK;
}

static int tiles_check(rtx_ctx *c, uint32_t w, uint32_t h, const void *conf, const void *tiles, const uint32_t *n_tiles)
{
	if (!c || !conf || !tiles || !n_tiles)
		return fail(RTX_ERR_ARG, "null argument");
	const int rc = up_size_check(w, h);
	if (rc)
		return rc;
	if (rtx_tiles_total(w, h) > (1ull << 26))
		return fail(RTX_ERR_ARG, "frame %ux%u has more than 2^26 tiles", w, h);
	return RTX_OK;
}

/* the list kernels enqueued, `after` recorded behind them, and their two results read back: the stream is synchronised */
static int tiles_run(rtx_ctx *c, uint32_t w, uint32_t h, const float *d_conf, float threshold, uint32_t *d_list, uint32_t *n_tiles,
		     uint64_t *n_pixels, hipEvent_t after, hipStream_t stream)
{
	const size_t T = (size_t)rtx_tiles_total(w, h);
	if (c->d_up_count.grow(T * sizeof(uint32_t)) != hipSuccess || c->d_up_out.grow(2 * sizeof(unsigned long long)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "tile counts of %zu tiles", T);
	HIP_TRY(rtx_launch_upsample_tiles(w, h, threshold, d_conf, c->d_up_count, d_list, c->d_up_out, stream));
	HIP_TRY(hipEventRecord(after, stream));
	unsigned long long out[2] = { 0, 0 };
	HIP_TRY(hipMemcpyAsync(out, c->d_up_out, sizeof(out), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	*n_tiles = (uint32_t)out[0];
	*n_pixels = out[1];
	return RTX_OK;
}

static int tiles_common(rtx_ctx *c, uint32_t w, uint32_t h, const void *d_conf, float threshold, void *d_tiles, uint32_t *n_tiles,
			hipStream_t stream)
{
	if (((uintptr_t)d_conf | (uintptr_t)d_tiles) & 3u)
		return fail(RTX_ERR_ARG, "the confidence buffer and the tile list must be 4-byte aligned");
	uint64_t pixels = 0;
	HIP_TRY(hipEventRecord(c->ev0, stream));
	int rc = tiles_run(c, w, h, (const float *)d_conf, threshold, (uint32_t *)d_tiles, n_tiles, &pixels, c->ev1, stream);
	if (rc)
		return rc;
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	c->up_stats.tiles = (uint32_t)rtx_tiles_total(w, h);
	c->up_stats.refined_tiles = *n_tiles;
	c->up_stats.low_conf_pixels = pixels;
	c->up_stats.upsample_ms = ms;
	return RTX_OK;
}

extern "C" int rtx_upsample_tiles_device(rtx_ctx *c, uint32_t w, uint32_t h, const void *d_conf, float threshold, void *d_tiles,
					 uint32_t *n_tiles, void *stream)
{
	int rc = tiles_check(c, w, h, d_conf, d_tiles, n_tiles);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return tiles_common(c, w, h, d_conf, threshold, d_tiles, n_tiles, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_upsample_tiles(rtx_ctx *c, uint32_t w, uint32_t h, const float *conf, float threshold, uint32_t *tiles,
				  uint32_t *n_tiles)
{
	int rc = tiles_check(c, w, h, conf, tiles, n_tiles);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)w * h, T = (size_t)rtx_tiles_total(w, h);
	if (c->d_up_conf.grow(n * sizeof(float)) != hipSuccess || c->d_up_list.grow(T * sizeof(uint32_t)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copies of %zu pixels", n);
	HIP_TRY(hipMemcpyAsync(c->d_up_conf, conf, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
	rc = tiles_common(c, w, h, c->d_up_conf, threshold, c->d_up_list, n_tiles, c->stream);
	if (rc)
		return rc;
	if (*n_tiles)
		HIP_TRY(hipMemcpy(tiles, c->d_up_list, (size_t)*n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* everything rtx_render_upsampled* refuses before it launches anything */
static int upsampled_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_upsample_params *up)
{
	if (!c || !fr || !p || !up)
		return fail(RTX_ERR_ARG, "null argument");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_render_upsampled before rtx_upload_scene");
	int rc = up_size_check(fr->width, fr->height);
	if (rc)
		return rc;
	if (rtx_tiles_total(fr->width, fr->height) > (1ull << 26))
		return fail(RTX_ERR_ARG, "frame %ux%u has more than 2^26 tiles", fr->width, fr->height);
	if (p->tile_offset != 0 || p->tile_stride != 1)
		return fail(RTX_ERR_ARG, "rtx_render_upsampled renders whole frames: tile sharding %u/%u is not 0/1", p->tile_offset,
			    p->tile_stride);
	if (p->max_bounces > RTX_MAX_BOUNCES)
		return fail(RTX_ERR_ARG, "max_bounces %u above the supported %u", p->max_bounces, RTX_MAX_BOUNCES);
	if (p->u32conv != RTX_U32_SAT && p->u32conv != RTX_U32_WRAP)
		return fail(RTX_ERR_ARG, "bad u32conv %d", p->u32conv);
	return up_params_check(up);
}

/* checked arguments, device outputs (either may be null) */
static int upsampled_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_upsample_params *up, float *d_rgb,
			    float *d_z, hipStream_t stream)
{
	rtx_frame low;
	int rc = rtx_frame_scaled(fr, up->scale, &low);
	if (rc)
		return rc;
	const uint32_t w = fr->width, h = fr->height;
	const size_t n = (size_t)w * h, nl = (size_t)low.width * low.height, T = (size_t)rtx_tiles_total(w, h);
	if (c->d_up_low_rgb.grow(nl * 3 * sizeof(float)) != hipSuccess || c->d_up_low_feat.grow(nl * sizeof(rtx_feature)) != hipSuccess ||
	    c->d_up_feat.grow(n * sizeof(rtx_feature)) != hipSuccess || c->d_up_conf.grow(n * sizeof(float)) != hipSuccess ||
	    c->d_up_list.grow(T * sizeof(uint32_t)) != hipSuccess || (!d_rgb && c->d_up_rgb.grow(n * 3 * sizeof(float)) != hipSuccess))
		return fail(RTX_ERR_NOMEM, "upsampling buffers of %zu pixels", n);
	if (!d_rgb)
		d_rgb = c->d_up_rgb;
	rtx_upsample_stats us{};
	us.low_width = low.width;
	us.low_height = low.height;
	us.tiles = (uint32_t)T;
	/* the low frame, as rtx_render renders it */
	rc = rtx_render_common(c, &low, p, c->d_up_low_rgb, nullptr, stream);
	if (rc)
		return rc;
	us.low_ms = c->stats.kernel_ms;
	us.closest_rays = c->stats.closest_rays;
	us.shadow_rays = c->stats.shadow_rays;
	/* the records of both frames; rtx_get_denoise_stats is left describing the full frame's */
	rc = rtx_features_common(c, &low, p->u32conv, c->d_up_low_feat, stream);
	if (rc)
		return rc;
	us.features_ms = c->dn_stats.features_ms;
	rc = rtx_features_common(c, fr, p->u32conv, c->d_up_feat, stream);
	if (rc)
		return rc;
	us.features_ms += c->dn_stats.features_ms;
	/* the upsample into the caller's rgb, z from the full frame's records, the list */
	rc = upsample_enqueue(c, w, h, up, c->d_up_low_rgb, c->d_up_low_feat, c->d_up_feat, d_rgb, c->d_up_conf, stream);
	if (rc)
		return rc;
	if (d_z)
		HIP_TRY(rtx_launch_upsample_z(n, c->d_up_feat, d_z, stream));
	uint32_t n_tiles = 0;
	rc = tiles_run(c, w, h, c->d_up_conf, up->refine_threshold, c->d_up_list, &n_tiles, &us.low_conf_pixels, c->ev[0], stream);
	if (rc)
		return rc;
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev[0]));
	us.upsample_ms = ms;
	us.refined_tiles = n_tiles;
	/* the tiles of low confidence at full resolution: the list is increasing and in range by construction */
	if (n_tiles) {
		rc = rtx_render_common(c, fr, p, d_rgb, d_z, stream, c->d_up_list, n_tiles);
		if (rc)
			return rc;
		us.refine_ms = c->stats.kernel_ms;
		us.closest_rays += c->stats.closest_rays;
		us.shadow_rays += c->stats.shadow_rays;
	}
	c->up_stats = us;
	return RTX_OK;
}

extern "C" int rtx_render_upsampled_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_upsample_params *up,
					   void *d_rgb, void *d_z, void *stream)
{
	int rc = upsampled_check(c, fr, p, up);
	if (rc)
		return rc;
	if (((uintptr_t)d_rgb | (uintptr_t)d_z) & 15u)
		return fail(RTX_ERR_ARG, "output buffers must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	return upsampled_common(c, fr, p, up, (float *)d_rgb, (float *)d_z, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_render_upsampled(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_upsample_params *up, float *rgb,
				    float *z)
{
	int rc = upsampled_check(c, fr, p, up);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	rc = upsampled_common(c, fr, p, up, rgb ? c->d_rgb.p : nullptr, z ? c->d_z.p : nullptr, c->stream);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}

extern "C" int rtx_get_upsample_stats(const rtx_ctx *c, rtx_upsample_stats *out)
{
	if (!c || !out)
		return fail(RTX_ERR_ARG, "null argument");
	*out = c->up_stats;
	return RTX_OK;
}
