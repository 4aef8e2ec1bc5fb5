/*
 * C-ABI of include/rtx.h, multi-pass rendering: the frame of pass k (host only), and the frame
 * rendered pass by pass through the render's own path, each pass folded on the device into a per-pixel mean
 * and the variance of that mean (rtx_passes.hip); and adaptive passes, in which each pass renders the tiles still
 * over their share of the error budget through the tile-list path (rtx_adaptive.hip).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_tiles.h"

extern "C" void rtx_pass_params_default(rtx_pass_params *p)
{
	if (!p)
		return;
	memset(p, 0, sizeof(*p));
	p->passes = 1;
	p->flags = 0;
	p->aperture = 0.f;
	p->focus = 1.f;
	p->target_error = 0.f;
	p->min_passes = 2;
}

/* the radical inverse of k in base b */
static double radical_inverse(uint32_t k, uint32_t b)
{
	const double inv = 1.0 / (double)b;
	double f = inv, r = 0.0;
	for (; k; k /= b, f *= inv)
		r += (double)(k % b) * f;
	return r;
}

/* what rtx_pass_frame refuses about the pass parameters alone (rtx_pass_filter_weights too, rtx_filter.cpp) */
int rtx_pass_params_check(const rtx_pass_params *pp)
{
	if (pp->passes < 1 || pp->passes > RTX_PASSES_MAX)
		return fail(RTX_ERR_ARG, "%u passes outside 1..%u", pp->passes, RTX_PASSES_MAX);
	if (pp->flags & ~(uint32_t)RTX_PASS_JITTER)
		return fail(RTX_ERR_ARG, "unknown pass flags 0x%x", pp->flags);
	if (!(pp->aperture >= 0.f))
		return fail(RTX_ERR_ARG, "aperture %g is negative or NaN", (double)pp->aperture);
	if (pp->aperture > 0.f && !(pp->focus > 0.f && pp->focus < INFINITY))
		return fail(RTX_ERR_ARG, "focus %g is not a finite value above 0", (double)pp->focus);
	if (!(pp->target_error >= 0.f))
		return fail(RTX_ERR_ARG, "target error %g is negative or NaN", (double)pp->target_error);
	if (pp->target_error > 0.f && (pp->min_passes < 2 || pp->min_passes > pp->passes))
		return fail(RTX_ERR_ARG, "min_passes %u outside 2..%u", pp->min_passes, pp->passes);
	return RTX_OK;
}

/* pass k's sub-pixel offset in pixel units: what rtx_pass_frame moves the corner by, and what the reconstruction
 * filter's weights are evaluated at (rtx_filter.cpp) */
void rtx_pass_offset(const rtx_pass_params *pp, uint32_t k, double *ox, double *oy)
{
	const bool jitter = (pp->flags & RTX_PASS_JITTER) && k != 0;
	*ox = jitter ? radical_inverse(k, 2) - 0.5 : 0.0;
	*oy = jitter ? radical_inverse(k, 3) - 0.5 : 0.0;
}

extern "C" int rtx_pass_frame(const rtx_frame *fr, const rtx_pass_params *pp, uint32_t k, rtx_frame *out)
{
	if (!fr || !pp || !out)
		return fail(RTX_ERR_ARG, "null argument");
	int rc = rtx_pass_params_check(pp);
	if (rc)
		return rc;
	if (k >= pp->passes)
		return fail(RTX_ERR_ARG, "pass %u of %u", k, pp->passes);
	const bool lens = pp->aperture > 0.f;
	double sx[3], sy[3], lx = 0.0, ly = 0.0;
	for (int i = 0; i < 3; i++) {
		sx[i] = (double)fr->step_x[i];
		sy[i] = (double)fr->step_y[i];
		lx += sx[i] * sx[i];
		ly += sy[i] * sy[i];
	}
	if (lens && !(lx > 0.0 && ly > 0.0))
		return fail(RTX_ERR_ARG, "a thin lens needs step_x and step_y of a length above 0");
	rtx_frame o = *fr;
	/* the corner in double: the offset-free one keeps the input's value (and, for a pinhole, its bits) */
	double cj[3];
	const bool jitter = (pp->flags & RTX_PASS_JITTER) && k != 0;
	double ox, oy;
	rtx_pass_offset(pp, k, &ox, &oy);
	for (int i = 0; i < 3; i++)
		cj[i] = jitter ? (double)fr->corner[i] + ox * sx[i] + oy * sy[i] : (double)fr->corner[i];
	if (!lens) {
		if (jitter)
			for (int i = 0; i < 3; i++)
				o.corner[i] = (float)cj[i];
		*out = o;
		return RTX_OK;
	}
	const double focus = (double)pp->focus;
	double lu = 0.0, lv = 0.0; /* the lens point in units of x^ and y^ */
	if (k != 0) {
		const double r = (double)pp->aperture * sqrt(radical_inverse(k, 5)), a = 2.0 * M_PI * radical_inverse(k, 7);
		lu = r * cos(a) / sqrt(lx);
		lv = r * sin(a) / sqrt(ly);
	}
	for (int i = 0; i < 3; i++) {
		const double org = (double)fr->origin[i];
		if (k != 0)
			o.origin[i] = (float)(org + (lu * sx[i] + lv * sy[i]));
		o.corner[i] = (float)(org + focus * (cj[i] - org));
		o.step_x[i] = (float)(focus * sx[i]);
		o.step_y[i] = (float)(focus * sy[i]);
	}
	*out = o;
	return RTX_OK;
}

/* what rtx_render_passes* (and, adaptive, rtx_render_adaptive*) refuse about a frame, its parameters and its pass
 * parameters, none of them null; the device group's entries share it (rtx_group_passes.cpp) */
int rtx_passes_args_check(const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, bool adaptive)
{
	if (!fr->width || !fr->height)
		return fail(RTX_ERR_ARG, "empty frame %ux%u", fr->width, fr->height);
	if (p->tile_offset != 0 || p->tile_stride != 1)
		return fail(RTX_ERR_ARG, "rtx_render_passes renders whole frames: tile sharding %u/%u is not 0/1", p->tile_offset,
			    p->tile_stride);
	rtx_frame f0;
	int rc = rtx_pass_frame(fr, pp, 0, &f0);
	if (rc || !adaptive)
		return rc;
	if (!(pp->target_error > 0.f))
		return fail(RTX_ERR_ARG, "adaptive passes need a target error above 0");
	if (rtx_tiles_total(fr->width, fr->height) > (1ull << 26))
		return fail(RTX_ERR_ARG, "frame %ux%u has more than 2^26 tiles", fr->width, fr->height);
	return RTX_OK;
}

/* everything rtx_render_passes* refuses before it launches anything (the filtered entries too, rtx_filter.cpp) */
int rtx_passes_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, bool adaptive)
{
	if (!c || !fr || !p || !pp)
		return fail(RTX_ERR_ARG, "null argument");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_render_passes before rtx_upload_scene");
	return rtx_passes_args_check(fr, p, pp, adaptive);
}

/* checked arguments, device outputs (each may be null) */
static int passes_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, float *d_rgb, float *d_z,
			 float *d_var, hipStream_t stream)
{
	const uint64_t n = (uint64_t)fr->width * fr->height;
	const uint32_t blocks = rtx_pass_blocks(n);
	if (c->d_pass_rgb.grow(n * 3 * sizeof(float)) != hipSuccess || c->d_pass_state.grow(n * 6 * sizeof(double)) != hipSuccess ||
	    c->d_pass_sums.grow(((size_t)blocks * 2 + 2) * sizeof(double)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "pass state of %llu pixels", (unsigned long long)n);
	double *partials = c->d_pass_sums, *d_sums = partials + (size_t)blocks * 2;
	rtx_pass_stats ps{};
	const bool stop_rule = pp->target_error > 0.f;
	for (uint32_t k = 0; k < pp->passes; k++) {
		rtx_frame fk;
		int rc = rtx_pass_frame(fr, pp, k, &fk);
		if (rc)
			return rc;
		rtx_params pk = *p;
		pk.seed = p->seed + k;
		rc = rtx_render_common(c, &fk, &pk, c->d_pass_rgb, k == 0 ? d_z : nullptr, stream);
		if (rc)
			return rc;
		ps.render_ms += c->stats.kernel_ms;
		ps.closest_rays += c->stats.closest_rays;
		ps.shadow_rays += c->stats.shadow_rays;
		/* the mean, its variance and the error leave the device after the last pass and after every pass the
		 * stopping rule looks at */
		const bool last = k + 1 == pp->passes;
		const bool look = stop_rule && k + 1 >= pp->min_passes;
		const bool out = last || look;
		HIP_TRY(hipEventRecord(c->ev0, stream));
		HIP_TRY(rtx_launch_pass_fold(n, k, out, c->d_pass_rgb, c->d_pass_state, d_rgb, d_var, partials, d_sums, stream));
		HIP_TRY(hipEventRecord(c->ev1, stream));
		double sums[2] = { 0.0, 0.0 };
		if (out && k > 0)
			HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
		ps.accum_ms += ms;
		ps.passes_run = k + 1;
		if (out) {
			ps.error = (k > 0 && sums[1] != 0.0) ? sqrt(sums[0]) / sums[1] : 0.0;
			if (look && ps.error <= (double)pp->target_error)
				break;
		}
	}
	c->pass_stats = ps;
	return RTX_OK;
}

extern "C" int rtx_render_passes_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, void *d_rgb,
					void *d_z, void *d_variance, void *stream)
{
	int rc = rtx_passes_check(c, fr, p, pp, false);
	if (rc)
		return rc;
	if (((uintptr_t)d_rgb | (uintptr_t)d_z | (uintptr_t)d_variance) & 15u)
		return fail(RTX_ERR_ARG, "output buffers must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	return passes_common(c, fr, p, pp, (float *)d_rgb, (float *)d_z, (float *)d_variance, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_render_passes(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, float *rgb, float *z,
				 float *variance)
{
	int rc = rtx_passes_check(c, fr, p, pp, false);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	if (variance && c->d_pass_var.grow(px * 3 * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copy of the variance of %zu pixels", px);
	rc = passes_common(c, fr, p, pp, rgb ? c->d_rgb.p : nullptr, z ? c->d_z.p : nullptr, variance ? c->d_pass_var.p : nullptr,
			   c->stream);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	if (variance)
		HIP_TRY(hipMemcpy(variance, c->d_pass_var, px * 12, hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* everything rtx_render_adaptive* refuses before it launches anything */
static int adaptive_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp)
{
	return rtx_passes_check(c, fr, p, pp, true);
}

/* checked arguments, device outputs (each may be null) */
static int adaptive_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, float *d_rgb, float *d_z,
			   float *d_var, uint32_t *d_tile_passes, hipStream_t stream)
{
	const uint64_t n = (uint64_t)fr->width * fr->height;
	const uint32_t T = (uint32_t)rtx_tiles_total(fr->width, fr->height);
	/* d_ad_tiles: n_t per tile | list A | list B | the next list's count;  d_ad_vs: V_t | S_t | V, A */
	if (c->d_pass_rgb.grow(n * 3 * sizeof(float)) != hipSuccess || c->d_ad_state.grow((size_t)T * 64 * 6 * sizeof(double)) != hipSuccess ||
	    c->d_ad_vs.grow(((size_t)T * 2 + 2) * sizeof(double)) != hipSuccess ||
	    c->d_ad_tiles.grow(((size_t)T * 3 + 1) * sizeof(uint32_t)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "adaptive pass state of %u tiles", T);
	uint32_t *count = c->d_ad_tiles, *list = count + T, *next = list + T, *d_n_next = next + T;
	double *vs = c->d_ad_vs, *d_sums = vs + (size_t)T * 2;
	rtx_adaptive_stats as{};
	as.tiles = T;
	uint32_t active = T;
	HIP_TRY(rtx_launch_tile_all(T, list, stream));
	for (uint32_t k = 0; k < pp->passes && active; k++) {
		rtx_frame fk;
		int rc = rtx_pass_frame(fr, pp, k, &fk);
		if (rc)
			return rc;
		rtx_params pk = *p;
		pk.seed = p->seed + k;
		rc = rtx_render_common(c, &fk, &pk, c->d_pass_rgb, k == 0 ? d_z : nullptr, stream, list, active);
		if (rc)
			return rc;
		as.render_ms += c->stats.kernel_ms;
		as.closest_rays += c->stats.closest_rays;
		as.shadow_rays += c->stats.shadow_rays;
		as.tile_passes += active;
		as.passes_run = k + 1;
		HIP_TRY(hipEventRecord(c->ev0, stream));
		HIP_TRY(rtx_launch_tile_fold(fr->width, fr->height, k, list, active, c->d_pass_rgb, c->d_ad_state, count, vs, stream));
		HIP_TRY(rtx_launch_tile_select(T, k, pp->min_passes, pp->target_error, count, vs, next, d_n_next, d_sums, stream));
		HIP_TRY(hipEventRecord(c->ev1, stream));
		/* the next list's length and the two totals: the pass's one read, on the sync it needs anyway */
		double sums[2] = { 0.0, 0.0 };
		uint32_t n_next = 0;
		HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(&n_next, d_n_next, sizeof(n_next), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
		as.fold_ms += ms;
		as.error = sums[1] != 0.0 ? sqrt(sums[0]) / sums[1] : 0.0;
		active = n_next;
		std::swap(list, next);
	}
	HIP_TRY(hipEventRecord(c->ev0, stream));
	HIP_TRY(rtx_launch_tile_out(fr->width, fr->height, c->d_ad_state, count, d_rgb, d_var, d_tile_passes, stream));
	HIP_TRY(hipEventRecord(c->ev1, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	as.fold_ms += ms;
	c->ad_stats = as;
	return RTX_OK;
}

extern "C" int rtx_render_adaptive_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, void *d_rgb,
					  void *d_z, void *d_variance, void *d_tile_passes, void *stream)
{
	int rc = adaptive_check(c, fr, p, pp);
	if (rc)
		return rc;
	if (((uintptr_t)d_rgb | (uintptr_t)d_z | (uintptr_t)d_variance | (uintptr_t)d_tile_passes) & 15u)
		return fail(RTX_ERR_ARG, "output buffers must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	return adaptive_common(c, fr, p, pp, (float *)d_rgb, (float *)d_z, (float *)d_variance, (uint32_t *)d_tile_passes,
			       stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_render_adaptive(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, float *rgb, float *z,
				   float *variance, uint32_t *tile_passes)
{
	int rc = adaptive_check(c, fr, p, pp);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	const size_t T = (size_t)rtx_tiles_total(fr->width, fr->height);
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	if ((variance && c->d_ad_var.grow(px * 3 * sizeof(float)) != hipSuccess) ||
	    (tile_passes && c->d_ad_passes.grow(T * sizeof(uint32_t)) != hipSuccess))
		return fail(RTX_ERR_NOMEM, "device copies of the variance and the pass counts of %zu pixels", px);
	rc = adaptive_common(c, fr, p, pp, rgb ? c->d_rgb.p : nullptr, z ? c->d_z.p : nullptr, variance ? c->d_ad_var.p : nullptr,
			     tile_passes ? c->d_ad_passes.p : nullptr, c->stream);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	if (variance)
		HIP_TRY(hipMemcpy(variance, c->d_ad_var, px * 12, hipMemcpyDeviceToHost));
	if (tile_passes)
		HIP_TRY(hipMemcpy(tile_passes, c->d_ad_passes, T * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}
