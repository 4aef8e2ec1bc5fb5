/*
 * C-ABI of include/rtx.h, pixel reconstruction filters for multi-pass rendering: the filter's two
 * weight tables of pass k (host only), and rtx_render_passes's loop with each pass gathered through them and
 * folded on the device into a weighted mean and the variance of that mean (rtx_filter.hip).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_launch.h"

extern "C" void rtx_filter_params_default(rtx_filter_params *p)
{
	if (!p)
		return;
	memset(p, 0, sizeof(*p));
	p->kind = RTX_FILTER_GAUSSIAN;
	p->radius = 1.5f;
	p->alpha = 2.f;
}

static int filter_params_check(const rtx_filter_params *fp)
{
	static const char *const names[] = { "box", "tent", "Gaussian", "Mitchell" };
	if (fp->kind > RTX_FILTER_MITCHELL)
		return fail(RTX_ERR_ARG, "unknown filter kind %u", fp->kind);
	const float lo = fp->kind == RTX_FILTER_BOX ? 0.5f : 1.f;
	if (!(fp->radius >= lo && fp->radius <= 2.5f))
		return fail(RTX_ERR_ARG, "%s filter radius %g outside %g..2.5", names[fp->kind], (double)fp->radius, (double)lo);
	if (fp->kind == RTX_FILTER_GAUSSIAN && !(fp->alpha > 0.f && fp->alpha < INFINITY))
		return fail(RTX_ERR_ARG, "Gaussian filter alpha %g is not a finite value above 0", (double)fp->alpha);
	if (fp->pad_)
		return fail(RTX_ERR_ARG, "rtx_filter_params.pad_ is not 0");
	return RTX_OK;
}

/* the Mitchell-Netravali cubic with B = C = 1/3 at x >= 0, by Horner's rule as the header writes it */
static double mitchell(double x)
{
	if (x < 1.0)
		return ((7.0 * x - 12.0) * x * x + 16.0 / 3.0) / 6.0;
	return (((-7.0 / 3.0 * x + 12.0) * x - 20.0) * x + 32.0 / 3.0) / 6.0;
}

/* f(d) of checked parameters */
static double filter_eval(const rtx_filter_params *fp, double d)
{
	const double r = (double)fp->radius, a = (double)fp->alpha;
	switch (fp->kind) {
	case RTX_FILTER_BOX:
		return (-r <= d && d < r) ? 1.0 : 0.0;
	case RTX_FILTER_TENT: {
		const double t = 1.0 - fabs(d) / r;
		return t > 0.0 ? t : 0.0;
	}
	case RTX_FILTER_GAUSSIAN:
		return fabs(d) < r ? exp(-a * (d * d)) - exp(-a * (r * r)) : 0.0;
	default:
		return fabs(d) < r ? mitchell(fabs(2.0 * d / r)) : 0.0;
	}
}

/* checked parameters, k < passes */
static void filter_weights(const rtx_pass_params *pp, const rtx_filter_params *fp, uint32_t k, double *wx, double *wy)
{
	double ox, oy;
	rtx_pass_offset(pp, k, &ox, &oy);
	for (int i = 0; i < RTX_FILTER_TAPS; i++) {
		wx[i] = filter_eval(fp, (double)(i - 2) + ox);
		wy[i] = filter_eval(fp, (double)(i - 2) + oy);
	}
}

extern "C" int rtx_pass_filter_weights(const rtx_pass_params *pp, const rtx_filter_params *fp, uint32_t k, double wx[RTX_FILTER_TAPS],
				       double wy[RTX_FILTER_TAPS])
{
	if (!pp || !fp || !wx || !wy)
		return fail(RTX_ERR_ARG, "null argument");
	int rc = rtx_pass_params_check(pp);
	if (rc)
		return rc;
	if (k >= pp->passes)
		return fail(RTX_ERR_ARG, "pass %u of %u", k, pp->passes);
	rc = filter_params_check(fp);
	if (rc)
		return rc;
	filter_weights(pp, fp, k, wx, wy);
	return RTX_OK;
}

/* everything rtx_render_passes_filtered* refuses before it launches anything */
static int filtered_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, const rtx_filter_params *fp)
{
	if (!fp)
		return fail(RTX_ERR_ARG, "null argument");
	int rc = rtx_passes_check(c, fr, p, pp, false);
	if (rc)
		return rc;
	rc = filter_params_check(fp);
	if (rc)
		return rc;
	if (rtx_filter_blocks(fr->width, fr->height) > (1u << 24))
		return fail(RTX_ERR_ARG, "frame %ux%u has more than 2^24 tiles of 32x8 pixels", fr->width, fr->height);
	return RTX_OK;
}

/* checked arguments, device outputs (each may be null): rtx_render_passes's loop with the filtered fold */
static int filtered_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, const rtx_filter_params *fp,
			   float *d_rgb, float *d_z, float *d_var, hipStream_t stream)
{
	const uint64_t n = (uint64_t)fr->width * fr->height;
	const size_t blocks = (size_t)rtx_filter_blocks(fr->width, fr->height);
	if (c->d_pass_rgb.grow(n * 3 * sizeof(float)) != hipSuccess || c->d_pass_state.grow(n * 7 * sizeof(double)) != hipSuccess ||
	    c->d_pass_sums.grow((blocks * 2 + 2) * sizeof(double)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "pass state of %llu pixels", (unsigned long long)n);
	double *partials = c->d_pass_sums, *d_sums = partials + blocks * 2;
	rtx_pass_stats ps{};
	const bool stop_rule = pp->target_error > 0.f;
	for (uint32_t k = 0; k < pp->passes; k++) {
		rtx_frame fk;
		int rc = rtx_pass_frame(fr, pp, k, &fk);
		if (rc)
			return rc;
		rtx_filter_weights fw;
		filter_weights(pp, fp, k, fw.wx, fw.wy);
		rtx_params pk = *p;
		pk.seed = p->seed + k;
		rc = rtx_render_common(c, &fk, &pk, c->d_pass_rgb, k == 0 ? d_z : nullptr, stream);
		if (rc)
			return rc;
		ps.render_ms += c->stats.kernel_ms;
		ps.closest_rays += c->stats.closest_rays;
		ps.shadow_rays += c->stats.shadow_rays;
		const bool last = k + 1 == pp->passes;
		const bool look = stop_rule && k + 1 >= pp->min_passes;
		const bool out = last || look;
		HIP_TRY(hipEventRecord(c->ev0, stream));
		HIP_TRY(rtx_launch_pass_filter_fold(fr->width, fr->height, k, out, &fw, c->d_pass_rgb, c->d_pass_state, d_rgb, d_var, partials,
						    d_sums, stream));
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

extern "C" int rtx_render_passes_filtered_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp,
						 const rtx_filter_params *fp, void *d_rgb, void *d_z, void *d_variance, void *stream)
{
	int rc = filtered_check(c, fr, p, pp, fp);
	if (rc)
		return rc;
	if (((uintptr_t)d_rgb | (uintptr_t)d_z | (uintptr_t)d_variance) & 15u)
		return fail(RTX_ERR_ARG, "output buffers must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	return filtered_common(c, fr, p, pp, fp, (float *)d_rgb, (float *)d_z, (float *)d_variance,
			       stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_render_passes_filtered(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp,
					  const rtx_filter_params *fp, float *rgb, float *z, float *variance)
{
	int rc = filtered_check(c, fr, p, pp, fp);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	if (variance && c->d_pass_var.grow(px * 3 * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "device copy of the variance of %zu pixels", px);
	rc = filtered_common(c, fr, p, pp, fp, rgb ? c->d_rgb.p : nullptr, z ? c->d_z.p : nullptr, variance ? c->d_pass_var.p : nullptr,
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
