/*
 * C-ABI of include/rtx.h, temporal accumulation: the projection of a world point into a frame (host
 * only), the accumulation of a frame into its reprojected history on caller's buffers (rtx_temporal.hip), and the
 * pipeline that renders a frame of a camera path, takes its feature records and accumulates it into the history the
 * context keeps.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"

extern "C" void rtx_temporal_params_default(rtx_temporal_params *p)
{
	if (!p)
		return;
	memset(p, 0, sizeof(*p));
	p->max_history = 32;
	p->match_material = 1;
	/* the feature sigmas are rtx_denoise's */
	p->sigma_normal = 0.05f;
	p->sigma_albedo = 0.1f;
	p->sigma_plane = 0.02f;
}

/* M = [step_x | step_y | corner - origin]^-1 and the origin of a frame that is not empty, in double.  The
 * determinant is (step_x x step_y) . (corner - origin): the cross product of two parallel float vectors whose ratio
 * is a power of two is exactly 0, as the products of floats are exact in double */
static int frame_proj(const rtx_frame *fr, rtx_temporal_proj *out)
{
	double a[3], b[3], c[3];
	for (int i = 0; i < 3; i++) {
		a[i] = (double)fr->step_x[i];
		b[i] = (double)fr->step_y[i];
		c[i] = (double)fr->corner[i] - (double)fr->origin[i];
	}
	const auto cross = [](const double *p, const double *q, double *r) {
		r[0] = p[1] * q[2] - p[2] * q[1];
		r[1] = p[2] * q[0] - p[0] * q[2];
		r[2] = p[0] * q[1] - p[1] * q[0];
	};
	double ab[3], bc[3], ca[3];
	cross(a, b, ab);
	cross(b, c, bc);
	cross(c, a, ca);
	const double det = ab[0] * c[0] + ab[1] * c[1] + ab[2] * c[2];
	if (det == 0.0 || !std::isfinite(det))
		return fail(RTX_ERR_ARG, "the frame's step_x, step_y and corner - origin span no volume (determinant %g)", det);
	rtx_temporal_proj pr;
	for (int i = 0; i < 3; i++) {
		pr.m[i] = bc[i] / det;
		pr.m[3 + i] = ca[i] / det;
		pr.m[6 + i] = ab[i] / det;
		pr.o[i] = (double)fr->origin[i];
	}
	for (double m : pr.m)
		if (!std::isfinite(m))
			return fail(RTX_ERR_ARG, "the frame's inverse is not finite (determinant %g)", det);
	*out = pr;
	return RTX_OK;
}

extern "C" int rtx_frame_project(const rtx_frame *fr, const float P[3], double *u, double *v, int *in_front)
{
	if (!fr || !P || !u || !v || !in_front)
		return fail(RTX_ERR_ARG, "null argument");
	if (!fr->width || !fr->height)
		return fail(RTX_ERR_ARG, "empty frame %ux%u", fr->width, fr->height);
	rtx_temporal_proj pr;
	const int rc = frame_proj(fr, &pr);
	if (rc)
		return rc;
	const double d[3] = { (double)P[0] - pr.o[0], (double)P[1] - pr.o[1], (double)P[2] - pr.o[2] };
	const double q0 = pr.m[0] * d[0] + pr.m[1] * d[1] + pr.m[2] * d[2];
	const double q1 = pr.m[3] * d[0] + pr.m[4] * d[1] + pr.m[5] * d[2];
	const double q2 = pr.m[6] * d[0] + pr.m[7] * d[1] + pr.m[8] * d[2];
	*in_front = q2 > 0.0;
	*u = q0 / q2 - 1.0;
	*v = q1 / q2;
	return RTX_OK;
}

static int tp_params_check(const rtx_temporal_params *tp)
{
	if (tp->max_history < 1 || tp->max_history > RTX_TEMPORAL_HISTORY_MAX)
		return fail(RTX_ERR_ARG, "max_history %u outside 1..%u", tp->max_history, RTX_TEMPORAL_HISTORY_MAX);
	for (float s : { tp->sigma_normal, tp->sigma_albedo, tp->sigma_plane })
		if (!(s > 0.f))
			return fail(RTX_ERR_ARG, "temporal sigma %g is not above 0", (double)s);
	return RTX_OK;
}

/* the buffers of one call, host or device */
struct TemporalArgs {
	const void *rgb, *var, *feat;
	const void *hist_rgb, *hist_var, *hist_len, *hist_feat;
	void *out_rgb, *out_var, *out_len, *out_conf;
};

static bool overlap(const void *p, size_t np, const void *q, size_t nq)
{
	const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
	return p && q && a < b + nq && b < a + np;
}

/* everything rtx_temporal* refuses before it launches anything; *same: the frames are bytewise equal; *pr: the previous
 * frame's projection (a history only) */
static int temporal_check(rtx_ctx *c, const rtx_temporal_params *tp, const rtx_frame *cur, const rtx_frame *prev, const TemporalArgs &a,
			  int *same, rtx_temporal_proj *pr)
{
	if (!c || !tp || !cur || !a.rgb || !a.feat || !a.out_rgb || !a.out_len)
		return fail(RTX_ERR_ARG, "null argument");
	const uint32_t w = cur->width, h = cur->height;
	if (!w || !h || (uint64_t)w * h > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad temporal size %ux%u", w, h);
	int rc = tp_params_check(tp);
	if (rc)
		return rc;
	const bool hist = prev || a.hist_rgb || a.hist_len || a.hist_feat;
	if (hist && !(prev && a.hist_rgb && a.hist_len && a.hist_feat))
		return fail(RTX_ERR_ARG, "the previous frame, its colour, length and records are all given or all null");
	if (!a.var != !a.out_var || (hist ? !a.var != !a.hist_var : a.hist_var != nullptr))
		return fail(RTX_ERR_ARG, "the variance buffers are all given or all null");
	*same = 0;
	memset(pr, 0, sizeof(*pr));
	if (!hist)
		return RTX_OK;
	if (prev->width != w || prev->height != h)
		return fail(RTX_ERR_ARG, "the previous frame is %ux%u, the current one %ux%u", prev->width, prev->height, w, h);
	rc = frame_proj(prev, pr);
	if (rc)
		return rc;
	*same = memcmp(cur, prev, sizeof(rtx_frame)) == 0;
	const size_t n = (size_t)w * h;
	const struct {
		const void *p;
		size_t bytes;
	} outs[4] = { { a.out_rgb, n * 12 }, { a.out_var, n * 12 }, { a.out_len, n * 4 }, { a.out_conf, n * 4 } },
	  hists[4] = { { a.hist_rgb, n * 12 }, { a.hist_var, n * 12 }, { a.hist_len, n * 4 }, { a.hist_feat, n * sizeof(rtx_feature) } };
	for (const auto &o : outs)
		for (const auto &q : hists)
			if (overlap(o.p, o.bytes, q.p, q.bytes))
				return fail(RTX_ERR_ARG, "an output overlaps the history");
	return RTX_OK;
}

/* checked arguments on device buffers: the counters zeroed, the kernel between ev0 and ev1, the counters read back;
 * synchronises the stream and fills c->tp_stats' kernel time and pixel counts (the rest 0) */
static int temporal_common(rtx_ctx *c, uint32_t w, uint32_t h, const rtx_temporal_params *tp, int same, const rtx_temporal_proj *pr,
			   const TemporalArgs &a, hipStream_t stream)
{
	if (((uintptr_t)a.feat | (uintptr_t)a.hist_feat) & 15u)
		return fail(RTX_ERR_ARG, "feature buffers must be 16-byte aligned");
	if (((uintptr_t)a.rgb | (uintptr_t)a.var | (uintptr_t)a.hist_rgb | (uintptr_t)a.hist_var | (uintptr_t)a.hist_len | (uintptr_t)a.out_rgb |
	     (uintptr_t)a.out_var | (uintptr_t)a.out_len | (uintptr_t)a.out_conf) & 3u)
		return fail(RTX_ERR_ARG, "colour, variance, length and confidence buffers must be 4-byte aligned");
	const size_t ctr_bytes = RTX_TEMPORAL_CTR_WORDS * sizeof(unsigned long long);
	if (c->d_tp_ctr.grow(ctr_bytes) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "temporal counters");
	c->tp_ctr.resize(RTX_TEMPORAL_CTR_WORDS);
	HIP_TRY(hipMemsetAsync(c->d_tp_ctr, 0, ctr_bytes, stream));
	HIP_TRY(hipEventRecord(c->ev0, stream));
	HIP_TRY(rtx_launch_temporal(w, h, tp, same, pr, (const float *)a.rgb, (const float *)a.var, (const float4 *)a.feat,
				    (const float *)a.hist_rgb, (const float *)a.hist_var, (const float *)a.hist_len,
				    (const float4 *)a.hist_feat, (float *)a.out_rgb, (float *)a.out_var, (float *)a.out_len,
				    (float *)a.out_conf, c->d_tp_ctr, stream));
	HIP_TRY(hipEventRecord(c->ev1, stream));
	HIP_TRY(hipMemcpyAsync(c->tp_ctr.data(), c->d_tp_ctr, ctr_bytes, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
	uint64_t live = 0, with_history = 0;
	for (uint32_t s = 0; s < RTX_TEMPORAL_CTR_SLOTS; s++) {
		const unsigned long long v = c->tp_ctr[(size_t)s * RTX_TEMPORAL_CTR_STRIDE];
		live += v & 0xFFFFFFFFull;
		with_history += v >> 32;
	}
	rtx_temporal_stats ts{};
	ts.temporal_ms = ms;
	ts.pixels = (uint64_t)w * h;
	ts.live_pixels = live;
	ts.history_pixels = with_history;
	ts.reset_pixels = live - with_history;
	c->tp_stats = ts;
	return RTX_OK;
}

extern "C" int rtx_temporal_device(rtx_ctx *c, const rtx_temporal_params *tp, const rtx_frame *cur, const void *d_rgb,
				   const void *d_variance, const void *d_features, const rtx_frame *prev, const void *d_hist_rgb,
				   const void *d_hist_variance, const void *d_hist_length, const void *d_hist_features, void *d_out_rgb,
				   void *d_out_variance, void *d_out_length, void *d_out_conf, void *stream)
{
	const TemporalArgs a = { d_rgb,         d_variance,     d_features,   d_hist_rgb, d_hist_variance, d_hist_length, d_hist_features,
				 d_out_rgb,     d_out_variance, d_out_length, d_out_conf };
	int same;
	rtx_temporal_proj pr;
	const int rc = temporal_check(c, tp, cur, prev, a, &same, &pr);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	return temporal_common(c, cur->width, cur->height, tp, same, &pr, a, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_temporal(rtx_ctx *c, const rtx_temporal_params *tp, const rtx_frame *cur, const float *rgb, const float *variance,
			    const rtx_feature *features, const rtx_frame *prev, const float *hist_rgb, const float *hist_variance,
			    const float *hist_length, const rtx_feature *hist_features, float *out_rgb, float *out_variance,
			    float *out_length, float *out_conf)
{
	const TemporalArgs a = { rgb,     variance,     features,   hist_rgb, hist_variance, hist_length, hist_features,
				 out_rgb, out_variance, out_length, out_conf };
	int same;
	rtx_temporal_proj pr;
	int rc = temporal_check(c, tp, cur, prev, a, &same, &pr);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t n = (size_t)cur->width * cur->height;
	rtx_ctx::TemporalSet &now = c->tp_host[0], &old = c->tp_host[1];
	bool ok = now.rgb.grow(n * 12) == hipSuccess && now.feat.grow(n * sizeof(rtx_feature)) == hipSuccess && now.len.grow(n * 4) == hipSuccess &&
		  (!variance || now.var.grow(n * 12) == hipSuccess) && (!out_conf || c->d_tp_conf.grow(n * 4) == hipSuccess);
	if (ok && prev)
		ok = old.rgb.grow(n * 12) == hipSuccess && old.feat.grow(n * sizeof(rtx_feature)) == hipSuccess && old.len.grow(n * 4) == hipSuccess &&
		     (!variance || old.var.grow(n * 12) == hipSuccess);
	if (!ok)
		return fail(RTX_ERR_NOMEM, "device copies of %zu pixels", n);
	HIP_TRY(hipMemcpyAsync(now.rgb, rgb, n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(hipMemcpyAsync(now.feat, features, n * sizeof(rtx_feature), hipMemcpyHostToDevice, c->stream));
	if (variance)
		HIP_TRY(hipMemcpyAsync(now.var, variance, n * 12, hipMemcpyHostToDevice, c->stream));
	if (prev) {
		HIP_TRY(hipMemcpyAsync(old.rgb, hist_rgb, n * 12, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(old.len, hist_length, n * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(hipMemcpyAsync(old.feat, hist_features, n * sizeof(rtx_feature), hipMemcpyHostToDevice, c->stream));
		if (variance)
			HIP_TRY(hipMemcpyAsync(old.var, hist_variance, n * 12, hipMemcpyHostToDevice, c->stream));
	}
	/* the outputs over the current inputs */
	const TemporalArgs d = { now.rgb.p,
				 variance ? now.var.p : nullptr,
				 now.feat.p,
				 prev ? old.rgb.p : nullptr,
				 prev && variance ? old.var.p : nullptr,
				 prev ? old.len.p : nullptr,
				 prev ? old.feat.p : nullptr,
				 now.rgb.p,
				 variance ? now.var.p : nullptr,
				 now.len.p,
				 out_conf ? c->d_tp_conf.p : nullptr };
	rc = temporal_common(c, cur->width, cur->height, tp, same, &pr, d, c->stream);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpy(out_rgb, now.rgb, n * 12, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(out_length, now.len, n * 4, hipMemcpyDeviceToHost));
	if (out_variance)
		HIP_TRY(hipMemcpy(out_variance, now.var, n * 12, hipMemcpyDeviceToHost));
	if (out_conf)
		HIP_TRY(hipMemcpy(out_conf, c->d_tp_conf, n * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* everything rtx_render_temporal* refuses before it launches anything */
static int render_temporal_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, const rtx_temporal_params *tp)
{
	if (!c || !fr || !p || !pp || !tp)
		return fail(RTX_ERR_ARG, "null argument");
	int rc = rtx_passes_check(c, fr, p, pp, false);
	if (rc)
		return rc;
	if ((uint64_t)fr->width * fr->height > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad temporal size %ux%u", fr->width, fr->height);
	if (p->u32conv != RTX_U32_SAT && p->u32conv != RTX_U32_WRAP)
		return fail(RTX_ERR_ARG, "bad u32conv %d", p->u32conv);
	return tp_params_check(tp);
}

/* checked arguments, device outputs (each may be null) */
static int render_temporal_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp,
				  const rtx_temporal_params *tp, float *d_rgb, float *d_z, float *d_var, float *d_len, hipStream_t stream)
{
	const uint32_t w = fr->width, h = fr->height;
	const size_t n = (size_t)w * h;
	const bool hist = c->tp_valid && c->tp_frame.width == w && c->tp_frame.height == h;
	rtx_ctx::TemporalSet &now = c->tp_set[c->tp_hist ^ 1u], &old = c->tp_set[c->tp_hist];
	/* a growth loses the contents: the set that is not the history grows, and a history of another size is no history */
	if (now.rgb.grow(n * 12) != hipSuccess || now.var.grow(n * 12) != hipSuccess || now.len.grow(n * 4) != hipSuccess ||
	    now.feat.grow(n * sizeof(rtx_feature)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "temporal buffers of %zu pixels", n);
	int same = 0;
	rtx_temporal_proj pr;
	memset(&pr, 0, sizeof(pr));
	if (hist) {
		const int rc = frame_proj(&c->tp_frame, &pr);
		if (rc)
			return rc;
		same = memcmp(fr, &c->tp_frame, sizeof(rtx_frame)) == 0;
	}
	rtx_temporal_stats ts{};
	int rc = rtx_render_passes_device(c, fr, p, pp, now.rgb.p, d_z, now.var.p, stream);
	if (rc)
		return rc;
	ts.render_ms = c->pass_stats.render_ms + c->pass_stats.accum_ms;
	ts.closest_rays = c->pass_stats.closest_rays;
	ts.shadow_rays = c->pass_stats.shadow_rays;
	rc = rtx_features_common(c, fr, p->u32conv, now.feat.p, stream);
	if (rc)
		return rc;
	ts.features_ms = c->dn_stats.features_ms;
	const TemporalArgs a = { now.rgb.p,
				 now.var.p,
				 now.feat.p,
				 hist ? old.rgb.p : nullptr,
				 hist ? old.var.p : nullptr,
				 hist ? old.len.p : nullptr,
				 hist ? old.feat.p : nullptr,
				 now.rgb.p,
				 now.var.p,
				 now.len.p,
				 nullptr };
	rc = temporal_common(c, w, h, tp, same, &pr, a, stream);
	if (rc)
		return rc;
	if (d_rgb)
		HIP_TRY(hipMemcpyAsync(d_rgb, now.rgb, n * 12, hipMemcpyDeviceToDevice, stream));
	if (d_var)
		HIP_TRY(hipMemcpyAsync(d_var, now.var, n * 12, hipMemcpyDeviceToDevice, stream));
	if (d_len)
		HIP_TRY(hipMemcpyAsync(d_len, now.len, n * 4, hipMemcpyDeviceToDevice, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	/* the results become the history */
	c->tp_frames = hist ? c->tp_frames + 1 : 1;
	c->tp_hist ^= 1u;
	c->tp_valid = true;
	c->tp_frame = *fr;
	ts.frames = c->tp_frames;
	ts.temporal_ms = c->tp_stats.temporal_ms;
	ts.pixels = c->tp_stats.pixels;
	ts.live_pixels = c->tp_stats.live_pixels;
	ts.history_pixels = c->tp_stats.history_pixels;
	ts.reset_pixels = c->tp_stats.reset_pixels;
	c->tp_stats = ts;
	return RTX_OK;
}

extern "C" int rtx_render_temporal_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp,
					  const rtx_temporal_params *tp, void *d_rgb, void *d_z, void *d_variance, void *d_length,
					  void *stream)
{
	int rc = render_temporal_check(c, fr, p, pp, tp);
	if (rc)
		return rc;
	if (((uintptr_t)d_rgb | (uintptr_t)d_z | (uintptr_t)d_variance | (uintptr_t)d_length) & 15u)
		return fail(RTX_ERR_ARG, "output buffers must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	return render_temporal_common(c, fr, p, pp, tp, (float *)d_rgb, (float *)d_z, (float *)d_variance, (float *)d_length,
				      stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_render_temporal(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp,
				   const rtx_temporal_params *tp, float *rgb, float *z, float *variance, float *length)
{
	int rc = render_temporal_check(c, fr, p, pp, tp);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	if (z && c->d_z.grow(px * sizeof(float)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "z buffer of %zu pixels", px);
	rc = render_temporal_common(c, fr, p, pp, tp, nullptr, z ? c->d_z.p : nullptr, nullptr, nullptr, c->stream);
	if (rc)
		return rc;
	/* the history now holds the results */
	const rtx_ctx::TemporalSet &res = c->tp_set[c->tp_hist];
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, res.rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	if (variance)
		HIP_TRY(hipMemcpy(variance, res.var, px * 12, hipMemcpyDeviceToHost));
	if (length)
		HIP_TRY(hipMemcpy(length, res.len, px * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}

extern "C" int rtx_temporal_reset(rtx_ctx *c)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null argument");
	c->tp_valid = false;
	c->tp_frames = 0;
	return RTX_OK;
}
