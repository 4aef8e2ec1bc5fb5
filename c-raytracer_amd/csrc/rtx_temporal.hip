/*
 * Temporal accumulation (include/rtx.h): a frame's colour and variance blended with the history of the
 * frames before it, which every pixel fetches at its world position's projection into the previous frame.
 *
 *   k_temporal     one pixel per lane, 256-thread blocks over tiles of 32x8 pixels (k_upsample's shape and reasons).  A
 *                  pixel reads its own record (three float4), colour and variance, and of each of its up to four
 *                  history taps the length, the colour, the variance and the record; neighbours share the taps,
 *                  which L1 / L2 serve: no LDS staging.  The projection (nine multiply-adds and two divisions) and
 *                  the floors are in double, so that the device and the float64 model agree on which taps a pixel
 *                  has; everything after fx and fy is in float with a fast exp.  Every tap index is checked against
 *                  the frame before any load.  The outputs may alias the current inputs: a pixel reads its own
 *                  colour and variance before it writes them and nobody else's, so those pointers are not
 *                  restrict.  No floating-point atomics: two runs give the same bits.  The statistics (live and
 *                  with-history pixels; the reset ones are their difference) are two ballots' popcounts per wave,
 *                  packed into one integer atomic add per wave, to one of RTX_TEMPORAL_CTR_SLOTS slots that the host
 *                  sums.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"
#include "rtx_wave.h"

#define TP_W 32
#define TP_H 8

static_assert(sizeof(rtx_feature) == 48, "k_temporal reads a feature record as three float4");

__device__ __forceinline__ bool tp_finite3(float x, float y, float z)
{
	return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

/* finite and not negative */
__device__ __forceinline__ bool tp_var3(float x, float y, float z)
{
	return x >= 0.f && y >= 0.f && z >= 0.f && tp_finite3(x, y, z);
}

template <bool VAR>
__global__ __launch_bounds__(256) void k_temporal(uint32_t w, uint32_t h, uint32_t tiles_x, float n_max, int match, float inv_n,
						  float inv_a, float sigma_p, int same_frame, rtx_temporal_proj pr, const float *rgb,
						  const float *var, const float4 *__restrict__ feat, const float *__restrict__ hist_rgb,
						  const float *__restrict__ hist_var, const float *__restrict__ hist_len,
						  const float4 *__restrict__ hist_feat, float *out_rgb, float *out_var,
						  float *__restrict__ out_len, float *__restrict__ out_conf,
						  unsigned long long *__restrict__ ctr)
{
#pragma clang fp contract(fast)
	const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
	const uint32_t x = bx * TP_W + threadIdx.x % TP_W, y = by * TP_H + threadIdx.x / TP_W;
	const bool inside = x < w && y < h;
	bool live = false, with_history = false;
	if (inside) {
		const size_t p = (size_t)y * w + x;
		const float4 f0 = feat[3 * p], f1 = feat[3 * p + 1], f2 = feat[3 * p + 2];
		const float cr = rgb[3 * p], cg = rgb[3 * p + 1], cb = rgb[3 * p + 2];
		float vr = 0.f, vg = 0.f, vb = 0.f;
		if (VAR) {
			vr = var[3 * p];
			vg = var[3 * p + 1];
			vb = var[3 * p + 2];
		}
		live = f0.w != 0.f && tp_finite3(cr, cg, cb) && (!VAR || tp_var3(vr, vg, vb));
		float o_r = cr, o_g = cg, o_b = cb, o_vr = vr, o_vg = vg, o_vb = vb;
		float len = 0.f, cf = f0.w == 0.f ? 1.f : 0.f;
		if (live) {
			len = 1.f;
			cf = 0.f;
			double u = (double)x, v = (double)y;
			bool reach = hist_rgb != nullptr;
			if (reach && !same_frame) {
				const double dx = (double)f0.x - pr.o[0], dy = (double)f0.y - pr.o[1], dz = (double)f0.z - pr.o[2];
				const double q0 = pr.m[0] * dx + pr.m[1] * dy + pr.m[2] * dz;
				const double q1 = pr.m[3] * dx + pr.m[4] * dy + pr.m[5] * dz;
				const double q2 = pr.m[6] * dx + pr.m[7] * dy + pr.m[8] * dz;
				u = q0 / q2 - 1.0;
				v = q1 / q2;
				/* a NaN fails every compare */
				reach = q2 > 0.0 && u > -1.0 && u < (double)w && v > -1.0 && v < (double)h;
			}
			if (reach) {
				const double xf = floor(u), yf = floor(v);
				const int64_t x0 = (int64_t)xf, y0 = (int64_t)yf;
				const float fx = (float)(u - xf), fy = (float)(v - yf);
				const int mat = (int)__float_as_uint(f1.w);
				const float sz = sigma_p * f0.w;
				const float inv_p = 1.f / (sz * sz);
				float S = 0.f, hr = 0.f, hg = 0.f, hb = 0.f, Hr = 0.f, Hg = 0.f, Hb = 0.f, n = 0.f;
#pragma unroll
				for (int b = 0; b < 2; b++) {
#pragma unroll
					for (int a = 0; a < 2; a++) {
						const int64_t qx = x0 + a, qy = y0 + b;
						const float bw = (a ? fx : 1.f - fx) * (b ? fy : 1.f - fy);
						if (qx < 0 || qy < 0 || qx >= (int64_t)w || qy >= (int64_t)h || !(bw > 0.f))
							continue;
						const size_t q = (size_t)qy * w + (size_t)qx;
						const float L = hist_len[q];
						if (!(L >= 1.f && L < INFINITY))
							continue;
						const float tr = hist_rgb[3 * q], tg = hist_rgb[3 * q + 1], tb = hist_rgb[3 * q + 2];
						if (!tp_finite3(tr, tg, tb))
							continue;
						float ur = 0.f, ug = 0.f, ub = 0.f;
						if (VAR) {
							ur = hist_var[3 * q];
							ug = hist_var[3 * q + 1];
							ub = hist_var[3 * q + 2];
							if (!tp_var3(ur, ug, ub))
								continue;
						}
						const float4 q0 = hist_feat[3 * q], q1 = hist_feat[3 * q + 1], q2 = hist_feat[3 * q + 2];
						if (q0.w == 0.f || (match && (int)__float_as_uint(q1.w) != mat))
							continue;
						const float nx = f1.x - q1.x, ny = f1.y - q1.y, nz = f1.z - q1.z;
						const float ax = f2.x - q2.x, ay = f2.y - q2.y, az = f2.z - q2.z;
						const float pd = f1.x * (q0.x - f0.x) + f1.y * (q0.y - f0.y) + f1.z * (q0.z - f0.z);
						const float e = (nx * nx + ny * ny + nz * nz) * inv_n + (ax * ax + ay * ay + az * az) * inv_a + pd * pd * inv_p;
						if (!(e <= RTX_TEMPORAL_E_MAX)) /* beyond the cut, or NaN (0 * inf) */
							continue;
						const float wt = bw * __expf(-e);
						S += wt;
						hr += wt * tr;
						hg += wt * tg;
						hb += wt * tb;
						if (VAR) {
							Hr += wt * wt * ur;
							Hg += wt * wt * ug;
							Hb += wt * wt * ub;
						}
						n += wt * L;
					}
				}
				if (S > 0.f) {
					with_history = true;
					hr /= S;
					hg /= S;
					hb /= S;
					const float np = fminf(n, n_max);
					const float alpha = 1.f / (np + 1.f), keep = 1.f - alpha;
					o_r = hr + alpha * (cr - hr);
					o_g = hg + alpha * (cg - hg);
					o_b = hb + alpha * (cb - hb);
					if (VAR) {
						const float s2 = S * S, k2 = keep * keep, a2 = alpha * alpha;
						o_vr = k2 * (Hr / s2) + a2 * vr;
						o_vg = k2 * (Hg / s2) + a2 * vg;
						o_vb = k2 * (Hb / s2) + a2 * vb;
					}
					len = np + 1.f;
					cf = S;
				}
			}
		}
		out_rgb[3 * p] = o_r;
		out_rgb[3 * p + 1] = o_g;
		out_rgb[3 * p + 2] = o_b;
		if (VAR) {
			out_var[3 * p] = o_vr;
			out_var[3 * p + 1] = o_vg;
			out_var[3 * p + 2] = o_vb;
		}
		out_len[p] = len;
		if (out_conf)
			out_conf[p] = cf;
	}
	/* every lane of the wave is here: the wave's live pixels in the low word and its with-history pixels in the high
	 * word of one add (a slot's sums stay below 2^32, so no carry crosses); the waves take the slots in turn, each slot
	 * on a cache line of its own (every wave adding to one line took 0.8 of the kernel's 0.9 ms at 1920x1080) */
	const u64 m_live = ballot(live), m_hist = ballot(with_history);
	if ((threadIdx.x & 63u) == 0 && m_live) {
		const uint32_t slot = (blockIdx.x * 4u + (threadIdx.x >> 6)) % RTX_TEMPORAL_CTR_SLOTS;
		atomicAdd(&ctr[(size_t)slot * RTX_TEMPORAL_CTR_STRIDE], (unsigned long long)popc64(m_live) | ((unsigned long long)popc64(m_hist) << 32));
	}
}

/* checked parameters and pointers (rtx_temporal.cpp); var, hist_var and out_var all given or none (hist_var follows the
 * history); hist_* all null: no history; ctr: RTX_TEMPORAL_CTR_WORDS zeroed words */
extern "C" RTX_HIDDEN hipError_t rtx_launch_temporal(uint32_t w, uint32_t h, const rtx_temporal_params *tp, int same_frame,
						     const rtx_temporal_proj *pr, const float *rgb, const float *var, const float4 *feat,
						     const float *hist_rgb, const float *hist_var, const float *hist_len,
						     const float4 *hist_feat, float *out_rgb, float *out_var, float *out_len,
						     float *out_conf, unsigned long long *ctr, hipStream_t stream)
{
	const uint32_t tiles_x = (w + TP_W - 1) / TP_W;
	const uint64_t blocks = (uint64_t)tiles_x * ((h + TP_H - 1) / TP_H);
	if (!blocks || blocks > 0x7FFFFFFFull)
		return hipErrorInvalidValue;
	const auto inv_sqr = [](double v) { return (float)(1.0 / (v * v)); }; /* INFINITY -> 0: the term is off */
	const float inv_n = inv_sqr(tp->sigma_normal), inv_a = inv_sqr(tp->sigma_albedo);
	const float n_max = (float)(tp->max_history - 1u);
	const dim3 grid((uint32_t)blocks), block(256);
	if (var)
		hipLaunchKernelGGL(k_temporal<true>, grid, block, 0, stream, w, h, tiles_x, n_max, tp->match_material != 0, inv_n, inv_a,
				   tp->sigma_plane, same_frame, *pr, rgb, var, feat, hist_rgb, hist_var, hist_len, hist_feat, out_rgb, out_var,
				   out_len, out_conf, ctr);
	else
		hipLaunchKernelGGL(k_temporal<false>, grid, block, 0, stream, w, h, tiles_x, n_max, tp->match_material != 0, inv_n, inv_a,
				   tp->sigma_plane, same_frame, *pr, rgb, var, feat, hist_rgb, hist_var, hist_len, hist_feat, out_rgb, out_var,
				   out_len, out_conf, ctr);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_upsample */
extern "C" RTX_HIDDEN hipError_t rtx_load_temporal(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_temporal<true>);
}
