/*
 * Pixel reconstruction filters for multi-pass rendering (include/rtx.h): the passes of
 * rtx_render_passes_filtered* gathered through a 5x5 stencil and folded into a per-pixel weighted mean and the
 * variance of that mean.
 *
 *   k_pass_filter_fold  one output pixel per lane, 256-thread blocks over tiles of 32x8 pixels (a wave is two
 *                 rows of 32).  The tile's pass colours and a 2-pixel halo, 36x12 pixels, are staged once in
 *                 LDS as three planes of floats (5 KB); a slot outside the frame holds 0 and is never read as a
 *                 tap: whether tap (i, j) of pixel p lies in the frame depends on p alone, so each lane carries
 *                 the two 5-bit masks of its in-frame columns and rows.  That keeps a frame narrower or lower
 *                 than the halo (1x1, 300x2) on the one path.  The ten weights are kernel arguments, uniform
 *                 over the wave, so a zero-weight tap is skipped by a scalar branch.  The taps accumulate in
 *                 double in row-major order from -0.0, addition's identity, so that a single tap of weight 1
 *                 returns its sample's bits, the sign of a zero included.
 *                 The state is planar doubles as k_pass_fold's, mean r, g, b and M2 r, g, b, then the weight
 *                 sum (56 B per pixel); pass 0 writes it without reading it.  With Wk the pass's weight sum
 *                 and f = S / Wk:  Wsum += Wk, d = f - mean, mean += (d Wk) / Wsum, M2 += (Wk d) (f - mean).
 *                 OUT writes rgb = (float)mean, variance = (float)(M2 / (Wsum k)) (0 for k = 0) and the block's
 *                 partial sums of the variance and of |mean| over the channels of its pixels whose mean is
 *                 finite, in k_pass_fold's order: a fixed butterfly over the wave, the four waves added in
 *                 order.  No atomics.  k_pass_error (rtx_passes.hip) totals the blocks' sums.
 * The grid is the frame's tile grid, so two runs give the same bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"

#define FT_W 32
#define FT_H 8
#define FT_HALO 2
#define FT_LW (FT_W + 2 * FT_HALO)
#define FT_LH (FT_H + 2 * FT_HALO)

static_assert(RTX_FILTER_TAPS == 2 * FT_HALO + 1, "the halo is the stencil's reach");

template <bool FIRST, bool OUT>
__global__ __launch_bounds__(256) void k_pass_filter_fold(uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t k, rtx_filter_weights fw,
							  const float *__restrict__ rgb, double *__restrict__ state,
							  float *__restrict__ out_rgb, float *__restrict__ out_var,
							  double *__restrict__ partials)
{
	__shared__ float tile[3][FT_LH][FT_LW];
	__shared__ double wave_sum[4][2];
	const uint64_t n = (uint64_t)w * h;
	const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
	const int64_t x0 = (int64_t)bx * FT_W - FT_HALO, y0 = (int64_t)by * FT_H - FT_HALO;
	for (uint32_t s = threadIdx.x; s < FT_LW * FT_LH; s += 256u) {
		const uint32_t ly = s / FT_LW, lx = s % FT_LW;
		const int64_t gx = x0 + lx, gy = y0 + ly;
		float r = 0.f, g = 0.f, b = 0.f;
		if (gx >= 0 && gx < (int64_t)w && gy >= 0 && gy < (int64_t)h) {
			const uint64_t q = (uint64_t)gy * w + (uint64_t)gx;
			r = rgb[3 * q];
			g = rgb[3 * q + 1];
			b = rgb[3 * q + 2];
		}
		tile[0][ly][lx] = r;
		tile[1][ly][lx] = g;
		tile[2][ly][lx] = b;
	}
	__syncthreads();
	const uint32_t tx = threadIdx.x % FT_W, ty = threadIdx.x / FT_W;
	const uint64_t px = (uint64_t)bx * FT_W + tx, py = (uint64_t)by * FT_H + ty;
	double sv = 0.0, sa = 0.0;
	if (px < w && py < h) {
		/* bit i: column px + i - 2 (row py + i - 2) lies in the frame */
		uint32_t xm = 0, ym = 0;
#pragma unroll
		for (int i = 0; i < RTX_FILTER_TAPS; i++) {
			const int64_t qx = (int64_t)px + i - FT_HALO, qy = (int64_t)py + i - FT_HALO;
			xm |= (qx >= 0 && qx < (int64_t)w) ? 1u << i : 0u;
			ym |= (qy >= 0 && qy < (int64_t)h) ? 1u << i : 0u;
		}
		double S[3] = { -0.0, -0.0, -0.0 }, Wk = -0.0;
#pragma unroll
		for (int j = 0; j < RTX_FILTER_TAPS; j++) {
#pragma unroll
			for (int i = 0; i < RTX_FILTER_TAPS; i++) {
				const double wt = fw.wx[i] * fw.wy[j];
				if (wt != 0.0 && ((xm >> i) & (ym >> j) & 1u)) {
					S[0] += wt * (double)tile[0][ty + j][tx + i];
					S[1] += wt * (double)tile[1][ty + j][tx + i];
					S[2] += wt * (double)tile[2][ty + j][tx + i];
					Wk += wt;
				}
			}
		}
		const uint64_t p = py * w + px;
		double wsum = Wk;
		if (!FIRST)
			wsum += state[6 * n + p];
		state[6 * n + p] = wsum;
		const double den = wsum * (double)k; /* Wsum (n - 1) */
		double mean[3], var[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double f = S[c] / Wk;
			double m, m2;
			if (FIRST) {
				m = f;
				m2 = 0.0;
			} else {
				m = state[(uint64_t)c * n + p];
				m2 = state[(uint64_t)(3 + c) * n + p];
				const double d = f - m;
				m += (d * Wk) / wsum;
				m2 += (Wk * d) * (f - m);
			}
			state[(uint64_t)c * n + p] = m;
			state[(uint64_t)(3 + c) * n + p] = m2;
			mean[c] = m;
			var[c] = k ? m2 / den : 0.0;
		}
		if (OUT) {
			if (out_rgb) {
				out_rgb[3 * p] = (float)mean[0];
				out_rgb[3 * p + 1] = (float)mean[1];
				out_rgb[3 * p + 2] = (float)mean[2];
			}
			if (out_var) {
				out_var[3 * p] = (float)var[0];
				out_var[3 * p + 1] = (float)var[1];
				out_var[3 * p + 2] = (float)var[2];
			}
			if (fabs(mean[0]) < (double)INFINITY && fabs(mean[1]) < (double)INFINITY && fabs(mean[2]) < (double)INFINITY) {
				sv += var[0];
				sv += var[1];
				sv += var[2];
				sa += fabs(mean[0]);
				sa += fabs(mean[1]);
				sa += fabs(mean[2]);
			}
		}
	}
	if (OUT) {
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			sv += __shfl_xor(sv, o, 64);
			sa += __shfl_xor(sa, o, 64);
		}
		if ((threadIdx.x & 63u) == 0) {
			wave_sum[threadIdx.x >> 6][0] = sv;
			wave_sum[threadIdx.x >> 6][1] = sa;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			partials[2 * (uint64_t)blockIdx.x] = ((wave_sum[0][0] + wave_sum[1][0]) + wave_sum[2][0]) + wave_sum[3][0];
			partials[2 * (uint64_t)blockIdx.x + 1] = ((wave_sum[0][1] + wave_sum[1][1]) + wave_sum[2][1]) + wave_sum[3][1];
		}
	}
}

/* the tile grid of a w x h frame: the fold's blocks, and the pairs of partial sums an OUT pass writes */
extern "C" RTX_HIDDEN uint64_t rtx_filter_blocks(uint32_t w, uint32_t h)
{
	return (((uint64_t)w + FT_W - 1) / FT_W) * (((uint64_t)h + FT_H - 1) / FT_H);
}

/* pass k (rgb: w x h pixels, packed) through the weights fw into state (7 w h doubles).  out != 0: the mean and its
 * variance into out_rgb / out_var (each may be null), the blocks' partial sums into partials (2 * rtx_filter_blocks
 * doubles) and their totals into sums[2].  The caller keeps rtx_filter_blocks(w, h) within 2^24. */
extern "C" RTX_HIDDEN hipError_t rtx_launch_pass_filter_fold(uint32_t w, uint32_t h, uint32_t k, int out, const rtx_filter_weights *fw,
							     const float *rgb, double *state, float *out_rgb, float *out_var,
							     double *partials, double *sums, hipStream_t stream)
{
	const uint64_t blocks = rtx_filter_blocks(w, h);
	if (!blocks || blocks > (1u << 24))
		return hipErrorInvalidValue;
	const uint32_t tiles_x = (uint32_t)(((uint64_t)w + FT_W - 1) / FT_W);
	const dim3 grid((uint32_t)blocks), block(256);
	if (out) {
		if (k == 0)
			hipLaunchKernelGGL((k_pass_filter_fold<true, true>), grid, block, 0, stream, w, h, tiles_x, k, *fw, rgb, state, out_rgb,
					   out_var, partials);
		else
			hipLaunchKernelGGL((k_pass_filter_fold<false, true>), grid, block, 0, stream, w, h, tiles_x, k, *fw, rgb, state,
					   out_rgb, out_var, partials);
		return rtx_launch_pass_error((uint32_t)blocks, partials, sums, stream);
	}
	if (k == 0)
		hipLaunchKernelGGL((k_pass_filter_fold<true, false>), grid, block, 0, stream, w, h, tiles_x, k, *fw, rgb, state,
				   (float *)nullptr, (float *)nullptr, (double *)nullptr);
	else
		hipLaunchKernelGGL((k_pass_filter_fold<false, false>), grid, block, 0, stream, w, h, tiles_x, k, *fw, rgb, state,
				   (float *)nullptr, (float *)nullptr, (double *)nullptr);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_passes */
extern "C" RTX_HIDDEN hipError_t rtx_load_filter(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_pass_filter_fold<false, false>);
}
