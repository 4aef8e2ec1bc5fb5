/*
 * Multi-pass rendering kernels: the passes of rtx_render_passes* folded into a per-pixel mean
 * and the variance of that mean.
 *
 *   k_pass_fold   pass k's packed rgb frame into the running state by Welford's update, per channel and in
 *                 double: d = x - mean, mean += d / (k+1), m2 += d (x - mean).  The state is planar, six
 *                 arrays of one double per pixel (mean r, g, b, then m2 r, g, b; 48 B per pixel), so a
 *                 wave's loads and stores of it are contiguous; the pass is read as three floats per lane,
 *                 whose cache lines the three loads use up between them.  One pixel per lane, 256-thread
 *                 blocks, a bounded grid that strides over the frame (as k_dn_pack).  Pass 0 writes the
 *                 state without reading it, so nothing has to be cleared.
 *                 OUT (the last pass, and every pass the stopping rule looks at) also writes
 *                 rgb = (float)mean and variance = (float)(m2 / (n (n-1))), n = k+1 (0 for n = 1), and the
 *                 block's partial sums of var_mean and |mean| over the channels of its pixels whose mean is
 *                 finite: lane sums in pixel order, a fixed butterfly over the wave, the four waves added in
 *                 order.  No atomics.
 *   k_pass_error  the blocks' partial sums added in index order by one wave (each lane a contiguous run of
 *                 blocks, then lane 0 the 64 lane sums): {sum var_mean, sum |mean|}, which the host reads.
 * The grid depends on the pixel count alone, so two runs give the same bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"

#define RTX_PASS_BLOCKS 2048u

template <bool FIRST, bool OUT>
__global__ __launch_bounds__(256) void k_pass_fold(uint64_t n, uint32_t k, const float *__restrict__ rgb, double *__restrict__ state,
						   float *__restrict__ out_rgb, float *__restrict__ out_var,
						   double *__restrict__ partials)
{
	__shared__ double wave_sum[4][2];
	const double kp1 = (double)k + 1.0;
	const double nn1 = kp1 * (double)k; /* n (n-1) */
	double sv = 0.0, sa = 0.0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		double mean[3], var[3];
#pragma unroll
		for (int c = 0; c < 3; c++) {
			const double x = (double)rgb[3 * i + c];
			double m, m2;
			if (FIRST) {
				m = x;
				m2 = 0.0;
			} else {
				m = state[(uint64_t)c * n + i];
				m2 = state[(uint64_t)(3 + c) * n + i];
				const double d = x - m;
				m += d / kp1;
				m2 += d * (x - m);
			}
			state[(uint64_t)c * n + i] = m;
			state[(uint64_t)(3 + c) * n + i] = m2;
			mean[c] = m;
			var[c] = k ? m2 / nn1 : 0.0;
		}
		if (OUT) {
			if (out_rgb) {
				out_rgb[3 * i] = (float)mean[0];
				out_rgb[3 * i + 1] = (float)mean[1];
				out_rgb[3 * i + 2] = (float)mean[2];
			}
			if (out_var) {
				out_var[3 * i] = (float)var[0];
				out_var[3 * i + 1] = (float)var[1];
				out_var[3 * i + 2] = (float)var[2];
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
			partials[2 * blockIdx.x] = ((wave_sum[0][0] + wave_sum[1][0]) + wave_sum[2][0]) + wave_sum[3][0];
			partials[2 * blockIdx.x + 1] = ((wave_sum[0][1] + wave_sum[1][1]) + wave_sum[2][1]) + wave_sum[3][1];
		}
	}
}

__global__ __launch_bounds__(64) void k_pass_error(uint32_t blocks, const double *__restrict__ partials, double *__restrict__ out)
{
	__shared__ double lane_sum[64][2];
	const uint32_t per = (blocks + 63u) / 64u;
	const uint32_t b0 = threadIdx.x * per, b1 = b0 + per < blocks ? b0 + per : blocks;
	double sv = 0.0, sa = 0.0;
	for (uint32_t b = b0; b < b1; b++) {
		sv += partials[2 * b];
		sa += partials[2 * b + 1];
	}
	lane_sum[threadIdx.x][0] = sv;
	lane_sum[threadIdx.x][1] = sa;
	__syncthreads();
	if (threadIdx.x == 0) {
		sv = 0.0;
		sa = 0.0;
		for (int l = 0; l < 64; l++) {
			sv += lane_sum[l][0];
			sa += lane_sum[l][1];
		}
		out[0] = sv;
		out[1] = sa;
	}
}

extern "C" RTX_HIDDEN uint32_t rtx_pass_blocks(uint64_t n)
{
	const uint64_t blocks = (n + 255) / 256;
	return (uint32_t)(blocks < RTX_PASS_BLOCKS ? blocks : RTX_PASS_BLOCKS);
}

/* the partial sums of `blocks` blocks (2 doubles each) totalled into sums[2]; the filtered fold's too (rtx_filter.hip) */
extern "C" RTX_HIDDEN hipError_t rtx_launch_pass_error(uint32_t blocks, const double *partials, double *sums, hipStream_t stream)
{
	hipLaunchKernelGGL(k_pass_error, dim3(1), dim3(64), 0, stream, blocks, partials, sums);
	return hipGetLastError();
}

/* pass k (rgb: n pixels, packed) into state (6 n doubles).  out != 0: the mean and its variance into out_rgb /
 * out_var (each may be null), the blocks' partial sums into partials (2 * rtx_pass_blocks(n) doubles) and their
 * totals into sums[2] */
extern "C" RTX_HIDDEN hipError_t rtx_launch_pass_fold(uint64_t n, uint32_t k, int out, const float *rgb, double *state, float *out_rgb,
						      float *out_var, double *partials, double *sums, hipStream_t stream)
{
	const uint32_t blocks = rtx_pass_blocks(n);
	const dim3 grid(blocks), block(256);
	if (out) {
		if (k == 0)
			hipLaunchKernelGGL((k_pass_fold<true, true>), grid, block, 0, stream, n, k, rgb, state, out_rgb, out_var, partials);
		else
			hipLaunchKernelGGL((k_pass_fold<false, true>), grid, block, 0, stream, n, k, rgb, state, out_rgb, out_var, partials);
		return rtx_launch_pass_error(blocks, partials, sums, stream);
	} else if (k == 0) {
		hipLaunchKernelGGL((k_pass_fold<true, false>), grid, block, 0, stream, n, k, rgb, state, (float *)nullptr, (float *)nullptr,
				   (double *)nullptr);
	} else {
		hipLaunchKernelGGL((k_pass_fold<false, false>), grid, block, 0, stream, n, k, rgb, state, (float *)nullptr, (float *)nullptr,
				   (double *)nullptr);
	}
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_denoise */
extern "C" RTX_HIDDEN hipError_t rtx_load_passes(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_pass_fold<false, false>);
}
