/*
 * Tile lists and adaptive passes: the check of a device tile list (rtx_render_tiles_device), and
 * the per-tile state of rtx_render_adaptive*, in which a tile stops receiving passes once its share of the
 * frame's error budget is met.
 *
 *   k_tiles_check  one lane per list entry: an index at or past the tile count, or one not above its
 *                  predecessor, raises the flag word the host reads before it launches anything else.
 *   k_tile_all     the first pass's list, every tile in index order.
 *   k_tile_fold    one wave per ACTIVE tile, lane p for pixel p of the tile: the pass (a packed rgb frame) into
 *                  per-pixel, per-channel double state by k_pass_fold's Welford update with n = n_t + 1, n_t the
 *                  tile's own count, which it then increments.  The state is tile-major and planar (plane c, tile
 *                  t, pixel p at c 64 T + 64 t + p; planes 0..2 the means, 3..5 the m2), so a wave's loads and
 *                  stores of a plane are 512 contiguous bytes; lanes outside the frame hold zeros.  The wave then
 *                  forms V_t = sum m2 / (n_t (n_t - 1)) and S_t = sum |mean| over the channels of the tile's
 *                  in-frame pixels whose three means are finite: channels in order per lane, then the xor
 *                  butterfly 32..1.  Lane 0 stores both, as doubles.  No atomics.
 *   k_tile_select  one workgroup: V = sum V_t and A = sum S_t over ALL tiles in index order (each lane a
 *                  contiguous run of tiles, then lane 0 the lane sums, as k_pass_error), then the tiles that stay
 *                  active compacted in increasing order into the next pass's list (ballot / mbcnt prefix per
 *                  wave, the waves' counts added in order).  Tile t stays active iff k+1 < min_passes, or
 *                  n_t == k+1 (it was active in pass k) and V_t T > target^2 A^2, in double: a NaN compares
 *                  false and the tile stops, and a stopped tile never restarts.  It writes the count, V and A.
 *   k_tile_out     after the last pass, one wave per tile: rgb = (float)mean, variance = (float)(m2 /
 *                  (n_t (n_t - 1))) (0 for n_t = 1) and tile_passes[t] = n_t.
 * Every sum has a fixed order and every grid depends on the list alone, so two runs give the same bits.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"
#include "rtx_tiles.h"
#include "rtx_wave.h"

#define RTX_SELECT_THREADS 256u

__global__ __launch_bounds__(256) void k_tiles_check(const uint32_t *__restrict__ tiles, uint32_t n, uint32_t total,
						     uint32_t *__restrict__ flag)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const uint32_t t = tiles[i];
	if (t >= total || (i && tiles[i - 1] >= t))
		*flag = 1u;
}

__global__ __launch_bounds__(256) void k_tile_all(uint32_t total, uint32_t *__restrict__ list)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < total)
		list[i] = i;
}

/* the pixel of lane p of tile t, and whether it lies in the frame */
__device__ __forceinline__ bool tile_pixel(uint32_t t, uint32_t p, uint32_t w, uint32_t h, uint64_t *pix)
{
	const uint32_t tiles_x = rtx_tiles_x(w);
	const uint32_t px = (t % tiles_x) * 8u + (p & 7u), py = (t / tiles_x) * 8u + (p >> 3);
	*pix = (uint64_t)py * w + px;
	return px < w && py < h;
}

template <bool FIRST>
__global__ __launch_bounds__(64) void k_tile_fold(uint32_t w, uint32_t h, const uint32_t *__restrict__ list,
						   const float *__restrict__ rgb, double *__restrict__ state,
						   uint32_t *__restrict__ count, double *__restrict__ vs)
{
	const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[blockIdx.x]);
	const uint64_t plane = 64ull * (uint64_t)rtx_tiles_total(w, h);
	const uint64_t at = 64ull * t + threadIdx.x;
	const uint32_t n = FIRST ? 1u : count[t] + 1u;
	const double dn = (double)n;
	const double nn1 = dn * (double)(n - 1u); /* n (n-1) */
	uint64_t pix;
	const bool in = tile_pixel(t, threadIdx.x, w, h, &pix);
	double mean[3], var[3];
#pragma unroll
	for (int c = 0; c < 3; c++) {
		double m = 0.0, m2 = 0.0;
		if (in) {
			const double x = (double)rgb[3 * pix + c];
			if (FIRST) {
				m = x;
			} else {
				m = state[(uint64_t)c * plane + at];
				m2 = state[(uint64_t)(3 + c) * plane + at];
				const double d = x - m;
				m += d / dn;
				m2 += d * (x - m);
			}
		}
		state[(uint64_t)c * plane + at] = m;
		state[(uint64_t)(3 + c) * plane + at] = m2;
		mean[c] = m;
		var[c] = n > 1u ? m2 / nn1 : 0.0;
	}
	double sv = 0.0, sa = 0.0;
	if (in && fabs(mean[0]) < (double)INFINITY && fabs(mean[1]) < (double)INFINITY && fabs(mean[2]) < (double)INFINITY) {
		sv += var[0];
		sv += var[1];
		sv += var[2];
		sa += fabs(mean[0]);
		sa += fabs(mean[1]);
		sa += fabs(mean[2]);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		sv += __shfl_xor(sv, o, 64);
		sa += __shfl_xor(sa, o, 64);
	}
	if (threadIdx.x == 0) {
		count[t] = n;
		vs[t] = sv;
		vs[(uint64_t)rtx_tiles_total(w, h) + t] = sa;
	}
}

__global__ __launch_bounds__(RTX_SELECT_THREADS) void k_tile_select(uint32_t total, uint32_t k, uint32_t min_passes, float target,
								    const uint32_t *__restrict__ count,
								    const double *__restrict__ vs, uint32_t *__restrict__ next,
								    uint32_t *__restrict__ n_next, double *__restrict__ sums)
{
	__shared__ double lane_sum[RTX_SELECT_THREADS][2];
	__shared__ double tot[2];
	__shared__ uint32_t wave_n[RTX_SELECT_THREADS / 64u];
	const uint32_t per = (total + RTX_SELECT_THREADS - 1u) / RTX_SELECT_THREADS;
	const uint32_t b0 = threadIdx.x * per < total ? threadIdx.x * per : total, b1 = b0 + per < total ? b0 + per : total;
	double sv = 0.0, sa = 0.0;
	for (uint32_t t = b0; t < b1; t++) {
		sv += vs[t];
		sa += vs[total + t];
	}
	lane_sum[threadIdx.x][0] = sv;
	lane_sum[threadIdx.x][1] = sa;
	__syncthreads();
	if (threadIdx.x == 0) {
		sv = 0.0;
		sa = 0.0;
		for (uint32_t l = 0; l < RTX_SELECT_THREADS; l++) {
			sv += lane_sum[l][0];
			sa += lane_sum[l][1];
		}
		tot[0] = sv;
		tot[1] = sa;
		sums[0] = sv;
		sums[1] = sa;
	}
	__syncthreads();
	const double A = tot[1];
	const double bound = ((double)target * (double)target) * (A * A);
	const bool all = k + 1u < min_passes;
	uint32_t base = 0; /* the next list's length so far: the same in every thread */
	for (uint32_t t0 = 0; t0 < total; t0 += RTX_SELECT_THREADS) {
		const uint32_t t = t0 + threadIdx.x;
		bool keep = false;
		if (t < total)
			keep = all || (count[t] == k + 1u && vs[t] * (double)total > bound);
		const u64 m = ballot(keep);
		if ((threadIdx.x & 63u) == 0)
			wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0, sum = 0;
#pragma unroll
		for (uint32_t v = 0; v < RTX_SELECT_THREADS / 64u; v++) {
			if (v < (threadIdx.x >> 6))
				before += wave_n[v];
			sum += wave_n[v];
		}
		if (keep)
			next[base + before + mbcnt(m)] = t;
		base += sum;
		__syncthreads();
	}
	if (threadIdx.x == 0)
		*n_next = base;
}

__global__ __launch_bounds__(64) void k_tile_out(uint32_t w, uint32_t h, const double *__restrict__ state,
						  const uint32_t *__restrict__ count, float *__restrict__ rgb,
						  float *__restrict__ var, uint32_t *__restrict__ tile_passes)
{
	const uint32_t t = blockIdx.x;
	const uint64_t plane = 64ull * (uint64_t)rtx_tiles_total(w, h);
	const uint64_t at = 64ull * t + threadIdx.x;
	const uint32_t n = count[t];
	const double nn1 = (double)n * (double)(n - 1u);
	if (tile_passes && threadIdx.x == 0)
		tile_passes[t] = n;
	uint64_t pix;
	if (!tile_pixel(t, threadIdx.x, w, h, &pix))
		return;
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (rgb)
			rgb[3 * pix + c] = (float)state[(uint64_t)c * plane + at];
		if (var)
			var[3 * pix + c] = n > 1u ? (float)(state[(uint64_t)(3 + c) * plane + at] / nn1) : 0.f;
	}
}

extern "C" RTX_HIDDEN hipError_t rtx_launch_tiles_check(const uint32_t *tiles, uint32_t n, uint32_t total, uint32_t *flag,
							 hipStream_t stream)
{
	if (!n)
		return hipSuccess;
	hipLaunchKernelGGL(k_tiles_check, dim3((n + 255u) / 256u), dim3(256), 0, stream, tiles, n, total, flag);
	return hipGetLastError();
}

extern "C" RTX_HIDDEN hipError_t rtx_launch_tile_all(uint32_t total, uint32_t *list, hipStream_t stream)
{
	hipLaunchKernelGGL(k_tile_all, dim3((total + 255u) / 256u), dim3(256), 0, stream, total, list);
	return hipGetLastError();
}

/* pass k (rgb: the w x h frame, packed) into the state of the n_list tiles of list (6 * 64 T doubles); count: n_t
 * per tile; vs: V_t for every tile, then S_t for every tile.  Pass 0 lists every tile and writes the state without
 * reading it, so nothing has to be cleared. */
extern "C" RTX_HIDDEN hipError_t rtx_launch_tile_fold(uint32_t w, uint32_t h, uint32_t k, const uint32_t *list, uint32_t n_list,
						       const float *rgb, double *state, uint32_t *count, double *vs,
						       hipStream_t stream)
{
	if (!n_list)
		return hipSuccess;
	if (k == 0)
		hipLaunchKernelGGL(k_tile_fold<true>, dim3(n_list), dim3(64), 0, stream, w, h, list, rgb, state, count, vs);
	else
		hipLaunchKernelGGL(k_tile_fold<false>, dim3(n_list), dim3(64), 0, stream, w, h, list, rgb, state, count, vs);
	return hipGetLastError();
}

/* after pass k: the tiles of pass k+1 into next (room for `total`), their number into *n_next, {V, A} into sums */
extern "C" RTX_HIDDEN hipError_t rtx_launch_tile_select(uint32_t total, uint32_t k, uint32_t min_passes, float target,
							 const uint32_t *count, const double *vs, uint32_t *next, uint32_t *n_next,
							 double *sums, hipStream_t stream)
{
	hipLaunchKernelGGL(k_tile_select, dim3(1), dim3(RTX_SELECT_THREADS), 0, stream, total, k, min_passes, target, count, vs,
			   next, n_next, sums);
	return hipGetLastError();
}

/* rgb / var (w x h, packed) and tile_passes (T words), each may be null */
extern "C" RTX_HIDDEN hipError_t rtx_launch_tile_out(uint32_t w, uint32_t h, const double *state, const uint32_t *count,
						      float *rgb, float *var, uint32_t *tile_passes, hipStream_t stream)
{
	if (!rgb && !var && !tile_passes)
		return hipSuccess;
	hipLaunchKernelGGL(k_tile_out, dim3((uint32_t)rtx_tiles_total(w, h)), dim3(64), 0, stream, w, h, state, count, rgb, var,
			   tile_passes);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_passes */
extern "C" RTX_HIDDEN hipError_t rtx_load_adaptive(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_tile_select);
}
