/*
 * Tile packing for the multi-device frame gather (rtx_group_render, rtx_group.cpp): each
 * device packs the tiles of its shard from its rgb/z framebuffer into 16-byte records
 * (rtx_tiles.h), RCCL carries them to device 0, which unpacks them into the full frame.
 * Pure HBM streaming: 28 B read + 16 B written per pixel.
 *
 * And what a group's multi-pass and adaptive renders move (rtx_group_passes.cpp), every value as bits:
 *   k_stat_pack / k_stat_scatter  {V_t, S_t, n_t} of every tile of a shard, 24 B each, out of and into the
 *                                 global per-tile arrays of rtx_adaptive.hip
 *   k_list_shard                  a tile list filtered to the tiles of one shard, order kept: one workgroup,
 *                                 ballot / mbcnt prefix per wave, the waves' counts added in order (as
 *                                 k_tile_select compacts); an index at or past the tile count is dropped
 *   k_pass_pack / k_pass_unpack   32-byte records {mean r, g, b, z, var r, g, b, 0}, 64 per tile
 */
#include <hip/hip_runtime.h>

#include "rtx.h"
#include "rtx_launch.h"
#include "rtx_tiles.h"
#include "rtx_wave.h"

__global__ void k_tile_pack(const float *__restrict__ rgb, const float *__restrict__ z, uint32_t w, uint32_t h,
			    uint32_t off, uint32_t stride, uint32_t nrec, float4 *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nrec)
		return;
	uint32_t x, y;
	rtx_shard_pixel(i, rtx_tiles_x(w), off, stride, &x, &y);
	float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
	if (x < w && y < h) {
		const size_t p = (size_t)y * w + x;
		v = make_float4(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], z[p]);
	}
	out[i] = v;
}

__global__ void k_tile_unpack(const float4 *__restrict__ in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride,
			      uint32_t nrec, float *__restrict__ rgb, float *__restrict__ z)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nrec)
		return;
	uint32_t x, y;
	rtx_shard_pixel(i, rtx_tiles_x(w), off, stride, &x, &y);
	if (x >= w || y >= h)
		return;
	const size_t p = (size_t)y * w + x;
	const float4 v = in[i];
	rgb[3 * p] = v.x;
	rgb[3 * p + 1] = v.y;
	rgb[3 * p + 2] = v.z;
	z[p] = v.w;
}

__global__ void k_stat_pack(const unsigned long long *__restrict__ vs, const uint32_t *__restrict__ count, uint32_t total,
			    uint32_t off, uint32_t stride, uint32_t ntiles, unsigned long long *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= ntiles)
		return;
	const uint32_t t = off + i * stride;
	out[3ull * i] = vs[t];
	out[3ull * i + 1] = vs[(uint64_t)total + t];
	out[3ull * i + 2] = count[t];
}

__global__ void k_stat_scatter(const unsigned long long *__restrict__ in, uint32_t total, uint32_t off, uint32_t stride,
			       uint32_t ntiles, unsigned long long *__restrict__ vs, uint32_t *__restrict__ count)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= ntiles)
		return;
	const uint32_t t = off + i * stride;
	vs[t] = in[3ull * i];
	vs[(uint64_t)total + t] = in[3ull * i + 1];
	count[t] = (uint32_t)in[3ull * i + 2];
}

#define RTX_SHARD_THREADS 256u

__global__ __launch_bounds__(RTX_SHARD_THREADS) void k_list_shard(const uint32_t *__restrict__ in, uint32_t n_in, uint32_t total,
								  uint32_t off, uint32_t stride, uint32_t *__restrict__ out,
								  uint32_t *__restrict__ n_out)
{
	__shared__ uint32_t wave_n[RTX_SHARD_THREADS / 64u];
	uint32_t base = 0; /* the output's length so far: the same in every thread */
	for (uint32_t i0 = 0; i0 < n_in; i0 += RTX_SHARD_THREADS) {
		const uint32_t i = i0 + threadIdx.x;
		uint32_t t = 0;
		bool keep = false;
		if (i < n_in) {
			t = in[i];
			keep = t < total && t % stride == off;
		}
		const u64 m = ballot(keep);
		if ((threadIdx.x & 63u) == 0)
			wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0, sum = 0;
#pragma unroll
		for (uint32_t v = 0; v < RTX_SHARD_THREADS / 64u; v++) {
			if (v < (threadIdx.x >> 6))
				before += wave_n[v];
			sum += wave_n[v];
		}
		if (keep)
			out[base + before + mbcnt(m)] = t;
		base += sum;
		__syncthreads();
	}
	if (threadIdx.x == 0)
		*n_out = base;
}

__global__ void k_pass_pack(const float *__restrict__ rgb, const float *__restrict__ z, const float *__restrict__ var, uint32_t w,
			    uint32_t h, uint32_t off, uint32_t stride, uint32_t nrec, float4 *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nrec)
		return;
	uint32_t x, y;
	rtx_shard_pixel(i, rtx_tiles_x(w), off, stride, &x, &y);
	float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
	if (x < w && y < h) {
		const size_t p = (size_t)y * w + x;
		a = make_float4(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], z[p]);
		b = make_float4(var[3 * p], var[3 * p + 1], var[3 * p + 2], 0.f);
	}
	out[2ull * i] = a;
	out[2ull * i + 1] = b;
}

__global__ void k_pass_unpack(const float4 *__restrict__ in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride, uint32_t nrec,
			      float *__restrict__ rgb, float *__restrict__ z, float *__restrict__ var)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nrec)
		return;
	uint32_t x, y;
	rtx_shard_pixel(i, rtx_tiles_x(w), off, stride, &x, &y);
	if (x >= w || y >= h)
		return;
	const size_t p = (size_t)y * w + x;
	const float4 a = in[2ull * i], b = in[2ull * i + 1];
	if (rgb) {
		rgb[3 * p] = a.x;
		rgb[3 * p + 1] = a.y;
		rgb[3 * p + 2] = a.z;
	}
	if (z)
		z[p] = a.w;
	if (var) {
		var[3 * p] = b.x;
		var[3 * p + 1] = b.y;
		var[3 * p + 2] = b.z;
	}
}

extern "C" hipError_t rtx_launch_tile_pack(const float *rgb, const float *z, uint32_t w, uint32_t h, uint32_t off,
					   uint32_t stride, float4 *out, hipStream_t stream)
{
	const uint32_t nrec = rtx_shard_tiles(w, h, off, stride) * RTX_TILE_PX;
	if (!nrec)
		return hipSuccess;
	hipLaunchKernelGGL(k_tile_pack, dim3((nrec + 255) / 256), dim3(256), 0, stream, rgb, z, w, h, off, stride, nrec, out);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_tile_unpack(const float4 *in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride,
					     float *rgb, float *z, hipStream_t stream)
{
	const uint32_t nrec = rtx_shard_tiles(w, h, off, stride) * RTX_TILE_PX;
	if (!nrec)
		return hipSuccess;
	hipLaunchKernelGGL(k_tile_unpack, dim3((nrec + 255) / 256), dim3(256), 0, stream, in, w, h, off, stride, nrec, rgb, z);
	return hipGetLastError();
}

/* {V_t, S_t, n_t} of the ntiles tiles off, off + stride, .. out of vs (V_t for every tile, then S_t) and count into
 * 3 x 8 bytes per tile, and back into them */
extern "C" RTX_HIDDEN hipError_t rtx_launch_stat_pack(const double *vs, const uint32_t *count, uint32_t total, uint32_t off,
						       uint32_t stride, uint32_t ntiles, void *out, hipStream_t stream)
{
	if (!ntiles)
		return hipSuccess;
	hipLaunchKernelGGL(k_stat_pack, dim3((ntiles + 255) / 256), dim3(256), 0, stream, (const unsigned long long *)vs, count, total,
			   off, stride, ntiles, (unsigned long long *)out);
	return hipGetLastError();
}

extern "C" RTX_HIDDEN hipError_t rtx_launch_stat_scatter(const void *in, uint32_t total, uint32_t off, uint32_t stride,
							  uint32_t ntiles, double *vs, uint32_t *count, hipStream_t stream)
{
	if (!ntiles)
		return hipSuccess;
	hipLaunchKernelGGL(k_stat_scatter, dim3((ntiles + 255) / 256), dim3(256), 0, stream, (const unsigned long long *)in, total, off,
			   stride, ntiles, (unsigned long long *)vs, count);
	return hipGetLastError();
}

/* the entries t < total of in[0..n_in) with t % stride == off into out (room for them), in order; their number into
 * *n_out.  One workgroup whatever n_in is (0 included: it writes the count) */
extern "C" RTX_HIDDEN hipError_t rtx_launch_list_shard(const uint32_t *in, uint32_t n_in, uint32_t total, uint32_t off,
							uint32_t stride, uint32_t *out, uint32_t *n_out, hipStream_t stream)
{
	hipLaunchKernelGGL(k_list_shard, dim3(1), dim3(RTX_SHARD_THREADS), 0, stream, in, n_in, total, off, stride, out, n_out);
	return hipGetLastError();
}

extern "C" RTX_HIDDEN hipError_t rtx_launch_pass_pack(const float *rgb, const float *z, const float *var, uint32_t w, uint32_t h,
						       uint32_t off, uint32_t stride, float4 *out, hipStream_t stream)
{
	const uint32_t nrec = rtx_shard_tiles(w, h, off, stride) * RTX_TILE_PX;
	if (!nrec)
		return hipSuccess;
	hipLaunchKernelGGL(k_pass_pack, dim3((nrec + 255) / 256), dim3(256), 0, stream, rgb, z, var, w, h, off, stride, nrec, out);
	return hipGetLastError();
}

/* rgb, z and var may each be null */
extern "C" RTX_HIDDEN hipError_t rtx_launch_pass_unpack(const float4 *in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride,
							 float *rgb, float *z, float *var, hipStream_t stream)
{
	const uint32_t nrec = rtx_shard_tiles(w, h, off, stride) * RTX_TILE_PX;
	if (!nrec)
		return hipSuccess;
	hipLaunchKernelGGL(k_pass_unpack, dim3((nrec + 255) / 256), dim3(256), 0, stream, in, w, h, off, stride, nrec, rgb, z, var);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded now (rtx_open) rather than at the
 * first launch inside an upload or a render */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_load_gather(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_tile_pack);
}
