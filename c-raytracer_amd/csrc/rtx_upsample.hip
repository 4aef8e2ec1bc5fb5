/*
 * Feature-guided upsampling (include/rtx.h): a low-resolution frame reconstructed at full resolution
 * under the guidance of the full-resolution feature records, and the list of the tiles to refine.
 *
 *   k_upsample     one full pixel per lane, 256-thread blocks over tiles of 32x8 pixels (a wave is two rows of 32,
 *                  as k_pass_filter_fold).  A pixel reads its own record (three float4), and of each of its up to
 *                  four low taps the record and the packed colour; neighbours share the taps, which L1 / L2 serve:
 *                  no LDS staging.  The tap positions and the bilinear weights come from integers (n = 2 X - (s - 1),
 *                  x0 = floor(n / 2 s), fx = (n - 2 s x0) / 2 s), so whether a tap's weight is 0 is exact.  The sums
 *                  start from -0.0, addition's identity, so that a single tap of weight 1 returns its colour's
 *                  bits, the sign of a zero included.  No atomics: two runs give the same bits.
 *   k_up_z         z of the full frame's records into a packed z buffer (rtx_render_upsampled*).
 *   k_up_count     one wave per 8x8 tile, lane p for pixel p: the tile's number of pixels with conf < threshold, by
 *                  a ballot.
 *   k_up_select    one workgroup: the tiles whose count is not 0 compacted in increasing order (ballot / mbcnt
 *                  prefix per wave, the waves' counts added in order, as k_tile_select), and the counts summed
 *                  (integers).  It writes the list's length and the pixel total.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"
#include "rtx_tiles.h"
#include "rtx_wave.h"

#define UP_W 32
#define UP_H 8
#define UP_SELECT_THREADS 256u

static_assert(sizeof(rtx_feature) == 48, "k_upsample reads a feature record as three float4");

__device__ __forceinline__ bool up_finite3(float x, float y, float z)
{
	return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

/* floor(n / d) and the remainder in [0, d) of a possibly negative n, d > 0 */
__device__ __forceinline__ int64_t up_floor_div(int64_t n, int d, int *rem)
{
	int64_t q = n / d, r = n - q * d;
	if (r < 0) {
		r += d;
		q -= 1;
	}
	*rem = (int)r;
	return q;
}

template <bool DEMOD>
__global__ __launch_bounds__(256) void k_upsample(uint32_t w, uint32_t h, uint32_t lw, uint32_t lh, uint32_t tiles_x, uint32_t s,
						  int match, float inv_n, float inv_a, float sigma_p, float albedo_min,
						  const float *__restrict__ low_rgb, const float4 *__restrict__ low_feat,
						  const float4 *__restrict__ feat, float *__restrict__ rgb, float *__restrict__ conf)
{
#pragma clang fp contract(fast)
	const uint32_t bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
	const uint32_t x = bx * UP_W + threadIdx.x % UP_W, y = by * UP_H + threadIdx.x / UP_W;
	if (x >= w || y >= h)
		return;
	const size_t p = (size_t)y * w + x;
	const float4 f0 = feat[3 * p], f1 = feat[3 * p + 1], f2 = feat[3 * p + 2];
	const bool hit = f0.w != 0.f;
	const int mat = (int)__float_as_uint(f1.w);
	const float sz = sigma_p * f0.w;
	const float inv_p = 1.f / (sz * sz);
	const int d = 2 * (int)s;
	int rx, ry;
	const int64_t x0 = up_floor_div(2 * (int64_t)x - ((int64_t)s - 1), d, &rx), y0 = up_floor_div(2 * (int64_t)y - ((int64_t)s - 1), d, &ry);
	const float fx = (float)rx / (float)d, fy = (float)ry / (float)d;
	float sr = -0.f, sg = -0.f, sb = -0.f, sw = -0.f; /* the guided sums and sum b g */
	float br = -0.f, bg = -0.f, bb = -0.f, bw = -0.f; /* the bilinear fallback over the finite taps */
	float ball = 0.f;                                  /* sum b over every considered tap */
#pragma unroll
	for (int j = 0; j < 2; j++) {
#pragma unroll
		for (int i = 0; i < 2; i++) {
			const int64_t qx = x0 + i, qy = y0 + j;
			const float b = (i ? fx : 1.f - fx) * (j ? fy : 1.f - fy);
			if (qx < 0 || qy < 0 || qx >= (int64_t)lw || qy >= (int64_t)lh || !(b > 0.f))
				continue;
			const size_t q = (size_t)qy * lw + (size_t)qx;
			const float cr = low_rgb[3 * q], cg = low_rgb[3 * q + 1], cb = low_rgb[3 * q + 2];
			ball += b;
			if (!up_finite3(cr, cg, cb))
				continue;
			br += b * cr;
			bg += b * cg;
			bb += b * cb;
			bw += b;
			const float4 q0 = low_feat[3 * q], q1 = low_feat[3 * q + 1], q2 = low_feat[3 * q + 2];
			const bool qhit = q0.w != 0.f;
			if (qhit != hit)
				continue;
			float g = 1.f, mr = 1.f, mg = 1.f, mb = 1.f;
			if (hit) {
				if (match && (int)__float_as_uint(q1.w) != mat)
					continue;
				const float nx = f1.x - q1.x, ny = f1.y - q1.y, nz = f1.z - q1.z;
				const float ax = f2.x - q2.x, ay = f2.y - q2.y, az = f2.z - q2.z;
				const float pd = f1.x * (q0.x - f0.x) + f1.y * (q0.y - f0.y) + f1.z * (q0.z - f0.z);
				const float e = (nx * nx + ny * ny + nz * nz) * inv_n + (ax * ax + ay * ay + az * az) * inv_a + pd * pd * inv_p;
				if (!(e <= RTX_UPSAMPLE_E_MAX)) /* beyond the cut, or NaN (0 * inf) */
					continue;
				g = __expf(-e);
				if (DEMOD) {
					mr = (f2.x >= albedo_min && q2.x >= albedo_min) ? f2.x / q2.x : 1.f;
					mg = (f2.y >= albedo_min && q2.y >= albedo_min) ? f2.y / q2.y : 1.f;
					mb = (f2.z >= albedo_min && q2.z >= albedo_min) ? f2.z / q2.z : 1.f;
				}
			}
			const float wt = b * g;
			sr += wt * (mr * cr);
			sg += wt * (mg * cg);
			sb += wt * (mb * cb);
			sw += wt;
		}
	}
	float r = 0.f, gg = 0.f, bl = 0.f, cf = 0.f;
	if (sw > 0.f) {
		r = sr / sw;
		gg = sg / sw;
		bl = sb / sw;
		cf = sw / ball;
	} else if (bw > 0.f) {
		r = br / bw;
		gg = bg / bw;
		bl = bb / bw;
	}
	rgb[3 * p] = r;
	rgb[3 * p + 1] = gg;
	rgb[3 * p + 2] = bl;
	if (conf)
		conf[p] = cf;
}

__global__ __launch_bounds__(256) void k_up_z(uint64_t n, const float4 *__restrict__ feat, float *__restrict__ z)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i < n)
		z[i] = feat[3 * i].w;
}

__global__ __launch_bounds__(64) void k_up_count(uint32_t w, uint32_t h, float threshold, const float *__restrict__ conf,
						 uint32_t *__restrict__ count)
{
	const uint32_t t = blockIdx.x, tiles_x = rtx_tiles_x(w);
	const uint32_t px = (t % tiles_x) * 8u + (threadIdx.x & 7u), py = (t / tiles_x) * 8u + (threadIdx.x >> 3);
	bool low = false;
	if (px < w && py < h)
		low = conf[(uint64_t)py * w + px] < threshold;
	const u64 m = ballot(low);
	if (threadIdx.x == 0)
		count[t] = (uint32_t)__popcll(m);
}

__global__ __launch_bounds__(UP_SELECT_THREADS) void k_up_select(uint32_t total, const uint32_t *__restrict__ count,
								 uint32_t *__restrict__ list, unsigned long long *__restrict__ out)
{
	__shared__ uint32_t wave_n[UP_SELECT_THREADS / 64u];
	__shared__ unsigned long long lane_px[UP_SELECT_THREADS];
	uint32_t base = 0; /* the list's length so far: the same in every thread */
	unsigned long long px = 0;
	for (uint32_t t0 = 0; t0 < total; t0 += UP_SELECT_THREADS) {
		const uint32_t t = t0 + threadIdx.x;
		const uint32_t c = t < total ? count[t] : 0u;
		const bool keep = c != 0u;
		px += c;
		const u64 m = ballot(keep);
		if ((threadIdx.x & 63u) == 0)
			wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = 0, sum = 0;
#pragma unroll
		for (uint32_t v = 0; v < UP_SELECT_THREADS / 64u; v++) {
			if (v < (threadIdx.x >> 6))
				before += wave_n[v];
			sum += wave_n[v];
		}
		if (keep)
			list[base + before + mbcnt(m)] = t;
		base += sum;
		__syncthreads();
	}
	lane_px[threadIdx.x] = px;
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long all = 0;
		for (uint32_t l = 0; l < UP_SELECT_THREADS; l++)
			all += lane_px[l];
		out[0] = base;
		out[1] = all;
	}
}

/* the w x h frame (rgb packed, conf may be null) from the ceil(w / s) x ceil(h / s) low frame; checked parameters */
extern "C" RTX_HIDDEN hipError_t rtx_launch_upsample(uint32_t w, uint32_t h, const rtx_upsample_params *up, const float *low_rgb,
						     const float4 *low_feat, const float4 *feat, float *rgb, float *conf,
						     hipStream_t stream)
{
	const uint32_t s = up->scale;
	const uint32_t lw = (w + s - 1) / s, lh = (h + s - 1) / s;
	const uint32_t tiles_x = (w + UP_W - 1) / UP_W;
	const uint64_t blocks = (uint64_t)tiles_x * ((h + UP_H - 1) / UP_H);
	if (!blocks || blocks > 0x7FFFFFFFull)
		return hipErrorInvalidValue;
	const auto inv_sqr = [](double v) { return (float)(1.0 / (v * v)); }; /* INFINITY -> 0: the term is off */
	const float inv_n = inv_sqr(up->sigma_normal), inv_a = inv_sqr(up->sigma_albedo);
	const dim3 grid((uint32_t)blocks), block(256);
	if (up->demodulate)
		hipLaunchKernelGGL(k_upsample<true>, grid, block, 0, stream, w, h, lw, lh, tiles_x, s, up->match_material != 0, inv_n, inv_a,
				   up->sigma_plane, up->albedo_min, low_rgb, low_feat, feat, rgb, conf);
	else
		hipLaunchKernelGGL(k_upsample<false>, grid, block, 0, stream, w, h, lw, lh, tiles_x, s, up->match_material != 0, inv_n, inv_a,
				   up->sigma_plane, up->albedo_min, low_rgb, low_feat, feat, rgb, conf);
	return hipGetLastError();
}

extern "C" RTX_HIDDEN hipError_t rtx_launch_upsample_z(uint64_t n, const float4 *feat, float *z, hipStream_t stream)
{
	hipLaunchKernelGGL(k_up_z, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, n, feat, z);
	return hipGetLastError();
}

/* the tiles of a w x h frame with a pixel of conf < threshold into list (room for every tile), in increasing order;
 * count: a word per tile of scratch; out[0] = the list's length, out[1] = the pixels below the threshold */
extern "C" RTX_HIDDEN hipError_t rtx_launch_upsample_tiles(uint32_t w, uint32_t h, float threshold, const float *conf,
							   uint32_t *count, uint32_t *list, unsigned long long *out,
							   hipStream_t stream)
{
	const uint32_t total = (uint32_t)rtx_tiles_total(w, h);
	hipLaunchKernelGGL(k_up_count, dim3(total), dim3(64), 0, stream, w, h, threshold, conf, count);
	hipLaunchKernelGGL(k_up_select, dim3(1), dim3(UP_SELECT_THREADS), 0, stream, total, count, list, out);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_adaptive */
extern "C" RTX_HIDDEN hipError_t rtx_load_upsample(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_up_select);
}
