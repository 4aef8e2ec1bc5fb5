/*
 * Denoiser kernels: per-pixel feature records of a frame's primary hits and an
 * edge-aware a-trous filter of an rgb frame guided by them.
 *
 *   k_dn_features  a frame ray (k_frame_rays) and its closest hit (k_rays) into an rtx_feature:
 *                  P = dir * t + origin as hit_info forms it, z = t, the hit's normal, material
 *                  and object, albedo = texture_color(material, P): the colour k_trace stores as
 *                  the shade point's tex.  One pixel per lane.
 *   k_dn_pack      rtx_feature records and the packed rgb frame into the filter's 16-byte
 *                  records, one array each: colour {r, g, b, live}, {P, z}, {n, -}, {albedo, -}.
 *                  live = the pixel takes part in the filter: z != 0 and a finite colour.  Counts the
 *                  hit pixels (an integer sum, one add per block) for rtx_denoise_stats.
 *   k_dn_level     one level of the filter at step s: the 5 x 5 taps at i + (u, v) * s, each four
 *                  16-byte loads, weight h[u] h[v] exp(-e) with
 *                    e = |c_i - c_j|^2 / sigma_c^2 + |n_i - n_j|^2 / sigma_n^2
 *                      + |a_i - a_j|^2 / sigma_a^2 + (n_i . (P_j - P_i))^2 / (sigma_p z_i)^2,
 *                  h = (1/16, 1/4, 3/8, 1/4, 1/16).  16 x 16 pixels per 256-thread block, one
 *                  output pixel per lane, every tap bounds-checked.  The weighted mean is formed
 *                  about the centre, out = c_i + sum w (c_j - c_i) / sum w (the differences are
 *                  there for e anyway), so a constant colour comes back exactly.  A pixel that
 *                  is not live keeps its colour's bits and no tap reads it.  No atomics: two
 *                  runs give the same bits.  The last level writes the packed rgb frame.
 * Levels read their taps from memory (L1 / L2 serve the 25-fold reuse); no LDS staging.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_launch.h"
#include "rtx_math.h"

static_assert(sizeof(rtx_feature) == 48, "k_dn_features writes a feature record as three float4");

__global__ __launch_bounds__(256) void k_dn_features(uint64_t n, const float4 *__restrict__ rays, const float4 *__restrict__ hits,
						     const DMaterial *__restrict__ mats, int u32conv, float4 *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const float4 h0 = hits[2 * i];
	const int32_t obj = (int32_t)__float_as_uint(h0.y), mat = (int32_t)__float_as_uint(h0.z);
	float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu)), f2 = f1;
	if (obj >= 0 && mat >= 0) {
		const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1], h1 = hits[2 * i + 1];
		const float t = h0.x;
		const f3 p = add3(mul3s(mk3(r1.x, r1.y, r1.z), t), mk3(r0.x, r0.y, r0.z));
		const f3 a = texture_color(mats[mat], p, u32conv);
		f0 = make_float4(p.x, p.y, p.z, t);
		f1 = make_float4(h1.x, h1.y, h1.z, h0.z);
		f2 = make_float4(a.x, a.y, a.z, h0.y);
	}
	out[3 * i] = f0;
	out[3 * i + 1] = f1;
	out[3 * i + 2] = f2;
}

__device__ __forceinline__ bool dn_finite3(float x, float y, float z)
{
	return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

__global__ __launch_bounds__(256) void k_dn_pack(uint64_t n, const float4 *__restrict__ feat, const float *__restrict__ rgb,
						 float4 *__restrict__ col, float4 *__restrict__ pz, float4 *__restrict__ nrm,
						 float4 *__restrict__ alb, unsigned long long *__restrict__ hit_count)
{
	/* a bounded grid that strides over the frame: the hit pixels are summed per block (one add per wave of a
	 * 1080p frame, 32 400 of them on one address, took 0.35 ms of this kernel's 0.39) */
	__shared__ uint32_t wave_hits[4];
	uint32_t hits = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		const float4 f0 = feat[3 * i], f1 = feat[3 * i + 1], f2 = feat[3 * i + 2];
		const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
		const bool hit = f0.w != 0.f;
		hits += hit;
		col[i] = make_float4(r, g, b, hit && dn_finite3(r, g, b) ? 1.f : 0.f);
		pz[i] = f0;
		nrm[i] = f1;
		alb[i] = f2;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		hits += __shfl_xor(hits, o, 64);
	if ((threadIdx.x & 63u) == 0)
		wave_hits[threadIdx.x >> 6] = hits;
	__syncthreads();
	if (threadIdx.x == 0) {
		const uint32_t s = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
		if (s)
			atomicAdd(hit_count, (unsigned long long)s);
	}
}

template <bool LAST>
__global__ __launch_bounds__(256) void k_dn_level(uint32_t w, uint32_t h, uint32_t tiles_x, uint64_t tiles, uint32_t step,
						  float inv_c, float inv_n, float inv_a, float sigma_p,
						  const float4 *__restrict__ col, const float4 *__restrict__ pz,
						  const float4 *__restrict__ nrm, const float4 *__restrict__ alb,
						  float4 *__restrict__ out, float *__restrict__ rgb)
{
#pragma clang fp contract(fast)
	constexpr float kh[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f };
	for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
		const uint32_t x = (uint32_t)(t % tiles_x) * 16u + (threadIdx.x & 15u);
		const uint32_t y = (uint32_t)(t / tiles_x) * 16u + (threadIdx.x >> 4);
		if (x >= w || y >= h)
			continue;
		const size_t i = (size_t)y * w + x;
		const float4 ci = col[i];
		float r = ci.x, g = ci.y, b = ci.z;
		if (ci.w != 0.f) {
			const float4 pi = pz[i], ni = nrm[i], ai = alb[i];
			const float sz = sigma_p * pi.w;
			const float inv_p = 1.f / (sz * sz);
			float ar = 0.f, ag = 0.f, ab = 0.f, sw = 0.f;
#pragma unroll
			for (int v = 0; v < 5; v++) {
				/* w * h < 2^31 and |offset| <= 256: a coordinate left of 0 wraps above any width */
				const uint32_t yj = y + (uint32_t)((v - 2) * (int)step);
				const bool iny = yj < h;
				const size_t row = (size_t)(iny ? yj : y) * w;
#pragma unroll
				for (int u = 0; u < 5; u++) {
					const uint32_t xj = x + (uint32_t)((u - 2) * (int)step);
					const bool in = iny && xj < w;
					const size_t j = in ? row + xj : i;
					const float4 cj = col[j], pj = pz[j], nj = nrm[j], aj = alb[j];
					const bool ok = in && cj.w != 0.f;
					const float dr = ok ? cj.x - r : 0.f, dg = ok ? cj.y - g : 0.f, db = ok ? cj.z - b : 0.f;
					const float nx = nj.x - ni.x, ny = nj.y - ni.y, nz = nj.z - ni.z;
					const float ax = aj.x - ai.x, ay = aj.y - ai.y, az = aj.z - ai.z;
					const float pd = ni.x * (pj.x - pi.x) + ni.y * (pj.y - pi.y) + ni.z * (pj.z - pi.z);
					const float e = (dr * dr + dg * dg + db * db) * inv_c + (nx * nx + ny * ny + nz * nz) * inv_n +
							(ax * ax + ay * ay + az * az) * inv_a + pd * pd * inv_p;
					float wt = kh[u] * kh[v] * __expf(-e);
					wt = (ok && wt >= 0.f) ? wt : 0.f; /* a NaN e (0 * inf) weighs nothing */
					ar += wt * dr;
					ag += wt * dg;
					ab += wt * db;
					sw += wt;
				}
			}
			if (sw > 0.f) {
				const float inv = 1.f / sw;
				const float fr = r + ar * inv, fg = g + ag * inv, fb = b + ab * inv;
				if (dn_finite3(fr, fg, fb)) { /* differences of colours near FLT_MAX overflow: keep c_i */
					r = fr;
					g = fg;
					b = fb;
				}
			}
		}
		if (LAST) {
			rgb[3 * i] = r;
			rgb[3 * i + 1] = g;
			rgb[3 * i + 2] = b;
		} else {
			out[i] = make_float4(r, g, b, ci.w);
		}
	}
}

extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_launch_dn_features(uint64_t n, const float4 *rays, const float4 *hits,
										      const DMaterial *mats, int u32conv, float4 *out,
										      hipStream_t stream)
{
	hipLaunchKernelGGL(k_dn_features, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, n, rays, hits, mats, u32conv, out);
	return hipGetLastError();
}

/* the filter on device buffers: feat (rtx_feature records) and rgb (packed, in/out) are the caller's,
 * work = 5 * n float4 of scratch (colour ping, colour pong, {P, z}, n, albedo), hit_count one zeroed word */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_launch_denoise(uint32_t w, uint32_t h, const rtx_denoise_params *dp,
										  const float4 *feat, float *rgb, float4 *work,
										  unsigned long long *hit_count, hipStream_t stream)
{
	const uint64_t n = (uint64_t)w * h;
	float4 *col[2] = { work, work + n };
	float4 *pz = work + 2 * n, *nrm = work + 3 * n, *alb = work + 4 * n;
	const uint64_t blocks = (n + 255) / 256;
	hipLaunchKernelGGL(k_dn_pack, dim3((uint32_t)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, n, feat, rgb, col[0], pz, nrm,
			   alb, hit_count);
	const uint32_t tiles_x = (w + 15) / 16;
	const uint64_t tiles = (uint64_t)tiles_x * ((h + 15) / 16);
	const dim3 grid((uint32_t)(tiles < (1u << 20) ? tiles : (1u << 20)));
	const auto inv_sqr = [](double s) { return (float)(1.0 / (s * s)); }; /* INFINITY -> 0: the term is off */
	const float inv_n = inv_sqr(dp->sigma_normal), inv_a = inv_sqr(dp->sigma_albedo);
	for (uint32_t k = 0; k < dp->iterations; k++) {
		const float inv_c = inv_sqr((double)dp->sigma_color / (double)(1u << k));
		const float4 *src = col[k & 1];
		if (k + 1 == dp->iterations)
			hipLaunchKernelGGL(k_dn_level<true>, grid, dim3(256), 0, stream, w, h, tiles_x, tiles, 1u << k, inv_c, inv_n, inv_a,
					   dp->sigma_plane, src, pz, nrm, alb, (float4 *)nullptr, rgb);
		else
			hipLaunchKernelGGL(k_dn_level<false>, grid, dim3(256), 0, stream, w, h, tiles_x, tiles, 1u << k, inv_c, inv_n, inv_a,
					   dp->sigma_plane, src, pz, nrm, alb, col[(k + 1) & 1], (float *)nullptr);
	}
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_post */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_load_denoise(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_dn_features);
}
