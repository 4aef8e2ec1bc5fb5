/*
 * Variance-guided denoiser kernels: the a-trous filter of rtx_denoise.hip with the colour
 * distance measured in the pixel's own estimated noise, the variance carried through the levels and
 * handed back.  Input: the mean and the variance of the mean that rtx_render_passes* / _adaptive* write.
 *
 *   k_dnv_pack     rtx_feature records, the packed rgb frame and the packed variance into the filter's
 *                  16-byte records, one array each: colour {r, g, b, live}, variance {V_r, V_g, V_b, live},
 *                  {P, z}, {n, -}, {albedo, -}.  live = the pixel takes part in the filter: z != 0, a
 *                  finite colour and every variance component finite and >= 0 (the variance record
 *                  repeats the flag, so the local noise needs the variance array alone).  Counts the hit
 *                  pixels as k_dn_pack does (an integer sum, one add per block).
 *   k_dnv_level    one level of the filter at step s.  Local noise g_i: the mean of V_r + V_g + V_b over
 *                  the adjacent (step 1 at every level) live in-frame pixels, weights b[u] b[v] with
 *                  b = (1/4, 1/2, 1/4), normalised by the weights used: 9 variance loads.  Then the 5 x 5
 *                  taps at i + (u, v) * s, each five 16-byte loads, weight h[u] h[v] exp(-e) with
 *                    e_c = 0 where |c_i - c_j|^2 == 0, else |c_i - c_j|^2 / (sigma_c^2 2 g_i)
 *                    e = e_c + |n_i - n_j|^2 / sigma_n^2 + |a_i - a_j|^2 / sigma_a^2
 *                      + (n_i . (P_j - P_i))^2 / (sigma_p z_i)^2,
 *                  h = (1/16, 1/4, 3/8, 1/4, 1/16); c' = c_i + sum w (c_j - c_i) / sum w and, per channel,
 *                  V' = sum w^2 V_j / (sum w)^2.  sigma_c is a number of standard deviations of a colour
 *                  difference and is the same at every level: the shrinking variance tightens it.  The
 *                  reciprocal 1 / (2 sigma_c^2 g_i) is formed once per pixel; g_i == 0 makes it infinite
 *                  and the zero-difference case is selected, not left to 0 * inf, so an all-zero
 *                  variance returns the colour's bits.  16 x 16 pixels per 256-thread block, one output
 *                  pixel per lane, every tap bounds-checked as in k_dn_level.  A pixel that is not live
 *                  keeps the bits of its colour and its variance and no tap reads it.  No atomics: two
 *                  runs give the same bits.  The last level writes the packed rgb and variance frames.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"

static_assert(sizeof(rtx_feature) == 48, "k_dnv_pack reads a feature record as three float4");

__device__ __forceinline__ bool dnv_finite3(float x, float y, float z)
{
	return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}

__global__ __launch_bounds__(256) void k_dnv_pack(uint64_t n, const float4 *__restrict__ feat, const float *__restrict__ rgb,
						  const float *__restrict__ variance, float4 *__restrict__ col,
						  float4 *__restrict__ var, float4 *__restrict__ pz, float4 *__restrict__ nrm,
						  float4 *__restrict__ alb, unsigned long long *__restrict__ hit_count)
{
	__shared__ uint32_t wave_hits[4];
	uint32_t hits = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
		const float4 f0 = feat[3 * i], f1 = feat[3 * i + 1], f2 = feat[3 * i + 2];
		const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
		const float vr = variance[3 * i], vg = variance[3 * i + 1], vb = variance[3 * i + 2];
		const bool hit = f0.w != 0.f;
		hits += hit;
		/* x >= 0 is false for a NaN, and -0 is a variance of 0 */
		const bool ok = hit && dnv_finite3(r, g, b) && dnv_finite3(vr, vg, vb) && vr >= 0.f && vg >= 0.f && vb >= 0.f;
		const float live = ok ? 1.f : 0.f;
		col[i] = make_float4(r, g, b, live);
		var[i] = make_float4(vr, vg, vb, live);
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
__global__ __launch_bounds__(256) void k_dnv_level(uint32_t w, uint32_t h, uint32_t tiles_x, uint64_t tiles, uint32_t step,
						   float two_c2, float inv_n, float inv_a, float sigma_p,
						   const float4 *__restrict__ col, const float4 *__restrict__ var,
						   const float4 *__restrict__ pz, const float4 *__restrict__ nrm,
						   const float4 *__restrict__ alb, float4 *__restrict__ out_col,
						   float4 *__restrict__ out_var, float *__restrict__ rgb, float *__restrict__ variance)
{
#pragma clang fp contract(fast)
	constexpr float kh[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f };
	constexpr float kb[3] = { 1.f / 4.f, 1.f / 2.f, 1.f / 4.f };
	for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
		const uint32_t x = (uint32_t)(t % tiles_x) * 16u + (threadIdx.x & 15u);
		const uint32_t y = (uint32_t)(t / tiles_x) * 16u + (threadIdx.x >> 4);
		if (x >= w || y >= h)
			continue;
		const size_t i = (size_t)y * w + x;
		const float4 ci = col[i], vi = var[i];
		float r = ci.x, g = ci.y, b = ci.z, vr = vi.x, vg = vi.y, vb = vi.z;
		if (ci.w != 0.f) {
			/* the local noise: the centre is live, so the weights used sum to 1/4 at least */
			float gs = 0.f, gw = 0.f;
#pragma unroll
			for (int v = 0; v < 3; v++) {
				const uint32_t yj = y + (uint32_t)(v - 1);
				const bool iny = yj < h;
				const size_t row = (size_t)(iny ? yj : y) * w;
#pragma unroll
				for (int u = 0; u < 3; u++) {
					const uint32_t xj = x + (uint32_t)(u - 1);
					const bool in = iny && xj < w;
					const float4 vj = var[in ? row + xj : i];
					const bool ok = in && vj.w != 0.f;
					gs += ok ? kb[u] * kb[v] * (vj.x + vj.y + vj.z) : 0.f;
					gw += ok ? kb[u] * kb[v] : 0.f;
				}
			}
			/* 1 / (2 sigma_c^2 g_i), once per pixel: infinite where g_i == 0, 0 where sigma_c is infinite */
			const float kc = two_c2 < INFINITY ? 1.f / (two_c2 * (gs / gw)) : 0.f;
			const float4 pi = pz[i], ni = nrm[i], ai = alb[i];
			const float sz = sigma_p * pi.w;
			const float inv_p = 1.f / (sz * sz);
			float ar = 0.f, ag = 0.f, ab = 0.f, sw = 0.f, qr = 0.f, qg = 0.f, qb = 0.f;
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
					const float4 cj = col[j], vj = var[j], pj = pz[j], nj = nrm[j], aj = alb[j];
					const bool ok = in && cj.w != 0.f;
					const float dr = ok ? cj.x - r : 0.f, dg = ok ? cj.y - g : 0.f, db = ok ? cj.z - b : 0.f;
					const float nx = nj.x - ni.x, ny = nj.y - ni.y, nz = nj.z - ni.z;
					const float ax = aj.x - ai.x, ay = aj.y - ai.y, az = aj.z - ai.z;
					const float pd = ni.x * (pj.x - pi.x) + ni.y * (pj.y - pi.y) + ni.z * (pj.z - pi.z);
					const float d2 = dr * dr + dg * dg + db * db;
					const float e = (d2 == 0.f ? 0.f : d2 * kc) + (nx * nx + ny * ny + nz * nz) * inv_n +
							(ax * ax + ay * ay + az * az) * inv_a + pd * pd * inv_p;
					float wt = kh[u] * kh[v] * __expf(-e);
					wt = (ok && wt >= 0.f) ? wt : 0.f; /* a NaN e (0 * inf) weighs nothing */
					const float w2 = wt * wt;
					ar += wt * dr;
					ag += wt * dg;
					ab += wt * db;
					sw += wt;
					qr += ok ? w2 * vj.x : 0.f;
					qg += ok ? w2 * vj.y : 0.f;
					qb += ok ? w2 * vj.z : 0.f;
				}
			}
			if (sw > 0.f) {
				const float inv = 1.f / sw, inv2 = inv * inv;
				/* a zero sum leaves c_i's bits (-0 + 0 would be +0) */
				const float fr = ar != 0.f ? r + ar * inv : r, fg = ag != 0.f ? g + ag * inv : g,
					    fb = ab != 0.f ? b + ab * inv : b;
				const float ur = qr * inv2, ug = qg * inv2, ub = qb * inv2;
				/* differences of colours near FLT_MAX overflow, and so can w^2 V: keep c_i and V_i */
				if (dnv_finite3(fr, fg, fb) && dnv_finite3(ur, ug, ub)) {
					r = fr;
					g = fg;
					b = fb;
					vr = ur;
					vg = ug;
					vb = ub;
				}
			}
		}
		if (LAST) {
			rgb[3 * i] = r;
			rgb[3 * i + 1] = g;
			rgb[3 * i + 2] = b;
			variance[3 * i] = vr;
			variance[3 * i + 1] = vg;
			variance[3 * i + 2] = vb;
		} else {
			out_col[i] = make_float4(r, g, b, ci.w);
			out_var[i] = make_float4(vr, vg, vb, vi.w);
		}
	}
}

/* the filter on device buffers: feat (rtx_feature records), rgb and variance (packed, in/out) are the caller's,
 * work = 7 * n float4 of scratch (colour ping and pong, variance ping and pong, {P, z}, n, albedo), hit_count
 * one zeroed word */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_launch_denoise_variance(uint32_t w, uint32_t h,
											    const rtx_denoise_variance_params *dp,
											    const float4 *feat, float *rgb, float *variance,
											    float4 *work, unsigned long long *hit_count,
											    hipStream_t stream)
{
	const uint64_t n = (uint64_t)w * h;
	float4 *col[2] = { work, work + n }, *var[2] = { work + 2 * n, work + 3 * n };
	float4 *pz = work + 4 * n, *nrm = work + 5 * n, *alb = work + 6 * n;
	const uint64_t blocks = (n + 255) / 256;
	hipLaunchKernelGGL(k_dnv_pack, dim3((uint32_t)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, stream, n, feat, rgb, variance,
			   col[0], var[0], pz, nrm, alb, hit_count);
	const uint32_t tiles_x = (w + 15) / 16;
	const uint64_t tiles = (uint64_t)tiles_x * ((h + 15) / 16);
	const dim3 grid((uint32_t)(tiles < (1u << 20) ? tiles : (1u << 20)));
	const auto inv_sqr = [](double s) { return (float)(1.0 / (s * s)); }; /* INFINITY -> 0: the term is off */
	const float inv_n = inv_sqr(dp->sigma_normal), inv_a = inv_sqr(dp->sigma_albedo);
	/* 2 sigma_c^2: the variance of a difference of two equally noisy estimates, in sigma_c standard deviations;
	 * INFINITY (or a product beyond float) switches the term off */
	const float two_c2 = (float)(2.0 * (double)dp->sigma_color * (double)dp->sigma_color);
	for (uint32_t k = 0; k < dp->iterations; k++) {
		const float4 *sc = col[k & 1], *sv = var[k & 1];
		if (k + 1 == dp->iterations)
			hipLaunchKernelGGL(k_dnv_level<true>, grid, dim3(256), 0, stream, w, h, tiles_x, tiles, 1u << k, two_c2, inv_n, inv_a,
					   dp->sigma_plane, sc, sv, pz, nrm, alb, (float4 *)nullptr, (float4 *)nullptr, rgb, variance);
		else
			hipLaunchKernelGGL(k_dnv_level<false>, grid, dim3(256), 0, stream, w, h, tiles_x, tiles, 1u << k, two_c2, inv_n,
					   inv_a, dp->sigma_plane, sc, sv, pz, nrm, alb, col[(k + 1) & 1], var[(k + 1) & 1],
					   (float *)nullptr, (float *)nullptr);
	}
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_denoise */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_load_denoise_variance(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_dnv_pack);
}
