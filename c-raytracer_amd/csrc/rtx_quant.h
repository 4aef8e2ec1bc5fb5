/*
 * Quantisation of the threaded BVH's boxes (rtx_device.h DQNode), shared by the uploader
 * (rtx_scene.cpp) and the device KAT of the quantised box test (rtx_shadow.hip), so the KAT
 * tests exactly the boxes the walk reads.  Compiled by hipcc only.
 *
 * A plane pair (lo, hi) on one axis of the frame (qo, qs) becomes 16-bit integers
 * ql = floor((lo - qo) * qs) - 1 and qh = ceil((hi - qo) * qs) + 1, clamped to [0, 65535]:
 * rounded outward and widened by one step on each side, so the quantised box contains the
 * float box (and the walk's rounding, far below one step, keeps the test conservative).
 */
#ifndef RTX_QUANT_H
#define RTX_QUANT_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

__host__ __device__ static inline uint32_t rtx_quantise(float lo, float hi, float qo, float qs)
{
	const double a = floor(((double)lo - qo) * (double)qs) - 1.0, b = ceil(((double)hi - qo) * (double)qs) + 1.0;
	const uint32_t ql = (uint32_t)fmin(65535.0, fmax(0.0, a)), qh = (uint32_t)fmin(65535.0, fmax(0.0, b));
	return ql | (qh << 16);
}

/* one axis of a child box in an 8-wide node's frame (rtx_device.h DW8): the 16-bit plane pair
 * q16 (rtx_quantise) relative to the node origin org (<= its lo) in steps of 2^e, rounded
 * outward, so [org + lo8 * 2^e, org + hi8 * 2^e] contains [lo16, hi16]; lo8 | hi8 << 8.  The
 * caller picks e so that hi8 <= 255. */
__host__ __device__ static inline uint32_t rtx_quantise8(uint32_t q16, uint32_t org, uint32_t e)
{
	const uint32_t lo = ((q16 & 0xFFFFu) - org) >> e, hi = ((q16 >> 16) - org + (1u << e) - 1u) >> e;
	return lo | (hi << 8);
}

/* The bounding sphere {centre, radius} of a record k_shadow tests one by one (rtx_device.h
 * DEmitter: a sphere itself, a triangle's circumscribing sphere about its centroid), formed in
 * double and padded like the cone cull's tree spheres (rtx_upload.cpp build_cull) for the kernel's
 * float test (rtx_shadow.hip point_masks). */
__host__ __device__ static inline void rtx_record_sphere(bool sphere, const float *p0, const float *p1, const float *p2, float radius,
							 float out[4])
{
	double c[3], r = 0, m = 0;
	for (int a = 0; a < 3; a++)
		c[a] = sphere ? (double)p0[a] : ((double)p0[a] + (double)p1[a] + (double)p2[a]) / 3.0;
	if (sphere) {
		r = fabs((double)radius);
	} else {
		const float *v[3] = { p0, p1, p2 };
		for (int k = 0; k < 3; k++) {
			double d2 = 0;
			for (int a = 0; a < 3; a++)
				d2 += ((double)v[k][a] - c[a]) * ((double)v[k][a] - c[a]);
			r = fmax(r, sqrt(d2));
		}
	}
	for (int a = 0; a < 3; a++) {
		m = fmax(m, fabs(c[a]));
		out[a] = (float)c[a];
	}
	out[3] = (float)(r * (1 + 1e-5) + 1e-5 * m + 1e-6);
}

#endif
