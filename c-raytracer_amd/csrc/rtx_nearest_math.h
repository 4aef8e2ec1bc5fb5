/*
 * THE DEFINITION of the closest-point queries (include/rtx.h rtx_closest_points*): the
 * distance from a point P to one object and the object's closest point cp, one function per object
 * type, compiled for the host (rtx_nearest.cpp rtx_closest_point_object) and for the device
 * (rtx_nearest.hip: the kernel's leaf tests and the known-answer entry) from this one text.
 *
 * Float32 throughout, a fixed operation order, and no floating-point contraction inside the
 * functions (the pragma below; the library's files are built with -ffp-contract=off as well), every
 * operation an IEEE one (+, -, *, /, sqrtf correctly rounded, fminf / fmaxf / fabsf exact), so the
 * host and the device return the same bits.
 *
 * Every candidate closest point is a point OF the object (up to the rounding of the point itself),
 * so a returned dist never lies below the true distance by more than that rounding: the property the
 * kernel's pruning bound relies on.
 *
 * Divisions and their guards:
 *   segment parameter  num / l2   only where l2 = |ab|^2 > 0; else t = 0 (the segment is a point).
 *                                 An overflowing quotient is clamped to [0, 1] by fmaxf / fminf, which
 *                                 also map a NaN to 0.
 *   face coordinates   ... / det  only where det = |e1|^2 |e2|^2 - (e1.e2)^2 > 0; a quotient that is
 *                                 not finite fails the in-triangle test (comparisons with NaN are
 *                                 false), and the face case is skipped: the edges answer.
 *   sphere             r / l      only where l = |P - c| > 0 and the quotient is finite; else
 *                                 cp = c + (r, 0, 0).
 */
#ifndef RTX_NEAREST_MATH_H
#define RTX_NEAREST_MATH_H

#include <math.h>

#if defined(__HIP__)
#define RTX_NM_FN __host__ __device__ static inline
#else
#define RTX_NM_FN static inline
#endif
#if defined(__clang__)
#define RTX_NM_NOCONTRACT _Pragma("clang fp contract(off)")
#else
#define RTX_NM_NOCONTRACT _Pragma("STDC FP_CONTRACT OFF")
#endif

RTX_NM_FN float rtx_nm_dot(float ax, float ay, float az, float bx, float by, float bz)
{
	RTX_NM_NOCONTRACT
	return (ax * bx + ay * by) + az * bz;
}

/* The point a + t ab of a segment closest to a + ap, as its offset t ab from a; t in [0, 1]
 * covers the two vertex regions by its clamp and the edge region between them. */
RTX_NM_FN void rtx_nm_segment(float apx, float apy, float apz, float abx, float aby, float abz, float q[3])
{
	RTX_NM_NOCONTRACT
	const float l2 = rtx_nm_dot(abx, aby, abz, abx, aby, abz);
	const float num = rtx_nm_dot(apx, apy, apz, abx, aby, abz);
	float t = 0.f;
	if (l2 > 0.f)
		t = fminf(fmaxf(num / l2, 0.f), 1.f);
	q[0] = t * abx;
	q[1] = t * aby;
	q[2] = t * abz;
}

/* |ap - q|^2, and q kept as the best offset where that is below *best2 (strictly) */
RTX_NM_FN void rtx_nm_keep(float apx, float apy, float apz, const float q[3], float *best2, float bq[3])
{
	RTX_NM_NOCONTRACT
	const float dx = apx - q[0], dy = apy - q[1], dz = apz - q[2];
	const float d2 = rtx_nm_dot(dx, dy, dz, dx, dy, dz);
	if (d2 < *best2) {
		*best2 = d2;
		bq[0] = q[0];
		bq[1] = q[1];
		bq[2] = q[2];
	}
}

/*
 * Triangle p0, p0 + e1, p0 + e2 (the record's vertex and edges: what the intersectors and the
 * device's primitive records hold).  The Voronoi regions of the closed triangle, by candidates:
 * the closest point of each edge segment (its clamp gives the vertex regions, its interior the edge
 * regions), then the face region: the foot of the perpendicular where its coordinates v, w say it
 * lies in the triangle (v >= 0, w >= 0, v + w <= 1).  The candidate of least squared distance wins,
 * the first one on ties, in the order edge p0-p1, edge p0-p2, edge p1-p2, face.
 * A zero-area triangle has det = 0 (or rounding noise of either sign): without the face case the
 * edges give the closest point of the segment or point it collapses to; with a noise det > 0 the
 * face candidate v e1 + w e2 still lies on that segment, as e1 and e2 are parallel.  No NaN: every
 * quotient is guarded as the header says.
 */
RTX_NM_FN void rtx_nm_triangle(const float p0[3], const float e1[3], const float e2[3], const float P[3], float *dist, float cp[3])
{
	RTX_NM_NOCONTRACT
	const float apx = P[0] - p0[0], apy = P[1] - p0[1], apz = P[2] - p0[2];
	float q[3], bq[3] = { 0.f, 0.f, 0.f };
	float best2 = INFINITY;
	/* edge p0 - p1 */
	rtx_nm_segment(apx, apy, apz, e1[0], e1[1], e1[2], q);
	rtx_nm_keep(apx, apy, apz, q, &best2, bq);
	/* edge p0 - p2 */
	rtx_nm_segment(apx, apy, apz, e2[0], e2[1], e2[2], q);
	rtx_nm_keep(apx, apy, apz, q, &best2, bq);
	/* edge p1 - p2, from p1 = p0 + e1 */
	{
		const float bcx = e2[0] - e1[0], bcy = e2[1] - e1[1], bcz = e2[2] - e1[2];
		rtx_nm_segment(apx - e1[0], apy - e1[1], apz - e1[2], bcx, bcy, bcz, q);
		q[0] = e1[0] + q[0];
		q[1] = e1[1] + q[1];
		q[2] = e1[2] + q[2];
		rtx_nm_keep(apx, apy, apz, q, &best2, bq);
	}
	/* face */
	{
		const float d11 = rtx_nm_dot(e1[0], e1[1], e1[2], e1[0], e1[1], e1[2]);
		const float d12 = rtx_nm_dot(e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]);
		const float d22 = rtx_nm_dot(e2[0], e2[1], e2[2], e2[0], e2[1], e2[2]);
		const float b1 = rtx_nm_dot(apx, apy, apz, e1[0], e1[1], e1[2]);
		const float b2 = rtx_nm_dot(apx, apy, apz, e2[0], e2[1], e2[2]);
		const float det = d11 * d22 - d12 * d12;
		if (det > 0.f) {
			const float v = (d22 * b1 - d12 * b2) / det, w = (d11 * b2 - d12 * b1) / det;
			if (v >= 0.f && w >= 0.f && v + w <= 1.f) {
				q[0] = v * e1[0] + w * e2[0];
				q[1] = v * e1[1] + w * e2[1];
				q[2] = v * e1[2] + w * e2[2];
				rtx_nm_keep(apx, apy, apz, q, &best2, bq);
			}
		}
	}
	*dist = sqrtf(best2);
	cp[0] = p0[0] + bq[0];
	cp[1] = p0[1] + bq[1];
	cp[2] = p0[2] + bq[2];
}

/* Sphere: dist = | |P - c| - r |, cp = c + (P - c) (r / |P - c|); P == c: cp = c + (r, 0, 0) */
RTX_NM_FN void rtx_nm_sphere(const float c[3], float r, const float P[3], float *dist, float cp[3])
{
	RTX_NM_NOCONTRACT
	const float dx = P[0] - c[0], dy = P[1] - c[1], dz = P[2] - c[2];
	const float l = sqrtf(rtx_nm_dot(dx, dy, dz, dx, dy, dz));
	*dist = fabsf(l - r);
	float s = 0.f;
	if (l > 0.f)
		s = r / l;
	if (l > 0.f && fabsf(s) <= 3.402823466e+38f) {
		cp[0] = c[0] + dx * s;
		cp[1] = c[1] + dy * s;
		cp[2] = c[2] + dz * s;
	} else {
		cp[0] = c[0] + r;
		cp[1] = c[1];
		cp[2] = c[2];
	}
}

/* Plane n . x = d (n of unit length): dist = | n . P - d |, cp = P - (n . P - d) n */
RTX_NM_FN void rtx_nm_plane(const float n[3], float d, const float P[3], float *dist, float cp[3])
{
	RTX_NM_NOCONTRACT
	const float s = rtx_nm_dot(n[0], n[1], n[2], P[0], P[1], P[2]) - d;
	*dist = fabsf(s);
	cp[0] = P[0] - s * n[0];
	cp[1] = P[1] - s * n[1];
	cp[2] = P[2] - s * n[2];
}

#endif
