/*
 * The camera models of rtx_projection (include/rtx.h): one text of the formulas for the host specification
 * (rtx_projection_ray, rtx_projection.cpp) and the generator kernel (k_projection_rays, rtx_projection.hip).
 * Everything is double; the caller rounds the ray once to float.
 */
#ifndef RTX_PROJECTION_H
#define RTX_PROJECTION_H

#include <math.h>
#include <stdint.h>

#include "rtx.h"

#if defined(__HIPCC__)
#define RTX_PROJ_FN __host__ __device__ inline
#else
#define RTX_PROJ_FN inline
#endif

#define RTX_PROJ_PI 3.14159265358979323846

/* a checked projection of a checked frame (rtx_projection_basis): the basis r, dn, f in double, the frame's origin and
 * size, and the projection's fields widened */
struct rtx_proj_basis {
	double r[3], dn[3], f[3], o[3];
	double fov, extent, offset_x, offset_y; /* extent: E, the image plane's own width where rtx_projection has 0 */
	uint32_t width, height;
	int32_t kind;
};

/* pixel (px, py)'s ray: false = a hole (o and d are not written) */
RTX_PROJ_FN bool rtx_proj_eval(const rtx_proj_basis &B, uint32_t px, uint32_t py, double o[3], double d[3])
{
	const double W = (double)B.width, H = (double)B.height;
	const double u = ((double)px + 0.5 + B.offset_x) / W, v = ((double)py + 0.5 + B.offset_y) / H;
	for (int k = 0; k < 3; k++)
		o[k] = B.o[k];
	if (B.kind == RTX_PROJ_PANORAMA) {
		const double lam = (u - 0.5) * B.fov;
		const double phi = (0.5 - v) * RTX_PROJ_PI * (B.fov / (2.0 * RTX_PROJ_PI)) * (2.0 * H / W);
		if (fabs(phi) > RTX_PROJ_PI / 2.0)
			return false;
		const double cp = cos(phi), sp = sin(phi), cl = cos(lam), sl = sin(lam);
		for (int k = 0; k < 3; k++)
			d[k] = cp * (sl * B.r[k] + cl * B.f[k]) - sp * B.dn[k];
		return true;
	}
	if (B.kind == RTX_PROJ_FISHEYE) {
		const double x = 2.0 * u - 1.0, y = (2.0 * v - 1.0) * H / W;
		const double rho = sqrt(x * x + y * y), theta = rho * B.fov / 2.0;
		if (theta > RTX_PROJ_PI)
			return false;
		if (rho == 0.0) {
			for (int k = 0; k < 3; k++)
				d[k] = B.f[k];
			return true;
		}
		const double ct = cos(theta), st = sin(theta);
		for (int k = 0; k < 3; k++)
			d[k] = ct * B.f[k] + st * (x * B.r[k] + y * B.dn[k]) / rho;
		return true;
	}
	/* RTX_PROJ_ORTHO */
	for (int k = 0; k < 3; k++) {
		d[k] = B.f[k];
		o[k] = B.o[k] + (u - 0.5) * B.extent * B.r[k] + (v - 0.5) * B.extent * (H / W) * B.dn[k];
	}
	return true;
}

#endif
