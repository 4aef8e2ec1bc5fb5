/*
 * C-ABI of include/rtx.h, the camera models beyond the pinhole: a projection's checks and basis, its host
 * specification (rtx_projection_ray), the generator (rtx_projection_rays_device, k_projection_rays) and the render of
 * its rays (rtx_render_projection*: the generator, then rtx_render_rays_device).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_projection.h"

extern "C" void rtx_projection_default(rtx_projection *p)
{
	if (!p)
		return;
	p->kind = RTX_PROJ_PANORAMA;
	p->fov = (float)(2.0 * RTX_PROJ_PI);
	p->extent = 0.f;
	p->offset_x = p->offset_y = 0.f;
}

/* what every projection entry refuses about non-null fr and pj, and the basis in double: r = unit(step_x),
 * dn = unit(step_y), f = +-(r x dn) towards the image plane's centre */
static int projection_basis(const rtx_frame *fr, const rtx_projection *pj, rtx_proj_basis *B)
{
	if (!fr->width || !fr->height || (uint64_t)fr->width * fr->height > RTX_RAYS_MAX)
		return fail(RTX_ERR_ARG, "bad frame %ux%u", fr->width, fr->height);
	if (pj->kind != RTX_PROJ_PANORAMA && pj->kind != RTX_PROJ_FISHEYE && pj->kind != RTX_PROJ_ORTHO)
		return fail(RTX_ERR_ARG, "unknown projection kind %d", pj->kind);
	/* the default, 2 pi rounded to float, lies above 2 pi */
	if (pj->kind != RTX_PROJ_ORTHO && !(pj->fov > 0.f && pj->fov <= (float)(2.0 * RTX_PROJ_PI)))
		return fail(RTX_ERR_ARG, "projection fov %g outside (0, 2 pi]", (double)pj->fov);
	if (pj->kind == RTX_PROJ_ORTHO && !(pj->extent >= 0.f && pj->extent < INFINITY))
		return fail(RTX_ERR_ARG, "orthographic extent %g is not a finite width >= 0", (double)pj->extent);
	if (!(fabsf(pj->offset_x) < INFINITY && fabsf(pj->offset_y) < INFINITY))
		return fail(RTX_ERR_ARG, "projection offsets are not finite");
	for (int k = 0; k < 3; k++)
		if (!(fabsf(fr->corner[k]) < INFINITY && fabsf(fr->step_x[k]) < INFINITY && fabsf(fr->step_y[k]) < INFINITY &&
		      fabsf(fr->origin[k]) < INFINITY))
			return fail(RTX_ERR_ARG, "the frame is not finite");
	double sx[3], sy[3], lx = 0, ly = 0;
	for (int k = 0; k < 3; k++) {
		sx[k] = fr->step_x[k];
		sy[k] = fr->step_y[k];
		lx += sx[k] * sx[k];
		ly += sy[k] * sy[k];
	}
	lx = sqrt(lx);
	ly = sqrt(ly);
	if (!(lx > 0.0) || !(ly > 0.0))
		return fail(RTX_ERR_ARG, "a frame step has zero length");
	double rd = 0;
	for (int k = 0; k < 3; k++) {
		B->r[k] = sx[k] / lx;
		B->dn[k] = sy[k] / ly;
		B->o[k] = fr->origin[k];
		rd += B->r[k] * B->dn[k];
	}
	if (fabs(rd) > 1e-3) /* a sanity limit, not a measured one */
		return fail(RTX_ERR_ARG, "the frame's steps are not perpendicular (r . dn = %g): not a rectangle", rd);
	double f[3] = { B->r[1] * B->dn[2] - B->r[2] * B->dn[1], B->r[2] * B->dn[0] - B->r[0] * B->dn[2],
			B->r[0] * B->dn[1] - B->r[1] * B->dn[0] };
	const double lf = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
	double towards = 0;
	for (int k = 0; k < 3; k++) {
		f[k] /= lf;
		const double centre = (double)fr->corner[k] + (fr->width / 2.0) * sx[k] + (fr->height / 2.0) * sy[k];
		towards += f[k] * (centre - B->o[k]);
	}
	if (!(towards != 0.0)) /* 0 or NaN */
		return fail(RTX_ERR_ARG, "the frame's origin lies in its image plane");
	for (int k = 0; k < 3; k++)
		B->f[k] = towards > 0.0 ? f[k] : -f[k];
	B->fov = pj->fov;
	B->extent = pj->extent > 0.f ? (double)pj->extent : fr->width * lx;
	B->offset_x = pj->offset_x;
	B->offset_y = pj->offset_y;
	B->width = fr->width;
	B->height = fr->height;
	B->kind = pj->kind;
	return RTX_OK;
}

extern "C" int rtx_projection_ray(const rtx_frame *fr, const rtx_projection *pj, uint32_t px, uint32_t py, rtx_ray *out)
{
	if (!fr || !pj || !out)
		return fail(RTX_ERR_ARG, "null argument");
	rtx_proj_basis B;
	const int rc = projection_basis(fr, pj, &B);
	if (rc)
		return rc;
	if (px >= fr->width || py >= fr->height)
		return fail(RTX_ERR_ARG, "pixel (%u, %u) outside the %ux%u frame", px, py, fr->width, fr->height);
	double o[3], d[3];
	memset(out, 0, sizeof(*out)); /* a hole: tmax 0 */
	if (rtx_proj_eval(B, px, py, o, d)) {
		for (int k = 0; k < 3; k++) {
			out->origin[k] = (float)o[k];
			out->dir[k] = (float)d[k];
		}
		out->tmax = INFINITY;
	}
	return RTX_OK;
}

/* checked basis, d_rays 16-byte aligned on c's device: the rays on stream, not synchronised */
static int projection_enqueue(const rtx_proj_basis &B, void *d_rays, hipStream_t stream)
{
	HIP_TRY(rtx_launch_projection_rays(&B, (float4 *)d_rays, stream));
	return RTX_OK;
}

extern "C" int rtx_projection_rays_device(rtx_ctx *c, const rtx_frame *fr, const rtx_projection *pj, void *d_rays, void *stream)
{
	if (!c || !fr || !pj || !d_rays)
		return fail(RTX_ERR_ARG, "null argument");
	rtx_proj_basis B;
	int rc = projection_basis(fr, pj, &B);
	if (rc)
		return rc;
	if ((uintptr_t)d_rays & 15u)
		return fail(RTX_ERR_ARG, "ray buffer must be 16-byte aligned");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = stream ? (hipStream_t)stream : c->stream;
	rc = projection_enqueue(B, d_rays, st);
	if (rc)
		return rc;
	HIP_TRY(hipStreamSynchronize(st));
	return RTX_OK;
}

/* what both render entries refuse before anything is launched, and the basis */
static int render_projection_check(rtx_ctx *c, const rtx_frame *fr, const rtx_projection *pj, const rtx_params *p, rtx_proj_basis *B)
{
	if (!c || !fr || !pj || !p)
		return fail(RTX_ERR_ARG, "null argument");
	const int rc = projection_basis(fr, pj, B);
	if (rc)
		return rc;
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_render_projection before rtx_upload_scene");
	return RTX_OK;
}

extern "C" int rtx_render_projection_device(rtx_ctx *c, const rtx_frame *fr, const rtx_projection *pj, const rtx_params *p, void *d_rgb,
					    void *d_z, void *stream)
{
	rtx_proj_basis B;
	int rc = render_projection_check(c, fr, pj, p, &B);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = stream ? (hipStream_t)stream : c->stream;
	if (c->d_rr_rays.grow((size_t)fr->width * fr->height * sizeof(rtx_ray)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "rays of %ux%u pixels", fr->width, fr->height);
	rc = projection_enqueue(B, c->d_rr_rays, st);
	if (rc)
		return rc;
	return rtx_render_rays_device(c, fr->width, fr->height, c->d_rr_rays, p, d_rgb, d_z, st);
}

extern "C" int rtx_render_projection(rtx_ctx *c, const rtx_frame *fr, const rtx_projection *pj, const rtx_params *p, float *rgb, float *z)
{
	rtx_proj_basis B;
	int rc = render_projection_check(c, fr, pj, p, &B);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	if (c->d_rr_rays.grow(px * sizeof(rtx_ray)) != hipSuccess)
		return fail(RTX_ERR_NOMEM, "rays of %ux%u pixels", fr->width, fr->height);
	/* pixels of tiles outside this shard keep the caller's values */
	if (p->tile_stride > 1) {
		if (rgb)
			HIP_TRY(hipMemcpyAsync(c->d_rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
		if (z)
			HIP_TRY(hipMemcpyAsync(c->d_z, z, px * 4, hipMemcpyHostToDevice, c->stream));
	}
	rc = projection_enqueue(B, c->d_rr_rays, c->stream);
	if (rc)
		return rc;
	rc = rtx_render_rays_device(c, fr->width, fr->height, c->d_rr_rays, p, rgb ? c->d_rgb : nullptr, z ? c->d_z : nullptr, c->stream);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}
