/*
 * k_projection_rays: the primary rays of a panoramic, fisheye or orthographic camera (include/rtx.h rtx_projection) as
 * rtx_ray records for rtx_render_rays_device, one pixel per lane, row-major.  The formulas (rtx_projection.h, the
 * text rtx_projection_ray evaluates on the host) run in double and each component is rounded once to float: the
 * kernel writes 32 bytes per pixel, which bounds it, not its arithmetic.  tmax = INFINITY, or 0 for a hole.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_launch.h"
#include "rtx_projection.h"

static_assert(sizeof(rtx_ray) == 32, "k_projection_rays writes a ray as two float4");

__global__ __launch_bounds__(256) void k_projection_rays(rtx_proj_basis B, float4 *__restrict__ rays)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= (uint64_t)B.width * B.height)
		return;
	const uint32_t px = (uint32_t)(i % B.width), py = (uint32_t)(i / B.width);
	double o[3], d[3];
	float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, 0.f, 0.f);
	if (rtx_proj_eval(B, px, py, o, d)) {
		r0 = make_float4((float)o[0], (float)o[1], (float)o[2], INFINITY);
		r1 = make_float4((float)d[0], (float)d[1], (float)d[2], 0.f);
	}
	rays[2 * i] = r0;
	rays[2 * i + 1] = r1;
}

/* B: a checked basis (rtx_projection.cpp), width * height <= RTX_RAYS_MAX; rays: width * height records, 16-byte aligned */
extern "C" RTX_HIDDEN hipError_t rtx_launch_projection_rays(const rtx_proj_basis *B, float4 *rays, hipStream_t stream)
{
	const uint64_t n = (uint64_t)B->width * B->height;
	if (!n || n > RTX_RAYS_MAX)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_projection_rays, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, *B, rays);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded at rtx_open like rtx_load_temporal */
extern "C" RTX_HIDDEN hipError_t rtx_load_projection(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_projection_rays);
}
