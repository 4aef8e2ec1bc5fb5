/*
 * The lane stack of the per-lane tree walks in the persistent one-wave-per-workgroup kernels: k_trace and
 * k_rays (rtx_trace.hip's translation unit: both closest-hit walks) and k_nearest (rtx_nearest.hip).
 */
#ifndef RTX_LANE_STACK_H
#define RTX_LANE_STACK_H

#include "rtx_device.h"
#include "rtx_w8.h"
#include "rtx_wave.h"

/* A lane's stack of node references: the first RTX_TRACE_LSTK entries in the workgroup's LDS, the rest in HBM
 * (DScene.ostk, which the host sizes for this launch's own grid), both [entry][lane].  A lane's address is
 * formed at each use (lane_id), none kept live across the walk.  CAP: a push beyond DScene.stack_size entries
 * is refused, never written (k_nearest; no tree is that deep, one entry per level at most). */
template <bool CAP> struct LaneStack {
	lds_u32 *ls;
	uint32_t *os;
	size_t ostride;
	uint32_t cap, sp;
	__device__ __forceinline__ void push(uint32_t v)
	{
		if (CAP && sp >= cap)
			return;
		if (sp < RTX_TRACE_LSTK)
			ls[sp * WAVE + lane_id()] = v;
		else
			os[(sp - RTX_TRACE_LSTK) * ostride + lane_id()] = v;
		sp++;
	}
	__device__ __forceinline__ uint32_t pop()
	{
		sp--;
		return sp < RTX_TRACE_LSTK ? ls[sp * WAVE + lane_id()] : os[(sp - RTX_TRACE_LSTK) * ostride + lane_id()];
	}
};
/* the empty stack of this wave, its LDS entries at lds */
template <bool CAP> __device__ __forceinline__ LaneStack<CAP> lane_stack(const DScene &S, void *lds)
{
	return { (lds_u32 *)lds, S.ostk + (size_t)blockIdx.x * WAVE, (size_t)gridDim.x * WAVE, S.stack_size, 0u };
}

#endif
