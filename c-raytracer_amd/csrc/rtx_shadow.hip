/*
 * k_shadow: direct lighting of every shade point (render.c:170-229) on gfx950.
 *
 * Shadow rays are 95.9-99.6 % of the reference's rays (is_light_blocked,
 * render.c:126-134 -> object.c:183-197 + accel.c:360-387).  Each (shade point,
 * light sample) pair is one lane: the lane samples its light point, tests the
 * unbound planes, walks the BVH for any opaque blocker (multiplying the
 * transmittance of transparent ones), then evaluates Phong / Blinn.
 *
 * The walk: every lane walks its own shadow ray over the 8-wide compressed BVH
 * (rtx_device.h DW8, shadow_walk8): one 64-byte node per step, eight box tests
 * per memory round trip, pending siblings as (base, slot mask) groups in a
 * register, an LDS lane stack and HBM below it (any depth).  A step whose walking
 * lanes share one node reads it through the scalar cache; other steps read the
 * tree's top three levels from the workgroup's LDS copy (DScene.w8top) and the
 * rest from memory.  Small scenes (the whole threaded BVH2 fits the LDS top copy)
 * may walk the threaded BVH2 instead (shadow_walk: one 16-byte record per step,
 * no stack, read from LDS), and tiny ones test their few objects one by one
 * (DScene.lin, no walk).  The walks test boxes in the tree's frame (DScene.tf:
 * the rotation the uploader chose for the leaf boxes) and primitives in world
 * space.  The emitter and material records of a one-point packet are read
 * through the scalar cache.
 *
 * Scheduling: persistent workgroups; each wave takes `per_wave` shade points at
 * a time from a global queue in Morton order of their position (rtx_sort.hip),
 * so the resident waves share one compact region of the tree in L2.  A point's
 * samples fill whole power-of-two lane slots and its sum runs inside one wave
 * in lane order, so its result does not depend on which wave takes it.
 *
 * This file holds everything compiled into a k_shadow<...> instance: the intersection
 * tests, both walks, shadow_query, sampling and shading, the per-point masks, the sample
 * order and the kernel.  The rest of the translation unit (one object, because the device
 * functions here are shared) is included at the end, a part each:
 *   rtx_shadow_premask.h    k_point_masks: the per-point masks ahead of k_shadow
 *   rtx_shadow_clearlane.h  the partition kernels and k_shadow_clear: all-clear points, one per lane
 *   rtx_shadow_rays.h       k_shadow_rays: shadow_query on a caller's shadow rays
 *                           (rtx_trace_shadow_rays)
 *   rtx_shadow_kat.h        the known-answer-test kernels of the device functions here
 *   rtx_shadow_launch.h     k_w8_fill and the host launch code
 * Code that k_shadow executes stays in this file: bench.py ties a committed counter summary
 * to the kernel by a hash of this file and of the headers included below, not of those parts.
 */
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdlib.h>

#include "rtx_kat.h"
#include "rtx_quant.h"
#include "rtx_wave.h"
#include "rtx_w8.h"
#include "rtx_launch.h"

/* The compile-time switches of this translation unit (rtx_w8.h has the 8-wide node test's, which k_trace
 * shares).  Measurement only, the images are wrong: */
#ifndef RTX_DEBUG_NOWALK
#define RTX_DEBUG_NOWALK 0 /* skip the BVH walk; 1: walking points become all-clear points, 2: their runs are still ordered */
#endif
#ifndef RTX_DEBUG_NOLEAF
#define RTX_DEBUG_NOLEAF 0 /* the walk tests no leaf (the cost of the leaf tests) */
#endif
/* The occupancy the instances are register-capped for (__launch_bounds__): */
#ifndef RTX_SHADOW_OCC_DEFAULT
#define RTX_SHADOW_OCC_DEFAULT 8 /* waves per SIMD the walk is register-capped for */
#endif
#ifndef RTX_SHADOW_OCC_SLOT
#define RTX_SHADOW_OCC_SLOT RTX_SHADOW_OCC_DEFAULT /* the same for the lane-slot kernel */
#endif
/* Tunable counts of the 8-wide walk (shadow_walk8): */
#ifndef RTX_W8_TQ
#define RTX_W8_TQ 4 /* deferred leaf groups per lane in LDS (besides the one in a register) */
#endif
#ifndef RTX_W8_DEFER
#define RTX_W8_DEFER 64 /* lanes holding deferred leaf tests that trigger a round of them (16 / 32 / 48 / 64: 613 / 601 / 598 / 594 ms) */
#endif
/* Numerical forms; 0 restores the reference's arithmetic (how a parity difference is bisected; the KATs name them): */
#ifndef RTX_SH_FASTSQRT
#define RTX_SH_FASTSQRT 1 /* the shadow ray's length from v_sqrt_f32 (1 ulp) instead of the correctly rounded sequence */
#endif
#ifndef RTX_SH_FASTPOW
#define RTX_SH_FASTPOW 1 /* specular powf from v_log_f32 / v_exp_f32 (sh_pow) */
#endif
#ifndef RTX_SH_FASTTRIG
#define RTX_SH_FASTTRIG 1 /* a sphere light's sines and cosines from the revolution-scaled v_sin_f32 / v_cos_f32 (light_point_sh) */
#endif
#ifndef RTX_SH_FASTDIV
#define RTX_SH_FASTDIV 1 /* 1/x in light sampling and attenuation from v_rcp_f32 (1 ulp); the closest-hit path keeps IEEE division */
#endif
#ifndef RTX_SH_PLANE_RCP
#define RTX_SH_PLANE_RCP 1 /* the plane test's quotient as num * v_rcp_f32(a) (plane_blocks) */
#endif
#ifndef RTX_SH_FARLIN
#define RTX_SH_FARLIN 0 /* far shade points: objects tested one by one are culled by their world boxes first (1), spheres only (2) */
#endif

/* ------------------------------------------------------------------------ */
/* intersection tests of the any-hit walk                                   */
/* ------------------------------------------------------------------------ */
/* The slab test (accel.c:112-158) against a DQNode box, in the quantisation frame: the ray is
 * transformed once per walk (o' = (o - qo) * qs, inv' = inv / qs, oi = o' * inv'), so
 * t = q * inv' - oi is the world ray parameter, with the 16-bit plane coordinates converted by
 * one SDWA v_cvt_f32_u32 each.  OCT < 8: every live lane's direction lies in octant OCT (bit a
 * set: inv[a] >= 0), so each axis' entry plane is known at compile time.  The boxes are
 * widened by one quantisation step on both sides, far more than the transform's rounding, so
 * the test is conservative (KAT: RTX_KAT_BOX_Q). */
template <int OCT> __device__ __forceinline__ bool box_hit_q(uint4 n, f3 oi, f3 inv, float tlim, float &tn_out);
template <int OCT> __device__ __forceinline__ bool box_hit_q(uint4 n, f3 oi, f3 inv, float tlim)
{
	float tn;
	return box_hit_q<OCT>(n, oi, inv, tlim, tn);
}
template <int OCT> __device__ __forceinline__ bool box_hit_q(uint4 n, f3 oi, f3 inv, float tlim, float &tn_out)
{
	const float tx0 = fmaf((float)(n.x & 0xFFFFu), inv.x, -oi.x), tx1 = fmaf((float)(n.x >> 16), inv.x, -oi.x);
	const float ty0 = fmaf((float)(n.y & 0xFFFFu), inv.y, -oi.y), ty1 = fmaf((float)(n.y >> 16), inv.y, -oi.y);
	const float tz0 = fmaf((float)(n.z & 0xFFFFu), inv.z, -oi.z), tz1 = fmaf((float)(n.z >> 16), inv.z, -oi.z);
	if (OCT == 8) {
		const float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.f));
		const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tlim));
		tn_out = tn;
		return tn <= tf;
	}
	const float nx = (OCT & 1) ? tx0 : tx1, fx = (OCT & 1) ? tx1 : tx0;
	const float ny = (OCT & 2) ? ty0 : ty1, fy = (OCT & 2) ? ty1 : ty0;
	const float nz = (OCT & 4) ? tz0 : tz1, fz = (OCT & 4) ? tz1 : tz0;
	const float tn = fmaxf(fmaxf(nx, ny), fmaxf(nz, 0.f));
	/* min with the segment end in asm: tlim is loop-carried and the compiler would
	 * canonicalise it before every fminf; no NaN reaches here */
	float tf = fminf(fminf(fx, fy), fz);
	asm("v_min_f32 %0, %0, %1" : "+v"(tf) : "v"(tlim));
	tn_out = tn;
	return tn <= tf;
}

/* moller_trumbore (object.c:422-441) as a branch-free any-hit test on (eps, tlim), with the
 * same accept set for finite inputs:
 *   reject |a| < eps;  reject u < 0, v < 0, u + v > 1 (u > 1 is implied);  accept eps < t < tlim.
 * Whenever t is finite, f = 1/a and u, v are finite too, so the three sign conditions fold into
 * one max3 compare and the t window into one min compare (a NaN or infinite t fails it).
 * Products are fused and 1/a comes from v_rcp_f32 (1 ulp): only hit/miss decisions at exact
 * edges can differ from the IEEE test (KAT: RTX_KAT_ANY_TRI). */
__device__ __forceinline__ f3 cross3_fma(f3 a, f3 b)
{
	return mk3(fmaf(a.y, b.z, -a.z * b.y), fmaf(a.z, b.x, -a.x * b.z), fmaf(a.x, b.y, -a.y * b.x));
}
__device__ __forceinline__ float dot3_fma(f3 a, f3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }

__device__ __forceinline__ bool any_tri(f3 v0, f3 e1, f3 e2, f3 o, f3 d, float eps, float tlim)
{
	const f3 h = cross3_fma(d, e2);
	const float a = dot3_fma(e1, h);
	const float f = __builtin_amdgcn_rcpf(a);
	const f3 s = sub3(o, v0);
	const float u = f * dot3_fma(s, h);
	const f3 q = cross3_fma(s, e1);
	const float v = f * dot3_fma(d, q);
	const float t = f * dot3_fma(e2, q);
	const float out = fmaxf(fmaxf(-u, -v), (u + v) - 1.f); /* > 0: outside the triangle */
	return ((int)(fabsf(a) >= eps) & (int)(out <= 0.f) & (int)(fminf(t - eps, tlim - t) > 0.f)) != 0;
}

/* ------------------------------------------------------------------------ */
/* one shadow ray per lane                                                  */
/* ------------------------------------------------------------------------ */
struct ShadowCount {
	u64 boxes;     /* box tests (records stepped through), summed over lanes */
	u64 gboxes;    /* ... of which from the DQNode array (not the LDS top) */
	u64 tris, sph; /* primitive tests */
	u64 pln;       /* plane tests */
	u64 steps;     /* walk-loop iterations of the waves (a wave runs until its longest ray ends) */
	u64 walks;     /* wave walks (64 rays each) */
	u64 lrounds;   /* 8-wide walk: wave iterations of the leaf loops (immediate and deferred) */
	u64 unif;      /* 8-wide walk: wave steps with one node for all walking lanes (scalar path) */
	u64 far;       /* rays from far shade points, walked from the light end (RTX_SP_FAR) */
	u64 spills;    /* 8-wide walk: lane-stack pushes beyond the LDS entries (to DScene.w8spill in HBM) */
	u64 clear;     /* rays of packets the cone cull let skip the walk (point_masks) */
	u64 pskip;     /* plane tests the point's plane mask let skip (point_masks) */
	u64 lskip;     /* listed-object tests its listed-object mask let skip */
	u64 pclear;    /* rays of all-clear points (clear_run) */
	u64 dark;      /* rays answered without a query: their sample adds nothing to the point (sample_dark) */
	u64 dpack;     /* ... of which in packets whose every sample was dark (no shadow query at all) */
	u64 ordpt;     /* runs of one emitter's samples of a point walked in key order (order_begin) */
	u64 ordray;    /* ... the rays walked in them */
};

/* one primitive record (a, b, c = its first 48 bytes) against this lane's shadow ray
 * (accel.c:362-373): the target emitter skipped; transparent hit -> li *= kt; opaque hit ->
 * true (blocked) */
template <bool COUNT>
__device__ __forceinline__ bool shadow_prim(float4 a, float4 b, float4 c, const DMaterial *__restrict__ mats, f3 o, f3 d,
					    float tl, uint32_t emit_obj, f3 &li, uint32_t &ntri, uint32_t &nsph)
{
	const uint32_t meta = __float_as_uint(c.w), obj = __float_as_uint(b.w);
	if (obj == emit_obj)
		return false;
	bool h;
	if ((meta >> 24) == RTX_SPHERE) {
		if (COUNT)
			nsph++;
		float t = 0.f;
		h = hit_sphere(mk3(a.x, a.y, a.z), b.x, o, d, a.w, t) && t < tl;
	} else {
		if (COUNT)
			ntri++;
		h = any_tri(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), o, d, a.w, tl);
	}
	if (!h)
		return false;
	if (meta & RTX_META_TRANSPARENT) {
		const auto *m = gptr(mats) + (meta & RTX_META_MAT);
		li = mul3v(li, mk3(m->kt[0], m->kt[1], m->kt[2]));
		return false;
	}
	return true;
}

/* every primitive of the leaf with ref L, in order, its records REC bytes apart from p (64-byte
 * DPrims for the BVH2 walk, 48-byte triangle records for the wide walk); true at the first
 * opaque hit */
template <bool COUNT, uint32_t REC>
__device__ __forceinline__ bool shadow_leaf(uint32_t L, const char *__restrict__ p, const DMaterial *__restrict__ mats, f3 o,
					    f3 d, float tl, uint32_t emit_obj, f3 &li, uint32_t &ntri, uint32_t &nsph)
{
	const uint32_t cnt = (L & RTX_REF_CNT) + 1;
	for (uint32_t k = 0; k < cnt; k++) {
		const char *pr = p + k * REC;
		if (shadow_prim<COUNT>(ldg4(pr, 0), ldg4(pr, 16), ldg4(pr, 32), mats, o, d, tl, emit_obj, li, ntri, nsph))
			return true;
	}
	return false;
}

/* the trees of the shadow walks and their 16-bit frame (rtx_device.h DQNode, DW8) */
struct QBvh {
	const DQNode *q;
	f3 qo, qs, qsi; /* qsi = 1 / qs (IEEE, per component) */
	const uint4 *top;     /* the workgroup's LDS copy of the top records */
	const uint32_t *tend; /* ... and of the cut records' range ends */
	uint32_t nt;          /* top records */
	const DW8 *w8;        /* the 8-wide BVH (rtx_device.h DW8), WALK_W8 */
	const DW8S *w8s;      /* ... its nodes' scalar-path copies */
	const uint4 *t8;      /* the workgroup's LDS copy of its entries [0, nt8) (top levels) */
	uint32_t nt8;
	uint32_t *spill;      /* the lane-stack entries from lstk on, [entry][grid lane] (w8_spill_at) */
	uint32_t wv;          /* this wave's index in its workgroup */
	uint32_t lstk;        /* lane-stack entries in LDS (<= RTX_W8_STACK) */
	lds_u32 *stk;         /* the wave's LDS stacks of sibling groups: lane l's entry k at stk[k * WAVE + l]
	                       * (LA false: this lane's, entry k at stk[k * WAVE]) */
	lds_u32 *tq;          /* WALK_W8: the LDS queues of deferred leaf groups, likewise */
	bool sph;             /* WALK_W8: the tree holds spheres (DScene.w8sph) */
};

/* the shadow walks k_shadow instantiates */
enum { WALK_BVH2 = 0, WALK_W8 = 2 }; /* the RTX_WALK_* values */

/* is_light_blocked's BVH part (accel.c:360-387) for this lane's ray.  The walk starts in the
 * workgroup's LDS copy of the tree's top levels: a cut record whose box is hit hands the lane
 * to the DQNode array for the index range of its children's subtrees, and the lane returns to
 * the top copy at the next top record when the range ends.  tl < 0 on entry: inactive lane.
 * On an opaque hit tl becomes -1. */
template <bool COUNT, int OCT>
__device__ __forceinline__ void shadow_walk(const QBvh &Q, const char *__restrict__ recs, const DMaterial *__restrict__ mats,
					    f3 o, f3 d, f3 ob, f3 inv, float &tl, uint32_t emit_obj, f3 &li, ShadowCount &sc)
{
	const f3 invq = mk3(inv.x * Q.qsi.x, inv.y * Q.qsi.y, inv.z * Q.qsi.z);
	const f3 oq = mk3((ob.x - Q.qo.x) * Q.qs.x, (ob.y - Q.qo.y) * Q.qs.y, (ob.z - Q.qo.z) * Q.qs.z);
	const f3 oi = mul3v(oq, invq);
	const uint32_t nt = Q.nt;
	uint32_t t = tl >= 0.f ? 0u : nt, g = 0, ge = 0;
	uint32_t nbox = 0, nglob = 0, ntri = 0, nsph = 0, nstep = 0;
	while (t < nt || g < ge) {
		const bool ing = g < ge;
		uint4 nd;
		if (ing)
			nd = ldg4u(Q.q + g);
		else
			nd = lds4u(Q.top + t);
		if (COUNT) {
			nbox++;
			nglob += ing ? 1u : 0u;
		}
		const bool hit = box_hit_q<OCT>(nd, oi, invq, tl);
		const uint32_t L = nd.w;
		if (L & RTX_REF_LEAF) {
			if (ing)
				g++;
			else
				t++;
			if (hit && shadow_leaf<COUNT, sizeof(DPrim)>(L, recs + (L & RTX_REF_OFF), mats, o, d, tl, emit_obj, li, ntri, nsph)) {
				tl = -1.f;
				t = nt;
				ge = 0;
			}
		} else if (ing) {
			g = hit ? g + 1 : L >> 6;
		} else if (L & RTX_QTOP_CUT) {
			if (hit) {
				g = L >> 6;
				ge = lds1u(Q.tend + t);
			}
			t++;
		} else {
			t = hit ? t + 1 : L >> 6;
		}
	}
	if (COUNT)
		nstep = nbox;
	if (COUNT) {
		uint32_t a = nbox, b = ntri, c = nsph, gq = nglob;
#pragma unroll
		for (int s = 32; s > 0; s >>= 1) {
			a += __shfl_xor(a, s, WAVE);
			b += __shfl_xor(b, s, WAVE);
			c += __shfl_xor(c, s, WAVE);
			gq += __shfl_xor(gq, s, WAVE);
			nstep = max(nstep, (uint32_t)__shfl_xor(nstep, s, WAVE));
		}
		sc.boxes += uni(a);
		sc.gboxes += uni(gq);
		sc.tris += uni(b);
		sc.sph += uni(c);
		sc.steps += uni(nstep);
		sc.walks++;
	}
}

/* is_light_blocked's BVH part (accel.c:360-387) over the 8-wide BVH (rtx_device.h DW8): one
 * 64-byte node per step (four 16-byte loads, or its DW8S copy through scalar loads when every live lane is at
 * the node), eight box tests.  Hit children are taken in the octant's visit order (slot p ^ K):
 *  - opaque leaf slots are tested at once (an opaque hit ends the ray);
 *  - transparent leaf slots (tmask) can only multiply the transmittance, so their tests are
 *    deferred: the lane keeps them as leaf groups (base << 8 | mask) in a register and an LDS
 *    queue of RTX_W8_TQ, and the wave runs a round of deferred tests only when at least
 *    RTX_W8_DEFER lanes hold some (or a queue is full, or no lane has node work left), so a
 *    round tests many lanes' primitives instead of a few;
 *  - the first hit inner child is visited next and the rest are kept as one group in a
 *    register, the older groups in the lane's LDS stack (entries from Q.lstk on in HBM,
 *    Q.spill), at most one per level, so any depth walks.
 * tl < 0 on entry: inactive lane.  On an opaque hit tl becomes -1. */
/* LA (the lane-slot kernels): the lane-stack / queue LDS addresses are formed from lane_id() at each access,
 * so no per-lane address register lives across the walk (the allocator spilled it to scratch there);
 * else Q.stk / Q.tq are this lane's own */
#define W8_LN (LA ? lane_id() : 0u)

/* a deferred leaf test: the transparent primitive at entry pr (rtx_device.h DW8 leaf entry,
 * whose 4th float4 holds its material's kt) against this lane's shadow ray; a hit multiplies
 * the transmittance (accel.c:370-377) */
template <bool COUNT, bool SPH>
__device__ __forceinline__ void w8_defer_test(const char *pr, f3 o, f3 d, float tl, f3 &li, uint32_t &ntri, uint32_t &nsph)
{
	const float4 a = ldg4(pr, 0), b = ldg4(pr, 16), c = ldg4(pr, 32);
	bool h;
	if (SPH && (__float_as_uint(c.w) >> 24) == RTX_SPHERE) {
		if (COUNT)
			nsph++;
		float t = 0.f;
		h = hit_sphere(mk3(a.x, a.y, a.z), b.x, o, d, a.w, t) && t < tl;
	} else {
		if (COUNT)
			ntri++;
		h = any_tri(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), o, d, a.w, tl);
	}
	if (h) {
		const float4 kt = ldg4(pr, 48);
		li = mul3v(li, mk3(kt.x, kt.y, kt.z));
	}
}

/* an opaque leaf test: does the primitive at entry pr block this lane's shadow ray?  (no
 * emitter or transparency cases: the 8-wide tree marks its leaves when built from host records).
 * SPH false: the tree holds no spheres (DScene.w8sph), the test is the triangle's alone */
template <bool COUNT, bool SPH>
__device__ __forceinline__ bool w8_opaque_test(const char *pr, f3 o, f3 d, float tl, uint32_t &ntri, uint32_t &nsph)
{
	const float4 a = ldg4(pr, 0), b = ldg4(pr, 16), c = ldg4(pr, 32);
	if (SPH && (__float_as_uint(c.w) >> 24) == RTX_SPHERE) {
		if (COUNT)
			nsph++;
		float t = 0.f;
		return hit_sphere(mk3(a.x, a.y, a.z), b.x, o, d, a.w, t) && t < tl;
	}
	if (COUNT)
		ntri++;
	return any_tri(mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), o, d, a.w, tl);
}

/* lane-stack entry k (>= Q.lstk) of this lane in HBM, [entry][grid lane]: its address formed where
 * it is used, from the launch's constant block size, the workgroup's and wave's indices and
 * lane_id() (volatile asm, so nothing of it is hoisted into the packet's set-up: round 5's
 * per-lane spill pointer and round 6's first stride / lane-offset pair were computed per packet
 * and spilled to scratch there, one 12-byte scratch store per lane and packet) */
__device__ __forceinline__ uint32_t *w8_spill_at(const QBvh &Q, uint32_t k)
{
	constexpr uint32_t B = WAVE * RTX_SH_NW; /* k_shadow's block size (rtx_launch_shadow) */
	return Q.spill + ((size_t)(k - Q.lstk) * ((size_t)gridDim.x * B) + (size_t)blockIdx.x * B + Q.wv * WAVE + lane_id());
}

/* the visit order of hit children (slot p ^ W8_SORDER): plain slot order.  Fixed: front to back from the
 * shade point or from the light measured no faster (scene5 567.3 against 577.2 / 575.5 ms) */
constexpr uint32_t W8_SORDER = 0u;

/* one lane's 8-wide any-hit walk: the node it is at (RTX_NONE: no node work), the kept sibling
 * group and the stack depth below it, the deferred transparent-leaf group and the queue depth */
struct W8Walk {
	uint32_t node, grp, sp, tgrp, tn;
};
/* the walk's counters (COUNT instances) */
struct W8Ctr {
	uint32_t nbox, ntri, nsph, nstep, nlr, nun, nspill;
};

/* this lane's opaque leaf hits lm (visit order) in the block at base, tested in turn: does one
 * block the ray?  (the wave's lanes in step, a lane leaving at its first blocking hit).  A round takes
 * two of the lane's hit leaves (the same tests in the same order, half the rounds: a Menger face's two
 * triangles share a box in the rotated frame, so a lane that meets one meets both) */
template <bool COUNT, bool SPH, uint32_t K>
__device__ __forceinline__ bool w8_opaque_leaves(const DW8 *w8, uint32_t lm, uint32_t base, f3 o, f3 d, float tl, W8Ctr &c)
{
	while (lm) {
		const uint32_t p = __builtin_ctz(lm);
		lm &= lm - 1;
		const bool two = lm != 0;
		const uint32_t q = two ? __builtin_ctz(lm) : p;
		lm &= lm - 1;
		if (w8_opaque_test<COUNT, SPH>((const char *)(w8 + base + (p ^ K)), o, d, tl, c.ntri, c.nsph))
			return true;
		if (two && w8_opaque_test<COUNT, SPH>((const char *)(w8 + base + (q ^ K)), o, d, tl, c.ntri, c.nsph))
			return true;
	}
	return false;
}

/* One iteration of the 8-wide any-hit walk for the wave: a round of deferred transparent-leaf
 * tests, or one node step with its opaque leaf tests (see shadow_walk8).  wk / hd: this lane has
 * node work / deferred tests; walking / holding: their ballots (at least one lane has one).  o / d: the
 * world ray; invq / oi: its inverse direction and origin term in the tree's 16-bit frame. */
template <bool COUNT, int OCT, bool LA>
__device__ __forceinline__ void w8_iter(const QBvh &Q, f3 o, f3 d, f3 invq, f3 oi, float &tl, f3 &li, W8Walk &w, W8Ctr &c,
					bool wk, bool hd, u64 walking, u64 holding)
{
	constexpr uint32_t K = W8_SORDER;
	lds_u32 *stk = Q.stk, *tq = Q.tq;
	if (!walking || popc64(holding) >= RTX_W8_DEFER || ballot(w.tn == RTX_W8_TQ)) {
		/* a round of deferred transparent-leaf tests */
		if (COUNT)
			c.nlr++;
		if (hd) {
			const char *pr = (const char *)(Q.w8 + (w.tgrp >> 8) + (__builtin_ctz(w.tgrp) ^ K));
			w.tgrp &= w.tgrp - 1;
			if (!(w.tgrp & 0xFFu))
				w.tgrp = w.tn ? tq[--w.tn * WAVE + W8_LN] : 0u;
			/* the lane's next queued leaf in the same round (the transmittance products in the same
			 * order) */
			const char *pr2 = nullptr;
			if (w.tgrp) {
				pr2 = (const char *)(Q.w8 + (w.tgrp >> 8) + (__builtin_ctz(w.tgrp) ^ K));
				w.tgrp &= w.tgrp - 1;
				if (!(w.tgrp & 0xFFu))
					w.tgrp = w.tn ? tq[--w.tn * WAVE + W8_LN] : 0u;
			}
			/* not counted here: a deferred test counts where its leaf is queued (below) */
			uint32_t n0 = 0, n1 = 0;
			if (Q.sph) {
				w8_defer_test<false, true>(pr, o, d, tl, li, n0, n1);
				if (pr2)
					w8_defer_test<false, true>(pr2, o, d, tl, li, n0, n1);
			} else { /* a tree without spheres: the triangle test alone */
				w8_defer_test<false, false>(pr, o, d, tl, li, n0, n1);
				if (pr2)
					w8_defer_test<false, false>(pr2, o, d, tl, li, n0, n1);
			}
		}
		return;
	}
	uint32_t lm = 0, base = 0; /* this step's opaque leaf hits (visit order) and their block */
	if (wk) {
		const uint32_t un = uni(w.node);
		W8Visit v;
		if (!ballot(w.node != un)) {
			/* every walking lane is at one node: its scalar-path copy through the scalar cache,
			 * the planes as SGPR float operands (no vector-memory address / data cycles) */
			v = w8_visit_s<OCT, K>(Q.w8s + (size_t)un, invq, oi, tl);
		} else {
			uint32_t wd[16];
			if (w.node < Q.nt8) { /* a top-level node: the workgroup's LDS copy (no texture-path traffic) */
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const uint4 x = lds4u(Q.t8 + 4 * w.node + k);
					wd[4 * k] = x.x;
					wd[4 * k + 1] = x.y;
					wd[4 * k + 2] = x.z;
					wd[4 * k + 3] = x.w;
				}
			} else {
				const DW8 *N = Q.w8 + (size_t)w.node;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const uint4 x = ldg4u((const uint32_t *)N + 4 * k);
					wd[4 * k] = x.x;
					wd[4 * k + 1] = x.y;
					wd[4 * k + 2] = x.z;
					wd[4 * k + 3] = x.w;
				}
			}
			v = w8_visit<OCT, K, false>(wd, invq, oi, tl);
		}
		const uint32_t hm = v.hm;
		base = v.base;
		lm = RTX_DEBUG_NOLEAF ? 0u : hm & ~v.io & ~v.to;
		uint32_t im = hm & v.io;
		const uint32_t dm = RTX_DEBUG_NOLEAF ? 0u : hm & v.to;
		if (COUNT) {
			c.nstep++;
			c.nbox += popc64(v.nv);
			c.nun += ballot(w.node != uni(w.node)) ? 0u : 1u;
		}
		if (COUNT) {
			/* the transparent leaves' tests count here, where the ray's own walk calls for them (as a
			 * ray walking alone tests them, in visit order, before a later opaque hit ends it): per-ray
			 * work.  Counted where they run, the figure would follow the deferred rounds, which the
			 * wave's lanes start together: a ray an opaque leaf blocks drops its queue, and how much of
			 * it was tested by then depends on the rays that share its packet */
			for (uint32_t m = dm; m; m &= m - 1) {
				const char *pr = (const char *)(Q.w8 + base + (__builtin_ctz(m) ^ K));
				if (Q.sph && (__float_as_uint(ldg4(pr, 32).w) >> 24) == RTX_SPHERE)
					c.nsph++;
				else
					c.ntri++;
			}
		}
		if (dm) { /* transparent leaves: deferred */
			const uint32_t g = (base << 8) | dm;
			if (w.tgrp)
				tq[w.tn++ * WAVE + W8_LN] = g;
			else
				w.tgrp = g;
		}
		/* the next node (a lane the opaque leaves below block drops it again) */
		if (im) {
			w.node = base + (__builtin_ctz(im) ^ K);
			im &= im - 1;
			if (im) {
				if (w.grp) {
					if (w.sp < Q.lstk)
						stk[w.sp * WAVE + W8_LN] = w.grp;
					else {
						*gptrw(w8_spill_at(Q, w.sp)) = w.grp;
						if (COUNT)
							c.nspill++;
					}
					w.sp++;
				}
				w.grp = (base << 8) | im;
			}
		} else if (w.grp) {
			w.node = (w.grp >> 8) + (__builtin_ctz(w.grp) ^ K);
			w.grp &= w.grp - 1;
			if (!(w.grp & 0xFFu)) {
				w.grp = 0;
				if (w.sp) {
					w.sp--;
					w.grp = w.sp < Q.lstk ? stk[w.sp * WAVE + W8_LN]
							      : *gptr(w8_spill_at(Q, w.sp));
				}
			}
		} else {
			w.node = RTX_NONE;
		}
	}
	/* opaque leaves, at once (an opaque hit ends the ray): the tree marks every leaf slot (built
	 * from the primitive records, emitters left out), each lane tests its own.  (Dealing the
	 * wave's tests over its lanes with ds_permute, one round for all, measured slower on scene6:
	 * 2834 vs 2806 ms, every dealt job tested without the early break) */
	if (!ballot(lm != 0))
		return;
	if (COUNT) {
		uint32_t r = 0;
		for (uint32_t m = lm;; m &= m - 1) {
			if (!ballot(m != 0))
				break;
			m &= m - 1; /* two leaves a round (w8_opaque_leaves) */
			r++;
		}
		c.nlr += r;
	}
	const bool blocked = Q.sph ? w8_opaque_leaves<COUNT, true, K>(Q.w8, lm, base, o, d, tl, c)
				   : w8_opaque_leaves<COUNT, false, K>(Q.w8, lm, base, o, d, tl, c);
	if (blocked) { /* the queue too: a full queue left behind would keep the wave in deferred rounds */
		tl = -1.f;
		w.node = RTX_NONE;
		w.tgrp = 0;
		w.tn = 0;
	}
}

/* the walk's counters summed over the wave into sc (walks: wave walks of 64 lane slots) */
template <bool COUNT> __device__ __forceinline__ void w8_count(W8Ctr c, ShadowCount &sc, uint32_t walks)
{
	if (!COUNT)
		return;
	uint32_t a = c.nbox, bb = c.ntri, cc = c.nsph, nstep = c.nstep, nun = c.nun, nlr = c.nlr, nsp = c.nspill;
#pragma unroll
	for (int k = 32; k > 0; k >>= 1) {
		a += __shfl_xor(a, k, WAVE);
		nsp += __shfl_xor(nsp, k, WAVE);
		bb += __shfl_xor(bb, k, WAVE);
		cc += __shfl_xor(cc, k, WAVE);
		nstep = max(nstep, (uint32_t)__shfl_xor(nstep, k, WAVE));
		nun = max(nun, (uint32_t)__shfl_xor(nun, k, WAVE));
		nlr = max(nlr, (uint32_t)__shfl_xor(nlr, k, WAVE));
	}
	sc.boxes += uni(a);
	sc.gboxes += uni(a);
	sc.lrounds += uni(nlr);
	sc.unif += uni(nun);
	sc.spills += uni(nsp);
	sc.tris += uni(bb);
	sc.sph += uni(cc);
	sc.steps += uni(nstep);
	sc.walks += walks;
}

template <bool COUNT, int OCT, bool LA>
__device__ __forceinline__ void shadow_walk8(const QBvh &Q, const DMaterial *__restrict__ mats, f3 o, f3 d, f3 ob, f3 inv,
					     float &tl, uint32_t emit_obj, f3 &li, ShadowCount &sc)
{
	/* the ray in the tree's 16-bit frame: ob / inv are its origin and inverse direction in the
	 * tree's rotated frame (shadow_query), o / d the world ray the primitives are tested with */
	const f3 invq = mk3(inv.x * Q.qsi.x, inv.y * Q.qsi.y, inv.z * Q.qsi.z);
	const f3 oq = mk3((ob.x - Q.qo.x) * Q.qs.x, (ob.y - Q.qo.y) * Q.qs.y, (ob.z - Q.qo.z) * Q.qs.z);
	const f3 oi = mul3v(oq, invq);
	W8Walk w = { tl >= 0.f ? 0u : RTX_NONE, 0u, 0u, 0u, 0u };
	W8Ctr c = { 0u, 0u, 0u, 0u, 0u, 0u, 0u };
	for (;;) {
		/* the lane's two conditions once, as lane masks the branches below reuse */
		const bool wk = w.node != RTX_NONE, hd = w.tgrp != 0;
		const u64 walking = ballot(wk);
		const u64 holding = ballot(hd);
		if (!(walking | holding))
			break;
		w8_iter<COUNT, OCT, LA>(Q, o, d, invq, oi, tl, li, w, c, wk, hd, walking, holding);
	}
	w8_count<COUNT>(c, sc, 1u);
}

/* is_light_blocked (render.c:126-134): planes first (unbound_objects_is_light_blocked,
 * object.c:183-197), then the BVH walk, specialised on the direction octant when every live
 * lane shares it.  Returns the lane's blocked flag; li carries the transmittance product. */
/* hit_plane(...) && t < dist (object.c:473-488 and is_light_blocked's plane test) with the
 * quotient t = num / a as num * v_rcp_f32(a) (within 2 ulp of the IEEE quotient, like the
 * light points of RTX_SH_FASTTRIG): the decisions differ from the IEEE test only for a t within
 * 2 ulp of the plane's epsilon or of the light sample's distance */
__device__ __forceinline__ bool plane_blocks(f3 n, float dd, f3 o, f3 d, float eps, float dist)
{
	float t;
	if (!RTX_SH_PLANE_RCP)
		return hit_plane(n, dd, o, d, eps, t) && t < dist;
	const float a = dot3(n, d);
	if (!(fabsf(a) >= eps)) /* hit_plane's fabsf(a) < eps (a NaN misses there too) */
		return false;
	t = (dd - dot3(n, o)) * __builtin_amdgcn_rcpf(a);
	return t > eps && t < dist;
}

template <bool COUNT, int WALK, bool LA>
__device__ __forceinline__ bool shadow_query(const QBvh &Q, const char *__restrict__ recs, const DMaterial *__restrict__ mats,
					     const DPlane *__restrict__ planes, uint32_t num_planes, const DEmitter *__restrict__ lin,
					     uint32_t num_lin, bool have_tree, const DTreeFrame &tf, bool act, bool far, f3 o, f3 d,
					     float dist, uint32_t emit_obj, f3 &li, ShadowCount &sc)
{
	float tl = act ? dist : -1.f;
	for (uint32_t i = 0; i < num_planes; i++) { /* plane records are wave-uniform: s_load */
		const auto *pl = cptr(planes) + i;
		const bool h = plane_blocks(mk3(pl->n[0], pl->n[1], pl->n[2]), pl->d, o, d, pl->eps, dist) && tl >= 0.f;
		if (pl->transparent) {
			if (h)
				li = mul3v(li, mk3(pl->kt[0], pl->kt[1], pl->kt[2]));
		} else if (h) {
			tl = -1.f;
		}
	}
	/* objects tested one by one like the planes, records wave-uniform (s_load): the emitters other
	 * than the one sampled when the 8-wide tree leaves them out (rtx_device.h DW8), or every bounded
	 * object of a tiny scene (DScene.lin), in object order */
	for (uint32_t i = 0; i < num_lin; i++) {
		const auto *e = cptr(lin) + i;
		if (e->obj == emit_obj || !(tl >= 0.f))
			continue;
		/* a far shade point: the object's world box first, from the light end like the walk */
		if (RTX_SH_FARLIN == 1 && far &&
		    !world_box_at(e->wlo[0], e->whi[0], e->wlo[1], e->whi[1], e->wlo[2], e->whi[2], o, d, dist, -1.f, dist))
			continue;
		bool h;
		if (e->type == RTX_SPHERE) {
			float t = 0.f;
			h = (RTX_SH_FARLIN != 2 || !far ||
			     world_box_at(e->wlo[0], e->whi[0], e->wlo[1], e->whi[1], e->wlo[2], e->whi[2], o, d, 0.f, 1.f, dist)) &&
			    hit_sphere(mk3(e->p0[0], e->p0[1], e->p0[2]), e->radius, o, d, e->eps, t) && t < tl;
		} else {
			h = any_tri(mk3(e->p0[0], e->p0[1], e->p0[2]), mk3(e->e1[0], e->e1[1], e->e1[2]),
				    mk3(e->e2[0], e->e2[1], e->e2[2]), o, d, e->eps, tl);
		}
		if (h) {
			if (e->transparent)
				li = mul3v(li, mk3(e->kt[0], e->kt[1], e->kt[2]));
			else
				tl = -1.f;
		}
	}
	if (COUNT)
		sc.pln += (u64)popc64(ballot(act)) * num_planes;
	const bool alive = tl >= 0.f;
	const u64 live = ballot(alive);
	if (!live || !have_tree)
		return act && !alive;
	/* the ray in the trees' frame (rtx_device.h DTreeFrame): origin ob, direction db.  A shade point
	 * far from the bounded objects (a plane point far out, rtx_math.h tf_far; k_trace marks its
	 * record RTX_SP_FAR): the walk runs the segment from its other end, the light point, x' formed
	 * in double there; the same boxes meet the segment [0, dist] from either end, and the
	 * primitives are still tested from o along d.  In every frame: the world trees' slab test
	 * rounds at 2^-24 |o| too. */
	f3 ob = o, db = d;
	if (uni(tf.rotated)) {
		float r[3][3], c[3];
#pragma unroll
		for (int i = 0; i < 3; i++) {
			c[i] = __uint_as_float(uni(__float_as_uint(tf.c[i])));
#pragma unroll
			for (int j = 0; j < 3; j++)
				r[i][j] = __uint_as_float(uni(__float_as_uint(tf.r[i][j])));
		}
		ob = tf_point(r, c, o);
		db = tf_dir(r, d);
		if (far) {
			ob = tf_point_at(r, c, o, d, dist);
			db = mk3(-db.x, -db.y, -db.z);
		}
	} else if (far) {
		ob = tf_world_at(o, d, dist);
		db = mk3(-d.x, -d.y, -d.z);
	}
	if (COUNT)
		sc.far += (u64)popc64(ballot(alive && far));
	const f3 inv = safe_inv_fast(db); /* boxes are padded 2e-6 relative: a 1-ulp 1/d keeps the test conservative */
	const uint32_t oct = ((~__float_as_uint(inv.x)) >> 31) | (((~__float_as_uint(inv.y)) >> 31) << 1) |
			     (((~__float_as_uint(inv.z)) >> 31) << 2);
	const uint32_t lead = readlane(oct, (uint32_t)__ffsll((long long)live) - 1);
	const uint32_t sel = ballot(alive & (oct != lead)) ? 8u : lead;
	switch (sel) {
#define RTX_WALK(K)                                                                            \
	case K:                                                                                \
		if (WALK == WALK_W8)                                                           \
			shadow_walk8<COUNT, K, LA>(Q, mats, o, d, ob, inv, tl, emit_obj, li, sc); \
		else                                                                           \
			shadow_walk<COUNT, K>(Q, recs, mats, o, d, ob, inv, tl, emit_obj, li, sc); \
		break;
		RTX_WALK(0) RTX_WALK(1) RTX_WALK(2) RTX_WALK(3) RTX_WALK(4) RTX_WALK(5) RTX_WALK(6) RTX_WALK(7)
#undef RTX_WALK
	default:
		if (WALK == WALK_W8)
			shadow_walk8<COUNT, 8, LA>(Q, mats, o, d, ob, inv, tl, emit_obj, li, sc);
		else
			shadow_walk<COUNT, 8>(Q, recs, mats, o, d, ob, inv, tl, emit_obj, li, sc);
		break;
	}
	return act && tl < 0.f;
}

/* ------------------------------------------------------------------------ */
/* light sampling and shading                                               */
/* ------------------------------------------------------------------------ */
/* k_shadow arguments.  Lane 0 copies them to LDS; the loops re-read them from there behind a
 * compiler memory barrier, so none stays live in registers across the walk. */
struct KShadow {
	uint32_t *ord;        /* RTX_OPT_SHADOW_ORDER: the waves' order / result slices (DScene.ordbuf), RTX_ORD_WORDS
	                       * words per grid wave; null: off, or the launch is not one it applies to */
	const char *recs;     /* base of the record array the leaf refs point into */	const DQNode *qnodes; /* threaded quantised BVH */
const DW8 *w8;        /* 8-wide compressed BVH (WALK_W8 instances; qo / qs / qsi are then its frame) */
	const DW8S *w8s;      /* its nodes' scalar-path copies */
	uint32_t *w8spill;    /* lane-stack spill area, [entry][grid lane] */
	uint32_t w8lstk;      /* lane-stack entries in LDS */
	uint32_t w8top;       /* entries of the 8-wide tree's top levels, copied to LDS per workgroup (DScene.w8top) */
	uint32_t w8sph;       /* the 8-wide tree holds spheres (DScene.w8sph) */
	uint32_t dark;        /* RTX_OPT_SHADOW_DARK (and the scene allows it, DScene.dark_ok): dark samples skip their query */
	const DEmitter *lin;  /* objects shadow_query tests one by one: the emitters the 8-wide tree leaves out,
	                       * or every bounded object of a tiny scene (no tree walk) */
	uint32_t num_lin;
	float qo[3], qs[3], qsi[3];
	DTreeFrame tf;        /* the trees' frame (their boxes are in it) */
	const uint32_t *top; /* its top levels (rtx_device.h RTX_QTOP_CUT), copied to LDS per workgroup */
	uint32_t ntop;
	const DMaterial *mats;
	const DPlane *planes;
	const DEmitter *emitters;
	const float4 *sp;
	const uint32_t *perm; /* shade points in processing (Morton) order, or null */
	float4 *contrib;
	unsigned long long *ctr;
	uint32_t have_tree, num_planes, num_emitters;
	uint32_t n_sp, per_wave, slot_b, slot_lg;
	int32_t rng, attenuation, reflection;
	float att_offset;
	const float4 *cull;   /* DScene.cull: the 8-wide tree's second-level bounding spheres (point_masks) */
	uint32_t num_cull;    /* 0: no cull (RTX_OPT_SHADOW_CULL off, or no such tree) */
	uint32_t cull_slots;  /* the lane-slot path culls too (RTX_OPT_SHADOW_CULL 2) */
	const float4 *lsph;   /* DScene.lsph: the bounding spheres of the `lin` records (point_masks) */
	uint32_t num_lsph;    /* num_lin when they are there, else 0 */
	uint32_t point;       /* RTX_OPT_SHADOW_POINT: planes and listed objects decided once per shade point */
	const uint32_t *pm;   /* the points' masks formed before the kernel (k_point_masks), by record index; null:
	                       * k_shadow forms them itself (point_masks) */
	uint32_t spec;        /* RTX_OPT_SHADOW_SPEC: a wave-uniform point of shininess 0 takes shade_terms_s0 / dark_terms_s0 */
};

__device__ __forceinline__ void reread_barrier() { asm volatile("" ::: "memory"); }

/* a pointer read from LDS, made wave-uniform (SGPRs) so accesses through it stay scalar */
template <typename T> __device__ __forceinline__ T *unip(T *p)
{
	const uint64_t v = (uint64_t)p;
	return (T *)(((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v));
}

__device__ __forceinline__ float sh_rcp(float x) { return RTX_SH_FASTDIV ? __builtin_amdgcn_rcpf(x) : 1.f / x; }

/* light_point (object.c:293-304, 403-419) as k_shadow evaluates it (RTX_SH_FASTTRIG) */
__device__ __forceinline__ f3 light_point_sh(const DEmitter &e, f3 p, float u1, float u2)
{
	if (RTX_SH_FASTTRIG && e.type == RTX_SPHERE) {
		const f3 c = ld3(e.p0);
		const f3 nrm = sub3(c, p);
		const float si = __builtin_amdgcn_sinf(u1), ci = __builtin_amdgcn_cosf(u1);
		const float sa = __builtin_amdgcn_sinf(u2), ca = __builtin_amdgcn_cosf(u2);
		f3 ld = mk3(e.radius * ca * si, e.radius * sa * si, e.radius * ci);
		if (dot3(nrm, ld) != 0.f)
			ld = mul3s(ld, -1.f);
		return add3(c, ld);
	}
	return light_point(e, p, u1, u2);
}

/* field k of a shade-point record: UNI (>= 64 lights, the record is wave-uniform) through
 * scalar loads, else per lane */
template <bool UNI> __device__ __forceinline__ float4 sp_field(const float4 *rec, int k)
{
	if (UNI) {
		const auto *r = (const __attribute__((address_space(4))) f4v *)rec;
		const f4v v = r[k];
		return make_float4(v.x, v.y, v.z, v.w);
	}
	return ldg4(rec, 16 * k);
}

/* powf(x, y) of the specular term (render.c:224, fmaxf(0, powf(specular_mul, shininess))).
 * RTX_SH_FASTPOW: exp2(y * log2|x|) from v_log_f32 / v_exp_f32, with powf's y = 0 -> 1 and its
 * sign rule for x < 0 (odd integer y negative, even positive, otherwise NaN, which fmaxf
 * turns into 0).  Relative error about |y log2 x| * 2^-24 (< 2e-6 for results above 1e-9). */
__device__ __forceinline__ float sh_pow(float x, float y)
{
	if (!RTX_SH_FASTPOW)
		return powf(x, y);
	if (y == 0.f)
		return 1.f;
	const float ax = fabsf(x);
	const bool den = ax < 1.17549435e-38f; /* v_log_f32 flushes denormal inputs: scale by 2^32 */
	const float lx = __builtin_amdgcn_logf(den ? ax * 4294967296.f : ax) - (den ? 32.f : 0.f);
	const float r = __builtin_amdgcn_exp2f(y * lx);
	if (!(x < 0.f))
		return r;
	if (rintf(y) != y)
		return __builtin_nanf("");
	const float h = 0.5f * y; /* exact; an integer iff y is even */
	return rintf(h) != h ? -r : r;
}

/* the attenuation factor of a light sample at distance ldist (render.c:217-222), formed before
 * the walk so one float, not ldist and dsq, lives across it (the product with the transmittance
 * after the walk is the same operation in the same order) */
__device__ __forceinline__ float sample_att_of(int32_t att, float att_offset, float ldist, float dsq)
{
	if (att == RTX_ATT_LIN)
		return sh_rcp(att_offset + ldist);
	if (att == RTX_ATT_SQR)
		return sh_rcp(att_offset + dsq);
	return 1.f;
}
__device__ __forceinline__ float sample_att(const KShadow &ks, float ldist, float dsq)
{
	return sample_att_of((int32_t)uni((uint32_t)ks.attenuation), ks.att_offset, ldist, dsq);
}

/* The two factors of a light sample's terms (render.c:202-226): pd = fmaxf(0, ldir.n) of the
 * diffuse term and pw = fmaxf(0, powf(specular_mul, shininess)) of the specular one.  shade_terms
 * and dark_terms both take them from here, so the two cannot disagree. */
__device__ __forceinline__ float shade_pd(f3 n, f3 ldir, float &a)
{
	a = dot3(ldir, n);
	return fmaxf(0.f, a);
}
__device__ __forceinline__ float shade_pw(int32_t refl, f3 n, f3 dir, float shin, f3 ldir, float a)
{
	float sm;
	if (refl == RTX_BLINN)
		sm = -dot3(n, norm3(add3(mul3s(ldir, -1.f), dir)));
	else
		sm = -dot3(sub3(mul3s(n, 2.f * a), ldir), dir);
	return fmaxf(0.f, sh_pow(sm, shin));
}

/* direct-lighting terms of one unblocked light sample (render.c:199-228) from the shade point's
 * normal n, view direction dir, diffuse colour kd and its material's ks3 / shin */
__device__ __forceinline__ f3 shade_terms(int32_t att, int32_t refl, f3 n, f3 dir, f3 kd, f3 ks3, float shin, f3 ldir, f3 li, float attf)
{
	float a;
	const float pd = shade_pd(n, ldir, a);
	if (att != RTX_ATT_NONE)
		li = mul3s(li, attf);
	const f3 diff = mul3s(mul3v(kd, li), pd);
	const f3 spec = mul3s(mul3v(ks3, li), shade_pw(refl, n, dir, shin, ldir, a));
	return add3(diff, spec);
}

/* A dark sample (RTX_OPT_SHADOW_DARK): shade_terms gives +-0 in every channel for this sample's li
 * and for li times any product of transmittances |kt| <= 1, so the sample adds nothing to its
 * point whether or not it is blocked (acc + (+-0) == acc bit for bit, what a blocked sample
 * leaves), and its shadow query need not run.  That is: a light behind the surface (pd == 0) or
 * a point without diffuse colour, and a specular factor of 0 (pw == 0: ks aside, specular_mul
 * <= 0 under an odd or non-integer shininess) or a material without ks.  The products must stay
 * finite, or a 0 factor would give NaN, not 0: kd li' and ks li' (li' = li attf) are finite
 * here, and with a transmittance T, |T| <= 1 (the scene's flag, rtx_upload.cpp scene_dark_ok),
 * |fl(fl(li T) attf)| <= |fl(li attf)| as rounding is monotonic, so the products formed after
 * a walk are no larger.  The lanes' pw is formed only when some lane passed the diffuse part
 * (a lit point's packets pay the dot product alone).  (KAT: RTX_KAT_DARK) */
__device__ __forceinline__ bool fin1(float x) { return fabsf(x) < __builtin_inff(); }
__device__ __forceinline__ bool fin3(f3 v) { return fin1(v.x) && fin1(v.y) && fin1(v.z); }
__device__ __forceinline__ bool zero3(f3 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }
__device__ __forceinline__ bool dark_terms(int32_t att, int32_t refl, f3 n, f3 dir, f3 kd, f3 ks3, float shin, f3 ldir, f3 li, float attf,
					   bool act)
{
	float a;
	const float pd = shade_pd(n, ldir, a);
	if (att != RTX_ATT_NONE)
		li = mul3s(li, attf);
	const bool fin = fin1(attf) && fin3(mul3v(kd, li)) && fin3(mul3v(ks3, li));
	const bool dk = act && fin && (pd == 0.f || (zero3(kd) && fin1(pd)));
	if (!ballot(dk))
		return false;
	const float pw = shade_pw(refl, n, dir, shin, ldir, a);
	return dk && (pw == 0.f || (zero3(ks3) && fin1(pw)));
}

/* The two for a point of shininess +-0 (RTX_OPT_SHADOW_SPEC).  sh_pow (and powf) give 1 for y == 0
 * whatever x is, NaN included, so pw = fmaxf(0, 1) = 1 and shade_pw, the reflection vector, its dot
 * product, the logarithm and the sign rule, need not run.  spec = (ks li) * 1 is ks li bit for bit
 * (a product is never a signalling NaN, and denormals are kept); pd, li attf, diff and the final sum
 * are shade_terms' operations in its order.  In dark_terms pw == 0 is false and fin1(pw) true, and
 * its early return only skips pw.  The callers branch here on the point's shininess where it is
 * wave-uniform (shin_zero of a scalar), so the lanes run none of what is left out; per-lane points
 * keep the generic forms.  (KAT: RTX_KAT_SPEC0) */
__device__ __forceinline__ bool shin_zero(float shin) { return (__float_as_uint(shin) << 1) == 0u; } /* shin == 0.f, on the bits */
__device__ __forceinline__ f3 shade_terms_s0(int32_t att, f3 n, f3 kd, f3 ks3, f3 ldir, f3 li, float attf)
{
	float a;
	const float pd = shade_pd(n, ldir, a);
	if (att != RTX_ATT_NONE)
		li = mul3s(li, attf);
	const f3 diff = mul3s(mul3v(kd, li), pd);
	const f3 spec = mul3v(ks3, li);
	return add3(diff, spec);
}
__device__ __forceinline__ bool dark_terms_s0(int32_t att, f3 n, f3 kd, f3 ks3, f3 ldir, f3 li, float attf, bool act)
{
	float a;
	const float pd = shade_pd(n, ldir, a);
	if (att != RTX_ATT_NONE)
		li = mul3s(li, attf);
	const bool fin = fin1(attf) && fin3(mul3v(kd, li)) && fin3(mul3v(ks3, li));
	const bool dk = act && fin && (pd == 0.f || (zero3(kd) && fin1(pd)));
	return dk && zero3(ks3);
}

/* the shading inputs of the shade point `rec`: normal, view direction, diffuse colour and its
 * material's ks / shininess (UNI: a wave-uniform record and its material through scalar reads) */
template <bool UNI>
__device__ __forceinline__ void point_shading(const KShadow &ks, const float4 *rec, f3 &n, f3 &dir, f3 &kd, f3 &ks3, float &shin)
{
	const float4 q1 = sp_field<UNI>(rec, 1), q2 = sp_field<UNI>(rec, 2), q3 = sp_field<UNI>(rec, 3);
	n = mk3(q1.x, q1.y, q1.z);
	dir = mk3(q2.x, q2.y, q2.z);
	kd = mk3(q3.x, q3.y, q3.z);
	if (UNI) { /* the material of a wave-uniform record: scalar reads */
		const auto &m = cptr(unip(ks.mats))[__float_as_uint(q3.w)];
		ks3 = mk3(m.ks[0], m.ks[1], m.ks[2]);
		shin = m.shininess;
	} else {
		const DMaterial &m = unip(ks.mats)[__float_as_uint(q3.w)];
		ks3 = ld3(m.ks);
		shin = m.shininess;
	}
}

/* shade_terms of the shade point `rec`, read after the walk */
template <bool UNI>
__device__ __forceinline__ f3 shade_light(const KShadow &ks, const float4 *rec, f3 ldir, f3 li, float attf)
{
	f3 n, dir, kd, ks3;
	float shin;
	point_shading<UNI>(ks, rec, n, dir, kd, ks3, shin);
	if (UNI && shin_zero(shin) && uni(ks.spec)) /* a wave-uniform branch: shin is a scalar here */
		return shade_terms_s0((int32_t)uni((uint32_t)ks.attenuation), n, kd, ks3, ldir, li, attf);
	return shade_terms((int32_t)uni((uint32_t)ks.attenuation), (int32_t)uni((uint32_t)ks.reflection), n, dir, kd, ks3, shin, ldir, li,
			   attf);
}

/* dark_terms of the shade point `rec`, read before the walk (nothing of it lives across it) */
template <bool UNI>
__device__ __forceinline__ bool sample_dark(const KShadow &ks, const float4 *rec, f3 ldir, f3 li, float attf, bool act)
{
	f3 n, dir, kd, ks3;
	float shin;
	point_shading<UNI>(ks, rec, n, dir, kd, ks3, shin);
	if (UNI && shin_zero(shin) && uni(ks.spec))
		return dark_terms_s0((int32_t)uni((uint32_t)ks.attenuation), n, kd, ks3, ldir, li, attf, act);
	return dark_terms((int32_t)uni((uint32_t)ks.attenuation), (int32_t)uni((uint32_t)ks.reflection), n, dir, kd, ks3, shin, ldir, li,
			  attf, act);
}

/* the light point of sample j of emitter E from its draws u1, u2 (object.c:293-304, 403-419:
 * stratified per the rng mode), its shadow ray's direction and length, and the sample's intensity */
__device__ __forceinline__ void sample_ray(int32_t rng, const DEmitter &E, uint32_t j, float u1, float u2, f3 p, f3 &ldir, float &ldist,
					   float &dsq, f3 &li)
{
	if (rng == RTX_RNG_STRAT) /* stratum j of the emitter's lights (IEEE, as the oracle) */
		u1 = ((float)j + u1) / (float)E.num_lights;
	const f3 lp = light_point_sh(E, p, u1, u2);
	const f3 dv = sub3(lp, p);
	dsq = magsqr3(dv);
	ldist = RTX_SH_FASTSQRT ? __builtin_amdgcn_sqrtf(dsq) : sqrtf(dsq); /* mag3(dv) */
	ldir = mul3s(dv, sh_rcp(ldist));
	li = ld3(E.li);
}

/* the same of sample j of emitter number e, E, its draws made here */
__device__ __forceinline__ void emitter_sample(const KShadow &ks, const DEmitter &E, uint32_t e, uint32_t j, uint32_t ka, uint32_t kb,
					       f3 p, f3 &ldir, float &ldist, float &dsq, f3 &li)
{
	float u1 = 0.5f, u2 = 0.5f;
	if (uni(ks.rng) != RTX_RNG_CONST) /* the key already carries the seed (rtx_key_pixel) */
		rtx_draw2(key_of(ka, kb), e, j, &u1, &u2);
	sample_ray(uni(ks.rng), E, j, u1, u2, p, ldir, ldist, dsq, li);
}

/* an emitter record read through the scalar cache (every lane reads the same one) */
__device__ __forceinline__ DEmitter emitter_uni(const DEmitter *e)
{
	uint32_t w[sizeof(DEmitter) / 4];
	const auto *W = cptr((const uint32_t *)e);
#pragma unroll
	for (int i = 0; i < (int)(sizeof(DEmitter) / 4); i++)
		w[i] = W[i];
	DEmitter E;
	__builtin_memcpy(&E, w, sizeof(E));
	return E;
}

/* the shadow walks' view of the trees (QBvh) from the kernel arguments and the workgroup's LDS */
template <int WALK>
__device__ __forceinline__ QBvh make_qbvh(const KShadow &ks, const uint4 *top_q, const uint32_t *top_e, lds_u32 *stk,
					  const uint4 *t8, uint32_t wv)
{
	QBvh Q;
	Q.q = unip(ks.qnodes);
	Q.qo = mk3(ks.qo[0], ks.qo[1], ks.qo[2]);
	Q.qs = mk3(ks.qs[0], ks.qs[1], ks.qs[2]);
	Q.qsi = mk3(ks.qsi[0], ks.qsi[1], ks.qsi[2]);
	Q.top = top_q;
	Q.tend = top_e;
	Q.nt = uni(ks.ntop);
	Q.w8 = WALK == WALK_W8 ? unip(ks.w8) : nullptr;
	Q.w8s = WALK == WALK_W8 ? unip(ks.w8s) : nullptr;
	Q.t8 = t8;
	Q.nt8 = WALK == WALK_W8 ? min(uni(ks.w8top), (uint32_t)RTX_W8_TOP_MAX) : 0u;
	Q.spill = WALK == WALK_W8 ? unip(ks.w8spill) : nullptr;
	Q.wv = wv;
	Q.lstk = uni(ks.w8lstk);
	Q.sph = uni(ks.w8sph) != 0;
	Q.stk = stk;
	Q.tq = stk + RTX_W8_STACK * WAVE;
	return Q;
}

/* The cone cull and the per-point masks (point_masks below): every shadow ray of a shade point p
 * toward an emitter runs from p to a point of the emitter, so it lies in the cone from p around the
 * emitter's bounding sphere, cut at the sphere's far side; what the cone cannot meet, no sample's
 * ray can. */
__device__ __forceinline__ void emitter_sphere(const DEmitter &E, f3 &lc, float &lr)
{
	/* the emitter's bounding sphere: a sphere light itself (its light points are c + ld with |ld|
	 * the radius to a few ulp, light_point_sh), a triangle's circumscribing sphere about its
	 * centroid (its light points lie in it); padded by 1e-4 of the radius and 1e-6 of |c| */
	if (E.type == RTX_SPHERE) {
		lc = ld3(E.p0);
		lr = E.radius;
	} else {
		const f3 a = ld3(E.p0), b = ld3(E.p1), c = ld3(E.p2);
		lc = mul3s(add3(add3(a, b), c), 1.f / 3.f);
		lr = sqrtf(fmaxf(fmaxf(magsqr3(sub3(a, lc)), magsqr3(sub3(b, lc))), magsqr3(sub3(c, lc))));
	}
	lr = lr * 1.0001f + 1e-6f * fmaxf(fmaxf(fabsf(lc.x), fabsf(lc.y)), fabsf(lc.z));
}

/* the cone from p around the emitter's sphere (lc, lr), L = |lc - p| > 1.01 lr */
struct Cone {
	f3 ax;
	float L, lr, sn, cs, mag;
};
__device__ __forceinline__ Cone cone_of(f3 p, f3 lc, float lr, f3 ax0, float L)
{
	Cone c;
	c.ax = mul3s(ax0, 1.f / L);
	c.L = L;
	c.lr = lr;
	c.sn = lr / L;
	c.cs = sqrtf(fmaxf(0.f, 1.f - c.sn * c.sn));
	c.mag = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)) + fmaxf(fmaxf(fabsf(lc.x), fabsf(lc.y)), fabsf(lc.z));
	return c;
}
/* does the bounding sphere sp = {centre, radius} meet the cone from p?  REC: the sphere of a listed
 * record, padded by 1e-3 of its distance besides: hit_sphere's discriminant (|rel|^2 - r^2 against
 * b^2, each rounded at 2^-24 |rel|^2) is sure to be negative only for a ray that passes the sphere
 * by more than about 6e-4 |rel|, however small the sphere */
template <bool REC> __device__ __forceinline__ bool cone_meets(const Cone &c, f3 p, float4 sp)
{
	const f3 v = sub3(mk3(sp.x, sp.y, sp.z), p);
	const float vv = magsqr3(v), t = dot3(v, c.ax);
	const float e = sqrtf(fmaxf(0.f, vv - t * t));
	float br = sp.w + 2e-5f * (c.mag + sqrtf(vv) + c.L + c.lr);
	if (REC)
		br += 1e-3f * sqrtf(vv);
	return vv <= br * br || (t >= -br && t <= c.L + c.lr + br && e * c.cs - t * c.sn <= br);
}

/* Plane (n, dd, eps) is clear for shade point p and the emitter in the padded sphere (lc, lr), L =
 * |lc - p|: no ray from p to a point lp of the sphere can pass plane_blocks.  With s = dd - n.p (the
 * very expression plane_blocks forms) and h = n.lp - dd in [sc - rho, sc + rho], rho = lr |n|, every
 * such ray has a dist = h + s and t / dist = s / (h + s).  The sphere must lie strictly on one
 * side (|sc| - rho > m); then either
 *  - same side: p lies on the sphere's side too, by more than m: t < 0, or t > dist by the factor
 *    1 + (|sc| - rho) / |s|;
 *  - on or near the plane: |s| (L + lr) <= eps (|sc| - rho - |s|), so |t| = |s| / |a| <= eps and
 *    t > eps fails.
 * m = 2e-5 (|dd| + |n| (2 (|p| + |lc|) + L + lr)), max norms: some sixty times the float rounding of
 * s, sc, a dist (n.(lp - p), whose error is absolute in the coordinates) and of the quotients (1 ulp
 * each: v_rcp_f32, v_sqrt_f32), as the cone test's pads are.  (KAT: RTX_KAT_PLANE_CLEAR) */
__device__ __forceinline__ bool plane_clear(f3 n, float dd, float eps, f3 p, f3 lc, float lr, float L)
{
	if (!(eps > 0.f))
		return false;
	const float s = dd - dot3(n, p);
	const float nn = sqrtf(magsqr3(n));
	const float sc = dot3(n, lc) - dd;
	const float as = fabsf(s), reach = L + lr;
	const float pm = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)), lm = fmaxf(fmaxf(fabsf(lc.x), fabsf(lc.y)), fabsf(lc.z));
	const float m = 2e-5f * (fabsf(dd) + nn * (2.f * (pm + lm) + reach));
	const float hmin = fabsf(sc) - lr * nn - m;
	if (!(hmin > 0.f)) /* the sphere touches or straddles the plane (or a NaN) */
		return false;
	if (as > m && (sc > 0.f) == (s < 0.f))
		return true;
	return as * reach * 1.0001f <= eps * (hmin - as);
}

/* what point_masks decides once per shade point of the wave-uniform path, bit e for emitter e < 64 */
struct PointMasks {
	u64 cone; /* the cone toward e meets no top-level box of the tree (point_masks) */
	u64 pln;  /* every plane is clear for e (plane_clear) */
	u64 lin;  /* the cone toward e meets no listed record's bounding sphere (the record of e itself apart) */
	u64 smp;  /* the point samples e (e is not the object the point lies on) */
};

/* The masks of shade point p on object obj, formed before its packets (a far point: none).  The cone
 * test of one emitter runs over the lanes: lane k < n tests bounding sphere k of the 8-wide tree's
 * second level (DScene.cull, world space), then lane k < nr the listed record k's sphere
 * (DScene.lsph; at most 64, else the records are never clear): centre distance t
 * along the axis, e off it; a sphere misses the cone when e cos(a) - t sin(a) > r or it lies wholly
 * before p or beyond the light.  r is padded by 2e-5 of the coordinates' and distances' magnitudes,
 * far above the rays' float rounding, so a clear packet is one whose walks / record tests could reach
 * no primitive: skipping them changes no bit of the image (test_gpu_cone_cull_is_invisible,
 * tests/test_gpu_pointclear.py). */
__device__ __forceinline__ PointMasks point_masks(const KShadow &ks, f3 p, uint32_t obj, bool far)
{
	PointMasks m = { 0ull, 0ull, 0ull, 0ull };
	const bool pt = uni(ks.point) != 0;
	const uint32_t n = uni(ks.num_cull);
	if ((!n && !pt) || far)
		return m;
	const DEmitter *emitters = unip(ks.emitters);
	const uint32_t ne = min(uni(ks.num_emitters), 64u);
	const uint32_t num_lin = uni(ks.num_lin), num_planes = uni(ks.num_planes);
	const uint32_t nr = pt ? min(uni(ks.num_lsph), (uint32_t)WAVE) : 0u;
	const bool lin_ok = pt && nr == num_lin; /* every listed record has its sphere (or there is none) */
	for (uint32_t e = 0; e < ne; e++) {
		const DEmitter E = emitter_uni(emitters + e);
		const u64 bit = 1ull << e;
		if (E.obj != obj)
			m.smp |= bit;
		f3 lc;
		float lr;
		emitter_sphere(E, lc, lr);
		const f3 ax0 = sub3(lc, p);
		const float L = sqrtf(magsqr3(ax0));
		if (pt) {
			bool pc = true;
			for (uint32_t i = 0; i < num_planes; i++) { /* plane records are wave-uniform: s_load */
				const auto *pl = cptr(unip(ks.planes)) + i;
				pc = plane_clear(mk3(pl->n[0], pl->n[1], pl->n[2]), pl->d, pl->eps, p, lc, lr, L) && pc;
			}
			if (pc)
				m.pln |= bit;
			if (!num_lin)
				m.lin |= bit;
		}
		if (!(L > 1.01f * lr)) /* the point at or inside the light's sphere: no cone */
			continue;
		if (!n && !nr)
			continue;
		const Cone c = cone_of(p, lc, lr, ax0, L);
		const uint32_t k = lane_id();
		if (n && !ballot(k < n && cone_meets<false>(c, p, ldg4((const char *)(unip(ks.cull) + min(k, n - 1u)), 0))))
			m.cone |= bit;
		/* the records in a pass of their own: the bench scene's tree alone fills the 64 lanes */
		if (lin_ok && nr) {
			const uint32_t kr = min(k, nr - 1u);
			const uint32_t ro = gptr((const uint32_t *)(unip(ks.lin) + kr))[0]; /* DEmitter.obj */
			if (!ballot(k < nr && ro != E.obj && cone_meets<true>(c, p, ldg4((const char *)(unip(ks.lsph) + kr), 0))))
				m.lin |= bit;
		}
	}
	return m;
}

/* The lane-slot path's cone mask (RTX_OPT_SHADOW_CULL 2): each lane tests its own point's cones (emitters
 * e < 8) against every sphere in turn, the sphere and the emitter read through the scalar cache;
 * bit e set when no sphere meets.  A packet whose every live lane is clear for its emitter skips
 * the walk, as a clear point's packets do on the wave-uniform path. */
__device__ __forceinline__ uint32_t cone_mask_lane(const KShadow &ks, f3 p, bool own)
{
	const uint32_t n = uni(ks.num_cull);
	if (!n)
		return 0u;
	const DEmitter *emitters = unip(ks.emitters);
	const uint32_t ne = min(uni(ks.num_emitters), 8u);
	const float4 *cull = unip(ks.cull);
	uint32_t m = 0u;
	for (uint32_t e = 0; e < ne; e++) {
		const DEmitter E = emitter_uni(emitters + e);
		f3 lc;
		float lr;
		if (E.type == RTX_SPHERE) {
			lc = ld3(E.p0);
			lr = E.radius;
		} else {
			const f3 a = ld3(E.p0), b = ld3(E.p1), c = ld3(E.p2);
			lc = mul3s(add3(add3(a, b), c), 1.f / 3.f);
			lr = sqrtf(fmaxf(fmaxf(magsqr3(sub3(a, lc)), magsqr3(sub3(b, lc))), magsqr3(sub3(c, lc))));
		}
		lr = lr * 1.0001f + 1e-6f * fmaxf(fmaxf(fabsf(lc.x), fabsf(lc.y)), fabsf(lc.z));
		const f3 ax0 = sub3(lc, p);
		const float L = sqrtf(magsqr3(ax0));
		bool meets = !own || !(L > 1.01f * lr);
		if (ballot(!meets)) {
			const f3 ax = mul3s(ax0, 1.f / L);
			const float sn = lr / L, cs = sqrtf(fmaxf(0.f, 1.f - sn * sn));
			const float mag = fmaxf(fmaxf(fabsf(p.x), fabsf(p.y)), fabsf(p.z)) + fmaxf(fmaxf(fabsf(lc.x), fabsf(lc.y)), fabsf(lc.z));
			for (uint32_t k = 0; k < n && ballot(!meets); k++) {
				const auto *q = (const __attribute__((address_space(4))) f4v *)(cull + k);
				const f4v sp = *q;
				const f3 v = sub3(mk3(sp.x, sp.y, sp.z), p);
				const float vv = magsqr3(v), t = dot3(v, ax);
				const float e2 = sqrtf(fmaxf(0.f, vv - t * t));
				const float br = sp.w + 2e-5f * (mag + sqrtf(vv) + L + lr);
				meets = meets || vv <= br * br || (t >= -br && t <= L + lr + br && e2 * cs - t * sn <= br);
			}
		}
		if (!meets)
			m |= 1u << e;
	}
	return m;
}

/* count mode: the plane and listed-object tests that `na` rays toward emitter object eobj skip */
__device__ __forceinline__ void count_skips(const KShadow &ks, uint32_t na, uint32_t eobj, bool pclr, bool lclr, ShadowCount &sc)
{
	if (pclr)
		sc.pskip += (u64)na * uni(ks.num_planes);
	if (lclr) {
		const auto *lin = cptr(unip(ks.lin));
		uint32_t others = 0;
		for (uint32_t i = 0; i < uni(ks.num_lin); i++)
			others += lin[i].obj != eobj ? 1u : 0u;
		sc.lskip += (u64)na * others;
	}
}

/* one light sample per lane of the shade point `rec` (render.c:170-229): the light point of
 * sample idx (emitters in scene order, the hit object skipped), its shadow ray, attenuation
 * and Phong / Blinn.  Argument-block fields are read from LDS behind reread barriers. */
template <bool COUNT, int WALK, bool UNI, bool LA, bool SC = false, bool DK = false>
__device__ __forceinline__ f3 light_sample(const KShadow &ks, const float4 *rec_uni, uint32_t sidv, uint32_t idx, bool act, ShadowCount &sc,
					   const uint4 *top_q, const uint32_t *top_e, lds_u32 *stk, const uint4 *t8, uint32_t wv,
					   const uint32_t *cmask, uint32_t lclr = 0u)
{
	reread_barrier();
	/* the shade point's record: wave-uniform (UNI), or this lane's record sidv, whose address is
	 * formed again after the walk (the asm below) so only the 32-bit index lives across it: the
	 * 64-bit address did, and the allocator spilled it to scratch around the generic-octant walk,
	 * one store per packet (scene6: 43 GB of WRITE_SIZE per frame) */
	const float4 *rec = UNI ? rec_uni : unip(ks.sp) + (size_t)sidv * SPREC;
	const float4 q0 = sp_field<UNI>(rec, 0), q4 = sp_field<UNI>(rec, 4);
	const f3 p = mk3(q0.x, q0.y, q0.z);
	const uint32_t obj = __float_as_uint(q4.x) & ~RTX_SP_FAR, far = __float_as_uint(q4.x) & RTX_SP_FAR;
	const DEmitter *emitters = unip(ks.emitters);
	const auto *EM = cptr(emitters);
	const uint32_t num_emitters = uni(ks.num_emitters);
	/* the sample's emitter: one pass over the emitter table, read through the scalar cache */
	uint32_t j = idx, e = RTX_NONE;
	for (uint32_t k = 0; k < num_emitters; k++) {
		const uint32_t eo = EM[k].obj, enl = EM[k].num_lights;
		if (eo == obj || e != RTX_NONE)
			continue;
		if (j < enl)
			e = k;
		else
			j -= enl;
	}
	if (e == RTX_NONE)
		e = 0;
	/* every live lane's emitter the same (a packet inside one emitter's samples: the usual case):
	 * its record through the scalar cache too, else per lane */
	const u64 am = ballot(act);
	const uint32_t lead = readlane(e, am ? (uint32_t)__ffsll((long long)am) - 1 : 0u);
	f3 ldir, li;
	float ldist, dsq;
	uint32_t eobj;
	bool clear = false; /* UNI: the packet's cone meets no top-level box of the tree (point_masks) */
	bool pclr = false, rclr = false; /* UNI: its planes / listed records are clear */
	if (!ballot(act && e != lead)) {
		const DEmitter Eu = emitter_uni(emitters + lead);
		emitter_sample(ks, Eu, lead, j, __float_as_uint(q4.y), __float_as_uint(q4.z), p, ldir, ldist, dsq, li);
		eobj = Eu.obj;
		/* the point's cone mask, kept in the wave's LDS table (a 64-bit mask in SGPRs across the walk
		 * cost the walk a spilled register) */
		clear = UNI && WALK == WALK_W8 && lead < 64u && ((uni(cmask[lead >> 5]) >> (lead & 31u)) & 1u);
		/* ... and its plane and listed-object masks (point_masks): the packet runs neither loop */
		if (UNI && lead < 64u) { /* the masks hold emitters 0..63 */
			pclr = (uni(cmask[2 + (lead >> 5)]) >> (lead & 31u)) & 1u;
			rclr = (uni(cmask[4 + (lead >> 5)]) >> (lead & 31u)) & 1u;
		}
	} else {
		const DEmitter &E = emitters[e];
		emitter_sample(ks, E, e, j, __float_as_uint(q4.y), __float_as_uint(q4.z), p, ldir, ldist, dsq, li);
		eobj = E.obj;
	}
	/* the lane-slot path: every live lane's point clear for its emitter (cone_mask_lane) */
	if (!UNI && SC) {
		const bool lc = e < 8u && ((lclr >> (e & 7u)) & 1u);
		clear = ballot(act) && !ballot(act && !lc);
	}
	const float attf = sample_att(ks, ldist, dsq);
	/* the wave-uniform path's dark samples (sample_dark) take no part in the query: their lanes
	 * enter it as idle ones, and a packet of dark samples alone runs neither loop nor walk.  A
	 * packet the cone cull cleared has no walk to save: its samples are not looked at */
	bool qry = act;
	bool none = false;
	if (UNI && DK && uni(ks.dark) && !far && !clear) {
		qry = act && !sample_dark<UNI>(ks, rec, ldir, li, attf, act);
		none = !ballot(qry);
	}
	const QBvh Q = make_qbvh<WALK>(ks, top_q, top_e, stk, t8, wv);
	const bool have_tree = uni(ks.have_tree) != 0 && !RTX_DEBUG_NOWALK && !clear && !none;
	if (COUNT && clear)
		sc.clear += (u64)popc64(ballot(act));
	if (COUNT && UNI) {
		count_skips(ks, popc64(ballot(act)), eobj, pclr, rclr, sc);
		/* the dark rays of packets the cone cull had not cleared; shadow_plane_tests keeps counting
		 * the plane tests of every ray the plane mask did not clear, dark ones included */
		const uint32_t nd = popc64(ballot(act && !qry));
		sc.dark += nd;
		if (none)
			sc.dpack += nd;
		sc.pln += (u64)nd * (pclr ? 0u : uni(ks.num_planes));
	}
	const bool blocked = shadow_query<COUNT, WALK, LA>(Q, unip(ks.recs), unip(ks.mats), unip(ks.planes),
							 (UNI && (pclr || none)) ? 0u : uni(ks.num_planes), unip(ks.lin),
							 (UNI && (rclr || none)) ? 0u : uni(ks.num_lin), have_tree, ks.tf, qry, far != 0, p, ldir,
							 ldist, eobj, li, sc);
	reread_barrier();
	if (!UNI) {
		asm volatile("" : "+v"(sidv));
		rec = unip(ks.sp) + (size_t)sidv * SPREC;
	}
	f3 contribution = mk3(0.f, 0.f, 0.f);
	if (qry && !blocked)
		contribution = shade_light<UNI>(ks, rec, ldir, li, attf);
	return contribution;
}

/* clear_run's packets of emitter E, whose samples are [start, end), from `base` up to the first that
 * straddles the next emitter or nl; S0: the point's shininess is 0 (shade_terms_s0).  Returns the rays. */
template <bool COUNT, bool S0>
__device__ __forceinline__ uint32_t clear_packets(const DEmitter &E, uint64_t mix, int32_t rng, int32_t att, int32_t refl, float att_offset,
						  f3 p, f3 n, f3 dir, f3 kd, f3 ks3, float shin, uint32_t nl, uint32_t start, uint32_t end,
						  uint32_t &base, f3 &acc)
{
	uint32_t rays = 0;
	for (; base < nl && min(base + WAVE, nl) <= end; base += WAVE) {
		const uint32_t idx = base + lane_id(), j = idx - start;
		const bool act = idx < nl;
		float u1 = 0.5f, u2 = 0.5f;
		if (rng != RTX_RNG_CONST)
			rtx_draw2_mixed(mix, j, &u1, &u2);
		f3 ldir, li;
		float ldist, dsq;
		sample_ray(rng, E, j, u1, u2, p, ldir, ldist, dsq, li);
		const float attf = sample_att_of(att, att_offset, ldist, dsq);
		f3 contribution = mk3(0.f, 0.f, 0.f);
		if (act)
			contribution = S0 ? shade_terms_s0(att, n, kd, ks3, ldir, li, attf) :
					    shade_terms(att, refl, n, dir, kd, ks3, shin, ldir, li, attf);
		acc = add3(acc, contribution);
		if (COUNT)
			rays += popc64(ballot(act));
	}
	return rays;
}

/* The packets of an all-clear shade point `rec` (point_masks: for every emitter it samples, the
 * tree part, the planes and the listed records are clear), from sample `base` on: every sample is
 * unblocked and its intensity untouched, so a packet inside one emitter's samples is light_sample
 * without shadow_query: the same float operations in the same order per sample, each lane adding
 * its samples to acc in packet order.  The shade point's fields, its material, the argument-block
 * fields and, per emitter, the emitter's record and the (key, stream) mix of its draws are formed
 * once here, not per packet, and nothing is re-read behind a barrier (there is no walk to keep
 * registers free for).  Returns the first packet that straddles two emitters (the caller runs it
 * through light_sample), or one at or beyond nl. */
template <bool COUNT, int WALK>
__device__ __forceinline__ uint32_t clear_run(const KShadow &ks, const float4 *rec, uint32_t nl, uint32_t base, f3 &acc, ShadowCount &sc,
					      const uint32_t *cmask)
{
	const float4 q0 = sp_field<true>(rec, 0), q1 = sp_field<true>(rec, 1), q2 = sp_field<true>(rec, 2), q3 = sp_field<true>(rec, 3),
		     q4 = sp_field<true>(rec, 4);
	const f3 p = mk3(q0.x, q0.y, q0.z), n = mk3(q1.x, q1.y, q1.z), dir = mk3(q2.x, q2.y, q2.z), kd = mk3(q3.x, q3.y, q3.z);
	const uint32_t obj = __float_as_uint(q4.x) & ~RTX_SP_FAR;
	const uint64_t key = key_of(__float_as_uint(q4.y), __float_as_uint(q4.z));
	const auto &mat = cptr(unip(ks.mats))[__float_as_uint(q3.w)];
	const f3 ks3 = mk3(mat.ks[0], mat.ks[1], mat.ks[2]);
	const float shin = mat.shininess;
	/* RTX_OPT_SHADOW_SPEC: a shininess-0 point's packets run shade_terms_s0, which reads no reflection model:
	 * refl = -1 says so (one scalar fewer across the loops than a flag of its own, which cost the walking
	 * instances SGPR spills); else RTX_BLINN or, as shade_pw reads every other value, RTX_PHONG */
	const int32_t rng = (int32_t)uni((uint32_t)ks.rng), att = (int32_t)uni((uint32_t)ks.attenuation),
		      refl = (shin_zero(shin) && uni(ks.spec)) ? -1 : (int32_t)uni((uint32_t)ks.reflection) == RTX_BLINN ? RTX_BLINN : RTX_PHONG;
	const float att_offset = __uint_as_float(uni(__float_as_uint(ks.att_offset)));
	const DEmitter *emitters = unip(ks.emitters);
	const auto *EM = cptr(emitters);
	const uint32_t ne = uni(ks.num_emitters);
	/* emitter cur's samples are [start, end); nxt: the next emitter to look at */
	uint32_t nxt = 0, cur = 0, start = 0, end = 0;
	while (base < nl) {
		while (base >= end && nxt < ne) {
			const uint32_t eo = EM[nxt].obj, enl = EM[nxt].num_lights;
			if (eo != obj) {
				cur = nxt;
				start = end;
				end = start + enl;
			}
			nxt++;
		}
		if (base >= end || min(base + WAVE, nl) > end) /* no emitter found (never), or a straddling packet */
			break;
		const DEmitter E = emitter_uni(emitters + cur);
		const uint64_t mix = rtx_draw_mix(key, cur);
		/* the point's shininess picks the loop, once: the one of a shininess-0 point holds no shade_pw */
		const uint32_t rays = refl < 0 ? clear_packets<COUNT, true>(E, mix, rng, att, refl, att_offset, p, n, dir, kd, ks3, shin, nl, start, end, base, acc) :
					   clear_packets<COUNT, false>(E, mix, rng, att, refl, att_offset, p, n, dir, kd, ks3, shin, nl, start, end, base, acc);
		if (COUNT) {
			if (WALK == WALK_W8 && ((uni(cmask[cur >> 5]) >> (cur & 31u)) & 1u))
				sc.clear += rays;
			count_skips(ks, rays, E.obj, true, true, sc);
		}
	}
	return base;
}

/* The sample order of a walking point (RTX_OPT_SHADOW_ORDER).  A packet of 64 samples walks as long
 * as its longest lane, and where a sample's light point lies across the cone from the shade point to
 * the emitter predicts what its ray crosses: the occluder's silhouette cuts the emitter's disc.  So
 * the samples [base, base + n) of one emitter, 64 < n <= RTX_ORD_CAP, every packet of them inside
 * that emitter's samples, are walked in the order of a key: the bucket, of RTX_ORD_BUCKETS, of
 * x = (lp - c) . b / lr, with (c, lr) the emitter's bounding sphere (emitter_sphere), lp the light
 * point (p + ldist ldir; c - p is along the axis, so x = ldist (ldir . b) / lr) and b the unit
 * vector across the cone axis toward the centre of the bounded objects' box (DTreeFrame c + cf; or, with that centre
 * on the axis, across the world axis the cone axis is least along).  Dark samples (sample_dark)
 * get no place in the order: they are never walked.
 *   The key pass runs the packets in index order: each lane forms its sample as light_sample does
 * (emitter_sample, sample_att, sample_dark: the same operations, so the same dark lanes), keeps
 * the bucket in registers (a run has at most 16 packets: 4 bits a packet and a "placed" bit) and
 * counts the buckets (lane b holds bucket b's count).  A second pass ranks every sample inside its
 * bucket from ballots of the bucket's bits (order_bits, order_same: stable in the index), stores
 * order[pos] = index - base, and zeroes the result slots of the samples without a place: a placed
 * sample's slot is stored after its walk, blocked or not.  The caller walks the packets of
 * positions [64 k, 64 k + 64), stores each contribution at its sample's result slot and adds the
 * slots in index order, lane l taking l, 64 + l, ..: the additions today's loop makes, in its order.
 *   ob: the wave's slice of KShadow.ord: order[RTX_ORD_CAP], then the samples' result records, 12
 * bytes (x, y, z) each, one store and one load a sample.  Nothing in a slice outlives its run, so
 * it is never cleared.  Returns 0 (the run is not ordered: today's packets), or
 * bit 31 | packets of the run << 16 | samples in the order.  (KAT: RTX_KAT_ORDER) */
__device__ __forceinline__ uint32_t order_bucket(float x)
{
	const float v = floorf((x + 1.f) * (0.5f * (float)RTX_ORD_BUCKETS));
	return (uint32_t)fminf(fmaxf(v, 0.f), (float)(RTX_ORD_BUCKETS - 1u)); /* NaN -> 0 */
}
/* the key's direction for the shade point p and the emitter sphere's centre lc */
__device__ __forceinline__ f3 order_dir(f3 p, f3 lc, f3 tc)
{
	const f3 ax = sub3(lc, p), ref = sub3(tc, p);
	const float aa = fmaxf(magsqr3(ax), 1e-37f);
	f3 b = sub3(ref, mul3s(ax, dot3(ref, ax) / aa));
	if (!(magsqr3(b) > 1e-8f * magsqr3(ref))) { /* the centre on the axis (or not finite) */
		const float fx = fabsf(ax.x), fy = fabsf(ax.y), fz = fabsf(ax.z);
		const f3 w = fx <= fy && fx <= fz ? mk3(1.f, 0.f, 0.f) : fy <= fz ? mk3(0.f, 1.f, 0.f) : mk3(0.f, 0.f, 1.f);
		b = sub3(w, mul3s(ax, dot3(w, ax) / aa));
	}
	return mul3s(b, 1.f / sqrtf(fmaxf(magsqr3(b), 1e-37f)));
}
/* sample j of emitter number e (Eu) of the shade point `rec` at p, formed as light_sample forms it:
 * its bucket, RTX_ORD_BUCKETS for a dark or idle one; *xo: the key's x */
__device__ __forceinline__ uint32_t order_key(const KShadow &ks, const float4 *rec, const DEmitter &Eu, uint32_t e, uint32_t j, uint32_t ka,
					      uint32_t kb, f3 p, f3 b, float ilr, bool dk_on, bool act, bool &dark, float *xo = nullptr)
{
	f3 ldir, li;
	float ldist, dsq;
	emitter_sample(ks, Eu, e, j, ka, kb, p, ldir, ldist, dsq, li);
	const float attf = sample_att(ks, ldist, dsq);
	dark = false;
	if (dk_on)
		dark = sample_dark<true>(ks, rec, ldir, li, attf, act);
	const float x = ldist * dot3(ldir, b) * ilr;
	if (xo)
		*xo = x;
	return act && !dark ? order_bucket(x) : RTX_ORD_BUCKETS;
}
/* sample jr's result record in the wave's slice ob: 12 bytes after the order's words, one store and
 * one load (global_*_dwordx3; the values through VGPRs formed here, or the zeroes of order_begin
 * are hoisted to the kernel's entry and spilled) */
__device__ __forceinline__ void order_slot_put(uint32_t *ob, uint32_t jr, f3 v)
{
	auto *r = gptrw((float *)ob + RTX_ORD_CAP + 3u * jr);
	asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z));
	r[0] = v.x;
	r[1] = v.y;
	r[2] = v.z;
}
__device__ __forceinline__ f3 order_slot_get(const uint32_t *ob, uint32_t jr)
{
	const auto *r = gptr((const float *)ob + RTX_ORD_CAP + 3u * jr);
	return mk3(r[0], r[1], r[2]);
}
/* One packet's buckets as lane masks: word b < 4 has the lanes whose bucket has bit b set, word 4 the
 * lanes with a place in the order.  The words are copied to VGPRs once, so what order_same does with
 * them has no scalar operand (any SGPR operand halves the VALU issue rate, bench.py's header). */
struct OrderBits {
	uint32_t lo[5], hi[5];
};
__device__ __forceinline__ void order_bits(uint32_t bk, OrderBits &o)
{
	for (uint32_t k = 0; k < 5; k++) {
		const u64 m = ballot(k < 4 ? ((bk >> k) & 1u) != 0u : bk < RTX_ORD_BUCKETS);
		o.lo[k] = (uint32_t)m;
		o.hi[k] = (uint32_t)(m >> 32);
		asm volatile("" : "+v"(o.lo[k]), "+v"(o.hi[k]));
	}
}
/* the packet's placed samples of bucket sel & 15 (sel per lane): the AND over the key's bits of
 * (bit set ? B_b : ~B_b), and the placed lanes.  Returns their number; *below: those in lanes below
 * this one, a sample's rank among its packet's samples of its bucket (stable in the index) */
__device__ __forceinline__ uint32_t order_same(const OrderBits &o, uint32_t sel, uint32_t *below)
{
	uint32_t lo = o.lo[4], hi = o.hi[4];
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t inv = ((sel >> k) & 1u) - 1u; /* all ones where the bit is clear */
		lo &= o.lo[k] ^ inv;
		hi &= o.hi[k] ^ inv;
	}
	if (below)
		*below = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
	return (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
}
template <bool COUNT, int WALK>
__device__ __forceinline__ uint32_t order_begin(const KShadow &ks, const float4 *rec, uint32_t nl, uint32_t base, const uint32_t *cmask,
						uint32_t *ob, ShadowCount &sc)
{
	const float4 q0 = sp_field<true>(rec, 0), q4 = sp_field<true>(rec, 4);
	if (__float_as_uint(q4.x) & RTX_SP_FAR)
		return 0u;
	const f3 p = mk3(q0.x, q0.y, q0.z);
	const uint32_t obj = __float_as_uint(q4.x);
	const DEmitter *emitters = unip(ks.emitters);
	const auto *EM = cptr(emitters);
	const uint32_t ne = uni(ks.num_emitters);
	/* the emitter of sample `base` (light_sample's search) and its samples [start, end) */
	uint32_t e = RTX_NONE, start = 0, end = 0;
	for (uint32_t k = 0; k < ne && e == RTX_NONE; k++) {
		const uint32_t eo = EM[k].obj, enl = EM[k].num_lights;
		if (eo == obj)
			continue;
		start = end;
		end += enl;
		if (base < end)
			e = k;
	}
	if (e == RTX_NONE || e >= 64u)
		return 0u;
	const uint32_t rend = end >= nl ? nl : (end & ~(uint32_t)(WAVE - 1)); /* the packets before it lie inside the emitter */
	/* a run begins at the emitter's first whole packet and takes all of them, or none: a longer run
	 * is not cut into ordered pieces */
	if (rend <= base || base - start >= WAVE || rend - base <= WAVE || rend - base > RTX_ORD_CAP)
		return 0u;
	if (WALK == WALK_W8 && ((uni(cmask[e >> 5]) >> (e & 31u)) & 1u)) /* cone-clear: its packets do not walk */
		return 0u;
	const uint32_t n = rend - base, npk = (n + WAVE - 1) / WAVE;
	const bool pclr = (uni(cmask[2 + (e >> 5)]) >> (e & 31u)) & 1u, rclr = (uni(cmask[4 + (e >> 5)]) >> (e & 31u)) & 1u;
	const DEmitter Eu = emitter_uni(emitters + e);
	f3 lc;
	float lr;
	emitter_sphere(Eu, lc, lr);
	/* the centre of the bounded objects' world box, as the trees' frame holds it */
	const f3 b = order_dir(p, lc, mk3(ks.tf.c[0] + ks.tf.cf[0], ks.tf.c[1] + ks.tf.cf[1], ks.tf.c[2] + ks.tf.cf[2]));
	const float ilr = lr > 0.f ? 1.f / lr : 0.f;
	const bool dk_on = uni(ks.dark) != 0;
	auto *ord = gptrw(ob);
	/* the lane's buckets of the run's packets: 4 bits a packet, and a bit a packet for "has a place" */
	u64 bks = 0;
	uint32_t plc = 0;
	uint32_t cnt = 0; /* lane l: the samples of bucket l & 15 */
	for (uint32_t m = 0; m < npk; m++) {
		const uint32_t idx = base + m * WAVE + lane_id();
		const bool act = idx < rend;
		bool dark;
		const uint32_t bk = order_key(ks, rec, Eu, e, idx - start, __float_as_uint(q4.y), __float_as_uint(q4.z), p, b, ilr, dk_on, act, dark);
		bks |= (u64)(bk & (RTX_ORD_BUCKETS - 1u)) << (4u * m);
		plc |= (bk < RTX_ORD_BUCKETS ? 1u : 0u) << m;
		OrderBits ob5;
		order_bits(bk, ob5);
		cnt += order_same(ob5, lane_id(), nullptr);
		if (COUNT) { /* what light_sample counts for the dark lanes of this packet in index order */
			const uint32_t na = popc64(ballot(act)), nd = popc64(ballot(act && dark));
			sc.dark += nd;
			if (nd == na)
				sc.dpack += nd;
			sc.pln += (u64)nd * (pclr ? 0u : uni(ks.num_planes));
			count_skips(ks, nd, Eu.obj, pclr, rclr, sc);
		}
	}
	uint32_t total;
	uint32_t first = wave_excl_scan(lane_id() < RTX_ORD_BUCKETS ? cnt : 0u, &total); /* lane b < 16: the first position of bucket b */
	for (uint32_t m = 0; m < npk; m++) {
		const uint32_t jr = m * WAVE + lane_id();
		const bool placed = (plc >> m) & 1u;
		const uint32_t bk = placed ? (uint32_t)(bks >> (4u * m)) & (RTX_ORD_BUCKETS - 1u) : RTX_ORD_BUCKETS;
		OrderBits ob5;
		order_bits(bk, ob5);
		uint32_t rank;
		order_same(ob5, bk, &rank);
		/* the bucket's first free position, from the lane that holds it (a sample without a place reads lane 16) */
		const uint32_t f = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(bk << 2), (int)first);
		first += order_same(ob5, lane_id(), nullptr);
		if (placed)
			ord[f + rank] = jr;
		else
			order_slot_put(ob, jr, mk3(0.f, 0.f, 0.f)); /* +0.f: what a dark or idle sample adds; a placed one's lane stores after its walk */
	}
	lds_sync(); /* the order and the zeroed slots, before other lanes read and write them */
	if (COUNT) {
		sc.ordpt += 1;
		sc.ordray += total;
	}
	return 0x80000000u | (npk << 16) | total;
}

/* ------------------------------------------------------------------------ */
/* the kernel                                                               */
/* ------------------------------------------------------------------------ */
/* Persistent workgroups of RTX_SH_NW waves.  A workgroup copies the threaded BVH's top levels
 * to LDS once; then each wave takes per_wave shade points at a time from a global queue
 * (RTX_C_SPQUEUE), in processing (Morton) order, until the points run out. */
/* PATH: 0 both packet layouts (a runtime branch on slot_b: the counting instances), 1 only the
 * wave-uniform packets (slot_b = 64), 2 only the lane slots (slot_b < 64), 3 the lane slots with
 * their cone cull (RTX_OPT_SHADOW_CULL 2), 4 the wave-uniform packets with their dark samples left
 * out of the query (RTX_OPT_SHADOW_DARK), 5 those with the walking points' samples in key order
 * besides (RTX_OPT_SHADOW_ORDER, order_begin).  The product launches a
 * kernel of one layout, so each gets a register allocation of its own: with both in one kernel a
 * change to the slot loop moved the uniform loop's spills into its walk */
template <bool COUNT, int OCC, int WALK, int PATH>
__global__ __launch_bounds__(WAVE *RTX_SH_NW, OCC) void k_shadow(KShadow ka)
{
	constexpr bool TOP = WALK == WALK_BVH2;
	__shared__ uint4 top_q[TOP ? RTX_TOP_MAX : 1];    /* the top records (rtx_device.h RTX_QTOP_CUT) */
	__shared__ uint32_t top_e[TOP ? RTX_TOP_MAX : 1]; /* cut records: the DQNode index after the subtree */
	/* the wide walks' lane stacks (16-byte aligned: the slot fold below reuses a wave's stack area as
	 * float4 records) */
	__shared__ __attribute__((aligned(16))) uint32_t wstk[RTX_SH_NW][WALK == WALK_W8 ? RTX_W8_STACK + RTX_W8_TQ : 1][WAVE];
	static_assert(WALK != WALK_W8 || (RTX_W8_STACK + RTX_W8_TQ) * WAVE * sizeof(uint32_t) >= WAVE * sizeof(float4),
		      "a wave's lane-stack area must hold one float4 per lane for the slot fold");
	__shared__ KShadow ks_s; /* the arguments, one copy for the workgroup */
	/* WALK_W8: the 8-wide tree's top levels (RTX_W8_TOP_LEVELS), read by divergent steps from LDS */
	__shared__ uint4 t8[WALK == WALK_W8 ? RTX_W8_TOP_MAX * 4 : 1];
	/* one wave's tables in one struct, so every lane addresses them from one base register */
	struct WaveTables {
		uint32_t off[WAVE + 1]; /* first lane slot of each shade point, total */
		uint32_t nls[WAVE];     /* shadow rays of each shade point */
		uint32_t sid[WAVE];     /* each shade point's index in the record array */
		float Ls[3][WAVE];      /* per shade point light sum, in packet order */
		uint32_t cm[8];         /* the current point's masks (wave-uniform path, point_masks): cone, planes, listed
		                         * objects (two words each), all-clear flag, unused */
		uint8_t clr[WAVE];      /* each shade point's cone_mask_lane, emitters 0..7 (lane-slot path; a byte:
		                         * the LDS of two workgroups must still fit a CU) */
	};
	__shared__ WaveTables wt_w[RTX_SH_NW];
	const uint32_t ntop = TOP ? ka.ntop : 0u;
	for (uint32_t i = threadIdx.x; i < ntop; i += WAVE * RTX_SH_NW) {
		top_q[i] = ldg4u(ka.top + 4 * i);
		top_e[i] = gptr(ka.top)[4 * ntop + i];
	}
	const uint32_t nt8 = WALK == WALK_W8 ? min(ka.w8top, (uint32_t)RTX_W8_TOP_MAX) : 0u;
	for (uint32_t i = threadIdx.x; i < 4 * nt8; i += WAVE * RTX_SH_NW)
		t8[i] = ldg4u((const uint32_t *)ka.w8 + 4 * i);
	const uint32_t wv = uni(threadIdx.x / WAVE);
	if (threadIdx.x == 0)
		ks_s = ka;
	__syncthreads();
	KShadow &ks = ks_s;
	uint32_t *off = wt_w[wv].off, *nls = wt_w[wv].nls, *sid = wt_w[wv].sid;
	uint8_t *clr = wt_w[wv].clr;
	float(*Ls)[WAVE] = wt_w[wv].Ls;
	/* the lane-stack addresses: per lane, or formed from lane_id() at each access in the lane-slot
	 * kernels, whose allocation spilled the per-lane address and reloaded it at every push and pop */
	constexpr bool LA = PATH == 2 || PATH == 3;
	/* the lane-slot path's cone cull (RTX_OPT_SHADOW_CULL 2) lives in its own instance, PATH 3, so
	 * the default lane-slot kernel keeps its register allocation (with the code present but off,
	 * scene6's k_shadow took 1083.4 against 1074.8 ms) */
	constexpr bool SC = WALK == WALK_W8 && (PATH == 3 || PATH == 0);
	/* the dark samples (RTX_OPT_SHADOW_DARK) live in an instance of their own too, PATH 4: PATH 1 with
	 * sample_dark, launched where the option is on and the scene walks a tree.  A scene without a
	 * tree keeps PATH 1 as it was (with the code present but off, scene3's k_shadow took 52.7
	 * against 52.4 ms) */
	constexpr bool DK = PATH == 4 || PATH == 5 || PATH == 0;
	/* the sample order (RTX_OPT_SHADOW_ORDER) likewise, PATH 5: PATH 4 with order_begin (the dark
	 * samples follow KShadow.dark at run time, so it serves RTX_OPT_SHADOW_DARK 0 too) */
	constexpr bool ORD = PATH == 5 || PATH == 0;
	lds_u32 *stk = (lds_u32 *)&wstk[wv][0][LA ? 0u : lane_id()];
	ShadowCount sc = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	u64 rays_total = 0;
	for (;;) {
		reread_barrier();
		uint32_t j0 = 0;
		if (lane_id() == 0)
			j0 = (uint32_t)atomicAdd(unip(ks.ctr) + RTX_C_SPQUEUE, (unsigned long long)uni(ks.per_wave));
		j0 = readlane(j0, 0);
		const uint32_t n_sp = uni(ks.n_sp);
		if (j0 >= n_sp)
			break;
		const uint32_t cnt = min(uni(ks.per_wave), n_sp - j0);
		const bool own = lane_id() < cnt;
		const uint32_t *perm = unip(ks.perm);
		const uint32_t my_sid = own ? (perm ? perm[j0 + lane_id()] : j0 + lane_id()) : 0u;
		const uint32_t nl_mine = own ? __float_as_uint(unip(ks.sp)[(size_t)my_sid * SPREC + 4].w) : 0u;
		/* each point's samples occupy whole lane slots of B lanes (B = power of two), so a point's
		 * packet partial sums never depend on which other points share its wave: deterministic */
		uint32_t total;
		const uint32_t ex = wave_excl_scan((nl_mine + uni(ks.slot_b) - 1) >> uni(ks.slot_lg), &total);
		off[lane_id()] = ex;
		nls[lane_id()] = nl_mine;
		sid[lane_id()] = my_sid;
		Ls[0][lane_id()] = 0.f;
		Ls[1][lane_id()] = 0.f;
		Ls[2][lane_id()] = 0.f;
		if (lane_id() == 0)
			off[WAVE] = total;
		lds_sync();
		if (PATH == 1 || PATH == 4 || PATH == 5 || (PATH == 0 && uni(ks.slot_b) == WAVE)) {
			/* >= 64 lights: every packet is 64 samples of ONE shade point.  The point is wave-uniform
			 * (its record is read once per packet through one address, no owner search), each lane
			 * sums its samples over the point's packets, and one butterfly per point reduces them. */
			for (uint32_t k = 0; k < cnt; k++) {
				reread_barrier();
				const uint32_t nl = uni(nls[k]);
				const float4 *rec = unip(ks.sp) + (size_t)uni(sid[k]) * SPREC;
				if (const uint32_t *pm = unip(ks.pm)) {
					/* the masks k_point_masks formed for this record, one scalar load: a byte each for
					 * cone, planes, listed objects and sampled emitters (at most 8 emitters), handed over
					 * as point_masks' are below.  The smp byte is 0 for a far point only */
					const uint32_t w = cptr(pm)[uni(sid[k])];
					const bool tree = uni(ks.have_tree) != 0 && RTX_DEBUG_NOWALK != 1;
					const uint32_t smp = w >> 24, ok = (w >> 8) & (w >> 16) & (tree ? w : ~0u) & 0xffu;
					const bool ac = uni(ks.point) != 0 && smp && !(smp & ~ok);
					if (lane_id() == 0) {
						wt_w[wv].cm[0] = w & 0xffu;
						wt_w[wv].cm[1] = 0u;
						wt_w[wv].cm[2] = (w >> 8) & 0xffu;
						wt_w[wv].cm[3] = 0u;
						wt_w[wv].cm[4] = (w >> 16) & 0xffu;
						wt_w[wv].cm[5] = 0u;
						wt_w[wv].cm[6] = ac ? 1u : 0u;
						if (ORD)
							wt_w[wv].cm[7] = 0u;
					}
					lds_sync();
				} else {
					/* the point through vector loads made uniform, not the scalar loads light_sample
					 * makes: shared with them, the point was live from here and the compiler hoisted
					 * the far path's double-precision copies of it out of the packet loop and
					 * spilled them, three stores per point */
					const float4 q0 = ldg4(rec, 0), q4 = ldg4(rec, 64);
					const f3 pu = mk3(__uint_as_float(uni(__float_as_uint(q0.x))), __uint_as_float(uni(__float_as_uint(q0.y))),
							  __uint_as_float(uni(__float_as_uint(q0.z))));
					const uint32_t ou = uni(__float_as_uint(q4.x));
					PointMasks m = { 0ull, 0ull, 0ull, 0ull };
					if (WALK == WALK_W8 || uni(ks.point))
						m = point_masks(ks, pu, ou & ~RTX_SP_FAR, (ou & RTX_SP_FAR) != 0);
					/* all-clear: every emitter the point samples is clear of the tree (or there is none),
					 * the planes and the listed records */
					const bool tree = uni(ks.have_tree) != 0 && RTX_DEBUG_NOWALK != 1;
					const u64 ok = m.pln & m.lin & (tree ? m.cone : ~0ull);
					const bool ac = uni(ks.point) != 0 && !(ou & RTX_SP_FAR) && uni(ks.num_emitters) <= 64u && !(m.smp & ~ok);
					if (lane_id() == 0) {
						wt_w[wv].cm[0] = (uint32_t)m.cone;
						wt_w[wv].cm[1] = (uint32_t)(m.cone >> 32);
						wt_w[wv].cm[2] = (uint32_t)m.pln;
						wt_w[wv].cm[3] = (uint32_t)(m.pln >> 32);
						wt_w[wv].cm[4] = (uint32_t)m.lin;
						wt_w[wv].cm[5] = (uint32_t)(m.lin >> 32);
						wt_w[wv].cm[6] = ac ? 1u : 0u;
						if (ORD)
							wt_w[wv].cm[7] = 0u;
					}
					lds_sync();
				}
				f3 acc = mk3(0.f, 0.f, 0.f);
				if (COUNT && uni(wt_w[wv].cm[6]))
					sc.pclear += nl;
				for (uint32_t base = 0; base < nl;) {
					/* an all-clear point: its packets inside one emitter's samples in clear_run */
					reread_barrier();
					if (uni(wt_w[wv].cm[6])) {
						base = clear_run<COUNT, WALK>(ks, rec, nl, base, acc, sc, wt_w[wv].cm);
						if (base >= nl)
							break;
					}
					uint32_t idx = base + lane_id();
					bool act = idx < nl;
					if (ORD) {
						/* the sample order: cm[7] holds a run's state across its walks (order_begin's word,
						 * the walked packets in bits 11..15), 0 outside a run.  At a packet outside one,
						 * an ordered run may begin; inside one, the lanes take the samples of the next 64
						 * positions of the order */
						uint32_t st = uni(wt_w[wv].cm[7]);
						uint32_t *ob = unip(ks.ord);
						if (ob)
							ob += (size_t)(blockIdx.x * RTX_SH_NW + wv) * RTX_ORD_WORDS;
						if (!st && ob && uni(ks.have_tree) && RTX_DEBUG_NOWALK != 1 && !uni(wt_w[wv].cm[6])) {
							st = order_begin<COUNT, WALK>(ks, rec, nl, base, wt_w[wv].cm, ob, sc);
							if (st && !(st & 0x7ffu)) {
								/* every sample dark: nothing to walk, and the slots' +0 leave acc as it is
								 * (acc is never -0: it starts at +0 and x + y is -0 only for x = y = -0) */
								base += ((st >> 16) & 31u) * WAVE;
								continue;
							}
							if (st) {
								if (lane_id() == 0)
									wt_w[wv].cm[7] = st;
								lds_sync();
							}
						}
						if (st) {
							const uint32_t pos = ((st >> 11) & 31u) * WAVE + lane_id();
							act = pos < (st & 0x7ffu);
							idx = base + (act ? gptr(ob)[pos] : 0u);
						}
					}
					const f3 contribution = light_sample<COUNT, WALK, true, LA, false, DK>(ks, rec, 0u, idx, act, sc, top_q, top_e, stk, t8,
													       wv, wt_w[wv].cm);
					if (ORD) {
						/* the run's state again from LDS, and the lane's sample again from the order: neither
						 * lives in a register across the walk */
						reread_barrier();
						const uint32_t st = uni(wt_w[wv].cm[7]);
						if (st) {
							uint32_t *ob = unip(ks.ord) + (size_t)(blockIdx.x * RTX_SH_NW + wv) * RTX_ORD_WORDS;
							const uint32_t pk = (st >> 11) & 31u, npk = (st >> 16) & 31u, no = st & 0x7ffu;
							const uint32_t pos = pk * WAVE + lane_id();
							if (pos < no) {
								order_slot_put(ob, gptr(ob)[pos], contribution);
							}
							const bool last = (pk + 1) * WAVE >= no;
							if (last) {
								lds_sync(); /* every lane's results, before the lanes that add them */
								for (uint32_t m = 0; m < npk; m++) {
									const uint32_t jr = m * WAVE + lane_id();
									acc = add3(acc, order_slot_get(ob, jr));
								}
								base += npk * WAVE;
							}
							if (lane_id() == 0)
								wt_w[wv].cm[7] = last ? 0u : st + (1u << 11);
							lds_sync();
							continue;
						}
					}
					acc = add3(acc, contribution);
					base += WAVE;
				}
				const float sx = wave_sum(acc.x), sy = wave_sum(acc.y), sz = wave_sum(acc.z);
				if (lane_id() == 0) {
					Ls[0][k] = sx;
					Ls[1][k] = sy;
					Ls[2][k] = sz;
				}
			}
			lds_sync();
		} else {
			/* several points share a packet: each point's samples fill consecutive slots of B
			 * (power of two) lanes, B = slot_b; a point may straddle packets */
			if (SC) { /* each lane its own point's cone_mask_lane */
				uint32_t m = 0u;
				if (uni(ks.num_cull) && uni(ks.cull_slots)) {
					const float4 *my = unip(ks.sp) + (size_t)my_sid * SPREC;
					const float4 q0 = ldg4(my, 0), q4 = ldg4(my, 64);
					const bool far = (__float_as_uint(q4.x) & RTX_SP_FAR) != 0;
					m = cone_mask_lane(ks, mk3(q0.x, q0.y, q0.z), own && !far);
				}
				clr[lane_id()] = (uint8_t)m;
				lds_sync();
			}
			uint32_t kp = 0; /* this lane's point in the previous packet (its slots only move forward) */
			for (uint32_t base = 0;;) {
				reread_barrier();
				const uint32_t tot = uni(off[WAVE]), slot_b = uni(ks.slot_b), slot_lg = uni(ks.slot_lg);
				if (base >= tot)
					break;
				const uint32_t slot = base + (lane_id() >> slot_lg);
				uint32_t k = 0;
				if (slot < tot) { /* the slot's point (rtx_wave.h owner_of) from the previous packet's: a step or two, not six */
					k = kp;
					while (off[k + 1] <= slot)
						k++;
					kp = k;
				}
				const uint32_t idx = ((slot - off[k]) << slot_lg) + (lane_id() & (slot_b - 1));
				const bool act = slot < tot && idx < nls[k];
				const f3 contribution = light_sample<COUNT, WALK, false, LA, SC>(ks, nullptr, sid[k], idx, act, sc, top_q, top_e, stk,
											 t8, wv, nullptr,
											 SC ? (uint32_t)clr[k] : 0u);
				/* per-shade-point sums.  Each slot's B lanes reduce in a fixed butterfly (masks B/2 .. 1),
				 * then the slot sums are added to their point's total one slot at a time in slot order, so a
				 * point whose slots straddle packets gets the same sum whatever its neighbours (with one slot
				 * per point this is the 64-lane butterfly over zeros and one slot it replaced, bit for bit) */
				const uint32_t t2 = uni(off[WAVE]), sb = uni(ks.slot_b), lg = uni(ks.slot_lg), spp = WAVE >> lg;
				f3 v = act ? contribution : mk3(0.f, 0.f, 0.f);
				if (sb > 16) {
					v.x += lane_xor_f<16>(v.x);
					v.y += lane_xor_f<16>(v.y);
					v.z += lane_xor_f<16>(v.z);
				}
				if (sb > 8) {
					v.x += lane_xor_f<8>(v.x);
					v.y += lane_xor_f<8>(v.y);
					v.z += lane_xor_f<8>(v.z);
				}
				if (sb > 4) {
					v.x += lane_xor_f<4>(v.x);
					v.y += lane_xor_f<4>(v.y);
					v.z += lane_xor_f<4>(v.z);
				}
				if (sb > 2) {
					v.x += lane_xor_f<2>(v.x);
					v.y += lane_xor_f<2>(v.y);
					v.z += lane_xor_f<2>(v.z);
				}
				if (sb > 1) {
					v.x += lane_xor_f<1>(v.x);
					v.y += lane_xor_f<1>(v.y);
					v.z += lane_xor_f<1>(v.z);
				}
				const uint32_t ns = min(t2 - base, spp);
				if (WALK == WALK_W8) {
					/* the same fold with the slot sums handed over in LDS instead of v_readlane (four
					 * single-issue reads and three adds on SGPR operands per slot): each slot's first
					 * lane stores (sum, point) in the wave's lane-stack area, empty between walks, and
					 * lane 0 folds them in slot order (an LDS read, a compare and three adds per slot) */
					float4 *sl = (float4 *)&wstk[wv][0][0];
					if (!(lane_id() & (sb - 1)) && (lane_id() >> lg) < ns)
						sl[lane_id() >> lg] = make_float4(v.x, v.y, v.z, __uint_as_float(k));
					lds_sync();
					if (lane_id() == 0) {
						uint32_t kc = __float_as_uint(sl[0].w);
						float rx = Ls[0][kc], ry = Ls[1][kc], rz = Ls[2][kc];
						for (uint32_t j = 0; j < ns; j++) {
							const float4 q = sl[j];
							const uint32_t kj = __float_as_uint(q.w);
							if (kj != kc) {
								Ls[0][kc] = rx;
								Ls[1][kc] = ry;
								Ls[2][kc] = rz;
								kc = kj;
								rx = Ls[0][kc];
								ry = Ls[1][kc];
								rz = Ls[2][kc];
							}
							rx += q.x;
							ry += q.y;
							rz += q.z;
						}
						Ls[0][kc] = rx;
						Ls[1][kc] = ry;
						Ls[2][kc] = rz;
					}
					lds_sync();
					base += spp;
					continue;
				}
				/* the BVH2 instances (no lane-stack area to hand the sums over in): the fold by v_readlane */
				uint32_t kc = readlane(k, 0);
				float rx = Ls[0][kc], ry = Ls[1][kc], rz = Ls[2][kc];
				for (uint32_t j = 0; j < ns; j++) {
					const uint32_t kj = readlane(k, j * sb);
					if (kj != kc) {
						if (lane_id() == 0) {
							Ls[0][kc] = rx;
							Ls[1][kc] = ry;
							Ls[2][kc] = rz;
						}
						kc = kj;
						rx = Ls[0][kc];
						ry = Ls[1][kc];
						rz = Ls[2][kc];
					}
					rx += readlanef(v.x, j * sb);
					ry += readlanef(v.y, j * sb);
					rz += readlanef(v.z, j * sb);
				}
				if (lane_id() == 0) {
					Ls[0][kc] = rx;
					Ls[1][kc] = ry;
					Ls[2][kc] = rz;
				}
				lds_sync();
				base += spp;
			}
		}
		reread_barrier();
		if (lane_id() < cnt) {
			const uint32_t me = sid[lane_id()]; /* re-read: my_sid need not stay live across the walks */
			const float4 *my = unip(ks.sp) + (size_t)me * SPREC;
			const float4 q0 = my[0], q1 = my[1], q2 = my[2], q5 = my[5];
			const f3 w = mk3(q0.w, q1.w, q2.w);
			const f3 c = mul3v(w, mk3(Ls[0][lane_id()], Ls[1][lane_id()], Ls[2][lane_id()]));
			unip(ks.contrib)[me] = make_float4(c.x, c.y, c.z, q5.x);
		}
		rays_total += uni(wave_sum_u(lane_id() < cnt ? nls[lane_id()] : 0u));
	}
	if (lane_id() == 0) {
		unsigned long long *ctr = unip(ks.ctr);
		atomicAdd(&ctr[RTX_C_SHADOW], rays_total);
		if (COUNT) {
			atomicAdd(&ctr[RTX_C_SBOXES], sc.boxes);
			atomicAdd(&ctr[RTX_C_SGBOXES], sc.gboxes);
			atomicAdd(&ctr[RTX_C_STRIS], sc.tris);
			atomicAdd(&ctr[RTX_C_SSPHERES], sc.sph);
			atomicAdd(&ctr[RTX_C_SPLANES], sc.pln);
			atomicAdd(&ctr[RTX_C_SSTEPS], sc.steps);
			atomicAdd(&ctr[RTX_C_SWALKS], sc.walks);
			atomicAdd(&ctr[RTX_C_SLEAFR], sc.lrounds);
			atomicAdd(&ctr[RTX_C_SUNIF], sc.unif);
			atomicAdd(&ctr[RTX_C_FARS], sc.far);
			atomicAdd(&ctr[RTX_C_SSPILL], sc.spills);
			atomicAdd(&ctr[RTX_C_SCLEAR], sc.clear);
			atomicAdd(&ctr[RTX_C_SPSKIP], sc.pskip);
			atomicAdd(&ctr[RTX_C_SLSKIP], sc.lskip);
			atomicAdd(&ctr[RTX_C_SPCLEAR], sc.pclear);
			atomicAdd(&ctr[RTX_C_SDARK], sc.dark);
			atomicAdd(&ctr[RTX_C_SDARKPK], sc.dpack);
			atomicAdd(&ctr[RTX_C_SORDPT], sc.ordpt);
			atomicAdd(&ctr[RTX_C_SORDRAY], sc.ordray);
		}
	}
}

/* ------------------------------------------------------------------------ */
/* the rest of this translation unit (one object: the device functions above are shared) */
/* ------------------------------------------------------------------------ */
/* Nothing below is compiled into a k_shadow instance.  Each part relies on the code above and on the
 * parts before it, and is included here only. */
#include "rtx_shadow_premask.h"   /* k_point_masks: the per-point masks ahead of k_shadow */
#include "rtx_shadow_clearlane.h" /* k_clear_count / _scan / _scatter, k_shadow_clear: the all-clear points, one per lane */
#include "rtx_shadow_rays.h"      /* k_shadow_rays: shadow_query on a caller's rays */
#include "rtx_shadow_kat.h"       /* the known-answer-test kernels */
#include "rtx_shadow_launch.h"    /* k_w8_fill and the host launch code (rtx_launch.h) */
