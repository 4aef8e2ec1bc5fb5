/*
 * Closest-point queries (include/rtx.h rtx_closest_points*) for gfx950.
 *
 *  k_nearest      (persistent, one wave per workgroup; 64-point packets from the ray queries' device
 *                 queues) the nearest surface point of the uploaded scene to each point of a batch:
 *                 the planes one by one, the emitters the 8-wide tree leaves out one by one, then a
 *                 best-first search of the 8-wide compressed BVH (rtx_device.h DW8), or of the float
 *                 BVH2 (DNode) on the scenes that have no 8-wide tree.
 *  k_nearest_kat  the three distance functions (rtx_nearest_math.h) on caller-given (object, point)
 *                 pairs; k_nearest_grid the distances of every object to every point.
 *
 * The distance functions are rtx_nearest_math.h's, the very text the host's rtx_closest_point_object
 * compiles.  A point's answer is a minimum over the objects the search did not prune, and the search
 * prunes a box only where a lower bound on the distance to everything inside it, deflated for every
 * rounding on the way (near_deflate), exceeds the best distance found: the answer never depends on
 * the batch, its order or the lanes a point shares a wave with.
 */
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_lane_stack.h"
#include "rtx_launch.h"
#include "rtx_math.h"
#include "rtx_nearest_math.h"
#include "rtx_w8.h"
#include "rtx_wave.h"

struct NearCount {
	uint32_t nodes, tris, sph, pln;
};

/* a point's best answer so far */
struct NearBest {
	float dist; /* the caller's max_dist at first: answers need dist < it, strictly */
	float cp[3];
	uint32_t obj, mat;
};

/*
 * The deflation of a box's lower bound (DESIGN 7.11 has the derivation).  With u = 2^-24 m and m the
 * largest coordinate magnitude among the point (world) and the bounded objects' world box:
 *   the point's transform into the trees' frame   <= 24 u per axis  (the subtraction of c, three
 *        products and two sums of magnitudes <= 6 m)
 *   its map onto the tree's 16-bit grid            <= 24 u per axis  (in frame units)
 *   the distance function's own rounding           <= 25 u           (a candidate point off the
 *        object by <= 8 u per axis, the squared sum and its root)
 * together under 2^7 u as vectors; the bound subtracts 2^8 u = 2^-16 m, and 2^-20 of itself for its
 * own arithmetic (a dozen roundings, <= 2^-20 relative).  The boxes themselves contain the objects
 * in exact arithmetic: the leaf boxes are formed in double and padded (rtx_frame.cpp), the 16-bit
 * planes are rounded outward by a whole grid step (rtx_quant.h), the 8-bit planes outward from
 * those, and the grid coordinates of the planes are integers below 2^24, exact in float32.  The
 * slack scales with the point's own magnitude, so it holds for far points (60 or 2000 scene radii)
 * as it does for near ones: there is no separate far path.
 */
__device__ __forceinline__ float near_deflate(float lb, float slack) { return lb - (lb * 0x1p-20f + slack); }

/* one bounded primitive, as the first 48 bytes of its 64-byte record (DPrim / a leaf entry of the
 * 8-wide tree): a = p0 | centre, b = e1 | (r, ., .), object index; c = e2, meta */
template <bool COUNT>
__device__ __forceinline__ void near_prim(float4 a, float4 b, float4 c, const float (&P)[3], NearBest &B, NearCount &nc)
{
	float dist, cp[3];
	const float p0[3] = { a.x, a.y, a.z };
	const uint32_t meta = __float_as_uint(c.w);
	if ((meta >> 24) == RTX_SPHERE) {
		if (COUNT)
			nc.sph++;
		rtx_nm_sphere(p0, b.x, P, &dist, cp);
	} else {
		if (COUNT)
			nc.tris++;
		const float e1[3] = { b.x, b.y, b.z }, e2[3] = { c.x, c.y, c.z };
		rtx_nm_triangle(p0, e1, e2, P, &dist, cp);
	}
	if (dist < B.dist) {
		B.dist = dist;
		B.cp[0] = cp[0];
		B.cp[1] = cp[1];
		B.cp[2] = cp[2];
		B.obj = __float_as_uint(b.w);
		B.mat = meta & RTX_META_MAT;
	}
}

/* the distance from p to the interval [lo, hi] on one axis (0 inside) */
__device__ __forceinline__ float axis_gap(float p, float lo, float hi) { return fmaxf(fmaxf(lo - p, p - hi), 0.f); }

/* child C of an 8-wide node: the lower bound on the distance from the point to its box.  pq: the
 * point on the tree's 16-bit grid; o: the node's origin and st its per-axis step 2^e, both in grid
 * units (integers, exact); iq: frame units per grid unit, per axis (the grid's scales differ, so the
 * gaps are taken to frame units axis by axis before they are squared). */
template <int C> __device__ __forceinline__ float near_child(const uint32_t (&w)[16], f3 pq, f3 o, f3 st, f3 iq)
{
	constexpr int W = C >> 2, B = C & 3;
	const float gx = axis_gap(pq.x, fmaf(ubyte<B>(w[4 + W]), st.x, o.x), fmaf(ubyte<B>(w[6 + W]), st.x, o.x)) * iq.x;
	const float gy = axis_gap(pq.y, fmaf(ubyte<B>(w[8 + W]), st.y, o.y), fmaf(ubyte<B>(w[10 + W]), st.y, o.y)) * iq.y;
	const float gz = axis_gap(pq.z, fmaf(ubyte<B>(w[12 + W]), st.z, o.z), fmaf(ubyte<B>(w[14 + W]), st.z, o.z)) * iq.z;
	return sqrtf(gx * gx + gy * gy + gz * gz);
}

/* the lane stack, sized as k_rays sizes its own (rtx_lane_stack.h), with the capacity check: DScene.stack_size
 * entries in all */
typedef LaneStack<true> NearStack;

/*
 * Best-first search of the 8-wide tree.  A node visit forms the eight bounds, tests the leaf slots
 * whose bound does not exceed the best distance (a leaf entry is the primitive's record: one
 * primitive per slot), then takes the inner children whose bound still does not exceed it: the
 * nearest one next, the others kept as one group word (base << 8 | slot mask), older groups on the
 * lane stack: one entry per level, as in the closest-hit walk.  A kept child carries no bound: when
 * its turn comes its node is read and its own children are bounded against the best distance of
 * that moment, which drops everything the stale entry no longer needs (at the price of one node
 * read), so nothing has to be stored beside the group word.
 */
template <bool COUNT>
__device__ __forceinline__ void near_walk8(const DScene &S, NearStack &stk, const float (&P)[3], f3 pb, float slack, NearBest &B,
					   NearCount &nc)
{
	const f3 qs = ld3(S.w8qs), qo = ld3(S.w8qo);
	const f3 pq = mk3((pb.x - qo.x) * qs.x, (pb.y - qo.y) * qs.y, (pb.z - qo.z) * qs.z);
	const f3 iq = mk3(1.f / qs.x, 1.f / qs.y, 1.f / qs.z);
	uint32_t node = 0, grp = 0;
	while (node != RTX_NONE) {
		uint32_t w[16];
		const DW8 *N = S.w8 + (size_t)node;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const uint4 x = ldg4u((const uint32_t *)N + 4 * k);
			w[4 * k] = x.x;
			w[4 * k + 1] = x.y;
			w[4 * k + 2] = x.z;
			w[4 * k + 3] = x.w;
		}
		if (COUNT)
			nc.nodes++;
		const f3 o = mk3((float)(w[0] & 0xFFFFu), (float)(w[0] >> 16), (float)(w[1] & 0xFFFFu));
		const f3 st = mk3((float)(1u << ((w[1] >> 16) & 15u)), (float)(1u << ((w[1] >> 20) & 15u)),
				  (float)(1u << ((w[1] >> 24) & 15u)));
		const uint32_t base = w[2] >> 8, imask = w[2] & 0xFFu, vmask = w[3] & 0xFFu;
		float lb[8];
		lb[0] = near_deflate(near_child<0>(w, pq, o, st, iq), slack);
		lb[1] = near_deflate(near_child<1>(w, pq, o, st, iq), slack);
		lb[2] = near_deflate(near_child<2>(w, pq, o, st, iq), slack);
		lb[3] = near_deflate(near_child<3>(w, pq, o, st, iq), slack);
		lb[4] = near_deflate(near_child<4>(w, pq, o, st, iq), slack);
		lb[5] = near_deflate(near_child<5>(w, pq, o, st, iq), slack);
		lb[6] = near_deflate(near_child<6>(w, pq, o, st, iq), slack);
		lb[7] = near_deflate(near_child<7>(w, pq, o, st, iq), slack);
		/* leaf slots, in slot order; each bound is looked at again with the best distance of its turn */
		uint32_t lm = 0;
#pragma unroll
		for (int k = 0; k < 8; k++)
			lm |= (((vmask & ~imask) >> k) & 1u) && !(lb[k] > B.dist) ? 1u << k : 0u;
		while (lm) {
			const uint32_t p = __builtin_ctz(lm);
			lm &= lm - 1;
			float l = lb[0];
#pragma unroll
			for (int k = 1; k < 8; k++)
				l = p == (uint32_t)k ? lb[k] : l;
			if (l > B.dist)
				continue;
			const char *pr = (const char *)(S.w8 + base + p);
			near_prim<COUNT>(ldg4(pr, 0), ldg4(pr, 16), ldg4(pr, 32), P, B, nc);
		}
		/* inner children that may still hold something nearer: the nearest next, the rest kept */
		uint32_t im = 0, nearp = 8;
		float nb = INFINITY;
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const bool in = ((imask & vmask) >> k) & 1u && !(lb[k] > B.dist);
			im |= in ? 1u << k : 0u;
			const bool nr = in && (nearp == 8 || lb[k] < nb);
			nearp = nr ? (uint32_t)k : nearp;
			nb = nr ? lb[k] : nb;
		}
		if (im) {
			node = base + nearp;
			im &= ~(1u << nearp);
			if (im) {
				if (grp)
					stk.push(grp);
				grp = (base << 8) | im;
			}
		} else if (grp) {
			node = (grp >> 8) + (uint32_t)__builtin_ctz(grp & 0xFFu);
			grp &= grp - 1;
			if (!(grp & 0xFFu))
				grp = stk.sp ? stk.pop() : 0u;
		} else {
			node = RTX_NONE;
		}
	}
}

/* the distance from pb to a float box of the BVH2 (the trees' frame), deflated */
__device__ __forceinline__ float near_box(f3 pb, float lx, float hx, float ly, float hy, float lz, float hz, float slack)
{
	const float gx = axis_gap(pb.x, lx, hx), gy = axis_gap(pb.y, ly, hy), gz = axis_gap(pb.z, lz, hz);
	return near_deflate(sqrtf(gx * gx + gy * gy + gz * gz), slack);
}

/* The same search on the float BVH2, for the tiny scenes that have no 8-wide tree: the nearer child
 * first, the other one on the stack (its node is bounded again when it is popped). */
template <bool COUNT>
__device__ __forceinline__ void near_walk2(const DScene &S, NearStack &stk, const float (&P)[3], f3 pb, float slack, NearBest &B,
					   NearCount &nc)
{
	uint32_t ref = S.root_ref;
	for (;;) {
		if (ref & RTX_REF_LEAF) {
			const uint32_t first = (ref & RTX_REF_OFF) / (uint32_t)sizeof(DNode) - S.num_nodes, cnt = (ref & RTX_REF_CNT) + 1;
			for (uint32_t k = 0; k < cnt && first + k < S.num_prims; k++) {
				const float4 *pr = (const float4 *)(S.prims + first + k);
				near_prim<COUNT>(pr[0], pr[1], pr[2], P, B, nc);
			}
			if (!stk.sp)
				break;
			ref = stk.pop();
		} else {
			const float4 *nd = (const float4 *)((const char *)S.nodes + (ref & RTX_REF_OFF));
			const float4 n0 = nd[0], n1 = nd[1], n2 = nd[2];
			const uint4 n3 = *(const uint4 *)(nd + 3);
			if (COUNT)
				nc.nodes++;
			const float l0 = near_box(pb, n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, slack);
			const float l1 = near_box(pb, n1.z, n1.w, n2.x, n2.y, n2.z, n2.w, slack);
			const bool h0 = !(l0 > B.dist), h1 = !(l1 > B.dist);
			if (h0 && h1) {
				const bool l_first = l0 < l1;
				stk.push(l_first ? n3.y : n3.x);
				ref = l_first ? n3.x : n3.y;
			} else if (h0) {
				ref = n3.x;
			} else if (h1) {
				ref = n3.y;
			} else {
				if (!stk.sp)
					break;
				ref = stk.pop();
			}
		}
	}
}

/* Persistent waves and packet queues as k_rays (rtx_trace_rays.h): wave b takes `grab` consecutive
 * 64-point packets at a time from queue b % queues.  A query is one float4 (rtx_point_query: p,
 * max_dist), a result two (rtx_closest: point, dist | object, material, 0, 0).  With perm (the
 * RTX_CLOSEST_REORDER sort's index list) lane i of a packet answers query perm[i]. */
template <bool COUNT>
__global__ __launch_bounds__(WAVE) void k_nearest(DScene S, const float4 *__restrict__ queries, float4 *__restrict__ results,
						  const uint32_t *__restrict__ perm, uint32_t n, uint32_t queues, uint32_t grab,
						  float wmag, int bounded_only, unsigned long long *__restrict__ ctr)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	const uint32_t packets = (uint32_t)(((uint64_t)n + WAVE - 1) / WAVE);
	NearCount nc = { 0, 0, 0, 0 };
	u64 n_found = 0, n_far = 0;
	const uint32_t queue = blockIdx.x % queues;
	unsigned long long *head = ctr + RTX_RQ_HEADS + (size_t)queue * RTX_RQ_HEAD_STRIDE;
	uint64_t pk = 0, pk_end = 0;
	for (;;) {
		if (pk == pk_end) {
			uint32_t k = 0;
			if (lane_id() == 0)
				k = (uint32_t)atomicAdd(head, 1ull);
			k = uni(__shfl(k, 0, WAVE));
			pk = ((uint64_t)k * queues + queue) * grab;
			if (pk >= packets)
				break;
			pk_end = pk + grab < packets ? pk + grab : packets;
		}
		const uint64_t i = pk++ * WAVE + lane_id();
		bool act = i < n;
		size_t idx = 0;
		float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
		if (act) {
			idx = perm ? (size_t)perm[i] : (size_t)i;
			q = queries[idx];
		}
		const float P[3] = { q.x, q.y, q.z };
		NearBest B;
		B.dist = (q.w != q.w || q.w > FLT_MAX) ? INFINITY : q.w; /* NaN or INFINITY: unbounded */
		B.cp[0] = B.cp[1] = B.cp[2] = 0.f;
		B.obj = B.mat = RTX_NONE;
		/* a point with a NaN or infinite coordinate, or a max_dist nothing lies below: a miss */
		act = act && fabsf(q.x) <= FLT_MAX && fabsf(q.y) <= FLT_MAX && fabsf(q.z) <= FLT_MAX && B.dist > 0.f;
		if (act && !bounded_only) {
			for (uint32_t k = 0; k < S.num_planes; k++) {
				const DPlane &pl = S.planes[k];
				const float nn[3] = { pl.n[0], pl.n[1], pl.n[2] };
				float dist, cp[3];
				if (COUNT)
					nc.pln++;
				rtx_nm_plane(nn, pl.d, P, &dist, cp);
				if (dist < B.dist) {
					B.dist = dist;
					B.cp[0] = cp[0];
					B.cp[1] = cp[1];
					B.cp[2] = cp[2];
					B.obj = pl.obj;
					B.mat = pl.mat;
				}
			}
		}
		if (act && S.root_ref != RTX_EMPTY_REF) {
			/* the emitters the 8-wide tree leaves out, by their primitive records */
			if (S.w8 && S.w8noemit) {
				for (uint32_t k = 0; k < S.num_emitters; k++) {
					const uint32_t pi = S.emitters[k].prim;
					if (pi >= S.num_prims)
						continue;
					const float4 *pr = (const float4 *)(S.prims + pi);
					near_prim<COUNT>(pr[0], pr[1], pr[2], P, B, nc);
				}
			}
			/* the point in the trees' frame (a rotation and a translation: distances carry over) */
			const f3 pw = mk3(q.x, q.y, q.z);
			const f3 pb = S.tf.rotated ? tf_point(S.tf.r, S.tf.c, pw) : pw;
			if (tf_far(pb, S.tf.cf, S.tf.rad))
				n_far++;
			const float mag = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), wmag));
			const float slack = mag * 0x1p-16f;
			NearStack stk = lane_stack<true>(S, lds_raw);
			if (S.w8)
				near_walk8<COUNT>(S, stk, P, pb, slack, B, nc);
			else
				near_walk2<COUNT>(S, stk, P, pb, slack, B, nc);
		}
		if (i < n) {
			const bool found = B.obj != RTX_NONE;
			results[2 * idx] = found ? make_float4(B.cp[0], B.cp[1], B.cp[2], B.dist) : make_float4(0.f, 0.f, 0.f, INFINITY);
			results[2 * idx + 1] = make_float4(__uint_as_float(B.obj), __uint_as_float(B.mat), 0.f, 0.f);
			n_found += found ? 1 : 0;
		}
	}
	u64 f = n_found, g = n_far, a = nc.nodes, b = nc.tris, c = nc.sph, d = nc.pln;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		f += __shfl_xor(f, o, WAVE);
		g += __shfl_xor(g, o, WAVE);
		if (COUNT) {
			a += __shfl_xor(a, o, WAVE);
			b += __shfl_xor(b, o, WAVE);
			c += __shfl_xor(c, o, WAVE);
			d += __shfl_xor(d, o, WAVE);
		}
	}
	if (lane_id() == 0) {
		if (f)
			atomicAdd(&ctr[RTX_NQ_FOUND], f);
		if (g)
			atomicAdd(&ctr[RTX_NQ_FAR], g);
		if (COUNT) {
			atomicAdd(&ctr[RTX_NQ_NODES], a);
			atomicAdd(&ctr[RTX_NQ_TRIS], b);
			atomicAdd(&ctr[RTX_NQ_SPHERES], c);
			atomicAdd(&ctr[RTX_NQ_PLANES], d);
		}
	}
}

/* ------------------------------------------------------------------------ */
/* known answers: the distance functions alone, no search                   */
/* ------------------------------------------------------------------------ */
__device__ __forceinline__ void near_object(const rtx_object &o, const float (&P)[3], float *dist, float cp[3])
{
	if (o.type == RTX_SPHERE) {
		rtx_nm_sphere(o.p0, o.radius, P, dist, cp);
	} else if (o.type == RTX_TRIANGLE) {
		rtx_nm_triangle(o.p0, o.e1, o.e2, P, dist, cp);
	} else {
		rtx_nm_plane(o.n, o.d, P, dist, cp);
	}
}

/* pair i: object index[i] (i itself without a list) and point i; out: dist, cp */
__global__ __launch_bounds__(256) void k_nearest_kat(const rtx_object *__restrict__ objs, const uint32_t *__restrict__ index,
						     const float *__restrict__ pts, uint64_t n, float4 *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const float P[3] = { pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] };
	float dist, cp[3];
	near_object(objs[index ? index[i] : i], P, &dist, cp);
	out[i] = make_float4(dist, cp[0], cp[1], cp[2]);
}

/* dist[p * n_obj + o]: every object to every point */
__global__ __launch_bounds__(256) void k_nearest_grid(const rtx_object *__restrict__ objs, uint32_t n_obj,
						      const float *__restrict__ pts, uint32_t n_pts, float *__restrict__ dist)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= (uint64_t)n_obj * n_pts)
		return;
	const uint32_t p = (uint32_t)(i / n_obj), o = (uint32_t)(i % n_obj);
	const float P[3] = { pts[3 * (size_t)p], pts[3 * (size_t)p + 1], pts[3 * (size_t)p + 2] };
	float d, cp[3];
	near_object(objs[o], P, &d, cp);
	dist[i] = d;
}

/* ------------------------------------------------------------------------ */
/* host side                                                                */
/* ------------------------------------------------------------------------ */
/* k_nearest keeps only the search's LDS lane-stack entries */
extern "C" size_t rtx_nearest_lds_bytes(uint32_t stack_size)
{
	const size_t lstk = stack_size < RTX_TRACE_LSTK ? stack_size : RTX_TRACE_LSTK;
	return lstk * WAVE * 4;
}

extern "C" hipError_t rtx_nearest_occupancy(uint32_t stack_size, int *blocks_per_cu)
{
	return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_nearest<false>, WAVE, rtx_nearest_lds_bytes(stack_size));
}

/* S->ostk must hold waves * 64 * (stack_size - RTX_TRACE_LSTK) entries: this launch's own grid.
 * wmag: the largest coordinate magnitude of the bounded objects' world box. */
extern "C" hipError_t rtx_launch_nearest(const DScene *S, const float4 *queries, float4 *results, const uint32_t *perm, uint32_t n,
					 uint32_t queues, uint32_t grab, float wmag, int bounded_only, unsigned long long *ctr,
					 uint32_t waves, int count, hipStream_t stream)
{
	const size_t lds = rtx_nearest_lds_bytes(S->stack_size);
	if (count)
		hipLaunchKernelGGL(k_nearest<true>, dim3(waves), dim3(WAVE), lds, stream, *S, queries, results, perm, n, queues, grab,
				   wmag, bounded_only, ctr);
	else
		hipLaunchKernelGGL(k_nearest<false>, dim3(waves), dim3(WAVE), lds, stream, *S, queries, results, perm, n, queues, grab,
				   wmag, bounded_only, ctr);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_nearest_kat(const rtx_object *objs, const uint32_t *index, const float *pts, uint64_t n,
					     float4 *out, hipStream_t stream)
{
	if (!n)
		return hipSuccess;
	hipLaunchKernelGGL(k_nearest_kat, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, objs, index, pts, n, out);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_nearest_grid(const rtx_object *objs, uint32_t n_obj, const float *pts, uint32_t n_pts,
					      float *dist, hipStream_t stream)
{
	const uint64_t n = (uint64_t)n_obj * n_pts;
	if (!n)
		return hipSuccess;
	hipLaunchKernelGGL(k_nearest_grid, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, objs, n_obj, pts, n_pts, dist);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded now (rtx_open) rather than at the
 * first query */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_load_nearest(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_nearest<false>);
}
