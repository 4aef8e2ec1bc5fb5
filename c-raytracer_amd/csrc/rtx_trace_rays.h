/*
 * A part of rtx_trace.hip's translation unit, included there once and not self-contained: it uses that file's
 * trace_closest, hit_info, TraceCount and RTX_PRIMARY_DIR, the walks and hit records k_trace runs.
 */
/* ------------------------------------------------------------------------ */
/* k_rays: closest / any hit of a caller's ray batch (rtx_trace_rays*)      */
/* ------------------------------------------------------------------------ */
/* Persistent waves, one per workgroup like k_trace (the closest walk's lane stack is per
 * workgroup: LDS, then DScene.ostk by blockIdx.x / gridDim.x, which the host sizes for THIS
 * grid), taking 64-ray packets from atomic counters, `grab` consecutive packets at a time.  A
 * walk of a packet is short next to a tile's ray trees, and one counter serves about 80 M
 * device-wide atomics a second (33 M rays took 6.5 ms whatever they hit; 1.2 ms with eight), so the packets are dealt
 * over `queues` counters on lines of their own: wave b takes from queue b % queues, which owns the
 * grabs j = queue + k * queues (an equal share, interleaved, for an equal share of the waves).  A ray is two float4 (rtx_ray: origin, tmax |
 * dir, pad), a hit two float4 (rtx_hit: t, object, material, outside | n, pad).  With perm (the
 * RTX_RAYS_REORDER sort's index list) lane i of a packet traces ray perm[i] and writes hit
 * perm[i]: a ray's result never depends on the rays it shares a wave with, as the closest t is
 * a minimum over accepted hits and the box tests only cull. */
template <bool COUNT, bool ANY>
__global__ __launch_bounds__(WAVE, RTX_TRACE_OCC) void k_rays(DScene S, const float4 *__restrict__ rays,
							      float4 *__restrict__ hits, const uint32_t *__restrict__ perm,
							      uint32_t n, uint32_t queues, uint32_t grab,
							      unsigned long long *__restrict__ ctr)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
	uint32_t *stk = (uint32_t *)lds_raw;
	const uint32_t packets = (uint32_t)(((uint64_t)n + WAVE - 1) / WAVE);
	TraceCount tc = { 0, 0, 0, 0, 0 };
	u64 n_hits = 0;
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
		const bool act = i < n;
		size_t idx = 0;
		float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, 1.f, 0.f);
		if (act) {
			idx = perm ? (size_t)perm[i] : (size_t)i;
			r0 = rays[2 * idx];
			r1 = rays[2 * idx + 1];
		}
		const f3 o = mk3(r0.x, r0.y, r0.z), d = mk3(r1.x, r1.y, r1.z);
		float t = r0.w < FLT_MAX ? r0.w : FLT_MAX; /* tmax: INFINITY (or NaN) = the renderer's unbounded ray */
		uint32_t hid;
		lds_sync();
		trace_closest<COUNT, ANY, true>(S, stk, act, o, d, RTX_NONE, t, hid, tc);
		const bool hit = act && hid != RTX_NONE;
		float4 h0 = make_float4(0.f, __uint_as_float(0xFFFFFFFFu), __uint_as_float(0xFFFFFFFFu), 0.f);
		float4 h1 = make_float4(0.f, 0.f, 0.f, 0.f);
		if (hit) {
			const HitInfo h = hit_info(S, hid, o, d, t);
			h0 = make_float4(t, __uint_as_float(h.obj), __uint_as_float(h.mat), __uint_as_float(h.outside ? 1u : 0u));
			h1 = make_float4(h.n.x, h.n.y, h.n.z, 0.f);
		}
		if (act) {
			hits[2 * idx] = h0;
			hits[2 * idx + 1] = h1;
		}
		n_hits += popc64(ballot(hit));
	}
	if (COUNT) {
		u64 a = tc.nodes, b = tc.tris, c = tc.sph, d2 = tc.pln, f = tc.far;
#pragma unroll
		for (int o2 = 32; o2 > 0; o2 >>= 1) {
			a += __shfl_xor(a, o2, WAVE);
			b += __shfl_xor(b, o2, WAVE);
			c += __shfl_xor(c, o2, WAVE);
			d2 += __shfl_xor(d2, o2, WAVE);
			f += __shfl_xor(f, o2, WAVE);
		}
		if (lane_id() == 0) {
			atomicAdd(&ctr[RTX_RQ_NODES], a);
			atomicAdd(&ctr[RTX_RQ_TRIS], b);
			atomicAdd(&ctr[RTX_RQ_SPHERES], c);
			atomicAdd(&ctr[RTX_RQ_PLANES], d2);
			atomicAdd(&ctr[RTX_RQ_FAR], f);
		}
	}
	if (lane_id() == 0 && n_hits)
		atomicAdd(&ctr[RTX_RQ_HITS], n_hits);
}

/* the W*H primary rays of a frame as rtx_ray records, row-major, tmax = INFINITY: k_trace's own rays */
__global__ __launch_bounds__(256) void k_frame_rays(DFrame F, float4 *__restrict__ rays)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (i >= (uint64_t)F.width * F.height)
		return;
	const uint32_t px = (uint32_t)(i % F.width), py = (uint32_t)(i / F.width);
	const f3 o = ld3(F.origin);
	f3 d;
	RTX_PRIMARY_DIR(F, px, py, o, d);
	rays[2 * i] = make_float4(o.x, o.y, o.z, INFINITY);
	rays[2 * i + 1] = make_float4(d.x, d.y, d.z, 0.f);
}
