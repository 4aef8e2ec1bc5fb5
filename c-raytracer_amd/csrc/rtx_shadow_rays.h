/*
 * A part of rtx_shadow.hip's translation unit, included there once and not self-contained: it uses that
 * file's KShadow, QBvh / make_qbvh, ShadowCount and shadow_query, the query k_shadow runs.
 *
 * k_shadow_rays: shadow_query on a caller's rays (rtx_trace_shadow_rays), so tests can hold the walk to
 * brute force ray by ray.
 */
/* One 64-ray packet per wave and turn, ray i in lane i % 64 of packet i / 64: k_shadow's workgroup
 * (block size, LDS copies of the trees' top levels, lane stacks, argument block) around one call of
 * shadow_query per packet, every plane and every listed record tested, nothing culled.  A workgroup
 * takes packets blockIdx.x * RTX_SH_NW + wave, then strides by the grid, so the grid never exceeds
 * the one the lane-stack spill area was sized for.  Rays are two float4 (origin, dist | direction,
 * light object), results one (transmittance, blocked). */
template <bool COUNT, int WALK, bool LA>
__global__ __launch_bounds__(WAVE *RTX_SH_NW) void k_shadow_rays(KShadow ka, const float4 *__restrict__ rays, float4 *__restrict__ res,
								 uint32_t n, unsigned long long *ctr)
{
	constexpr bool TOP = WALK == WALK_BVH2;
	__shared__ uint4 top_q[TOP ? RTX_TOP_MAX : 1];
	__shared__ uint32_t top_e[TOP ? RTX_TOP_MAX : 1];
	__shared__ __attribute__((aligned(16))) uint32_t wstk[RTX_SH_NW][WALK == WALK_W8 ? RTX_W8_STACK + RTX_W8_TQ : 1][WAVE];
	__shared__ KShadow ks_s;
	__shared__ uint4 t8[WALK == WALK_W8 ? RTX_W8_TOP_MAX * 4 : 1];
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
	lds_u32 *stk = (lds_u32 *)&wstk[wv][0][LA ? 0u : lane_id()];
	ShadowCount sc = {};
	u64 n_live = 0, n_blocked = 0;
	const uint32_t packets = (n + WAVE - 1) / WAVE;
	for (uint32_t pk = blockIdx.x * RTX_SH_NW + wv; pk < packets; pk += gridDim.x * RTX_SH_NW) {
		reread_barrier();
		const size_t i = (size_t)pk * WAVE + lane_id();
		const bool in = i < n;
		float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 0.f, 1.f, __uint_as_float(RTX_NONE));
		if (in) {
			r0 = rays[2 * i];
			r1 = rays[2 * i + 1];
		}
		/* an idle lane: dist <= 0 or NaN, or a NaN direction component */
		const bool act = in && r0.w > 0.f && r1.x == r1.x && r1.y == r1.y && r1.z == r1.z;
		const f3 o = act ? mk3(r0.x, r0.y, r0.z) : mk3(0.f, 0.f, 0.f);
		const f3 d = act ? mk3(r1.x, r1.y, r1.z) : mk3(0.f, 0.f, 1.f);
		const float dist = act ? r0.w : 0.f;
		/* far as k_trace marks a shade point (sp_far) */
		const f3 of = uni(ks.tf.rotated) ? tf_point(ks.tf.r, ks.tf.c, o) : o;
		const bool far = act && tf_far(of, ks.tf.cf, ks.tf.rad);
		f3 li = mk3(1.f, 1.f, 1.f);
		const QBvh Q = make_qbvh<WALK>(ks, top_q, top_e, stk, t8, wv);
		const bool blocked = shadow_query<COUNT, WALK, LA>(Q, unip(ks.recs), unip(ks.mats), unip(ks.planes), uni(ks.num_planes),
								 unip(ks.lin), uni(ks.num_lin), uni(ks.have_tree) != 0, ks.tf, act, far, o, d,
								 dist, __float_as_uint(r1.w), li, sc);
		reread_barrier();
		if (in)
			res[i] = blocked ? make_float4(0.f, 0.f, 0.f, __uint_as_float(1u)) : make_float4(li.x, li.y, li.z, 0.f);
		n_live += popc64(ballot(act));
		n_blocked += popc64(ballot(blocked));
	}
	if (lane_id() == 0) {
		atomicAdd(&ctr[RTX_SQ_RAYS], n_live);
		atomicAdd(&ctr[RTX_SQ_BLOCKED], n_blocked);
		if (COUNT) {
			atomicAdd(&ctr[RTX_SQ_FAR], sc.far);
			atomicAdd(&ctr[RTX_SQ_BOXES], sc.boxes);
			atomicAdd(&ctr[RTX_SQ_TRIS], sc.tris);
			atomicAdd(&ctr[RTX_SQ_SPHERES], sc.sph);
			atomicAdd(&ctr[RTX_SQ_STEPS], sc.steps);
			atomicAdd(&ctr[RTX_SQ_UNIF], sc.unif);
			atomicAdd(&ctr[RTX_SQ_LEAFR], sc.lrounds);
			atomicAdd(&ctr[RTX_SQ_SPILL], sc.spills);
		}
	}
}
