/*
 * A part of rtx_shadow.hip's translation unit, included there once and not self-contained: it uses that
 * file's KShadow, emitter_uni, sample_ray, sample_att_of, shade_terms and shade_terms_s0, so its sums are
 * formed by the very code k_shadow runs.
 *
 * k_shadow_clear: the all-clear points, one per lane (RTX_OPT_SHADOW_CLEARLANE).
 */
/* An all-clear point (clear_run) needs neither the walk nor the layout made for it: in k_shadow a whole
 * wave reads one record, searches the emitter table, forms the draws' mix and reduces three butterflies
 * per point, and nearly every operand of its sample loop is a scalar.  Here the chunk's points are split
 * first (k_clear_count, k_clear_scan, k_clear_scatter: a stable partition of the processing order by
 * clear_lane_point), k_shadow takes the rest as before, and k_shadow_clear takes the clear list, a point
 * per lane, the samples in sequence.
 *   The clear list holds the points that pass k_shadow's all-clear predicate on their mask word and whose
 * smp byte names every emitter: the point lies on no emitter, so sample idx belongs to the same emitter
 * for every one of them and the sample index and the emitter stay wave-uniform. */
#define RTX_CL_BLOCK 256
#define RTX_CL_ITEMS 1024 /* positions of the processing order per workgroup of the partition */

__device__ __forceinline__ bool clear_lane_point(uint32_t w, bool tree, uint32_t point, uint32_t all)
{
	const uint32_t smp = w >> 24, ok = (w >> 8) & (w >> 16) & (tree ? w : ~0u) & 0xffu;
	const bool ac = point != 0 && smp && !(smp & ~ok); /* k_shadow's, word for word */
	return ac && smp == all;
}

/* position i of the processing order: its record index, and whether it goes to the clear list */
__device__ __forceinline__ bool clear_lane_at(const KShadow &ks, uint32_t i, uint32_t &sid)
{
	const bool tree = ks.have_tree != 0 && RTX_DEBUG_NOWALK != 1;
	sid = 0u;
	if (i >= ks.n_sp)
		return false;
	sid = ks.perm ? ks.perm[i] : i;
	return clear_lane_point(ks.pm[sid], tree, ks.point, (1u << ks.num_emitters) - 1u);
}

/* the clear points among each workgroup's RTX_CL_ITEMS positions */
__global__ __launch_bounds__(RTX_CL_BLOCK) void k_clear_count(KShadow ks, uint32_t *__restrict__ cnt)
{
	__shared__ uint32_t wc[RTX_CL_BLOCK / WAVE];
	uint32_t c = 0;
	for (uint32_t r = 0; r < RTX_CL_ITEMS / RTX_CL_BLOCK; r++) {
		uint32_t sid;
		c += popc64(ballot(clear_lane_at(ks, blockIdx.x * RTX_CL_ITEMS + r * RTX_CL_BLOCK + threadIdx.x, sid)));
	}
	if (lane_id() == 0)
		wc[threadIdx.x / WAVE] = c;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t t = 0;
		for (uint32_t w = 0; w < RTX_CL_BLOCK / WAVE; w++)
			t += wc[w];
		cnt[blockIdx.x] = t;
	}
}

/* one workgroup: the counts' exclusive prefix sums in place, and their total, the clear list's length, to
 * RTX_C_CLPTS (k_shadow_clear reads it there) and to k_shadow's queue head: the rest list follows the
 * clear list in one array, and k_shadow, given the whole array, begins behind the clear list */
__global__ __launch_bounds__(1024) void k_clear_scan(uint32_t *__restrict__ cnt, uint32_t nb, unsigned long long *__restrict__ ctr)
{
	__shared__ uint32_t part[1024];
	const uint32_t per = (nb + 1023u) / 1024u, lo = min(threadIdx.x * per, nb), hi = min(lo + per, nb);
	uint32_t s = 0;
	for (uint32_t i = lo; i < hi; i++)
		s += cnt[i];
	part[threadIdx.x] = s;
	__syncthreads();
	for (uint32_t d = 1; d < 1024u; d <<= 1) {
		const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
		__syncthreads();
		part[threadIdx.x] += v;
		__syncthreads();
	}
	uint32_t run = part[threadIdx.x] - s;
	for (uint32_t i = lo; i < hi; i++) {
		const uint32_t c = cnt[i];
		cnt[i] = run;
		run += c;
	}
	if (threadIdx.x == 1023u) {
		ctr[RTX_C_CLPTS] = part[1023];
		ctr[RTX_C_SPQUEUE] = part[1023];
	}
}

/* out = clear list | rest list, each in the processing order: a clear point goes to the number of clear
 * points before it, any other behind the clear list to the number of other points before it */
__global__ __launch_bounds__(RTX_CL_BLOCK) void k_clear_scatter(KShadow ks, const uint32_t *__restrict__ off, uint32_t *__restrict__ out)
{
	__shared__ uint32_t wc[RTX_CL_BLOCK / WAVE];
	const uint32_t nc = (uint32_t)ks.ctr[RTX_C_CLPTS], wv = threadIdx.x / WAVE;
	uint32_t run = off[blockIdx.x];
	for (uint32_t r = 0; r < RTX_CL_ITEMS / RTX_CL_BLOCK; r++) {
		const uint32_t i = blockIdx.x * RTX_CL_ITEMS + r * RTX_CL_BLOCK + threadIdx.x;
		uint32_t sid;
		const bool f = clear_lane_at(ks, i, sid);
		const u64 m = ballot(f);
		__syncthreads(); /* the round before has read wc */
		if (lane_id() == 0)
			wc[wv] = popc64(m);
		__syncthreads();
		uint32_t before = run + mbcnt(m), all = 0;
		for (uint32_t w = 0; w < RTX_CL_BLOCK / WAVE; w++) {
			before += w < wv ? wc[w] : 0u;
			all += wc[w];
		}
		if (i < ks.n_sp)
			out[f ? before : nc + (i - before)] = sid;
		run += all;
	}
}

/* a float in a vector register of its own, so the arithmetic on it takes the two-VGPR forms */
__device__ __forceinline__ float in_vgpr(float x)
{
	asm("" : "+v"(x));
	return x;
}

/* what the sample loop reads of an emitter, per lane: k_shadow holds them in scalar registers, and a
 * scalar operand keeps an add, mul or fma from dual issue */
struct EmLane {
	uint32_t type, num_lights;
	f3 li, p0, p1, p2;
	float radius;
};
__device__ __forceinline__ void st3(float *d, f3 v)
{
	d[0] = v.x;
	d[1] = v.y;
	d[2] = v.z;
}
__device__ __forceinline__ EmLane emitter_lanes(const DEmitter &E)
{
	EmLane v;
	v.type = E.type;
	v.num_lights = E.num_lights;
	v.li = mk3(in_vgpr(E.li[0]), in_vgpr(E.li[1]), in_vgpr(E.li[2]));
	v.p0 = mk3(in_vgpr(E.p0[0]), in_vgpr(E.p0[1]), in_vgpr(E.p0[2]));
	v.p1 = v.p2 = v.p0;
	if (E.type != RTX_SPHERE) { /* a sphere light reads neither */
		v.p1 = mk3(in_vgpr(E.p1[0]), in_vgpr(E.p1[1]), in_vgpr(E.p1[2]));
		v.p2 = mk3(in_vgpr(E.p2[0]), in_vgpr(E.p2[1]), in_vgpr(E.p2[2]));
	}
	v.radius = in_vgpr(E.radius);
	return v;
}

/* The light sum of this lane's point, today's bit for bit.  In k_shadow lane l adds samples l, l + 64, ...
 * to a sum that starts at +0, and wave_sum adds lane ^ M's value for M = 32, 16, ..., 1; lane 0's total
 * is a binary tree over the lanes' sums whose leaves, left to right, are lanes 0, 32, 16, 48, ...: the
 * 6-bit reversal of 0, 1, 2, ....  So leaf t is lane l = rev6(t): its samples in index order (each inside
 * its emitter's range: the packets clear_run hands to light_sample give the same terms), then the tree
 * folded as a binary counter: level b holds the left child until bit b of t says the right one is here,
 * the left operand the one with the lower lanes.  18 registers of stack.  S0: shade_terms_s0. */
template <bool S0>
__device__ __forceinline__ f3 clear_lane_sum(const KShadow &ks, const uint2 *mixs, uint32_t nl, int32_t rng, int32_t att, int32_t refl,
					     float att_offset, f3 p, f3 n, f3 dir, f3 kd, f3 ks3, float shin)
{
	const auto *EM = cptr(ks.emitters);
	const uint32_t ne = ks.num_emitters;
	const f3 zero = mk3(0.f, 0.f, 0.f);
	f3 s0 = zero, s1 = zero, s2 = zero, s3 = zero, s4 = zero, s5 = zero, x = zero;
	EmLane ev = { 0u, 0u, zero, zero, zero, zero, 0.f };
	uint32_t ev_e = RTX_NONE;
	for (uint32_t t = 0; t < WAVE; t++) {
		const uint32_t l = __builtin_bitreverse32(t) >> 26;
		x = zero;
		for (uint32_t e = 0, start = 0; e < ne && start < nl; e++) {
			const uint32_t end = start + EM[e].num_lights, lim = min(end, nl);
			uint32_t idx = start <= l ? l : l + ((start - l + (WAVE - 1u)) & ~(WAVE - 1u));
			if (idx < lim) {
				if (ev_e != e) { /* once per render where there is one emitter */
					ev = emitter_lanes(emitter_uni(ks.emitters + e));
					ev_e = e;
				}
				DEmitter E = {};
				E.type = ev.type;
				E.num_lights = ev.num_lights;
				E.radius = ev.radius;
				st3(E.li, ev.li);
				st3(E.p0, ev.p0);
				st3(E.p1, ev.p1);
				st3(E.p2, ev.p2);
				const uint2 mw = mixs[e * RTX_CL_BLOCK];
				const uint64_t mix = key_of(mw.x, mw.y);
				for (; idx < lim; idx += WAVE) {
					const uint32_t j = idx - start;
					float u1 = 0.5f, u2 = 0.5f;
					if (rng != RTX_RNG_CONST)
						rtx_draw2_mixed(mix, j, &u1, &u2);
					f3 ldir, li;
					float ldist, dsq;
					sample_ray(rng, E, j, u1, u2, p, ldir, ldist, dsq, li);
					const float attf = sample_att_of(att, att_offset, ldist, dsq);
					x = add3(x, S0 ? shade_terms_s0(att, n, kd, ks3, ldir, li, attf) :
							 shade_terms(att, refl, n, dir, kd, ks3, shin, ldir, li, attf));
				}
			}
			start = end;
		}
		if (!(t & 1u)) {
			s0 = x;
			continue;
		}
		x = add3(s0, x);
		if (!(t & 2u)) {
			s1 = x;
			continue;
		}
		x = add3(s1, x);
		if (!(t & 4u)) {
			s2 = x;
			continue;
		}
		x = add3(s2, x);
		if (!(t & 8u)) {
			s3 = x;
			continue;
		}
		x = add3(s3, x);
		if (!(t & 16u)) {
			s4 = x;
			continue;
		}
		x = add3(s4, x);
		if (!(t & 32u)) {
			s5 = x;
			continue;
		}
		x = add3(s5, x);
	}
	return x; /* t = 63 falls through every level: the root */
}

/* Lane i of the grid takes entry i of the clear list (RTX_C_CLPTS entries): its record and material per
 * lane, its draws' mix per emitter (kept in LDS, a slot per lane: 64-bit multiplies, not to be redone
 * per leaf), clear_lane_sum, and k_shadow's tail.  No loads in the loops but the emitter table's, through
 * the scalar cache.  The shininess-0 loop runs where every lane's point has shininess 0; else every lane
 * runs the generic one (the two give the same bits, RTX_OPT_SHADOW_SPEC).  One lane per wave counts the rays. */
__global__ __launch_bounds__(RTX_CL_BLOCK) void k_shadow_clear(KShadow ks, const uint32_t *__restrict__ list)
{
	__shared__ uint2 mixs[8 * RTX_CL_BLOCK];
	const uint32_t nc = uni((uint32_t)ks.ctr[RTX_C_CLPTS]);
	const uint32_t i = blockIdx.x * RTX_CL_BLOCK + threadIdx.x;
	if (uni(i) >= nc) /* the wave's first entry */
		return;
	const bool own = i < nc;
	const uint32_t sid = list[own ? i : nc - 1u]; /* the lanes past the list redo its last point and store nothing */
	const float4 *rec = ks.sp + (size_t)sid * SPREC;
	const float4 q0 = ldg4(rec, 0), q1 = ldg4(rec, 16), q2 = ldg4(rec, 32), q3 = ldg4(rec, 48), q4 = ldg4(rec, 64), q5 = ldg4(rec, 80);
	const f3 p = mk3(q0.x, q0.y, q0.z), n = mk3(q1.x, q1.y, q1.z), dir = mk3(q2.x, q2.y, q2.z), kd = mk3(q3.x, q3.y, q3.z);
	const uint64_t key = key_of(__float_as_uint(q4.y), __float_as_uint(q4.z));
	const DMaterial &mat = ks.mats[__float_as_uint(q3.w)];
	const f3 ks3 = ld3(mat.ks);
	const float shin = mat.shininess;
	const uint32_t ne = min(ks.num_emitters, 8u);
	const auto *EM = cptr(ks.emitters);
	uint32_t nl = 0;
	for (uint32_t e = 0; e < ne; e++) {
		nl += EM[e].num_lights;
		const uint64_t mix = rtx_draw_mix(key, e);
		mixs[e * RTX_CL_BLOCK + threadIdx.x] = make_uint2((uint32_t)mix, (uint32_t)(mix >> 32));
	}
	const int32_t rng = ks.rng, att = ks.attenuation, refl = ks.reflection == RTX_BLINN ? RTX_BLINN : RTX_PHONG;
	const float att_offset = in_vgpr(ks.att_offset);
	const bool s0 = ks.spec && !ballot(!shin_zero(shin));
	const f3 Ls = s0 ? clear_lane_sum<true>(ks, mixs + threadIdx.x, nl, rng, att, refl, att_offset, p, n, dir, kd, ks3, shin) :
			   clear_lane_sum<false>(ks, mixs + threadIdx.x, nl, rng, att, refl, att_offset, p, n, dir, kd, ks3, shin);
	if (own) {
		const f3 c = mul3v(mk3(q0.w, q1.w, q2.w), Ls);
		ks.contrib[sid] = make_float4(c.x, c.y, c.z, q5.x);
	}
	if (lane_id() == 0)
		atomicAdd(&ks.ctr[RTX_C_CLRAYS], (unsigned long long)min(nc - i, (uint32_t)WAVE) * nl);
}
