/*
 * A part of rtx_shadow.hip's translation unit, included there once and not self-contained: its kernels
 * call that file's device functions (any_tri, box_hit_q, light_point_sh, sh_pow, plane_clear, cone_meets,
 * dark_terms, shade_terms and their _s0 forms, order_begin, order_key), so a known answer is the answer of
 * the code k_shadow runs.
 *
 * Known answers of the fast device functions k_shadow runs (rtx_kat.h).
 */
__global__ void k_kat_shadow(int kind, uint32_t n, const float *__restrict__ in, float *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const float *x = in + (size_t)i * rtx_kat_in_width[kind];
	float *y = out + (size_t)i * rtx_kat_out_width[kind];
	switch (kind) {
	case RTX_KAT_ANY_TRI:
		y[0] = any_tri(ld3(x + 6), ld3(x + 9), ld3(x + 12), ld3(x), ld3(x + 3), x[15], x[16]) ? 1.f : 0.f;
		break;
	case RTX_KAT_SPH_LIGHT_SH: {
		DEmitter e;
		e.type = RTX_SPHERE;
		for (int k = 0; k < 3; k++)
			e.p0[k] = x[k];
		e.radius = x[3];
		const f3 l = light_point_sh(e, ld3(x + 4), x[7], x[8]);
		y[0] = l.x;
		y[1] = l.y;
		y[2] = l.z;
	} break;
	case RTX_KAT_SPEC_POW:
		y[0] = fmaxf(0.f, sh_pow(x[0], x[1]));
		break;
	case RTX_KAT_PLANE_CLEAR:
	case RTX_KAT_LIN_CLEAR: {
		/* point_masks' predicates for one point, light and plane / record, beside the per-ray test of
		 * one of k_shadow's own samples of that light */
		const f3 p = ld3(x);
		DEmitter e;
		e.type = x[3] == 0.f ? RTX_SPHERE : RTX_TRIANGLE;
		e.num_lights = 1;
		for (int k = 0; k < 3; k++) {
			e.p0[k] = x[4 + k];
			e.p1[k] = x[7 + k];
			e.p2[k] = x[10 + k];
			e.li[k] = 1.f;
		}
		e.radius = x[13];
		f3 lc, ldir, li;
		float lr, ldist, dsq;
		emitter_sphere(e, lc, lr);
		const f3 ax0 = sub3(lc, p);
		const float L = sqrtf(magsqr3(ax0));
		const bool pk = kind == RTX_KAT_PLANE_CLEAR;
		sample_ray(RTX_RNG_CONST, e, 0u, x[pk ? 19 : 26], x[pk ? 20 : 27], p, ldir, ldist, dsq, li);
		bool clear, blocks;
		if (pk) {
			clear = plane_clear(ld3(x + 14), x[17], x[18], p, lc, lr, L);
			blocks = plane_blocks(ld3(x + 14), x[17], p, ldir, x[18], ldist);
		} else {
			const bool sph = x[14] == 0.f;
			float rs[4];
			rtx_record_sphere(sph, x + 15, x + 18, x + 21, x[24], rs);
			clear = L > 1.01f * lr && !cone_meets<true>(cone_of(p, lc, lr, ax0, L), p, make_float4(rs[0], rs[1], rs[2], rs[3]));
			if (sph) {
				float t = 0.f;
				blocks = hit_sphere(ld3(x + 15), x[24], p, ldir, x[25], t) && t < ldist;
			} else {
				const f3 w0 = ld3(x + 15);
				blocks = any_tri(w0, sub3(ld3(x + 18), w0), sub3(ld3(x + 21), w0), p, ldir, x[25], ldist);
			}
		}
		y[0] = clear ? 1.f : 0.f;
		y[1] = blocks ? 1.f : 0.f;
		y[2] = ldir.x;
		y[3] = ldir.y;
		y[4] = ldir.z;
		y[5] = ldist;
	} break;
	case RTX_KAT_DARK: {
		/* dark_terms beside shade_terms for the sample's li and for li through one transparent
		 * surface, the attenuation factor formed as light_sample forms it */
		const f3 n = ld3(x), dir = ld3(x + 3), kd = ld3(x + 6), ks3 = ld3(x + 9), ldir = ld3(x + 13), li = ld3(x + 17), kt = ld3(x + 23);
		const float shin = x[12], ldist = x[16];
		const int32_t att = (int32_t)x[20], refl = (int32_t)x[22];
		const float attf = sample_att_of(att, x[21], ldist, ldist * ldist);
		const bool ok = fin3(li) && fabsf(kt.x) <= 1.f && fabsf(kt.y) <= 1.f && fabsf(kt.z) <= 1.f; /* scene_dark_ok */
		const bool dark = ok && dark_terms(att, refl, n, dir, kd, ks3, shin, ldir, li, attf, true);
		const f3 t0 = shade_terms(att, refl, n, dir, kd, ks3, shin, ldir, li, attf);
		const f3 t1 = shade_terms(att, refl, n, dir, kd, ks3, shin, ldir, mul3v(li, kt), attf);
		y[0] = dark ? 1.f : 0.f;
		y[1] = t0.x;
		y[2] = t0.y;
		y[3] = t0.z;
		y[4] = t1.x;
		y[5] = t1.y;
		y[6] = t1.z;
	} break;
	case RTX_KAT_SPEC0: {
		/* RTX_KAT_DARK's record through the shininess-0 forms (its shin is not read): what
		 * dark_terms / shade_terms give for the same record with shin = +-0, bit for bit */
		const f3 n = ld3(x), kd = ld3(x + 6), ks3 = ld3(x + 9), ldir = ld3(x + 13), li = ld3(x + 17), kt = ld3(x + 23);
		const float ldist = x[16];
		const int32_t att = (int32_t)x[20];
		const float attf = sample_att_of(att, x[21], ldist, ldist * ldist);
		const bool ok = fin3(li) && fabsf(kt.x) <= 1.f && fabsf(kt.y) <= 1.f && fabsf(kt.z) <= 1.f; /* scene_dark_ok */
		const bool dark = ok && dark_terms_s0(att, n, kd, ks3, ldir, li, attf, true);
		const f3 t0 = shade_terms_s0(att, n, kd, ks3, ldir, li, attf);
		const f3 t1 = shade_terms_s0(att, n, kd, ks3, ldir, mul3v(li, kt), attf);
		y[0] = dark ? 1.f : 0.f;
		y[1] = t0.x;
		y[2] = t0.y;
		y[3] = t0.z;
		y[4] = t1.x;
		y[5] = t1.y;
		y[6] = t1.z;
	} break;
	case RTX_KAT_BOX_Q: {
		/* the walk's setup (shadow_query / shadow_walk) and its box test on the quantised box */
		const f3 o = ld3(x), d = ld3(x + 3), qo = ld3(x + 12), qs = ld3(x + 15);
		const uint4 nd = make_uint4(rtx_quantise(x[6], x[9], qo.x, qs.x), rtx_quantise(x[7], x[10], qo.y, qs.y),
					    rtx_quantise(x[8], x[11], qo.z, qs.z), 0u);
		const f3 inv = safe_inv_fast(d);
		const f3 invq = mk3(inv.x * (1.f / qs.x), inv.y * (1.f / qs.y), inv.z * (1.f / qs.z));
		const f3 oq = mk3((o.x - qo.x) * qs.x, (o.y - qo.y) * qs.y, (o.z - qo.z) * qs.z);
		const f3 oi = mul3v(oq, invq);
		const uint32_t oct = ((~__float_as_uint(inv.x)) >> 31) | (((~__float_as_uint(inv.y)) >> 31) << 1) |
				     (((~__float_as_uint(inv.z)) >> 31) << 2);
		bool ho = false;
		switch (oct) {
#define RTX_KATOCT(K)                                      \
	case K:                                                \
		ho = box_hit_q<K>(nd, oi, invq, x[18]);            \
		break;
			RTX_KATOCT(0) RTX_KATOCT(1) RTX_KATOCT(2) RTX_KATOCT(3) RTX_KATOCT(4) RTX_KATOCT(5) RTX_KATOCT(6)
			RTX_KATOCT(7)
#undef RTX_KATOCT
		}
		y[0] = box_hit_q<8>(nd, oi, invq, x[18]) ? 1.f : 0.f;
		y[1] = ho ? 1.f : 0.f;
	} break;
	case RTX_KAT_BOX_Q8: {
		/* the 8-wide walk's setup and child test on the box quantised to 16 bits, then to 8 bits in
		 * the node frame (org, e) given by the record, exactly as rtx_wide8_build does */
		const f3 o = ld3(x), d = ld3(x + 3), qo = ld3(x + 12), qs = ld3(x + 15);
		uint32_t w[16];
		for (int k = 0; k < 16; k++)
			w[k] = 0;
		const uint32_t org[3] = { (uint32_t)x[19], (uint32_t)x[20], (uint32_t)x[21] };
		const uint32_t ex[3] = { (uint32_t)x[22], (uint32_t)x[23], (uint32_t)x[24] };
		w[0] = org[0] | (org[1] << 16);
		w[1] = org[2] | (ex[0] << 16) | (ex[1] << 20) | (ex[2] << 24);
		w[3] = 1u;
		for (int a = 0; a < 3; a++) {
			const uint32_t q8 = rtx_quantise8(rtx_quantise(x[6 + a], x[9 + a], x[12 + a], x[15 + a]), org[a], ex[a]);
			w[4 + 4 * a] = (q8 & 0xFFu) | 0xFFFFFF00u; /* slot 0 the box, slots 1..7 empty */
			w[5 + 4 * a] = 0xFFFFFFFFu;
			w[6 + 4 * a] = q8 >> 8;
			w[7 + 4 * a] = 0u;
		}
		const f3 inv = safe_inv_fast(d);
		const f3 invq = mk3(inv.x * (1.f / qs.x), inv.y * (1.f / qs.y), inv.z * (1.f / qs.z));
		const f3 oq = mk3((o.x - qo.x) * qs.x, (o.y - qo.y) * qs.y, (o.z - qo.z) * qs.z);
		const f3 oi = mul3v(oq, invq);
		const uint32_t oct = ((~__float_as_uint(inv.x)) >> 31) | (((~__float_as_uint(inv.y)) >> 31) << 1) |
				     (((~__float_as_uint(inv.z)) >> 31) << 2);
		f3 sc, bc;
		w8_frame(w, invq, oi, sc, bc);
		uint32_t ho = 0;
		switch (oct) {
#define RTX_KATOCT8(K)                                                        \
	case K:                                                                   \
		ho = w8_hits<K, (~(uint32_t)K & 7u)>(w, sc, bc, x[18]);               \
		ho = ho == (1u << (~(uint32_t)K & 7u)) ? 1u : ho ? 2u : 0u;           \
		break;
			RTX_KATOCT8(0) RTX_KATOCT8(1) RTX_KATOCT8(2) RTX_KATOCT8(3) RTX_KATOCT8(4) RTX_KATOCT8(5) RTX_KATOCT8(6)
			RTX_KATOCT8(7)
#undef RTX_KATOCT8
		}
		const uint32_t hg = w8_hits<8, 0u>(w, sc, bc, x[18]);
		/* 1 = slot 0 hit alone; 2 would flag an empty slot hit (never expected) */
		y[0] = hg == 1u ? 1.f : hg ? 2.f : 0.f;
		y[1] = (float)ho;
	} break;
	}
}

/* RTX_KAT_ORDER: order_begin for one shade point and one emitter of nl lights, one wave per record.
 * The point's record, the emitter, the material, the masks and the wave's slice live in the output
 * record's tail (rtx_kat.h); k_kat_order_fill writes them first, in a launch of its own, as
 * order_begin reads them through the scalar cache */
static_assert(sizeof(DEmitter) <= 256 && sizeof(DMaterial) <= 256, "the KAT record's emitter and material slots");
__global__ void k_kat_order_fill(uint32_t n, const float *__restrict__ in, float *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const float *x = in + (size_t)i * rtx_kat_in_width[RTX_KAT_ORDER];
	float *y = out + (size_t)i * rtx_kat_out_width[RTX_KAT_ORDER];
	float4 *rec = (float4 *)(y + RTX_KAT_ORDER_REC);
	DEmitter *em = (DEmitter *)(y + RTX_KAT_ORDER_REC + 24);
	DMaterial *mat = (DMaterial *)(y + RTX_KAT_ORDER_REC + 24 + 64);
	uint32_t *cm = (uint32_t *)y + RTX_KAT_ORDER_REC + 24 + 128;
	const uint32_t nl = (uint32_t)x[26];
	DEmitter e;
	memset(&e, 0, sizeof(e));
	e.obj = 1u;
	e.type = x[16] == 0.f ? RTX_SPHERE : RTX_TRIANGLE;
	e.num_lights = nl;
	for (int k = 0; k < 3; k++) {
		e.li[k] = 1.f;
		e.p0[k] = x[17 + k];
		e.p1[k] = x[20 + k];
		e.p2[k] = x[23 + k];
		e.e1[k] = e.p1[k] - e.p0[k];
		e.e2[k] = e.p2[k] - e.p0[k];
	}
	e.radius = x[29];
	*em = e;
	DMaterial m;
	memset(&m, 0, sizeof(m));
	for (int k = 0; k < 3; k++)
		m.ks[k] = x[12 + k];
	m.shininess = x[15];
	*mat = m;
	rec[0] = make_float4(x[0], x[1], x[2], 1.f);
	rec[1] = make_float4(x[3], x[4], x[5], 1.f);
	rec[2] = make_float4(x[6], x[7], x[8], 1.f);
	rec[3] = make_float4(x[9], x[10], x[11], __uint_as_float(0u));
	rec[4] = make_float4(__uint_as_float(0u), __uint_as_float((uint32_t)x[27]), __uint_as_float((uint32_t)x[28]), __uint_as_float(nl));
	rec[5] = make_float4(0.f, 0.f, 0.f, 0.f);
	for (int k = 0; k < 8; k++)
		cm[k] = 0u;
}
__global__ __launch_bounds__(WAVE) void k_kat_order(uint32_t n, const float *__restrict__ in, float *__restrict__ out)
{
	const float *x = in + (size_t)blockIdx.x * rtx_kat_in_width[RTX_KAT_ORDER];
	float *y = out + (size_t)blockIdx.x * rtx_kat_out_width[RTX_KAT_ORDER];
	uint32_t *yu = (uint32_t *)y;
	const float4 *rec = (const float4 *)(y + RTX_KAT_ORDER_REC);
	const DEmitter *em = (const DEmitter *)(y + RTX_KAT_ORDER_REC + 24);
	const DMaterial *mat = (const DMaterial *)(y + RTX_KAT_ORDER_REC + 24 + 64);
	uint32_t *cm = yu + RTX_KAT_ORDER_REC + 24 + 128, *ob = cm + 8;
	const uint32_t nl = (uint32_t)x[26];
	__shared__ KShadow ks;
	if (threadIdx.x == 0) {
		memset(&ks, 0, sizeof(ks));
		ks.emitters = em;
		ks.num_emitters = 1u;
		ks.mats = mat;
		ks.rng = RTX_RNG_COUNTER;
		ks.reflection = (int32_t)x[33];
		ks.attenuation = (int32_t)x[34];
		ks.att_offset = x[35];
		ks.dark = x[36] != 0.f ? 1u : 0u;
		ks.spec = 1u; /* the default, as the product's key pass runs */
		for (int k = 0; k < 3; k++)
			ks.tf.c[k] = x[30 + k];
	}
	__syncthreads();
	ShadowCount sc = {};
	const uint32_t st = order_begin<false, WALK_W8>(ks, rec, nl, 0u, cm, ob, sc);
	if (threadIdx.x == 0) {
		y[0] = st ? (float)(st & 0x7ffu) : 0.f;
		y[1] = st ? (float)((st >> 16) & 31u) : 0.f;
		y[2] = 0.f;
		y[3] = 0.f;
	}
	/* every sample's bucket and x again, from the function order_begin takes them from */
	const DEmitter Eu = emitter_uni(em);
	const f3 p = ld3(x);
	f3 lc;
	float lr;
	emitter_sphere(Eu, lc, lr);
	const f3 b = order_dir(p, lc, mk3(x[30], x[31], x[32]));
	const float ilr = lr > 0.f ? 1.f / lr : 0.f;
	for (uint32_t j = threadIdx.x; j < RTX_ORD_CAP; j += WAVE) {
		bool dark;
		float xv = 0.f;
		const uint32_t bk = order_key(ks, rec, Eu, 0u, j, (uint32_t)x[27], (uint32_t)x[28], p, b, ilr, ks.dark != 0, j < nl, dark, &xv);
		y[4 + j] = st && j < (st & 0x7ffu) ? (float)ob[j] : -1.f;
		y[4 + RTX_ORD_CAP + j] = (float)bk;
		y[4 + 2 * RTX_ORD_CAP + j] = j < nl ? xv : 0.f;
	}
}
