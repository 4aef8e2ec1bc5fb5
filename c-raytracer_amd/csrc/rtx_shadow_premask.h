/*
 * A part of rtx_shadow.hip's translation unit, included there once and not self-contained: it uses that
 * file's KShadow, emitter_uni, emitter_sphere, plane_clear, cone_of and cone_meets.
 */
/* point_masks ahead of k_shadow (RTX_OPT_SHADOW_PREMASK), one shade point per lane: in point_masks a
 * whole wave works on one point, and all but its two sphere passes is wave-uniform arithmetic done 64
 * times over for one answer.  Here lane i takes record i of the chunk and walks the emitters, the
 * planes, the cull spheres and the listed records' spheres in turn, each read through the scalar
 * cache at a wave-uniform index, through the very functions point_masks calls (one translation unit: its compile
 * flags, -ffp-contract=off, hold for both), so every predicate has the same operands and the same
 * answer.  Scenes of at most 8 emitters only: the word written for record i is
 * cone | pln << 8 | lin << 16 | smp << 24, bit e of each byte for emitter e, and 0 for a far point
 * (point_masks gives a far point no mask).  k_shadow reads it where it would call point_masks.
 * Every shade point has a light sample (k_trace emits no other), so a point that is not far samples
 * some emitter and its smp byte is not 0: the byte tells the far points apart. */
#define RTX_PM_BLOCK 256
__global__ __launch_bounds__(RTX_PM_BLOCK) void k_point_masks(KShadow ks, uint32_t *__restrict__ out)
{
	const uint32_t i = blockIdx.x * RTX_PM_BLOCK + threadIdx.x;
	const bool own = i < ks.n_sp;
	const float4 *rec = ks.sp + (size_t)(own ? i : ks.n_sp - 1u) * SPREC;
	const float4 q0 = ldg4(rec, 0), q4 = ldg4(rec, 64);
	const f3 p = mk3(q0.x, q0.y, q0.z);
	const uint32_t ow = __float_as_uint(q4.x), obj = ow & ~RTX_SP_FAR;
	const bool live = own && !(ow & RTX_SP_FAR);
	const bool pt = ks.point != 0;
	const uint32_t n = min(ks.num_cull, (uint32_t)WAVE);
	const uint32_t ne = min(ks.num_emitters, 8u);
	const uint32_t num_lin = ks.num_lin, num_planes = ks.num_planes;
	const uint32_t nr = pt ? min(ks.num_lsph, (uint32_t)WAVE) : 0u;
	const bool lin_ok = pt && nr == num_lin;
	uint32_t cone = 0u, pln = 0u, lin = 0u, smp = 0u;
	for (uint32_t e = 0; e < ne; e++) {
		const DEmitter E = emitter_uni(ks.emitters + e);
		const uint32_t bit = 1u << e;
		if (E.obj != obj)
			smp |= bit;
		f3 lc;
		float lr;
		emitter_sphere(E, lc, lr);
		const f3 ax0 = sub3(lc, p);
		const float L = sqrtf(magsqr3(ax0));
		if (pt) {
			bool pc = true;
			for (uint32_t k = 0; k < num_planes; k++) {
				const auto *pl = cptr(ks.planes) + k;
				pc = plane_clear(mk3(pl->n[0], pl->n[1], pl->n[2]), pl->d, pl->eps, p, lc, lr, L) && pc;
			}
			if (pc)
				pln |= bit;
			if (!num_lin)
				lin |= bit;
		}
		/* a lane whose point has no cone toward e (at or inside the light's sphere) counts as met */
		const bool go = live && L > 1.01f * lr;
		if ((!n && !nr) || !ballot(go))
			continue;
		const Cone c = cone_of(p, lc, lr, ax0, L);
		if (n) {
			/* four spheres a turn, their scalar loads issued together (one wait, not four; past the
			 * last sphere the last one again), until every lane of the wave has met one */
			bool meets = !go;
			for (uint32_t k = 0; k < n && ballot(!meets); k += 4) {
				f4v s[4];
#pragma unroll
				for (uint32_t j = 0; j < 4; j++)
					s[j] = *(const __attribute__((address_space(4))) f4v *)(ks.cull + min(k + j, n - 1u));
#pragma unroll
				for (uint32_t j = 0; j < 4; j++)
					meets = cone_meets<false>(c, p, make_float4(s[j].x, s[j].y, s[j].z, s[j].w)) || meets;
			}
			if (!meets)
				cone |= bit;
		}
		if (lin_ok && nr) {
			bool meets = !go;
			for (uint32_t k = 0; k < nr && ballot(!meets); k++) {
				const uint32_t ro = cptr((const uint32_t *)(ks.lin + k))[0]; /* DEmitter.obj */
				const f4v s = *(const __attribute__((address_space(4))) f4v *)(ks.lsph + k);
				meets = meets || (ro != E.obj && cone_meets<true>(c, p, make_float4(s.x, s.y, s.z, s.w)));
			}
			if (!meets)
				lin |= bit;
		}
	}
	if (own)
		out[i] = live ? (cone | pln << 8 | lin << 16 | smp << 24) : 0u;
}
