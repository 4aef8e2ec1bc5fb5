/*
 * rtx_kat.h — known-answer-test record layouts for rtx_kat() (GPU) and
 * rtx_oracle_kat() (CPU oracle).  Each kind evaluates one function of the hot
 * path over n fixed-size float records; integers travel as their float bit
 * patterns.  Fixtures come from the reference's own functions (oracle/ref_kat.c).
 *
 * kind               in (floats per record)                         out                        reference
 * KAT_MOLLER (0)     o3 d3 v0_3 e1_3 e2_3 eps          = 16          hit t                  = 2  object.c:422-441
 * KAT_SPHERE (1)     o3 d3 c3 r eps                    = 11          hit t n3               = 5  object.c:254-265,306-321
 * KAT_PLANE  (2)     o3 d3 n3 dd eps                   = 11          hit t n3               = 5  object.c:473-488
 * KAT_SLAB   (3)     o3 d3 lo3 hi3 eps                 = 13          hit tmin tmax          = 3  accel.c:112-158
 * KAT_NOISE  (4)     x y z                             = 3           noise                  = 1  SimplexNoise.c:99-194
 * KAT_TEXTURE(5)     type periodic c0_3 c1_3 scale mortar nfs ns fs P3 = 16  rgb3          = 3  material.c:152-200
 * KAT_SPH_LIGHT(6)   c3 r P3 u1 u2                     = 9           L3                     = 3  object.c:293-304
 * KAT_TRI_LIGHT(7)   v0_3 v1_3 v2_3 u1 u2              = 11          L3                     = 3  object.c:403-419
 * KAT_MORTON (8)     x y z (in [0,1])                  = 3           code(bits)             = 1  accel.c:72-88
 * KAT_U32    (9)     x                                 = 1           sat(bits) wrap(bits)   = 2  material.c:164
 * KAT_GI_DIR (10)    n3 eps u1 u2                      = 6           dir3                   = 3  render.c:240-281
 * KAT_REFRACT(11)    d3 n3 ior                         = 7           dir3                   = 3  render.c:320-335
 * -- the fast forms k_shadow actually runs (rtx_shadow.hip), checked against the exact ones --
 * KAT_ANY_TRI(12)    o3 d3 v0_3 e1_3 e2_3 eps tlim     = 17          hit                    = 1  object.c:422-441 (t < tlim)
 * KAT_SPH_LIGHT_SH(13) c3 r P3 u1 u2                   = 9           L3                     = 3  object.c:293-304
 * KAT_BOX_Q  (14)    o3 d3 lo3 hi3 qo3 qs3 tlim        = 19          hit(generic) hit(octant) = 2  accel.c:112-158
 *                    (the box is quantised on the device exactly as rtx_upload_scene quantises the
 *                     threaded BVH, rtx_quant.h, then tested by box_hit_q on the segment (0, tlim))
 * KAT_SPEC_POW(15)   x y                               = 2           fmaxf(0, pow(x, y))    = 1  render.c:224 (specular term,
 *                    x = specular_mul, y = shininess; the device runs sh_pow, the oracle glibc powf)
 * KAT_BOX_Q8 (16)   o3 d3 lo3 hi3 qo3 qs3 tlim org3 e3 = 25        hit(generic) hit(octant) = 2  accel.c:112-158
 *                    (the box quantised to 16 bits as for KAT_BOX_Q, then to 8 bits in an 8-wide node frame of
 *                     origin org (grid units, <= the 16-bit lo) and steps 2^e, rtx_quant.h rtx_quantise8, and
 *                     tested by the 8-wide walk's child test, rtx_shadow.hip w8_child)
 * -- k_shadow's per-point masks (rtx_shadow.hip point_masks) against the per-ray tests they stand for --
 * KAT_PLANE_CLEAR(17) P3 etype v0_3 v1_3 v2_3 r n3 dd eps u1 u2 = 21   clear blocks d3 dist      = 6
 *                    (etype 0: a sphere light of centre v0 and radius r; 1: the triangle light v0 v1 v2.  clear:
 *                     plane_clear for the light's padded bounding sphere; blocks: plane_blocks of the shadow ray
 *                     from P to the light point of (u1, u2), k_shadow's own sample; d dist: that ray's direction and length)
 * KAT_LIN_CLEAR(18)  P3 etype v0_3 v1_3 v2_3 r rtype w0_3 w1_3 w2_3 rr reps u1 u2 = 28  clear blocks d3 dist = 6
 *                    (the listed record: rtype 0 the sphere (w0, rr), 1 the triangle w0 w1 w2, epsilon reps; clear:
 *                     the cone from P around the light misses the record's padded bounding sphere, formed as at
 *                     upload (rtx_quant.h rtx_record_sphere); blocks: the record's shadow test of that sample's ray)
 * -- k_shadow's dark samples (rtx_shadow.hip dark_terms) against the terms they stand for --
 * KAT_DARK   (19)    n3 view3 kd3 ks3 shin ldir3 ldist li3 att att_offset refl kt3 = 26  dark terms3 terms_kt3 = 7
 *                    (att: RTX_ATT_*, refl: RTX_PHONG / RTX_BLINN, as floats; dark: dark_terms of the sample of
 *                     direction ldir and length ldist, 0 when li is not finite or |kt| > 1 as the scene's flag
 *                     has it; terms: shade_terms of the sample for li; terms_kt: for li * kt, the product a
 *                     walk through one transparent surface leaves)
 * -- k_shadow's sample order (rtx_shadow.hip order_begin), one wave per record --
 * KAT_ORDER  (20)    P3 n3 view3 kd3 ks3 shin etype v0_3 v1_3 v2_3 nl key_lo key_hi r centre3 refl att att_offset dark = 37
 *                    n_ord packets - - order[1024] bucket[1024] x[1024] scratch = 7332
 *                    (the shade point P of normal n, view direction and material (kd, ks, shin) on object 0; one
 *                     emitter, object 1, of nl lights: etype 0 the sphere (v0, r), 1 the triangle v0 v1 v2; the
 *                     point's draw key (integers below 2^24); centre: of the bounded objects' box; dark: the
 *                     RTX_OPT_SHADOW_DARK flag.  n_ord: the samples in the order (0: the run is not ordered),
 *                     order[pos]: the sample at position pos (-1 beyond n_ord), bucket[j]: sample j's bucket
 *                     (16: dark, or j >= nl), x[j]: its key value; scratch: the kernel's own records)
 * -- k_shadow's shininess-0 forms (rtx_shadow.hip shade_terms_s0 / dark_terms_s0) against the generic ones --
 * KAT_SPEC0  (21)    KAT_DARK's record (shin is not read)             = 26  dark terms3 terms_kt3 = 7
 *                    (what KAT_DARK gives for the same record with shin = +-0, bit for bit: the forms
 *                     RTX_OPT_SHADOW_SPEC runs for a wave-uniform point of shininess 0)
 * Texture records use the params' u32conv for the float->uint32 conversion.
 */
#ifndef RTX_KAT_H
#define RTX_KAT_H

enum rtx_kat_kind {
	RTX_KAT_MOLLER = 0,
	RTX_KAT_SPHERE = 1,
	RTX_KAT_PLANE = 2,
	RTX_KAT_SLAB = 3,
	RTX_KAT_NOISE = 4,
	RTX_KAT_TEXTURE = 5,
	RTX_KAT_SPH_LIGHT = 6,
	RTX_KAT_TRI_LIGHT = 7,
	RTX_KAT_MORTON = 8,
	RTX_KAT_U32 = 9,
	RTX_KAT_GI_DIR = 10,
	RTX_KAT_REFRACT = 11,
	RTX_KAT_ANY_TRI = 12,
	RTX_KAT_SPH_LIGHT_SH = 13,
	RTX_KAT_BOX_Q = 14,
	RTX_KAT_SPEC_POW = 15,
	RTX_KAT_BOX_Q8 = 16,
	RTX_KAT_PLANE_CLEAR = 17,
	RTX_KAT_LIN_CLEAR = 18,
	RTX_KAT_DARK = 19,
	RTX_KAT_ORDER = 20,
	RTX_KAT_SPEC0 = 21,
	RTX_KAT_NKINDS = 22,
};
#define RTX_KAT_FIRST_SHADOW RTX_KAT_ANY_TRI /* kinds >= this run in rtx_shadow.hip's translation unit (rtx_shadow_kat.h) */

static const int rtx_kat_in_width[RTX_KAT_NKINDS] = { 16, 11, 11, 13, 3, 16, 9, 11, 3, 1, 6, 7, 17, 9, 19, 2, 25, 21, 28, 26, 37, 26 };
static const int rtx_kat_out_width[RTX_KAT_NKINDS] = { 2, 5, 5, 3, 1, 3, 3, 3, 1, 2, 3, 3, 1, 3, 2, 1, 2, 6, 6, 7, 7332, 7 };
/* KAT_ORDER's output record: 4 header words, order / bucket / x (1024 each), then the kernel's scratch from word
 * RTX_KAT_ORDER_REC on: the shade-point record (24 words), the emitter (64), the material (64), the masks (8) and
 * the wave's slice (4096) */
#define RTX_KAT_ORDER_REC (4 + 3 * 1024)

#endif
