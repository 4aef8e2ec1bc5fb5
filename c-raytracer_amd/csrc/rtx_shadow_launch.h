/*
 * A part of rtx_shadow.hip's translation unit, included there last and not self-contained: the host side
 * of every kernel of that file and of the parts before this one (declared in rtx_launch.h), and k_w8_fill.
 */
#include <type_traits>
#include <utility>

/* the 8-wide BVH's leaf entries: the primitive records they stand for (leafmap[i] = primitive
 * index, RTX_NONE for node entries and holes) */
__global__ void k_w8_fill(const DPrim *__restrict__ prims, const DMaterial *__restrict__ mats, const uint32_t *__restrict__ leafmap,
			  uint32_t n, DW8 *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= 4 * n)
		return;
	const uint32_t e = i >> 2, p = leafmap[e];
	if (p == RTX_NONE)
		return;
	float4 v = ldg4((const char *)(prims + p), 16 * (i & 3));
	if ((i & 3) == 3) { /* the walks' copy: the material's kt in place of the normal, the record index */
		const DMaterial &m = mats[__float_as_uint(prims[p].c[3]) & RTX_META_MAT];
		v = make_float4(m.kt[0], m.kt[1], m.kt[2], __uint_as_float(p));
	}
	((float4 *)(out + e))[i & 3] = v;
}

extern "C" hipError_t rtx_launch_w8_fill(const DPrim *prims, const DMaterial *mats, const uint32_t *leafmap, uint32_t n, DW8 *out,
					  hipStream_t stream)
{
	if (!n)
		return hipSuccess;
	hipLaunchKernelGGL(k_w8_fill, dim3((4 * n + 255) / 256), dim3(256), 0, stream, prims, mats, leafmap, n, out);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_kat_shadow(int kind, uint32_t n, const float *in, float *out, hipStream_t stream)
{
	if (kind < RTX_KAT_FIRST_SHADOW || kind >= RTX_KAT_NKINDS)
		return hipErrorInvalidValue;
	if (kind == RTX_KAT_ORDER) {
		hipLaunchKernelGGL(k_kat_order_fill, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, n, in, out);
		hipLaunchKernelGGL(k_kat_order, dim3(n), dim3(WAVE), 0, stream, n, in, out);
	} else
		hipLaunchKernelGGL(k_kat_shadow, dim3((n + 255) / 256), dim3(256), 0, stream, kind, n, in, out);
	return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* launcher (declared in rtx_launch.h)                                      */
/* ------------------------------------------------------------------------ */
template <bool C, int O, int W, int P> static hipError_t shadow_slots(uint32_t cus, uint32_t *slots)
{
	int per_cu = 0;
	hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(&k_shadow<C, O, W, P>),
								   WAVE * RTX_SH_NW, 0);
	*slots = per_cu > 0 && cus > 0 ? (uint32_t)per_cu * cus : 1024u;
	return e;
}

/* the persistent grid: as many workgroups as are resident on the device at once (no more than
 * the work needs); the waves then share the shade points through RTX_C_SPQUEUE */
template <bool C, int O, int W, int P>
static hipError_t launch_shadow_p(const KShadow &ka, uint32_t nw, uint32_t cus, hipStream_t stream, uint32_t max_wgs)
{
	uint32_t slots = 0;
	hipError_t e = shadow_slots<C, O, W, P>(cus, &slots);
	if (e != hipSuccess)
		return e;
	const uint32_t need = (nw + RTX_SH_NW - 1) / RTX_SH_NW;
	if (ka.ord && max_wgs && slots > max_wgs) /* no more workgroups than the order buffer has slices for */
		slots = max_wgs;
	hipLaunchKernelGGL((k_shadow<C, O, W, P>), dim3(need < slots ? need : slots), dim3(WAVE * RTX_SH_NW), 0, stream, ka);
	return hipGetLastError();
}

/* The k_shadow instances the launcher uses, listed once: launch_walk picks a row, and rtx_shadow_grid_lanes
 * takes the largest grid over all of them.  The product has a kernel per packet layout (k_shadow's PATH), the
 * lane-slot ones capped for RTX_SHADOW_OCC_SLOT; the counting instance keeps both layouts in one kernel (PATH 0)
 * at the compiler's occupancy.  A measurement build (-DRTX_MEASURE=1) adds the product's rows at the compiler's
 * occupancy, launched with RTX_SHADOW_OCC=1 in the environment. */
struct ShadowInst {
	bool count;
	int occ, path;
};
enum { SH_UNI, SH_DARK, SH_ORDER, SH_SLOT, SH_SLOTCULL, SH_LAYOUTS }; /* the layouts, in the order of each block of rows */
constexpr int shadow_slot_occ(int occ) { return occ == RTX_SHADOW_OCC_DEFAULT ? RTX_SHADOW_OCC_SLOT : occ; }
#define RTX_SH_ROWS(O) { false, O, 1 }, { false, O, 4 }, { false, O, 5 }, { false, shadow_slot_occ(O), 2 }, { false, shadow_slot_occ(O), 3 }
static constexpr ShadowInst shadow_insts[] = {
	RTX_SH_ROWS(RTX_SHADOW_OCC_DEFAULT),
#if RTX_MEASURE
	RTX_SH_ROWS(1),
#endif
	{ true, 1, 0 },
};
#undef RTX_SH_ROWS
constexpr size_t SH_NINST = sizeof(shadow_insts) / sizeof(shadow_insts[0]);

/* f(r) for every row r of shadow_insts, r a compile-time constant (shadow_insts[r] can be template arguments) */
template <class F, size_t... I> static void each_shadow_inst(F f, std::index_sequence<I...>)
{
	(f(std::integral_constant<size_t, I>{}), ...);
}
template <class F> static void each_shadow_inst(F f) { each_shadow_inst(f, std::make_index_sequence<SH_NINST>{}); }

template <int W> static hipError_t launch_walk(const KShadow &ka, uint32_t nw, uint32_t cus, int count, hipStream_t stream, uint32_t max_wgs)
{
	size_t row = SH_NINST - 1; /* the counting instance */
	if (!count) {
		if (ka.slot_b == WAVE)
			row = ka.ord ? SH_ORDER : ka.dark ? SH_DARK : SH_UNI;
		else
			row = (W == WALK_W8 && ka.cull_slots && ka.num_cull) ? SH_SLOTCULL : SH_SLOT;
#if RTX_MEASURE
		/* occupancy variant (measurement builds): RTX_SHADOW_OCC = 1 (the compiler's choice) */
		const char *env = getenv("RTX_SHADOW_OCC");
		if (env && atoi(env) != RTX_SHADOW_OCC_DEFAULT)
			row += SH_LAYOUTS;
#endif
	}
	hipError_t e = hipErrorInvalidValue;
	each_shadow_inst([&](auto r) {
		constexpr ShadowInst t = shadow_insts[r];
		if (r == row)
			e = launch_shadow_p<t.count, t.occ, W, t.path>(ka, nw, cus, stream, max_wgs);
	});
	return e;
}

/* the walk k_shadow runs for a scene: the 8-wide BVH when built, else the threaded BVH2 */
static int walk_of(const DScene *S) { return S->w8 ? WALK_W8 : WALK_BVH2; }

/* grid lanes of the largest k_shadow launch on `cus` CUs (sizes the 8-wide walk's spill area): the most
 * workgroups over every row of shadow_insts */
extern "C" hipError_t rtx_shadow_grid_lanes(uint32_t cus, uint32_t *lanes)
{
	hipError_t e = hipSuccess;
	uint32_t most = 0;
	each_shadow_inst([&](auto r) {
		constexpr ShadowInst t = shadow_insts[r];
		uint32_t s = 0;
		if (e == hipSuccess)
			e = shadow_slots<t.count, t.occ, WALK_W8, t.path>(cus, &s);
		most = s > most ? s : most;
	});
	*lanes = most * WAVE * RTX_SH_NW;
	return e;
}

/* the scene's part of k_shadow's arguments (trees, frames, records, the walk's LDS stack size): what
 * rtx_launch_shadow and rtx_launch_shadow_rays share.  Checks what the kernels rely on: the top levels
 * fit their LDS copy, the lane stack its LDS entries, and a deep 8-wide tree has a spill area for
 * the largest grid */
static hipError_t shadow_scene_args(const DScene *S, uint32_t cus, KShadow &ka)
{
	if (S->num_top > RTX_TOP_MAX)
		return hipErrorInvalidValue;
	const int walk = walk_of(S);
	if (walk == WALK_W8 && (S->w8lstk < 1 || S->w8lstk > RTX_W8_STACK))
		return hipErrorInvalidValue;
	if (walk == WALK_W8 && S->w8depth > S->w8lstk + 1) {
		/* deep trees spill lane-stack entries to HBM: the area must cover this launch's grid */
		uint32_t lanes = 0;
		hipError_t e = rtx_shadow_grid_lanes(cus, &lanes);
		if (e != hipSuccess)
			return e;
		if (!S->w8spill || S->w8spill_lanes < lanes)
			return hipErrorInvalidValue;
	}
	ka.recs = (const char *)S->nodes;
	ka.qnodes = S->qnodes;
	ka.top = S->top;
	ka.ntop = S->num_top;
	ka.tf = S->tf;
	for (int a = 0; a < 3; a++) {
		ka.qo[a] = S->qo[a];
		ka.qs[a] = S->qs[a];
		ka.qsi[a] = 1.f / S->qs[a];
	}
	ka.mats = S->mats;
	ka.planes = S->planes;
	ka.emitters = S->emitters;
	ka.have_tree = S->root_ref != RTX_EMPTY_REF && !S->lin && (S->w8 || S->qnodes); /* the walk of walk_of(S) has its tree */
	ka.num_planes = S->num_planes;
	ka.num_emitters = S->num_emitters;
	ka.w8 = S->w8;
	ka.w8s = S->w8s;
	ka.w8spill = S->w8spill;
	ka.w8lstk = S->w8lstk;
	ka.w8top = S->w8top;
	ka.w8sph = S->w8sph;
	ka.lin = S->lin; /* a tiny scene: every bounded object, no walk */
	ka.cull = (const float4 *)S->cull;
	ka.num_cull = (walk == WALK_W8 && S->cull) ? S->num_cull : 0u;
	ka.cull_slots = S->cull_slots;
	ka.point = S->point;
	/* only where shadow rays walk a tree: against a handful of listed objects the predicate costs
	 * more than the tests it saves (scene3, RTX_WALK_LINEAR: 59.9 -> 61.7 ms per frame with it) */
	ka.dark = (S->dark && S->dark_ok && ka.have_tree) ? 1u : 0u;
	ka.spec = S->spec;
	ka.num_lin = S->lin ? S->num_lin : 0u;
	if (walk == WALK_W8) { /* the 8-wide tree's own frame; the emitters it leaves out are tested linearly */
		for (int a = 0; a < 3; a++) {
			ka.qo[a] = S->w8qo[a];
			ka.qs[a] = S->w8qs[a];
			ka.qsi[a] = 1.f / S->w8qs[a];
		}
		ka.lin = S->emitters;
		ka.num_lin = S->w8noemit ? S->num_emitters : 0u;
	}
	/* the listed records' bounding spheres, when they are those of the records this walk lists */
	ka.lsph = (const float4 *)S->lsph;
	ka.num_lsph = (S->lsph && S->num_lsph == ka.num_lin) ? S->num_lsph : 0u;
	return hipSuccess;
}

extern "C" hipError_t rtx_launch_shadow(const DScene *S, const DParams *P, const float4 *sp, const uint32_t *perm,
					uint32_t n_sp, uint32_t per_wave, uint32_t slot_b, float4 *contrib,
					unsigned long long *ctr, int count, uint32_t cus, hipStream_t stream, uint32_t *pmask,
					int *premasked, uint32_t *clbuf, int *clearlane)
{
	if (premasked)
		*premasked = 0;
	if (clearlane)
		*clearlane = 0;
	const uint32_t nw = per_wave ? (n_sp + per_wave - 1) / per_wave : 0u;
	if (!slot_b || (slot_b & (slot_b - 1)) || slot_b > WAVE || !per_wave || per_wave > WAVE)
		return hipErrorInvalidValue;
	if (!nw)
		return hipSuccess;
	KShadow ka;
	hipError_t e = shadow_scene_args(S, cus, ka);
	if (e != hipSuccess)
		return e;
	ka.sp = sp;
	ka.perm = perm;
	ka.contrib = contrib;
	ka.ctr = ctr;
	ka.n_sp = n_sp;
	ka.per_wave = per_wave;
	ka.slot_b = slot_b;
	ka.slot_lg = (uint32_t)__builtin_ctz(slot_b);
	ka.rng = P->rng;
	ka.attenuation = P->attenuation;
	ka.reflection = P->reflection;
	ka.att_offset = P->att_offset;
	/* the points' masks ahead of the kernel (k_point_masks, pmask: a word per record of the chunk): where
	 * k_shadow would form them, one point per wave (the wave-uniform packets), and a byte per mask holds
	 * the emitters; else k_shadow forms them itself */
	/* the sample order: where shadow rays walk a tree, with the waves' slices for this launch's grid */
	ka.ord = nullptr;
	uint32_t ord_wgs = 0; /* the workgroups its buffer has slices for: the grid is held to them */
	if (S->order && slot_b == WAVE && ka.have_tree) {
		if (!S->ordbuf || S->ordbuf_waves < RTX_SH_NW)
			return hipErrorInvalidValue;
		ka.ord = S->ordbuf;
		ord_wgs = S->ordbuf_waves / RTX_SH_NW;
	}
	ka.pm = nullptr;
	if (pmask && slot_b == WAVE && ka.num_emitters <= 8u && (ka.num_cull || ka.point)) {
		hipLaunchKernelGGL(k_point_masks, dim3((n_sp + RTX_PM_BLOCK - 1) / RTX_PM_BLOCK), dim3(RTX_PM_BLOCK), 0, stream, ka, pmask);
		e = hipGetLastError();
		if (e != hipSuccess)
			return e;
		ka.pm = pmask;
		if (premasked)
			*premasked = 1;
	}
	/* RTX_OPT_SHADOW_CLEARLANE: the wave-uniform packets of a render that does not count, their masks formed
	 * above and RTX_OPT_SHADOW_POINT on.  clbuf (rtx_clearlane_words(n_sp) words) takes the processing order
	 * split into the clear list and the rest, then the partition's prefix sums; k_clear_scan leaves the
	 * clear list's length in k_shadow's queue head, so k_shadow, handed the whole array and n_sp as they
	 * are, takes the rest list alone, and k_shadow_clear takes the clear list.  Nothing is read back here. */
	if (S->clearlane && clbuf && ka.pm && ka.point && slot_b == WAVE && !count) {
		const uint32_t nb = (n_sp + RTX_CL_ITEMS - 1) / RTX_CL_ITEMS;
		uint32_t *off = clbuf + n_sp;
		hipLaunchKernelGGL(k_clear_count, dim3(nb), dim3(RTX_CL_BLOCK), 0, stream, ka, off);
		hipLaunchKernelGGL(k_clear_scan, dim3(1), dim3(1024), 0, stream, off, nb, ctr);
		hipLaunchKernelGGL(k_clear_scatter, dim3(nb), dim3(RTX_CL_BLOCK), 0, stream, ka, (const uint32_t *)off, clbuf);
		hipLaunchKernelGGL(k_shadow_clear, dim3((n_sp + RTX_CL_BLOCK - 1) / RTX_CL_BLOCK), dim3(RTX_CL_BLOCK), 0, stream, ka,
				   (const uint32_t *)clbuf);
		e = hipGetLastError();
		if (e != hipSuccess)
			return e;
		ka.perm = clbuf;
		if (clearlane)
			*clearlane = 1;
	}
	if (walk_of(S) == WALK_W8)
		return launch_walk<WALK_W8>(ka, nw, cus, count, stream, ord_wgs);
	return launch_walk<WALK_BVH2>(ka, nw, cus, count, stream, ord_wgs);
}

/* the words of rtx_launch_shadow's clbuf for a chunk of n_sp shade points */
extern "C" size_t rtx_clearlane_words(uint32_t n_sp)
{
	return (size_t)n_sp + (n_sp + RTX_CL_ITEMS - 1) / RTX_CL_ITEMS + 1;
}

/* n caller's shadow rays through shadow_query (k_shadow_rays): the instance follows the scene as
 * rtx_launch_shadow's does (walk_of; a tiny scene's list has no tree), `slots` picks the lane-slot
 * kernels' stack addressing (LA), `count` the counting instance.  ctr: RTX_SQ_N zeroed counters. */
template <bool C, int W, bool LA>
static hipError_t launch_shadow_rays(const KShadow &ka, const float4 *rays, float4 *res, uint32_t n, unsigned long long *ctr,
				     uint32_t cus, uint32_t spill_lanes, hipStream_t stream)
{
	int per_cu = 0;
	hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(&k_shadow_rays<C, W, LA>),
								   WAVE * RTX_SH_NW, 0);
	if (e != hipSuccess)
		return e;
	uint32_t grid = per_cu > 0 && cus > 0 ? (uint32_t)per_cu * cus : 1024u;
	if (spill_lanes) /* no more workgroups than the spill area has lanes for (w8_spill_at) */
		grid = grid < spill_lanes / (WAVE * RTX_SH_NW) ? grid : spill_lanes / (WAVE * RTX_SH_NW);
	const uint32_t need = ((n + WAVE - 1) / WAVE + RTX_SH_NW - 1) / RTX_SH_NW;
	grid = grid < need ? grid : need;
	if (!grid)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_shadow_rays<C, W, LA>), dim3(grid), dim3(WAVE * RTX_SH_NW), 0, stream, ka, rays, res, n, ctr);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_shadow_rays(const DScene *S, const float4 *rays, float4 *res, uint32_t n, unsigned long long *ctr,
					     int slots, int count, uint32_t cus, hipStream_t stream)
{
	if (!n)
		return hipSuccess;
	KShadow ka{};
	hipError_t e = shadow_scene_args(S, cus, ka);
	if (e != hipSuccess)
		return e;
	const uint32_t spill = (walk_of(S) == WALK_W8 && S->w8depth > S->w8lstk + 1) ? S->w8spill_lanes : 0u;
#define RTX_SR(C, W, LA) launch_shadow_rays<C, W, LA>(ka, rays, res, n, ctr, cus, spill, stream)
	if (walk_of(S) == WALK_W8) {
		if (count)
			return slots ? RTX_SR(true, WALK_W8, true) : RTX_SR(true, WALK_W8, false);
		return slots ? RTX_SR(false, WALK_W8, true) : RTX_SR(false, WALK_W8, false);
	}
	/* the BVH2 walk and the listed objects keep no lane stack: LA changes nothing there */
	return count ? RTX_SR(true, WALK_BVH2, false) : RTX_SR(false, WALK_BVH2, false);
#undef RTX_SR
}

/* the code object of this file on the current device, loaded now (rtx_open) rather than at the
 * first launch inside an upload or a render */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_load_shadow(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_w8_fill);
}
