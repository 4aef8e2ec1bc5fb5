/*
 * C-ABI of include/rtx.h, the render (replaces render_init + render, render.c:61-116 / 345-368):
 * a frame, a tile shard, a caller's list of tiles (rtx_render_tiles*) or a caller's primary rays (rtx_render_rays*,
 * rtx_rays_render.cpp) in chunks of tiles through k_trace,
 * the shade-point sort, k_shadow and k_accum, and its statistics.
 */
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_tiles.h"

int rtx_render_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, float *d_rgb, float *d_z,
			 hipStream_t stream, const uint32_t *d_tiles, uint32_t n_tiles, const void *d_prim_rays)
{
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_render before rtx_upload_scene");
	if (!fr || !p)
		return fail(RTX_ERR_ARG, "null frame/params");
	if (!fr->width || !fr->height)
		return fail(RTX_ERR_ARG, "empty frame %ux%u", fr->width, fr->height);
	if (!p->tile_stride || p->tile_offset >= p->tile_stride)
		return fail(RTX_ERR_ARG, "bad tile sharding %u/%u", p->tile_offset, p->tile_stride);
	if (d_tiles && (p->tile_offset != 0 || p->tile_stride != 1))
		return fail(RTX_ERR_ARG, "a tile list takes no tile sharding: %u/%u is not 0/1", p->tile_offset, p->tile_stride);
	const DFrame F = rtx_dframe(fr);
	DParams P;
	memset(&P, 0, sizeof(P));
	P.max_bounces = p->max_bounces;
	P.min_intensity_sqr = p->min_intensity_sqr;
	P.reflection = p->reflection;
	P.gi = p->gi;
	P.samples = p->samples;
	P.attenuation = p->attenuation;
	P.att_offset = p->attenuation_offset;
	P.rng = p->rng;
	P.seed = p->seed;
	P.u32conv = p->u32conv;
	P.tile_offset = p->tile_offset;
	P.tile_stride = p->tile_stride;
	P.tiles_x = (fr->width + RTX_TILE_W - 1) / RTX_TILE_W;
	const uint64_t tiles_y = (fr->height + RTX_TILE_H - 1) / RTX_TILE_H;
	const uint64_t total = (uint64_t)P.tiles_x * tiles_y;
	P.ntiles = p->tile_offset < total ? (uint32_t)((total - p->tile_offset + p->tile_stride - 1) / p->tile_stride) : 0;
	if (d_tiles) /* a tile list (checked by the caller): the chunks run over list positions */
		P.ntiles = n_tiles;

	int per_cu = 0;
	HIP_TRY(rtx_trace_occupancy(c->scene.stack_size, &per_cu));
	if (per_cu <= 0)
		return fail(RTX_ERR_HIP, "trace kernel does not fit (LDS %zu B)", rtx_trace_lds_bytes(c->scene.stack_size));
	const uint32_t waves = (uint32_t)std::min<uint64_t>((uint64_t)per_cu * c->cus, std::max<uint32_t>(P.ntiles, 1));
	/* LIFO task stack: each batch pops <= 64 and pushes <= 128, depth <= max_bounces */
	if (P.max_bounces > RTX_MAX_BOUNCES)
		return fail(RTX_ERR_ARG, "max_bounces %u above the supported %u", P.max_bounces, RTX_MAX_BOUNCES);
	const uint32_t mb = P.max_bounces;
	const uint32_t task_cap = 64u * (mb + 3u);
	/* shade points per tile: 64 px x (primary + GI samples) + secondary-ray allowance */
	const uint64_t gi_n = P.gi == RTX_GI_PATH ? (uint64_t)P.samples : 0u;
	uint64_t staging_cap = 64ull * (1 + gi_n) + 64ull * 4 * std::min<uint32_t>(mb, 16u) * (gi_n ? 2 : 1) + 64;
	uint64_t avg_tile = 64ull * (1 + gi_n) * 5 / 4 + 64;
	/* a render of the same scene and settings before: its shade points per tile (x 1.25, + 64)
	 * instead of the bound above; an overflow still halves the chunk and retries */
	/* every setting the shade points per tile depend on: the scene (reset by an upload), the
	 * frame and camera, the ray-tree and GI settings and the shard */
	SpKey sp_key{};
	sp_key.v[0] = (uint32_t)P.gi;
	sp_key.v[1] = P.samples;
	sp_key.v[2] = P.max_bounces;
	sp_key.v[3] = (uint32_t)P.reflection;
	sp_key.v[4] = P.tile_offset;
	sp_key.v[5] = P.tile_stride;
	sp_key.v[6] = F.width;
	sp_key.v[7] = F.height;
	memcpy(&sp_key.v[8], &P.min_intensity_sqr, 4);
	memcpy(&sp_key.v[9], F.corner, 12);
	memcpy(&sp_key.v[12], F.step_x, 12);
	memcpy(&sp_key.v[15], F.step_y, 12);
	memcpy(&sp_key.v[18], F.origin, 12);
	sp_key.set = 1;
	/* a ray batch (rtx_render_rays*) has no camera to key the estimate with: it neither reads nor writes it */
	if (!d_prim_rays && c->sp_tile_key == sp_key && c->sp_tile_seen > 0.0)
		avg_tile = std::min<uint64_t>(avg_tile, (uint64_t)(c->sp_tile_seen * 1.25) + 64);
	if (c->opt_sp_tile) /* RTX_OPT_SP_PER_TILE: tests drive the overflow path with a low figure */
		avg_tile = c->opt_sp_tile;
	size_t free_b = 0, total_b = 0;
	HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	/* shade points of a chunk: up to a third of free HBM (96 GB cap; 288 GB per MI355X), shared
	 * out among the contexts rendering on this device at once (rtx_group_open_loopback) */
	const uint64_t budget = std::min<uint64_t>(96ull << 30, free_b / 3) / std::max<uint32_t>(c->mem_share, 1u);
	/* 128 B per shade point: its record (96), its light term (16) and its sort keys / values (16) */
	uint32_t chunk_cap = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(P.ntiles, budget / (avg_tile * 128)));
	if (c->opt_chunk) /* RTX_OPT_CHUNK_TILES */
		chunk_cap = std::min(chunk_cap, c->opt_chunk);
	uint32_t chunk_tiles = chunk_cap;

	HIP_TRY(c->d_tasks.grow((size_t)waves * task_cap * sizeof(DTask)));
	HIP_TRY(rtx_ensure_ostk(c, waves)); /* the closest-hit stack entries beyond the LDS part */
	c->scene.trace_w8 = (c->scene.w8 && c->opt_trace_walk != RTX_WALK_BVH2) ? 1u : 0u;
	/* RTX_OPT_TRACE_PACK: path GI on the 8-wide tree takes the packed instances, a region per wave */
	const uint32_t pack_seg = c->opt_trace_pack == 1 ? RTX_TRACE_PACK_SEG : c->opt_trace_pack;
	const bool pack = pack_seg && c->scene.trace_w8 && P.gi == RTX_GI_PATH;
	if (pack)
		HIP_TRY(c->d_pack.grow((size_t)waves * rtx_trace_pack_bytes(pack_seg)));
	c->stats.trace_walk = c->scene.trace_w8 ? RTX_WALK_W8 : RTX_WALK_BVH2;
	HIP_TRY(rtx_ensure_w8spill(c, c->scene));

	HIP_TRY(hipEventRecord(c->ev0, stream));
	double t_trace = 0, t_sort = 0, t_shadow = 0, t_accum = 0;
	uint64_t shade_points = 0, premask_points = 0;
	uint32_t chunks = 0;
	unsigned long long tot[RTX_C_N] = {}; /* counters of the chunks that completed */
	/* shadow kernel: lane slots of slot_b = pow2ceil(lights) (<= 64) lanes per point; ~16 packets per wave */
	uint32_t slot_b = 1;
	while (slot_b < 64 && slot_b < c->total_lights)
		slot_b <<= 1;
	{
		/* a point's lanes in slots of pow2ceil(lights) (one point per 64-lane packet from 64 lights
		 * up) leave lanes idle when the count is awkward (100 lights: 64 + 36 of 128 lanes); below
		 * 90 % use, points take consecutive 4-lane slots and straddle packets instead (k_shadow
		 * sums a point's slots in slot order, so the result does not depend on its neighbours) */
		const uint32_t n = std::max<uint32_t>(c->total_lights, 1);
		const uint32_t used = slot_b * ((n + slot_b - 1) / slot_b);
		if (n > 4 && (double)n / used < 0.9)
			slot_b = 4;
	}
	if (c->opt_slot) /* RTX_OPT_SHADOW_SLOT */
		slot_b = c->opt_slot;
	const uint32_t slots_per_point = (std::max<uint32_t>(c->total_lights, 1) + slot_b - 1) / slot_b;
	const uint32_t grab = c->opt_grab; /* lane slots per k_shadow queue grab (1024 -> 4096: 903 -> 885 ms) */
	const uint32_t per_wave = std::max<uint32_t>(1, std::min<uint32_t>(64, grab / (slot_b * slots_per_point)));
	const bool spsort = c->opt_spsort;
	bool overflowed = false; /* a chunk of this frame overflowed the shade-point array */
	for (uint32_t begin = 0; begin < P.ntiles;) {
		const uint32_t end = std::min<uint32_t>(P.ntiles, begin + chunk_tiles);
		const uint64_t sp_cap64 = std::min<uint64_t>((uint64_t)(end - begin) * avg_tile + staging_cap, 0xFFFFFFF0ull);
		const uint32_t sp_cap = (uint32_t)sp_cap64;
		HIP_TRY(c->d_staging.grow((size_t)waves * staging_cap * 6 * sizeof(float4)));
		HIP_TRY(c->d_sp.grow((size_t)sp_cap * 6 * sizeof(float4)));
		HIP_TRY(c->d_contrib.grow((size_t)sp_cap * sizeof(float4)));
		if (c->opt_premask) /* 4 B per point beside the 128 budgeted above, out of the two thirds of HBM left free */
			HIP_TRY(c->d_pmask.grow((size_t)sp_cap * sizeof(uint32_t)));
		HIP_TRY(c->d_tile_rec.grow((size_t)(end - begin) * sizeof(uint2)));
		HIP_TRY(hipMemsetAsync(c->d_ctr, 0, sizeof(unsigned long long) * RTX_C_N, stream));
		HIP_TRY(hipEventRecord(c->ev[0], stream));
		HIP_TRY(rtx_launch_trace(&c->scene, &F, &P, d_rgb, d_z, c->d_tasks, task_cap, c->d_staging,
					 (uint32_t)staging_cap, c->d_sp, sp_cap, c->d_tile_rec, begin, end, c->d_ctr,
					 std::min<uint32_t>(waves, end - begin), p->count_traversal, d_tiles,
					 pack ? (void *)c->d_pack : nullptr, pack_seg, (const float4 *)d_prim_rays, stream));
		HIP_TRY(hipEventRecord(c->ev[1], stream));
		unsigned long long head[RTX_C_N];
		HIP_TRY(hipMemcpyAsync(head, c->d_ctr, sizeof(head), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		if (head[RTX_C_TASKOVERFLOW])
			return fail(RTX_ERR_STATE, "reflection/refraction task stack overflow (%u entries per wave)", task_cap);
		if (head[RTX_C_OVERFLOW]) {
			if (staging_cap >= (1ull << 26))
				return fail(RTX_ERR_STATE, "shade-point staging overflow (%llu shade points per tile)",
					    (unsigned long long)staging_cap);
			staging_cap *= 2; /* retry the chunk (counters reset) with room for larger ray trees */
			continue;
		}
		if (head[RTX_C_SPOVERFLOW]) {
			if (end - begin == 1)
				return fail(RTX_ERR_STATE, "shade-point array overflow on a single tile");
			chunk_tiles = std::max<uint32_t>(1, (end - begin) / 2);
			overflowed = true;
			continue;
		}
		const uint32_t n_sp = (uint32_t)head[RTX_C_SPCOUNT];
		shade_points += n_sp;
		/* shade points in Morton order of their position (rtx_sort.hip); RTX_SPSORT=0 keeps
		 * emission order (same image, bit for bit) */
		const uint32_t *perm = nullptr;
		if (n_sp > 1 && c->scene.root_ref != RTX_EMPTY_REF && spsort) {
			/* keys and values (two ping-pong buffers each) sized for the chunk's capacity, like the
			 * shade-point array: a later render with more points per chunk (its chunks sized from
			 * this one's count) then reuses them instead of reallocating inside its frame */
			size_t tmp = 0;
			const size_t cap = std::max<size_t>(n_sp, c->d_sp.bytes / (6 * sizeof(float4)));
			HIP_TRY(rtx_spsort_temp_bytes((uint32_t)std::min<size_t>(cap, 0xFFFFFFF0u), &tmp));
			HIP_TRY(c->d_sortbuf.grow(cap * 4 * sizeof(uint32_t)));
			HIP_TRY(c->d_sorttmp.grow(tmp));
			const size_t q = c->d_sortbuf.bytes / (4 * sizeof(uint32_t)); /* the buffer's capacity in points */
			uint32_t *b = c->d_sortbuf;
			HIP_TRY(rtx_launch_spsort(c->d_sp, n_sp, c->bound_lo, c->bound_hi, b, b + q, b + 2 * q, b + 3 * q, c->d_sorttmp,
						  c->d_sorttmp.bytes, &perm, stream));
		}
		HIP_TRY(hipEventRecord(c->ev[4], stream));
		DScene Ssh = c->scene; /* RTX_OPT_SHADOW_CULL: 0 no cull spheres, 2 the lane slots cull too */
		if (!c->opt_cull)
			Ssh.num_cull = 0;
		Ssh.cull_slots = c->opt_cull == 2 ? 1u : 0u;
		Ssh.point = (c->opt_cull && c->opt_point) ? 1u : 0u; /* RTX_OPT_SHADOW_POINT */
		Ssh.dark = (c->opt_cull && c->opt_dark) ? 1u : 0u;   /* RTX_OPT_SHADOW_DARK */
		Ssh.spec = c->opt_spec ? 1u : 0u;                    /* RTX_OPT_SHADOW_SPEC */
		/* RTX_OPT_SHADOW_ORDER: wave-uniform packets that walk a tree, the waves' slices for the largest grid */
		Ssh.order = 0u;
		Ssh.ordbuf = nullptr;
		Ssh.ordbuf_waves = 0u;
		if (c->opt_order && slot_b == 64 && Ssh.root_ref != RTX_EMPTY_REF && !Ssh.lin) {
			uint32_t lanes = 0;
			HIP_TRY(rtx_shadow_grid_lanes((uint32_t)c->cus, &lanes));
			HIP_TRY(c->d_ordbuf.grow((size_t)(lanes / 64) * RTX_ORD_WORDS * sizeof(uint32_t)));
			Ssh.order = 1u;
			Ssh.ordbuf = c->d_ordbuf;
			Ssh.ordbuf_waves = lanes / 64;
		}
		/* RTX_OPT_SHADOW_CLEARLANE: where the launch can take it (the masks formed ahead, wave-uniform packets, no
		 * counting), 4 B per point more for the split processing order */
		Ssh.clearlane = 0u;
		if (c->opt_clearlane && c->opt_premask && Ssh.point && slot_b == 64 && !p->count_traversal && n_sp) {
			HIP_TRY(c->d_clbuf.grow(rtx_clearlane_words((uint32_t)std::max<size_t>(n_sp, c->d_sp.bytes / (6 * sizeof(float4)))) *
						sizeof(uint32_t)));
			Ssh.clearlane = 1u;
		}
		int premasked = 0; /* RTX_OPT_SHADOW_PREMASK: k_point_masks ran for this chunk */
		int clearlane = 0; /* ... and k_shadow_clear */
		HIP_TRY(rtx_launch_shadow(&Ssh, &P, c->d_sp, perm, n_sp, per_wave, slot_b, c->d_contrib, c->d_ctr,
					  p->count_traversal, (uint32_t)c->cus, stream, c->opt_premask ? c->d_pmask : nullptr,
					  &premasked, Ssh.clearlane ? (uint32_t *)c->d_clbuf : nullptr, &clearlane));
		if (premasked)
			premask_points += n_sp;
		HIP_TRY(hipEventRecord(c->ev[2], stream));
		HIP_TRY(rtx_launch_accum(&F, &P, c->d_tile_rec, c->d_contrib, begin, end - begin, d_rgb, d_tiles, stream));
		HIP_TRY(hipEventRecord(c->ev[3], stream));
		unsigned long long ctr[RTX_C_N];
		HIP_TRY(hipMemcpyAsync(ctr, c->d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipStreamSynchronize(stream));
		for (int k = RTX_C_CLOSEST; k < RTX_C_N; k++)
			tot[k] += ctr[k];
		float a = 0, b = 0, cc = 0, so = 0;
		HIP_TRY(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
		HIP_TRY(hipEventElapsedTime(&so, c->ev[1], c->ev[4]));
		HIP_TRY(hipEventElapsedTime(&b, c->ev[4], c->ev[2]));
		HIP_TRY(hipEventElapsedTime(&cc, c->ev[2], c->ev[3]));
		t_trace += a;
		t_sort += so;
		t_shadow += b;
		t_accum += cc;
		chunks++;
		begin = end;
		/* a chunk an overflow halved grows back by a quarter per chunk that fits, so a dense region of
		 * the image does not overflow (and re-trace) every other chunk */
		if (overflowed)
			chunk_tiles = std::min<uint32_t>(chunk_cap, chunk_tiles + std::max<uint32_t>(1, chunk_tiles / 4));
	}
	HIP_TRY(hipEventRecord(c->ev1, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	/* a list render reads the estimate (the whole frame's settings key it) and leaves it as it is */
	if (P.ntiles && !d_tiles && !d_prim_rays) {
		c->sp_tile_seen = (double)shade_points / P.ntiles;
		c->sp_tile_key = sp_key;
	}
	const unsigned long long *ctr = tot;
	rtx_stats &st = c->stats;
	st.closest_rays = ctr[RTX_C_CLOSEST];
	st.shadow_rays = ctr[RTX_C_SHADOW] + ctr[RTX_C_CLRAYS]; /* k_shadow_clear counts its points' rays apart */
	/* the threaded walk counts box tests; a node visit is a BVH2 inner node (two box tests) */
	st.shadow_node_visits = ctr[RTX_C_SBOXES] / 2;
	st.shadow_tri_tests = ctr[RTX_C_STRIS];
	st.shadow_sphere_tests = ctr[RTX_C_SSPHERES];
	st.shadow_plane_tests = ctr[RTX_C_SPLANES];
	st.shadow_box_tests = ctr[RTX_C_SBOXES];
	st.shadow_global_box_tests = ctr[RTX_C_SGBOXES];
	st.shadow_wave_steps = ctr[RTX_C_SSTEPS];
	st.shadow_wave_walks = ctr[RTX_C_SWALKS];
	st.shadow_leaf_rounds = ctr[RTX_C_SLEAFR];
	st.shadow_uniform_steps = ctr[RTX_C_SUNIF];
	st.far_closest_rays = ctr[RTX_C_FARC];
	st.far_shadow_rays = ctr[RTX_C_FARS];
	st.shadow_stack_spills = ctr[RTX_C_SSPILL];
	st.shadow_cone_clear = ctr[RTX_C_SCLEAR];
	c->pstats.shadow_plane_skipped = ctr[RTX_C_SPSKIP];
	c->pstats.shadow_lin_skipped = ctr[RTX_C_SLSKIP];
	c->pstats.shadow_point_clear = ctr[RTX_C_SPCLEAR];
	c->dstats.shadow_dark_rays = ctr[RTX_C_SDARK];
	c->dstats.shadow_dark_packet_rays = ctr[RTX_C_SDARKPK];
	c->ostats.shadow_ordered_points = ctr[RTX_C_SORDPT];
	c->ostats.shadow_ordered_rays = ctr[RTX_C_SORDRAY];
	c->mstats.premask_points = premask_points;
	c->cstats.clear_points = ctr[RTX_C_CLPTS];
	c->cstats.clear_rays = ctr[RTX_C_CLRAYS];
	st.node_visits = ctr[RTX_C_NODES] + st.shadow_node_visits;
	st.tri_tests = ctr[RTX_C_TRIS] + ctr[RTX_C_STRIS];
	st.sphere_tests = ctr[RTX_C_SPHERES] + ctr[RTX_C_SSPHERES];
	st.plane_tests = ctr[RTX_C_PLANES] + ctr[RTX_C_SPLANES];
	st.shade_points = shade_points;
	st.kernel_ms = t_trace + t_sort + t_shadow + t_accum;
	st.sort_ms = t_sort;
	st.trace_ms = t_trace;
	st.shadow_ms = t_shadow;
	st.accum_ms = t_accum;
	st.waves = waves;
	st.chunks = chunks;
	return RTX_OK;
}

extern "C" int rtx_render_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, void *d_rgb, void *d_z,
				 void *stream)
{
	if (!c)
		return fail(RTX_ERR_ARG, "null context");
	HIP_TRY(hipSetDevice(c->device));
	return rtx_render_common(c, fr, p, (float *)d_rgb, (float *)d_z, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int rtx_render(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, float *rgb, float *z)
{
	if (!c || !fr || !p)
		return fail(RTX_ERR_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	/* pixels of tiles outside this shard keep the caller's values */
	if (p->tile_stride > 1) {
		if (rgb)
			HIP_TRY(hipMemcpyAsync(c->d_rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
		if (z)
			HIP_TRY(hipMemcpyAsync(c->d_z, z, px * 4, hipMemcpyHostToDevice, c->stream));
	}
	int rc = rtx_render_common(c, fr, p, rgb ? c->d_rgb : nullptr, z ? c->d_z : nullptr, c->stream);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* a host tile list: strictly increasing, every index below the frame's tile count */
static int tile_list_check(const rtx_frame *fr, const uint32_t *tiles, uint32_t n_tiles)
{
	const uint64_t total = rtx_tiles_total(fr->width, fr->height);
	for (uint32_t i = 0; i < n_tiles; i++) {
		if (tiles[i] >= total)
			return fail(RTX_ERR_ARG, "tile list entry %u: tile %u of %llu", i, tiles[i], (unsigned long long)total);
		if (i && tiles[i - 1] >= tiles[i])
			return fail(RTX_ERR_ARG, "tile list entry %u: %u after %u is not strictly increasing", i, tiles[i], tiles[i - 1]);
	}
	return RTX_OK;
}

/* what both tile-list entries refuse before they look at the list */
static int tiles_args_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const void *tiles, uint32_t n_tiles)
{
	if (!c || !fr || !p)
		return fail(RTX_ERR_ARG, "null argument");
	if (!c->have_scene)
		return fail(RTX_ERR_STATE, "rtx_render_tiles before rtx_upload_scene");
	if (!fr->width || !fr->height)
		return fail(RTX_ERR_ARG, "empty frame %ux%u", fr->width, fr->height);
	if (p->tile_offset != 0 || p->tile_stride != 1)
		return fail(RTX_ERR_ARG, "a tile list takes no tile sharding: %u/%u is not 0/1", p->tile_offset, p->tile_stride);
	if (n_tiles && !tiles)
		return fail(RTX_ERR_ARG, "null tile list of %u tiles", n_tiles);
	if (n_tiles > rtx_tiles_total(fr->width, fr->height))
		return fail(RTX_ERR_ARG, "%u tiles listed of a frame of %llu", n_tiles,
			    (unsigned long long)rtx_tiles_total(fr->width, fr->height));
	return RTX_OK;
}

/* no tile: nothing is launched, and the statistics describe a render of nothing */
static int render_no_tiles(rtx_ctx *c)
{
	const uint32_t walk = c->stats.trace_walk;
	c->stats = rtx_stats{};
	c->stats.trace_walk = walk;
	c->pstats = rtx_point_stats{};
	c->dstats = rtx_dark_stats{};
	c->ostats = rtx_order_stats{};
	c->mstats = rtx_premask_stats{};
	c->cstats = rtx_clearlane_stats{};
	return RTX_OK;
}

extern "C" int rtx_render_tiles_device(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const void *d_tiles, uint32_t n_tiles,
				       void *d_rgb, void *d_z, void *stream)
{
	int rc = tiles_args_check(c, fr, p, d_tiles, n_tiles);
	if (rc)
		return rc;
	if ((uintptr_t)d_tiles & 3u)
		return fail(RTX_ERR_ARG, "the tile list must be 4-byte aligned");
	if (!n_tiles)
		return render_no_tiles(c);
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = stream ? (hipStream_t)stream : c->stream;
	/* one lane per entry raises a flag word, read back before anything else is launched */
	HIP_TRY(c->d_tile_flag.grow(sizeof(uint32_t)));
	HIP_TRY(hipMemsetAsync(c->d_tile_flag, 0, sizeof(uint32_t), st));
	HIP_TRY(rtx_launch_tiles_check((const uint32_t *)d_tiles, n_tiles, (uint32_t)rtx_tiles_total(fr->width, fr->height),
				       c->d_tile_flag, st));
	uint32_t flag = 0;
	HIP_TRY(hipMemcpyAsync(&flag, c->d_tile_flag, sizeof(flag), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (flag)
		return fail(RTX_ERR_ARG, "the tile list is not strictly increasing below the frame's %llu tiles",
			    (unsigned long long)rtx_tiles_total(fr->width, fr->height));
	return rtx_render_common(c, fr, p, (float *)d_rgb, (float *)d_z, st, (const uint32_t *)d_tiles, n_tiles);
}

extern "C" int rtx_render_tiles(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const uint32_t *tiles, uint32_t n_tiles,
				float *rgb, float *z)
{
	int rc = tiles_args_check(c, fr, p, tiles, n_tiles);
	if (rc)
		return rc;
	rc = tile_list_check(fr, tiles, n_tiles);
	if (rc)
		return rc;
	if (!n_tiles)
		return render_no_tiles(c);
	HIP_TRY(hipSetDevice(c->device));
	const size_t px = (size_t)fr->width * fr->height;
	HIP_TRY(rtx_ensure_framebuffer(c, px));
	HIP_TRY(c->d_tile_list.grow((size_t)n_tiles * sizeof(uint32_t)));
	HIP_TRY(hipMemcpyAsync(c->d_tile_list, tiles, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	/* pixels of tiles outside the list keep the caller's values */
	if (n_tiles < rtx_tiles_total(fr->width, fr->height)) {
		if (rgb)
			HIP_TRY(hipMemcpyAsync(c->d_rgb, rgb, px * 12, hipMemcpyHostToDevice, c->stream));
		if (z)
			HIP_TRY(hipMemcpyAsync(c->d_z, z, px * 4, hipMemcpyHostToDevice, c->stream));
	}
	rc = rtx_render_common(c, fr, p, rgb ? c->d_rgb : nullptr, z ? c->d_z : nullptr, c->stream, c->d_tile_list, n_tiles);
	if (rc)
		return rc;
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c->d_rgb, px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c->d_z, px * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}
