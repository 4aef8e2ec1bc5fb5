/*
 * A part of rtx_trace.hip's translation unit, included there once and not self-contained: the host launch code
 * of every kernel of the unit (declared in rtx_launch.h), its LDS sizes and occupancy queries.
 */
/* ------------------------------------------------------------------------ */
/* launchers (declared in rtx_launch.h)                                     */
/* ------------------------------------------------------------------------ */
extern "C" size_t rtx_trace_lds_bytes(uint32_t stack_size)
{
	size_t pad = 0;
#if RTX_MEASURE
	/* RTX_TRACE_LDS_PAD (measurement builds): extra bytes per wave, to read k_trace's occupancy slope */
	const char *e = getenv("RTX_TRACE_LDS_PAD");
	pad = e ? (size_t)atoi(e) : 0;
#endif
	const size_t lstk = stack_size < RTX_TRACE_LSTK ? stack_size : RTX_TRACE_LSTK;
	return (size_t)WAVE * SPW * 4 + 80 * 4 + lstk * WAVE * 4 + pad;
}

extern "C" size_t rtx_trace_pack_bytes(uint32_t pack_seg)
{
	return (size_t)pack_seg * RTX_PACK_BYTES;
}

extern "C" hipError_t rtx_trace_occupancy(uint32_t stack_size, int *blocks_per_cu)
{
	return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_trace<false, false, false>, WAVE,
							     rtx_trace_lds_bytes(stack_size));
}

/* One k_trace instance's launch.  Every instance takes rtx_launch_trace's own arguments, so the launcher picks
 * one from a table by its flags and the kernel's argument list is written once. */
template <bool C, bool L, bool K, bool R>
static hipError_t launch_trace(const DScene *S, const DFrame *F, const DParams *P, float *rgb, float *z, DTask *tasks,
			       uint32_t task_cap, float4 *staging, uint32_t staging_cap, float4 *sp_out, uint32_t sp_cap,
			       uint2 *tile_rec, uint32_t tile_begin, uint32_t tile_end, unsigned long long *ctr, uint32_t waves,
			       int count, const uint32_t *tile_list, void *pack, uint32_t pack_seg, const float4 *prim_rays,
			       hipStream_t stream)
{
	PrimaryRays<R> pr{};
	TileList<L> tl{};
	TracePack<K> pk{};
	if constexpr (R)
		pr.p = prim_rays;
	if constexpr (L)
		tl.p = tile_list;
	if constexpr (K) {
		pk.buf = (unsigned char *)pack;
		pk.seg = pack_seg;
	}
	hipLaunchKernelGGL((k_trace<C, L, K, R>), dim3(waves), dim3(WAVE), rtx_trace_lds_bytes(S->stack_size), stream, *S, *F, *P,
			   rgb, z, tasks, task_cap, staging, staging_cap, sp_out, sp_cap, pr, tile_rec, tile_begin, tile_end, ctr, tl,
			   pk);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_trace(const DScene *S, const DFrame *F, const DParams *P, float *rgb, float *z,
				       DTask *tasks, uint32_t task_cap, float4 *staging, uint32_t staging_cap,
				       float4 *sp_out, uint32_t sp_cap, uint2 *tile_rec, uint32_t tile_begin,
				       uint32_t tile_end, unsigned long long *ctr, uint32_t waves, int count,
				       const uint32_t *tile_list, void *pack, uint32_t pack_seg, const float4 *prim_rays,
				       hipStream_t stream)
{
	if (pack && (!S->trace_w8 || !pack_seg || pack_seg % WAVE)) /* the packed instances walk the 8-wide tree alone */
		return hipErrorInvalidValue;
	if (prim_rays && tile_list) /* a ray batch (rtx_render_rays*): the whole image or a shard, never a tile list */
		return hipErrorInvalidValue;
	/* The twelve instances <count, list, pack, rays>.  Their order here is the order the compiler lays the kernels
	 * out in, and their code holds pc-relative addresses of the unit's constant tables: another order changes
	 * the bytes of every kernel that moves.  So the table keeps the order the kernels have had: ray batches by
	 * pack, then count; tile lists and then arithmetic shards by count, then pack; the set one first. */
	static constexpr decltype(&rtx_launch_trace) inst[12] = {
		launch_trace<true, false, true, true>,   launch_trace<false, false, true, true>,
		launch_trace<true, false, false, true>,  launch_trace<false, false, false, true>,
		launch_trace<true, true, true, false>,   launch_trace<true, true, false, false>,
		launch_trace<false, true, true, false>,  launch_trace<false, true, false, false>,
		launch_trace<true, false, true, false>,  launch_trace<true, false, false, false>,
		launch_trace<false, false, true, false>, launch_trace<false, false, false, false>,
	};
	const int c = !count, k = !pack;
	return inst[prim_rays ? 2 * k + c : (tile_list ? 4 : 8) + 2 * c + k](
		S, F, P, rgb, z, tasks, task_cap, staging, staging_cap, sp_out, sp_cap, tile_rec, tile_begin, tile_end, ctr, waves,
		count, tile_list, pack, pack_seg, prim_rays, stream);
}

extern "C" hipError_t rtx_launch_accum(const DFrame *F, const DParams *P, const uint2 *tile_rec,
				       const float4 *contrib, uint32_t tile_begin, uint32_t ntiles, float *rgb,
				       const uint32_t *tile_list, hipStream_t stream)
{
	if (!ntiles || !rgb)
		return hipSuccess;
	if (tile_list)
		hipLaunchKernelGGL(k_accum<true>, dim3(ntiles), dim3(WAVE), 0, stream, *F, *P, tile_rec, contrib, tile_begin, rgb,
				   TileList<true>{ tile_list });
	else
		hipLaunchKernelGGL(k_accum<false>, dim3(ntiles), dim3(WAVE), 0, stream, *F, *P, tile_rec, contrib, tile_begin, rgb,
				   TileList<false>{});
	return hipGetLastError();
}

/* k_rays keeps only the closest walk's LDS lane-stack entries */
extern "C" size_t rtx_rays_lds_bytes(uint32_t stack_size)
{
	const size_t lstk = stack_size < RTX_TRACE_LSTK ? stack_size : RTX_TRACE_LSTK;
	return lstk * WAVE * 4;
}

extern "C" hipError_t rtx_rays_occupancy(uint32_t stack_size, int *blocks_per_cu)
{
	return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_rays<false, false>, WAVE,
							     rtx_rays_lds_bytes(stack_size));
}

template <bool C, bool A>
static hipError_t launch_rays(const DScene *S, const float4 *rays, float4 *hits, const uint32_t *perm, uint32_t n, uint32_t queues,
			      uint32_t grab, unsigned long long *ctr, uint32_t waves, int count, int any, hipStream_t stream)
{
	hipLaunchKernelGGL((k_rays<C, A>), dim3(waves), dim3(WAVE), rtx_rays_lds_bytes(S->stack_size), stream, *S, rays, hits, perm,
			   n, queues, grab, ctr);
	return hipGetLastError();
}

/* S->ostk must hold waves * 64 * (stack_size - RTX_TRACE_LSTK) entries: this launch's own grid */
extern "C" hipError_t rtx_launch_rays(const DScene *S, const float4 *rays, float4 *hits, const uint32_t *perm, uint32_t n,
				      uint32_t queues, uint32_t grab, unsigned long long *ctr, uint32_t waves, int count, int any,
				      hipStream_t stream)
{
	/* [no count][not any], in the order the kernels are laid out in (rtx_launch_trace has the reason) */
	static constexpr decltype(&rtx_launch_rays) inst[2][2] = { { launch_rays<true, true>, launch_rays<true, false> },
								   { launch_rays<false, true>, launch_rays<false, false> } };
	return inst[!count][!any](S, rays, hits, perm, n, queues, grab, ctr, waves, count, any, stream);
}

extern "C" hipError_t rtx_launch_frame_rays(const DFrame *F, float4 *rays, hipStream_t stream)
{
	const uint64_t n = (uint64_t)F->width * F->height;
	hipLaunchKernelGGL(k_frame_rays, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, *F, rays);
	return hipGetLastError();
}

extern "C" hipError_t rtx_launch_kat(int kind, uint32_t n, const float *in, float *out, int u32mode,
				     hipStream_t stream)
{
	hipLaunchKernelGGL(k_kat, dim3((n + 255) / 256), dim3(256), 0, stream, kind, n, in, out, u32mode);
	return hipGetLastError();
}

/* the code object of this file on the current device, loaded now (rtx_open) rather than at the
 * first launch inside an upload or a render */
extern "C" __attribute__((visibility("hidden"))) hipError_t rtx_load_trace(void)
{
	hipFuncAttributes a;
	return hipFuncGetAttributes(&a, (const void *)k_accum<false>);
}
