/*
 * Library-internal declarations shared by the host files of the C-ABI: rtx_ctx.cpp (context,
 * options, statistics), rtx_scene.cpp (flattening, BVH builds), rtx_upload.cpp, rtx_render.cpp,
 * rtx_query.cpp (ray and shadow queries), rtx_nearest.cpp (closest-point queries), rtx_image.cpp (postprocess, feature buffers, denoiser),
 * rtx_passes.cpp (multi-pass rendering, adaptive passes), rtx_upsample.cpp (feature-guided upsampling), rtx_temporal.cpp (temporal accumulation), rtx_group.cpp (multi-device) and rtx_group_passes.cpp (multi-pass rendering on a group).  The device context, its scratch buffers' owner type, a
 * host-built scene, and the steps more than one of the files takes.
 * Not installed; nothing outside librtx includes it.
 */
#ifndef RTX_INTERNAL_H
#define RTX_INTERNAL_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtx.h"
#include "rtx_device.h"
#include "rtx_launch.h"

/* sets the calling thread's rtx_last_error() message, returns code */
int rtx_fail(int code, const char *fmt, ...);
#define fail rtx_fail

#define HIP_TRY(expr)                                                                                   \
	do {                                                                                            \
		hipError_t e_ = (expr);                                                                 \
		if (e_ != hipSuccess)                                                                   \
			return fail(RTX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
	} while (0)

template <class T> static inline void dfree(T *&p)
{
	if (p)
		(void)hipFree(p);
	p = nullptr;
}

/* Device scratch and its owner: the pointer and its capacity in bytes.  It only grows, converts
 * to its pointer where a launcher or a copy takes one, and is freed with whatever holds it: a
 * context (rtx_ctx's grow-only work buffers), or a scope (a build's temporaries, freed on every
 * exit).  The device it was allocated on must be current when it is freed. */
template <class T> struct RTX_HIDDEN DevBuf {
	T *p = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	~DevBuf() { dfree(p); }
	/* room for `need` bytes; the contents do not survive a growth, and a failed one leaves the
	 * buffer empty with capacity 0, so no later, smaller request takes a null pointer for room */
	hipError_t grow(size_t need)
	{
		if (need <= bytes)
			return hipSuccess;
		dfree(p);
		bytes = 0;
		const hipError_t e = hipMalloc(&p, need);
		if (e == hipSuccess)
			bytes = need;
		else
			p = nullptr;
		return e;
	}
	operator T *() const { return p; }
};

/* a host vector into a fresh device buffer, copied on `stream` (the context's own: no
 * synchronisation with the null stream) and complete on return */
template <class T> static inline int upload(T *&dst, const std::vector<T> &v, hipStream_t stream)
{
#if RTX_MEASURE
	const auto t0 = std::chrono::steady_clock::now();
#endif
	dfree(dst);
	size_t n = std::max<size_t>(v.size(), 1);
	HIP_TRY(hipMalloc(&dst, n * sizeof(T)));
#if RTX_MEASURE
	const auto t1 = std::chrono::steady_clock::now();
#endif
	if (!v.empty()) {
		HIP_TRY(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
		HIP_TRY(hipStreamSynchronize(stream));
	}
#if RTX_MEASURE
	const auto t2 = std::chrono::steady_clock::now();
	const double a = std::chrono::duration<double, std::milli>(t1 - t0).count(), b = std::chrono::duration<double, std::milli>(t2 - t1).count();
	if (a + b > 1.0)
		fprintf(stderr, "[rtx upload]   upload of %zu B: free + malloc %.2f ms, copy %.2f ms\n", v.size() * sizeof(T), a, b);
#endif
	return RTX_OK;
}

/* a scoped temporary: the vector into d, which frees the buffer with its scope */
template <class T> static inline int upload(DevBuf<T> &d, const std::vector<T> &v, hipStream_t stream)
{
	d.bytes = 0;
	const int rc = upload(d.p, v, stream);
	if (!rc)
		d.bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
	return rc;
}

/* measurement builds (EXTRA=-DRTX_MEASURE=1): host-side phase times of an upload on stderr */
#if RTX_MEASURE
struct PhaseClock {
	std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
	void mark(const char *what, hipStream_t st)
	{
		(void)hipStreamSynchronize(st);
		const auto n = std::chrono::steady_clock::now();
		fprintf(stderr, "[rtx upload] %-24s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
		t = n;
	}
};
#define PHASE(clk, what, st) clk.mark(what, st)
#else
struct PhaseClock {};
#define PHASE(clk, what, st) ((void)clk)
#endif

/* RTX_OPT_TRACE_PACK 1: the rays of a segment of k_trace's packed GI walk (the sweep) */
#ifndef RTX_TRACE_PACK_SEG
#define RTX_TRACE_PACK_SEG 4096u
#endif

/* the settings a render's shade points per tile depend on (rtx_ctx.sp_tile_key) */
struct SpKey {
	uint32_t v[21] = {};
	uint32_t set = 0;
	bool operator==(const SpKey &o) const { return set && o.set && std::equal(v, v + 21, o.v); }
};

/* a context's stream and events.  A base of rtx_ctx, so that they are destroyed after its members:
 * rtx_close frees the buffers first, then the events and the stream. */
struct RTX_HIDDEN CtxHandles {
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
	CtxHandles() = default;
	CtxHandles(const CtxHandles &) = delete;
	CtxHandles &operator=(const CtxHandles &) = delete;
	~CtxHandles()
	{
		for (hipEvent_t e : { ev[0], ev[1], ev[2], ev[3], ev[4], ev0, ev1 })
			if (e)
				(void)hipEventDestroy(e);
		if (stream)
			(void)hipStreamDestroy(stream);
	}
};

struct rtx_ctx : CtxHandles {
	RTX_HIDDEN ~rtx_ctx() = default; /* out of the library's exported symbols, like every new internal one */
	int device = 0;
	int builder = RTX_BUILD_SAH_GPU; /* the host's SAH tree, built on the device (29 vs 343 ms on the dragon) */
	int cus = 0;
	/* scene: exact-size buffers that change hands between the builder, a group and the context
	 * (rtx_upload.cpp rtx_free_scene) */
	DNode *d_nodes = nullptr;
	DPlane *d_planes = nullptr;
	DMaterial *d_mats = nullptr;
	DEmitter *d_emitters = nullptr;
	DEmitter *d_lin = nullptr; /* RTX_WALK_LINEAR: the bounded objects as shadow-test records */
	DQNode *d_qnodes = nullptr;
	uint32_t *d_top = nullptr;
	DW8 *d_w8 = nullptr;
	DW8S *d_w8s = nullptr;
	float4 *d_cull = nullptr;      /* the 8-wide tree's top-level bounding spheres (DScene.cull) */
	float4 *d_lsph = nullptr;      /* the listed records' bounding spheres (DScene.lsph) */
	DScene scene{};
	bool have_scene = false;
	/* work buffers (grow-only) */
	DevBuf<DTask> d_tasks;
	DevBuf<void> d_pack;        /* k_trace's packed GI walk: a result table and a walk queue per wave (RTX_OPT_TRACE_PACK) */
	DevBuf<uint32_t> d_ostk;    /* k_trace lane-stack overflow (DScene.ostk) */
	DevBuf<uint32_t> d_w8spill; /* k_shadow lane-stack spill of deep 8-wide trees (DScene.w8spill) */
	DevBuf<float4> d_staging;
	DevBuf<float4> d_sp;
	DevBuf<float4> d_contrib;
	DevBuf<uint32_t> d_ordbuf; /* k_shadow's order / result slices, RTX_ORD_WORDS words per grid wave (DScene.ordbuf) */
	DevBuf<uint32_t> d_pmask; /* the chunk's per-point masks, a word per record (k_point_masks) */
	DevBuf<uint32_t> d_clbuf; /* the chunk's processing order split into clear list and rest, and the split's prefix sums
	                           * (RTX_OPT_SHADOW_CLEARLANE, rtx_clearlane_words) */
	DevBuf<uint2> d_tile_rec;
	/* shade points per tile seen by the last render of this scene with the same GI / bounce
	 * settings: sizes the next render's chunks (the static estimate is 5x too high on scene6) */
	double sp_tile_seen = 0.0;
	SpKey sp_tile_key{};
	DevBuf<uint32_t> d_sortbuf; /* keys0 | keys1 | vals0 | vals1 (shade-point sort) */
	DevBuf<void> d_sorttmp;
	DevBuf<int> d_post_rad; /* postprocess: per-pixel DoF radius, pv, scratch */
	DevBuf<float4> d_post_pv;
	DevBuf<unsigned> d_post_scratch;
	float bound_lo[3] = { 0, 0, 0 }, bound_hi[3] = { 0, 0, 0 }; /* bounded objects' box */
	uint32_t total_lights = 0;
	DevBuf<unsigned long long> d_ctr;
	DevBuf<float> d_rgb, d_z; /* the host-buffer calls' framebuffer (rtx_ensure_framebuffer) */
	rtx_stats stats{};
	rtx_point_stats pstats{}; /* rtx_get_point_stats */
	rtx_dark_stats dstats{};  /* rtx_get_dark_stats */
	rtx_order_stats ostats{}; /* rtx_get_order_stats */
	rtx_premask_stats mstats{}; /* rtx_get_premask_stats */
	rtx_clearlane_stats cstats{}; /* rtx_get_clearlane_stats */
	/* ray queries (rtx_trace_rays*): counters of their own, the host-buffer call's device copies */
	DevBuf<unsigned long long> d_rctr;
	DevBuf<float4> d_qrays, d_qhits;
	rtx_ray_stats ray_stats{};
	rtx_shadow_ray_stats shadow_ray_stats{}; /* rtx_trace_shadow_rays */
	rtx_closest_stats closest_stats{};       /* rtx_closest_points* */
	/* denoiser (rtx_frame_features*, rtx_denoise*): grow-only scratch of its own */
	DevBuf<float4> d_dn_rays, d_dn_hits; /* the frame's rays and their closest hits */
	DevBuf<float4> d_dn_work;            /* the filter's 16-byte records (rtx_launch_denoise, rtx_launch_denoise_variance) */
	DevBuf<float4> d_dn_feat;            /* the host-buffer calls' device copies */
	DevBuf<float> d_dn_rgb, d_dn_var;
	DevBuf<unsigned long long> d_dn_ctr; /* k_dn_pack's hit-pixel count */
	/* ray batches (rtx_render_rays*, rtx_ray_features, rtx_render_projection*): grow-only scratch of its own */
	DevBuf<float4> d_rr_rays;            /* the host-buffer calls' device copy of the rays; a projection's generated rays */
	rtx_denoise_stats dn_stats{};
	/* multi-pass rendering (rtx_render_passes*): grow-only scratch of its own */
	DevBuf<float> d_pass_rgb;     /* the pass being rendered */
	DevBuf<double> d_pass_state;  /* mean r, g, b and m2 r, g, b, one double per pixel each (rtx_passes.hip); the
	                               * filtered fold's seventh plane, the weight sum, follows them (rtx_filter.hip) */
	DevBuf<double> d_pass_sums;   /* the blocks' partial sums of the error, then their two totals */
	DevBuf<float> d_pass_var;     /* the host-buffer call's device copy of the variance */
	rtx_pass_stats pass_stats{};
	/* tile-list renders (rtx_render_tiles*) */
	DevBuf<uint32_t> d_tile_list; /* the host-buffer call's device copy of the list */
	DevBuf<uint32_t> d_tile_flag; /* the device call's list check raises it */
	/* adaptive passes (rtx_render_adaptive*): grow-only scratch of its own, rtx_adaptive.hip */
	DevBuf<double> d_ad_state;    /* mean r, g, b and m2 r, g, b, tile-major planes of 64 T doubles */
	DevBuf<double> d_ad_vs;       /* V_t then S_t per tile, then the pass's totals V and A */
	DevBuf<uint32_t> d_ad_tiles;  /* n_t per tile, the two pass lists in turn, the next list's count */
	DevBuf<float> d_ad_var;       /* the host-buffer call's device copies */
	DevBuf<uint32_t> d_ad_passes;
	rtx_adaptive_stats ad_stats{};
	/* feature-guided upsampling (rtx_upsample*, rtx_render_upsampled*): grow-only scratch of its own, rtx_upsample.hip */
	DevBuf<float> d_up_low_rgb;       /* the low frame: the pipeline's render, the host-buffer call's device copy */
	DevBuf<float4> d_up_low_feat, d_up_feat; /* the records of the low and of the full frame, likewise */
	DevBuf<float> d_up_rgb, d_up_conf;
	DevBuf<uint32_t> d_up_count;      /* pixels below the threshold per tile */
	DevBuf<uint32_t> d_up_list;       /* the refinement list */
	DevBuf<unsigned long long> d_up_out; /* its length, and the pixels below the threshold */
	rtx_upsample_stats up_stats{};
	/* temporal accumulation (rtx_temporal*, rtx_render_temporal*): grow-only scratch of its own, rtx_temporal.hip */
	struct TemporalSet {              /* a frame as the pipeline keeps it: the current one, then the history */
		DevBuf<float> rgb, var, len;
		DevBuf<float4> feat;
	};
	TemporalSet tp_set[2];            /* the pipeline's two sets, used in turn */
	TemporalSet tp_host[2];           /* the host-buffer call's device copies of the current frame and of the history */
	DevBuf<float> d_tp_conf;          /* the host-buffer call's device copy of the confidence */
	DevBuf<unsigned long long> d_tp_ctr; /* k_temporal's RTX_TEMPORAL_CTR_WORDS words of statistics */
	std::vector<unsigned long long> tp_ctr; /* ... read back */
	uint32_t tp_hist = 0;             /* the set that holds the history */
	bool tp_valid = false;            /* ... if there is one: cleared by rtx_temporal_reset and by an upload */
	rtx_frame tp_frame{};             /* the history's frame */
	uint32_t tp_frames = 0;           /* pipeline calls since the history was last forgotten */
	rtx_temporal_stats tp_stats{};
	/* rtx_set_option (include/rtx.h RTX_OPT_*) */
	int opt_walk = RTX_WALK_AUTO;
	uint32_t opt_leaf = 1;
	bool opt_spsort = true;
	uint32_t opt_slot = 0;
	uint32_t opt_grab = 4096;
	uint32_t opt_lstk = RTX_W8_STACK;
	int opt_trace_walk = RTX_WALK_AUTO;
	int opt_frame = RTX_FRAME_AUTO;
	uint32_t opt_chunk = 0;   /* most tiles per chunk (0: as many as the shade-point budget allows) */
	uint32_t opt_sp_tile = 0; /* shade points per tile a chunk is sized for (0: the estimate / last render's count) */
	uint32_t opt_rays_grab = 0;   /* RTX_OPT_RAYS_GRAB: packets per k_rays queue grab (0: automatic) */
	uint32_t opt_rays_queues = 0; /* RTX_OPT_RAYS_QUEUES: k_rays packet queues (0: automatic) */
	int opt_cull = 1;         /* RTX_OPT_SHADOW_CULL: 0 off, 1 wave-uniform packets, 2 lane slots too */
	int opt_point = 1;        /* RTX_OPT_SHADOW_POINT: planes and listed objects decided once per shade point */
	int opt_dark = 1;         /* RTX_OPT_SHADOW_DARK: light samples that add nothing skip their shadow query */
	int opt_spec = 1;         /* RTX_OPT_SHADOW_SPEC: a shininess-0 point's samples skip the specular factor */
	int opt_clearlane = 1;    /* RTX_OPT_SHADOW_CLEARLANE: the all-clear points shaded one per lane, in a kernel of their own */
	int opt_order = 1;        /* RTX_OPT_SHADOW_ORDER: a walking point's light samples walked in key order */
	int opt_premask = 1;      /* RTX_OPT_SHADOW_PREMASK: the per-point masks formed before k_shadow, one point per lane */
	uint32_t opt_trace_pack = 1; /* RTX_OPT_TRACE_PACK: 0 off, 1 RTX_TRACE_PACK_SEG rays per segment, else that many */
	uint32_t mem_share = 1;  /* contexts sharing this device's HBM at once (a loopback group's n): the shade-point
	                           * budget of a render is a third of the free HBM divided by it */
};

struct QFrame {
	float qo[3], qs[3];
};

/* a scene flattened and its BVHs built (on the host, or on the building context's device), ready
 * to upload to one or more devices.  Device buffers it still owns are freed with it. */
struct HostScene {
	int builder = RTX_BUILD_SAH_HOST;
	int device = 0;               /* the building context's device */
	bool recs_on_device = false;  /* device builder: the building context holds the records */
	std::vector<DNode> recs;      /* inner nodes then primitives (64-byte records) */
	uint32_t nnodes = 0, nb = 0, root_ref = RTX_EMPTY_REF, depth = 0;
	std::vector<DQNode> qnodes;   /* threaded BVH2 */
	QFrame qf{};
	std::vector<uint32_t> qtop;
	uint32_t ntop = 0;
	std::vector<DW8> w8;          /* 8-wide BVH entries (leaf entries filled on the device) */
	std::vector<uint32_t> w8leaf; /* entry -> primitive index (RTX_NONE: node or hole) */
	uint32_t w8depth = 0;
	QFrame w8f{};                 /* its 16-bit frame */
	bool w8noemit = false;        /* emitters left out of it */
	/* collapsed on the device (rtx_wide8_dev.hip): the buffers, handed to the context on upload
	 * (rtx_upload_built clears these pointers when it takes them) */
	bool w8_on_device = false;
	DW8 *dev_w8 = nullptr;
	DW8S *dev_w8s = nullptr;
	uint32_t *dev_w8leaf = nullptr;
	uint32_t w8_entries = 0, w8_wide = 0;
	uint32_t w8s_entries = 0; /* device collapse: scalar-path copies allocated (entries below the last node entry) */
	uint32_t w8top = 0; /* entries of the 8-wide tree's top levels (rtx_device.h DScene.w8top) */
	bool w8sph = true;  /* the 8-wide tree holds spheres (DScene.w8sph) */
	std::vector<DPlane> planes;
	std::vector<DMaterial> mats;
	std::vector<DEmitter> emit;
	std::vector<DEmitter> lin;    /* RTX_WALK_LINEAR: every bounded object as a shadow-test record */
	float bound_lo[3] = { 0, 0, 0 }, bound_hi[3] = { 0, 0, 0 }, ambient[3] = { 0, 0, 0 };
	uint32_t num_emitters = 0;
	DTreeFrame tf{};              /* the frame every tree's boxes are in (rtx_frame.cpp) */
	double frame_ratio = 1.0;     /* its sampled leaf-box cost over the identity's */
	double frame_pad = 0;         /* the leaf boxes' padding for the ray transform (rtx_frame.cpp) */
	double frame_ms = 0;          /* choosing it and the leaf boxes in it */
	double build_ms = 0;
	HostScene() = default;
	HostScene(const HostScene &) = delete;
	HostScene &operator=(const HostScene &) = delete;
	~HostScene()
	{
		if (dev_w8 || dev_w8s || dev_w8leaf) {
			(void)hipSetDevice(device);
			dfree(dev_w8);
			dfree(dev_w8s);
			dfree(dev_w8leaf);
		}
	}
};

/* flatten sc and build its BVHs (on c's device for the device builder), then upload to c */
int rtx_build_scene(rtx_ctx *c, const rtx_scene_desc *sc, HostScene &hs);
int rtx_upload_built(rtx_ctx *c, HostScene &hs);
/* a device-collapsed 8-wide tree's buffers on one device (hs.w8_on_device): the building device's
 * own, or a device group's peer copies of them */
struct DevTree {
	DW8 *w8 = nullptr;
	DW8S *w8s = nullptr;
	uint32_t *leaf = nullptr;
	int device = 0;
};
/* upload a built scene to c, taking the device tree from `take` (c's device; c owns the buffers
 * after the call and take's pointers are cleared once handed over: on failure the caller frees
 * whatever take still holds).  hs is only read, so several contexts may upload one scene at once
 * from their own host threads. */
int rtx_upload_built(rtx_ctx *c, const HostScene &hs, DevTree *take);
/* rtx_wide8.cpp: the 8-wide shadow BVH collapsed from the BVH2 (0 = not built); boxes it takes
 * from primitive records (leaves of several primitives) in the trees' frame tf, padded by fpad */
uint32_t rtx_wide8_build(const std::vector<DNode> &inner, uint32_t nnodes, const DPrim *prims, uint32_t root_ref,
			 const float lo[3], const float hi[3], const std::vector<uint32_t> &skip_objs, const DTreeFrame &tf,
			 double fpad, QFrame &F, bool &skipped, std::vector<DW8> &out, std::vector<uint32_t> &leafmap);
/* one frame (or tile shard) into device buffers on stream.  d_tiles: a checked device list of n_tiles tile indices
 * (strictly increasing, below the frame's tile count) to render instead, with tile sharding 0/1.  d_prim_rays: the
 * fr->width * fr->height rtx_ray records of a ray batch (16-byte aligned, no tile list) in place of the frame's own
 * primary rays; fr then gives the size alone, and the shade-points-per-tile estimate is neither read nor written */
int rtx_render_common(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, float *d_rgb, float *d_z, hipStream_t stream,
		      const uint32_t *d_tiles = nullptr, uint32_t n_tiles = 0, const void *d_prim_rays = nullptr);
/* rtx_rays_render.cpp: checked arguments, both buffers on the device (16-byte aligned): the closest hits of the w * h
 * rays d_rays as feature records, on stream (synchronised); fills c->dn_stats */
RTX_HIDDEN int rtx_ray_features_common(rtx_ctx *c, uint32_t w, uint32_t h, const void *d_rays, int32_t u32conv, void *d_features,
				       hipStream_t stream);
/* rtx_scene.cpp: c's scene buffers freed (c's device current) */
RTX_HIDDEN void rtx_free_scene(rtx_ctx *c);
/* rtx_query.cpp: n checked rays on device buffers into c->ray_stats (the feature buffers' query too) */
RTX_HIDDEN int rtx_rays_common(rtx_ctx *c, uint32_t n, const void *d_rays, void *d_hits, uint32_t flags, hipStream_t stream);

/* rtx_image.cpp: the feature records of a checked frame into a 16-byte aligned device buffer, on stream (synchronised);
 * fills c->dn_stats as rtx_frame_features_device does (the upsampling pipeline's two feature calls, rtx_upsample.cpp) */
RTX_HIDDEN int rtx_features_common(rtx_ctx *c, const rtx_frame *fr, int32_t u32conv, void *d_features, hipStream_t stream);

/* rtx_passes.cpp: what the multi-pass (adaptive: and the adaptive) entries refuse about non-null arguments */
RTX_HIDDEN int rtx_passes_args_check(const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, bool adaptive);
/* ... everything they refuse before they launch anything, null arguments and a scene-less context included;
 * what rtx_pass_frame refuses about the pass parameters alone; and pass k's sub-pixel offset in pixel units
 * (the filtered entries share all three, rtx_filter.cpp) */
RTX_HIDDEN int rtx_passes_check(rtx_ctx *c, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, bool adaptive);
RTX_HIDDEN int rtx_pass_params_check(const rtx_pass_params *pp);
RTX_HIDDEN void rtx_pass_offset(const rtx_pass_params *pp, uint32_t k, double *ox, double *oy);

/* Steps that more than one entry point takes.  They return the HIP error and each caller reports it
 * with its own code and text. */

/* c->d_rgb and c->d_z with room for px pixels (rtx_render, rtx_postprocess, rtx_group_render) */
static inline hipError_t rtx_ensure_framebuffer(rtx_ctx *c, size_t px)
{
	const hipError_t e = c->d_rgb.grow(px * 3 * sizeof(float));
	return e != hipSuccess ? e : c->d_z.grow(px * sizeof(float));
}

/* k_trace's and k_rays' lane-stack entries beyond the LDS part, [entry][grid lane], for a grid of
 * `waves` waves on c's scene: the render sizes the buffer for its own waves, and a query may come
 * first or run a larger grid */
static inline hipError_t rtx_ensure_ostk(rtx_ctx *c, uint32_t waves)
{
	hipError_t e = hipSuccess;
	if (c->scene.stack_size > RTX_TRACE_LSTK)
		e = c->d_ostk.grow((size_t)waves * 64 * (c->scene.stack_size - RTX_TRACE_LSTK) * sizeof(uint32_t));
	c->scene.ostk = c->d_ostk;
	return e;
}

/* k_shadow's LDS stack size and spill area into S (c's scene for a render, which sets them at
 * every render; a query's own copy, since a query may come first): 8-wide trees deeper than the
 * LDS lane stacks spill the deeper entries of every lane of the largest k_shadow grid (one group
 * per level at most).  A caller that reports a failed allocation in its own way learns of one through
 * *alloc (false: the grid-size query failed). */
static inline hipError_t rtx_ensure_w8spill(rtx_ctx *c, DScene &S, bool *alloc = nullptr)
{
	if (alloc)
		*alloc = false;
	S.w8lstk = c->opt_lstk;
	S.w8spill = nullptr;
	S.w8spill_lanes = 0;
	if (!(S.w8 && S.w8depth > S.w8lstk + 1))
		return hipSuccess;
	uint32_t lanes = 0;
	hipError_t e = rtx_shadow_grid_lanes((uint32_t)c->cus, &lanes);
	if (e != hipSuccess)
		return e;
	if (alloc)
		*alloc = true;
	e = c->d_w8spill.grow((size_t)lanes * (S.w8depth - 1 - S.w8lstk) * sizeof(uint32_t));
	if (e != hipSuccess)
		return e;
	S.w8spill = c->d_w8spill;
	S.w8spill_lanes = lanes;
	return hipSuccess;
}

/* the queries' counters (c->d_rctr), allocated at the first query and zeroed on stream */
static inline hipError_t rtx_reset_query_counters(rtx_ctx *c, hipStream_t stream)
{
	const hipError_t e = c->d_rctr.grow(sizeof(unsigned long long) * RTX_RQ_N);
	return e != hipSuccess ? e : hipMemsetAsync(c->d_rctr, 0, sizeof(unsigned long long) * RTX_RQ_N, stream);
}

static inline DFrame rtx_dframe(const rtx_frame *fr)
{
	DFrame F;
	F.width = fr->width;
	F.height = fr->height;
	memcpy(F.corner, fr->corner, 12);
	memcpy(F.step_x, fr->step_x, 12);
	memcpy(F.step_y, fr->step_y, 12);
	memcpy(F.origin, fr->origin, 12);
	return F;
}

#endif
