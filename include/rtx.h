/*
 * rtx.h — C-ABI of the MI355X-native trace/intersect/shade path.
 *
 * Drop-in boundary for C-Raytracer's hot path.  The reference
 * enters the path at src/raytracer/main.c:76-79:
 *
 *     accel_init();   // accel.c:266-315   BVH build over objects[]
 *     render_init();  // render.c:61-116   CLI -> render globals
 *     render();       // render.c:345-368  per-pixel cast_ray() recursion
 *     ...
 *     accel_deinit(); // accel.c:100-103
 *
 * with all inputs passed through globals (objects[], emittant_objects[],
 * unbound_objects[], materials[], camera, image, global_ambient_light_intensity)
 * and the outputs image.raster / image.z_buffer.  Here every input crosses the
 * boundary explicitly as plain structs and pointers:
 *
 *     rtx_open()          replaces nothing (device context; owns device memory)
 *     rtx_upload_scene()  replaces accel_init()           accel.c:266
 *     rtx_render()        replaces render_init()+render() render.c:61, 345
 *     rtx_close()         replaces accel_deinit()         accel.c:100
 *
 * Host glue that the reference keeps outside the path (scene.c JSON loader,
 * object.c STL ingest, image.c image-plane setup and TIFF writer, argv.c CLI)
 * lives in librtxscene and is declared in rtx_scene.h.
 *
 * Conventions: every int-returning call returns RTX_OK (0) or a negative
 * RTX_ERR_* code and sets a thread-local message readable with
 * rtx_last_error().  The library never calls exit().  Buffers passed in are
 * caller-owned and copied; the library owns device memory only.
 */
#ifndef RTX_H
#define RTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 1

enum rtx_status {
	RTX_OK = 0,
	RTX_ERR_ARG = -1,     /* bad argument / shape */
	RTX_ERR_HIP = -2,     /* HIP runtime failure */
	RTX_ERR_NOMEM = -3,   /* host or device allocation failed */
	RTX_ERR_SCENE = -4,   /* scene rejected (reference would error()/exit(1)) */
	RTX_ERR_NODEV = -5,   /* no usable gfx950 device */
	RTX_ERR_STATE = -6,   /* call order (e.g. render before upload) */
	RTX_ERR_IO = -7,      /* file I/O (scene / mesh / TIFF) */
};

/* object.h:17-23 enum ObjectType (UNBOUND_OBJECTS build) */
enum rtx_object_type { RTX_SPHERE = 0, RTX_TRIANGLE = 1, RTX_PLANE = 2 };

/* material.c:27-53 texture kinds, material.h:17-22 enum PeriodicFunction */
enum rtx_texture_type {
	RTX_TEX_UNIFORM = 0,
	RTX_TEX_CHECKERBOARD = 1,
	RTX_TEX_BRICK = 2,
	RTX_TEX_NOISY_PERIODIC = 3,
};
enum rtx_periodic { RTX_PERIODIC_SIN = 0, RTX_PERIODIC_SAW = 1, RTX_PERIODIC_TRIANGLE = 2, RTX_PERIODIC_SQUARE = 3 };

/* struct Material (material.h:30-44) + its texture, flattened. */
typedef struct rtx_material {
	int32_t id;
	float ks[3], ka[3], kr[3], kt[3], ke[3];
	float shininess;
	float refractive_index;
	int32_t texture;        /* enum rtx_texture_type */
	int32_t periodic;       /* enum rtx_periodic (noisy periodic only) */
	/* uniform: color[0]; checkerboard/brick: colors[0], colors[1];
	 * noisy periodic: color[0] = color, color[1] = color gradient */
	float color[2][3];
	float scale;            /* checkerboard, brick */
	float mortar_width;     /* brick */
	float noise_feature_scale, noise_scale, frequency_scale; /* noisy periodic */
	/* material_init (material.c:81-83): ‖k‖ > 1e-6 */
	int32_t emittant, reflective, transparent;
} rtx_material;

/*
 * One object of the reference's objects[] array (object.c:25-44), in load
 * order, with the values its *_postinit / *_scale produced:
 *   sphere   : p0 = position, radius                                (object.c:25-29)
 *   triangle : p0,p1,p2 = vertices, e1 = v1-v0, e2 = v2-v0,
 *              n = norm(e1 x e2)                                    (object.c:31-36, 327-340)
 *   plane    : n = unit normal, d = n . position                    (object.c:39-43, 457-466)
 * epsilon is resolved (per-type default applied), num_lights as loaded.
 */
typedef struct rtx_object {
	int32_t type;           /* enum rtx_object_type */
	int32_t material;       /* index into rtx_scene_desc.materials */
	uint32_t num_lights;
	float epsilon;
	float p0[3], p1[3], p2[3];
	float e1[3], e2[3];
	float n[3];
	float radius;
	float d;
} rtx_object;

/* struct Camera (camera.h:17-22) after camera_init/camera_scale. */
typedef struct rtx_camera {
	float position[3];
	float vectors[3][3];    /* v0, v1 normalised; v2 = v0 x v1 (camera.c:29-32) */
	float fov;
	float focal_length;
} rtx_camera;

/* Everything accel_init() + render() read from globals. */
typedef struct rtx_scene_desc {
	uint32_t num_materials;
	const rtx_material *materials;
	uint32_t num_objects;
	const rtx_object *objects;       /* reference order */
	uint32_t num_emitters;
	const uint32_t *emitters;        /* object indices, emittant_objects[] order */
	float ambient[3];                /* global_ambient_light_intensity */
	rtx_camera camera;
} rtx_scene_desc;

/* struct Image's plane (image.h:17-26) as image_init (image.c:34-56) built it. */
typedef struct rtx_frame {
	uint32_t width, height;
	float corner[3];        /* image.corner */
	float step_x[3];        /* image.vectors[X] */
	float step_y[3];        /* image.vectors[Y] */
	float origin[3];        /* camera.position */
} rtx_frame;

enum rtx_reflection { RTX_PHONG = 0, RTX_BLINN = 1 };                       /* render.c:32-35 */
enum rtx_gi { RTX_GI_AMBIENT = 0, RTX_GI_PATH = 1 };                        /* render.c:37-40 */
enum rtx_attenuation { RTX_ATT_NONE = 0, RTX_ATT_LIN = 1, RTX_ATT_SQR = 2 }; /* render.c:42-46 */
/* rand_flt (system.c:93-96) replacement */
enum rtx_rng {
	RTX_RNG_COUNTER = 0,  /* counter-based hash of (seed, pixel, ray-tree node, draw): i.i.d. draws like
	                       * rand_flt, two per light sample (object.c:298-299, 403-419); the default */
	RTX_RNG_CONST = 1,    /* every draw == 0.5f (the oracle's REF_CONST_RNG) */
	RTX_RNG_STRAT = 2,    /* RTX_RNG_COUNTER with the light samples stratified (opt-in): sample j
	                       * of an emitter's n draws its first number (the sphere's inclination, the
	                       * triangle's p) from [j/n, (j+1)/n) as ((float)j + u) / n; each stratum is
	                       * sampled uniformly, so the estimator keeps render.c:170-229's expectation
	                       * (a different estimator from the reference's i.i.d. one, lower variance) */
};
/* (uint32_t)float in texture_get_color_checkerboard/brick (material.c:164,173)
 * is UB for negatives; its result depends on the host ISA. */
enum rtx_u32conv {
	RTX_U32_SAT = 0,      /* x86 AVX-512 vcvttss2usi: x <= -1 or >= 2^32 or NaN -> 0xFFFFFFFF */
	RTX_U32_WRAP = 1,     /* 64-bit cvttss2si truncated to 32 bits (generic x86-64) */
};

/* render_init() globals (render.c:53-60) + library extensions. */
#define RTX_MAX_BOUNCES 4096 /* the reflection/refraction task stacks are sized for max_bounces up to this */
typedef struct rtx_params {
	uint32_t max_bounces;        /* -b, default 10, at most RTX_MAX_BOUNCES (RTX_ERR_ARG above) */
	float min_intensity_sqr;     /* -a squared, default 1e-4 */
	int32_t reflection;          /* -s, enum rtx_reflection, default phong */
	int32_t gi;                  /* -g, enum rtx_gi, default ambient */
	uint32_t samples;            /* -n, default 1 (path GI samples at the primary hit) */
	int32_t attenuation;         /* -l, enum rtx_attenuation, default sqr */
	float attenuation_offset;    /* -o, default 1.0 */
	int32_t rng;                 /* enum rtx_rng */
	uint64_t seed;
	int32_t u32conv;             /* enum rtx_u32conv */
	/* sharding: render only tiles t with t % tile_stride == tile_offset
	 * (1 tile = 8x8 pixels, row-major over the frame).  Pixels of other tiles are
	 * left untouched in the output.  Defaults 0 / 1 = whole frame. */
	uint32_t tile_offset, tile_stride;
	/* count BVH node visits and primitive tests (slower kernel instance) */
	int32_t count_traversal;
} rtx_params;

/* Defaults of render.c:53-60 (+ counter RNG, seed 1, SAT conversion, whole frame). */
void rtx_params_default(rtx_params *p);

typedef struct rtx_stats {
	uint64_t closest_rays;       /* cast_ray() calls (render.c:136) */
	uint64_t shadow_rays;        /* is_light_blocked() calls (render.c:126) */
	/* only with count_traversal: per-ray work summed over all rays (closest + shadow).  A shadow ray's
	 * tests of transparent leaves of the 8-wide tree count where its walk meets them, whether or not an
	 * opaque hit ends the ray before the wave runs them (they are deferred): the counts do not depend on
	 * which rays share a packet */
	uint64_t node_visits;        /* BVH inner nodes fetched (2 child boxes tested) */
	uint64_t tri_tests;
	uint64_t sphere_tests;
	uint64_t plane_tests;
	/* ... of which by shadow rays (node visits in BVH2 units: shadow_box_tests / 2) */
	uint64_t shadow_node_visits;
	uint64_t shadow_tri_tests;
	uint64_t shadow_sphere_tests;
	uint64_t shadow_plane_tests;
	uint64_t shade_points;       /* hits whose direct lighting was evaluated */
	double kernel_ms;            /* device time of the last rtx_render*, HIP events, all kernels */
	double trace_ms;             /* ... closest-hit / shading kernel */
	double shadow_ms;            /* ... shadow-ray kernel */
	double accum_ms;             /* ... per-tile accumulation kernel */
	double sort_ms;              /* ... shade-point ordering (key + radix sort) */
	double build_ms;             /* host wall time of the last rtx_upload_scene's BVH build (incl. its uploads) */
	uint32_t bvh_nodes;
	uint32_t bvh_depth;
	uint32_t bvh_prims;
	uint32_t waves;              /* persistent waves of the closest-hit kernel */
	uint32_t chunks;             /* tile chunks the frame was split into */
	uint32_t builder;            /* RTX_BUILD_* used by the last upload */
	/* only with count_traversal: the shadow walk (k_shadow) */
	uint64_t shadow_box_tests;        /* box tests (threaded-BVH records stepped through), summed over shadow rays */
	uint64_t shadow_global_box_tests; /* ... of which read from the DQNode array (the rest from the LDS top copy) */
	uint64_t shadow_wave_steps;       /* walk-loop iterations summed over waves (a wave steps until its longest ray ends) */
	uint64_t shadow_wave_walks;       /* wave walks (64 lane slots each): steps / walks = the waves' mean walk length */
	uint32_t wide_nodes;              /* 8-wide BVH nodes (0: k_shadow walks the threaded BVH2) */
	uint32_t wide_depth;
	uint64_t shadow_leaf_rounds;      /* only with count_traversal, 8-wide walk: wave iterations of its leaf loops */
	double gather_ms;                 /* rtx_group_render: shard pack + RCCL gather + unpack (0 on one device) */
	uint32_t devices;                 /* devices that rendered the last frame */
	uint32_t pad_;
	uint64_t shadow_uniform_steps;    /* only with count_traversal, 8-wide walk: wave steps whose active lanes were all at one node */
	uint32_t shadow_walk;             /* the BVH k_shadow walks: RTX_WALK_W8 / RTX_WALK_BVH2 / RTX_WALK_LINEAR */
	uint32_t wide_entries;            /* 8-wide walk: 64-byte entries (nodes, primitive records, holes) */
	uint32_t trace_walk;              /* the BVH k_trace walks for closest hits: RTX_WALK_W8 / RTX_WALK_BVH2 */
	uint32_t pad2_;
	uint32_t tree_rotated;            /* the trees are built in a rotated frame (rtx_tree_frame) */
	uint32_t pad3_;
	double frame_cost;                /* its sampled leaf-box surface area over the world frame's (1: world frame) */
	double frame_ms;                  /* host time choosing the frame and taking the leaf boxes in it */
	double upload_copy_ms;            /* device groups: this device's copies of the scene built on device 0
	                                   * (last rtx_group_upload_scene; 0 on device 0 and for single contexts) */
	uint32_t transport;               /* device groups: RTX_TRANSPORT_* of the shard gather */
	uint32_t peer_access;             /* device groups: this device and device 0 have peer access enabled
	                                   * (hipDeviceEnablePeerAccess both ways; 1 on device 0 itself) */
	/* only with count_traversal: rays whose origin lies more than 4 scene radii from the bounded
	 * objects, whose box tests start from a point formed in double near them (any tree frame) */
	uint64_t far_closest_rays;        /* closest-hit rays (the frame origin moved along the ray) */
	uint64_t far_shadow_rays;         /* shadow rays from far shade points (walked from the light end) */
	uint64_t shadow_stack_spills;     /* only with count_traversal, 8-wide walk: lane-stack entries pushed beyond
	                                   * the LDS ones (to HBM, DScene.w8spill) */
	uint64_t shadow_cone_clear;       /* only with count_traversal: shadow rays of packets whose light cone met no
	                                   * box of the 8-wide tree's top levels, so they were not walked
	                                   * (RTX_OPT_SHADOW_CULL) */
} rtx_stats;

/* What a shade point's masks let skip (RTX_OPT_SHADOW_POINT), only with count_traversal: the
 * continuation of rtx_stats, in a struct of its own so that rtx_stats keeps its size for callers
 * built against it (rtx_get_point_stats, after the render like rtx_get_stats) */
typedef struct rtx_point_stats {
	uint64_t shadow_plane_skipped;    /* plane tests of shadow rays not run (shadow_plane_tests counts those run) */
	uint64_t shadow_lin_skipped;      /* tests of objects taken one by one (the emitters out of the 8-wide tree,
	                                   * RTX_WALK_LINEAR's objects) not run */
	uint64_t shadow_point_clear;      /* shadow rays of all-clear shade points: nothing can block any of their
	                                   * samples, so their packets run no shadow query at all */
} rtx_point_stats;

/* What RTX_OPT_SHADOW_DARK answered without a shadow query, only with count_traversal; a struct of
 * its own for the same reason (rtx_get_dark_stats, after the render) */
typedef struct rtx_dark_stats {
	uint64_t shadow_dark_rays;        /* shadow rays of dark light samples (their terms are 0 whatever the ray
	                                   * meets): not queried.  Packets the cone cull cleared are not looked at */
	uint64_t shadow_dark_packet_rays; /* ... of which in packets of dark samples alone: no plane or object test
	                                   * and no walk for the packet */
} rtx_dark_stats;

/* What RTX_OPT_SHADOW_ORDER put in order, only with count_traversal; a struct of its own for the same
 * reason (rtx_get_order_stats, after the render) */
typedef struct rtx_order_stats {
	uint64_t shadow_ordered_points; /* runs of one emitter's light samples of a shade point walked in key order
	                                 * (a point counts once per emitter it orders) */
	uint64_t shadow_ordered_rays;   /* the shadow rays walked in them (their dark samples are not walked) */
} rtx_order_stats;

/* Whether RTX_OPT_SHADOW_PREMASK took effect, with or without count_traversal; a struct of its own for
 * the same reason (rtx_get_premask_stats, after the render) */
typedef struct rtx_premask_stats {
	uint64_t premask_points; /* shade points whose masks were formed ahead of k_shadow (every point of the
	                          * frame, or 0: the option is off or the scene is not one it applies to) */
} rtx_premask_stats;

/* What RTX_OPT_SHADOW_CLEARLANE took in the last render, with or without count_traversal (a counting render
 * takes none); a struct of its own for the same reason (rtx_get_clearlane_stats, after the render) */
typedef struct rtx_clearlane_stats {
	uint64_t clear_points; /* shade points shaded one per lane by the kernel of the all-clear points */
	uint64_t clear_rays;   /* their shadow rays (counted in rtx_stats.shadow_rays too) */
} rtx_clearlane_stats;

typedef struct rtx_ctx rtx_ctx;

/* BVH builders for rtx_upload_scene (replacing accel_init, accel.c:266-315) */
enum {
	RTX_BUILD_SAH_HOST = 0, /* binned SAH on the host (bvh_build.cpp) */
	RTX_BUILD_LBVH_GPU = 1, /* Morton-code linear BVH built on the device (rtx_build.hip) */
	RTX_BUILD_PLOC_GPU = 2, /* locally-ordered clustering (PLOC) on the device (rtx_build.hip) */
	RTX_BUILD_SAH_GPU = 3   /* default: the host's binned SAH run on the device, level by level (rtx_build.hip), the same tree */
};

int rtx_device_count(int *count);
/* Open a context on HIP device `device` (must be gfx950).  Loads the library's device code on
 * that device and primes host-to-device copies once (~0.1 s), so uploads and renders do not. */
int rtx_open(int device, rtx_ctx **out);
/* Flatten + copy the scene to the device, build the BVH (replaces accel_init). */
int rtx_upload_scene(rtx_ctx *ctx, const rtx_scene_desc *scene);
/* Render into caller-owned HOST buffers rgb[W*H*3] (row-major, row 0 = top,
 * overwritten, not accumulated) and z[W*H] (primary-hit distance, 0 on miss);
 * either may be NULL.  Replaces render_init()+render(). */
int rtx_render(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, float *rgb, float *z);
/* Same into DEVICE buffers on the context's device, enqueued on `stream`
 * (hipStream_t, NULL = the context's own stream); synchronises the stream. */
int rtx_render_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, void *d_rgb, void *d_z,
		      void *stream);
int rtx_get_stats(const rtx_ctx *ctx, rtx_stats *out);
int rtx_get_point_stats(const rtx_ctx *ctx, rtx_point_stats *out);
int rtx_get_dark_stats(const rtx_ctx *ctx, rtx_dark_stats *out);
int rtx_get_order_stats(const rtx_ctx *ctx, rtx_order_stats *out);
int rtx_get_premask_stats(const rtx_ctx *ctx, rtx_premask_stats *out);
int rtx_get_clearlane_stats(const rtx_ctx *ctx, rtx_clearlane_stats *out);
/* Builder used by subsequent rtx_upload_scene calls on this context (RTX_BUILD_*). */
int rtx_set_builder(rtx_ctx *ctx, int builder);

/* Shadow-walk BVH layouts (rtx_stats.shadow_walk, RTX_OPT_SHADOW_WALK); 1 was the 4-wide walk */
enum {
	RTX_WALK_AUTO = -1, /* the fastest available: LINEAR for tiny scenes, the threaded BVH2 from LDS for
	                     * small ones (<= 1024 bounded objects), else 8-wide */
	RTX_WALK_BVH2 = 0,  /* threaded quantised BVH2 (DQNode), no stack */
	RTX_WALK_W8 = 2,    /* 8-wide compressed BVH (8-bit child boxes in each node's frame) */
	RTX_WALK_LINEAR = 3 /* no tree: every bounded object tested one by one, like the planes (AUTO for
	                     * scenes of at most RTX_SHADOW_LINEAR_MAX bounded objects) */
};
#define RTX_SHADOW_LINEAR_MAX 8
/* The frame the BVHs are built in (RTX_OPT_TREE_FRAME, rtx_tree_frame) */
enum {
	RTX_FRAME_AUTO = 0,  /* default: a rotated frame when it shrinks the leaf boxes (a rotated mesh's own axes) */
	RTX_FRAME_WORLD = 1  /* always the world axes, as accel.c:266-315 */
};
/* Context options: the defaults are the tuned values; the others exist for A/B measurement and
 * tests.  Build options take effect at the next rtx_upload_scene. */
enum rtx_option {
	RTX_OPT_SHADOW_WALK = 1, /* RTX_WALK_* (build; default RTX_WALK_AUTO) */
	RTX_OPT_BVH_LEAF = 2,    /* most primitives per BVH2 leaf, 1..16 (build; default 1) */
	RTX_OPT_SPSORT = 3,      /* 1: shade points in Morton order for k_shadow (default); 0: emission order */
	RTX_OPT_SHADOW_SLOT = 4, /* k_shadow lanes per shade-point slot: 0 = automatic (default), else a power of two <= 64 */
	RTX_OPT_SHADOW_GRAB = 5, /* lane slots per k_shadow work-queue grab, >= 1 (default 4096) */
	RTX_OPT_SHADOW_LDS_STACK = 6, /* 8-wide walk: lane-stack entries kept in LDS, 1..8 (default 8); deeper
	                               * ones spill to HBM (tests use 1 to exercise the spill on any tree) */
	RTX_OPT_TRACE_WALK = 7,       /* closest hits (k_trace): RTX_WALK_AUTO (the 8-wide tree when built,
	                               * default), RTX_WALK_W8 or RTX_WALK_BVH2 (the float BVH2) */
	RTX_OPT_TREE_FRAME = 8,       /* RTX_FRAME_* (build; default RTX_FRAME_AUTO) */
	RTX_OPT_CHUNK_TILES = 9,      /* most 8x8 tiles per chunk of a render (0 = as many as the shade-point budget,
	                               * a third of free HBM, allows; default 0) */
	RTX_OPT_SP_PER_TILE = 10,     /* shade points per tile a chunk is sized for (0 = automatic, default): a
	                               * chunk that overflows is halved and retried, so any value gives the same
	                               * image (tests drive the overflow path with a low one) */
	RTX_OPT_SHADOW_CULL = 11,     /* 1 (default): a packet of one shade point's light samples skips the 8-wide
	                               * walk when the cone from the point around the light's bounding sphere
	                               * meets no box of the tree's top two levels (the walk would find nothing,
	                               * so the image is the same); 2: packets of several points (points with
	                               * fewer than 64 samples) too, when every lane's point is clear for its
	                               * emitter (emitters 0..7); 0: every packet walks */
	RTX_OPT_RAYS_GRAB = 12,       /* ray queries: 64-ray packets a wave takes per queue grab, 1..64 (0 = automatic,
	                               * default: 1, up to 4 for batches of 16 packets per wave and more) */
	RTX_OPT_RAYS_QUEUES = 13,     /* ray queries: atomic packet queues the waves are dealt over, 1..8 (0 =
	                               * automatic, default: 8); any value gives the same hits */
	RTX_OPT_SHADOW_POINT = 14,    /* 1 (default): a shade point with 64 light samples or more decides once, per
	                               * emitter, that no sample's ray can meet a plane or an object k_shadow tests
	                               * one by one; its packets then skip those tests, and a point clear of
	                               * everything runs a loop with no shadow query (same image); 0: every packet
	                               * tests them.  RTX_OPT_SHADOW_CULL 0 turns this off too */
	RTX_OPT_SHADOW_DARK = 15,     /* 1 (default): a light sample of a shade point with 64 samples or more whose
	                               * diffuse and specular factors are both 0 (a light behind the surface, and
	                               * no specular term toward the viewer) skips its shadow query: it adds +-0
	                               * blocked or not (same image).  Only where shadow rays walk a tree and
	                               * the cone cull has not cleared the packet, in scenes whose transmittances are
	                               * finite with |kt| <= 1 and whose emitters are finite; 0: every sample is
	                               * queried.  RTX_OPT_SHADOW_CULL 0 turns this off too */
	RTX_OPT_SHADOW_PREMASK = 16,  /* 1 (default): the masks of RTX_OPT_SHADOW_CULL and RTX_OPT_SHADOW_POINT are formed
	                               * by a kernel of their own ahead of k_shadow, one shade point per lane, where
	                               * k_shadow would form them one point per wave (points with 64 light samples
	                               * or more) and the scene has at most 8 emitters (same masks, same image);
	                               * 0: k_shadow forms them itself */
	RTX_OPT_SHADOW_ORDER = 17,    /* 1 (default): a shade point that walks the tree takes the light samples of one
	                               * emitter, more than 64 and at most 1024 of them, in the order of where their
	                               * light points lie across the cone toward the emitter (16 buckets), so the 64
	                               * rays of a packet cross much the same part of the tree; the samples' terms
	                               * are still added in index order (same image, bit for bit); 0: index order */
	RTX_OPT_SHADOW_SPEC = 18,     /* 1 (default): a shade point with 64 light samples or more whose material has
	                               * shininess 0 does not evaluate the specular factor of its samples: powf(x, 0)
	                               * is 1 for every x, so the specular term is ks li (same image, bit for bit);
	                               * 0: every sample evaluates it */
	RTX_OPT_TRACE_PACK = 19,      /* 1 (default): k_trace takes a tile's path-GI rays, on the 8-wide tree, in
	                               * segments: every ray up to its visit of the root, then the rays that go on
	                               * into the tree packed 64 to a wave, then the hits in the rays' own order (same
	                               * image, shade points and counters, bit for bit); 512, 1024, 2048 or 4096: the
	                               * same with that many rays per segment (1 takes the library's own figure);
	                               * 0: every batch of 64 rays walks to the end on its own */
	RTX_OPT_SHADOW_CLEARLANE = 20, /* 1 (default): the shade points with 64 light samples or more that RTX_OPT_SHADOW_POINT
	                               * finds clear of everything, and that lie on no emitter, are split off the
	                               * processing order and shaded by a kernel of their own, one point per lane, its
	                               * samples in sequence, summed in the order of the 64-lane reduction (same image,
	                               * bit for bit).  Only where RTX_OPT_SHADOW_PREMASK formed the masks, and not in
	                               * a render with count_traversal; 0: k_shadow shades them, one point per wave */
};
int rtx_set_option(rtx_ctx *ctx, int option, int64_t value);
/* The frame rtx_upload_scene builds the scene's BVHs in under RTX_FRAME_AUTO (a diagnostic; no
 * device needed): *rotated = 0 for the world axes, else rot = R (rows, x' = R (x - center)) and
 * *cost_ratio = its sampled leaf-box surface area over the world frame's.  Every primitive is
 * still tested in world space: the frame changes which boxes a ray meets, not any hit. */
int rtx_tree_frame(const rtx_scene_desc *scene, int *rotated, float rot[9], float center[3], double *cost_ratio);
void rtx_close(rtx_ctx *ctx);
const char *rtx_last_error(void);
/* Diagnostics (tests): the uploaded 8-wide tree's 64-byte entries (csrc/rtx_device.h DW8) copied to
 * host memory, at most `capacity` of them; *count = the tree's entry count (0: no 8-wide tree),
 * frame[6] = its 16-bit frame (origin, scale per axis).  entries may be NULL to query the count. */
int rtx_read_wide_tree(rtx_ctx *ctx, void *entries, uint32_t capacity, uint32_t *count, float frame[6]);
/* Diagnostics (tests): the uploaded BVH2.  records: its 64-byte records (csrc/rtx_device.h), *num_nodes DNode
 * inner nodes followed by *num_prims DPrim primitive records in leaf order, at most record_capacity of them;
 * *root_ref = the root's ref (RTX_EMPTY_REF 0xFFFFFFFF: no bounded objects).  qnodes: the threaded 16-bit copy's
 * 16-byte DQNode records, at most qnode_capacity of them; *num_qnodes = their count (0: the context holds no
 * threaded copy, as when the shadow walk takes the 8-wide tree or no tree), qframe[6] = its 16-bit frame (origin,
 * scale per axis).  records, qnodes and qframe may be NULL to query the counts. */
int rtx_read_bvh2(rtx_ctx *ctx, void *records, uint32_t record_capacity, uint32_t *num_nodes, uint32_t *num_prims,
		  uint32_t *root_ref, void *qnodes, uint32_t qnode_capacity, uint32_t *num_qnodes, float qframe[6]);

/*
 * Ray queries: the closest hit (or any hit) of a caller's own rays against the uploaded scene,
 * what the reference's get_closest_intersection (render.c:118-124) finds with inside_object ==
 * NULL: every plane (unbound_objects[]), the emitters the 8-wide tree leaves out and the tree
 * (RTX_OPT_TRACE_WALK: the 8-wide tree or the float BVH2), each object with its own epsilon as
 * the lower bound of t (object.c:254-265, 356-365, 473-488), the exact intersectors of the
 * renderer.  A query renders nothing and leaves rtx_get_stats, the next render's image and its
 * chunk sizing as they were; it shares (and may grow) the context's scratch buffers, so like
 * every call on a context it must not run concurrently with another.
 */
typedef struct rtx_ray {          /* 32 B */
	float origin[3];
	float tmax;               /* hits need t < tmax, strictly: tmax = a hit's own t excludes it, the next float above
	                           * keeps it; INFINITY (or NaN) = unbounded, as the renderer's rays; 0, a negative
	                           * value or -INFINITY = no hit (every t lies above its object's epsilon) */
	float dir[3];             /* unit length (the caller's duty: t is in units of |dir|); a NaN component =
	                           * miss, as cast_ray's total-internal-reflection rays */
	uint32_t pad_;
} rtx_ray;
typedef struct rtx_hit {          /* 32 B */
	float t;                  /* hit distance; 0 on a miss (as the z buffer, render.c:304-305) */
	int32_t object;           /* index into rtx_scene_desc.objects; -1 on a miss */
	int32_t material;         /* index into rtx_scene_desc.materials; -1 on a miss */
	uint32_t outside;         /* signbit(n . dir) (render.c:166-167); 0 on a miss */
	float n[3];               /* the normal cast_ray shades with: sphere (P - centre) / r, the triangle's n,
	                           * a plane's n turned to face the ray (object.c:254-265, 356-365, 473-488) */
	uint32_t pad_;
} rtx_hit;
enum {
	RTX_RAYS_ANY_HIT = 1, /* stop at the first hit found with t < tmax (an occlusion test): whether a ray
	                       * hits is exact, but t / object / n are that hit's, not the closest one's */
	RTX_RAYS_REORDER = 2, /* sort the batch for coherence first (key: Morton code of the origin in the
	                       * bounded objects' box, then the direction's octant); results land in input order */
	RTX_RAYS_COUNT = 4    /* fill the traversal counters of rtx_ray_stats (slower kernel instance) */
};
#define RTX_RAYS_MAX 0x7FFFFFFFu /* most rays per call (2^31 - 1) */
/* n rays from / hits to HOST buffers.  n == 0 returns RTX_OK and launches nothing; RTX_ERR_STATE
 * before an upload; RTX_ERR_ARG for a null buffer with n > 0, unknown flag bits or n > RTX_RAYS_MAX.
 * A ray's t never depends on the batch it is in, its order or RTX_RAYS_REORDER (the closest t is
 * a minimum over the accepted hits; box tests only cull); object may differ between two orders
 * only where two objects' intersectors return the very same t (the first one found keeps it). */
int rtx_trace_rays(rtx_ctx *ctx, uint64_t n, const rtx_ray *rays, rtx_hit *hits, uint32_t flags);
/* Same on DEVICE buffers of the context's device (16-byte aligned), enqueued on `stream`
 * (hipStream_t, NULL = the context's own); synchronises the stream.  hits[n..] is not written. */
int rtx_trace_rays_device(rtx_ctx *ctx, uint64_t n, const void *d_rays, void *d_hits, uint32_t flags, void *stream);
/* The width * height primary rays of a frame into a DEVICE buffer, row-major (row 0 = top), tmax =
 * INFINITY: the rays rtx_render traces for it (render.c:353-363), formed by the same device code,
 * so a closest query of them returns the render's z buffer bit for bit (max_bounces >= 1). */
int rtx_frame_rays_device(rtx_ctx *ctx, const rtx_frame *frame, void *d_rays, void *stream);
typedef struct rtx_ray_stats {    /* the last rtx_trace_rays* of the context */
	uint64_t rays, hits;
	/* only with RTX_RAYS_COUNT (as rtx_stats' closest-hit counters) */
	uint64_t node_visits, tri_tests, sphere_tests, plane_tests, far_rays;
	double kernel_ms;         /* k_rays, HIP events */
	double sort_ms;           /* RTX_RAYS_REORDER: key kernel + radix sort (else 0) */
} rtx_ray_stats;
int rtx_get_ray_stats(const rtx_ctx *ctx, rtx_ray_stats *out);

/*
 * Shadow queries: a caller's shadow rays through the render's own shadow query (k_shadow's
 * shadow_query: the planes, the objects it tests one by one, the any-hit walk of the scene's shadow
 * tree with its fast intersectors), with is_light_blocked's semantics (render.c:126-134).
 * rtx_trace_rays(RTX_RAYS_ANY_HIT) answers with the closest-hit kernel's walk instead.
 */
typedef struct rtx_shadow_ray {   /* 32 B */
	float origin[3];
	float dist;               /* the segment's length (finite): objects count with eps < t < dist.  0, a negative
	                           * value or NaN = an idle lane: unblocked, transmittance (1, 1, 1) */
	float dir[3];             /* unit length; a NaN component = an idle lane */
	int32_t light_object;     /* index of the object the ray is aimed at (never blocks or filters it), -1: none */
} rtx_shadow_ray;
typedef struct rtx_shadow_result { /* 16 B */
	float transmittance[3];   /* not blocked: the product of kt over every transparent object hit, each once,
	                           * from (1, 1, 1); blocked: (0, 0, 0) (the walk ends at the first opaque hit) */
	uint32_t blocked;         /* 1: an opaque object other than light_object is hit with eps < t < dist */
} rtx_shadow_result;
enum {
	RTX_SHADOW_RAYS_SLOTS = 1, /* the lane-slot kernels' lane-stack addressing (k_shadow for fewer than 64 lights) */
	RTX_SHADOW_RAYS_COUNT = 2  /* fill the traversal counters of rtx_shadow_ray_stats (counting instance) */
};
/* n rays from / results to HOST buffers.  Ray i runs in lane i % 64 of the 64-ray packet i / 64, with
 * no reordering: a caller chooses which rays share a wave (the walk specialises on a direction
 * octant its live lanes share, takes scalar steps where they sit on one node, and runs its
 * deferred rounds wave-wide), and a ray's result never depends on that choice.  A ray is far where
 * its origin is (rtx_math.h tf_far, as the render marks a shade point).  Errors as rtx_trace_rays:
 * n == 0 returns RTX_OK and launches nothing; RTX_ERR_STATE before an upload; RTX_ERR_ARG for a
 * null buffer with n > 0, unknown flag bits or n > RTX_RAYS_MAX.  Touches neither rtx_stats nor
 * the next render. */
int rtx_trace_shadow_rays(rtx_ctx *ctx, uint64_t n, const rtx_shadow_ray *rays, rtx_shadow_result *results, uint32_t flags);
typedef struct rtx_shadow_ray_stats { /* the last rtx_trace_shadow_rays of the context */
	uint64_t rays, blocked;   /* live rays (not idle), blocked ones */
	/* only with RTX_SHADOW_RAYS_COUNT (as rtx_stats' shadow counters) */
	uint64_t far_rays;        /* far rays that reached the walk (run from the segment's other end) */
	uint64_t box_tests, tri_tests, sphere_tests;
	uint64_t wave_steps, uniform_steps, leaf_rounds, stack_spills;
	double kernel_ms;         /* k_shadow_rays, HIP events */
} rtx_shadow_ray_stats;
int rtx_get_shadow_ray_stats(const rtx_ctx *ctx, rtx_shadow_ray_stats *out);

/*
 * Closest-point queries: the nearest surface point of the uploaded scene to each of a caller's points,
 * and how far it is.
 *
 * THE DEFINITION is rtx_closest_point_object: the distance from a point P to ONE object and that
 * object's closest point cp, in float32 with a fixed operation order (csrc/rtx_nearest_math.h, the one
 * text the host and the device compile, so both return the same bits):
 *   triangle  the closest point of the closed triangle p0, p0 + e1, p0 + e2 (the record's vertex and
 *             edges): the closest points of its three edge segments (the clamp of a segment's
 *             parameter gives the vertex regions) and, where the foot of the perpendicular lies in the
 *             triangle, that foot; the candidate of least squared distance, dist = sqrtf of it.  A
 *             zero-area triangle gives the closest point of the segment or point it collapses to;
 *             never NaN.
 *   sphere    dist = | |P - c| - r |, cp = c + (P - c) (r / |P - c|); P == c: cp = c + (r, 0, 0)
 *   plane     dist = | n . P - d |, cp = P - (n . P - d) n
 * It touches no device and needs no context.  RTX_ERR_ARG for a null pointer or an unknown type.
 */
int rtx_closest_point_object(const rtx_object *obj, const float P[3], float *dist, float cp[3]);

typedef struct rtx_point_query {  /* 16 B */
	float p[3];               /* a NaN or infinite coordinate = a miss */
	float max_dist;           /* answers need dist < max_dist, strictly: an answer's own dist excludes it, the next
	                           * float above keeps it; INFINITY (or NaN) = unbounded; 0, a negative value or
	                           * -INFINITY = a miss */
} rtx_point_query;
typedef struct rtx_closest {      /* 32 B */
	float point[3];           /* the reported object's cp; 0 on a miss */
	float dist;               /* the least dist over the scene's objects; INFINITY on a miss */
	uint32_t object;          /* index into rtx_scene_desc.objects; RTX_NONE on a miss */
	uint32_t material;        /* index into rtx_scene_desc.materials; RTX_NONE on a miss */
	uint32_t pad[2];          /* 0 */
} rtx_closest;
#ifndef RTX_NONE
#define RTX_NONE 0xFFFFFFFFu
#endif
enum {
	RTX_CLOSEST_BOUNDED_ONLY = 1, /* leave the planes out */
	RTX_CLOSEST_REORDER = 2,      /* sort the batch by the point's cell first (30-bit Morton code of the point in
	                               * the bounded objects' box); results land in input order */
	RTX_CLOSEST_COUNT = 4         /* fill the traversal counters of rtx_closest_stats (counting kernel instance) */
};
/* n queries from / results to HOST buffers.  A query's answer is the object of least dist (the definition's)
 * among those with dist < max_dist.  dist never depends on the batch a point is in, its order or
 * RTX_CLOSEST_REORDER (it is a minimum over the objects the search did not prune, and the search prunes only
 * what a deflated lower bound proves farther); object may differ between two orders only where two objects'
 * functions return the very same dist (the first one found keeps it); point is the reported object's cp.
 * Errors as rtx_trace_rays: n == 0 returns RTX_OK and launches nothing; RTX_ERR_STATE before an upload;
 * RTX_ERR_ARG for a null context, a null buffer with n > 0, unknown flag bits or n > RTX_RAYS_MAX.  Like a ray
 * query it renders nothing, leaves rtx_get_stats and the next render as they were, and shares (and may grow) the
 * context's scratch buffers. */
int rtx_closest_points(rtx_ctx *ctx, uint64_t n, const rtx_point_query *queries, rtx_closest *results, uint32_t flags);
/* Same on DEVICE buffers of the context's device (16-byte aligned, RTX_ERR_ARG otherwise), enqueued on
 * `stream` (hipStream_t, NULL = the context's own); synchronises the stream.  results[n..] is not written. */
int rtx_closest_points_device(rtx_ctx *ctx, uint64_t n, const void *d_queries, void *d_results, uint32_t flags, void *stream);
typedef struct rtx_closest_stats { /* the last rtx_closest_points* of the context */
	uint64_t points, found;
	/* only with RTX_CLOSEST_COUNT: node visits of the search, distance-function calls per object type */
	uint64_t node_visits, tri_tests, sphere_tests, plane_tests;
	uint64_t far_points;      /* points far from the bounded objects (more than 4 radii from their centre) */
	double kernel_ms;         /* k_nearest, HIP events */
	double sort_ms;           /* RTX_CLOSEST_REORDER: key kernel + radix sort (else 0) */
} rtx_closest_stats;
int rtx_get_closest_stats(const rtx_ctx *ctx, rtx_closest_stats *out);
/* Known answers of the definition on the DEVICE, without any search (the tests hold the kernel's search and
 * its arithmetic apart with them).  Host buffers; the first device.  rtx_closest_kat: pair i is object
 * object_index[i] (i itself where object_index is NULL) of objects[n_objects] and point points[3 i ..];
 * out[4 i ..] = dist, cp.  rtx_closest_kat_grid: every object to every point, dist[p * n_objects + o].
 * RTX_ERR_ARG for a null buffer, an index out of range or more than RTX_RAYS_MAX pairs. */
int rtx_closest_kat(uint32_t n_objects, const rtx_object *objects, uint64_t n, const uint32_t *object_index,
		    const float *points, float *out);
int rtx_closest_kat_grid(uint32_t n_objects, const rtx_object *objects, uint32_t n_points, const float *points, float *dist);

/*
 * Several devices rendering one frame (the reference's own parallel point is
 * the OpenMP row loop of render.c:349-352).  The group builds the scene's BVHs once, on its
 * first device (rtx_upload_scene's work: device SAH build, 8-wide collapse), and the other
 * devices copy the built records and trees from it over xGMI (peer access enabled at open, one
 * host thread per device); rtx_group_render deals the frame's 8x8 tiles round-robin (tile t ->
 * device t % n), renders every shard on its own host thread, packs each shard into 16-byte
 * {r, g, b, z} records (64 per tile) and gathers them to the first device over RCCL (grouped
 * ncclSend / ncclRecv on xGMI), which unpacks the frame and copies it to the caller.  Pixels
 * are independent and the RNG is counter-based, so the frame is bit-identical for any n.  One
 * host thread calls the group; it must not be shared.
 */
typedef struct rtx_group rtx_group;
enum { RTX_TRANSPORT_NONE = 0, RTX_TRANSPORT_RCCL = 1, RTX_TRANSPORT_LOOPBACK = 2, RTX_TRANSPORT_RCCL_SELF = 3 };

/* n devices: devices[0..n-1], or 0..n-1 when devices is NULL (each must be gfx950, distinct) */
int rtx_group_open(int n, const int *devices, rtx_group **out);
/* Test transport: a group of n shards as n contexts on ONE device.  Everything is the group's
 * own path (scene built once and copied to every context from one host thread each, one host
 * thread per shard, tile pack, unpack, statistics) except the gather, which is a device-to-device
 * copy in place of RCCL send/recv.  Lets a one-GPU machine check rtx_group_render at any n. */
int rtx_group_open_loopback(int n, int device, rtx_group **out);
/* Test transport: a group of ONE device whose gather still runs the RCCL calls: a one-rank
 * communicator (ncclCommInitAll), shard 0 packed, sent to itself with the grouped ncclSend /
 * ncclRecv of rtx_group_render into a NaN-filled buffer and unpacked over the frame.  Lets a
 * one-GPU machine execute the group's RCCL code; the image must equal rtx_render's. */
int rtx_group_open_rccl_self(int device, rtx_group **out);
int rtx_group_size(const rtx_group *g);
int rtx_group_set_builder(rtx_group *g, int builder);
int rtx_group_set_option(rtx_group *g, int option, int64_t value); /* rtx_set_option on every device */
int rtx_group_upload_scene(rtx_group *g, const rtx_scene_desc *scene);
/* params->tile_offset / tile_stride must be 0 / 1: the group shards the frame itself.
 * rgb / z: HOST buffers as for rtx_render (either may be NULL). */
int rtx_group_render(rtx_group *g, const rtx_frame *frame, const rtx_params *params, float *rgb, float *z);
/* ray and traversal counts summed over the devices, kernel times the slowest device's,
 * gather_ms the pack + RCCL + unpack time */
int rtx_group_get_stats(const rtx_group *g, rtx_stats *out);
/* the statistics of device r (0 <= r < rtx_group_size) for the last frame */
int rtx_group_device_stats(const rtx_group *g, int r, rtx_stats *out);
/* rtx_point_stats of the last group render: summed over the devices, and device r's own */
int rtx_group_get_point_stats(const rtx_group *g, rtx_point_stats *out);
int rtx_group_device_point_stats(const rtx_group *g, int r, rtx_point_stats *out);
/* rtx_dark_stats likewise */
int rtx_group_get_dark_stats(const rtx_group *g, rtx_dark_stats *out);
int rtx_group_device_dark_stats(const rtx_group *g, int r, rtx_dark_stats *out);
/* rtx_order_stats likewise */
int rtx_group_get_order_stats(const rtx_group *g, rtx_order_stats *out);
int rtx_group_device_order_stats(const rtx_group *g, int r, rtx_order_stats *out);
/* rtx_premask_stats likewise */
int rtx_group_get_premask_stats(const rtx_group *g, rtx_premask_stats *out);
int rtx_group_device_premask_stats(const rtx_group *g, int r, rtx_premask_stats *out);
/* rtx_clearlane_stats likewise */
int rtx_group_get_clearlane_stats(const rtx_group *g, rtx_clearlane_stats *out);
int rtx_group_device_clearlane_stats(const rtx_group *g, int r, rtx_clearlane_stats *out);
/* What the runtime reports about member r, read back rather than assumed (a line that claims N
 * devices can show that N communicators of one clique formed on N distinct devices) */
typedef struct rtx_group_member {
	int32_t device;           /* the HIP device ordinal of member r */
	int32_t comm_count;       /* ncclCommCount of its RCCL communicator (0: none, n = 1 or loopback) */
	int32_t comm_rank;        /* ncclCommUserRank (-1: none) */
	int32_t comm_device;      /* ncclCommCuDevice (-1: none) */
	uint32_t can_access_peer0; /* hipDeviceCanAccessPeer(device, device of member 0) */
	uint32_t peer0_can_access; /* hipDeviceCanAccessPeer(device of member 0, device) */
	uint32_t peer_enabled;    /* peer access enabled both ways at rtx_group_open (1 for member 0) */
	uint32_t transport;       /* RTX_TRANSPORT_* */
	char pci_bus_id[32];      /* hipDeviceGetPCIBusId */
} rtx_group_member;
int rtx_group_member_info(const rtx_group *g, int r, rtx_group_member *out);
void rtx_group_close(rtx_group *g);

/* The gather's tile records (rtx_tiles.h): shard `offset` of `stride` of a W x H frame packs
 * to rtx_tile_pack_count() records of 4 floats.  Host reference and device versions. */
size_t rtx_tile_pack_count(uint32_t width, uint32_t height, uint32_t offset, uint32_t stride);
int rtx_tile_pack_host(const float *rgb, const float *z, uint32_t width, uint32_t height, uint32_t offset,
		       uint32_t stride, float *out);
int rtx_tile_unpack_host(const float *in, uint32_t width, uint32_t height, uint32_t offset, uint32_t stride,
			 float *rgb, float *z);
int rtx_tile_pack_device(rtx_ctx *ctx, const void *d_rgb, const void *d_z, uint32_t width, uint32_t height,
			 uint32_t offset, uint32_t stride, void *d_out, void *stream);
int rtx_tile_unpack_device(rtx_ctx *ctx, const void *d_in, uint32_t width, uint32_t height, uint32_t offset,
			   uint32_t stride, void *d_rgb, void *d_z, void *stream);

/*
 * Postprocess: the reference's separate `postprocess` binary
 * (src/postprocess/postproc.c:36-188) applied on the device to an rgb+z frame:
 * brighten (-b), depth of field (--dof scale bias | --dof-camera aperture focal plane),
 * mist (--mist start depth falloff r g b), in that order, with the reference's float
 * arithmetic; the DoF scatter is restated as an ordered gather so every output pixel
 * sums its contributions in the reference's order (bit-identical results).
 */
enum { RTX_DOF_NONE = 0, RTX_DOF_SCALE_BIAS = 1, RTX_DOF_CAMERA = 2 };
enum { RTX_FALLOFF_QUAD = 0, RTX_FALLOFF_LIN = 1, RTX_FALLOFF_INV_QUAD = 2 };

typedef struct rtx_post {
	int32_t brighten;           /* -b given (postproc.c:43-47) */
	float brighten_factor;
	int32_t dof;                /* RTX_DOF_* (postproc.c:49-68) */
	float dof_scale, dof_bias;  /* --dof */
	float aperture, focal_length, plane_in_focus; /* --dof-camera */
	int32_t mist;               /* --mist given (postproc.c:70-90) */
	float mist_start, mist_depth;
	int32_t mist_falloff;       /* RTX_FALLOFF_* */
	float mist_color[3];
} rtx_post;

/* rgb[W*H*3] in/out and z[W*H] in, HOST buffers (replaces postprocess() between
 * image_load() and save_image(), src/postprocess/main.c:66-68). */
int rtx_postprocess(rtx_ctx *ctx, uint32_t width, uint32_t height, const rtx_post *post, float *rgb, const float *z);
/* Same on DEVICE buffers, enqueued on `stream` (NULL = the context's stream); synchronises it. */
int rtx_postprocess_device(rtx_ctx *ctx, uint32_t width, uint32_t height, const rtx_post *post, void *d_rgb,
			   const void *d_z, void *stream);

/*
 * Denoiser: per-pixel feature records of a frame's primary hits, and an edge-aware
 * a-trous filter of an rgb frame guided by them.  The features are a closest query of the frame's
 * own rays (rtx_frame_rays_device, then the ray queries' kernel), so z is the render's z buffer bit
 * for bit; a feature call renders nothing and leaves rtx_get_stats, rtx_get_ray_stats and the next
 * render as they were.  The filter needs no uploaded scene (like rtx_postprocess).
 */
typedef struct rtx_feature {      /* 48 B, one per pixel, row-major, row 0 = top */
	float position[3];        /* P = dir * t + origin, formed as the renderer's shade point; 0 on a miss */
	float z;                  /* the primary hit's t (the render's z buffer); 0 on a miss */
	float normal[3];          /* rtx_hit.n; 0 on a miss */
	int32_t material;         /* -1 on a miss */
	float albedo[3];          /* the material's texture colour at P (material.c:152-200), the colour the renderer
	                           * shades the point with; 0 on a miss */
	int32_t object;           /* -1 on a miss */
} rtx_feature;
/* The frame's width * height records into a DEVICE buffer (16-byte aligned), enqueued on `stream` (NULL =
 * the context's own); synchronises it.  u32conv: enum rtx_u32conv, as rtx_params.u32conv of the render.
 * Errors as rtx_frame_rays_device, RTX_ERR_STATE before an upload, RTX_ERR_ARG for another u32conv. */
int rtx_frame_features_device(rtx_ctx *ctx, const rtx_frame *frame, int32_t u32conv, void *d_features, void *stream);
/* Same into a HOST buffer. */
int rtx_frame_features(rtx_ctx *ctx, const rtx_frame *frame, int32_t u32conv, rtx_feature *features);

/*
 * The filter: for level k = 0 .. iterations-1, step s = 2^k and sigma_c,k = sigma_color * 2^-k.  With c
 * the level's input colour and f the features, a pixel i with f_i.z == 0 or a non-finite component of
 * c_i keeps c_i's bits.  Otherwise, over the taps (u, v) in {-2..2}^2 with j = i + (u s, v s) inside
 * the frame, f_j.z != 0 and c_j finite:
 *     e = |c_i-c_j|^2 / sigma_c,k^2 + |n_i-n_j|^2 / sigma_normal^2 + |a_i-a_j|^2 / sigma_albedo^2
 *       + (n_i . (P_j-P_i))^2 / (sigma_plane z_i)^2
 *     w = h[u] h[v] exp(-e),  h = (1/16, 1/4, 3/8, 1/4, 1/16),   out_i = sum w c_j / sum w
 * (n the normal, a the albedo, P the position).  Deterministic: two runs give the same bits.
 */
typedef struct rtx_denoise_params {
	uint32_t iterations;      /* 1..8, default 1 */
	float sigma_color, sigma_normal, sigma_albedo, sigma_plane;   /* each > 0; INFINITY switches its term off.  Defaults
	                           * 0.004 / 0.05 / 0.1 / 0.02; sigma_color is in the frame's own radiance units (the
	                           * default suits raw frames of the order of 1e-4: scale it with the frame) */
} rtx_denoise_params;
void rtx_denoise_params_default(rtx_denoise_params *p);
/* d_features: w * h rtx_feature records, d_rgb: 3 floats per pixel, in/out; DEVICE buffers (d_features 16-byte
 * aligned), enqueued on `stream` (NULL = the context's own); synchronises it.  RTX_ERR_ARG for iterations
 * outside 1..8, a sigma <= 0 or NaN, a null buffer, w * h == 0 or above RTX_RAYS_MAX. */
int rtx_denoise_device(rtx_ctx *ctx, uint32_t w, uint32_t h, const rtx_denoise_params *params, const void *d_features,
		       void *d_rgb, void *stream);
/* Same on HOST buffers. */
int rtx_denoise(rtx_ctx *ctx, uint32_t w, uint32_t h, const rtx_denoise_params *params, const rtx_feature *features,
		float *rgb);
typedef struct rtx_denoise_stats {
	double features_ms;       /* device time of the last rtx_frame_features*: rays, closest query, records (HIP events) */
	double filter_ms;         /* device time of the last rtx_denoise*: every level (HIP events) */
	uint64_t pixels;          /* of the last call of either kind */
	uint64_t hit_pixels;      /* ... of which z != 0 */
	uint32_t iterations;      /* levels the last rtx_denoise* ran */
	uint32_t pad_;
} rtx_denoise_stats;
int rtx_get_denoise_stats(const rtx_ctx *ctx, rtx_denoise_stats *out);

/*
 * The variance-guided filter: the same a-trous filter over the mean and the variance of the
 * mean that rtx_render_passes* / rtx_render_adaptive* write, with the colour distance measured in the pixel's
 * own estimated noise, so sigma_color is a number of standard deviations and does not depend on the frame's
 * units or on how many passes a pixel received.  For level k = 0 .. iterations-1, step s = 2^k, with c the
 * level's input colour, V its per-channel variance and f the features: a pixel is live iff f.z != 0, c is
 * finite and every component of V is finite and >= 0.  A pixel that is not live keeps the bits of its colour
 * and its variance, and no tap reads it.  For a live pixel i:
 *     g_i = the mean of V_r + V_g + V_b over the adjacent (step 1 at every level) live pixels inside the
 *           frame, weights b[u] b[v], b = (1/4, 1/2, 1/4), normalised by the weights of the taps used
 * and over the taps (u, v) in {-2..2}^2 with j = i + (u s, v s) inside the frame and live:
 *     e_c = 0 if |c_i-c_j|^2 == 0, else |c_i-c_j|^2 / (sigma_color^2 2 g_i)      (+inf where g_i == 0)
 *     e   = e_c + |n_i-n_j|^2 / sigma_normal^2 + |a_i-a_j|^2 / sigma_albedo^2
 *         + (n_i . (P_j-P_i))^2 / (sigma_plane z_i)^2
 *     w   = h[u] h[v] exp(-e),  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *     c'_i = c_i + sum w (c_j-c_i) / sum w,     V'_i = sum w^2 V_j / (sum w)^2  (per channel)
 * sigma_color is the same at every level: the shrinking V tightens it.  The 2 is the variance of a difference
 * of two equally noisy estimates.  An all-zero variance (one pass, a deterministic frame) returns the colour's
 * bits.  The variance handed back guides the next level and underestimates the filtered frame's real error
 * after the first level, as the taps are no longer independent: it is not an error bar.  Deterministic: two
 * runs give the same bits.  Needs no uploaded scene.
 */
typedef struct rtx_denoise_variance_params {
	uint32_t iterations;      /* 1..8, default 1 */
	float sigma_color;        /* in standard deviations of a colour difference, > 0; INFINITY = term off.  Default 3 */
	float sigma_normal, sigma_albedo, sigma_plane;   /* as rtx_denoise_params, the same defaults */
} rtx_denoise_variance_params;
void rtx_denoise_variance_params_default(rtx_denoise_variance_params *p);
/* d_features: w * h rtx_feature records, d_rgb and d_variance: 3 floats per pixel each, both in/out, in the layouts
 * rtx_render_passes_device writes; DEVICE buffers (d_features 16-byte aligned), enqueued on `stream` (NULL = the
 * context's own); synchronises it.  Errors as rtx_denoise_device, and RTX_ERR_ARG for a null d_variance.  Fills
 * rtx_denoise_stats (filter_ms, iterations, pixels, hit_pixels) as rtx_denoise_device does. */
int rtx_denoise_variance_device(rtx_ctx *ctx, uint32_t w, uint32_t h, const rtx_denoise_variance_params *params,
				const void *d_features, void *d_rgb, void *d_variance, void *stream);
/* Same on HOST buffers. */
int rtx_denoise_variance(rtx_ctx *ctx, uint32_t w, uint32_t h, const rtx_denoise_variance_params *params,
			 const rtx_feature *features, float *rgb, float *variance);

/*
 * Multi-pass rendering: the frame rendered K times and the passes combined on the device
 * into a per-pixel mean and the variance of that mean.  Pass k has its own seed (params->seed + k), its own
 * sub-pixel offset (anti-aliasing) and its own lens point (a thin lens).  k_trace forms a pixel's ray from
 * nothing but the rtx_frame, so a jittered or thin-lens pass is just another rtx_frame: rtx_pass_frame
 * returns it, and a pass is the frame rtx_render gives for that frame and seed, to the bit.
 */
enum { RTX_PASS_JITTER = 1 };            /* sub-pixel offsets (anti-aliasing) */
#define RTX_PASSES_MAX 65536u
typedef struct rtx_pass_params {
	uint32_t passes;        /* 1..RTX_PASSES_MAX */
	uint32_t flags;         /* RTX_PASS_JITTER or 0 */
	float aperture;         /* lens radius in world units; 0 = pinhole (the default) */
	float focus;            /* aperture > 0: the plane in focus is the image plane scaled about frame->origin
	                         * by this (focus distance / camera focal_length), > 0 */
	float target_error;     /* 0 = run every pass; > 0: stop after the first pass k+1 >= min_passes whose error
	                         * (below) is <= target_error */
	uint32_t min_passes;    /* 2..passes, read only when target_error > 0 */
} rtx_pass_params;
void rtx_pass_params_default(rtx_pass_params *p);   /* 1 pass, no flags, aperture 0, focus 1, target 0, min 2 */
/*
 * The frame of pass k (host only, no device needed).  With phi_b(k) the radical inverse of k in base b, every
 * component evaluated in double from the float inputs and rounded to float once, width and height copied:
 *   offset    (ox, oy) = (0, 0) for k = 0 or without RTX_PASS_JITTER, else (phi_2(k) - 1/2, phi_3(k) - 1/2);
 *             cj = corner + ox step_x + oy step_y
 *   pinhole   (aperture == 0): out = {cj, step_x, step_y, origin}; pass 0 is *frame bit for bit
 *   thin lens (aperture > 0): L = origin for k = 0, else origin + aperture sqrt(phi_5(k)) (cos(2 pi phi_7(k)) x^
 *             + sin(2 pi phi_7(k)) y^), x^ and y^ the unit vectors of step_x and step_y; out.origin = L,
 *             out.corner = origin + focus (cj - origin), out.step_x = focus step_x, out.step_y = focus step_y:
 *             the image plane moves to the plane in focus, so a pixel's rays from every lens point pass
 *             through one focal point
 * RTX_ERR_ARG: a null pointer, k >= passes, passes outside 1..RTX_PASSES_MAX, unknown flag bits, aperture < 0
 * or NaN, aperture > 0 with focus <= 0 or not finite, target_error < 0 or NaN, min_passes outside 2..passes
 * while target_error > 0, a zero-length step_x or step_y while aperture > 0.
 */
int rtx_pass_frame(const rtx_frame *frame, const rtx_pass_params *pp, uint32_t k, rtx_frame *out);
/*
 * Renders rtx_pass_frame(frame, pp, k) with params and seed + k (uint64 wrap) for k = 0 .. passes-1 through
 * rtx_render_device's path and folds each pass into per-pixel, per-channel running state held in double
 * (Welford: d = x - mean, mean += d / (k+1), m2 += d (x - mean)).  With n the number of passes run:
 *   rgb[W*H*3]      = (float)mean
 *   variance[W*H*3] = (float)(m2 / (n (n-1))) per channel, the variance OF THE MEAN; 0 when n = 1
 *   z[W*H]          = pass 0's z (with a pinhole: rtx_render's z buffer bit for bit)
 * HOST buffers; each may be NULL.  A non-finite pass value poisons that pixel's mean as the arithmetic does.
 * The error E = sqrt(sum var_mean) / sum |mean|, both sums over the channels of the pixels whose mean is
 * finite (0 if the denominator is 0), is a deterministic reduction (per-block partial sums in double, added
 * in index order, no atomics): two runs stop after the same pass and return the same bits.
 * params->tile_offset / tile_stride must be 0 / 1.  Errors as rtx_render (RTX_ERR_STATE before an upload),
 * and every rtx_pass_frame error, raised before anything is launched.  rtx_get_stats afterwards describes the
 * last pass.  Device groups: rtx_group_render_passes.
 */
int rtx_render_passes(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
		      float *rgb, float *z, float *variance);
/* Same into DEVICE buffers (16-byte aligned, each may be NULL), enqueued on `stream` (NULL = the context's
 * own); synchronises the stream. */
int rtx_render_passes_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			     void *d_rgb, void *d_z, void *d_variance, void *stream);
typedef struct rtx_pass_stats {   /* the last rtx_render_passes* of the context */
	uint32_t passes_run, pad_;
	double error;            /* the error after the last pass (0 after one pass) */
	double render_ms;        /* sum of the passes' rtx_stats.kernel_ms */
	double accum_ms;         /* the accumulation / error kernels, HIP events */
	uint64_t closest_rays, shadow_rays;   /* summed over the passes */
} rtx_pass_stats;
int rtx_get_pass_stats(const rtx_ctx *ctx, rtx_pass_stats *out);

/*
 * Pixel reconstruction filters for multi-pass rendering.  rtx_render_passes gives a pass's sample
 * to one pixel, a box one pixel wide; the filtered entries give it to every pixel whose filter footprint holds it.
 * In pass k pixel q = (qx, qy) is sampled at q + (ox_k, oy_k) in pixel-index units, (ox_k, oy_k) rtx_pass_frame's
 * offset, each in the open interval (-1/2, 1/2).  The filter is separable, w(dx, dy) = f(dx) f(dy), of radius r
 * pixels:
 *   RTX_FILTER_BOX       f(d) = 1 if -r <= d < r, else 0                                   r in 0.5 .. 2.5
 *   RTX_FILTER_TENT      f(d) = max(0, 1 - |d| / r)                                        r in 1 .. 2.5
 *   RTX_FILTER_GAUSSIAN  f(d) = exp(-alpha d^2) - exp(-alpha r^2) if |d| < r, else 0       r in 1 .. 2.5,
 *                        alpha > 0 and finite (the default: r = 1.5, alpha = 2)
 *   RTX_FILTER_MITCHELL  f(d) = m(|2 d / r|) if |d| < r, else 0, m the Mitchell-Netravali   r in 1 .. 2.5
 *                        cubic with B = C = 1/3, evaluated by Horner's rule as
 *                        m(x) = ((7 x - 12) x x + 16/3) / 6 for x < 1, else (((-7/3 x + 12) x - 20) x + 32/3) / 6
 * all in double from the float parameters.  With r <= 2.5 only the taps dq in -2 .. 2 per axis can carry weight:
 * the stencil is always RTX_FILTER_TAPS x RTX_FILTER_TAPS.  For pass k the host evaluates wx[i] = f(i - 2 + ox_k),
 * wy[j] = f(j - 2 + oy_k); a tap's weight is the double product wx[i] wy[j].
 *
 * For output pixel p and pass k, over the taps q = p + (i - 2, j - 2) that lie inside the frame and whose weight
 * is not 0 (a zero-weight tap is skipped, not multiplied: a non-finite neighbour outside the footprint does not
 * reach p), in row-major tap order (j outer, i inner), per channel and in double:
 *   S_k = sum w c_k(q),  W_k = sum w,  f_k = S_k / W_k
 * and the fold, per channel, on double state (mean, M2, and Wsum per pixel):
 *   k = 0:  mean = f_0, M2 = 0, Wsum = W_0
 *   k > 0:  Wsum += W_k;  d = f_k - mean;  mean += (d W_k) / Wsum;  M2 += (W_k d) (f_k - mean)
 *   rgb = (float)mean,  variance = (float)(M2 / (Wsum (n - 1))), n = k + 1 passes (0 for n = 1),  z = pass 0's z
 * With equal weights this is rtx_render_passes's update; with RTX_FILTER_BOX of radius 0.5 every pass has the one
 * tap q = p of weight 1, and rgb, variance and z are rtx_render_passes's bit for bit.  W_k > 0 always: the tap
 * q = p lies in the frame and has a positive weight under box, tent and Gaussian, and Mitchell's per-axis weight
 * sum stays above 0.05 under every truncation by the frame's border over its radius range.  A non-finite tap of
 * non-zero weight makes p non-finite from then on (as a non-finite pass value does in rtx_render_passes).
 * The error, the stopping rule and rtx_pass_stats are rtx_render_passes's, on the filtered mean and variance; the
 * error's partial sums are per 32x8-pixel tile, so it differs from rtx_render_passes's by double rounding.
 * A filter without RTX_PASS_JITTER is allowed: a plain blur with the weights at integer offsets.
 * Not filtered: rtx_render_adaptive* and the device group's entries (a stopped or foreign tile's neighbours have
 * no sample to gather).
 */
enum { RTX_FILTER_BOX = 0, RTX_FILTER_TENT = 1, RTX_FILTER_GAUSSIAN = 2, RTX_FILTER_MITCHELL = 3 };
#define RTX_FILTER_TAPS 5
typedef struct rtx_filter_params {
	uint32_t kind;          /* RTX_FILTER_* */
	float radius;           /* in pixels, within the kind's range above */
	float alpha;            /* RTX_FILTER_GAUSSIAN's falloff; ignored by the other kinds */
	uint32_t pad_;          /* 0 */
} rtx_filter_params;
void rtx_filter_params_default(rtx_filter_params *p);   /* Gaussian, radius 1.5, alpha 2 */
/* The two weight tables of pass k (host only, no device needed).  RTX_ERR_ARG: a null pointer, every rtx_pass_frame
 * error about pp and k, an unknown kind, a radius outside the kind's range or NaN, a Gaussian alpha <= 0 or not
 * finite, a non-zero pad_. */
int rtx_pass_filter_weights(const rtx_pass_params *pp, const rtx_filter_params *fp, uint32_t k, double wx[RTX_FILTER_TAPS],
			    double wy[RTX_FILTER_TAPS]);
/* rtx_render_passes with the reconstruction filter fp.  HOST buffers; each may be NULL.  Errors: everything
 * rtx_render_passes refuses, with its codes; RTX_ERR_ARG for a null fp, every rtx_pass_filter_weights error about
 * fp, and a frame of more than 2^24 tiles of 32x8 pixels.  A refused call leaves the context and its statistics as
 * they were.  rtx_get_pass_stats afterwards describes this call (accum_ms: the filtered fold's). */
int rtx_render_passes_filtered(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			       const rtx_filter_params *fp, float *rgb, float *z, float *variance);
/* Same into DEVICE buffers (16-byte aligned, each may be NULL), enqueued on `stream` (NULL = the context's
 * own); synchronises the stream. */
int rtx_render_passes_filtered_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params,
				      const rtx_pass_params *pp, const rtx_filter_params *fp, void *d_rgb, void *d_z,
				      void *d_variance, void *stream);

/*
 * Tile-list renders: exactly the tiles the caller names, each bit for bit the tile rtx_render gives for the whole
 * frame (a pixel's random numbers are keyed on the seed and the pixel, and a tile's pixels do not depend on which
 * other tiles are rendered with it).  tiles[i] is a row-major index of an 8x8-pixel tile (tile t covers columns
 * 8 (t % tiles_x) .. and rows 8 (t / tiles_x) .., tiles_x = ceil(W / 8)); the list is strictly increasing and
 * every index lies below the frame's tile count ceil(W / 8) * ceil(H / 8).  Pixels of tiles not in the list keep
 * the caller's values (the host form uploads the caller's buffers first, as rtx_render does for a tile shard).
 * n_tiles == 0 returns RTX_OK and launches nothing.  params->tile_offset / tile_stride must be 0 / 1.
 * rtx_get_stats afterwards describes this render: its ray counts are those of the listed tiles only.
 * RTX_ERR_ARG: a null list with n_tiles > 0, n_tiles above the frame's tile count, a list that is not strictly
 * increasing or holds an index past the last tile; otherwise the errors of rtx_render.
 */
int rtx_render_tiles(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const uint32_t *tiles, uint32_t n_tiles,
		     float *rgb, float *z);
/* Same with DEVICE buffers, the list (4-byte aligned) included, enqueued on `stream` (NULL = the context's own).
 * The list is checked by a kernel whose flag word is read back before anything else is launched. */
int rtx_render_tiles_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const void *d_tiles,
			    uint32_t n_tiles, void *d_rgb, void *d_z, void *stream);

/*
 * Adaptive passes: multi-pass rendering as rtx_render_passes, in which an 8x8 tile stops receiving
 * passes once its share of the frame's error budget is met.  pp is read as by rtx_render_passes (passes is the
 * most any tile receives), with target_error > 0 required.  With T the number of tiles, n_t the passes tile t has
 * received, tau = target_error, and after every pass k
 *   V_t = sum m2 / (n_t (n_t - 1)),  S_t = sum |mean|   over the channels of the tile's pixels with a finite mean,
 *   V = sum V_t,  A = sum S_t   over ALL tiles, stopped ones included, in tile order,
 * tile t receives pass k+1 iff k+1 < min_passes, or it received pass k and V_t T > tau^2 A^2 (in double; a NaN
 * compares false, so the tile stops).  A stopped tile never restarts: the passes folded into tile t are always
 * 0 .. n_t - 1, each the tile as rtx_render_tiles renders it for rtx_pass_frame(frame, pp, k) and seed + k.  The
 * run ends after pass k when no tile is left or k + 1 == passes.
 *   rgb, variance   as rtx_render_passes, per pixel with its tile's n_t (variance 0 where n_t = 1)
 *   z               pass 0's
 *   tile_passes[T]  n_t, row-major tiles
 * HOST buffers; each may be NULL.  Every sum has a fixed order and no atomics: two runs give the same bits and
 * the same counts.
 * The error reported is sqrt(V) / A after the last pass (0 if A == 0), rtx_render_passes's E.  When every tile
 * has stopped on the rule, sum V_t <= tau^2 times the mean of A^2 at the tiles' stops, so E is ABOUT tau; it is
 * NOT guaranteed to be <= tau, because A goes on moving after a tile has stopped.  Read the final error from
 * rtx_get_adaptive_stats.
 * RTX_ERR_ARG: target_error not above 0, and every error of rtx_render_passes, raised before anything is
 * launched.  rtx_get_stats afterwards describes the last pass's tile-list render.  Device groups:
 * rtx_group_render_adaptive.
 */
int rtx_render_adaptive(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			float *rgb, float *z, float *variance, uint32_t *tile_passes);
/* Same into DEVICE buffers (16-byte aligned, each may be NULL), enqueued on `stream` (NULL = the context's
 * own); synchronises the stream. */
int rtx_render_adaptive_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			       void *d_rgb, void *d_z, void *d_variance, void *d_tile_passes, void *stream);
typedef struct rtx_adaptive_stats {   /* the last rtx_render_adaptive* of the context */
	uint32_t passes_run, tiles;      /* R = max n_t, and T */
	uint64_t tile_passes;            /* sum of n_t over the tiles (R T for a run that stopped no tile early) */
	double error;                    /* sqrt(V) / A after the last pass */
	double render_ms;                /* sum of the passes' rtx_stats.kernel_ms */
	double fold_ms;                  /* the fold / select / output kernels, HIP events */
	uint64_t closest_rays, shadow_rays;   /* summed over the passes */
} rtx_adaptive_stats;
int rtx_get_adaptive_stats(const rtx_ctx *ctx, rtx_adaptive_stats *out);

/*
 * Multi-pass and adaptive rendering on a device group.  Member r owns the tiles t = r (mod n)
 * and keeps their Welford state, n_t, V_t and S_t at the GLOBAL tile index, in the arrays a single context holds
 * (48 B per pixel on every member; it never touches the other members' slices).  The fold, the selection and the
 * output are rtx_render_adaptive's own kernels, so every result below is rtx_render_adaptive's to the bit for any
 * number of members.  Host buffers only; every output may be NULL.  The argument errors are those of
 * rtx_render_passes / rtx_render_adaptive (params->tile_offset / tile_stride 0 / 1 included) and a frame of more
 * than 2^25 tiles, all raised before anything is launched; a null group is RTX_ERR_ARG, a call before
 * rtx_group_upload_scene RTX_ERR_STATE.  A refused call leaves the statistics of the last successful one as they were.
 *
 * rtx_group_render_adaptive, per pass k: every member, on its own host thread, list-renders its active tiles
 * (z on pass 0), folds them and packs {V_t, S_t, n_t} of ALL its tiles (24 B each); the records travel to member 0,
 * which scatters them into its global arrays and runs the selection over all T tiles: V, A, the next list and its
 * length are a single context's.  The list travels to every member, which keeps its own tiles in order.  A member
 * with no active tile launches nothing and still takes part in every exchange.  After the last pass every member
 * forms its pixels' mean and variance and packs 32-byte records {mean r, g, b, z, var r, g, b, 0} (rtx_pass_pack_*),
 * which one gather brings to member 0.  tile_passes is member 0's n_t array.  Records and lists move as bits.
 *
 * rtx_group_render_passes: member r renders its tile shard every pass and folds it with the same per-tile kernel;
 * the tile statistics travel only after the passes the stopping rule looks at and after the last.  rgb, z and
 * variance are rtx_render_adaptive's with min_passes == passes, to the bit.  The error is sqrt(V) / A with V and A
 * summed over the tiles in the selection's order, the error rtx_render_adaptive reports: it does not depend on n,
 * and differs from rtx_render_passes's block-strided sum by double rounding only (so a target_error within that
 * rounding of a pass's error may stop the two a pass apart).
 */
int rtx_group_render_passes(rtx_group *g, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			    float *rgb, float *z, float *variance);
/* ray counts summed over members and passes; render_ms the sum over passes of the slowest member's kernel_ms;
 * accum_ms the sum over passes of the slowest member's fold, plus member 0's selection and output kernels */
int rtx_group_get_pass_stats(const rtx_group *g, rtx_pass_stats *out);
int rtx_group_render_adaptive(rtx_group *g, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			      float *rgb, float *z, float *variance, uint32_t *tile_passes);
/* likewise, fold_ms as accum_ms above */
int rtx_group_get_adaptive_stats(const rtx_group *g, rtx_adaptive_stats *out);
typedef struct rtx_group_exchange_stats { /* the last rtx_group_render_passes / rtx_group_render_adaptive */
	uint32_t exchanges;      /* passes after which statistics (and, adaptive, the next list) travelled; 0 when nothing
	                          * travels (one member without RCCL) */
	uint32_t pad_;
	uint64_t bytes;          /* bytes moved between members: every exchange and the final gather */
	double exchange_ms;      /* host wall time of the per-pass exchanges (moves, scatter, list filter, count reads) */
	double gather_ms;        /* host wall time of the final record gather and its unpack */
} rtx_group_exchange_stats;
int rtx_group_get_exchange_stats(const rtx_group *g, rtx_group_exchange_stats *out);

/* The pass records of the gather above: shard `offset` of `stride` of a W x H frame packs to rtx_tile_pack_count()
 * records of 8 floats {mean r, g, b, z, var r, g, b, 0}, 64 per tile in the tile records' pixel order, pixels
 * outside the frame as zeros; every value keeps its bits.  Host reference and device versions; the outputs of an
 * unpack may be NULL. */
int rtx_pass_pack_host(const float *rgb, const float *z, const float *variance, uint32_t width, uint32_t height,
		       uint32_t offset, uint32_t stride, float *out);
int rtx_pass_unpack_host(const float *in, uint32_t width, uint32_t height, uint32_t offset, uint32_t stride, float *rgb,
			 float *z, float *variance);
int rtx_pass_pack_device(rtx_ctx *ctx, const void *d_rgb, const void *d_z, const void *d_variance, uint32_t width,
			 uint32_t height, uint32_t offset, uint32_t stride, void *d_out, void *stream);
int rtx_pass_unpack_device(rtx_ctx *ctx, const void *d_in, uint32_t width, uint32_t height, uint32_t offset,
			   uint32_t stride, void *d_rgb, void *d_z, void *d_variance, void *stream);

/*
 * Feature-guided upsampling with full-resolution tile refinement: the frame rendered at 1/s of the
 * resolution per axis, reconstructed at full resolution by a joint-bilateral upsampler guided by the full-resolution
 * feature records, and the 8x8 tiles in which the low frame has no usable sample re-rendered at full resolution.
 *
 * The low frame.  rtx_frame_scaled (host only, no device needed): out->width = ceil(W / s), out->height =
 * ceil(H / s), step_x and step_y multiplied by s, the origin kept, and
 *     corner_low = corner + ((1 - s) / 2) step_x + ((s - 1) / 2) step_y
 * every component in double from the float fields, rounded to float once.  The renderer forms pixel (col, row)'s
 * plane point as corner + row step_y + (col + 1) step_x (render.c:353-363), so low pixel (c, r) looks through the
 * centre of the s x s block of full pixels (c s .., r s ..) it stands for, the blocks the frame's border cuts off
 * included.  s = 1 returns *frame bit for bit.  The result is an ordinary rtx_frame: every render entry renders it.
 * Full pixel (X, Y) sits at the low coordinates u = (X - (s - 1) / 2) / s, v = (Y - (s - 1) / 2) / s.
 * RTX_ERR_ARG: a null pointer, s outside 1..RTX_UPSAMPLE_SCALE_MAX, an empty frame.
 *
 * The upsampler.  For full pixel p = (X, Y): x0 = floor(u), fx = u - x0 (exactly: with n = 2 X - (s - 1), x0 =
 * floor(n / 2 s) and fx = (n - 2 s x0) / 2 s), likewise y0 and fy.  The taps are the four low pixels q = (x0 + i,
 * y0 + j), i, j in {0, 1}, of bilinear weight b = (i ? fx : 1 - fx) (j ? fy : 1 - fy).  Only the taps inside the low
 * frame with b > 0 are considered (a zero-weight tap is skipped, not multiplied); at least one always remains.
 * With f_p the full frame's record of p, f_q the low frame's record of q and c_q the low frame's colour, a tap is
 * usable iff c_q is finite and q is of p's kind:
 *     both are misses (z == 0):                                                              g = 1
 *     both are hits and (match_material == 0 or material_p == material_q):
 *         e = |n_p - n_q|^2 / sigma_normal^2 + |a_p - a_q|^2 / sigma_albedo^2
 *           + (n_p . (P_q - P_p))^2 / (sigma_plane z_p)^2,                                   g = exp(-e)
 *         where e > RTX_UPSAMPLE_E_MAX or e is NaN (0 * inf) the tap is not usable
 * and every other tap has g = 0.  Over the considered taps in row-major order (j outer, i inner):
 *     out  = sum b g (m o c_q) / sum b g        m = 1, or with demodulate per channel a_p / a_q where both are
 *                                               >= albedo_min and 1 otherwise
 *     conf = sum b g / sum b                    (the denominator over ALL considered taps: an unusable one lowers it)
 * Where sum b g == 0: out = sum b c_q / sum b over the considered taps with a finite colour (0 if there is none) and
 * conf = 0.  The cut at RTX_UPSAMPLE_E_MAX (exp(-32) = 1.3e-14) keeps every weight a normal float whose relative
 * error is bounded; a pixel whose every tap lies beyond it has no usable sample and is better refined than averaged.
 * With s = 1 and the same records on both sides every pixel has its one tap of weight 1 with e = 0: out is the
 * input's bits (a finite colour) and conf is 1, with or without demodulate.  One pixel per lane, no atomics: two
 * runs give the same bits.  Needs no uploaded scene (like rtx_denoise).
 */
#define RTX_UPSAMPLE_SCALE_MAX 8u
#define RTX_UPSAMPLE_E_MAX 32.f
typedef struct rtx_upsample_params {
	uint32_t scale;            /* 1..RTX_UPSAMPLE_SCALE_MAX, default 2 */
	int32_t match_material;    /* default 1: a tap of another material is rejected */
	int32_t demodulate;        /* default 0 */
	float sigma_normal, sigma_albedo, sigma_plane;   /* each > 0; INFINITY switches its term off.  Defaults 0.05 / 0.1 /
	                            * 0.02 (rtx_denoise's) */
	float albedo_min;          /* > 0, default 1/64: below it a channel is not demodulated */
	float refine_threshold;    /* default 0.5; read by rtx_render_upsampled* only */
} rtx_upsample_params;
void rtx_upsample_params_default(rtx_upsample_params *p);
int rtx_frame_scaled(const rtx_frame *frame, uint32_t scale, rtx_frame *out);
/* HOST buffers: low_rgb 3 floats and low_features one record per pixel of the ceil(w / s) x ceil(h / s) low frame,
 * features one record per pixel of the w x h full frame; rgb[w*h*3] and conf[w*h] are written (conf may be NULL).
 * RTX_ERR_ARG before anything is launched: a null context, params or buffer (conf excepted), a scale outside
 * 1..RTX_UPSAMPLE_SCALE_MAX, a sigma or albedo_min that is <= 0 or NaN, w * h == 0 or above RTX_RAYS_MAX. */
int rtx_upsample(rtx_ctx *ctx, uint32_t w, uint32_t h, const rtx_upsample_params *params, const float *low_rgb,
		 const rtx_feature *low_features, const rtx_feature *features, float *rgb, float *conf);
/* Same on DEVICE buffers (both feature buffers 16-byte aligned, RTX_ERR_ARG otherwise; the others 4-byte aligned),
 * enqueued on `stream` (NULL = the context's own); synchronises it. */
int rtx_upsample_device(rtx_ctx *ctx, uint32_t w, uint32_t h, const rtx_upsample_params *params, const void *d_low_rgb,
			const void *d_low_features, const void *d_features, void *d_rgb, void *d_conf, void *stream);
/*
 * The refinement list: the row-major indices of the 8x8 tiles of a w x h frame that hold at least one pixel with
 * conf < threshold (a float compare: a NaN is not below), strictly increasing, which is what rtx_render_tiles
 * accepts; *n_tiles their number.  tiles has room for ceil(w / 8) * ceil(h / 8) entries; entries past *n_tiles are
 * not written.  A per-tile count and an ordered compaction (ballot prefix per wave, the waves' counts added in
 * order), no atomics: the same input gives the same list.  Every conf the upsampler writes lies in 0..1, so a
 * threshold <= 0 gives an empty list and one > 1 every tile.  RTX_ERR_ARG: a null argument, w * h == 0 or above RTX_RAYS_MAX,
 * more than 2^26 tiles.  Fills tiles, refined_tiles and low_conf_pixels of rtx_upsample_stats.
 */
int rtx_upsample_tiles(rtx_ctx *ctx, uint32_t w, uint32_t h, const float *conf, float threshold, uint32_t *tiles,
		       uint32_t *n_tiles);
/* Same with DEVICE conf and tiles (4-byte aligned); n_tiles is a HOST pointer (the call synchronises the stream). */
int rtx_upsample_tiles_device(rtx_ctx *ctx, uint32_t w, uint32_t h, const void *d_conf, float threshold, void *d_tiles,
			      uint32_t *n_tiles, void *stream);
/*
 * The whole pipeline: rtx_frame_scaled(frame, up->scale); rtx_render of the low frame with params as given; the
 * feature records of both frames with params->u32conv; the upsample into rgb; z from the full frame's records
 * (rtx_render's z buffer bit for bit); the tile list at up->refine_threshold; rtx_render_tiles of the full frame
 * over that list with the same params.  Every refined tile is bit for bit the tile rtx_render(frame, params) gives;
 * a threshold > 1 returns rtx_render's rgb and z bit for bit; a threshold <= 0 renders no full-resolution pixel.
 * HOST buffers rgb[W*H*3] and z[W*H]; either may be NULL.
 * RTX_ERR_ARG: a null context, frame, params or up, an empty frame, params->tile_offset / tile_stride other than
 * 0 / 1, and what rtx_upsample refuses about up; RTX_ERR_STATE before an upload; otherwise the errors of rtx_render.
 * All raised before anything is launched.  rtx_get_stats afterwards describes the last render the call made (the
 * refinement, or the low render when no tile was refined); rtx_get_denoise_stats the full frame's feature call.
 */
int rtx_render_upsampled(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_upsample_params *up,
			 float *rgb, float *z);
/* Same into DEVICE buffers (16-byte aligned, either may be NULL), enqueued on `stream` (NULL = the context's own);
 * synchronises the stream. */
int rtx_render_upsampled_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params,
				const rtx_upsample_params *up, void *d_rgb, void *d_z, void *stream);
typedef struct rtx_upsample_stats {   /* the last rtx_upsample*, rtx_upsample_tiles* or rtx_render_upsampled* of the context */
	uint32_t low_width, low_height;  /* the low frame (rtx_upsample*, rtx_render_upsampled*) */
	uint32_t tiles, refined_tiles;   /* T, and the tiles listed (rtx_upsample_tiles*, rtx_render_upsampled*) */
	uint64_t low_conf_pixels;        /* pixels with conf < threshold */
	double low_ms;                   /* rtx_render_upsampled*: the low render's rtx_stats.kernel_ms */
	double features_ms;              /* ... both feature calls, HIP events */
	double upsample_ms;              /* the upsample kernel (rtx_upsample*), the list kernels (rtx_upsample_tiles*), or
	                                  * both and the z copy (rtx_render_upsampled*), HIP events */
	double refine_ms;                /* rtx_render_upsampled*: the refinement's rtx_stats.kernel_ms (0: no tile) */
	uint64_t closest_rays, shadow_rays;   /* rtx_render_upsampled*: summed over both renders */
} rtx_upsample_stats;
int rtx_get_upsample_stats(const rtx_ctx *ctx, rtx_upsample_stats *out);

/*
 * Temporal accumulation: the samples of the frames before carried into the current frame along a
 * camera path, by reprojecting every pixel's world position into the previous frame.  The scene is static between
 * uploads; only the camera moves.
 *
 * The projection.  Pixel (x, y) of a frame looks through corner + y step_y + (x + 1) step_x (render.c:353-363; the
 * + 1 is the reference's).  rtx_frame_project (host only, no device needed), everything in double from the float
 * fields: A = [step_x | step_y | corner - origin] (columns), M = A^-1 (adjugate over determinant), q = M (P - origin),
 *     in_front = q2 > 0,   u = q0 / q2 - 1,   v = q1 / q2
 * so a point seen by pixel (x, y) maps to (u, v) = (x, y).  RTX_ERR_ARG: a null argument, an empty frame, a
 * determinant that is 0 or not finite, a non-finite entry of M; a refused call writes nothing.  The entries below
 * form M once per call, on the host.
 *
 * The accumulation.  w and h are cur_frame's; c the current colour, Vc its variance of the mean, f its records; hc,
 * Vh, L (a float per pixel: the number of frames a pixel's history holds) and g the colour, variance, length and
 * records of the previous frame.  Pixel i = (x, y) is live iff f_i.z != 0 and c_i is finite (and, with variance,
 * every component of Vc_i is finite and >= 0).  A pixel that is not live keeps the bits of c_i and Vc_i and gets
 * length 0, and conf 1 where f_i.z == 0 (a miss has nothing to lose) and 0 otherwise.  For a live pixel (u, v) is
 * P_i = f_i.position projected into prev_frame; IF THE TWO rtx_frame STRUCTS ARE BYTEWISE EQUAL, (u, v) = (x, y) BY
 * DEFINITION (a hit point formed in float projects back up to 2e-3 pixels off its own pixel at 1920x1080, so a static
 * camera would not be the identity numerically).  There is no history unless the point is in front, u and v are
 * finite, -1 < u < w and -1 < v < h.  Otherwise x0 = floor(u), fx = (float)(u - x0), likewise y0 and fy, and the
 * taps are j = (x0 + a, y0 + b), a, b in {0, 1}, of weight b_j = (a ? fx : 1 - fx) (b ? fy : 1 - fy) in float, in
 * row-major order.  A tap is considered iff it lies inside the frame and b_j > 0, and accepted iff L_j >= 1 and
 * finite, hc_j finite (and Vh_j finite and >= 0), g_j.z != 0, the materials equal (when match_material) and
 * e <= RTX_TEMPORAL_E_MAX (a NaN is not), with
 *     e   = |n_i-n_j|^2 / sigma_normal^2 + |a_i-a_j|^2 / sigma_albedo^2 + (n_i . (P_j-P_i))^2 / (sigma_plane z_i)^2
 *     w_j = b_j exp(-e),   S = sum w_j,   conf = S          (the four b sum to 1, so S <= 1)
 *     S > 0:  h = sum w_j hc_j / S,   H = sum w_j^2 Vh_j / S^2,   n = sum w_j L_j
 *             n' = min(n, max_history - 1),   alpha = 1 / (n' + 1)
 *             out = h + alpha (c_i - h),   V = (1 - alpha)^2 H + alpha^2 Vc_i,   len = n' + 1
 *     S = 0:  out = c_i's bits,   V = Vc_i's bits,   len = 1,   conf = 0
 * n is NOT divided by S: weight lost to rejected taps shortens the history.  With a static camera and unchanged
 * records this is the cumulative mean of the frames up to max_history of them and an exponential mean from then on,
 * and V is the exact variance of that weighted mean for independent frames.  After a reprojection the taps are
 * correlated (neighbours share history pixels), so V guides a filter (rtx_denoise_variance) and is no error bar: the
 * caveat rtx_denoise_variance's own variance carries.  View-dependent shading (specular highlights, reflections,
 * refractions) is carried along with the surface point and lags behind a moving camera; max_history bounds the lag.
 * One pixel per lane, no floating-point atomics: two runs give the same bits.  Needs no uploaded scene.
 */
#define RTX_TEMPORAL_HISTORY_MAX 65536u
#define RTX_TEMPORAL_E_MAX 32.f
typedef struct rtx_temporal_params {
	uint32_t max_history;     /* 1..RTX_TEMPORAL_HISTORY_MAX, default 32: the new frame's weight never falls below 1/max_history */
	int32_t match_material;   /* default 1: a tap of another material is rejected */
	float sigma_normal, sigma_albedo, sigma_plane;   /* each > 0; INFINITY switches its term off.  Defaults 0.05 / 0.1 /
	                           * 0.02 (rtx_denoise's) */
	uint32_t pad_;
} rtx_temporal_params;
void rtx_temporal_params_default(rtx_temporal_params *p);
int rtx_frame_project(const rtx_frame *frame, const float P[3], double *u, double *v, int *in_front);
/* HOST buffers of cur_frame's w x h pixels: rgb, variance, hist_rgb, hist_variance, out_rgb and out_variance 3 floats per
 * pixel, hist_length, out_length and out_conf one, features and hist_features one record.  variance, out_variance and
 * (where there is a history) hist_variance are all given or all NULL.  prev_frame, hist_rgb, hist_length and
 * hist_features are all given or all NULL (then hist_variance is NULL too); all NULL means the first frame: every live
 * pixel takes the S = 0 branch.  out_conf may be NULL.  The outputs may alias the current inputs (out_rgb == rgb,
 * out_variance == variance): a pixel's outputs depend on the current frame through that pixel alone.  They may not
 * overlap the history.
 * RTX_ERR_ARG before anything is launched: a null context, params, cur_frame, rgb, features, out_rgb or out_length,
 * the pointer rules above, an output that overlaps a history buffer, max_history outside
 * 1..RTX_TEMPORAL_HISTORY_MAX, a sigma that is <= 0 or NaN, w * h == 0 or above RTX_RAYS_MAX, a prev_frame of another
 * size, and what rtx_frame_project refuses about prev_frame. */
int rtx_temporal(rtx_ctx *ctx, const rtx_temporal_params *params, const rtx_frame *cur_frame, const float *rgb,
		 const float *variance, const rtx_feature *features, const rtx_frame *prev_frame, const float *hist_rgb,
		 const float *hist_variance, const float *hist_length, const rtx_feature *hist_features, float *out_rgb,
		 float *out_variance, float *out_length, float *out_conf);
/* Same on DEVICE buffers (both feature buffers 16-byte aligned, RTX_ERR_ARG otherwise; the others 4-byte aligned),
 * enqueued on `stream` (NULL = the context's own); synchronises it. */
int rtx_temporal_device(rtx_ctx *ctx, const rtx_temporal_params *params, const rtx_frame *cur_frame, const void *d_rgb,
			const void *d_variance, const void *d_features, const rtx_frame *prev_frame, const void *d_hist_rgb,
			const void *d_hist_variance, const void *d_hist_length, const void *d_hist_features, void *d_out_rgb,
			void *d_out_variance, void *d_out_length, void *d_out_conf, void *stream);
/*
 * The pipeline along a camera path: rtx_render_passes_device of the frame; rtx_frame_features_device with
 * params->u32conv; rtx_temporal_device against the history the context holds, which is the previous call's rgb,
 * variance, length, records and rtx_frame (two sets of device buffers used in turn, 76 bytes per pixel each); the
 * results become the history.  There is no history on the first call, after rtx_temporal_reset, after
 * rtx_upload_scene, and when the frame's size differs from the history's.  rgb, variance and length are bit for bit
 * what the three public calls chained by hand give, z is the render's.
 * THE CALLER VARIES params->seed FROM FRAME TO FRAME (by at least pp->passes, as pass k renders with seed + k): with
 * the same seed successive frames are correlated and the variance is wrong.
 * HOST buffers rgb[W*H*3], z[W*H], variance[W*H*3], length[W*H]; each may be NULL.
 * Errors as rtx_render_passes (RTX_ERR_STATE before an upload) and what rtx_temporal refuses about tp, all raised
 * before anything is launched; a failed call leaves the history as it was.  rtx_get_stats and rtx_get_pass_stats
 * afterwards describe the call's render as they would after rtx_render_passes, rtx_get_denoise_stats its feature call.
 * Not covered: device groups, the filtered and the adaptive renders as the first step (chain rtx_temporal after them),
 * objects that move.
 */
int rtx_render_temporal(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			const rtx_temporal_params *tp, float *rgb, float *z, float *variance, float *length);
/* Same into DEVICE buffers (16-byte aligned, each may be NULL), enqueued on `stream` (NULL = the context's own);
 * synchronises the stream. */
int rtx_render_temporal_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_params *params, const rtx_pass_params *pp,
			       const rtx_temporal_params *tp, void *d_rgb, void *d_z, void *d_variance, void *d_length,
			       void *stream);
/* Forgets the context's history (its buffers stay allocated): the next rtx_render_temporal* is a first frame. */
int rtx_temporal_reset(rtx_ctx *ctx);
typedef struct rtx_temporal_stats {   /* the last rtx_temporal* or rtx_render_temporal* of the context */
	uint32_t frames, pad_;           /* rtx_render_temporal*: calls since the history was last forgotten, this one included;
	                                  * rtx_temporal*: 0 */
	double render_ms;                /* rtx_render_temporal*: rtx_pass_stats' render_ms + accum_ms of the call's render */
	double features_ms;              /* ... its feature call, HIP events */
	double temporal_ms;              /* the accumulation kernel, HIP events */
	uint64_t pixels;                 /* w * h */
	uint64_t live_pixels;            /* ... of which live */
	uint64_t history_pixels;         /* live pixels with S > 0 */
	uint64_t reset_pixels;           /* live pixels with S == 0: live_pixels = history_pixels + reset_pixels */
	uint64_t closest_rays, shadow_rays;   /* rtx_render_temporal*: the call's render */
} rtx_temporal_stats;
int rtx_get_temporal_stats(const rtx_ctx *ctx, rtx_temporal_stats *out);

/*
 * A frame whose primary rays are the caller's: the renderer's whole shading (ray trees, path GI,
 * area lights) behind any camera.  rays: width * height rtx_ray records, row-major, row 0 = top; pixel (px, py)
 * traces record py * width + px from its origin along its dir, and everything after that ray is rtx_render's:
 * the pixel's RNG key is (seed, py * width + px), so a pixel's value depends on its own record, its index and the
 * parameters alone, never on its neighbours' records.  Of the frame's own rays (rtx_frame_rays_device) the image is
 * rtx_render's bit for bit, rgb and z.  A record follows rtx_ray, with these rules for a primary ray:
 *   hole       tmax of 0, a negative value or -INFINITY: nothing is traced or counted, the pixel is rgb 0 and z 0;
 *   unbounded  every other tmax, a finite positive one, INFINITY and NaN alike: a primary ray is not clipped
 *              (clipping at a finite tmax is not built);
 *   NaN dir    a NaN direction component is a traced miss (rgb 0, z 0, one closest ray), as in rtx_trace_rays.
 * dir is unit length, the caller's duty (z is in units of |dir|).
 * The call honours tile_offset / tile_stride and fills rtx_get_stats and the per-feature statistics as rtx_render
 * does.  It leaves the next rtx_render's chunk sizing as it was (the estimate is keyed by a camera, which a batch
 * has not); its own chunks take the static bound, and the overflow retry.
 * HOST buffers; rgb[W*H*3] and z[W*H] may each be NULL.  RTX_ERR_STATE before an upload; RTX_ERR_ARG for a null
 * context, rays or params, a zero dimension, width * height > RTX_RAYS_MAX, bad tile sharding, max_bounces above the
 * limit.  Not covered: device groups; tile lists, adaptive, multi-pass, filtered, upsampled and temporal renders of
 * a batch; a finite primary tmax.
 */
int rtx_render_rays(rtx_ctx *ctx, uint32_t width, uint32_t height, const rtx_ray *rays, const rtx_params *params, float *rgb,
		    float *z);
/* Same on DEVICE buffers (d_rays 16-byte aligned; d_rgb / d_z may each be NULL), enqueued on `stream` (NULL = the
 * context's own); synchronises the stream. */
int rtx_render_rays_device(rtx_ctx *ctx, uint32_t width, uint32_t height, const void *d_rays, const rtx_params *params,
			   void *d_rgb, void *d_z, void *stream);
/* rtx_frame_features* with the caller's rays in place of the frame's own: a closest query of the batch (the ray
 * queries' kernel), then the records.  A hole gives a miss record; on a batch of unbounded rays z is
 * rtx_render_rays' z bit for bit (max_bounces >= 1).  (The query is rtx_trace_rays': a finite positive tmax does
 * clip here.)  Errors as rtx_frame_features*, with the batch's size for the frame's. */
int rtx_ray_features(rtx_ctx *ctx, uint32_t width, uint32_t height, const rtx_ray *rays, int32_t u32conv,
		     rtx_feature *features);
int rtx_ray_features_device(rtx_ctx *ctx, uint32_t width, uint32_t height, const void *d_rays, int32_t u32conv,
			    void *d_features, void *stream);

/*
 * Camera models on top of it: a panoramic, a fisheye and an orthographic camera that looks where the pinhole
 * rtx_frame looks.  From the frame, in double:
 *     r = unit(step_x),  dn = unit(step_y),  f = +-(r x dn), the sign such that
 *     f . (corner + (W/2) step_x + (H/2) step_y - origin) > 0
 * (RTX_ERR_ARG for a step of zero length, for |r . dn| > 1e-3, which is no rectangle, and for an origin in the image
 * plane).  With u = (px + 1/2 + offset_x) / W and v = (py + 1/2 + offset_y) / H:
 *   RTX_PROJ_PANORAMA (equirectangular), fov in (0, 2 pi], the angle across the width:
 *     lambda = (u - 1/2) fov,   phi = (1/2 - v) pi (fov / (2 pi)) (2 H / W);   |phi| > pi/2: a hole
 *     d = cos phi (sin lambda r + cos lambda f) - sin phi dn,   origin = the frame's
 *     (a 2:1 image at fov 2 pi spans the full sphere)
 *   RTX_PROJ_FISHEYE (equidistant), fov in (0, 2 pi], the full angle across the width:
 *     x = 2u - 1,  y = (2v - 1) H / W,  rho = sqrt(x^2 + y^2),  theta = rho fov / 2;   theta > pi: a hole
 *     d = cos theta f + sin theta (x r + y dn) / rho,   d = f at rho = 0,   origin = the frame's
 *   RTX_PROJ_ORTHO:
 *     d = f,   origin = origin + (u - 1/2) E r + (v - 1/2) E (H / W) dn,
 *     E = extent, the width of the view in scene units; 0: the image plane's own width W |step_x|
 * Every formula is evaluated in double and each component rounded once to float; a ray has tmax = INFINITY, a hole is
 * an all-zero record (tmax 0).  offset_x / offset_y are sub-pixel offsets in pixels: a caller anti-aliases by moving
 * them and averaging renders of different seeds (rtx_render_passes does not do it for a projection).
 * (2 pi rounded to float, the default fov, lies just above 2 pi and is accepted.)
 */
enum { RTX_PROJ_PANORAMA = 0, RTX_PROJ_FISHEYE = 1, RTX_PROJ_ORTHO = 2 };
typedef struct rtx_projection {
	int32_t kind;             /* RTX_PROJ_* */
	float fov;                /* panorama, fisheye: radians, in (0, 2 pi] */
	float extent;             /* ortho: E >= 0, finite */
	float offset_x, offset_y; /* finite */
} rtx_projection;
/* panorama, fov 2 pi, extent 0, offsets 0 */
void rtx_projection_default(rtx_projection *p);
/* THE DEFINITION: pixel (px, py)'s ray by the formulas above, on the host, no device needed.  RTX_ERR_ARG for a null
 * argument, a frame with a zero dimension or more than RTX_RAYS_MAX pixels or a non-finite field, the frame rules
 * above, an unknown kind, a fov or extent outside its range, a non-finite offset, a pixel outside the frame. */
int rtx_projection_ray(const rtx_frame *frame, const rtx_projection *proj, uint32_t px, uint32_t py, rtx_ray *out);
/* The frame's width * height rays into a DEVICE buffer (16-byte aligned), formed by the device in double by the same
 * text, enqueued on `stream` (NULL = the context's own); synchronises it.  Needs no uploaded scene.  Against
 * rtx_projection_ray a component can differ by one float ulp, where the two doubles straddle a rounding boundary. */
int rtx_projection_rays_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_projection *proj, void *d_rays, void *stream);
/* The generator into a scratch buffer of the context, then rtx_render_rays_device: bit for bit what the two calls
 * chained by hand give.  HOST buffers as rtx_render_rays.  Errors as the two calls, all but the sharding and
 * max_bounces raised before anything is launched. */
int rtx_render_projection(rtx_ctx *ctx, const rtx_frame *frame, const rtx_projection *proj, const rtx_params *params,
			  float *rgb, float *z);
/* Same into DEVICE buffers. */
int rtx_render_projection_device(rtx_ctx *ctx, const rtx_frame *frame, const rtx_projection *proj, const rtx_params *params,
				 void *d_rgb, void *d_z, void *stream);

/*
 * Known-answer entry: evaluates one device function over n inputs on the GPU
 * (used by the -m gpu parity tests against the oracle's KAT fixtures).
 * kind / record layouts are listed in rtx_kat.h.
 */
int rtx_kat(int kind, uint32_t n, const float *in, float *out, const rtx_params *params);

#ifdef __cplusplus
}
#endif

#endif /* RTX_H */
