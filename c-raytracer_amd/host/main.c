/*
 * engine — drop-in for the reference CLI (src/raytracer/main.c:57-89):
 *
 *   engine <input.json> <output.tif> <resX> <resY> [flags]
 *
 * Same flow: system_init -> scene_load -> image_init -> accel_init ->
 * render_init -> render -> save_image, with accel_init/render replaced by the
 * MI355X path (rtx_upload_scene / rtx_render) and the host glue from
 * librtxscene.  Reference flags: -m -b -a -s -n -r -l -o -p -g -f (HELPTEXT,
 * main.c:23-53; -o is undocumented there).  Extensions:
 *   --gpus N     render on N devices (rtx_group: BVH built once, tiles dealt round-robin,
 *                shards gathered to the first device over RCCL)
 *   --device D   first device (default 0)
 *   --seed S     counter-RNG seed (default 1)
 *   --rng const  every rand_flt() draw = 0.5 (the oracle's REF_CONST_RNG)
 *   --rng counter  counter-based i.i.d. draws like rand_flt (the default)
 *   --rng strat    the same stream with the light samples stratified (opt-in, another estimator)
 *   --u32 wrap   float->uint32 texture conversion of a generic x86-64 build
 *                (default: AVX-512 saturating, like -march=native on AVX-512 hosts)
 *   --denoise    the rendered rgb through rtx_frame_features + rtx_denoise (defaults) before it is saved
 *   --passes K   the frame rendered K times (seed + k) and the passes' mean saved (rtx_render_passes)
 *   --aa         pass k at its own sub-pixel offset (RTX_PASS_JITTER); 16 passes unless --passes is given
 *   --lens APERTURE FOCUS_DISTANCE   a thin lens of that radius focused at that distance (world units),
 *                pass k from its own lens point; 16 passes unless --passes is given
 *   --target-error E   stop after the first pass (of at least 2) whose error estimate is <= E
 *   --adaptive   with --target-error E: each 8x8 tile stops receiving passes once its share of the error
 *                budget is met (rtx_render_adaptive); 16 passes at most unless --passes is given
 *                The multi-pass flags render on one device; --denoise then filters the mean.
 *   --denoise-variance   with a multi-pass flag: the render also returns the variance of the mean, and the mean
 *                goes through rtx_frame_features + rtx_denoise_variance (defaults) before it is saved (before
 *                --denoise, where both are given)
 *   --filter box|tent|gaussian|mitchell [--filter-radius R] [--filter-alpha A]   a pixel reconstruction filter
 *                wider than the pixel (rtx_render_passes_filtered; defaults: radius 1.5, Gaussian alpha 2); implies
 *                --aa; composes with --lens, --target-error, --denoise and --denoise-variance, not with --adaptive
 *   --upsample S [--refine T]   the frame rendered at 1/S of the resolution per axis (S in 1..8), upsampled under the
 *                guidance of the full-resolution feature records, and the 8x8 tiles that hold a pixel of confidence
 *                below T (default 0.5) re-rendered at full resolution (rtx_render_upsampled).  One GPU; implies
 *                nothing else, composes with --denoise, not with the multi-pass flags
 *   --projection panorama | fisheye DEGREES | ortho EXTENT   another camera model that looks where the scene's camera
 *                looks (rtx_render_projection): an equirectangular panorama of the full 360 degrees across the width, an
 *                equidistant fisheye of that full angle across the width, or an orthographic view EXTENT scene units wide
 *                (0: the image plane's own width).  One GPU; composes with --denoise (rtx_ray_features of the
 *                rtx_projection_ray rays), not with the multi-pass flags or --upsample
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "rtx.h"
#include "rtx_scene.h"

static const char *HELPTEXT =
	"Render a scene using raytracing (MI355X / gfx950 path).\n"
	"Usage: ./engine <input> <output> <resolution> [OPTIONAL_PARAMETERS]\n"
	"\n"
	"REQUIRED PARAMETERS:\n"
	"<input>      (string)            : .json scene file.\n"
	"<output>     (string)            : .tif file to which the image will be saved.\n"
	"<resolution> (integer) (integer) : resolution of the output image.\n"
	"OPTIONAL PARAMETERS:\n"
	"[-m] (integer | \"max\")           : accepted for compatibility (CPU threads; unused)\n"
	"[-b] (integer)                   : DEFAULT = 10      : maximum number of times that a light ray can bounce.\n"
	"[-a] (float)                     : DEFAULT = 0.01    : minimum light intensity for which a ray is cast.\n"
	"[-s] (\"phong\" | \"blinn\")         : DEFAULT = phong   : reflection model.\n"
	"[-n] (integer)                   : DEFAULT = 1       : number of samples which are rendered per pixel.\n"
	"[-r] (\"norm\" | float)            : DEFAULT = 1.0     : scene scaling factor.\n"
	"[-l] (\"none\" | \"lin\" | \"sqr\")    : DEFAULT = sqr     : light attenuation.\n"
	"[-o] (float)                     : DEFAULT = 1.0     : light attenuation offset.\n"
	"[-p] (\"real\" | \"cpu\")            : DEFAULT = real    : time to print with status messages.\n"
	"[-g] (string)                    : DEFAULT = ambient : global illumination model (ambient | path).\n"
	"[-f]                             : DEFAULT = OFF     : save raw output for post-processing.\n"
	"[--gpus N] [--device D] [--seed S] [--rng counter|strat|const] [--u32 sat|wrap]\n"
	"[--denoise]                      : DEFAULT = OFF     : filter the image with the edge-aware denoiser before saving.\n"
	"[--passes] (integer)             : DEFAULT = 1       : render the frame this many times (seed + k) and save the mean.\n"
	"[--aa]                           : DEFAULT = OFF     : anti-aliasing: every pass at its own sub-pixel offset (16 passes unless --passes).\n"
	"[--lens] (float) (float)         : DEFAULT = OFF     : thin lens: aperture radius and focus distance (16 passes unless --passes).\n"
	"[--target-error] (float)         : DEFAULT = 0       : stop once the passes' error estimate is at most this (one GPU only).\n"
	"[--adaptive]                     : DEFAULT = OFF     : with --target-error: a tile stops receiving passes once its share of the error is met.\n"
	"[--denoise-variance]             : DEFAULT = OFF     : with --passes, --aa, --lens, --target-error or --adaptive: filter the mean guided by its variance.\n"
	"[--filter] (box | tent | gaussian | mitchell) : DEFAULT = OFF : pixel reconstruction filter over the passes; implies --aa (not with --adaptive, one GPU only).\n"
	"[--filter-radius] (float)        : DEFAULT = 1.5     : with --filter: the filter's radius in pixels (box 0.5..2.5, the others 1..2.5).\n"
	"[--filter-alpha] (float)         : DEFAULT = 2       : with --filter gaussian: the falloff exp(-alpha d^2).\n"
	"[--upsample] (integer)           : DEFAULT = OFF     : render at 1/S of the resolution per axis (S in 1..8), upsample guided by the full-resolution features, refine the uncertain tiles (one GPU only, not with the multi-pass flags).\n"
	"[--refine] (float)               : DEFAULT = 0.5     : with --upsample: re-render at full resolution the 8x8 tiles that hold a pixel of confidence below this.\n"
	"[--projection] (panorama | fisheye DEGREES | ortho EXTENT) : DEFAULT = OFF : a 360 degree panorama, an equidistant fisheye of that angle across the width, or an orthographic view that wide, looking where the camera looks (one GPU only, not with the multi-pass flags or --upsample).\n";

static struct timespec t0;
static int log_cpu = 0;

static double now_s(void)
{
	if (log_cpu)
		return (double)clock() / CLOCKS_PER_SEC;
	struct timespec t;
	timespec_get(&t, TIME_UTC);
	return (t.tv_sec - t0.tv_sec) + (t.tv_nsec - t0.tv_nsec) * 1e-9;
}

#define LOG(fmt, ...) printf("[%08.3f] %10s:%18s:%3u: " fmt "\n", now_s(), "main.c", __func__, __LINE__, ##__VA_ARGS__)

static int argv_find(int argc, char **argv, const char *flag, int nargs)
{
	uint32_t h = rtx_hash_djb(flag);
	for (int i = 1; i < argc; i++)
		if (rtx_hash_djb(argv[i]) == h)
			return (i + nargs < argc) ? i : 0;
	return 0;
}

int main(int argc, char **argv)
{
	timespec_get(&t0, TIME_UTC);
	if (argv_find(argc, argv, "--help", 0) || argv_find(argc, argv, "-h", 0)) {
		puts(HELPTEXT);
		return 0;
	} else if (argc < 5) {
		puts("Too few arguments. Use --help to find out which arguments are required to call this program.");
		return 1;
	}
	int idx;
	if ((idx = argv_find(argc, argv, "-p", 1)) && rtx_hash_djb(argv[idx + 1]) == 193416643u)
		log_cpu = 1;

	rtx_params p;
	rtx_params_default(&p);
	rtx_params_from_argv(argc, argv, &p);
	int ngpu = 1, dev0 = 0;
	if ((idx = argv_find(argc, argv, "--gpus", 1)))
		ngpu = atoi(argv[idx + 1]);
	if ((idx = argv_find(argc, argv, "--device", 1)))
		dev0 = atoi(argv[idx + 1]);
	if ((idx = argv_find(argc, argv, "--seed", 1)))
		p.seed = strtoull(argv[idx + 1], NULL, 10);
	if ((idx = argv_find(argc, argv, "--rng", 1)) && !strcmp(argv[idx + 1], "const"))
		p.rng = RTX_RNG_CONST;
	if ((idx = argv_find(argc, argv, "--rng", 1)) && !strcmp(argv[idx + 1], "counter"))
		p.rng = RTX_RNG_COUNTER;
	if ((idx = argv_find(argc, argv, "--rng", 1)) && !strcmp(argv[idx + 1], "strat"))
		p.rng = RTX_RNG_STRAT;
	if ((idx = argv_find(argc, argv, "--u32", 1)) && !strcmp(argv[idx + 1], "wrap"))
		p.u32conv = RTX_U32_WRAP;
	if (ngpu < 1)
		ngpu = 1;
	/* multi-pass rendering (rtx_render_passes): any of its flags turns it on, on one context */
	rtx_pass_params pp;
	rtx_pass_params_default(&pp);
	int multipass = 0, lens = 0;
	double focus_distance = 0.0;
	if ((idx = argv_find(argc, argv, "--passes", 1))) {
		pp.passes = (uint32_t)strtoul(argv[idx + 1], NULL, 10);
		multipass = 1;
	}
	if (argv_find(argc, argv, "--aa", 0)) {
		pp.flags |= RTX_PASS_JITTER;
		if (!multipass)
			pp.passes = 16;
		multipass = 1;
	}
	if ((idx = argv_find(argc, argv, "--lens", 2))) {
		pp.aperture = (float)atof(argv[idx + 1]);
		focus_distance = atof(argv[idx + 2]);
		if (!multipass)
			pp.passes = 16;
		multipass = lens = 1;
	}
	if ((idx = argv_find(argc, argv, "--target-error", 1))) {
		pp.target_error = (float)atof(argv[idx + 1]);
		multipass = 1;
	}
	/* a reconstruction filter (rtx_render_passes_filtered): the jittered passes gathered through it */
	rtx_filter_params fp;
	rtx_filter_params_default(&fp);
	int filtered = 0;
	for (int i = 1; i < argc; i++)
		if (!strcmp(argv[i], "--filter"))
			filtered = 1;
	if (filtered) {
		static const char *const kinds[] = { "box", "tent", "gaussian", "mitchell" };
		const char *name = (idx = argv_find(argc, argv, "--filter", 1)) ? argv[idx + 1] : "";
		uint32_t kind = 0;
		while (kind < 4 && strcmp(name, kinds[kind]))
			kind++;
		if (kind == 4) {
			LOG("--filter needs one of box, tent, gaussian, mitchell, not '%s'.", name);
			return 1;
		}
		fp.kind = kind;
		if ((idx = argv_find(argc, argv, "--filter-radius", 1)))
			fp.radius = (float)atof(argv[idx + 1]);
		if ((idx = argv_find(argc, argv, "--filter-alpha", 1)))
			fp.alpha = (float)atof(argv[idx + 1]);
		pp.flags |= RTX_PASS_JITTER;
		if (!argv_find(argc, argv, "--passes", 1))
			pp.passes = 16;
		multipass = 1;
		if (argv_find(argc, argv, "--adaptive", 0)) {
			LOG("--filter does not combine with --adaptive: a stopped tile's neighbours have no sample to gather.");
			return 1;
		}
		if (ngpu > 1) {
			LOG("--filter renders on one GPU, not on %d.", ngpu);
			return 1;
		}
		double wx[RTX_FILTER_TAPS], wy[RTX_FILTER_TAPS];
		if (rtx_pass_filter_weights(&pp, &fp, 0, wx, wy)) {
			LOG("%s", rtx_last_error());
			return 1;
		}
	} else if (argv_find(argc, argv, "--filter-radius", 0) || argv_find(argc, argv, "--filter-alpha", 0)) {
		LOG("--filter-radius and --filter-alpha need --filter.");
		return 1;
	}
	const int adaptive = argv_find(argc, argv, "--adaptive", 0) != 0;
	if (adaptive) {
		if (!(pp.target_error > 0.f)) {
			LOG("--adaptive needs --target-error E with E above 0.");
			return 1;
		}
		if (!argv_find(argc, argv, "--passes", 1))
			pp.passes = 16;
		multipass = 1;
	}
	const int denoise_variance = argv_find(argc, argv, "--denoise-variance", 0) != 0;
	if (denoise_variance && !multipass) {
		LOG("--denoise-variance needs a multi-pass flag: --passes, --aa, --lens, --target-error or --adaptive.");
		return 1;
	}
	if (multipass && ngpu > 1) {
		LOG("--passes, --aa, --lens, --target-error and --adaptive render on one GPU, not on %d.", ngpu);
		return 1;
	}
	/* feature-guided upsampling (rtx_render_upsampled): a low-resolution render, refined where it is uncertain */
	rtx_upsample_params up;
	rtx_upsample_params_default(&up);
	int upsample = 0;
	for (int i = 1; i < argc; i++)
		if (!strcmp(argv[i], "--upsample"))
			upsample = 1;
	if (upsample) {
		const long S = (idx = argv_find(argc, argv, "--upsample", 1)) ? strtol(argv[idx + 1], NULL, 10) : 0;
		if (S < 1 || S > (long)RTX_UPSAMPLE_SCALE_MAX) {
			LOG("--upsample needs a scale in 1..%u.", RTX_UPSAMPLE_SCALE_MAX);
			return 1;
		}
		up.scale = (uint32_t)S;
		if ((idx = argv_find(argc, argv, "--refine", 1)))
			up.refine_threshold = (float)atof(argv[idx + 1]);
		if (ngpu > 1) {
			LOG("--upsample renders on one GPU, not on %d.", ngpu);
			return 1;
		}
		if (multipass || denoise_variance) {
			LOG("--upsample does not combine with --passes, --aa, --lens, --filter, --adaptive, --target-error or "
			    "--denoise-variance: render the scaled frame (rtx_frame_scaled) through the library instead.");
			return 1;
		}
	} else if (argv_find(argc, argv, "--refine", 0)) {
		LOG("--refine needs --upsample.");
		return 1;
	}
	/* a camera model other than the pinhole (rtx_render_projection): the scene's camera gives the view direction */
	rtx_projection proj;
	rtx_projection_default(&proj);
	int projection = 0;
	for (int i = 1; i < argc; i++)
		if (!strcmp(argv[i], "--projection"))
			projection = i;
	if (projection) {
		const char *name = projection + 1 < argc ? argv[projection + 1] : "";
		const char *arg = projection + 2 < argc ? argv[projection + 2] : NULL;
		if (!strcmp(name, "panorama")) {
			proj.kind = RTX_PROJ_PANORAMA;
		} else if (!strcmp(name, "fisheye") && arg) {
			proj.kind = RTX_PROJ_FISHEYE;
			proj.fov = (float)(atof(arg) * (3.14159265358979323846 / 180.0));
			if (!(proj.fov > 0.f) || atof(arg) > 360.0) {
				LOG("--projection fisheye needs an angle in (0, 360] degrees, not '%s'.", arg);
				return 1;
			}
		} else if (!strcmp(name, "ortho") && arg) {
			proj.kind = RTX_PROJ_ORTHO;
			proj.extent = (float)atof(arg);
			if (!(proj.extent >= 0.f) || isinf(proj.extent)) {
				LOG("--projection ortho needs a width of at least 0 (0: the image plane's own), not '%s'.", arg);
				return 1;
			}
		} else {
			LOG("--projection needs panorama, fisheye DEGREES or ortho EXTENT.");
			return 1;
		}
		if (ngpu > 1) {
			LOG("--projection renders on one GPU, not on %d.", ngpu);
			return 1;
		}
		if (multipass || denoise_variance) {
			LOG("--projection does not combine with --passes, --aa, --lens, --filter, --adaptive, --target-error or "
			    "--denoise-variance: move rtx_projection's offsets and average the renders through the library instead.");
			return 1;
		}
		if (upsample) {
			LOG("--projection does not combine with --upsample: the upsampler's scaled frame is a pinhole's.");
			return 1;
		}
	}

	LOG("Loading scene.");
	const char *scale = NULL;
	if ((idx = argv_find(argc, argv, "-r", 1)))
		scale = argv[idx + 1];
	rtx_scene *scene = NULL;
	if (rtx_scene_load(argv[1], scale, NULL, &scene)) {
		LOG("%s", rtx_scene_last_error());
		return 1;
	}
	const rtx_scene_desc *desc = rtx_scene_desc_of(scene);
	LOG("Loaded %u materials, %u objects (%u emitters).", desc->num_materials, desc->num_objects, desc->num_emitters);

	LOG("Initializing image.");
	uint32_t w = (uint32_t)abs(atoi(argv[3])), h = (uint32_t)abs(atoi(argv[4]));
	rtx_frame fr;
	if (rtx_frame_setup(&desc->camera, w, h, &fr)) {
		LOG("Invalid resolution.");
		return 1;
	}
	size_t px = (size_t)w * h;
	float *rgb = calloc(px * 3, sizeof(float)), *z = calloc(px, sizeof(float));
	float *var = denoise_variance ? calloc(px * 3, sizeof(float)) : NULL; /* the variance of the passes' mean */
	int *devs = calloc((size_t)ngpu, sizeof(int));
	if (!rgb || !z || !devs || (denoise_variance && !var)) {
		LOG("Unable to allocate the framebuffer.");
		return 1;
	}
	for (int g = 0; g < ngpu; g++)
		devs[g] = dev0 + g;
	LOG("Commencing raytracing on %d GPU(s).", ngpu);
	rtx_stats st = { 0 };
	uint64_t closest, shadow;
	double kms;
	if (multipass) {
		/* one context on the first device: every pass through the render's own path, the mean saved */
		if (lens)
			pp.focus = (float)(focus_distance / (double)desc->camera.focal_length);
		rtx_ctx *ctx = NULL;
		rtx_pass_stats ps;
		rtx_adaptive_stats as;
		if (rtx_open(dev0, &ctx) || rtx_upload_scene(ctx, desc) ||
		    (adaptive ? rtx_render_adaptive(ctx, &fr, &p, &pp, rgb, z, var, NULL) || rtx_get_adaptive_stats(ctx, &as)
		     : filtered ? rtx_render_passes_filtered(ctx, &fr, &p, &pp, &fp, rgb, z, var) || rtx_get_pass_stats(ctx, &ps)
				: rtx_render_passes(ctx, &fr, &p, &pp, rgb, z, var) || rtx_get_pass_stats(ctx, &ps))) {
			LOG("%s", rtx_last_error());
			rtx_close(ctx);
			return 1;
		}
		rtx_close(ctx);
		if (adaptive) {
			const double all = (double)as.passes_run * (double)as.tiles;
			LOG("Adaptive passes: %u of %u run, %llu of %.0f tile passes (%.1f %%), error %.6g, render %.3f ms, fold %.3f ms.",
			    as.passes_run, pp.passes, (unsigned long long)as.tile_passes, all, all > 0 ? 100.0 * as.tile_passes / all : 0.0,
			    as.error, as.render_ms, as.fold_ms);
			closest = as.closest_rays;
			shadow = as.shadow_rays;
			kms = as.render_ms;
		} else {
			LOG("Passes: %u of %u run, error %.6g, render %.3f ms, accumulation %.3f ms.", ps.passes_run, pp.passes, ps.error,
			    ps.render_ms, ps.accum_ms);
			closest = ps.closest_rays;
			shadow = ps.shadow_rays;
			kms = ps.render_ms;
		}
	} else if (upsample) {
		rtx_ctx *ctx = NULL;
		rtx_upsample_stats us;
		if (rtx_open(dev0, &ctx) || rtx_upload_scene(ctx, desc) || rtx_render_upsampled(ctx, &fr, &p, &up, rgb, z) ||
		    rtx_get_upsample_stats(ctx, &us)) {
			LOG("%s", rtx_last_error());
			rtx_close(ctx);
			return 1;
		}
		rtx_close(ctx);
		LOG("Upsampled %ux%u by %u: %u of %u tiles refined (%.1f %%), %llu pixels below confidence %g; low render %.3f ms, "
		    "features %.3f ms, upsample %.3f ms, refinement %.3f ms.",
		    us.low_width, us.low_height, up.scale, us.refined_tiles, us.tiles, us.tiles ? 100.0 * us.refined_tiles / us.tiles : 0.0,
		    (unsigned long long)us.low_conf_pixels, (double)up.refine_threshold, us.low_ms, us.features_ms, us.upsample_ms,
		    us.refine_ms);
		closest = us.closest_rays;
		shadow = us.shadow_rays;
		kms = us.low_ms + us.features_ms + us.upsample_ms + us.refine_ms;
	} else if (projection) {
		rtx_ctx *ctx = NULL;
		if (rtx_open(dev0, &ctx) || rtx_upload_scene(ctx, desc) || rtx_render_projection(ctx, &fr, &proj, &p, rgb, z) ||
		    rtx_get_stats(ctx, &st)) {
			LOG("%s", rtx_last_error());
			rtx_close(ctx);
			return 1;
		}
		rtx_close(ctx);
		closest = st.closest_rays;
		shadow = st.shadow_rays;
		kms = st.kernel_ms;
	} else {
		rtx_group *grp = NULL;
		if (rtx_group_open(ngpu, devs, &grp) || rtx_group_upload_scene(grp, desc) ||
		    rtx_group_render(grp, &fr, &p, rgb, z) || rtx_group_get_stats(grp, &st)) {
			LOG("%s", rtx_last_error());
			rtx_group_close(grp);
			return 1;
		}
		rtx_group_close(grp);
		closest = st.closest_rays;
		shadow = st.shadow_rays;
		kms = st.kernel_ms;
	}
	if (ngpu > 1)
		LOG("Gathered %d shards in %.3f ms.", ngpu, st.gather_ms);
	LOG("Rays: %llu closest + %llu shadow in %.3f ms device time (%.1f Mrays/s).", (unsigned long long)closest,
	    (unsigned long long)shadow, kms, kms > 0 ? (closest + shadow) / (kms * 1e3) : 0.0);

	if (denoise_variance) {
		/* as --denoise below, with the variance the passes gave: both are filtered, the mean is saved */
		LOG("Denoising with the variance.");
		rtx_ctx *ctx = NULL;
		rtx_feature *feat = malloc(px * sizeof(rtx_feature));
		rtx_denoise_variance_params dp;
		rtx_denoise_stats ds;
		rtx_denoise_variance_params_default(&dp);
		if (!feat) {
			LOG("Unable to allocate the feature buffer.");
			return 1;
		}
		if (rtx_open(dev0, &ctx) || rtx_upload_scene(ctx, desc) || rtx_frame_features(ctx, &fr, p.u32conv, feat) ||
		    rtx_denoise_variance(ctx, w, h, &dp, feat, rgb, var) || rtx_get_denoise_stats(ctx, &ds)) {
			LOG("%s", rtx_last_error());
			rtx_close(ctx);
			return 1;
		}
		rtx_close(ctx);
		free(feat);
		LOG("Denoised %llu hit pixels: features %.3f ms, %u variance-guided filter levels %.3f ms.",
		    (unsigned long long)ds.hit_pixels, ds.features_ms, ds.iterations, ds.filter_ms);
	}

	if (argv_find(argc, argv, "--denoise", 0)) {
		/* a context of its own on the first device: the frame's feature records, then the filter with its
		 * defaults over the gathered rgb (z is left as rendered) */
		LOG("Denoising.");
		rtx_ctx *ctx = NULL;
		rtx_feature *feat = malloc(px * sizeof(rtx_feature));
		rtx_denoise_params dp;
		rtx_denoise_stats ds;
		rtx_denoise_params_default(&dp);
		/* a projection's records: rtx_ray_features of its rays, formed on the host by their definition */
		rtx_ray *rays = projection ? malloc(px * sizeof(rtx_ray)) : NULL;
		if (!feat || (projection && !rays)) {
			LOG("Unable to allocate the feature buffer.");
			return 1;
		}
		for (size_t i = 0; rays && i < px; i++)
			if (rtx_projection_ray(&fr, &proj, (uint32_t)(i % w), (uint32_t)(i / w), &rays[i])) {
				LOG("%s", rtx_last_error());
				return 1;
			}
		if (rtx_open(dev0, &ctx) || rtx_upload_scene(ctx, desc) ||
		    (projection ? rtx_ray_features(ctx, w, h, rays, p.u32conv, feat) : rtx_frame_features(ctx, &fr, p.u32conv, feat)) ||
		    rtx_denoise(ctx, w, h, &dp, feat, rgb) || rtx_get_denoise_stats(ctx, &ds)) {
			LOG("%s", rtx_last_error());
			rtx_close(ctx);
			return 1;
		}
		rtx_close(ctx);
		free(feat);
		free(rays);
		LOG("Denoised %llu hit pixels: features %.3f ms, %u filter levels %.3f ms.", (unsigned long long)ds.hit_pixels,
		    ds.features_ms, ds.iterations, ds.filter_ms);
	}

	LOG("Saving image.");
	const char *out = argv[2];
	if (!strstr(out, ".tif"))
		LOG("Expected output file [%s] with extension .tif.", out);
	if (rtx_tiff_write(out, w, h, rgb, z, argv_find(argc, argv, "-f", 0) != 0)) {
		LOG("Failed to open output file [%s].", out);
		return 1;
	}
	LOG("Terminating.");
	rtx_scene_free(scene);
	return 0;
}
