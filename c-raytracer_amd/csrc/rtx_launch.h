/*
 * The host entry points of the library's device files, declared once: every extern "C" launcher,
 * code-object loader and size / occupancy query a .hip file defines.  The host callers include it,
 * and so does each .hip file for its own definitions, so a definition that drifts from its
 * declaration does not compile (C linkage alone would link it).
 *
 * The functions take the D* records (rtx_device.h) by pointer only, so they are forward-declared
 * here and a device file includes nothing it did not include before.
 */
#ifndef RTX_LAUNCH_H
#define RTX_LAUNCH_H

#include <hip/hip_runtime.h>

#include "rtx.h"

struct DNode;
struct DPrim;
struct DW8;
struct DW8S;
struct DMaterial;
struct DScene;
struct DFrame;
struct DParams;
struct DTask;

#define RTX_HIDDEN __attribute__((visibility("hidden")))

extern "C" {

/* rtx_build.hip: the BVH2 builders on the device */
hipError_t rtx_lbvh_build(uint32_t n, const float *d_lo, const float *d_hi, const DPrim *d_prims_in, const float blo[3],
			  const float bhi[3], uint32_t max_leaf, DNode **recs_out, uint32_t *nnodes_out, uint32_t *root_out,
			  uint32_t *depth_out, hipStream_t st);
hipError_t rtx_ploc_build(uint32_t n, const float *d_lo, const float *d_hi, const DPrim *d_prims_in, const float blo[3],
			  const float bhi[3], uint32_t max_leaf, DNode **recs_out, uint32_t *nnodes_out, uint32_t *root_out,
			  uint32_t *depth_out, uint32_t *rounds_out, hipStream_t st);
hipError_t rtx_sah_build(uint32_t n, const float *d_lo, const float *d_hi, const DPrim *d_prims_in, uint32_t max_leaf,
			 uint32_t bins, uint32_t max_depth, float c_trav, float c_isect, DNode **recs_out, uint32_t *nnodes_out,
			 uint32_t *root_out, uint32_t *depth_out, uint32_t *levels_out, hipStream_t st);
hipError_t rtx_launch_find_prims(const DPrim *prims, uint32_t n, const uint32_t *objs, uint32_t nobj, uint32_t *out,
				 hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_build(void);

/* rtx_wide8_dev.hip: the 8-wide tree collapsed on the device */
hipError_t rtx_launch_w8_scalar(uint32_t n, const DW8 *w8, const uint32_t *leafmap, DW8S *w8s, hipStream_t st);
hipError_t rtx_w8_collapse_device(const DNode *recs, uint32_t nnodes, uint32_t nb, const uint32_t *skip_obj,
				  uint32_t num_objects, DW8 **w8_out, DW8S **w8s_out, uint32_t **leafmap_out,
				  uint32_t *entries_out, uint32_t *scalar_entries_out, uint32_t *depth_out, uint32_t *wide_out,
				  uint32_t *top_out, float qo[3], float qs[3], hipStream_t st);
RTX_HIDDEN hipError_t rtx_load_wide8_dev(void);

/* rtx_trace.hip (defined in its part rtx_trace_launch.h): k_trace, k_accum, k_rays, the frame's rays.  tile_list: the device list of a tile-list render
 * (rtx_render_tiles*), indexed by the chunk positions tile_begin..; null: the shard of P.  pack: the packed GI
 * walk's region (RTX_OPT_TRACE_PACK), waves * rtx_trace_pack_bytes(pack_seg) bytes, for a scene that walks the
 * 8-wide tree (S->trace_w8); null: every GI batch walks on its own.  prim_rays: the F->width * F->height rtx_ray
 * records of a ray batch (rtx_render_rays*), 16-byte aligned, in place of the frame's own primary rays (no
 * tile_list then); null: the pinhole frame F.  Every instance is capped to the occupancy rtx_trace_occupancy
 * reports for the default one (__launch_bounds__), so one query sizes every launch. */
size_t rtx_trace_pack_bytes(uint32_t pack_seg);
size_t rtx_trace_lds_bytes(uint32_t stack_size);
hipError_t rtx_trace_occupancy(uint32_t stack_size, int *blocks_per_cu);
hipError_t rtx_launch_trace(const DScene *S, const DFrame *F, const DParams *P, float *rgb, float *z, DTask *tasks,
			    uint32_t task_cap, float4 *staging, uint32_t staging_cap, float4 *sp_out, uint32_t sp_cap,
			    uint2 *tile_rec, uint32_t tile_begin, uint32_t tile_end, unsigned long long *ctr, uint32_t waves,
			    int count, const uint32_t *tile_list, void *pack, uint32_t pack_seg, const float4 *prim_rays,
			    hipStream_t stream);
hipError_t rtx_launch_accum(const DFrame *F, const DParams *P, const uint2 *tile_rec, const float4 *contrib,
			    uint32_t tile_begin, uint32_t ntiles, float *rgb, const uint32_t *tile_list, hipStream_t stream);
size_t rtx_rays_lds_bytes(uint32_t stack_size);
hipError_t rtx_rays_occupancy(uint32_t stack_size, int *blocks_per_cu);
hipError_t rtx_launch_rays(const DScene *S, const float4 *rays, float4 *hits, const uint32_t *perm, uint32_t n,
			   uint32_t queues, uint32_t grab, unsigned long long *ctr, uint32_t waves, int count, int any,
			   hipStream_t stream);
hipError_t rtx_launch_frame_rays(const DFrame *F, float4 *rays, hipStream_t stream);
hipError_t rtx_launch_kat(int kind, uint32_t n, const float *in, float *out, int u32mode, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_trace(void);

/* rtx_shadow.hip: k_shadow, k_point_masks, k_shadow_rays, the 8-wide tree's leaf fill */
hipError_t rtx_launch_w8_fill(const DPrim *prims, const DMaterial *mats, const uint32_t *leafmap, uint32_t n, DW8 *out,
			      hipStream_t stream);
hipError_t rtx_launch_kat_shadow(int kind, uint32_t n, const float *in, float *out, hipStream_t stream);
hipError_t rtx_shadow_grid_lanes(uint32_t cus, uint32_t *lanes);
hipError_t rtx_launch_shadow(const DScene *S, const DParams *P, const float4 *sp, const uint32_t *perm, uint32_t n_sp,
			     uint32_t per_wave, uint32_t slot_b, float4 *contrib, unsigned long long *ctr, int count,
			     uint32_t cus, hipStream_t stream, uint32_t *pmask, int *premasked, uint32_t *clbuf, int *clearlane);
size_t rtx_clearlane_words(uint32_t n_sp);
hipError_t rtx_launch_shadow_rays(const DScene *S, const float4 *rays, float4 *res, uint32_t n, unsigned long long *ctr,
				  int slots, int count, uint32_t cus, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_shadow(void);

/* rtx_sort.hip: the shade points' and the query rays' Morton sorts */
hipError_t rtx_spsort_temp_bytes(uint32_t n, size_t *bytes);
hipError_t rtx_launch_spsort(const float4 *sp, uint32_t n, const float lo[3], const float hi[3], uint32_t *keys0,
			     uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, void *temp, size_t temp_bytes,
			     const uint32_t **perm, hipStream_t stream);
hipError_t rtx_raysort_temp_bytes(uint32_t n, size_t *bytes);
hipError_t rtx_launch_raysort(const float4 *rays, uint32_t n, const float lo[3], const float hi[3], uint32_t *keys0,
			      uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, void *temp, size_t temp_bytes,
			      const uint32_t **perm, hipStream_t stream);
/* ... and the closest-point queries' (RTX_CLOSEST_REORDER): points: n rtx_point_query records */
hipError_t rtx_pointsort_temp_bytes(uint32_t n, size_t *bytes);
hipError_t rtx_launch_pointsort(const float4 *points, uint32_t n, const float lo[3], const float hi[3], uint32_t *keys0,
				uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, void *temp, size_t temp_bytes,
				const uint32_t **perm, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_sort(void);

/* rtx_nearest.hip: k_nearest (rtx_closest_points*) and the distance functions' known answers.  wmag: the largest
 * coordinate magnitude of the bounded objects' world box; the lane stack is k_rays' (S->ostk sized for THIS grid) */
size_t rtx_nearest_lds_bytes(uint32_t stack_size);
hipError_t rtx_nearest_occupancy(uint32_t stack_size, int *blocks_per_cu);
hipError_t rtx_launch_nearest(const DScene *S, const float4 *queries, float4 *results, const uint32_t *perm, uint32_t n,
			      uint32_t queues, uint32_t grab, float wmag, int bounded_only, unsigned long long *ctr,
			      uint32_t waves, int count, hipStream_t stream);
hipError_t rtx_launch_nearest_kat(const rtx_object *objs, const uint32_t *index, const float *pts, uint64_t n, float4 *out,
				  hipStream_t stream);
hipError_t rtx_launch_nearest_grid(const rtx_object *objs, uint32_t n_obj, const float *pts, uint32_t n_pts, float *dist,
				   hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_nearest(void);

/* rtx_post.hip */
hipError_t rtx_launch_post(uint32_t w, uint32_t h, const rtx_post *pp, float *rgb, const float *z, int *rad, float4 *pv,
			   unsigned *scratch, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_post(void);

/* rtx_gather.hip: a device group's tile records */
hipError_t rtx_launch_tile_pack(const float *rgb, const float *z, uint32_t w, uint32_t h, uint32_t off, uint32_t stride,
				float4 *out, hipStream_t stream);
hipError_t rtx_launch_tile_unpack(const float4 *in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride, float *rgb,
				  float *z, hipStream_t stream);
/* ... and a group's multi-pass renders: tile statistics, a list's shard, pass records */
RTX_HIDDEN hipError_t rtx_launch_stat_pack(const double *vs, const uint32_t *count, uint32_t total, uint32_t off, uint32_t stride,
					   uint32_t ntiles, void *out, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_stat_scatter(const void *in, uint32_t total, uint32_t off, uint32_t stride, uint32_t ntiles,
					      double *vs, uint32_t *count, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_list_shard(const uint32_t *in, uint32_t n_in, uint32_t total, uint32_t off, uint32_t stride,
					    uint32_t *out, uint32_t *n_out, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_pass_pack(const float *rgb, const float *z, const float *var, uint32_t w, uint32_t h,
					   uint32_t off, uint32_t stride, float4 *out, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_pass_unpack(const float4 *in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride, float *rgb,
					     float *z, float *var, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_gather(void);

/* rtx_denoise.hip */
RTX_HIDDEN hipError_t rtx_launch_dn_features(uint64_t n, const float4 *rays, const float4 *hits, const DMaterial *mats,
					     int u32conv, float4 *out, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_denoise(uint32_t w, uint32_t h, const rtx_denoise_params *dp, const float4 *feat,
					 float *rgb, float4 *work, unsigned long long *hit_count, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_denoise(void);

/* rtx_denoise_variance.hip */
RTX_HIDDEN hipError_t rtx_launch_denoise_variance(uint32_t w, uint32_t h, const rtx_denoise_variance_params *dp,
						  const float4 *feat, float *rgb, float *variance, float4 *work,
						  unsigned long long *hit_count, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_denoise_variance(void);

/* rtx_passes.hip: the passes of rtx_render_passes* folded into a mean and its variance */
RTX_HIDDEN uint32_t rtx_pass_blocks(uint64_t n);
RTX_HIDDEN hipError_t rtx_launch_pass_fold(uint64_t n, uint32_t k, int out, const float *rgb, double *state, float *out_rgb,
					   float *out_var, double *partials, double *sums, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_pass_error(uint32_t blocks, const double *partials, double *sums, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_passes(void);

/* rtx_filter.hip: the passes of rtx_render_passes_filtered* folded through a 5x5 reconstruction filter */
struct rtx_filter_weights {
	double wx[RTX_FILTER_TAPS], wy[RTX_FILTER_TAPS];
};
RTX_HIDDEN uint64_t rtx_filter_blocks(uint32_t w, uint32_t h);
RTX_HIDDEN hipError_t rtx_launch_pass_filter_fold(uint32_t w, uint32_t h, uint32_t k, int out, const rtx_filter_weights *fw,
						  const float *rgb, double *state, float *out_rgb, float *out_var, double *partials,
						  double *sums, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_filter(void);

/* rtx_adaptive.hip: a device tile list's check, and the per-tile state of rtx_render_adaptive* */
RTX_HIDDEN hipError_t rtx_launch_tiles_check(const uint32_t *tiles, uint32_t n, uint32_t total, uint32_t *flag, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_tile_all(uint32_t total, uint32_t *list, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_tile_fold(uint32_t w, uint32_t h, uint32_t k, const uint32_t *list, uint32_t n_list,
					   const float *rgb, double *state, uint32_t *count, double *vs, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_tile_select(uint32_t total, uint32_t k, uint32_t min_passes, float target,
					     const uint32_t *count, const double *vs, uint32_t *next, uint32_t *n_next,
					     double *sums, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_tile_out(uint32_t w, uint32_t h, const double *state, const uint32_t *count, float *rgb,
					  float *var, uint32_t *tile_passes, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_adaptive(void);

/* rtx_upsample.hip: the feature-guided upsampler, the z copy and the refinement list of rtx_render_upsampled* */
RTX_HIDDEN hipError_t rtx_launch_upsample(uint32_t w, uint32_t h, const rtx_upsample_params *up, const float *low_rgb,
					  const float4 *low_feat, const float4 *feat, float *rgb, float *conf, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_upsample_z(uint64_t n, const float4 *feat, float *z, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_launch_upsample_tiles(uint32_t w, uint32_t h, float threshold, const float *conf, uint32_t *count,
						uint32_t *list, unsigned long long *out, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_upsample(void);

/* rtx_temporal.hip: the temporal accumulation of rtx_temporal* and rtx_render_temporal*.  The previous frame's
 * projection, formed on the host in double: q = m (P - o) row-major, u = q0 / q2 - 1, v = q1 / q2 */
struct rtx_temporal_proj {
	double m[9], o[3];
};
/* its statistics: RTX_TEMPORAL_CTR_SLOTS 64-bit sums, one per 128-byte line (live pixels | with-history pixels << 32) */
#define RTX_TEMPORAL_CTR_SLOTS 256u
#define RTX_TEMPORAL_CTR_STRIDE 16u
#define RTX_TEMPORAL_CTR_WORDS (RTX_TEMPORAL_CTR_SLOTS * RTX_TEMPORAL_CTR_STRIDE)
RTX_HIDDEN hipError_t rtx_launch_temporal(uint32_t w, uint32_t h, const rtx_temporal_params *tp, int same_frame,
					  const rtx_temporal_proj *pr, const float *rgb, const float *var, const float4 *feat,
					  const float *hist_rgb, const float *hist_var, const float *hist_len, const float4 *hist_feat,
					  float *out_rgb, float *out_var, float *out_len, float *out_conf, unsigned long long *ctr,
					  hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_temporal(void);

/* rtx_projection.hip: the rays of a panoramic, fisheye or orthographic camera (rtx_projection.h) */
struct rtx_proj_basis;
RTX_HIDDEN hipError_t rtx_launch_projection_rays(const rtx_proj_basis *B, float4 *rays, hipStream_t stream);
RTX_HIDDEN hipError_t rtx_load_projection(void);

}

#endif
