/*
 * Multi-pass and adaptive rendering on a device group (include/rtx.h rtx_group_render_passes,
 * rtx_group_render_adaptive).  Member r owns the tiles t = r (mod n).  Its per-tile state lives in
 * its own context's adaptive buffers (rtx_internal.h d_ad_*), addressed by the GLOBAL tile index as in a single
 * context; the fold, the selection and the output are rtx_adaptive.hip's kernels, so the result is
 * rtx_render_adaptive's to the bit.  d_ad_tiles holds, per member:
 *
 *     n_t per tile | the member's own list | the frame's list as it arrives | its length (member 0) | own length
 *
 * A pass: the members render and fold on one host thread each; then ONE host thread moves the travelling members'
 * {V_t, S_t, n_t} records to member 0 (move_to_first), scatters them, selects on member 0, moves the next list to
 * every travelling member (move_from_first) and has each member keep its own tiles of it.  Every member but the
 * first travels; in a group that sends to itself (rccl_self) the first does too, into buffers filled with 0xFF.
 * The transports are those of rtx_group_render: device-to-device copies (loopback) or grouped ncclSend / ncclRecv
 * of whole bytes.  Zero-length moves are skipped on both ends alike.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <math.h>
#include <string.h>

#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "rtx_group_internal.h"
#include "rtx_internal.h"
#include "rtx_tiles.h"

#define RTX_STAT_BYTES 24u /* {V_t, S_t, n_t}: three 8-byte words */
#define RTX_PASS_REC_BYTES 32u

typedef std::chrono::steady_clock Clock;
static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

static int grow_buf(GroupBuf &b, size_t need)
{
	if (need <= b.bytes)
		return RTX_OK;
	dfree(b.p);
	b.bytes = 0;
	HIP_TRY(hipMalloc(&b.p, need));
	b.bytes = need;
	return RTX_OK;
}

/* one call's view of the group */
struct Run {
	rtx_group *g;
	int n, r0;       /* members, the first that travels */
	uint32_t w, h, T;
	size_t px;
	std::vector<uint32_t> tiles; /* tiles of member r's shard */
	std::vector<uint32_t> mine;  /* entries of member r's own list */
	rtx_group_exchange_stats ex{};

	bool travels(int r) const { return r >= r0; }
	uint32_t *count(int r) const { return g->ctx[r]->d_ad_tiles; }
	uint32_t *own(int r) const { return count(r) + T; }
	uint32_t *in(int r) const { return count(r) + 2 * (size_t)T; }
	uint32_t *d_n_in(int r) const { return count(r) + 3 * (size_t)T; }
	uint32_t *d_n_own(int r) const { return count(r) + 3 * (size_t)T + 1; }
	double *vs(int r) const { return g->ctx[r]->d_ad_vs; }
	double *d_sums(int r) const { return vs(r) + 2 * (size_t)T; }
};

/* fn(r) for every member, each on its own host thread (as rtx_group_render's shards); the first failure is reported */
template <class F> static int on_members(const Run &R, F fn)
{
	std::vector<int> rcs(R.n, RTX_OK);
	std::vector<std::string> errs(R.n);
	auto body = [&](int r) {
		if (hipSetDevice(R.g->ctx[r]->device) != hipSuccess) {
			rcs[r] = RTX_ERR_HIP;
			errs[r] = "hipSetDevice failed";
			return;
		}
		rcs[r] = fn(r);
		if (rcs[r])
			errs[r] = rtx_last_error();
	};
	if (R.n == 1) {
		body(0);
	} else {
		std::vector<std::thread> th;
		for (int r = 0; r < R.n; r++)
			th.emplace_back(body, r);
		for (auto &t : th)
			t.join();
	}
	for (int r = 0; r < R.n; r++)
		if (rcs[r])
			return fail(rcs[r], "device %d: %s", R.g->ctx[r]->device, errs[r].c_str());
	return RTX_OK;
}

/* arguments, state, buffers: everything before the first launch */
static int begin(Run &R, rtx_group *g, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, bool adaptive)
{
	if (!g || !fr || !p || !pp)
		return fail(RTX_ERR_ARG, "null argument");
	for (rtx_ctx *c : g->ctx)
		if (!c->have_scene)
			return fail(RTX_ERR_STATE, "multi-pass render before rtx_group_upload_scene");
	int rc = rtx_passes_args_check(fr, p, pp, adaptive);
	if (rc)
		return rc;
	if (rtx_tiles_total(fr->width, fr->height) > (1ull << 25)) /* a shard's records are counted in 32 bits */
		return fail(RTX_ERR_ARG, "frame %ux%u has more than 2^25 tiles", fr->width, fr->height);
	R.g = g;
	R.n = g->n;
	R.r0 = g->rccl_self ? 0 : 1;
	R.w = fr->width;
	R.h = fr->height;
	R.T = (uint32_t)rtx_tiles_total(R.w, R.h);
	R.px = (size_t)R.w * R.h;
	R.tiles.resize(R.n);
	R.mine.assign(R.n, 0);
	g->ps_stat.resize(R.n);
	g->ps_rec.resize(R.n);
	g->ps_stat_recv.resize(R.n);
	g->ps_rec_recv.resize(R.n);
	const size_t T = R.T;
	for (int r = 0; r < R.n; r++) {
		rtx_ctx *c = g->ctx[r];
		R.tiles[r] = rtx_shard_tiles(R.w, R.h, (uint32_t)r, (uint32_t)R.n);
		HIP_TRY(hipSetDevice(c->device));
		if (rtx_ensure_framebuffer(c, R.px) != hipSuccess || c->d_ad_var.grow(R.px * 3 * sizeof(float)) != hipSuccess ||
		    c->d_pass_rgb.grow(R.px * 3 * sizeof(float)) != hipSuccess || c->d_ad_state.grow(T * 64 * 6 * sizeof(double)) != hipSuccess ||
		    c->d_ad_vs.grow((T * 2 + 2) * sizeof(double)) != hipSuccess || c->d_ad_tiles.grow((T * 3 + 2) * sizeof(uint32_t)) != hipSuccess)
			return fail(RTX_ERR_NOMEM, "device %d: pass state of %u tiles", c->device, R.T);
		if (!R.travels(r))
			continue;
		if ((rc = grow_buf(g->ps_stat[r], (size_t)R.tiles[r] * RTX_STAT_BYTES)) ||
		    (rc = grow_buf(g->ps_rec[r], (size_t)R.tiles[r] * RTX_TILE_PX * RTX_PASS_REC_BYTES)))
			return rc;
		HIP_TRY(hipSetDevice(g->ctx[0]->device));
		if ((rc = grow_buf(g->ps_stat_recv[r], (size_t)R.tiles[r] * RTX_STAT_BYTES)) ||
		    (rc = grow_buf(g->ps_rec_recv[r], (size_t)R.tiles[r] * RTX_TILE_PX * RTX_PASS_REC_BYTES)))
			return rc;
	}
	if (g->rccl_self) {
		HIP_TRY(hipSetDevice(g->ctx[0]->device));
		if ((rc = grow_buf(g->ps_list_recv, T * sizeof(uint32_t))))
			return rc;
	}
	return RTX_OK;
}

/* the travelling members' src[r] (bytes[r] of them, on device r) into dst[r] on device 0; complete for device 0's
 * stream on return, RCCL's in stream order.  One host thread, after the member threads have joined. */
static int move_to_first(Run &R, const std::vector<GroupBuf> &src, const std::vector<GroupBuf> &dst, const std::vector<size_t> &bytes)
{
	rtx_group *g = R.g;
	rtx_ctx *c0 = g->ctx[0];
	if (R.r0 >= R.n) /* one member without RCCL: nothing travels */
		return RTX_OK;
	if (g->loopback) {
		for (int r = R.r0; r < R.n; r++) {
			if (!bytes[r])
				continue;
			HIP_TRY(hipMemcpyAsync(dst[r].p, src[r].p, bytes[r], hipMemcpyDeviceToDevice, g->ctx[r]->stream));
			HIP_TRY(hipStreamSynchronize(g->ctx[r]->stream));
			R.ex.bytes += bytes[r];
		}
		return RTX_OK;
	}
	if (g->rccl_self && bytes[0]) { /* what RCCL does not deliver stays 0xFF and fails the comparison */
		HIP_TRY(hipSetDevice(c0->device));
		HIP_TRY(hipMemsetAsync(dst[0].p, 0xFF, bytes[0], c0->stream));
	}
	NCCL_TRY(ncclGroupStart());
	for (int r = R.r0; r < R.n; r++) {
		if (!bytes[r])
			continue;
		NCCL_TRY(ncclSend(src[r].p, bytes[r], ncclUint8, 0, g->comm[r], g->ctx[r]->stream));
		NCCL_TRY(ncclRecv(dst[r].p, bytes[r], ncclUint8, r, g->comm[0], c0->stream));
		R.ex.bytes += bytes[r];
	}
	NCCL_TRY(ncclGroupEnd());
	return RTX_OK;
}

/* n_list words of device 0's list (complete: the host has read its length) to every travelling member; where member
 * r then reads the list from is *from[r] */
static int move_from_first(Run &R, uint32_t n_list, std::vector<const uint32_t *> &from)
{
	rtx_group *g = R.g;
	rtx_ctx *c0 = g->ctx[0];
	const uint32_t *src = R.in(0);
	const size_t bytes = (size_t)n_list * sizeof(uint32_t);
	for (int r = 0; r < R.n; r++)
		from[r] = r == 0 ? (g->rccl_self ? (const uint32_t *)g->ps_list_recv.p : src) : R.in(r);
	if (!bytes)
		return RTX_OK;
	if (g->loopback) {
		for (int r = R.r0; r < R.n; r++) {
			HIP_TRY(hipMemcpyAsync(R.in(r), src, bytes, hipMemcpyDeviceToDevice, g->ctx[r]->stream));
			R.ex.bytes += bytes;
		}
		return RTX_OK;
	}
	if (R.n == 1 && !g->rccl_self)
		return RTX_OK;
	if (g->rccl_self) {
		HIP_TRY(hipSetDevice(c0->device));
		HIP_TRY(hipMemsetAsync(g->ps_list_recv.p, 0xFF, bytes, c0->stream));
	}
	NCCL_TRY(ncclGroupStart());
	for (int r = R.r0; r < R.n; r++) {
		NCCL_TRY(ncclSend(src, bytes, ncclUint8, r, g->comm[0], c0->stream));
		NCCL_TRY(ncclRecv((void *)from[r], bytes, ncclUint8, 0, g->comm[r], g->ctx[r]->stream));
		R.ex.bytes += bytes;
	}
	NCCL_TRY(ncclGroupEnd());
	return RTX_OK;
}

/* every member keeps its own tiles of the list it reads from from[r] (n_list entries) and the host reads the counts */
static int shard_lists(Run &R, uint32_t n_list, const std::vector<const uint32_t *> &from)
{
	rtx_group *g = R.g;
	for (int r = 0; r < R.n; r++) {
		rtx_ctx *c = g->ctx[r];
		HIP_TRY(hipSetDevice(c->device));
		HIP_TRY(rtx_launch_list_shard(from[r], n_list, R.T, (uint32_t)r, (uint32_t)R.n, R.own(r), R.d_n_own(r), c->stream));
		HIP_TRY(hipMemcpyAsync(&R.mine[r], R.d_n_own(r), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	}
	uint64_t sum = 0;
	for (int r = 0; r < R.n; r++) {
		HIP_TRY(hipSetDevice(g->ctx[r]->device));
		HIP_TRY(hipStreamSynchronize(g->ctx[r]->stream));
		if (R.mine[r] > R.tiles[r])
			return fail(RTX_ERR_HIP, "device %d: %u tiles listed of a shard of %u", g->ctx[r]->device, R.mine[r], R.tiles[r]);
		sum += R.mine[r];
	}
	if (sum != n_list)
		return fail(RTX_ERR_HIP, "the members hold %llu of the %u tiles listed", (unsigned long long)sum, n_list);
	return RTX_OK;
}

/* the first lists: every member's own tiles of k_tile_all's list */
static int first_lists(Run &R)
{
	std::vector<const uint32_t *> from(R.n);
	for (int r = 0; r < R.n; r++) {
		rtx_ctx *c = R.g->ctx[r];
		HIP_TRY(hipSetDevice(c->device));
		HIP_TRY(rtx_launch_tile_all(R.T, R.in(r), c->stream));
		from[r] = R.in(r);
	}
	return shard_lists(R, R.T, from);
}

/* what a member's pass left for the host thread */
struct PassOut {
	double kernel_ms = 0, fold_ms = 0;
	uint64_t closest = 0, shadow = 0;
};

/* member r's pass k on its own thread: the render of its tiles (a list, or its tile shard when list is null) into
 * its pass buffer, the fold of `listed` tiles of its own list, and, when the statistics travel, their records */
static int member_pass(const Run &R, int r, const rtx_frame *fk, const rtx_params *pk, uint32_t k, bool by_list, uint32_t listed,
		       bool pack, PassOut &o)
{
	rtx_ctx *c = R.g->ctx[r];
	o = PassOut{};
	if (listed) { /* a zero-block grid is an error: a member with nothing to render launches nothing */
		rtx_params pr = *pk;
		if (!by_list) {
			pr.tile_offset = (uint32_t)r;
			pr.tile_stride = (uint32_t)R.n;
		}
		int rc = rtx_render_common(c, fk, &pr, c->d_pass_rgb, k == 0 ? c->d_z.p : nullptr, c->stream, by_list ? R.own(r) : nullptr,
					   by_list ? listed : 0);
		if (rc)
			return rc;
		o.kernel_ms = c->stats.kernel_ms;
		o.closest = c->stats.closest_rays;
		o.shadow = c->stats.shadow_rays;
		HIP_TRY(hipEventRecord(c->ev0, c->stream));
		HIP_TRY(rtx_launch_tile_fold(R.w, R.h, k, R.own(r), listed, c->d_pass_rgb, c->d_ad_state, R.count(r), R.vs(r), c->stream));
		HIP_TRY(hipEventRecord(c->ev1, c->stream));
	}
	if (pack && R.travels(r))
		HIP_TRY(rtx_launch_stat_pack(R.vs(r), R.count(r), R.T, (uint32_t)r, (uint32_t)R.n, R.tiles[r], R.g->ps_stat[r].p, c->stream));
	HIP_TRY(hipStreamSynchronize(c->stream));
	if (listed) {
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
		o.fold_ms = ms;
	}
	return RTX_OK;
}

/* after the members' pass k: their statistics to member 0, which selects.  all_tiles: every tile goes on (plain
 * passes read the two sums only).  Returns the next list's length and {V, A}; *select_ms the kernel's time. */
static int exchange_and_select(Run &R, uint32_t k, uint32_t min_passes, float target, uint32_t *n_next, double sums[2], double *select_ms)
{
	rtx_group *g = R.g;
	rtx_ctx *c0 = g->ctx[0];
	const auto t0 = Clock::now();
	std::vector<size_t> bytes(R.n, 0);
	for (int r = R.r0; r < R.n; r++)
		bytes[r] = (size_t)R.tiles[r] * RTX_STAT_BYTES;
	int rc = move_to_first(R, g->ps_stat, g->ps_stat_recv, bytes);
	if (rc)
		return rc;
	HIP_TRY(hipSetDevice(c0->device));
	for (int r = R.r0; r < R.n; r++)
		HIP_TRY(rtx_launch_stat_scatter(g->ps_stat_recv[r].p, R.T, (uint32_t)r, (uint32_t)R.n, R.tiles[r], R.vs(0), R.count(0), c0->stream));
	HIP_TRY(hipStreamSynchronize(c0->stream));
	R.ex.exchange_ms += ms_since(t0);
	HIP_TRY(hipEventRecord(c0->ev0, c0->stream));
	HIP_TRY(rtx_launch_tile_select(R.T, k, min_passes, target, R.count(0), R.vs(0), R.in(0), R.d_n_in(0), R.d_sums(0), c0->stream));
	HIP_TRY(hipEventRecord(c0->ev1, c0->stream));
	HIP_TRY(hipMemcpyAsync(sums, R.d_sums(0), 2 * sizeof(double), hipMemcpyDeviceToHost, c0->stream));
	HIP_TRY(hipMemcpyAsync(n_next, R.d_n_in(0), sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream));
	HIP_TRY(hipStreamSynchronize(c0->stream));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, c0->ev0, c0->ev1));
	*select_ms = ms;
	return RTX_OK;
}

/* after the last pass: every member's mean and variance into its own frame buffers and, where it travels, into pass
 * records; one gather to member 0, which unpacks them; then the caller's copies.  *out_ms member 0's output kernel. */
static int finish(Run &R, float *rgb, float *z, float *variance, uint32_t *tile_passes, double *out_ms)
{
	rtx_group *g = R.g;
	rtx_ctx *c0 = g->ctx[0];
	std::vector<double> oms(R.n, 0.0);
	int rc = on_members(R, [&](int r) -> int {
		rtx_ctx *c = g->ctx[r];
		HIP_TRY(hipEventRecord(c->ev0, c->stream));
		HIP_TRY(rtx_launch_tile_out(R.w, R.h, c->d_ad_state, R.count(r), c->d_rgb, c->d_ad_var, nullptr, c->stream));
		HIP_TRY(hipEventRecord(c->ev1, c->stream));
		if (R.travels(r))
			HIP_TRY(rtx_launch_pass_pack(c->d_rgb, c->d_z, c->d_ad_var, R.w, R.h, (uint32_t)r, (uint32_t)R.n,
						     (float4 *)g->ps_rec[r].p, c->stream));
		HIP_TRY(hipStreamSynchronize(c->stream));
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
		oms[r] = ms;
		return RTX_OK;
	});
	if (rc)
		return rc;
	*out_ms = oms[0];
	const auto t0 = Clock::now();
	if (R.r0 < R.n) {
		std::vector<size_t> bytes(R.n, 0);
		for (int r = R.r0; r < R.n; r++)
			bytes[r] = (size_t)R.tiles[r] * RTX_TILE_PX * RTX_PASS_REC_BYTES;
		if ((rc = move_to_first(R, g->ps_rec, g->ps_rec_recv, bytes)))
			return rc;
		HIP_TRY(hipSetDevice(c0->device));
		for (int r = R.r0; r < R.n; r++)
			HIP_TRY(rtx_launch_pass_unpack((const float4 *)g->ps_rec_recv[r].p, R.w, R.h, (uint32_t)r, (uint32_t)R.n, c0->d_rgb, c0->d_z,
						       c0->d_ad_var, c0->stream));
		for (int r = 1; r < R.n; r++) {
			HIP_TRY(hipSetDevice(g->ctx[r]->device));
			HIP_TRY(hipStreamSynchronize(g->ctx[r]->stream));
		}
		HIP_TRY(hipSetDevice(c0->device));
		HIP_TRY(hipStreamSynchronize(c0->stream));
		R.ex.gather_ms = ms_since(t0);
	}
	HIP_TRY(hipSetDevice(c0->device));
	if (rgb)
		HIP_TRY(hipMemcpy(rgb, c0->d_rgb, R.px * 12, hipMemcpyDeviceToHost));
	if (z)
		HIP_TRY(hipMemcpy(z, c0->d_z, R.px * 4, hipMemcpyDeviceToHost));
	if (variance)
		HIP_TRY(hipMemcpy(variance, c0->d_ad_var, R.px * 12, hipMemcpyDeviceToHost));
	if (tile_passes) /* member 0's n_t array, complete since the last scatter */
		HIP_TRY(hipMemcpy(tile_passes, R.count(0), (size_t)R.T * 4, hipMemcpyDeviceToHost));
	return RTX_OK;
}

/* the members' pass k and what it adds to the totals */
struct PassSum {
	double render_ms = 0, fold_ms = 0;
	uint64_t closest = 0, shadow = 0;
};

static int run_pass(Run &R, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, uint32_t k, bool by_list, bool pack,
		    PassSum &s)
{
	rtx_frame fk;
	int rc = rtx_pass_frame(fr, pp, k, &fk);
	if (rc)
		return rc;
	rtx_params pk = *p;
	pk.seed = p->seed + k;
	std::vector<PassOut> po(R.n);
	rc = on_members(R, [&](int r) { return member_pass(R, r, &fk, &pk, k, by_list, by_list ? R.mine[r] : R.tiles[r], pack, po[r]); });
	if (rc)
		return rc;
	double km = 0, fm = 0;
	for (const PassOut &o : po) {
		km = std::max(km, o.kernel_ms);
		fm = std::max(fm, o.fold_ms);
		s.closest += o.closest;
		s.shadow += o.shadow;
	}
	s.render_ms += km;
	s.fold_ms += fm;
	return RTX_OK;
}

extern "C" int rtx_group_render_adaptive(rtx_group *g, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, float *rgb,
					 float *z, float *variance, uint32_t *tile_passes)
{
	Run R;
	int rc = begin(R, g, fr, p, pp, true);
	if (rc || (rc = first_lists(R)))
		return rc;
	rtx_adaptive_stats as{};
	as.tiles = R.T;
	PassSum s;
	uint32_t active = R.T;
	std::vector<const uint32_t *> from(R.n);
	for (uint32_t k = 0; k < pp->passes && active; k++) {
		if ((rc = run_pass(R, fr, p, pp, k, true, true, s)))
			return rc;
		as.tile_passes += active;
		as.passes_run = k + 1;
		double sums[2] = { 0.0, 0.0 }, select_ms = 0;
		uint32_t n_next = 0;
		if ((rc = exchange_and_select(R, k, pp->min_passes, pp->target_error, &n_next, sums, &select_ms)))
			return rc;
		s.fold_ms += select_ms;
		as.error = sums[1] != 0.0 ? sqrt(sums[0]) / sums[1] : 0.0;
		if (n_next > R.T)
			return fail(RTX_ERR_HIP, "%u tiles selected of %u", n_next, R.T);
		const auto t0 = Clock::now();
		if ((rc = move_from_first(R, n_next, from)) || (rc = shard_lists(R, n_next, from)))
			return rc;
		R.ex.exchange_ms += ms_since(t0);
		if (R.r0 < R.n)
			R.ex.exchanges++;
		active = n_next;
	}
	double out_ms = 0;
	if ((rc = finish(R, rgb, z, variance, tile_passes, &out_ms)))
		return rc;
	as.render_ms = s.render_ms;
	as.fold_ms = s.fold_ms + out_ms;
	as.closest_rays = s.closest;
	as.shadow_rays = s.shadow;
	g->ad_stats = as;
	g->ex_stats = R.ex;
	return RTX_OK;
}

extern "C" int rtx_group_render_passes(rtx_group *g, const rtx_frame *fr, const rtx_params *p, const rtx_pass_params *pp, float *rgb,
				       float *z, float *variance)
{
	Run R;
	int rc = begin(R, g, fr, p, pp, false);
	if (rc || (rc = first_lists(R))) /* a member's own list is its shard, the same for every pass */
		return rc;
	rtx_pass_stats ps{};
	PassSum s;
	const bool stop_rule = pp->target_error > 0.f;
	for (uint32_t k = 0; k < pp->passes; k++) {
		/* the tile statistics leave the members after the last pass and after every pass the stopping rule looks at */
		const bool last = k + 1 == pp->passes;
		const bool look = stop_rule && k + 1 >= pp->min_passes;
		if ((rc = run_pass(R, fr, p, pp, k, false, last || look, s)))
			return rc;
		ps.passes_run = k + 1;
		if (!(last || look))
			continue;
		double sums[2] = { 0.0, 0.0 }, select_ms = 0;
		uint32_t n_next = 0;
		/* V and A in the selection's order; its list (every tile: min_passes is never reached) is not used */
		if ((rc = exchange_and_select(R, k, 0xFFFFFFFFu, 0.f, &n_next, sums, &select_ms)))
			return rc;
		s.fold_ms += select_ms;
		if (R.r0 < R.n)
			R.ex.exchanges++;
		ps.error = sums[1] != 0.0 ? sqrt(sums[0]) / sums[1] : 0.0;
		if (look && ps.error <= (double)pp->target_error)
			break;
	}
	double out_ms = 0;
	if ((rc = finish(R, rgb, z, variance, nullptr, &out_ms)))
		return rc;
	ps.render_ms = s.render_ms;
	ps.accum_ms = s.fold_ms + out_ms;
	ps.closest_rays = s.closest;
	ps.shadow_rays = s.shadow;
	g->pass_stats = ps;
	g->ex_stats = R.ex;
	return RTX_OK;
}

extern "C" int rtx_group_get_pass_stats(const rtx_group *g, rtx_pass_stats *out)
{
	if (!g || !out)
		return fail(RTX_ERR_ARG, "null argument");
	*out = g->pass_stats;
	return RTX_OK;
}

extern "C" int rtx_group_get_adaptive_stats(const rtx_group *g, rtx_adaptive_stats *out)
{
	if (!g || !out)
		return fail(RTX_ERR_ARG, "null argument");
	*out = g->ad_stats;
	return RTX_OK;
}

extern "C" int rtx_group_get_exchange_stats(const rtx_group *g, rtx_group_exchange_stats *out)
{
	if (!g || !out)
		return fail(RTX_ERR_ARG, "null argument");
	*out = g->ex_stats;
	return RTX_OK;
}

/* ---- pass records: host reference and device entry points (rtx_tiles.h) ---- */

extern "C" int rtx_pass_pack_host(const float *rgb, const float *z, const float *var, uint32_t w, uint32_t h, uint32_t off,
				  uint32_t stride, float *out)
{
	if (!rgb || !z || !var || !out || !stride || off >= stride)
		return fail(RTX_ERR_ARG, "bad pass pack arguments");
	const size_t nrec = rtx_tile_pack_count(w, h, off, stride);
	const uint32_t tx = rtx_tiles_x(w);
	for (size_t i = 0; i < nrec; i++) {
		uint32_t x, y;
		rtx_shard_pixel((uint32_t)i, tx, off, stride, &x, &y);
		float *o = out + 8 * i;
		memset(o, 0, 8 * sizeof(float));
		if (x < w && y < h) { /* bytes, not values: a NaN keeps its payload */
			const size_t q = (size_t)y * w + x;
			memcpy(o, rgb + 3 * q, 12);
			memcpy(o + 3, z + q, 4);
			memcpy(o + 4, var + 3 * q, 12);
		}
	}
	return RTX_OK;
}

extern "C" int rtx_pass_unpack_host(const float *in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride, float *rgb, float *z,
				    float *var)
{
	if (!in || !stride || off >= stride)
		return fail(RTX_ERR_ARG, "bad pass unpack arguments");
	const size_t nrec = rtx_tile_pack_count(w, h, off, stride);
	const uint32_t tx = rtx_tiles_x(w);
	for (size_t i = 0; i < nrec; i++) {
		uint32_t x, y;
		rtx_shard_pixel((uint32_t)i, tx, off, stride, &x, &y);
		if (x >= w || y >= h)
			continue;
		const size_t q = (size_t)y * w + x;
		const float *r = in + 8 * i;
		if (rgb)
			memcpy(rgb + 3 * q, r, 12);
		if (z)
			memcpy(z + q, r + 3, 4);
		if (var)
			memcpy(var + 3 * q, r + 4, 12);
	}
	return RTX_OK;
}

extern "C" int rtx_pass_pack_device(rtx_ctx *c, const void *d_rgb, const void *d_z, const void *d_var, uint32_t w, uint32_t h,
				    uint32_t off, uint32_t stride, void *d_out, void *stream)
{
	if (!c || !d_rgb || !d_z || !d_var || !d_out || !stride || off >= stride)
		return fail(RTX_ERR_ARG, "bad pass pack arguments");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	HIP_TRY(rtx_launch_pass_pack((const float *)d_rgb, (const float *)d_z, (const float *)d_var, w, h, off, stride, (float4 *)d_out, s));
	HIP_TRY(hipStreamSynchronize(s));
	return RTX_OK;
}

extern "C" int rtx_pass_unpack_device(rtx_ctx *c, const void *d_in, uint32_t w, uint32_t h, uint32_t off, uint32_t stride, void *d_rgb,
				      void *d_z, void *d_var, void *stream)
{
	if (!c || !d_in || !stride || off >= stride)
		return fail(RTX_ERR_ARG, "bad pass unpack arguments");
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t s = stream ? (hipStream_t)stream : c->stream;
	HIP_TRY(rtx_launch_pass_unpack((const float4 *)d_in, w, h, off, stride, (float *)d_rgb, (float *)d_z, (float *)d_var, s));
	HIP_TRY(hipStreamSynchronize(s));
	return RTX_OK;
}
