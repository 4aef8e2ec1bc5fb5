/*
 * The device group's own state, shared by rtx_group.cpp (open, upload, rtx_group_render, close) and
 * rtx_group_passes.cpp (multi-pass and adaptive rendering on a group).  Not installed; nothing outside
 * librtx includes it.
 */
#ifndef RTX_GROUP_INTERNAL_H
#define RTX_GROUP_INTERNAL_H

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <vector>

#include "rtx_internal.h"

#define NCCL_TRY(expr)                                                                                  \
	do {                                                                                            \
		ncclResult_t r_ = (expr);                                                               \
		if (r_ != ncclSuccess)                                                                  \
			return fail(RTX_ERR_HIP, "%s failed: %s", #expr, ncclGetErrorString(r_));       \
	} while (0)

/* a grow-once device buffer of the group: the group frees it with its device current (rtx_group_close) */
struct GroupBuf {
	void *p = nullptr;
	size_t bytes = 0;
};

struct rtx_group {
	int n = 0;
	bool loopback = false;         /* rtx_group_open_loopback: every context on one device */
	bool rccl_self = false;        /* rtx_group_open_rccl_self: shard 0 sent to itself over RCCL */
	std::vector<uint32_t> peer;    /* peer access between device r and device 0 enabled */
	std::vector<rtx_ctx *> ctx;
	std::vector<ncclComm_t> comm;  /* n > 1 or rccl_self: one per device, rank r = ctx[r] */
	std::vector<float4 *> d_buf;   /* r > 0 (rccl_self: r = 0): shard r's packed records on device r */
	std::vector<float4 *> d_recv;  /* the same shards' records received on device 0 */
	std::vector<size_t> buf_cap;   /* capacity of d_buf[r] in records */
	std::vector<size_t> recv_cap;  /* capacity of d_recv[r] in records */
	rtx_stats stats{};
	rtx_point_stats pstats{};
	rtx_dark_stats dstats{};
	rtx_order_stats ostats{};
	rtx_premask_stats mstats{};
	rtx_clearlane_stats cstats{};
	/* rtx_group_render_passes / rtx_group_render_adaptive (rtx_group_passes.cpp), sized at the first call: the
	 * travelling members' packed tile statistics and pass records on their own devices, and where device 0
	 * receives them; the list as a group of one receives it from itself (rccl_self) */
	std::vector<GroupBuf> ps_stat, ps_rec;           /* on device r */
	std::vector<GroupBuf> ps_stat_recv, ps_rec_recv; /* on device 0 */
	GroupBuf ps_list_recv;                           /* on device 0 */
	rtx_pass_stats pass_stats{};
	rtx_adaptive_stats ad_stats{};
	rtx_group_exchange_stats ex_stats{};
};

#endif
