// sg_msg_plan.cpp -- the launch geometry of one long message (host only, no
// HIP): how the MAC stream -- ad || le64(|ad|) || ct || le64(|ct|)
// (chacha20_poly1305.rs:19-42), or with SG_MSG_RFC8439 the padded stream of
// RFC 8439 section 2.8 (msg_stream_len) -- is cut into tiles and the tiles
// into workgroups.  The kernels of sg_msg.hip take the struct computed here as a
// kernel argument, so the plan the tests check is the plan that runs.  The
// batch plan (sg_msg_batch_plan_for, for sg_msg_batch.hip) applies the same
// geometry per message and cuts the messages' tiles into the groups' segments.
#include "sg_msg_plan.h"

#include <atomic>

#include "sg_env.h"

namespace sg {
namespace {
std::atomic<int>& groups_setting() {
    static std::atomic<int> g{env_int("SG_MSG_GROUPS", 0, (int)kMsgMaxGroups, 0)};
    return g;
}
}  // namespace

int msg_groups() { return groups_setting().load(); }

}  // namespace sg

extern "C" {

int sg_msg_plan_for_flags(uint64_t n, uint64_t adlen, uint32_t flags, uint32_t groups, sg_msg_plan* out) {
    if (!out || n > SG_MSG_MAX_LEN || adlen > SG_MSG_MAX_LEN || (flags & ~sg::kMsgKnownFlags)) return SG_E_ARG;
    // both lengths < 2^32: the stream length stays far below 2^64
    const uint64_t L = sg::msg_stream_len(n, adlen, flags);
    const uint64_t B = (L + 15u) / 16u;  // >= 1
    const uint64_t K = sg::kMsgTileBlocks;
    const uint64_t T = (B + K - 1u) / K;  // >= 1
    uint64_t G = groups ? groups : sg::kMsgMaxGroups;
    if (G > sg::kMsgMaxGroups) G = sg::kMsgMaxGroups;
    if (G > T) G = T;
    const uint64_t per = (T + G - 1u) / G;
    G = (T + per - 1u) / per;  // no empty group; the last takes the rest
    out->mac_blocks = B;
    out->tiles = T;
    out->zero_blocks = T * K - B;  // < K
    out->tile_blocks = (uint32_t)K;
    out->tile_bytes = (uint32_t)(16u * K);
    out->groups = (uint32_t)G;
    out->tiles_per_group = (uint32_t)per;  // T < 2^30
    return SG_OK;
}

int sg_msg_plan_for(uint64_t n, uint64_t adlen, uint32_t groups, sg_msg_plan* out) {
    return sg_msg_plan_for_flags(n, adlen, 0u, groups, out);
}

// The batch plan: every message keeps its own tile geometry, the tiles of all
// messages form one sequence, the groups take equal contiguous runs of it and
// a run is cut where a message ends.  One pass over the messages with the
// group boundary moving along: O(count + groups).
int sg_msg_batch_plan_for_flags(const uint64_t* n, const uint64_t* adlen, uint32_t count, uint32_t flags,
                                uint32_t groups, sg_msg_batch_plan* plan, sg_msg_plan* msgs, sg_msg_seg* segs,
                                uint32_t seg_cap, sg_msg_span* group_segs, sg_msg_span* msg_segs) {
    if (!plan || count > SG_MSG_BATCH_MAX_COUNT || (count && (!n || !adlen)) || (flags & ~sg::kMsgKnownFlags))
        return SG_E_ARG;
    const uint64_t K = sg::kMsgTileBlocks;
    uint64_t TT = 0;
    for (uint32_t m = 0; m < count; ++m) {
        sg_msg_plan one;
        if (sg_msg_plan_for_flags(n[m], adlen[m], flags, groups, &one) != SG_OK) return SG_E_ARG;
        if (msgs) msgs[m] = one;
        TT += one.tiles;  // < 2^20 * 2^19
    }
    uint64_t G = groups ? groups : sg::kMsgMaxGroups;
    if (G > sg::kMsgMaxGroups) G = sg::kMsgMaxGroups;
    if (G > TT) G = TT;
    const uint64_t per = G ? (TT + G - 1u) / G : 0u;
    G = per ? (TT + per - 1u) / per : 0u;  // no empty group; the last takes the rest
    plan->tiles = TT;
    plan->tiles_per_group = per;
    plan->groups = (uint32_t)G;
    plan->tile_blocks = (uint32_t)K;
    plan->tile_bytes = (uint32_t)(16u * K);

    uint32_t S = 0;       // segments so far
    uint64_t g = 0;       // the group that owns global tile `base + a`
    uint64_t base = 0;    // global index of the message's tile 0
    for (uint32_t m = 0; m < count; ++m) {
        const uint64_t B = (sg::msg_stream_len(n[m], adlen[m], flags) + 15u) / 16u;
        const uint64_t T = (B + K - 1u) / K;
        const uint32_t first = S;
        for (uint64_t a = 0; a < T;) {
            const uint64_t group_end = (g + 1u) * per - base;  // in the message's tile units, > a
            const uint64_t b = group_end < T ? group_end : T;
            if (segs) {
                if (S >= seg_cap) return SG_E_ARG;
                segs[S] = sg_msg_seg{m, (uint32_t)a, (uint32_t)b, (uint32_t)g};
            }
            if (group_segs) {
                if (S == 0u || (base + a) % per == 0u) group_segs[g] = sg_msg_span{S, 0u};
                ++group_segs[g].count;
            }
            ++S;
            if (b == group_end) ++g;  // the run of group g ends here, with or without the message
            a = b;
        }
        if (msg_segs) msg_segs[m] = sg_msg_span{first, S - first};
        base += T;
    }
    plan->segments = S;
    return SG_OK;
}

int sg_msg_batch_plan_for(const uint64_t* n, const uint64_t* adlen, uint32_t count, uint32_t groups,
                          sg_msg_batch_plan* plan, sg_msg_plan* msgs, sg_msg_seg* segs, uint32_t seg_cap,
                          sg_msg_span* group_segs, sg_msg_span* msg_segs) {
    return sg_msg_batch_plan_for_flags(n, adlen, count, 0u, groups, plan, msgs, segs, seg_cap, group_segs, msg_segs);
}

int sg_set_msg_groups(int n) {
    if (n < 0) return sg::msg_groups();
    if (n > (int)sg::kMsgMaxGroups) n = (int)sg::kMsgMaxGroups;
    return sg::groups_setting().exchange(n);
}

}  // extern "C"
