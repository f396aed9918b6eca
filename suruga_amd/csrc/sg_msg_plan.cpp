// sg_msg_plan.cpp -- the launch geometry of one long message (host only, no
// HIP): how the MAC stream ad || le64(|ad|) || ct || le64(|ct|)
// (chacha20_poly1305.rs:19-42) is cut into tiles and the tiles into
// workgroups.  The kernels of sg_msg.hip take the struct computed here as a
// kernel argument, so the plan the tests check is the plan that runs.
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

int sg_msg_plan_for(uint64_t n, uint64_t adlen, uint32_t groups, sg_msg_plan* out) {
    if (!out || n > SG_MSG_MAX_LEN || adlen > SG_MSG_MAX_LEN) return SG_E_ARG;
    // both lengths < 2^32: the stream length stays far below 2^64
    const uint64_t L = adlen + 16u + n;
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

int sg_set_msg_groups(int n) {
    if (n < 0) return sg::msg_groups();
    if (n > (int)sg::kMsgMaxGroups) n = (int)sg::kMsgMaxGroups;
    return sg::groups_setting().exchange(n);
}

}  // extern "C"
