// sg_msg_plan.h -- geometry of the long-message path (sg_msg.hip), host only
// (no HIP): shared by the plan (sg_msg_plan.cpp), the kernels and the C ABI.
// Not part of the public ABI; the plan struct itself is (suruga_gpu.h).
#pragma once

#include <stdint.h>

#include "../../include/suruga_gpu.h"

namespace sg {

// One tile is the work of one pass of a 256-thread workgroup: kMsgMacLanes
// lanes run Horner over kMsgLaneBlocks contiguous MAC blocks each.  The tile
// is 16,320 bytes of MAC stream, not 16 KiB: a run of L bytes that starts
// anywhere in a 64-byte ChaCha20 block touches at most ceil((63 + L) / 64)
// blocks, which is <= 256 -- one per lane -- exactly for L <= 16,321.
constexpr uint32_t kMsgThreads = 256;
constexpr uint32_t kMsgLaneBlocks = 4;
constexpr uint32_t kMsgMacLanes = 255;
constexpr uint32_t kMsgTileBlocks = kMsgMacLanes * kMsgLaneBlocks;  // 1020
constexpr uint32_t kMsgTileBytes = 16u * kMsgTileBlocks;            // 16320
static_assert(63u + kMsgTileBytes <= 64u * kMsgThreads, "one ChaCha20 block per lane covers a tile");
// Workgroups: at most kMsgMaxGroups (the workspace holds one partial each);
// the automatic grid is that many or one per tile, four per CU of a 256-CU part.
constexpr uint32_t kMsgMaxGroups = 1024;
constexpr uint32_t kMsgPartialWords = 8;  // 5 radix-2^26 limbs, padded to 32 bytes

int msg_groups();  // sg_set_msg_groups / SG_MSG_GROUPS

}  // namespace sg
