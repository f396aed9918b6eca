// sg_msg_plan.h -- geometry of the long-message path (sg_msg.hip), host only
// (no HIP): shared by the plan (sg_msg_plan.cpp), the kernels and the C ABI.
// Not part of the public ABI; the plan struct itself is (suruga_gpu.h).
#pragma once

#include <stdint.h>

#include "../../include/suruga_gpu.h"
#include "sg_layout.h"

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

// Bytes of a message's MAC stream (sg_layout.h), the construction chosen by
// SG_MSG_RFC8439.  Both lengths <= SG_MSG_MAX_LEN: far below 2^64.
inline uint64_t msg_stream_len(uint64_t n, uint64_t adlen, uint32_t flags) {
    return flags & SG_MSG_RFC8439 ? stream_bytes<Construction::kRfc8439>(adlen, n)
                                  : stream_bytes<Construction::kDraft>(adlen, n);
}
// the flags the plan functions and the message calls know
constexpr uint32_t kMsgKnownFlags = SG_MSG_KEEP_FAILED | SG_MSG_RFC8439;

// The argument checks of one message, shared by sg_seal_msg_dev /
// sg_open_msg_dev and every item of sg_seal_msg_batch / sg_open_msg_batch, in
// the order the single call reports them.  No pointer is dereferenced.  (The
// batch checks its key table and status array once, ahead of its items.)
struct MsgArgs {
    const void* key;
    const void* ad;
    uint64_t ad_len;
    const void* in;
    uint64_t in_len;
    const void* out;
    const void* status;  // open only
};
// NULL: the message may run, *n its data bytes -- or, with *shrt set, it is an
// open of fewer than SG_MAC_LEN bytes (chacha20_poly1305.rs:68-70): the caller's
// SG_E_SHORT, not an argument error, and nothing else was looked at.
// Otherwise the message of the SG_E_ARG to report (a format for sg::fail).
// (Inline: the batch runs it once per item inside its timed call, and as a
// call into another file it cost 3 ns per item, 50 us per 16384 messages.)
inline const char* msg_check_args(const MsgArgs& a, bool open, uint64_t* n, bool* shrt) {
    *n = 0;
    *shrt = open && a.in_len < SG_MAC_LEN;
    if (*shrt) return nullptr;
    *n = open ? a.in_len - SG_MAC_LEN : a.in_len;
    if (*n > SG_MSG_MAX_LEN) return "message longer than SG_MSG_MAX_LEN%s";
    if (a.ad_len > SG_MSG_MAX_LEN) return "ad_len exceeds SG_MSG_MAX_LEN%s";
    const uint64_t out_len = open ? *n : *n + SG_MAC_LEN;
    if (!a.key) return "key must be non-NULL%s";
    if ((a.in_len && !a.in) || (out_len && !a.out) || (a.ad_len && !a.ad)) return "in/out/ad must be non-NULL%s";
    if (open && !a.status) return "open requires a status byte%s";
    if (a.in != a.out && a.in_len && out_len) {
        const uintptr_t x = (uintptr_t)a.in, y = (uintptr_t)a.out;
        if (x < y + out_len && y < x + a.in_len) return "out overlaps in (only out == in is allowed)%s";
    }
    return nullptr;
}

// ---- the message batch (sg_msg_batch.hip, sg_msg_batch_capi.cpp)
// One message as the batch kernels read it (wave-uniform loads): the host
// resolves the key index and the nonce words (n13: state word 13, the first
// word of an RFC 8439 nonce; 0 and never read in the draft).  skip: an open of
// fewer than 16 bytes -- no kernel touches its buffers, the finish kernel
// reports SG_E_SHORT.
struct MsgBatchItem {
    const uint8_t* key;
    const uint8_t* ad;
    const uint8_t* in;
    uint8_t* out;
    uint64_t n, adlen;
    uint32_t n14, n15, skip, n13;
};
static_assert(sizeof(MsgBatchItem) == 64, "device layout");

// The batch's workspace, a function of count alone.  The host writes
// [items | plans | msg_segs | segs | group_segs] (sg_msg_batch_plan_for's tables
// as they stand) and uploads them in one copy; the partials (one per segment,
// kMsgPartialWords words) follow and never leave the device.
struct MsgBatchLayout {
    size_t items, plans, msg_segs, segs, group_segs, upload_bytes, partials, total;
    uint32_t seg_cap;
};
inline MsgBatchLayout msg_batch_layout(uint32_t count) {
    auto up = [](size_t x) { return (x + 15u) & ~(size_t)15u; };
    MsgBatchLayout l;
    l.seg_cap = kMsgMaxGroups + count;  // >= groups + count - 1
    l.items = 0;
    l.plans = l.items + sizeof(MsgBatchItem) * (size_t)count;
    l.msg_segs = l.plans + sizeof(sg_msg_plan) * (size_t)count;
    l.segs = up(l.msg_segs + sizeof(sg_msg_span) * (size_t)count);
    l.group_segs = l.segs + sizeof(sg_msg_seg) * (size_t)l.seg_cap;
    l.upload_bytes = up(l.group_segs + sizeof(sg_msg_span) * (size_t)kMsgMaxGroups);
    l.partials = l.upload_bytes;
    l.total = l.partials + 4u * kMsgPartialWords * (size_t)l.seg_cap;
    return l;
}

}  // namespace sg
