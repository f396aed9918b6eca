// sg_dtls13_host.cpp -- the host-only part of the DTLS 1.3 record batch: the argument
// rules of sg_seal_batch_dtls13 / sg_open_batch_dtls13, sg_dtls13_header_len,
// sg_dtls13_inner_len and sg_dtls13_record_len.  No HIP (tests/cpp/test_dtls13_san.cpp
// builds it with g++ under sanitizers); the launch is sg_dtls13_capi.cpp's and the key
// derivation sg_keysched.cpp's.
#include "sg_dtls13.h"

namespace sg {
namespace dtls13 {

const char* check_args(const sg_dtls13_batch* b, bool open, uint32_t* max_len) {
    if (!b) return "sg_dtls13_batch is NULL%s";
    static_assert(sizeof(sg_dtls13_batch) == 208, "sg_dtls13_batch layout");
    if (b->flags & ~(SG_DTLS13_SEQ16 | SG_DTLS13_LENGTH | SG_DTLS13_EPOCH_ROWS | SG_DTLS13_KEEP_FAILED))
        return "unknown flags in sg_dtls13_batch%s";
    if (!b->keys || !b->ivs || !b->sn_keys) return "keys, ivs or sn_keys is NULL%s";
    if (!b->status || !b->in || !b->out) return "status, in or out is NULL%s";
    if (!open && !b->seq) return "seal needs seq%s";
    if (open && (!b->expected || !b->seq_out || !b->epoch_out || !b->content_len || !b->type_out))
        return "open needs expected, seq_out, epoch_out, content_len and type_out%s";
    if (b->cid_len > SG_DTLS13_MAX_CID_LEN) return "cid_len above SG_DTLS13_MAX_CID_LEN%s";
    if (!open && b->cid_len && !b->cids) return "seal with a cid_len needs cids%s";
    if (((uintptr_t)b->ivs | (uintptr_t)b->key_index | (uintptr_t)b->content_len | (uintptr_t)b->len) & 3u)
        return "ivs, key_index, content_len and len must be 4-byte aligned%s";
    if (((uintptr_t)b->seq | (uintptr_t)b->expected | (uintptr_t)b->seq_out | (uintptr_t)b->in_off | (uintptr_t)b->out_off) & 7u)
        return "seq, expected, seq_out, in_off and out_off must be 8-byte aligned%s";
    if (b->num_conns == 0) return "num_conns is 0%s";
    if (b->pad_to > kMaxPadTo) return "pad_to above 2^14%s";
    const uint32_t bound = b->len ? b->max_len : b->uniform_len;
    if (bound > (open ? SG_DTLS13_MAX_RECORD_LEN : SG_DTLS13_MAX_CONTENT_LEN))
        return "records longer than SG_DTLS13_MAX_RECORD_LEN (seal: content longer than SG_DTLS13_MAX_CONTENT_LEN)%s";
    if (max_len) *max_len = bound;
    return nullptr;
}

}  // namespace dtls13
}  // namespace sg

extern "C" {

uint32_t sg_dtls13_header_len(uint32_t flags, uint32_t cid_len) { return sg::dtls13::header_len(flags, cid_len); }
uint32_t sg_dtls13_inner_len(uint32_t len, uint32_t pad_to) { return sg::dtls13::inner_len(len, pad_to); }
uint32_t sg_dtls13_record_len(uint32_t len, uint32_t pad_to, uint32_t flags, uint32_t cid_len) {
    return sg::dtls13::record_len(len, pad_to, flags, cid_len);
}

}  // extern "C"
