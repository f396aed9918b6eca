/*
 * suruga_gpu.h -- C ABI of the MI355X (gfx950) ChaCha20-Poly1305 record AEAD.
 *
 * This is the drop-in boundary for suruga's cipher plugin interface
 * (klutzy/suruga src/cipher/mod.rs:14-32).  Every entry point below replaces
 * one item of that interface; the reference-side bindings a maintainer would
 * add are shown in INTEGRATION.md.
 *
 *   Aead::key_size / fixed_iv_len / mac_len      mod.rs:15-17
 *       -> sg_key_size / sg_fixed_iv_len / sg_mac_len
 *          (values from chacha20_poly1305.rs:15-17, 102-119)
 *   Aead::new_encryptor / new_decryptor           mod.rs:18-19, chacha20_poly1305.rs:121-134
 *       -> sg_ctx_new (one context per direction, key moved in) / sg_ctx_free
 *   Encryptor::encrypt(nonce, plain, ad) -> Vec   mod.rs:22-24, chacha20_poly1305.rs:48-59
 *       -> sg_seal   (caller-provided out of n + 16 bytes: ct || tag)
 *   Decryptor::decrypt(nonce, encrypted, ad)      mod.rs:28-31, chacha20_poly1305.rs:65-94
 *       -> sg_open   (returns SG_E_BAD_MAC / SG_E_SHORT where the reference
 *                     returns Err(TlsError{kind: BadRecordMac, ..}))
 *   Decryptor::mac_len                            mod.rs:31, chacha20_poly1305.rs:96-99
 *       -> sg_mac_len
 *   TlsWriter::write_data chunk loop / TlsReader::read_record (tls.rs:99-147,217-281)
 *       -> sg_seal_batch / sg_open_batch: many records per call, nonce and the
 *          13-byte additional data built on the device from the record-layer
 *          rules (tls.rs:103-112, 250-265) in SG_BATCH_TLS mode.
 *
 * Construction: draft-agl-tls-chacha20poly1305-04 as implemented by suruga
 * (64-bit nonce, 32-bit block counter in state word 12 only, Poly1305 key =
 * keystream block 0, MAC over ad || le64(|ad|) || ct || le64(|ct|) with no
 * padding).  NOT RFC 7539 / RFC 8439: this holds for sg_seal / sg_open,
 * sg_seal_batch / sg_open_batch and sg_write_records / sg_read_records, which
 * speak only the draft.  The suites deployed peers negotiate have calls of
 * their own beside each of the last two: the record batch as
 * sg_*_batch_rfc8439 (RFC 7905) and sg_*_batch_tls13 (RFC 8446), the record
 * layer over host memory as sg_write_records_rfc7905 / sg_read_records_rfc7905
 * and sg_write_records_tls13 / sg_read_records_tls13, on a context that has
 * its write IV (sg_ctx_set_iv).
 *
 * The message calls (sg_*_msg*, further below) speak the draft by default and,
 * with SG_MSG_RFC8439 or through sg_seal_msg_rfc8439 / sg_open_msg_rfc8439,
 * RFC 8439 (= RFC 7539): 96-bit nonce in state words 13-15, MAC over
 * ad || zeros to 16 || ct || zeros to 16 || le64(|ad|) || le64(|ct|) -- what
 * TLS 1.2 0xCCA8, TLS 1.3, QUIC, WireGuard, libsodium's _ietf form and
 * OpenSSL's EVP_chacha20_poly1305 compute.
 *
 * Plain C types only: no HIP or torch types cross this boundary.  Device
 * pointers are passed as plain pointers; a HIP stream as void*.
 */
#ifndef SURUGA_GPU_H
#define SURUGA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------ */
#define SG_OK          0
#define SG_E_BAD_MAC   1   /* tag mismatch: TlsErrorKind::BadRecordMac "wrong mac"
                              (chacha20_poly1305.rs:89-90)                        */
#define SG_E_SHORT     2   /* input shorter than the tag: BadRecordMac "message too
                              short" (chacha20_poly1305.rs:68-70)                 */
#define SG_E_ARG      -1   /* bad argument (lengths, NULL pointers, limits); the
                              reference panics here (chacha20.rs:26-27)           */
#define SG_E_HIP      -2   /* HIP runtime error                                  */
#define SG_E_NODEV    -3   /* no usable gfx950 device                            */

/* ---- limits ------------------------------------------------------------ */
#define SG_KEY_LEN         32u
#define SG_NONCE_LEN        8u
#define SG_MAC_LEN         16u
#define SG_MAX_AD_LEN     255u
/* The size-class kernels (every batch that is not uniform 16 KiB records or
 * a mixed TLS batch of 64-byte multiples) stage a record's MAC stream in LDS,
 * which bounds a record at 32 KiB; the wave-per-record and packed kernels
 * stream their records.  TLS records are at most 2^14 (+2048 expansion) bytes
 * (tls.rs:32-35). */
#define SG_MAX_RECORD_LEN 32768u

/* ---- Aead constants (chacha20_poly1305.rs:15-17, 104-119) --------------- */
size_t sg_key_size(void);     /* 32 */
size_t sg_fixed_iv_len(void); /* 0  */
size_t sg_mac_len(void);      /* 16 */
int    sg_abi_version(void);  /* SG_ABI_VERSION */

/* ---- per-direction context (Aead::new_encryptor / new_decryptor) -------- */
typedef struct sg_ctx sg_ctx;

/* Copies the 32-byte key to device `device` (HIP ordinal).  Returns NULL on
 * failure (sg_last_error() says why). */
sg_ctx* sg_ctx_new(const uint8_t key[32], int device);
void    sg_ctx_free(sg_ctx* ctx);

/* Encryptor::encrypt.  Host pointers.  out receives n + 16 bytes (ct || tag).
 * nonce is 8 bytes (TLS: be64(seq), tls.rs:103).  Returns SG_OK or < 0. */
int sg_seal(sg_ctx* ctx, const uint8_t* nonce, size_t nonce_len,
            const uint8_t* pt, size_t n, const uint8_t* ad, size_t adlen, uint8_t* out);

/* Decryptor::decrypt.  Host pointers.  in = ct || tag (in_len bytes); out
 * receives in_len - 16 bytes of plaintext on SG_OK.  On SG_E_BAD_MAC the
 * plaintext is withheld (out is zero-filled), as the reference returns no
 * plaintext with its Err (chacha20_poly1305.rs:89-93); the decryption itself
 * always runs (:80-82).  Returns SG_OK, SG_E_BAD_MAC, SG_E_SHORT or < 0. */
int sg_open(sg_ctx* ctx, const uint8_t* nonce, size_t nonce_len,
            const uint8_t* in, size_t in_len, const uint8_t* ad, size_t adlen, uint8_t* out);

/* ---- batch interface (record-layer batching point, tls.rs:140) --------- */
#define SG_BATCH_TLS  0x1u  /* nonce = be64(seq_i); ad = be64(seq_i) || content_type ||
                               ver_major || ver_minor || be16(n_i)  (tls.rs:103-112,
                               250-265); `nonces`/`ads` are ignored               */
#define SG_BATCH_KEEP_FAILED 0x2u  /* open: leave the (unauthenticated) plaintext of
                                      records whose status is SG_E_BAD_MAC in `out`.
                                      By default it is zero-filled after the batch, as
                                      the reference hands out no plaintext with its
                                      Err (chacha20_poly1305.rs:89-93; the decryption
                                      itself always runs, :80-82).                   */

typedef struct sg_batch {
    uint32_t count;            /* number of records                                 */
    uint32_t flags;            /* SG_BATCH_*                                        */

    /* keys: key table [num_keys][32] in device memory; record i uses
     * key_index[i] (device array) or key 0 when key_index is NULL.  Indices
     * must be < num_keys; the kernels clamp a larger one to num_keys - 1, so
     * it never reads outside the table (that record's output is meaningless). */
    const uint8_t*  keys;
    uint32_t        num_keys;
    const uint32_t* key_index;

    /* TLS mode: seq_i = seq ? seq[i] : seq0 + i   (device array)            */
    const uint64_t* seq;
    uint64_t        seq0;
    uint8_t         content_type;   /* 23 = application_data (tls.rs:26)     */
    uint8_t         ver_major;      /* 3                                     */
    uint8_t         ver_minor;      /* 3                                     */
    uint8_t         _pad0;

    /* explicit mode: nonce_i = nonces + 8*i; ad_i = ads + ad_stride*i, ad_len
     * bytes (device memory)                                                   */
    const uint8_t*  nonces;
    const uint8_t*  ads;
    uint32_t        ad_len;
    uint32_t        ad_stride;

    /* record layout (device memory).  Record i reads in + in_off_i and writes
     * out + out_off_i, where off_i = off ? off[i] : stride * i.
     *   seal: input = plaintext of len_i bytes, output = ct || tag (len_i + 16)
     *   open: input = ct || tag of len_i bytes (len_i >= 16 else status
     *         SG_E_SHORT), output = plaintext (len_i - 16)
     * len_i = len ? len[i] : uniform_len.  max_len >= every len_i is required
     * when len != NULL (it sizes the LDS staging of one record); a longer
     * record is skipped and the call returns SG_E_ARG once every other record
     * is done (on a NULL stream: after the device work has finished; under
     * stream capture it is skipped silently).                                  */
    const uint8_t*  in;
    const uint64_t* in_off;
    uint64_t        in_stride;
    uint8_t*        out;
    const uint64_t* out_off;
    uint64_t        out_stride;
    const uint32_t* len;
    uint32_t        uniform_len;
    uint32_t        max_len;

    /* open: per-record status, device: SG_OK / SG_E_BAD_MAC / SG_E_SHORT, or
     * SG_STATUS_SKIPPED for a record longer than max_len (not processed, its
     * output left untouched).  The output of an SG_E_BAD_MAC record is zeroed
     * unless flags has SG_BATCH_KEEP_FAILED: it is never authenticated
     * plaintext.                                                             */
    uint8_t*        status;

    /* HIP stream (hipStream_t).  Non-NULL: the call is asynchronous on that
     * stream, except that a mixed-size batch (len != NULL, records in more
     * than one size class) waits once for its classification so that every
     * class runs on an exact grid; under stream capture it does not wait
     * (persistent class grids), so the whole call is graph-capturable with a
     * caller workspace.  A mixed TLS batch also runs its keying and two of its
     * record launches on library-owned side streams, which wait for this
     * stream's earlier work and are joined back into it before the call
     * returns.  NULL: the null (default) stream -- ordered after the
     * caller's earlier work on it -- and the call returns when the batch is
     * done.  No library lock is held while a call waits, so calls on
     * different streams (e.g. a writer and a reader thread, client.rs:19-24)
     * run concurrently on the device. */
    void*           stream;

    /* scratch of >= sg_workspace_size(count) bytes of 16-byte aligned device
     * memory, or NULL to use a library-owned cache: each call takes a buffer
     * no other call is enqueuing on and orders its reuse on the device with an
     * event, so asynchronous calls on different streams never share scratch.
     * A call under stream capture must pass a workspace. */
    void*           workspace;
    size_t          workspace_size;
} sg_batch;

#define SG_STATUS_SKIPPED 3  /* open status of a record with len_i > max_len;
                                sg_*_batch then returns SG_E_ARG            */

size_t sg_workspace_size(uint32_t count);

/* Batch seal / open on device-resident records.  Records are independent
 * (one wave each for 4-16 KiB records, 64-byte blocks of many small records
 * packed into one wave, or 2-256 lanes per record in the size classes).
 * Returns SG_OK or < 0 for argument/HIP errors; per-record MAC results of
 * open land in b->status. */
int sg_seal_batch(const sg_batch* b);
int sg_open_batch(const sg_batch* b);

/* The record batch in RFC 8439 (section 2.8; the construction SG_MSG_RFC8439
 * names further below): the suites deployed peers negotiate -- TLS 1.2
 * 0xCCA8 / 0xCCA9 (RFC 7905), TLS 1.3 and QUIC records -- where the two calls
 * above speak draft-agl-04 (0xCC13).  `b` is the unchanged sg_batch and means
 * what it means above (flags, statuses, SG_E_SHORT, SG_STATUS_SKIPPED, the
 * scrub, workspace, stream and capture rules, SG_MAX_RECORD_LEN,
 * SG_MAX_AD_LEN), except for the nonce:
 *   explicit mode: nonce_i = nonces + 12*i, 12 bytes (SG_RFC8439_NONCE_LEN);
 *     state words 13-15 are its three little-endian words.  ads / ad_len /
 *     ad_stride as above.  A TLS 1.3 or QUIC caller passes its 5-byte header
 *     as AD and its own nonces.
 *   SG_BATCH_TLS (RFC 7905 section 2): nonce_i = ivs[key_i] XOR
 *     (00 00 00 00 || be64(seq_i)), key_i the record's (clamped) key index;
 *     the AD is the 13 bytes be64(seq) || type || major || minor || be16(n).
 * SG_E_ARG, before any GPU work: x NULL, x->flags non-zero, ivs not 4-byte
 * aligned, ivs NULL in TLS mode, unknown b->flags, and whatever the draft
 * calls reject.  The batch takes the routes of the draft calls, every kernel
 * in its RFC 8439 form: uniform 16 KiB batches the wave-per-record kernel,
 * the eligible records of a mixed TLS batch the packed kernel (64 B-4 KiB) and
 * the 4-16 KiB buckets, everything else the size classes. */
typedef struct sg_batch_rfc8439 {
    const uint8_t* ivs;   /* device, [num_keys][12], 4-byte aligned: TLS mode only */
    uint32_t       flags; /* 0; anything else SG_E_ARG */
    uint32_t       _pad;
} sg_batch_rfc8439;
int sg_seal_batch_rfc8439(const sg_batch* b, const sg_batch_rfc8439* x);
int sg_open_batch_rfc8439(const sg_batch* b, const sg_batch_rfc8439* x);

/* The record batch as TLS 1.3 protects records (RFC 8446 section 5.2 - 5.4) with
 * TLS_CHACHA20_POLY1305_SHA256: RFC 8439 over TLSInnerPlaintext = content ||
 * type || zeros.  Nonce, additional data and the inner type byte are built on
 * the device, and open strips type and padding; through the RFC calls above a
 * TLS 1.3 caller has to do all of that itself, in explicit mode.
 * `b` is the unchanged sg_batch with these rules:
 *   flags        SG_BATCH_TLS must be set; SG_BATCH_KEEP_FAILED is allowed.
 *   nonces, ads, ver_major, ver_minor   ignored.
 *   nonce_i      ivs[key_i] XOR (00 00 00 00 || be64(seq_i))      (section 5.3)
 *   AD_i         17 03 03 be16(L_i), L_i the fragment length: the inner length
 *                + 16 on seal, len_i on open                       (section 5.2)
 * Seal: len_i is the content length, 0..2^14.  b->content_type is the inner
 *   type of every record of the call and must be non-zero (a zero would read
 *   as padding).  Record i reads len_i bytes and writes len_i + 17:
 *   ct(content || type) || tag.  This call adds no padding and gives every
 *   record the one type; sg_seal_batch_tls13_ex below does both.
 * Open: len_i is the fragment length, at most 2^14 + 256; below 16 the status
 *   is SG_E_SHORT.  The len_i - 16 inner bytes go to `out` as in the RFC call.
 *   Then, for every record whose status is SG_OK, the last non-zero inner byte
 *   goes to inner_type[i] and the number of bytes before it to content_len[i];
 *   a record with no non-zero byte (or no byte) gets SG_STATUS_NO_TYPE.  Every
 *   record with another status gets type 0 and length 0.  The scrub,
 *   SG_STATUS_SKIPPED, the workspace, stream and capture rules are those of
 *   sg_open_batch_rfc8439.  content_len > 2^14 is the caller's to map to
 *   record_overflow.
 * SG_E_ARG before any GPU work: x NULL, x->flags non-zero, SG_BATCH_TLS not
 * set, other flags, ivs NULL or not 4-byte aligned, a zero content_type on
 * seal, max_len / uniform_len above 2^14 (seal) or 2^14 + 256 (open), open
 * without inner_type or content_len or with content_len not 4-byte aligned,
 * and whatever the RFC calls reject.
 * Routes: a uniform batch of full records (uniform_len 2^14 on seal, 2^14 + 17
 * on open; bases and strides 16-byte aligned, no len / offset arrays) runs on
 * the wave-per-record kernel, whose keying pre-pass takes the type byte and
 * its MAC block.  In every other batch with a len array, a record whose inner
 * length (seal: as sealed; open: len_i - 16) is a multiple of 64 in 64..4096
 * and whose input and output addresses are 16-byte aligned runs on the packed
 * kernel in its TLS 1.3 form -- on seal that needs padding (below), on open a
 * peer that pads so -- under the conditions of the RFC call (not under capture,
 * per-record arrays 4-byte aligned, sg_set_packed); everything else, padded
 * records above 4 KiB included, on the size classes.  Under
 * sg_set_tls13_buckets(1) (off by default) a record whose inner length is a
 * multiple of 64 in 4160..2^14, addresses 16-byte aligned, runs on the
 * wave-per-record buckets J = 2..4 instead, under the conditions of the RFC
 * call's buckets (sg_set_lockstep, not under capture, per-record arrays 4-byte
 * aligned); a full record in such a batch (inner length 2^14 + 1) stays on the
 * size classes.  sg_last_batch_routes reports where the records of a mixed call
 * went. */
typedef struct sg_batch_tls13 {
    const uint8_t* ivs;          /* device [num_keys][12], 4-byte aligned, required        */
    uint8_t*       inner_type;   /* open: device, count bytes, required; seal: not read    */
    uint32_t*      content_len;  /* open: device, count words, 4-byte aligned, required    */
    uint32_t       flags;        /* 0; anything else SG_E_ARG                              */
    uint32_t       _pad;
} sg_batch_tls13;                /* 32 bytes */
int sg_seal_batch_tls13(const sg_batch* b, const sg_batch_tls13* x);
int sg_open_batch_tls13(const sg_batch* b, const sg_batch_tls13* x);
#define SG_STATUS_NO_TYPE 5      /* open: tag good, inner plaintext all zero (or empty)    */
/* Which route a TLS 1.3 batch would take (host only, no GPU call): 1 = the
 * uniform wave-per-record kernel, 0 = not that route (the size classes and,
 * for the eligible records of a mixed batch, the packed kernel: those are
 * chosen per record on the device, see sg_last_batch_routes), SG_E_ARG for a
 * batch the calls above reject on its own fields; honours sg_set_lockstep. */
int sg_batch_tls13_route(const sg_batch* b, int open);

/* TLS 1.3 seal with record padding (RFC 8446 section 5.4) and a type per record.
 * `b` and `x` are those of sg_seal_batch_tls13.  Record i reads len_i content
 * bytes -- no byte of `in` at or beyond len_i, except that a record on the packed
 * kernel or on a wave-per-record bucket (sg_set_tls13_buckets) may load the
 * aligned 16-byte unit holding its last content byte whole --
 * and writes exactly inner_i + 16 bytes:
 *   ct(content_i || type_i || zeros) || tag,  inner_i = sg_tls13_inner_len(len_i, pad_to)
 * under the AD 17 03 03 be16(inner_i + 16).  Room in `out` (strides, offsets) for
 * the padded fragments is the caller's to provide; max_len / uniform_len still
 * bound the content lengths, and the library derives the largest inner length.
 * type_i is inner_types[i], or b->content_type for every record when inner_types
 * is NULL.  With {NULL, 0 or 1, 0} the call is sg_seal_batch_tls13 byte for byte,
 * routes included.  A seal with inner_types never takes the uniform wave-per-record
 * route (its pre-pass appends the call's one type); at 2^14 content bytes padding
 * changes nothing.  Padding to a multiple of 64 makes every record of up to 4095
 * content bytes eligible for the packed kernel (above).
 * SG_E_ARG before any GPU work: o NULL, o->flags non-zero, pad_to above 2^14, and
 * everything sg_seal_batch_tls13 rejects -- a zero b->content_type only when
 * inner_types is NULL. */
#define SG_TLS13_MAX_INNER (16384u + 1u)
/* inner plaintext length of a record of `len` (<= 2^14) content bytes under pad_to:
 * pad_to <= 1: len + 1;  else min(roundup(len + 1, pad_to), 2^14 + 1).  Host only. */
uint32_t sg_tls13_inner_len(uint32_t len, uint32_t pad_to);

typedef struct sg_tls13_seal_opts {
    const uint8_t* inner_types; /* device, count bytes, or NULL: b->content_type for every record.
                                   Entries must be non-zero; not checked (device memory) */
    uint32_t       pad_to;      /* 0 or 1: no padding; else 2..2^14, any value (no power-of-two rule) */
    uint32_t       flags;       /* 0; anything else SG_E_ARG */
} sg_tls13_seal_opts;           /* 16 bytes */
int sg_seal_batch_tls13_ex(const sg_batch* b, const sg_batch_tls13* x, const sg_tls13_seal_opts* o);

/* ---- QUIC packet protection batch (RFC 9001 section 5.3 - 5.4) ----------------
 * AEAD_CHACHA20_POLY1305 packet protection and ChaCha20 header protection of many
 * packets in one launch (sg_quic.hip).  A packet differs from a record: its
 * additional data is its own header, in front of the payload and of its own length;
 * the nonce is iv XOR the packet number, which on receive has to be recovered from 1
 * to 4 truncated bytes (RFC 9000 appendix A.3); and the first byte and the packet
 * number bytes are masked with a ChaCha20 block under a third key (section 5.4.4).
 *
 * Packet i lies at in + in_off_i (off_i = off ? off[i] : stride * i) and has len_i =
 * len ? len[i] : uniform_len bytes; pn_off_i = pn_off ? pn_off[i] : uniform_pn_off is
 * the offset of its packet number field, 1..SG_QUIC_MAX_PN_OFF.  Parsing a datagram
 * (coalesced packets, the long header's variable-length fields) is the caller's.
 * Any alignment of `in`, `out` and the offsets; `in` and `out` of a call must not
 * overlap (not checked; the result is undefined where they do).
 *
 * Rows.  k = min(key_index ? key_index[i] : 0, rows - 1).  Without
 * SG_QUIC_KEY_PHASE rows = num_keys and key, IV and header protection key are row k
 * of their tables.  With it rows = num_keys / 2: hp_keys has one row per connection
 * (the HP key does not change at a key update, RFC 9001 section 6), row k, and key
 * and IV are row 2 k + phase, phase = bit 2 (0x04) of the unprotected first byte of
 * a short-header packet (bit 7 clear) and 0 for a long-header packet.
 *
 * Seal.  The input is header || payload, len_i bytes.  pn_len = (first byte & 3) + 1,
 * hdr_len = pn_off_i + pn_len; the packet number field is written by the call, the low
 * pn_len bytes of pn[i], big-endian, whatever the input holds there.  AD = that header,
 * nonce = iv XOR (00 00 00 00 || be64(pn[i])).  The output is len_i + 16 bytes:
 * protected header || ciphertext || tag.  Header protection: sample = the 16 output
 * bytes at pn_off_i + 4; mask = the first 5 bytes of the ChaCha20 block under the HP
 * key with counter le32(sample[0..4)) and nonce sample[4..16); first byte ^= mask[0] &
 * 0x1f (short header) or & 0x0f (long header), packet number bytes ^= mask[1..].
 * Status SG_OK; SG_E_SHORT, nothing written, where len_i < hdr_len or pn_len + payload
 * length < 4 (no full sample: the sender has to pad, section 5.4.2).  max_len is at
 * most SG_QUIC_MAX_PACKET_LEN - 16.
 *
 * Open.  The input is a protected packet of len_i bytes; SG_E_SHORT, nothing written,
 * where len_i < pn_off_i + 20.  The mask comes off the first byte (bit 7, not masked,
 * tells the form), pn_len is read, the packet number bytes are unmasked and the full
 * number is decoded against pn[i] as expected_pn (largest received + 1).  `out`
 * receives len_i - 16 bytes, unprotected header || plaintext, pn_out[i] the number, and
 * status[i] SG_OK or SG_E_BAD_MAC.  The decryption always runs; on SG_E_BAD_MAC all
 * len_i - 16 output bytes are zero and pn_out[i] is 0, unless SG_QUIC_KEEP_FAILED is
 * set: nothing derived from an unauthenticated packet leaves the call.
 *
 * Both.  A packet with len_i > max_len (len != NULL; with len == NULL the bound is
 * uniform_len itself) gets SG_STATUS_SKIPPED and is untouched; the call still returns
 * SG_OK and reads nothing back.  A per-packet pn_off outside 1..251 gives SG_E_SHORT.
 * One launch, no workspace, no host read-back: the call is capturable.
 * count == 0 returns SG_OK and launches nothing.
 * SG_E_ARG before any GPU work: NULL b, unknown flags, NULL keys / ivs / hp_keys /
 * status / in / out / pn, pn_out NULL on open, ivs or a per-packet array misaligned
 * (4 bytes; 8 for pn, pn_out, in_off, out_off), uniform_pn_off (pn_off == NULL) outside
 * 1..251, the length bound above SG_QUIC_MAX_PACKET_LEN (seal: - 16), num_keys zero, or
 * odd under SG_QUIC_KEY_PHASE. */
#define SG_QUIC_MAX_PACKET_LEN 16384u  /* protected packet, tag included */
#define SG_QUIC_MAX_PN_OFF       251u  /* so that the header (AD) is <= 255 = SG_MAX_AD_LEN */
#define SG_QUIC_KEY_PHASE        0x1u
#define SG_QUIC_KEEP_FAILED      0x2u

typedef struct sg_quic_batch {
    uint32_t        count, flags;
    const uint8_t*  keys;       /* device [num_keys][32]                                       */
    const uint8_t*  ivs;        /* device [num_keys][12], 4-byte aligned                       */
    const uint8_t*  hp_keys;    /* device [rows][32] (above)                                   */
    const uint32_t* key_index;  /* device, or NULL: 0                                          */
    const uint64_t* pn;         /* device. seal: the packet number; open: the expected number  */
    uint64_t*       pn_out;     /* open: device, the decoded packet number; seal: not read     */
    const uint32_t* pn_off;     /* device, or NULL: uniform_pn_off                             */
    uint32_t        num_keys;
    uint32_t        uniform_pn_off;
    const uint8_t*  in;
    const uint64_t* in_off;
    uint64_t        in_stride;
    uint8_t*        out;
    const uint64_t* out_off;
    uint64_t        out_stride;
    const uint32_t* len;
    uint32_t        uniform_len;
    uint32_t        max_len;
    uint8_t*        status;     /* device, count bytes, required for seal and open             */
    void*           stream;     /* as sg_batch.stream: non-NULL asynchronous, NULL waits       */
} sg_quic_batch;                /* 152 bytes */
int sg_seal_batch_quic(const sg_quic_batch* b);
int sg_open_batch_quic(const sg_quic_batch* b);

/* RFC 9000 appendix A.3 on the host (no GPU), what the open kernel runs per packet:
 * the full packet number of `truncated` (pn_len bytes, 1..4) given expected_pn =
 * largest received + 1.  pn_len outside 1..4 is taken into that range and truncated is
 * cut to 8 * pn_len bits. */
uint64_t sg_quic_decode_pn(uint64_t expected_pn, uint32_t truncated, uint32_t pn_len);

/* ---- WireGuard transport data batch (whitepaper section 5.4.6) ----------------
 * Many transport data messages sealed or opened in one launch (sg_wg.hip).  The message:
 *
 *   le32(4)                       type 4, three reserved zero bytes
 *   le32(receiver)                the peer's index for this session
 *   le64(counter)
 *   AEAD(key, nonce = 00 00 00 00 || le64(counter), plaintext = inner || zeros, AD = empty)   -> P bytes || 16-byte tag
 *
 * A message is 32 + P bytes; a keepalive has P = 0.  The AEAD is RFC 8439: ChaCha20
 * blocks 1 onward, the Poly1305 key from block 0, the MAC over ct || pad16 || le64(0) ||
 * le64(P).  A generic AEAD call cannot give the two things fused here: the zero padding
 * of the inner packet on seal, and the inner packet's length from its IP header on open.
 *
 * Packet i lies at in + in_off_i (off_i = off ? off[i] : stride * i) and has len_i =
 * len ? len[i] : uniform_len bytes, as in sg_quic_batch; any alignment of `in`, `out`
 * and the offsets.  k = min(key_index ? key_index[i] : 0, num_keys - 1) names the row of
 * `keys` and, on seal, of `receiver`.
 *
 * Seal.  The input is the inner packet, len_i bytes (0 allowed), contents not inspected.
 * P_i = sg_wg_padded_len(len_i, pad_cap): len_i rounded up to 16 and, where pad_cap != 0,
 * at most max(len_i, pad_cap) -- the Linux implementation's min(MTU, ALIGN(len, 16)) for
 * len <= MTU; a pad_cap that is no multiple of 16 yields ragged messages, which open
 * accepts.  The output is 32 + P_i bytes: header (receiver[k], counter[i]), ciphertext,
 * tag.  Plaintext bytes len_i .. P_i are zero and are never read from the input: no
 * input byte at or beyond len_i is read.  Status SG_OK, or SG_STATUS_SKIPPED and nothing
 * written where len_i > max_len.  max_len is at most SG_WG_MAX_MESSAGE_LEN - 32.
 *
 * Open.  The input is a message of len_i bytes.  In this order: len_i > max_len is
 * SG_STATUS_SKIPPED, len_i < 32 is SG_E_SHORT, a type word other than 04 00 00 00 is
 * SG_STATUS_BAD_HEADER; nothing is written for any of them (counter_out and inner_len
 * included).  Otherwise the counter is read from bytes 8..16 and n = len_i - 32 bytes are
 * decrypted into `out`.  Bad tag: SG_E_BAD_MAC, all n output bytes zero, counter_out[i]
 * 0 and inner_len[i] 0; under SG_WG_KEEP_FAILED the decryption and the wire counter are
 * left instead and inner_len[i] stays 0: nothing derived from an unauthenticated message
 * leaves the call by default.  Good tag: counter_out[i] is the counter, and with
 * inner_len != NULL: n == 0 is a keepalive, inner_len[i] = 0, SG_OK; version nibble 4
 * needs n >= 20 and L = be16(out[2..4]) with 20 <= L <= n; version nibble 6 needs
 * n >= 40 and L = 40 + be16(out[4..6]) with L <= n; then inner_len[i] = L, SG_OK.
 * Anything else is SG_STATUS_BAD_INNER with inner_len[i] = 0, the plaintext and
 * counter_out[i] left in place: the packet was authentic, and the receiver's replay
 * window advances for it, as in the Linux receive path.  With inner_len == NULL nothing
 * is parsed and a good tag is SG_OK.
 *
 * In place.  Per packet, `in` and `out` either do not overlap or overlap in exactly one
 * way, the payload staying at its address: seal out_i + 16 == in_i (16 bytes of headroom
 * in front of the inner packet, sg_wg_message_len bytes of room from out_i), open
 * out_i == in_i + 16.  Any other overlap is undefined and not checked (the offsets are
 * device arrays).
 *
 * Left with the caller: the mapping from a received message's receiver index to
 * key_index; the replay window (RFC 6479) over counter_out; the counter limit
 * REJECT_AFTER_MESSAGES (2^64 - 2^13 - 1); the allowed-IPs check of the inner source
 * address; the handshake messages (types 1-3) and their BLAKE2s key derivation.
 *
 * One launch, no workspace, no host read-back: the call is capturable.  count == 0
 * returns SG_OK and launches nothing.  SG_E_ARG before any GPU work: NULL b, unknown
 * flags, NULL keys / status / in / out, NULL receiver or counter on seal, NULL
 * counter_out on open, a misaligned per-packet array (4 bytes; 8 for counter,
 * counter_out, in_off, out_off), num_keys zero, pad_cap above SG_WG_MAX_MESSAGE_LEN - 32,
 * the length bound above SG_WG_MAX_MESSAGE_LEN (seal: - 32). */
#define SG_WG_HEADER_LEN      16u
#define SG_WG_MAX_MESSAGE_LEN 16384u      /* header and tag included */
#define SG_WG_KEEP_FAILED     0x1u
#define SG_STATUS_BAD_HEADER  6           /* open: first four bytes are not 04 00 00 00 */
#define SG_STATUS_BAD_INNER   7           /* open: tag good, inner IP header's length does not fit */

typedef struct sg_wg_batch {
    uint32_t        count, flags;
    const uint8_t*  keys;        /* device [num_keys][32]: one row per session direction              */
    const uint32_t* receiver;    /* seal: device [num_keys], the index written into the header; open: not read */
    const uint32_t* key_index;   /* device, or NULL: 0                                                */
    const uint64_t* counter;     /* seal: device, the counter of each packet; open: not read          */
    uint64_t*       counter_out; /* open: device, the counter read from the wire; seal: not read      */
    uint32_t*       inner_len;   /* open: device or NULL (above); seal: not read                      */
    uint32_t        num_keys, pad_cap;
    const uint8_t*  in;
    const uint64_t* in_off;
    uint64_t        in_stride;
    uint8_t*        out;
    const uint64_t* out_off;
    uint64_t        out_stride;
    const uint32_t* len;
    uint32_t        uniform_len;
    uint32_t        max_len;
    uint8_t*        status;      /* device, count bytes, required for seal and open                   */
    void*           stream;      /* as sg_batch.stream: non-NULL asynchronous, NULL waits             */
} sg_wg_batch;                   /* 144 bytes */
int sg_seal_batch_wg(const sg_wg_batch* b);
int sg_open_batch_wg(const sg_wg_batch* b);

/* Host only.  sg_wg_padded_len: P of an inner packet of len bytes (above); a len whose
 * rounding does not fit 32 bits is returned as it is.  sg_wg_message_len: 32 + P, the
 * room a seal needs from out_i; 0xffffffff where that does not fit 32 bits. */
uint32_t sg_wg_padded_len(uint32_t len, uint32_t pad_cap);
uint32_t sg_wg_message_len(uint32_t len, uint32_t pad_cap);

/* ---- IPsec ESP batch, ChaCha20-Poly1305 (RFC 7634 over RFC 4303) ---------------
 * Many ESP packets sealed or opened in one launch (sg_esp.hip).  The packet:
 *
 *   be32(spi)
 *   be32(seq_lo)                        low 32 bits of the sequence number
 *   iv, 8 bytes                         be64(iv_i)
 *   AEAD(key, nonce = salt(4) || iv(8),
 *        plaintext = payload || 01 02 .. pad || u8(pad) || u8(next_header),
 *        AD = be32(spi) || be32(seq_lo)                  (8 bytes), or under SG_ESP_ESN
 *             be32(spi) || be32(seq_hi) || be32(seq_lo)  (12 bytes; seq_hi is not on the wire))
 *                                       -> P bytes || 16-byte ICV
 *
 * A packet is 32 + P bytes: 16 bytes of header, P bytes of ciphertext and a 16-byte ICV.
 * The AEAD is RFC 8439: ChaCha20 blocks 1 onward, the Poly1305 key from block 0, the MAC
 * over pad16(AD) || ct || pad16 || le64(|AD|) || le64(P).  A generic AEAD call leaves the
 * nonce, the AD with its implicit high half, the trailer and, on receive, the look at the
 * plaintext that finds the trailer to the host; here they are part of the launch.
 *
 * Packet i lies at in + in_off_i (off_i = off ? off[i] : stride * i) and has len_i =
 * len ? len[i] : uniform_len bytes, as in sg_wg_batch; any alignment of `in`, `out` and
 * the offsets.  k = min(sa_index ? sa_index[i] : 0, num_sas - 1) names the row of `keys`,
 * `salts`, `spi` and `replay_top`: one row per security association and direction.
 *
 * Seal.  The input is the payload, len_i bytes (0 allowed), contents not inspected.
 * pad_i = (align - (len_i + 2) mod align) mod align with `align` a multiple of 4 in
 * 4..256, so pad_i <= 255 and P_i = len_i + pad_i + 2 = sg_esp_padded_len(len_i, align).
 * The padding bytes are 1 .. pad_i (RFC 4303 section 2.4), then u8(pad_i), then the next
 * header: next_header ? next_header[i] : uniform_next_header.  They are never read from
 * the input: no input byte at or beyond len_i is read.  The sequence number is seq[i];
 * without SG_ESP_ESN it is taken mod 2^32 (the high half is ignored, also where it
 * stands in for the IV).  The IV is iv ? iv[i] : that sequence number; it must never
 * repeat under one key (RFC 7634 section 2), which a counter gives.  The output is
 * 32 + P_i bytes: header (spi[k]), ciphertext, ICV.  Status SG_OK, or SG_STATUS_SKIPPED
 * and nothing written where len_i > max_len.  The bound is on P: sg_esp_packet_len(
 * max_len or uniform_len, align) is at most SG_ESP_MAX_PACKET_LEN, so no packet of a seal
 * is longer than that -- a payload bound of SG_ESP_MAX_PACKET_LEN - 34 at align 4 and 16.
 *
 * Open.  The input is a packet of len_i bytes.  In this order: len_i > max_len is
 * SG_STATUS_SKIPPED, len_i < 34 is SG_E_SHORT (no trailer fits), a wire SPI other than
 * spi[k] is SG_STATUS_BAD_HEADER; nothing is written for any of them (seq_out,
 * payload_len and next_header_out included).  Otherwise seq_lo and the IV are read off
 * the wire, under SG_ESP_ESN seq_hi = sg_esp_seq_hi(replay_top[k], window, seq_lo) (RFC
 * 4303 appendix A2.1: the one 64-bit number with those low bits in [T - W + 1,
 * T - W + 1 + 2^32), all arithmetic mod 2^32 as in Linux xfrm_replay_seqhi; a wrapped
 * guess fails its ICV), and n = len_i - 32 bytes are decrypted into `out`: payload,
 * padding and trailer, left in place.  Bad ICV: SG_E_BAD_MAC, all n output bytes zero,
 * seq_out[i], payload_len[i] and next_header_out[i] 0; under SG_ESP_KEEP_FAILED the
 * decryption and the inferred 64-bit sequence number are left instead, payload_len[i]
 * and next_header_out[i] still 0.  Good ICV: seq_out[i] is the 64-bit sequence number
 * (zero-extended without ESN), and with payload_len != NULL: pad = out[n - 2], nh =
 * out[n - 1]; where pad + 2 <= n and the pad bytes are exactly 1 .. pad, payload_len[i] =
 * n - 2 - pad, next_header_out[i] = nh, SG_OK.  Anything else is SG_STATUS_BAD_INNER with
 * payload_len[i] and next_header_out[i] 0, the plaintext and seq_out[i] left: the packet
 * was authentic, and the caller's window advances for it.  With payload_len == NULL
 * nothing is parsed and a good ICV is SG_OK.  max_len is at most SG_ESP_MAX_PACKET_LEN.
 *
 * In place.  Per packet, `in` and `out` either do not overlap or overlap in exactly one
 * way, the payload staying at its address: seal out_i + 16 == in_i (16 bytes of headroom
 * in front of the payload, sg_esp_packet_len bytes of room from out_i), open
 * out_i == in_i + 16.  Any other overlap is undefined and not checked.
 *
 * Left with the caller: the lookup from a received SPI to sa_index; the anti-replay
 * window itself over seq_out and the update of replay_top; sequence number overflow and
 * rekeying; TFC padding and dummy packets (next header 59); tunnel versus transport
 * mode, that is what the payload is; UDP encapsulation (RFC 3948); IKE.
 *
 * One launch, no workspace, no host read-back: the call is capturable.  count == 0
 * returns SG_OK and launches nothing.  SG_E_ARG before any GPU work: NULL b, unknown
 * flags, NULL keys / salts / spi / status / in / out, NULL seq on seal, NULL seq_out on
 * open, payload_len without next_header_out or the reverse, under SG_ESP_ESN on open a
 * NULL replay_top or a window outside 1..2^31, a misaligned array (4 bytes for salts,
 * spi, sa_index, payload_len, len; 8 for seq, iv, seq_out, replay_top, in_off, out_off),
 * num_sas zero, an align that is no multiple of 4 in 4..256, uniform_next_header above
 * 255, the length bounds above. */
#define SG_ESP_HEADER_LEN     16u
#define SG_ESP_MAX_PACKET_LEN 16384u      /* header and ICV included */
#define SG_ESP_ESN            0x1u        /* extended sequence numbers: 12-byte AD, seq_hi implicit */
#define SG_ESP_KEEP_FAILED    0x2u

typedef struct sg_esp_batch {
    uint32_t        count, flags;
    const uint8_t*  keys;            /* device [num_sas][32]                                             */
    const uint8_t*  salts;           /* device [num_sas][4], 4-byte aligned                              */
    const uint32_t* spi;             /* device [num_sas], values: written and compared big-endian        */
    const uint32_t* sa_index;        /* device, or NULL: 0                                               */
    const uint64_t* seq;             /* seal: device, the sequence number of each packet; open: not read */
    const uint64_t* iv;              /* seal: device, or NULL: the sequence number; open: not read       */
    const uint8_t*  next_header;     /* seal: device, or NULL: uniform_next_header; open: not read       */
    uint64_t*       seq_out;         /* open: device, the 64-bit sequence number; seal: not read         */
    uint32_t*       payload_len;     /* open: device or NULL (above); seal: not read                     */
    uint8_t*        next_header_out; /* open: device, with payload_len; seal: not read                   */
    const uint64_t* replay_top;      /* open under SG_ESP_ESN: device [num_sas], T of each SA            */
    uint32_t        num_sas, align;
    uint32_t        uniform_next_header, window;
    const uint8_t*  in;
    const uint64_t* in_off;
    uint64_t        in_stride;
    uint8_t*        out;
    const uint64_t* out_off;
    uint64_t        out_stride;
    const uint32_t* len;
    uint32_t        uniform_len;
    uint32_t        max_len;
    uint8_t*        status;          /* device, count bytes, required for seal and open                  */
    void*           stream;          /* as sg_batch.stream: non-NULL asynchronous, NULL waits            */
} sg_esp_batch;                      /* 192 bytes */
int sg_seal_batch_esp(const sg_esp_batch* b);
int sg_open_batch_esp(const sg_esp_batch* b);

/* Host only.  sg_esp_padded_len: P of a payload of len bytes (above; an align of 0 is
 * taken as 1); sg_esp_packet_len: 32 + P, the room a seal needs from out_i.  Both give
 * 0xffffffff where the result does not fit 32 bits.  sg_esp_seq_hi: what the open kernel
 * infers per packet from T = top and W = window. */
uint32_t sg_esp_padded_len(uint32_t len, uint32_t align);
uint32_t sg_esp_packet_len(uint32_t len, uint32_t align);
uint32_t sg_esp_seq_hi(uint64_t top, uint32_t window, uint32_t seq_lo);

/* ---- DTLS 1.3 record batch, TLS_CHACHA20_POLY1305_SHA256 (RFC 9147 section 4) ----
 * Many DTLSCiphertext records sealed or opened in one launch (sg_dtls13.hip).  The record:
 *
 *   0 0 1 C S L E E                     first byte: C = 0x10, S = 0x08, L = 0x04, EE = epoch mod 4
 *   connection ID, cid_len bytes        where C is set
 *   sequence number, low 8 bits (S = 0) or low 16 bits (S = 1), big-endian
 *   be16(|encrypted_record|)            where L is set
 *   encrypted_record = AEAD(key, nonce = iv XOR (00 00 00 00 || be64(seq)),
 *        plaintext = content || u8(type) || zeros,
 *        AD = the header above, its sequence number bytes as they are before record
 *             number encryption)        -> n bytes || 16-byte tag
 *
 * hdr_len = sg_dtls13_header_len(flags, cid_len) = 1 + cid_len + (S ? 2 : 1) + (L ? 2 : 0),
 * 2..255 bytes; a record is hdr_len + n + 16 bytes.  The AEAD is RFC 8439: ChaCha20 blocks
 * 1 onward, the Poly1305 key from block 0, the MAC over pad16(AD) || ct || pad16 ||
 * le64(hdr_len) || le64(n).  The nonce takes the 64-bit sequence number alone; the epoch
 * does not enter it.  Record number encryption (section 4.2.3): sample = the first 16
 * bytes of encrypted_record (tag bytes among them where n < 16); mask = the first bytes
 * of the ChaCha20 block under sn_key with counter le32(sample[0..4)) and nonce
 * sample[4..16); the one or two sequence number bytes are XORed with mask[0..].  The
 * first byte is not masked.
 *
 * Tables.  k = min(key_index ? key_index[i] : 0, num_conns - 1).  Without
 * SG_DTLS13_EPOCH_ROWS keys, ivs, sn_keys and expected have num_conns rows and the row is
 * k.  With it they have 4 * num_conns rows and the row is 4 k + EE: unlike QUIC's header
 * protection key, sn_key changes with the epoch.  EE is epoch ? epoch[i] : uniform_epoch,
 * mod 4, on seal and the wire's two bits on open.  cids has one row of cid_len bytes per
 * connection, row k, and is read on seal only.
 *
 * Record i lies at in + in_off_i (off_i = off ? off[i] : stride * i) and has len_i =
 * len ? len[i] : uniform_len bytes, as in sg_quic_batch; any alignment of `in`, `out` and
 * the offsets.  `in` and `out` of a call must not overlap (not checked; the result is
 * undefined where they do): there is no in-place form.
 *
 * Seal.  The input is the content, len_i bytes (0 allowed), not inspected.  n_i =
 * sg_dtls13_inner_len(len_i, pad_to): len_i + 1, and where pad_to > 1 that rounded up to
 * a multiple of pad_to but to at most 2^14 + 1.  The type byte (type ? type[i] :
 * uniform_type; a zero would read as padding) and the zeros are made by the call: no
 * input byte at or beyond len_i is read.  SG_DTLS13_SEQ16 and SG_DTLS13_LENGTH choose S
 * and L for the whole call; C is set where cid_len != 0.  The output is
 * sg_dtls13_record_len(len_i, pad_to, flags, cid_len) bytes: header, ciphertext, tag,
 * with the mask applied last.  Status SG_OK, or SG_STATUS_SKIPPED and nothing written
 * where len_i > max_len.  max_len is at most SG_DTLS13_MAX_CONTENT_LEN.
 *
 * Open.  The input is a record of len_i bytes; cid_len is the call's (the caller found
 * the connection by its CID), S, L and EE are the record's.  In this order, with nothing
 * written (seq_out, epoch_out, content_len and type_out included): len_i > max_len is
 * SG_STATUS_SKIPPED; len_i == 0 is SG_E_SHORT; top three bits other than 001, or C
 * disagreeing with cid_len != 0, is SG_STATUS_BAD_HEADER; len_i < hdr_len + 16 is
 * SG_E_SHORT; L set and the length field other than len_i - hdr_len is
 * SG_STATUS_BAD_HEADER.  Otherwise the sequence number bytes are unmasked and the full
 * number is sg_quic_decode_pn(expected[row], those bits, 1 or 2): expected is the
 * caller's to keep at the highest deprotected number + 1 of each row, as ESP's
 * replay_top.  n = len_i - hdr_len - 16 inner bytes are decrypted into `out`;
 * epoch_out[i] = EE.  Bad tag: SG_E_BAD_MAC, all n output bytes zero, seq_out[i],
 * content_len[i] and type_out[i] 0; under SG_DTLS13_KEEP_FAILED the decryption and the
 * decoded number are left instead, content_len[i] and type_out[i] still 0.  Good tag:
 * seq_out[i] is the number, and the last non-zero inner byte is the type: type_out[i],
 * content_len[i] = its index, SG_OK; no such byte (or n = 0) is SG_STATUS_NO_TYPE with
 * both 0.  The inner plaintext is left in `out` either way.  max_len is at most
 * SG_DTLS13_MAX_RECORD_LEN.
 *
 * Left with the caller: the handshake and its messages; ACKs; the replay window over
 * seq_out and the update of expected; the epoch's upper bits (which of the generations
 * with these two low bits is meant) and the key tables behind them; the AEAD usage limits
 * of section 4.5.3; splitting a datagram into records (a record without L ends it) and
 * the lookup from a CID to key_index.  The AES suites, whose mask is AES-ECB, are not here.
 *
 * One launch, no workspace, no host read-back: the call is capturable.  count == 0
 * returns SG_OK and launches nothing.  SG_E_ARG before any GPU work: NULL b, unknown
 * flags, NULL keys / ivs / sn_keys / status / in / out, NULL seq on seal, NULL expected /
 * seq_out / epoch_out / content_len / type_out on open, cids NULL with cid_len != 0 on
 * seal, a misaligned array (4 bytes for ivs, key_index, content_len, len; 8 for seq,
 * expected, seq_out, in_off, out_off), num_conns zero, cid_len above
 * SG_DTLS13_MAX_CID_LEN, pad_to above 2^14, the length bounds above. */
#define SG_DTLS13_MAX_CONTENT_LEN 16384u
#define SG_DTLS13_MAX_CID_LEN       250u  /* so that the header (AD) is <= 255 = SG_MAX_AD_LEN */
#define SG_DTLS13_MAX_RECORD_LEN  (255u + 16384u + 1u + 16u)
#define SG_DTLS13_SEQ16           0x1u    /* seal: 16-bit sequence number on the wire (S) */
#define SG_DTLS13_LENGTH          0x2u    /* seal: the length field is present (L) */
#define SG_DTLS13_EPOCH_ROWS      0x4u    /* four rows per connection, chosen by EE */
#define SG_DTLS13_KEEP_FAILED     0x8u

typedef struct sg_dtls13_batch {
    uint32_t        count, flags;
    const uint8_t*  keys;          /* device [rows][32]                                              */
    const uint8_t*  ivs;           /* device [rows][12], 4-byte aligned                              */
    const uint8_t*  sn_keys;       /* device [rows][32]                                              */
    const uint8_t*  cids;          /* seal: device [num_conns][cid_len], NULL where cid_len is 0; open: not read */
    const uint32_t* key_index;     /* device, or NULL: 0                                             */
    const uint64_t* seq;           /* seal: device, the sequence number of each record; open: not read */
    const uint8_t*  type;          /* seal: device, or NULL: uniform_type; open: not read            */
    const uint8_t*  epoch;         /* seal: device, or NULL: uniform_epoch; open: not read           */
    const uint64_t* expected;      /* open: device [rows], highest deprotected number + 1; seal: not read */
    uint64_t*       seq_out;       /* open: device, the decoded sequence number; seal: not read      */
    uint8_t*        epoch_out;     /* open: device, EE off the wire; seal: not read                  */
    uint32_t*       content_len;   /* open: device, the content's length; seal: not read             */
    uint8_t*        type_out;      /* open: device, the content type; seal: not read                 */
    uint32_t        num_conns, cid_len;
    uint32_t        pad_to;        /* seal: 0 or 1 none, else the inner plaintext's multiple         */
    uint8_t         uniform_type, uniform_epoch;
    const uint8_t*  in;
    const uint64_t* in_off;
    uint64_t        in_stride;
    uint8_t*        out;
    const uint64_t* out_off;
    uint64_t        out_stride;
    const uint32_t* len;
    uint32_t        uniform_len;
    uint32_t        max_len;
    uint8_t*        status;        /* device, count bytes, required for seal and open                */
    void*           stream;        /* as sg_batch.stream: non-NULL asynchronous, NULL waits          */
} sg_dtls13_batch;                 /* 208 bytes */
int sg_seal_batch_dtls13(const sg_dtls13_batch* b);
int sg_open_batch_dtls13(const sg_dtls13_batch* b);

/* Host only.  sg_dtls13_header_len: hdr_len of a seal with these flags (the bits other
 * than SG_DTLS13_SEQ16 and SG_DTLS13_LENGTH are ignored).  sg_dtls13_inner_len: n of a
 * content of len bytes (above; a len of 2^14 or more is not padded).  sg_dtls13_record_len:
 * hdr_len + n + 16, the room a seal needs from out_i.  The last two give 0xffffffff where
 * the result does not fit 32 bits. */
uint32_t sg_dtls13_header_len(uint32_t flags, uint32_t cid_len);
uint32_t sg_dtls13_inner_len(uint32_t len, uint32_t pad_to);
uint32_t sg_dtls13_record_len(uint32_t len, uint32_t pad_to, uint32_t flags, uint32_t cid_len);

/* ---- long messages: any data and AD length, one message over the whole chip
 * Encryptor::encrypt / Decryptor::decrypt take data and additional data of any
 * length (cipher/mod.rs:22-32, chacha20_poly1305.rs:19-94).  sg_seal, sg_open
 * and the record batch (sg_seal_batch / sg_open_batch) keep their bounds
 * (SG_MAX_AD_LEN, SG_MAX_RECORD_LEN); the message batch further below
 * (sg_seal_msg_batch / sg_open_msg_batch) has none but SG_MSG_MAX_LEN.
 * The message calls below take one key, one nonce, n data bytes and ad_len AD
 * bytes, same construction, and spread the one message over a persistent grid
 * (sg_msg.hip: the MAC stream is cut into tiles whose Poly1305 partial sums
 * are combined exactly, so the tag is the sequential one bit for bit).
 *
 * The bound is 4 GiB - 64 for data and, separately, for AD: well inside the
 * 2^32 blocks of the counter (state word 12 only).  The kernels index with 64
 * bits throughout; the bound is where the CPU parity checker can still verify
 * a message within a test's time, and lifting it needs only a faster checker. */
#define SG_MSG_MAX_LEN      0xFFFFFFC0ull   /* data bytes and, separately, AD bytes */
#define SG_MSG_KEEP_FAILED  0x1u            /* open: leave the unauthenticated plaintext
                                               of a failed open in `out` (default: zeroed
                                               on the device, same stream)              */
/* RFC 8439 (sections 2.3, 2.8) instead of the draft, in sg_msg.flags and
 * sg_msg_batch.flags (the whole batch call; there is no per-item choice):
 *   - the 96-bit nonce is nonce_hi[0..4) || nonce[0..8): state word 13 =
 *     le32(nonce_hi), words 14 and 15 = the two words of nonce, as in the draft;
 *     word 12 is the 32-bit block counter, block 0 gives the Poly1305 key and
 *     the data uses blocks 1 onward, as in the draft;
 *   - the MAC runs over ad || zeros to a multiple of 16 || ct || zeros to a
 *     multiple of 16 || le64(ad_len) || le64(n); nothing is padded where a
 *     length is a multiple of 16 already, 0 included.
 * Without the flag nonce_hi is never read (callers of before the field existed
 * leave whatever their padding held there).  The value is not 0x2 or 0x4. */
#define SG_MSG_RFC8439      0x100u
#define SG_RFC8439_NONCE_LEN 12u

typedef struct sg_msg {
    const uint8_t* key;        /* 32 bytes, device                                  */
    uint8_t        nonce[8];   /* by value; RFC 8439: the nonce's last 8 bytes      */
    const uint8_t* ad;         /* device, ad_len bytes                              */
    uint64_t       ad_len;
    const uint8_t* in;         /* device; seal: n bytes of pt, open: n + 16 (ct||tag) */
    uint64_t       in_len;
    uint8_t*       out;        /* device; seal: n + 16, open: n. out == in allowed   */
    uint8_t*       status;     /* open: one device byte (SG_OK / SG_E_BAD_MAC)      */
    uint32_t       flags;      /* SG_MSG_*                                          */
    uint8_t        nonce_hi[4]; /* SG_MSG_RFC8439: the nonce's first 4 bytes; else
                                  never read (the struct's former padding)          */
    void*          stream;     /* as sg_batch.stream; non-NULL: fully asynchronous   */
    void*          workspace;  /* >= sg_msg_workspace_size() bytes, 16-byte aligned
                                  device memory, or NULL: library cache (not under
                                  stream capture)                                    */
    size_t         workspace_size;
} sg_msg;

size_t sg_msg_workspace_size(void);
/* Device-resident message.  Any alignment of in, out and ad; out may equal in
 * exactly (in place), any other overlap is SG_E_ARG.  Open returns SG_E_SHORT
 * for in_len < 16 before anything is touched; otherwise the MAC result lands
 * in *status, after the decryption has run unconditionally
 * (chacha20_poly1305.rs:80-93).  Returns SG_OK, SG_E_SHORT or < 0. */
int sg_seal_msg_dev(const sg_msg* m);
int sg_open_msg_dev(const sg_msg* m);

/* Host pointers, same argument meaning and return values as sg_seal / sg_open,
 * any length up to SG_MSG_MAX_LEN.  AD and data are copied into device buffers
 * of a per-context cache that only grows, the device form runs on the
 * context's stream, and the result is copied back; a failed open copies
 * nothing back and zeroes out.  There is no chunked pipeline: these calls are
 * bound by the host link and exist for the trait path (Encryptor::encrypt /
 * Decryptor::decrypt above the single-record bounds). */
int sg_seal_msg(sg_ctx* ctx, const uint8_t* nonce, size_t nonce_len, const uint8_t* pt, size_t n,
                const uint8_t* ad, size_t adlen, uint8_t* out);
int sg_open_msg(sg_ctx* ctx, const uint8_t* nonce, size_t nonce_len, const uint8_t* in, size_t in_len,
                const uint8_t* ad, size_t adlen, uint8_t* out);
/* The same two calls in RFC 8439 (SG_MSG_RFC8439 above): nonce_len must be 12
 * (else SG_E_ARG "nonce must be 12 bytes"); sg_seal_msg / sg_open_msg keep
 * refusing anything but 8.  Any length from 0 up, same context, same returns. */
int sg_seal_msg_rfc8439(sg_ctx* ctx, const uint8_t* nonce, size_t nonce_len, const uint8_t* pt, size_t n,
                        const uint8_t* ad, size_t adlen, uint8_t* out);
int sg_open_msg_rfc8439(sg_ctx* ctx, const uint8_t* nonce, size_t nonce_len, const uint8_t* in, size_t in_len,
                        const uint8_t* ad, size_t adlen, uint8_t* out);

/* The launch geometry of a message (host only, no GPU): the MAC stream
 * ad || le64(ad_len) || ct || le64(n) has mac_blocks 16-byte blocks (the last
 * may be short); zero_blocks virtual all-zero blocks in front make
 * zero_blocks + mac_blocks == tiles * tile_blocks; tile_bytes = 16 *
 * tile_blocks; group g of `groups` workgroups owns tiles
 * [g * tiles_per_group, min(tiles, (g + 1) * tiles_per_group)).  The kernels
 * take exactly this struct.  groups: 0 = automatic, else the wanted number of
 * workgroups (the plan may use fewer: no group is empty).  SG_OK or SG_E_ARG
 * (NULL out, a length above SG_MSG_MAX_LEN). */
typedef struct sg_msg_plan {
    uint64_t mac_blocks, tiles, zero_blocks;
    uint32_t tile_blocks, tile_bytes, groups, tiles_per_group; /* last group takes the rest */
} sg_msg_plan;
int sg_msg_plan_for(uint64_t n, uint64_t adlen, uint32_t groups /* 0 = automatic */, sg_msg_plan* out);
/* The same for a call with `flags` (SG_MSG_*): with SG_MSG_RFC8439 the stream
 * is the padded one, 16 * ceil(adlen / 16) + 16 * ceil(n / 16) + 16 bytes, so
 * its last block is always full; every other rule is the same.  Flags 0 give
 * sg_msg_plan_for, field for field.  Unknown flags: SG_E_ARG. */
int sg_msg_plan_for_flags(uint64_t n, uint64_t adlen, uint32_t flags, uint32_t groups, sg_msg_plan* out);

/* Workgroups of the message kernels: 0 = automatic, else that many (at most
 * 1024); a test and A/B switch like sg_set_lockstep.  Initial value:
 * environment SG_MSG_GROUPS, else 0.  Returns the previous setting; a negative
 * argument only queries. */
int sg_set_msg_groups(int n);

/* ---- message batch: many long messages of any length on one grid ---------
 * The message path's decomposition applied across messages: every message of
 * the call has its own key index, nonce, AD and lengths (data and AD each 0 to
 * SG_MSG_MAX_LEN, any pointer alignment), one persistent grid walks the tiles
 * of all messages and one finish launch writes (or compares) all tags
 * (sg_msg_batch.hip).  Same construction, bit for bit the sequential tag.
 *
 * The items array lives in HOST memory and is consumed before the call
 * returns; everything it points to is device memory.  Within a message
 * out == in exactly is allowed and any other overlap of its in and out is
 * SG_E_ARG, as in the single call.  Overlap BETWEEN messages of a call (one
 * message's out with another's in, out or ad) is the caller's responsibility:
 * it is not checked, and the result is undefined.
 *
 * Open: status[i] is SG_OK, SG_E_BAD_MAC or SG_E_SHORT and the call itself
 * returns SG_OK.  A message with in_len < 16 gets SG_E_SHORT, its output is
 * left untouched and the other messages proceed (as sg_open_batch per record).
 * The decryption always runs (chacha20_poly1305.rs:80-93); a failed message's
 * out[0, n) is zeroed on the device in the same stream unless
 * SG_MSG_KEEP_FAILED is set.
 *
 * stream and workspace as in sg_msg: non-NULL stream = fully asynchronous,
 * NULL = synchronous on the null stream; a caller workspace of
 * sg_msg_batch_workspace_size(count) bytes, 16-byte aligned, or NULL for the
 * library cache.  The plan and the per-message descriptors are uploaded into
 * the workspace by a copy that a stream capture cannot record: under capture
 * the call returns SG_E_ARG, with or without a caller workspace.
 * count == 0 returns SG_OK and launches nothing.  NULL pointers where a
 * length is non-zero, unknown flags, count above SG_MSG_BATCH_MAX_COUNT, a
 * workspace too small or misaligned and key_index >= num_keys are SG_E_ARG
 * before any GPU call. */
#define SG_MSG_BATCH_MAX_COUNT  (1u << 20)

typedef struct sg_msg_item {
    uint32_t       key_index;  /* < num_keys                                        */
    uint8_t        nonce[8];   /* by value; RFC 8439: the nonce's last 8 bytes      */
    uint8_t        nonce_hi[4]; /* SG_MSG_RFC8439: the nonce's first 4 bytes; else
                                  never read (the struct's former padding)          */
    const uint8_t* ad;         /* device, ad_len bytes                              */
    uint64_t       ad_len;
    const uint8_t* in;         /* device; seal: n bytes of pt, open: n + 16 (ct||tag) */
    uint64_t       in_len;
    uint8_t*       out;        /* device; seal: n + 16, open: n. out == in allowed   */
} sg_msg_item;

typedef struct sg_msg_batch {
    uint32_t           count;
    uint32_t           flags;      /* SG_MSG_KEEP_FAILED, SG_MSG_RFC8439            */
    const uint8_t*     keys;       /* device key table [num_keys][32], as sg_batch  */
    uint32_t           num_keys;
    const sg_msg_item* items;      /* HOST, count entries                           */
    uint8_t*           status;     /* device, count bytes; required for open        */
    void*              stream;
    void*              workspace;
    size_t             workspace_size;
} sg_msg_batch;

size_t sg_msg_batch_workspace_size(uint32_t count);
int sg_seal_msg_batch(const sg_msg_batch* b);
int sg_open_msg_batch(const sg_msg_batch* b);

/* The plan of a message batch (host only, no GPU).  Message m gets exactly
 * the geometry of sg_msg_plan_for(n[m], adlen[m], groups, &msgs[m]); only its
 * mac_blocks, tiles, zero_blocks and tile size matter here.  The messages'
 * tiles, in order, form one global sequence of plan->tiles tiles; group g of
 * plan->groups workgroups owns global tiles [g * tiles_per_group,
 * min(tiles, (g + 1) * tiles_per_group)), none empty.  A group's run is cut at
 * message boundaries into segments: segment s is tiles [tile_begin, tile_end)
 * of message segs[s].msg, walked by group segs[s].group; segments are in
 * global tile order, at most groups + count - 1 of them.  group_segs[g] and
 * msg_segs[m] are the (first, count) runs of segs that belong to group g and
 * to message m.  groups: 0 = automatic (min(tiles, 1024)), else the wanted
 * number (the plan may use fewer).  msgs, segs, group_segs (1024 entries) and
 * msg_segs may each be NULL when not wanted; seg_cap is the room of segs.
 * O(count + groups).  The kernels take exactly these tables.
 * SG_OK, or SG_E_ARG (NULL plan, a NULL length array with count > 0, count
 * above SG_MSG_BATCH_MAX_COUNT, a length above SG_MSG_MAX_LEN, seg_cap too
 * small). */
typedef struct sg_msg_seg {
    uint32_t msg, tile_begin, tile_end, group;
} sg_msg_seg;
typedef struct sg_msg_span {
    uint32_t first, count;
} sg_msg_span;
typedef struct sg_msg_batch_plan {
    uint64_t tiles, tiles_per_group;
    uint32_t groups, segments, tile_blocks, tile_bytes;
} sg_msg_batch_plan;
int sg_msg_batch_plan_for(const uint64_t* n, const uint64_t* adlen, uint32_t count, uint32_t groups,
                          sg_msg_batch_plan* plan, sg_msg_plan* msgs, sg_msg_seg* segs, uint32_t seg_cap,
                          sg_msg_span* group_segs, sg_msg_span* msg_segs);
/* The same for a call with `flags`: message m gets the geometry of
 * sg_msg_plan_for_flags(n[m], adlen[m], flags, groups, &msgs[m]).  Flags 0
 * give sg_msg_batch_plan_for; unknown flags: SG_E_ARG. */
int sg_msg_batch_plan_for_flags(const uint64_t* n, const uint64_t* adlen, uint32_t count, uint32_t flags,
                                uint32_t groups, sg_msg_batch_plan* plan, sg_msg_plan* msgs, sg_msg_seg* segs,
                                uint32_t seg_cap, sg_msg_span* group_segs, sg_msg_span* msg_segs);

/* ---- batched record layer over host memory ------------------------------
 * The throughput form of TlsWriter / TlsReader (tls.rs:68-380): many records
 * per call, pipelined inside the library, up to four chunks of 256 records in
 * flight.  Unregistered (pageable) buffers: the records are framed through
 * pinned staging that the kernels read and write over the host link
 * themselves.  Registered buffers (sg_host_register): host<->device copies
 * straight from and into them, each step (copy in, kernels, copy out)
 * enqueued by the calling thread once the step before it has completed, so
 * that a reader and a writer on two contexts never queue behind each other's
 * unfinished work.  Wire format exactly as the reference writes and parses it:
 *   header = content_type || major || minor || be16(fragment length)
 *   (tls.rs:126-130, 218-236) followed by the fragment (ct || tag).        */
#define SG_RECORD_MAX_LEN      16384u              /* RECORD_MAX_LEN      tls.rs:32 */
#define SG_ENC_RECORD_MAX_LEN  (16384u + 2048u)    /* ENC_RECORD_MAX_LEN  tls.rs:35 */
#define SG_HEADER_LEN          5u
/* record-layer error codes (TlsErrorKind, tls_result.rs:5-20) */
#define SG_E_UNEXPECTED_MESSAGE 3  /* unknown content type (tls.rs:218-225)          */
#define SG_E_RECORD_OVERFLOW    4  /* fragment > 2^14 + 2048 (tls.rs:232-234), or a
                                      decrypted fragment > 2^14 (tls.rs:269-272,
                                      where the reference panics)                  */

/* Caller buffers for the record layer's zero-copy path: page-locks [p, p+len)
 * (hipHostRegister) and records the range.  When sg_write_records' `data` and
 * `wire`, or sg_read_records' `wire` and `out`, both lie inside registered
 * ranges, the record bytes move by DMA straight between those buffers and the
 * device -- no framing copy through the library's pinned staging
 * (sg_write_records builds each chunk's wire image, headers included, in HBM;
 * sg_read_records parses the headers on the host, takes the zero-copy path for
 * chunks of equal, back-to-back records, whose wire image it takes apart in
 * HBM, and clears the plaintext of a failed record and of every record after
 * it in `out`, as it delivers none of them).  Unregister only when no call uses the range.
 * SG_ZERO_COPY=0 in the environment disables the path.  SG_OK or SG_E_ARG /
 * SG_E_HIP. */
int sg_host_register(void* p, size_t len);
int sg_host_unregister(void* p);

/* Upper bound of the wire bytes sg_write_records produces for len bytes. */
size_t sg_wire_bound(size_t len);

/* TlsWriter::write_data (tls.rs:137-147) + write_record (:99-135) for a whole
 * buffer: `data` is cut into ceil(len / 2^14) fragments (len == 0 writes no
 * record, as the reference's chunks() loop yields none), record i is sealed with
 * seq = seq0 + i (nonce be64(seq), AD be64(seq)||type||major||minor||be16(n)),
 * and its wire image is appended to `wire`.  Host memory in and out.
 * Returns the number of records written (the caller adds it to its
 * write_count, tls.rs:132) or < 0; *wire_len = bytes written. */
int64_t sg_write_records(sg_ctx* ctx, uint64_t seq0, uint8_t content_type, uint8_t ver_major,
                         uint8_t ver_minor, const uint8_t* data, size_t len, uint8_t* wire,
                         size_t wire_cap, size_t* wire_len);

/* TlsReader::read_record (tls.rs:217-281) for every COMPLETE record at the
 * start of `wire`: header checks in the reference's order (unknown type ->
 * SG_E_UNEXPECTED_MESSAGE, length > 2^14+2048 -> SG_E_RECORD_OVERFLOW,
 * length < 16 -> SG_E_SHORT), AD = be64(seq)||type||major||minor||be16(len-16)
 * with seq = seq0 + i, open, and append the plaintext fragments to `out`.
 * Processing stops at the first failing record; the records before it are
 * delivered.  Per-record content types / plaintext lengths go to `types` /
 * `frag_lens` (capacity max_records, either may be NULL). */
typedef struct sg_read_result {
    uint64_t records;    /* records opened successfully (the caller adds this to read_count) */
    uint64_t consumed;   /* wire bytes of those records                                     */
    uint64_t out_len;    /* plaintext bytes written to out                                  */
    int32_t  error;      /* SG_OK, or the status of record number `records`                 */
    uint32_t _pad;
} sg_read_result;
int sg_read_records(sg_ctx* ctx, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out,
                    size_t out_cap, uint8_t* types, uint32_t* frag_lens, size_t max_records,
                    sg_read_result* res);

/* The header checks of sg_read_records alone (TlsReader::read_record,
 * tls.rs:217-238, 258-262, 269-272), host only -- no context, no GPU: the
 * complete records at the start of `wire` (at most max_records) go to `recs`
 * (offset of the fragment after its 5-byte header, fragment length, type,
 * version), *count of them; *error = SG_OK, or the error of the first bad
 * header (SG_E_UNEXPECTED_MESSAGE, SG_E_RECORD_OVERFLOW, SG_E_SHORT) that
 * stopped the parse.  An incomplete record at the end is not an error.
 * Returns SG_OK or SG_E_ARG. */
typedef struct sg_wire_record {
    uint64_t offset;
    uint32_t frag_len;
    uint8_t  type, ver_major, ver_minor, _pad;
} sg_wire_record;
int sg_parse_records(const uint8_t* wire, size_t wire_len, size_t max_records, sg_wire_record* recs,
                     size_t* count, int32_t* error);

/* Time (ms) spent by the last sg_write_records / sg_read_records call of this
 * thread in host->device copies, kernels and device->host copies (HIP events;
 * summed over the pipelined chunks; with unregistered buffers the kernels move
 * the bytes over the host link themselves and all device time counts as
 * kernels) and in host-side framing memcpy. */
int sg_record_timing(double* h2d_ms, double* kernel_ms, double* d2h_ms, double* host_ms);

/* ---- the record layer in RFC 7905 and TLS 1.3 -----------------------------
 * The calls above speak draft-agl-04 (suite 0xCC13).  The ones below carry the
 * same byte streams in the suites deployed peers negotiate, through the same
 * pipeline: sg_host_register, SG_ZERO_COPY, the direct pipeline,
 * sg_record_timing and the rule that calls on two contexts run concurrently
 * apply unchanged.  Each of them needs the context's write IV and returns
 * SG_E_ARG before any GPU work on a context that has none. */

/* Gives the context its 12-byte write IV (RFC 7905 section 2, RFC 8446 section
 * 5.3): a host copy and a 4-byte aligned device copy.  May be called again
 * (the last value holds; not while another call uses the context's records).
 * sg_ctx_new and every draft call behave as before, with or without an IV. */
int sg_ctx_set_iv(sg_ctx* ctx, const uint8_t iv[12]);

/* Derives key and IV from a TLS 1.3 traffic secret (RFC 8446 section 7.3) and
 * installs them: the 32 key bytes replace the context's key on the device, the
 * IV as sg_ctx_set_iv does.  The context keeps the secret for sg_ctx_key_update.
 * Not while another call uses the context, as sg_ctx_set_iv. */
int sg_ctx_set_traffic_secret(sg_ctx* ctx, const uint8_t secret[32]);
/* KeyUpdate (RFC 8446 section 4.6.3, 7.2): secret <- Expand-Label(secret,
 * "traffic upd", "", 32), then as above; the old secret's host copy is
 * overwritten.  SG_E_ARG on a context that never had a secret.  The caller
 * restarts its sequence numbers at 0 (section 5.3). */
int sg_ctx_key_update(sg_ctx* ctx);

/* RFC 7905 (TLS 1.2 suites 0xCCA8 / 0xCCA9): the signatures, wire format,
 * header checks, 13-byte AD, error order and sg_read_result of
 * sg_write_records / sg_read_records; the sealing is the RFC 8439 record batch
 * with nonce = iv XOR (00 00 00 00 || be64(seq)).  A read chunk whose records
 * differ in type or version runs in explicit mode with 12-byte nonces built on
 * the host from the context's IV. */
int64_t sg_write_records_rfc7905(sg_ctx* ctx, uint64_t seq0, uint8_t content_type, uint8_t ver_major,
                                 uint8_t ver_minor, const uint8_t* data, size_t len, uint8_t* wire,
                                 size_t wire_cap, size_t* wire_len);
int sg_read_records_rfc7905(sg_ctx* ctx, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out,
                            size_t out_cap, uint8_t* types, uint32_t* frag_lens, size_t max_records,
                            sg_read_result* res);

/* TLS 1.3 write (RFC 8446 section 5.1 - 5.3): `data` is cut into 2^14-byte
 * fragments (len == 0 writes no record); record i is
 *   17 03 03 be16(n_i + 17) || ct(content_i || inner_type) || tag
 * with seq = seq0 + i and no padding, so exactly len + 22 * nrec ==
 * sg_wire_bound_tls13(len) wire bytes are written.  inner_type == 0 is
 * SG_E_ARG (a zero would read as padding).  Returns the records written or
 * < 0; *wire_len = bytes written. */
size_t  sg_wire_bound_tls13(size_t len);
int64_t sg_write_records_tls13(sg_ctx* ctx, uint64_t seq0, uint8_t inner_type, const uint8_t* data, size_t len,
                               uint8_t* wire, size_t wire_cap, size_t* wire_len);

/* The header checks of sg_read_records_tls13 alone, host only; arguments and
 * results as sg_parse_records.  In this order: outer type other than 23 ->
 * SG_E_UNEXPECTED_MESSAGE, length above 2^14 + 256 -> SG_E_RECORD_OVERFLOW,
 * length below 16 -> SG_E_SHORT.  The version bytes are reported, not checked:
 * the additional data is built as 17 03 03 be16(length), so a record with
 * other version bytes fails its tag. */
int sg_parse_records_tls13(const uint8_t* wire, size_t wire_len, size_t max_records, sg_wire_record* recs,
                           size_t* count, int32_t* error);

/* TLS 1.3 read: every complete record at the start of `wire` is opened with
 * seq = seq0 + i and stripped of its inner type and padding; types[r] receives
 * the inner type, frag_lens[r] the content length, and the contents of the
 * delivered records lie back to back in `out`.  Processing stops at the first
 * record that fails its tag (SG_E_BAD_MAC), has no non-zero inner byte
 * (SG_E_UNEXPECTED_MESSAGE, RFC 8446 section 5.4) or has content longer than
 * 2^14 (SG_E_RECORD_OVERFLOW); records, consumed, out_len and error as in
 * sg_read_records.  out_cap must cover the sum of frag_len - 17 over the parsed
 * records with frag_len >= 17 (else SG_E_ARG).  On return no byte of `out`
 * beyond out_len holds plaintext and no byte outside [out, out + out_cap) has
 * been written: the contents are packed on the device (sg_gather_records'
 * kernel), chunk after chunk on one stream, and nothing behind the first
 * failing record leaves device memory on the zero-copy path. */
int sg_read_records_tls13(sg_ctx* ctx, uint64_t seq0, const uint8_t* wire, size_t wire_len, uint8_t* out,
                          size_t out_cap, uint8_t* types, uint32_t* frag_lens, size_t max_records,
                          sg_read_result* res);

/* The device step of the TLS 1.3 read on its own (tests, and callers of
 * sg_open_batch_tls13 that want its output packed): count <= 256 opened
 * records, record i at src + i * stride (src 16-byte aligned, stride a
 * multiple of 16 and >= 2^14), their status and content_len as
 * sg_open_batch_tls13 leaves them.  With ok = the first record whose status is
 * not SG_OK or whose content_len exceeds 2^14 (count if none; 0 if in->stopped)
 * and pre[i] = the content bytes before record i:
 *   dst[base + pre[i], + content_len[i]) <- the record's first content_len[i]
 *       bytes for i < ok, base = in->offset if use_base else 0; no other byte
 *       of dst is written; dst may have any alignment
 *   *out    = {in->offset + pre[ok], in->stopped | (ok < count)}
 *   result  = {ok, pre[ok]}
 * Every pointer is device memory (or device-visible host memory); in != out.
 * Asynchronous on `stream` (NULL: the null stream, and the call waits).
 * SG_OK, SG_E_ARG or SG_E_HIP. */
typedef struct sg_gather_cursor {
    uint64_t offset;
    uint32_t stopped;
    uint32_t _pad;
} sg_gather_cursor;
int sg_gather_records(const uint8_t* src, uint32_t stride, const uint8_t* status, const uint32_t* content_len,
                      uint32_t count, uint8_t* dst, int use_base, const sg_gather_cursor* in,
                      sg_gather_cursor* out, uint32_t* result, void* stream);

/* How a TLS 1.3 read chunk that goes through the library's pinned staging
 * (unregistered buffers) leaves it: 1 = the gather kernel packs the chunk's
 * contents into the pinned output and the host makes one memcpy per chunk,
 * 0 = the host copies record by record from the content lengths, as the draft
 * path does.  Calls on registered buffers gather on the device either way.
 * Same bytes and results in both; an A/B and test switch like sg_set_lockstep.
 * Initial value: environment SG_RECORD13_GATHER ("0"/"1"), else 0 (by
 * measurement).  Returns the previous setting; a negative
 * argument only queries. */
int sg_set_record13_gather(int enable);

/* ---- TLS 1.2 key schedule on the host (cipher/prf.rs, client.rs:130-225) --
 * Produces the per-connection key tables the batch calls take.  CPU only
 * (no device needed); the reference's hmac_sha256 panics for keys longer than
 * 64 bytes (prf.rs:11-14): SG_E_ARG here. */
void sg_sha256(const uint8_t* msg, size_t len, uint8_t out[32]);          /* crypto/sha2.rs:18-116 */
int  sg_hmac_sha256(const uint8_t* key, size_t key_len, const uint8_t* msg, size_t len,
                    uint8_t out[32]);                                     /* prf.rs:8-29          */
typedef struct sg_prf sg_prf;                                             /* prf.rs:31-36 Prf     */
sg_prf* sg_prf_new(const uint8_t* secret, size_t secret_len,
                   const uint8_t* seed, size_t seed_len);                 /* prf.rs:38-48         */
int  sg_prf_get_bytes(sg_prf* prf, uint8_t* out, size_t n);               /* prf.rs:60-89         */
void sg_prf_free(sg_prf* prf);
/* client.rs:130-163 for `count` connections (threads >= 1):
 *   master_secret_i = PRF(pre_master_i, "master secret" || client_random_i || server_random_i)[0..48]
 *   key block = PRF(master_secret_i, "key expansion" || server_random_i || client_random_i)
 *   client_write_key_i = key block[0..32] (the client's encryptor key, client.rs:152-154)
 *   server_write_key_i = key block[32..64] (the client's decryptor key, :157)
 * pre_master_i = pre_master + pm_stride*i (pm_len bytes); randoms are [count][32];
 * master_secret ([count][48]) may be NULL. */
int  sg_derive_keys(uint32_t count, const uint8_t* pre_master, size_t pm_len, size_t pm_stride,
                    const uint8_t* client_random, const uint8_t* server_random, uint8_t* master_secret,
                    uint8_t* client_write_keys, uint8_t* server_write_keys, int threads);
/* The same with the write IVs of RFC 7905 section 2 ([count][12] each): the key
 * block is 88 bytes, the two 32-byte keys (as above, the same bytes) and then
 * client_write_IV and server_write_IV (RFC 5246 section 6.3 with no MAC keys).
 * The IVs feed sg_batch_rfc8439.ivs. */
int  sg_derive_keys_ivs(uint32_t count, const uint8_t* pre_master, size_t pm_len, size_t pm_stride,
                        const uint8_t* client_random, const uint8_t* server_random, uint8_t* master_secret,
                        uint8_t* client_write_keys, uint8_t* server_write_keys, uint8_t* client_write_ivs,
                        uint8_t* server_write_ivs, int threads);
/* client.rs:184-192 (server = 0, "client finished") / :213-221 (server = 1,
 * "server finished"): PRF(master_secret, label || handshake_hash)[0..12]. */
int  sg_finished_verify_data(const uint8_t master_secret[48], int server,
                             const uint8_t handshake_hash[32], uint8_t out[12]);

/* ---- TLS 1.3 traffic keys and KeyUpdate (RFC 8446 section 7.1 - 7.3) -------
 * TLS_CHACHA20_POLY1305_SHA256 is the one TLS 1.3 suite the library speaks, so
 * the hash is SHA-256 throughout.  The first three calls are CPU only, as the
 * TLS 1.2 schedule above; the early and handshake secrets' Derive-Secret chains
 * are the caller's to compose from the first two. */

/* RFC 5869 section 2.2 with SHA-256.  salt NULL / 0 bytes = 32 zero bytes; salt_len <= 64
 * (the HMAC key bound of sg_hmac_sha256), else SG_E_ARG. */
int sg_hkdf_extract(const uint8_t* salt, size_t salt_len, const uint8_t* ikm, size_t ikm_len, uint8_t prk[32]);

/* RFC 8446 section 7.1: HKDF-Expand(secret, HkdfLabel, out_len) with
 * HkdfLabel = be16(out_len) || u8(6 + label_len) || "tls13 " || label || u8(context_len) || context.
 * label_len <= 249, context_len <= 255, out_len <= 255 * 32; out_len 0 writes nothing. */
int sg_hkdf_expand_label(const uint8_t secret[32], const char* label, size_t label_len,
                         const uint8_t* context, size_t context_len, uint8_t* out, size_t out_len);

/* RFC 8446 section 7.3 / 7.2 for `count` connections, host memory, threads >= 1:
 *   update != 0:  secrets[i] <- Expand-Label(secrets[i], "traffic upd", "", 32)   (in place, first)
 *   keys[i]  = Expand-Label(secrets[i], "key", "", 32)      [count][32], may be NULL
 *   ivs[i]   = Expand-Label(secrets[i], "iv",  "", 12)      [count][12], may be NULL
 * count == 0 is SG_OK; a call that would do nothing (no keys, no ivs, no update) is SG_E_ARG. */
int sg_tls13_traffic_keys(uint32_t count, uint8_t* secrets, uint8_t* keys, uint8_t* ivs, int update, int threads);

/* QUIC packet protection keys (RFC 9001 section 5.1, 6.1) for `count` connections, with
 * the shape and rules of the call above:
 *   update != 0:  secrets[i] <- Expand-Label(secrets[i], "quic ku", "", 32)   (in place, first)
 *   keys[i] = Expand-Label(secrets[i], "quic key", "", 32)   [count][32], may be NULL
 *   ivs[i]  = Expand-Label(secrets[i], "quic iv",  "", 12)   [count][12], may be NULL
 *   hps[i]  = Expand-Label(secrets[i], "quic hp",  "", 32)   [count][32], may be NULL
 * The header protection key does not change at a key update (section 6): a caller that
 * updates passes hps == NULL.  count == 0 is SG_OK; a call that would do nothing is
 * SG_E_ARG.  Host memory; the tables feed sg_quic_batch. */
int sg_quic_packet_keys(uint32_t count, uint8_t* secrets, uint8_t* keys, uint8_t* ivs, uint8_t* hps, int update,
                        int threads);

/* DTLS 1.3 record protection keys (RFC 9147 section 5.9, 4.2.3) for `count` traffic secrets,
 * with the shape and rules of the call above.  Expand-Label is RFC 8446's with the label
 * prefix "dtls13" (no space) where TLS 1.3 has "tls13 ":
 *   update != 0:  secrets[i] <- Expand-Label(secrets[i], "traffic upd", "", 32)   (in place, first)
 *   keys[i]    = Expand-Label(secrets[i], "key", "", 32)   [count][32], may be NULL
 *   ivs[i]     = Expand-Label(secrets[i], "iv",  "", 12)   [count][12], may be NULL
 *   sn_keys[i] = Expand-Label(secrets[i], "sn",  "", 32)   [count][32], may be NULL
 * count == 0 is SG_OK; a call that would do nothing is SG_E_ARG.  Host memory; the tables
 * feed sg_dtls13_batch (under SG_DTLS13_EPOCH_ROWS one secret per connection and epoch). */
int sg_dtls13_record_keys(uint32_t count, uint8_t* secrets, uint8_t* keys, uint8_t* ivs, uint8_t* sn_keys, int update,
                          int threads);

/* The same on the device: one launch turns a device table of traffic secrets
 * into the keys / ivs tables of the batch calls, in place in HBM (sg_hkdf.hip:
 * one lane per row).  Per row exactly the host call.  The selected rows of keys
 * and ivs are written, 32 and 12 bytes each, and under UPDATE the same rows of
 * secrets; no other byte of any table is.  Ordered on its stream like a batch
 * call -- a sg_seal_batch_tls13 enqueued on the same stream right after it sees
 * the new rows -- and capturable: no workspace, no host read-back.
 * SG_E_ARG before any GPU work: NULL k, unknown flags, NULL secrets, a
 * misaligned pointer, keys == ivs == NULL without UPDATE, index == NULL with
 * count > rows.  count == 0 returns SG_OK and launches nothing. */
#define SG_TLS13_KEYS_UPDATE 0x1u   /* ratchet the secret first (KeyUpdate), in place */
typedef struct sg_tls13_keys {
    uint32_t        count;    /* rows to derive                                                       */
    uint32_t        flags;    /* 0 or SG_TLS13_KEYS_UPDATE; anything else SG_E_ARG                    */
    uint32_t        rows;     /* rows of every table                                                  */
    uint32_t        _pad;
    const uint32_t* index;    /* device, count row numbers, 4-byte aligned; NULL: rows 0..count-1
                                 (then count <= rows).  An entry >= rows is skipped: nothing is read
                                 or written for it.  A row named twice in an UPDATE call holds an
                                 unspecified generation afterwards (no fault; the caller's to avoid) */
    uint8_t*        secrets;  /* device [rows][32], 4-byte aligned; read, and written under UPDATE    */
    uint8_t*        keys;     /* device [rows][32], 4-byte aligned, or NULL  -> sg_batch.keys         */
    uint8_t*        ivs;      /* device [rows][12], 4-byte aligned, or NULL  -> sg_batch_tls13.ivs    */
    void*           stream;   /* as sg_batch.stream: non-NULL asynchronous, NULL waits                */
} sg_tls13_keys;              /* 56 bytes */
int sg_tls13_traffic_keys_dev(const sg_tls13_keys* k);

/* ---- synthetic workload helpers (bench / tests) ------------------------ */
/* Fills records on the device: byte i of record j =
 * byte (i mod 8) of splitmix64(seed ^ ((j0 + j) << 32) ^ (i / 8)).
 * Records are len bytes each at buf + stride * j.                         */
int sg_fill_records(uint8_t* buf, uint64_t stride, uint32_t len, uint32_t count,
                    uint64_t seed, uint64_t j0, void* stream);
/* Byte-compares a[j] and b[j] (len bytes at stride_a / stride_b); adds the
 * number of mismatching records to *mismatches (device uint64).            */
int sg_compare_records(const uint8_t* a, uint64_t stride_a, const uint8_t* b,
                       uint64_t stride_b, uint32_t len, uint32_t count,
                       unsigned long long* mismatches, void* stream);

/* ---- diagnostics -------------------------------------------------------- */
const char* sg_last_error(void);       /* thread-local message of the last failure */
const char* sg_build_info(void);       /* arch + kernel configuration string       */
const char* sg_source_hash(void);      /* hash of the sources the library was built
                                          from (16 hex digits; suruga_amd/_build.py) */
/* Kernel timing with HIP events recorded on the launch stream.  While timing
 * is enabled every batch call brackets its keying kernel and its seal/open
 * kernel with events; sg_timing_read synchronises on them and returns the
 * average duration (ms) per launch of each kind and the launch counts.
 * sg_set_timing(1) resets the accumulators; sg_set_timing(0) stops them. */
int sg_set_timing(int enable);
int sg_timing_read(double* seal_ms, double* open_ms, double* keying_ms,
                   uint32_t* n_seal, uint32_t* n_open, uint32_t* n_keying);

/* Kernel form for uniform batches of full 16 KiB records (n = 2^14, the
 * size TlsWriter::write_data gives every record but a stream's tail; C1):
 * 1 = the wave-per-record kernel (one wave per record, lock-step ChaCha20
 * rounds, Poly1305 on the matrix cores fed from the ciphertext registers),
 * 0 = the size-class kernel used for every other batch.  Both are bit-exact;
 * the switch exists for A/B measurement and for tests that cover both.
 * Initial value: environment SG_LOCKSTEP ("0"/"1"), else 1.  Returns the
 * previous setting; a negative argument only queries. */
int sg_set_lockstep(int enable);

/* Kernel form for the small records of mixed TLS batches (64 B .. 4 KiB, a
 * multiple of 64 bytes, 16-byte aligned; C2): 1 = the packed kernel (the
 * 64-byte blocks of runs of 128 records of the packed list laid end to end
 * over the lanes of a 512-thread workgroup, keyed in the same kernel), 0 = the
 * size-class kernels.  Both are
 * bit-exact; A/B and test switch like sg_set_lockstep.  Initial value:
 * environment SG_PACK ("0"/"1"), else 1.  Returns the previous setting; a
 * negative argument only queries. */
int sg_set_packed(int enable);

/* Route of the padded TLS 1.3 records of 4-16 KiB in mixed batches
 * (sg_seal_batch_tls13_ex, sg_open_batch_tls13): 1 = a record whose inner length
 * is a multiple of 64 in 4160..2^14 and whose input and output addresses are
 * 16-byte aligned runs on the wave-per-record buckets J = 2..4 in their TLS 1.3
 * form, under the conditions of the RFC call's buckets (sg_set_lockstep on, not
 * under capture, per-record arrays 4-byte aligned); 0 = on the size classes.
 * Both are bit-exact.  Initial value: environment SG_TLS13_BUCKETS ("0"/"1"),
 * else 0 -- unlike the two switches above this one is off unless asked for.
 * Returns the previous setting; a negative argument only queries. */
int sg_set_tls13_buckets(int enable);

/* Where the records of a mixed batch went (host-only bookkeeping of the
 * dispatcher: no device work, no wait, no kernel argument).  The counts are
 * the list populations the call read back anyway; they serve the draft calls
 * and the RFC 8439 ones alike.  Thread-local: the calling thread's last
 * sg_seal_batch / sg_open_batch / sg_*_batch_rfc8439 call. */
typedef struct sg_batch_routes {
    uint32_t known;      /* 1: this thread's last sg_*_batch* call classified its records and
                            read the populations back (a mixed batch, not under capture);
                            0: the other fields are not meaningful */
    uint32_t classes;    /* records run by the size-class kernels */
    uint32_t bucket[3];  /* wave-per-record buckets J = 2, 3, 4 */
    uint32_t packed;     /* packed kernel */
    uint32_t skipped;    /* longer than max_len */
    uint32_t _pad;
} sg_batch_routes;
int sg_last_batch_routes(sg_batch_routes* out);   /* SG_OK, or SG_E_ARG for NULL */

#ifdef __cplusplus
}
#endif
#endif /* SURUGA_GPU_H */
