// sg_keysched.cpp -- TLS 1.2 key schedule on the host (SURVEY.md section 8f,
// rank 4): SHA-256, HMAC-SHA256 and the P_SHA256 PRF of suruga
// (src/crypto/sha2.rs, src/cipher/prf.rs) and the client's derivation of the
// per-direction AEAD keys (src/client.rs:130-163) and Finished verify data
// (client.rs:184-225).  It produces the key tables that sg_seal_batch /
// sg_open_batch consume; it is a few microseconds of CPU per connection, so
// it stays on the CPU as the survey ranks it, threaded over connections.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/suruga_gpu.h"
#include "sg_err.h"  // host only: no HIP (tests/cpp/test_host_san.cpp builds it with g++ under sanitizers)
#include "sg_hkdf.h"

namespace sg {
namespace {

// ---- SHA-256 (FIPS 180-4; the algorithm of crypto/sha2.rs:18-116) ----------
// The compression function is sg_hkdf.h's, which the device key table kernel shares.
struct Sha256 {
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                     0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint8_t blk[64];
    size_t fill = 0;
    uint64_t total = 0;

    void compress(const uint8_t* p) {
        uint32_t w[16];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        hkdf::compress(h, w);
    }
    void update(const uint8_t* p, size_t n) {
        total += n;
        while (n) {
            const size_t k = std::min(n, (size_t)64 - fill);
            std::memcpy(blk + fill, p, k);
            fill += k;
            p += k;
            n -= k;
            if (fill == 64) {
                compress(blk);
                fill = 0;
            }
        }
    }
    void finish(uint8_t out[32]) {
        const uint64_t bits = total * 8;
        const uint8_t pad = 0x80;
        update(&pad, 1);
        const uint8_t zero[64] = {0};
        update(zero, (fill <= 56 ? 56 : 120) - fill);
        uint8_t len[8];
        for (int i = 0; i < 8; ++i) len[i] = (uint8_t)(bits >> (56 - 8 * i));
        update(len, 8);
        for (int i = 0; i < 8; ++i) {
            out[4 * i] = (uint8_t)(h[i] >> 24);
            out[4 * i + 1] = (uint8_t)(h[i] >> 16);
            out[4 * i + 2] = (uint8_t)(h[i] >> 8);
            out[4 * i + 3] = (uint8_t)h[i];
        }
    }
};

// prf.rs:8-29: ipad/opad with the key XORed in; keys longer than the block
// are unimplemented!() in the reference.
void hmac(const uint8_t* key, size_t key_len, const uint8_t* m1, size_t n1, const uint8_t* m2, size_t n2,
          uint8_t out[32]) {
    uint8_t ipad[64], opad[64];
    std::memset(ipad, 0x36, 64);
    std::memset(opad, 0x5c, 64);
    for (size_t i = 0; i < key_len; ++i) {
        ipad[i] ^= key[i];
        opad[i] ^= key[i];
    }
    uint8_t inner[32];
    Sha256 hi;
    hi.update(ipad, 64);
    hi.update(m1, n1);
    if (n2) hi.update(m2, n2);
    hi.finish(inner);
    Sha256 ho;
    ho.update(opad, 64);
    ho.update(inner, 32);
    ho.finish(out);
}

}  // namespace

// prf.rs:31-89: A(1) = HMAC(secret, seed); block i = HMAC(secret, A(i) || seed);
// A(i+1) = HMAC(secret, A(i)); get_bytes hands out the stream in order, keeping
// the unused tail of the last block.
struct Prf {
    std::vector<uint8_t> secret, seed;
    uint8_t a[32];
    uint8_t buf[32];
    size_t buf_len = 0, buf_off = 0;

    Prf(const uint8_t* s, size_t sl, const uint8_t* sd, size_t sdl) : secret(s, s + sl), seed(sd, sd + sdl) {
        hmac(secret.data(), secret.size(), seed.data(), seed.size(), nullptr, 0, a);
    }
    void next_block(uint8_t out[32]) {
        hmac(secret.data(), secret.size(), a, 32, seed.data(), seed.size(), out);
        uint8_t na[32];
        hmac(secret.data(), secret.size(), a, 32, nullptr, 0, na);
        std::memcpy(a, na, 32);
    }
    void get_bytes(uint8_t* out, size_t n) {
        while (n) {
            if (buf_off == buf_len) {
                next_block(buf);
                buf_len = 32;
                buf_off = 0;
            }
            const size_t k = std::min(n, buf_len - buf_off);
            std::memcpy(out, buf + buf_off, k);
            buf_off += k;
            out += k;
            n -= k;
        }
    }
};

namespace {
constexpr size_t kMaxHmacKey = 64;

// cwiv / swiv (both or neither): the 12-byte write IVs that follow the keys in
// the key block (RFC 5246 section 6.3 with no MAC keys, RFC 7905 section 2)
void derive_one(const uint8_t* pm, size_t pm_len, const uint8_t* cr, const uint8_t* sr, uint8_t* ms_out,
                uint8_t* cwk, uint8_t* swk, uint8_t* cwiv = nullptr, uint8_t* swiv = nullptr) {
    // client.rs:130-137: master_secret = PRF(pre_master, "master secret" || client_random || server_random)[..48]
    uint8_t seed[13 + 64];
    std::memcpy(seed, "master secret", 13);
    std::memcpy(seed + 13, cr, 32);
    std::memcpy(seed + 45, sr, 32);
    uint8_t ms[48];
    Prf(pm, pm_len, seed, 77).get_bytes(ms, 48);
    // client.rs:142-160: key block = PRF(master, "key expansion" || server_random || client_random);
    // client write key first, then the read (server write) key; no MAC keys, no IVs (AEAD, fixed_iv_len 0)
    std::memcpy(seed, "key expansion", 13);
    std::memcpy(seed + 13, sr, 32);
    std::memcpy(seed + 45, cr, 32);
    Prf kb(ms, 48, seed, 77);
    kb.get_bytes(cwk, SG_KEY_LEN);
    kb.get_bytes(swk, SG_KEY_LEN);
    if (cwiv) {
        kb.get_bytes(cwiv, 12);
        kb.get_bytes(swiv, 12);
    }
    if (ms_out) std::memcpy(ms_out, ms, 48);
}
}  // namespace
}  // namespace sg

using sg::fail;

extern "C" {

void sg_sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
    sg::Sha256 h;
    if (len) h.update(msg, len);
    h.finish(out);
}

int sg_hmac_sha256(const uint8_t* key, size_t key_len, const uint8_t* msg, size_t len, uint8_t out[32]) {
    if (key_len > sg::kMaxHmacKey) return fail(SG_E_ARG, "HMAC key longer than 64 bytes (unimplemented in prf.rs:11-14)%s");
    if ((key_len && !key) || (len && !msg) || !out) return fail(SG_E_ARG, "NULL argument%s");
    sg::hmac(key, key_len, msg, len, nullptr, 0, out);
    return SG_OK;
}

sg_prf* sg_prf_new(const uint8_t* secret, size_t secret_len, const uint8_t* seed, size_t seed_len) {
    if (secret_len > sg::kMaxHmacKey || (secret_len && !secret) || (seed_len && !seed)) {
        fail(SG_E_ARG, "bad PRF secret/seed%s");
        return nullptr;
    }
    return reinterpret_cast<sg_prf*>(new sg::Prf(secret, secret_len, seed, seed_len));
}

int sg_prf_get_bytes(sg_prf* prf, uint8_t* out, size_t n) {
    if (!prf || (n && !out)) return fail(SG_E_ARG, "NULL argument%s");
    reinterpret_cast<sg::Prf*>(prf)->get_bytes(out, n);
    return SG_OK;
}

void sg_prf_free(sg_prf* prf) { delete reinterpret_cast<sg::Prf*>(prf); }

static int derive_keys(uint32_t count, const uint8_t* pre_master, size_t pm_len, size_t pm_stride,
                       const uint8_t* client_random, const uint8_t* server_random, uint8_t* master_secret,
                       uint8_t* client_write_keys, uint8_t* server_write_keys, uint8_t* client_write_ivs,
                       uint8_t* server_write_ivs, int threads) {
    if (!count) return SG_OK;
    if (!pre_master || !client_random || !server_random || !client_write_keys || !server_write_keys)
        return fail(SG_E_ARG, "NULL argument%s");
    if (pm_len > sg::kMaxHmacKey || pm_stride < pm_len) return fail(SG_E_ARG, "bad pre-master length/stride%s");
    const uint32_t nt = (uint32_t)std::max(1, std::min<int>(threads, (int)count));
    auto work = [&](uint32_t t) {
        for (uint32_t i = t; i < count; i += nt)
            sg::derive_one(pre_master + (size_t)pm_stride * i, pm_len, client_random + 32ull * i,
                           server_random + 32ull * i, master_secret ? master_secret + 48ull * i : nullptr,
                           client_write_keys + 32ull * i, server_write_keys + 32ull * i,
                           client_write_ivs ? client_write_ivs + 12ull * i : nullptr,
                           client_write_ivs ? server_write_ivs + 12ull * i : nullptr);
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < nt; ++t) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    return SG_OK;
}

int sg_derive_keys(uint32_t count, const uint8_t* pre_master, size_t pm_len, size_t pm_stride,
                   const uint8_t* client_random, const uint8_t* server_random, uint8_t* master_secret,
                   uint8_t* client_write_keys, uint8_t* server_write_keys, int threads) {
    return derive_keys(count, pre_master, pm_len, pm_stride, client_random, server_random, master_secret,
                       client_write_keys, server_write_keys, nullptr, nullptr, threads);
}

int sg_derive_keys_ivs(uint32_t count, const uint8_t* pre_master, size_t pm_len, size_t pm_stride,
                       const uint8_t* client_random, const uint8_t* server_random, uint8_t* master_secret,
                       uint8_t* client_write_keys, uint8_t* server_write_keys, uint8_t* client_write_ivs,
                       uint8_t* server_write_ivs, int threads) {
    if (count && (!client_write_ivs || !server_write_ivs)) return fail(SG_E_ARG, "NULL argument%s");
    return derive_keys(count, pre_master, pm_len, pm_stride, client_random, server_random, master_secret,
                       client_write_keys, server_write_keys, client_write_ivs, server_write_ivs, threads);
}

int sg_finished_verify_data(const uint8_t master_secret[48], int server, const uint8_t handshake_hash[32],
                            uint8_t out[12]) {
    if (!master_secret || !handshake_hash || !out) return fail(SG_E_ARG, "NULL argument%s");
    // client.rs:184-192 / 213-221: PRF(master, "client finished"|"server finished" || sha256(msgs))[..12]
    uint8_t seed[15 + 32];
    std::memcpy(seed, server ? "server finished" : "client finished", 15);
    std::memcpy(seed + 15, handshake_hash, 32);
    sg::Prf(master_secret, 48, seed, sizeof seed).get_bytes(out, 12);
    return SG_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// TLS 1.3: HKDF (RFC 5869) with SHA-256, HKDF-Expand-Label (RFC 8446 section
// 7.1) and the traffic keys of section 7.3 with the KeyUpdate ratchet of 7.2.
// The label bytes and the per-connection derivation are sg_hkdf.h's, shared
// with the device form (sg_hkdf.hip).
// ---------------------------------------------------------------------------
namespace sg {
namespace {

// HKDF-Expand, the general one: T(i) = HMAC(prk, T(i - 1) || info || i), i = 1 .. ceil(n / 32)
void hkdf_expand(const uint8_t prk[32], const uint8_t* info, size_t info_len, uint8_t* out, size_t n) {
    uint8_t pad[64];
    std::memset(pad, 0x36, 64);
    for (int i = 0; i < 32; ++i) pad[i] ^= prk[i];
    Sha256 inner0;
    inner0.update(pad, 64);
    std::memset(pad, 0x5c, 64);
    for (int i = 0; i < 32; ++i) pad[i] ^= prk[i];
    Sha256 outer0;
    outer0.update(pad, 64);
    uint8_t t[32];
    for (size_t done = 0, i = 1; done < n; done += 32, ++i) {
        Sha256 hi = inner0;
        if (i > 1) hi.update(t, 32);
        if (info_len) hi.update(info, info_len);
        const uint8_t ctr = (uint8_t)i;
        hi.update(&ctr, 1);
        hi.finish(t);
        Sha256 ho = outer0;
        ho.update(t, 32);
        ho.finish(t);
        std::memcpy(out + done, t, std::min<size_t>(32, n - done));
    }
}

inline void load_be(const uint8_t* p, uint32_t* w, int words) {
    for (int i = 0; i < words; ++i)
        w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
}
inline void store_be(const uint32_t* w, uint8_t* p, int words) {
    for (int i = 0; i < words; ++i) {
        p[4 * i] = (uint8_t)(w[i] >> 24);
        p[4 * i + 1] = (uint8_t)(w[i] >> 16);
        p[4 * i + 2] = (uint8_t)(w[i] >> 8);
        p[4 * i + 3] = (uint8_t)w[i];
    }
}

void traffic_one(uint8_t* secret, uint8_t* key, uint8_t* iv, bool update) {
    uint32_t s[8], k[8], v[8];
    load_be(secret, s, 8);
    hkdf::traffic_row(s, update, key != nullptr, iv != nullptr, k, v);
    if (update) store_be(s, secret, 8);
    if (key) store_be(k, key, 8);
    if (iv) store_be(v, iv, 3);
}

}  // namespace
}  // namespace sg

extern "C" {

int sg_hkdf_extract(const uint8_t* salt, size_t salt_len, const uint8_t* ikm, size_t ikm_len, uint8_t prk[32]) {
    if (salt_len > sg::kMaxHmacKey) return fail(SG_E_ARG, "HKDF salt longer than 64 bytes (the HMAC key bound)%s");
    if ((salt_len && !salt) || (ikm_len && !ikm) || !prk) return fail(SG_E_ARG, "NULL argument%s");
    const uint8_t zeros[32] = {0};  // RFC 5869 section 2.2: no salt = HashLen zeros
    sg::hmac(salt_len ? salt : zeros, salt_len ? salt_len : 32, ikm, ikm_len, nullptr, 0, prk);
    return SG_OK;
}

int sg_hkdf_expand_label(const uint8_t secret[32], const char* label, size_t label_len, const uint8_t* context,
                         size_t context_len, uint8_t* out, size_t out_len) {
    if (label_len > sg::hkdf::kMaxLabel) return fail(SG_E_ARG, "HKDF label longer than 249 bytes%s");
    if (context_len > sg::hkdf::kMaxContext) return fail(SG_E_ARG, "HKDF context longer than 255 bytes%s");
    if (out_len > sg::hkdf::kMaxOut) return fail(SG_E_ARG, "HKDF output longer than 255 * 32 bytes%s");
    if (!secret || (label_len && !label) || (context_len && !context) || (out_len && !out))
        return fail(SG_E_ARG, "NULL argument%s");
    if (!out_len) return SG_OK;
    uint8_t info[sg::hkdf::kMaxInfo];
    const size_t n = sg::hkdf::hkdf_label(info, out_len, label, label_len, context, context_len);
    sg::hkdf_expand(secret, info, n, out, out_len);
    return SG_OK;
}

int sg_tls13_traffic_keys(uint32_t count, uint8_t* secrets, uint8_t* keys, uint8_t* ivs, int update, int threads) {
    if (!count) return SG_OK;
    if (!secrets) return fail(SG_E_ARG, "NULL argument%s");
    if (!keys && !ivs && !update) return fail(SG_E_ARG, "nothing to do: no keys, no ivs and no update%s");
    const uint32_t nt = (uint32_t)std::max(1, std::min<int>(threads, (int)std::min<uint32_t>(count, 1u << 16)));
    auto work = [&](uint32_t t) {
        for (uint32_t i = t; i < count; i += nt)
            sg::traffic_one(secrets + 32ull * i, keys ? keys + 32ull * i : nullptr, ivs ? ivs + 12ull * i : nullptr,
                            update != 0);
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < nt; ++t) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    return SG_OK;
}

int sg_quic_packet_keys(uint32_t count, uint8_t* secrets, uint8_t* keys, uint8_t* ivs, uint8_t* hps, int update,
                        int threads) {
    if (!count) return SG_OK;
    if (!secrets) return fail(SG_E_ARG, "NULL argument%s");
    if (!keys && !ivs && !hps && !update) return fail(SG_E_ARG, "nothing to do: no keys, no ivs, no hps and no update%s");
    const uint32_t nt = (uint32_t)std::max(1, std::min<int>(threads, (int)std::min<uint32_t>(count, 1u << 16)));
    auto work = [&](uint32_t t) {
        for (uint32_t i = t; i < count; i += nt) {
            uint8_t* s = secrets + 32ull * i;
            if (update) {  // RFC 9001 section 6.1: the next generation's secret
                uint8_t next[32];
                (void)sg_hkdf_expand_label(s, "quic ku", 7, nullptr, 0, next, 32);
                std::memcpy(s, next, 32);
            }
            if (keys) (void)sg_hkdf_expand_label(s, "quic key", 8, nullptr, 0, keys + 32ull * i, 32);
            if (ivs) (void)sg_hkdf_expand_label(s, "quic iv", 7, nullptr, 0, ivs + 12ull * i, 12);
            if (hps) (void)sg_hkdf_expand_label(s, "quic hp", 7, nullptr, 0, hps + 32ull * i, 32);
        }
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < nt; ++t) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    return SG_OK;
}

int sg_dtls13_record_keys(uint32_t count, uint8_t* secrets, uint8_t* keys, uint8_t* ivs, uint8_t* sn_keys, int update,
                          int threads) {
    if (!count) return SG_OK;
    if (!secrets) return fail(SG_E_ARG, "NULL argument%s");
    if (!keys && !ivs && !sn_keys && !update) return fail(SG_E_ARG, "nothing to do: no keys, no ivs, no sn_keys and no update%s");
    // RFC 9147 section 5.9: RFC 8446's Expand-Label with the prefix "dtls13"
    auto expand = [](const uint8_t* s, const char* label, size_t label_len, uint8_t* out, size_t out_len) {
        uint8_t info[sg::hkdf::kMaxInfo];
        const size_t n = sg::hkdf::hkdf_label(info, out_len, label, label_len, nullptr, 0, sg::hkdf::kPrefixDtls13);
        sg::hkdf_expand(s, info, n, out, out_len);
    };
    const uint32_t nt = (uint32_t)std::max(1, std::min<int>(threads, (int)std::min<uint32_t>(count, 1u << 16)));
    auto work = [&](uint32_t t) {
        for (uint32_t i = t; i < count; i += nt) {
            uint8_t* s = secrets + 32ull * i;
            if (update) {  // RFC 8446 section 7.2: the next generation's secret
                uint8_t next[32];
                expand(s, "traffic upd", 11, next, 32);
                std::memcpy(s, next, 32);
            }
            if (keys) expand(s, "key", 3, keys + 32ull * i, 32);
            if (ivs) expand(s, "iv", 2, ivs + 12ull * i, 12);
            if (sn_keys) expand(s, "sn", 2, sn_keys + 32ull * i, 32);
        }
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < nt; ++t) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    return SG_OK;
}

}  // extern "C"
