// test_wire13_san.cpp -- the record layer's host-only code of the RFC 7905 and
// TLS 1.3 forms (sg_wire.h / sg_wire.cpp) as a stand-alone program: the plan
// arithmetic per record form, the explicit-mode nonces, the chunk shape and the
// TLS 1.3 parser over truncated and hostile headers.  Every wire buffer is
// heap-allocated at its exact size, so a parser that reads one byte past it, or
// an offset that overflows, is a sanitizer report.
// tests/test_wire13_sanitizers.py builds it with g++ -fsanitize=address,undefined
// and runs it directly.  No GPU, no HIP header.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/suruga_gpu.h"
#include "../../suruga_amd/csrc/sg_err.h"
#include "../../suruga_amd/csrc/sg_wire.h"

#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) {                                                            \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

using sg::RecordForm;

// sg_capi.cpp owns the thread-local message; this program only needs the code
int sg::fail(int code, const char*, const char*) { return code; }

namespace {

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// an exact-size heap copy: reads past the end are reports
std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size());
    return p;
}

void put_rec(std::vector<uint8_t>& w, uint8_t type, uint8_t major, uint8_t minor, uint32_t flen, size_t have) {
    const uint8_t h[5] = {type, major, minor, (uint8_t)(flen >> 8), (uint8_t)flen};
    w.insert(w.end(), h, h + 5);
    w.insert(w.end(), have, (uint8_t)0xA5);
}

void test_plan_per_form() {
    const RecordForm forms[] = {RecordForm::kDraft, RecordForm::kRfc8439, RecordForm::kTls13};
    const size_t lens[] = {0, 1, 16383, 16384, 16385, 3 * 16384, 3 * 16384 + 7, (size_t)257 * 16384 + 3};
    for (RecordForm f : forms) {
        const uint32_t extra = f == RecordForm::kTls13 ? 17u : 16u;
        CHECK(sg::frag_extra(f) == extra);
        CHECK(sg::wire_rec(f) == 5u + 16384u + extra);
        CHECK(sg::max_fragment(f) == (f == RecordForm::kTls13 ? 16384u + 256u : 16384u + 2048u));
        CHECK(sg::frag_capacity(f, 0) == 0 && sg::frag_capacity(f, 16) == 0 && sg::frag_capacity(f, extra) == 0);
        CHECK(sg::frag_capacity(f, extra + 9) == 9);
        for (size_t len : lens) {
            const sg::WritePlan plan(len, f);
            CHECK(plan.nrec == (len + 16383) / 16384);
            size_t sum = 0;
            for (uint64_t r = 0; r < plan.nrec; ++r) {
                CHECK(plan.frag_len(r) == plan.rec_len(r) + extra);
                CHECK(plan.wire_off(r) == r * (5u + 16384u + extra));
                sum += plan.rec_len(r);
            }
            CHECK(sum == len);
            CHECK(plan.wire_need() == len + plan.nrec * (5u + extra));
            if (f == RecordForm::kTls13) CHECK(plan.wire_need() == sg_wire_bound_tls13(len));
            else CHECK(plan.wire_need() == sg_wire_bound(len));
        }
    }
    CHECK(sg_wire_bound_tls13(0) == 0 && sg_wire_bound_tls13(1) == 23 && sg_wire_bound_tls13(16384) == 16406);
    // the draft's plan is the default argument's
    CHECK(sg::WritePlan(40000).wire_need() == sg::WritePlan(40000, RecordForm::kDraft).wire_need());
}

void test_explicit_nonces() {
    std::vector<uint8_t> meta((size_t)sg::kChunk * sg::kMetaBytesMax, 0xEE);
    uint8_t iv[12];
    for (int i = 0; i < 12; ++i) iv[i] = (uint8_t)(0x10 + i);
    const sg::WireRec R = {5, 100 + 16, 22, 3, 1};
    const uint64_t seq = 0x0102030405060708ull;
    sg::put_explicit_meta(meta.data(), sg::kChunk - 1, seq, R, RecordForm::kRfc8439, iv);
    const uint8_t* n = meta.data() + 12 * (sg::kChunk - 1);
    for (int i = 0; i < 4; ++i) CHECK(n[i] == iv[i]);
    for (int i = 0; i < 8; ++i) CHECK(n[4 + i] == (uint8_t)(iv[4 + i] ^ (uint8_t)(i + 1)));
    const uint8_t* ad = meta.data() + 12 * sg::kChunk + 13 * (sg::kChunk - 1);
    for (int i = 0; i < 8; ++i) CHECK(ad[i] == (uint8_t)(i + 1));
    CHECK(ad[8] == 22 && ad[9] == 3 && ad[10] == 1 && ad[11] == 0 && ad[12] == 100);
    CHECK(ad + 13 == meta.data() + meta.size());  // the last record's AD ends the block
    // the draft's layout is untouched: 8-byte nonces, then the ads
    std::vector<uint8_t> d((size_t)sg::kChunk * sg::kMetaBytes, 0xEE);
    sg::put_explicit_meta(d.data(), sg::kChunk - 1, seq, R);
    CHECK(d[8 * (sg::kChunk - 1)] == 1 && d[8 * sg::kChunk + 13 * (sg::kChunk - 1) + 12] == 100);
}

struct Parsed {
    std::vector<sg::WireRec> recs;
    int32_t error;
};
Parsed parse13(const std::vector<uint8_t>& w, size_t max_records = 1u << 20) {
    auto p = exact(w);
    Parsed out;
    out.error = sg::parse_wire_tls13(p.get(), w.size(), max_records, out.recs);
    // the C entry point agrees and stays inside its arrays
    std::vector<sg_wire_record> recs(out.recs.size() + 1);
    size_t count = 99;
    int32_t error = 99;
    CHECK(sg_parse_records_tls13(p.get(), w.size(), recs.size(), recs.data(), &count, &error) == SG_OK);
    if (max_records > out.recs.size()) CHECK(count == out.recs.size() && error == out.error);
    for (size_t i = 0; i < out.recs.size(); ++i) {
        CHECK(recs[i].offset == out.recs[i].off && recs[i].frag_len == out.recs[i].flen);
        CHECK(out.recs[i].off + out.recs[i].flen <= w.size());
        CHECK(out.recs[i].flen >= 16 && out.recs[i].flen <= 16384 + 256 && out.recs[i].type == 23);
    }
    return out;
}

void test_parser_checks_in_order() {
    for (uint8_t ty : {(uint8_t)20, (uint8_t)21, (uint8_t)22, (uint8_t)24, (uint8_t)0, (uint8_t)255}) {
        std::vector<uint8_t> w;
        put_rec(w, 23, 3, 3, 40, 40);
        put_rec(w, ty, 3, 3, 0xFFFF, 0);  // the type comes first, whatever the length says
        const Parsed p = parse13(w);
        CHECK(p.error == SG_E_UNEXPECTED_MESSAGE && p.recs.size() == 1);
    }
    const struct {
        uint32_t flen;
        int32_t error;
    } lim[] = {{15, SG_E_SHORT}, {16, SG_OK}, {17, SG_OK}, {16384 + 256, SG_OK}, {16384 + 257, SG_E_RECORD_OVERFLOW},
               {0, SG_E_SHORT}, {0xFFFF, SG_E_RECORD_OVERFLOW}};
    for (const auto& l : lim) {
        std::vector<uint8_t> w;
        put_rec(w, 23, 3, 3, l.flen, l.error == SG_E_RECORD_OVERFLOW ? 0 : l.flen);
        const Parsed p = parse13(w);
        CHECK(p.error == l.error && p.recs.size() == (l.error == SG_OK ? 1u : 0u));
    }
    {  // version bytes are recorded, not checked
        std::vector<uint8_t> w;
        put_rec(w, 23, 9, 7, 20, 20);
        const Parsed p = parse13(w);
        CHECK(p.error == SG_OK && p.recs.size() == 1 && p.recs[0].major == 9 && p.recs[0].minor == 7);
    }
}

void test_parser_truncation() {
    std::vector<uint8_t> whole;
    put_rec(whole, 23, 3, 3, 50, 50);
    put_rec(whole, 23, 3, 3, 16384 + 256, 16384 + 256);
    put_rec(whole, 23, 3, 3, 16, 16);
    for (size_t n = 0; n <= whole.size(); n += (n < 70 || n + 70 > whole.size()) ? 1 : 997) {
        const std::vector<uint8_t> w(whole.begin(), whole.begin() + n);
        const Parsed p = parse13(w);
        CHECK(p.error == SG_OK);
        const size_t want = n >= whole.size() ? 3 : (n >= 55 + 5 + 16384 + 256 ? 2 : (n >= 55 ? 1 : 0));
        CHECK(p.recs.size() == want);
    }
    CHECK(parse13(whole, 2).recs.size() == 2);
    CHECK(parse13(whole, 0).recs.empty());
}

void test_parser_hostile_corpus() {
    for (int it = 0; it < 4000; ++it) {
        std::vector<uint8_t> w;
        const uint32_t nrec = rnd() % 6;
        for (uint32_t r = 0; r < nrec; ++r) {
            const uint32_t pick = rnd() % 8;
            const uint8_t ty = pick == 0 ? (uint8_t)rnd() : 23;
            uint32_t flen = pick == 1 ? rnd() & 0xFFFF : (pick == 2 ? rnd() % 32 : 16 + rnd() % 600);
            const size_t have = pick == 3 ? rnd() % (flen + 1) : flen;
            put_rec(w, ty, (uint8_t)rnd(), (uint8_t)rnd(), flen, have);
        }
        if (rnd() % 4 == 0 && !w.empty()) w.resize(rnd() % w.size());
        const Parsed p = parse13(w);
        CHECK(p.error == SG_OK || p.error == SG_E_UNEXPECTED_MESSAGE || p.error == SG_E_RECORD_OVERFLOW ||
              p.error == SG_E_SHORT);
        if (!p.recs.empty()) {
            // the shape of the parsed records as a chunk, capacity prefix included
            const uint32_t k = (uint32_t)p.recs.size();
            std::unique_ptr<sg::ChunkShape> sh(new sg::ChunkShape);
            sg::chunk_shape(p.recs.data(), k, sh.get(), RecordForm::kTls13);
            uint32_t sum = 0;
            for (uint32_t i = 0; i < k; ++i) sum += p.recs[i].flen >= 17 ? p.recs[i].flen - 17 : 0;
            CHECK(sh->pre[0] == 0 && sh->pre[k] == sum && sh->flen == p.recs[0].flen);
        }
    }
}

}  // namespace

int main() {
    test_plan_per_form();
    test_explicit_nonces();
    test_parser_checks_in_order();
    test_parser_truncation();
    test_parser_hostile_corpus();
    std::printf("wire13 sanitizer checks passed\n");
    return 0;
}
