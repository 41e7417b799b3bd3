// check_request_host.cpp -- the shared host functions of quantize_amd/csrc/qe_request.hpp on their own, under the sanitizers.
// Host code only, no GPU and no HIP header.  From the repository root:
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g -o tools/check_request_host tools/check_request_host.cpp && tools/check_request_host
//
// Prints "check_request_host: ok" and exits 0, or names the first failing line.
#include "../quantize_amd/csrc/qe_request.hpp"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

using namespace qe;

// the stored-code range of every (n_bits, sign): the values of tpack.cu:108-111, written out
static const struct { int n_bits, sign; unsigned offset, mask; float lo, hi; } kRanges[16] = {
    {1, 0, 0u, 0x01u, 0.0f, 1.0f},   {1, 1, 1u, 0x01u, -1.0f, 0.0f},
    {2, 0, 0u, 0x03u, 0.0f, 3.0f},   {2, 1, 2u, 0x03u, -2.0f, 1.0f},
    {3, 0, 0u, 0x07u, 0.0f, 7.0f},   {3, 1, 4u, 0x07u, -4.0f, 3.0f},
    {4, 0, 0u, 0x0fu, 0.0f, 15.0f},  {4, 1, 8u, 0x0fu, -8.0f, 7.0f},
    {5, 0, 0u, 0x1fu, 0.0f, 31.0f},  {5, 1, 16u, 0x1fu, -16.0f, 15.0f},
    {6, 0, 0u, 0x3fu, 0.0f, 63.0f},  {6, 1, 32u, 0x3fu, -32.0f, 31.0f},
    {7, 0, 0u, 0x7fu, 0.0f, 127.0f}, {7, 1, 64u, 0x7fu, -64.0f, 63.0f},
    {8, 0, 0u, 0xffu, 0.0f, 255.0f}, {8, 1, 128u, 0xffu, -128.0f, 127.0f},
};

static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }

int main()
{
    for (const auto &r : kRanges) {
        const CodeRange c = code_range(r.n_bits, r.sign);
        CHECK(c.offset == r.offset && c.mask == r.mask && c.lo == r.lo && c.hi == r.hi);
    }
    CHECK(!bits_ok(0) && bits_ok(1) && bits_ok(8) && !bits_ok(9) && !bits_ok(-1));
    CHECK(one_or_per_channel(1, 8) && one_or_per_channel(8, 8) && !one_or_per_channel(0, 8) && !one_or_per_channel(9, 8));

    // operands: null pointers, then n_bits, then n_param < 1
    float f = 0.0f;
    uint8_t b = 0;
    qe_qparam q{&b, 8, 1, &f, &f, 1};
    CHECK(check_qparam(&q) == QE_OK && check_qparam(nullptr) == QE_ERR_ARG);
    q.n_bits = 9; q.n_param = 0;
    CHECK(check_qparam(&q) == QE_ERR_NBITS && check_operand(&q) == QE_ERR_NBITS);
    q.zero = nullptr;
    CHECK(check_qparam(&q) == QE_ERR_ARG);
    q.zero = &f; q.n_bits = 8;
    CHECK(check_qparam(&q) == QE_ERR_ARG && check_operand(&q) == QE_OK);
    qe_requant rq{&f, &f, 1, -128.0f, 127.0f, 8, 1};
    CHECK(check_requant(&rq) == QE_OK && check_requant(nullptr) == QE_ERR_ARG);
    rq.n_bits = 0; rq.n_param = 0;
    CHECK(check_requant(&rq) == QE_ERR_NBITS);
    rq.scale = nullptr;
    CHECK(check_requant(&rq) == QE_ERR_ARG);
    rq.scale = &f; rq.n_bits = 1;
    CHECK(check_requant(&rq) == QE_ERR_ARG);

    // spans: [0x1000, 0x1010)
    const Span a = span_of(at(0x1000), 16);
    CHECK(a.lo == 0x1000 && a.hi == 0x1010);
    CHECK(!overlaps(a, span_of(at(0x1010), 16)) && !overlaps(span_of(at(0x1010), 16), a));    // touching above
    CHECK(!overlaps(a, span_of(at(0x0ff0), 16)) && !overlaps(span_of(at(0x0ff0), 16), a));    // touching below
    CHECK(overlaps(a, span_of(at(0x100f), 16)) && overlaps(span_of(at(0x100f), 16), a));      // one byte
    CHECK(overlaps(a, span_of(at(0x0ff1), 16)) && overlaps(span_of(at(0x0ff1), 16), a));      // one byte, from below
    CHECK(overlaps(a, span_of(at(0x1004), 4)) && overlaps(span_of(at(0x1004), 4), a));        // nested
    CHECK(overlaps(a, a));
    CHECK(!overlaps(a, span_of(nullptr, 0)) && !overlaps(span_of(nullptr, 0), a));            // null: no operand
    CHECK(!overlaps(a, span_of(nullptr, 0x2000)) && !overlaps(span_of(nullptr, 0x2000), a));  // null with a length
    CHECK(!overlaps(a, span_of(at(0x1000), 0)) && !overlaps(span_of(at(0x1000), 0), a));      // zero length at either end
    CHECK(!overlaps(a, span_of(at(0x1010), 0)) && !overlaps(span_of(at(0x1010), 0), a));
    CHECK(!overlaps(span_of(at(0x1000), 0), span_of(at(0x1000), 0)));

    // outputs against operands and against each other
    const Span outs[3] = {span_of(at(0x1000), 16), span_of(at(0x2000), 16), span_of(nullptr, 0)};
    const Span clear[2] = {span_of(at(0x1010), 16), span_of(nullptr, 64)};
    const Span hit[2] = {span_of(at(0x3000), 16), span_of(at(0x200f), 1)};
    CHECK(outputs_clear(outs, 3, clear, 2) && outputs_clear(outs, 3, nullptr, 0) && outputs_clear(nullptr, 0, clear, 2));
    CHECK(!outputs_clear(outs, 3, hit, 2));
    const Span twice[3] = {span_of(at(0x1000), 16), span_of(nullptr, 0), span_of(at(0x100c), 4)};
    CHECK(!outputs_clear(twice, 3, clear, 2) && outputs_clear(twice, 2, clear, 2));

    // the same address or disjoint
    CHECK(same_or_disjoint(at(0x1000), at(0x1000), 0) && same_or_disjoint(at(0x1000), at(0x1000), 1));
    CHECK(same_or_disjoint(at(0x1000), at(0x1000), 64));
    CHECK(same_or_disjoint(at(0x1000), at(0x1004), 0) && same_or_disjoint(at(0x1000), at(0x1001), 1));
    CHECK(same_or_disjoint(at(0x1000), at(0x1040), 64) && same_or_disjoint(at(0x1040), at(0x1000), 64));    // adjacent
    CHECK(!same_or_disjoint(at(0x1000), at(0x103c), 64) && !same_or_disjoint(at(0x103c), at(0x1000), 64));  // one element
    CHECK(same_or_disjoint(nullptr, at(0x1000), 64) && same_or_disjoint(at(0x1000), nullptr, 64));

    // pool windows
    int OH = -1, OW = -1;
    CHECK(check_pool_window(1, 1, 1, 1, 1, 1, 0, OH, OW) == QE_OK && OH == 1 && OW == 1);         // kernel 1
    CHECK(check_pool_window(2, 3, 5, 7, 1, 2, 0, OH, OW) == QE_OK && OH == 3 && OW == 4);
    CHECK(check_pool_window(1, 1, 4, 4, 2, 2, 1, OH, OW) == QE_OK && OH == 3 && OW == 3);         // 2 * padding == kernel
    CHECK(check_pool_window(1, 1, 4, 4, 2, 2, 2, OH, OW) == QE_ERR_ARG);                          // ... and one more
    CHECK(check_pool_window(1, 1, 1, 1, 3, 1, 1, OH, OW) == QE_OK && OH == 1 && OW == 1);         // H + 2 * padding == kernel
    CHECK(check_pool_window(1, 1, 2, 1, 4, 3, 1, OH, OW) == QE_ERR_ARG);                          // W one too small
    CHECK(check_pool_window(1, 1, 1, 2, 4, 3, 1, OH, OW) == QE_ERR_ARG);                          // H one too small
    CHECK(check_pool_window(0, 0, 8, 8, 3, 2, 1, OH, OW) == QE_OK && OH == 4 && OW == 4);         // no planes is no fault
    CHECK(check_pool_window(-1, 1, 8, 8, 3, 2, 1, OH, OW) == QE_ERR_ARG && check_pool_window(1, 1, 0, 8, 3, 2, 1, OH, OW) == QE_ERR_ARG);
    CHECK(check_pool_window(1, 1, 8, 8, 0, 2, 0, OH, OW) == QE_ERR_ARG && check_pool_window(1, 1, 8, 8, 3, 0, 1, OH, OW) == QE_ERR_ARG);
    CHECK(check_pool_window(1, 1, 8, 8, 3, 2, -1, OH, OW) == QE_ERR_ARG);

    std::puts("check_request_host: ok");
    return 0;
}
