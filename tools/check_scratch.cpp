// check_scratch.cpp -- the layout of a call's arrays in one allocation (csrc/tsdf_scratch.h), checked
// on the CPU over lists of 1..7 requests of 1-, 4- and 8-byte elements with counts around 0, 1 and
// the 256-byte boundaries, and over counts past 2^31 (offsets only).
//   g++ -std=c++17 -fsanitize=address,undefined -I union-thesis-slam_amd/csrc tools/check_scratch.cpp
// Prints one line per property, "scratch <name> checked <n> bad <n>"; exit status 1 if any is bad.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tsdf_scratch.h"

using namespace tsdf;

namespace {

enum { kAligned, kOrdered, kBytes, kBound, kLarge, kRepeat, kNProps };
const char* const kNames[kNProps] = {"aligned", "ordered", "bytes", "bound", "large", "repeat"};
long long g_checked[kNProps], g_bad[kNProps];

void check(int prop, bool ok) {
    ++g_checked[prop];
    if (!ok) ++g_bad[prop];
}

// one request: n elements of es bytes, and the pointer of that type the layout sets
struct Request {
    int es;
    size_t n;
    unsigned char* p1 = nullptr;
    uint32_t* p4 = nullptr;
    uint64_t* p8 = nullptr;
    Request(int es_, size_t n_) : es(es_), n(n_) {}
    size_t add_to(Layout& l) { return es == 1 ? l.add(&p1, n) : es == 4 ? l.add(&p4, n) : l.add(&p8, n); }
    char* ptr() const { return es == 1 ? (char*)p1 : es == 4 ? (char*)p4 : (char*)p8; }
    uint64_t pattern(size_t array, size_t j) const {  // (its own for each array, in every byte width)
        const uint64_t v = (uint64_t)(array + 1) + 251 * (uint64_t)j + ((uint64_t)(array + 1) << 40);
        return es == 1 ? (v & 0xFF) : es == 4 ? (v & 0xFFFFFFFFu) : v;
    }
    void write(size_t array) const {
        for (size_t j = 0; j < n; ++j) {
            const uint64_t v = pattern(array, j);
            if (es == 1) p1[j] = (unsigned char)v;
            else if (es == 4) p4[j] = (uint32_t)v;
            else p8[j] = v;
        }
    }
    bool read(size_t array) const {
        bool ok = true;
        for (size_t j = 0; j < n; ++j) ok = ok && (es == 1 ? p1[j] : es == 4 ? p4[j] : p8[j]) == pattern(array, j);
        return ok;
    }
};

void check_list(std::vector<Request> rq) {
    Layout l;
    std::vector<size_t> off;
    for (Request& r : rq) off.push_back(r.add_to(l));
    // every offset a multiple of 256; the ranges disjoint and in request order; bytes(): the end of
    // the last range, rounded up
    size_t end = 0;
    for (size_t i = 0; i < rq.size(); ++i) {
        check(kAligned, off[i] % 256 == 0 && l.req[i].off == off[i]);
        check(kOrdered, off[i] >= end);
        end = off[i] + (size_t)rq[i].es * rq[i].n;
    }
    check(kBytes, l.bytes() == (end + 255) / 256 * 256);
    // a second layout of the same requests: the same offsets
    {
        std::vector<Request> again;
        for (const Request& r : rq) again.emplace_back(r.es, r.n);
        Layout l2;
        bool same = true;
        for (size_t i = 0; i < again.size(); ++i) same = same && again[i].add_to(l2) == off[i];
        check(kRepeat, same && l2.bytes() == l.bytes());
    }
    // bound into a block of exactly bytes(): every array written end to end, then all read back
    char* base = (char*)std::malloc(l.bytes());
    if (!base && l.bytes()) {
        check(kBound, false);
        return;
    }
    l.bind(base);
    for (size_t i = 0; i < rq.size(); ++i) check(kBound, rq[i].ptr() == base + off[i]);
    for (size_t i = 0; i < rq.size(); ++i) rq[i].write(i);
    for (size_t i = 0; i < rq.size(); ++i) check(kBound, rq[i].read(i));
    std::free(base);
}

// counts past 2^31: nothing of the arithmetic is in 32 bits (offsets only: nothing is bound)
void check_large() {
    Request a(8, ((size_t)1 << 31) + 3), b(4, 5), c(1, ((size_t)1 << 32) + 1), d(8, 1), e(4, ((size_t)1 << 31) + 3);
    Layout l;
    check(kLarge, a.add_to(l) == 0);
    // a: 8 * (2^31 + 3) = 2^34 + 24 bytes; c: 2^32 + 1; e: 4 * (2^31 + 3) = 2^33 + 12; each rounded up to 256
    const size_t G = (size_t)1 << 32;
    check(kLarge, b.add_to(l) == 4 * G + 256);
    check(kLarge, c.add_to(l) == 4 * G + 512);
    check(kLarge, d.add_to(l) == 5 * G + 768);
    check(kLarge, e.add_to(l) == 5 * G + 1024);
    check(kLarge, l.bytes() == 7 * G + 1280);
    check(kLarge, sizeof(size_t) == 8);
}

}  // namespace

int main() {
    const size_t counts[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000};
    const int sizes[] = {1, 4, 8};
    constexpr int kNc = sizeof(counts) / sizeof(counts[0]);
    // every single request, every pair, and longer lists drawn by a fixed generator
    for (int es : sizes)
        for (size_t n : counts) check_list({Request(es, n)});
    for (int e1 : sizes)
        for (size_t n1 : counts)
            for (int e2 : sizes)
                for (size_t n2 : counts) check_list({Request(e1, n1), Request(e2, n2)});
    unsigned long long state = 12345;
    auto draw = [&](int m) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((state >> 33) % (unsigned)m);
    };
    for (int k = 0; k < 2000; ++k) {
        std::vector<Request> rq;
        const int len = 3 + draw(5);
        for (int i = 0; i < len; ++i) {
            const int es = sizes[draw(3)];
            rq.emplace_back(es, counts[draw(kNc)]);
        }
        check_list(rq);
    }
    check_large();
    long long bad = 0;
    for (int p = 0; p < kNProps; ++p) {
        std::printf("scratch %s checked %lld bad %lld\n", kNames[p], g_checked[p], g_bad[p]);
        bad += g_bad[p];
    }
    return bad ? 1 : 0;
}
