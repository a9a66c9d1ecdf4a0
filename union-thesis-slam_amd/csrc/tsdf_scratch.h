// tsdf_scratch.h -- the layout of several arrays in one allocation (host only, no HIP: the CPU
// check tools/check_scratch.cpp compiles it alone).
#pragma once
#include <cstddef>
#include <vector>

namespace tsdf {

// A call records its arrays once -- add(&pointer, elements) -- allocates bytes() and bind()s: every
// recorded pointer then points at its array.  Arrays lie in the order of their requests, each from
// a 256-byte boundary (the alignment an allocation of its own would give it, enough for any element
// type and for hipcub's temporary storage); an array of 0 elements takes no room.  The offsets
// depend on the requests alone, and all arithmetic is in size_t.
struct Layout {
    struct Req {
        void* out;  // the T* to set, by the function that knows T
        size_t off;
        void (*set)(void* out, char* p);
    };
    std::vector<Req> req;
    size_t end = 0;

    template <typename T>
    size_t add(T** out, size_t n) {  // returns the array's offset
        const size_t off = end;
        req.push_back({out, off, [](void* o, char* p) { *(T**)o = (T*)p; }});
        end += (sizeof(T) * n + 255) & ~(size_t)255;
        return off;
    }
    size_t bytes() const { return end; }
    void bind(char* base) const {
        for (const Req& r : req) r.set(r.out, base + r.off);
    }
};

}  // namespace tsdf
