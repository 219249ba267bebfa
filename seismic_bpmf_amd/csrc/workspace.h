// One statement of a workspace layout for both of its readers.  A layout is a function that takes regions from
// a Carver in order; bpmf_*_workspace_bytes runs it on a null base and reads bytes(), the *_dev entry point runs
// it on the caller's workspace and uses the addresses.  The two cannot disagree: there is one list of regions.
// Plain C++17, no HIP: a host program can compile this header alone (tests/test_workspace_layout.py does).
#pragma once
#include <cstddef>

namespace bpmf {

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

class Carver {
public:
    explicit Carver(void* base) : base_((char*)base) {}

    // `count` elements of T and `extra_bytes`, the end rounded up to `align`.  On a null base: nullptr, and
    // the offset advances all the same (no nullptr + offset is ever formed).
    template <class T>
    T* take(size_t count, size_t extra_bytes = 0, size_t align = 256)
    {
        return (T*)nest(count * sizeof(T) + extra_bytes, align);
    }
    // a region of `bytes` that a layout of its own carves (from the address returned)
    void* nest(size_t bytes, size_t align = 256)
    {
        void* at = base_ ? base_ + off_ : nullptr;
        off_ += align_up(bytes, align);
        return at;
    }
    void skip(size_t bytes) { off_ += bytes; }

    size_t offset() const { return off_; }   // of the next region
    size_t bytes() const { return off_; }    // of the whole layout, once every region is taken

private:
    char* base_;
    size_t off_ = 0;
};

}  // namespace bpmf
