// movi_buffers.hpp -- the owning types of device and page-locked host memory: plain C++, no HIP include (a host program can compile it:
// tests/host/buffers_driver.cpp).  A memory policy M says where the bytes come from:
//     using error = ...;  static constexpr error ok = ...;  static error alloc(void **p, size_t bytes);  static void free(void *p);
// The library's two -- DeviceMem (hipMalloc / hipFree) and PinnedMem (hipHostMalloc / hipHostFree) -- are defined where HIP is visible
// (movi_kernels.hpp).  Nothing here synchronises: whoever releases a buffer has drained the streams that may touch it.
#pragma once
#include <cstddef>
#include <memory>
#include <utility>
#include <vector>

namespace movi {

// A grow-only buffer: move-only, the destructor frees.  reserve() is the one primitive.  CONTENTS ARE NEVER CARRIED OVER: a growth frees
// the old block first (the peak is one block, not two) and then allocates; after a failed allocation the buffer is empty, capacity 0.
template <class M>
class GrowBuf {
    void *p_ = nullptr;
    size_t cap_ = 0;
public:
    GrowBuf() = default;
    GrowBuf(GrowBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    GrowBuf &operator=(GrowBuf &&o) noexcept {
        if (this != &o) { release(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
        return *this;
    }
    ~GrowBuf() { release(); }
    void *ptr() const { return p_; }
    template <class T> T *as() const { return static_cast<T *>(p_); }
    size_t cap() const { return cap_; }
    void release() {
        if (p_) M::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // cap() >= need: no call at all.  Otherwise the block is replaced by one of `alloc` bytes (the caller's slack rule; alloc >= need).
    typename M::error reserve(size_t need, size_t alloc) {
        if (cap_ >= need) return M::ok;
        release();
        const typename M::error e = M::alloc(&p_, alloc);
        if (e != M::ok) { p_ = nullptr; return e; }
        cap_ = alloc;
        return M::ok;
    }
};

// The grow-only buffer for memory that a captured graph may hold the address of: a block that a captured call has used (mark_in_graph)
// is never freed by a growth -- it is retired, i.e. kept on the list the buffer was made with until release().  One list serves every
// such buffer of a handle; release() of any of them frees the list (the graphs captured over the handle are invalid from there on).
template <class M>
class GraphSafeBuf {
public:
    using Retired = std::vector<GrowBuf<M>>;
    explicit GraphSafeBuf(Retired *retired) : retired_(retired) {}
    void *ptr() const { return live_.ptr(); }
    template <class T> T *as() const { return live_.template as<T>(); }
    size_t cap() const { return live_.cap(); }
    void mark_in_graph() { in_graph_ = true; }
    typename M::error reserve(size_t need, size_t alloc) {
        if (live_.cap() >= need) return M::ok;
        if (live_.ptr() && in_graph_) retired_->push_back(std::move(live_));
        in_graph_ = false;
        return live_.reserve(need, alloc);
    }
    void release() {
        live_.release();
        in_graph_ = false;
        retired_->clear();
    }
    size_t held_bytes() const {                              // the live block and every retired one of the list
        size_t b = live_.cap();
        for (const GrowBuf<M> &r : *retired_) b += r.cap();
        return b;
    }
private:
    GrowBuf<M> live_;
    bool in_graph_ = false;
    Retired *retired_;
};

// The slack rules (B: either buffer type).  Their numbers show through movi_index_info and are asserted to the byte by the tests.
// Device staging and scratch: at least 8 bytes, an eighth on top.
template <class B> auto grow(B &b, size_t bytes) {
    if (bytes < 8) bytes = 8;
    return b.reserve(bytes, bytes + (bytes >> 3));
}
// A page-locked vector of 8-byte entries (the synchronous host path's relative offsets): an eighth more entries.
template <class B> auto grow_entries(B &b, size_t entries) { return b.reserve(entries * 8, (entries + (entries >> 3)) * 8); }
// A pipeline slot's page-locked block: a quarter on top.
template <class B> auto grow_block(B &b, size_t bytes) { return b.reserve(bytes, bytes + (bytes >> 2)); }
// (the segment workspace brings its own `alloc`: reserve() itself)

// A table that is allocated once: std::unique_ptr whose deleter frees through the policy -- or does not, for memory that stays its
// owner's (borrowed(): caller rows adopted by movi_index_create_from_device_rows).
template <class M>
struct FreeWith {
    bool owned = true;
    void operator()(void *p) const { if (owned) M::free(p); }
};
template <class T, class M> using OwnedPtr = std::unique_ptr<T, FreeWith<M>>;
template <class T, class M> OwnedPtr<T, M> borrowed(T *p) { return OwnedPtr<T, M>(p, FreeWith<M>{false}); }
// p = a fresh block of `bytes` (what p held is freed first); empty after a failure
template <class T, class M> typename M::error alloc_owned(OwnedPtr<T, M> &p, size_t bytes) {
    p.reset();
    void *q = nullptr;
    const typename M::error e = M::alloc(&q, bytes);
    p = OwnedPtr<T, M>(e == M::ok ? static_cast<T *>(q) : nullptr);
    return e;
}

}  // namespace movi
