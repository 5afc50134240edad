// th_mem.hpp - who owns device and pinned memory.  A buffer is a DevBuf / HostBuf MEMBER of whatever uses it - the
// context, a captured graph, a slot order, a function's frame - and is freed when that goes, on every path: nothing names it
// again at teardown or in front of an early return.  Host side only; included by th_ctx.hpp (behind TH_HIP / thi::fail).
// The exception is the ring: ring / view_ring elements, and the two state buffers that trade places with ring elements
// (`spare`, `asort.dst`), are raw pointers - their ADDRESSES are identities (buf_order, gathered_of, seen, asort, the
// rotation) - allocated and freed by hand in th_api.hip / th_order.hip / th_draw.hip.
#pragma once
#include <type_traits>

namespace thi {
namespace detail {

// move-only owner of `count` elements of hipMalloc (Pinned = false) or hipHostMalloc (Pinned = true) memory
template <class T, bool Pinned>
class Buf {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~Buf() { reset(); }

    void reset()
    {
        if (p_) { if (Pinned) (void)hipHostFree(p_); else (void)hipFree(p_); }
        p_ = nullptr; n_ = 0;
    }
    // frees, then allocates exactly `count` elements (uninitialised); on failure the buffer is empty.  `flags`: hipHostMalloc's (a DevBuf has none)
    th_status alloc(size_t count, unsigned flags = hipHostMallocDefault)
    {
        reset();
        void *p = nullptr;
        if (Pinned) TH_HIP(hipHostMalloc(&p, count * sizeof(T), flags));
        else TH_HIP(hipMalloc(&p, count * sizeof(T)));
        p_ = static_cast<T *>(p); n_ = count;
        return TH_OK;
    }
    // grow-only: nothing when `need` elements are there, else alloc(cap) - the caller's growth rule (cap >= need) stays its own
    th_status reserve(size_t need, size_t cap, unsigned flags = hipHostMallocDefault) { return n_ >= need ? TH_OK : alloc(cap, flags); }
    void swap(Buf &o) noexcept { T *p = p_; p_ = o.p_; o.p_ = p; const size_t n = n_; n_ = o.n_; o.n_ = n; }

    size_t size() const { return n_; }                 // elements
    size_t bytes() const { return n_ * sizeof(T); }
    T *get() const { return p_; }                      // (for a reinterpret_cast: everything else converts by itself)
    operator T *() const { return p_; }                // launch sites, pointer arithmetic and `if (!c->x)` read as with a raw pointer

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace detail

template <class T> using DevBuf = detail::Buf<T, false>;
template <class T> using HostBuf = detail::Buf<T, true>;
// (GraphEntry and th_context::SlotOrder live in std::vectors: a move that could throw would make them copy)
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<HostBuf<float>>::value &&
              !std::is_copy_constructible<DevBuf<float>>::value, "DevBuf / HostBuf: move-only, noexcept");

}  // namespace thi
