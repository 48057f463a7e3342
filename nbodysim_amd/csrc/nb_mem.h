// nb_mem.h — one owner for device and page-locked host memory.  Host only: no kernels, nothing of nb_sim.
// A MemPool fills pointers and remembers them: release(p) gives one block back, release_all() (and the destructor) the
// rest, and both null the pointer; regrow(cap, want, p...) is the grow-only scratch, arrays that share one capacity.
// No memset, no alignment policy, no caching: a request is one call of the backend B:
//   B::error, B::ok, B::misuse (alloc into a pointer that is not null), and static device / pinned (void **, bytes),
//   free_device / free_pinned (void *).  The library's is HipMem (nb_sim.hip.h); nb_fuzz.cpp runs the pool over malloc.
#pragma once
#include <cstddef>
#include <type_traits>
#include <vector>

namespace nbk {
template <typename B>
class MemPool {
    struct Block { void **slot; bool pinned; };       // *slot is the block
    std::vector<Block> blocks;

    static void give_back(const Block &b)
    {
        if (b.pinned) B::free_pinned(*b.slot); else B::free_device(*b.slot);
        *b.slot = nullptr;
    }
    // `count` elements of T (bytes for a void *) into p.  On failure p stays null and nothing is recorded.
    template <typename T>
    typename B::error take(T *&p, size_t count, bool pinned)
    {
        if (p) return B::misuse;
        void *q = nullptr;
        const size_t bytes = count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>);
        blocks.reserve(blocks.size() + 1);            // the push_back below cannot fail and strand the block
        const typename B::error e = pinned ? B::pinned(&q, bytes) : B::device(&q, bytes);
        if (e != B::ok) return e;
        p = static_cast<T *>(q);
        blocks.push_back(Block{(void **)&p, pinned});
        return B::ok;
    }

    template <typename C, typename... T>
    typename B::error regrow_as(bool pinned, C &cap, size_t want, T *&...p)
    {
        if (cap >= want) return B::ok;
        (release(p), ...);
        cap = 0;
        typename B::error e = B::ok;
        (void)(((e = take(p, want, pinned)) == B::ok) && ...);    // stops at the first refusal
        if (e == B::ok) cap = (C)want;
        return e;
    }

public:
    MemPool() = default;
    MemPool(const MemPool &) = delete;
    ~MemPool() { release_all(); }
    size_t size() const { return blocks.size(); }

    template <typename T> typename B::error alloc(T *&p, size_t count) { return take(p, count, false); }
    template <typename T> typename B::error alloc_pinned(T *&p, size_t count) { return take(p, count, true); }
    template <typename T>
    void release(T *&p)                               // null: nothing; a pointer the pool did not fill is left alone
    {
        for (size_t k = blocks.size(); p && k-- > 0;)
            if (blocks[k].slot == (void **)&p) { give_back(blocks[k]); blocks.erase(blocks.begin() + (long)k); }
    }
    // Arrays p... that share the capacity `cap` (elements each; bytes for a void *).  cap >= want: nothing.  Otherwise all are released
    // and allocated anew with `want` elements; cap is 0 from the first release until the last request succeeded.  After a failure (the
    // backend's error) every p is null or a live recorded block, and the next regrow of the set starts over.
    template <typename C, typename... T>
    typename B::error regrow(C &cap, size_t want, T *&...p) { return regrow_as(false, cap, want, p...); }
    template <typename C, typename... T>
    typename B::error regrow_pinned(C &cap, size_t want, T *&...p) { return regrow_as(true, cap, want, p...); }
    void release_all()
    {
        for (const Block &b : blocks) give_back(b);
        blocks.clear();
    }
};
}  // namespace nbk
