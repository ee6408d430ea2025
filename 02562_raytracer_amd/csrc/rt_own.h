// rt_own.h -- owners of runtime handles, free of the HIP headers (tests/native/own_check.cpp
// runs them over a counting stub).  Tr names the handle and its two calls:
//   using type = ...; using status = ...;   (a null type{} is "no handle", status{} is success)
//   static status create(type* out, unsigned flags);   static void destroy(type h);
// csrc/rt_ctx.h has the HIP traits: Event, Stream, EventPool.
#pragma once
#include <stddef.h>

#include <utility>
#include <vector>

// One handle, made at the first ensure() and destroyed with its owner.  Move-only.
template <class Tr>
class Handle {
    typename Tr::type h_ = {};

public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, {})) {}
    Handle& operator=(Handle&& o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, {});
        }
        return *this;
    }
    ~Handle() { reset(); }
    void reset()
    {
        if (h_) Tr::destroy(h_);
        h_ = {};
    }
    typename Tr::status ensure(unsigned flags = 0)
    {
        if (h_) return {};
        const typename Tr::status e = Tr::create(&h_, flags);
        if (e != typename Tr::status{}) h_ = {};
        return e;
    }
    typename Tr::type get() const { return h_; }
    operator typename Tr::type() const { return h_; }   // (the runtime's calls take the owner as they took the handle)
};

// Handles used in groups of K, at most Cap of them: [0, used) are taken since the last
// `used = 0`, which keeps the handles for the next round.  The pool grows by a whole
// group or not at all.
template <class Tr, size_t K, size_t Cap>
struct Pool {
    std::vector<Handle<Tr>> h;
    size_t used = 0;
    bool full() const { return used + K > Cap; }
    // the K handles from `used` on exist (not full())
    typename Tr::status ensure_group()
    {
        if (h.size() >= used + K) return {};
        Handle<Tr> g[K];   // (a failure destroys the ones made so far)
        for (Handle<Tr>& x : g)
            if (const typename Tr::status e = x.ensure(); e != typename Tr::status{}) return e;
        h.resize(h.size() + K);
        for (size_t i = 0; i < K; i++) h[h.size() - K + i] = std::move(g[i]);
        return {};
    }
    typename Tr::type operator[](size_t i) const { return h[i].get(); }
};
