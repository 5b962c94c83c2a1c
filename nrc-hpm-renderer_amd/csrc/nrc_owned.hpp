// nrc_owned.hpp -- move-only owners of what the host layer has to give back: a handle with its destroy function, a device allocation.
// A member of one of these types OWNS (its class needs no destructor for it, and a constructor that throws releases what it had built);
// a raw pointer or handle next to it BORROWS.  Device-free: tests/cpp/host_logic_main.cpp supplies dev_alloc / dev_free itself.
#pragma once
#include <cstddef>
#include <utility>

namespace nrc {

// Every device allocation of the library goes through these two (nrc_api.hip); NRC_DEBUG=poison_alloc / guard_alloc (nrc_common.hpp) make
// them fill what they hand out with NaN bytes / fence it with canaries that nrc_debug_check_guards() and every dev_free verify.
void dev_alloc(void** p, size_t bytes, const char* what = "");
void dev_free(void* p);
template <class T>
inline void dev_alloc(T** p, size_t bytes, const char* what = "") { dev_alloc(reinterpret_cast<void**>(p), bytes, what); }

// a handle H (H{} = none) that Destroy(h) gives back
template <class H, auto Destroy>
class Owned {
public:
    Owned() = default;
    explicit Owned(H h) : h_(h) {}
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
    Owned& operator=(Owned&& o) noexcept { if (this != &o) reset(std::exchange(o.h_, H{})); return *this; }
    ~Owned() { reset(); }
    void reset(H h = H{}) { if (h_ != H{}) (void)Destroy(h_); h_ = h; }
    H get() const { return h_; }
    operator H() const { return h_; }

private:
    H h_{};
};

template <class T>
inline void dev_release(T* p) { dev_free(p); }

// device memory from dev_alloc
template <class T>
class DevBuf {
public:
    // frees what the buffer held FIRST: a failing allocation leaves it empty, not dangling
    void alloc(size_t bytes, const char* what)
    {
        p_.reset();
        T* p = nullptr;
        dev_alloc(&p, bytes, what);
        p_.reset(p);
    }
    void reset() { p_.reset(); }
    T* get() const { return p_.get(); }
    operator T*() const { return p_.get(); }
    explicit operator bool() const { return p_.get() != nullptr; }
    template <class U>
    explicit operator U*() const { return static_cast<U*>(p_.get()); }      // (half_t*)buf of a DevBuf<void>: the cast its reader writes

private:
    Owned<T*, dev_release<T>> p_;
};

}  // namespace nrc
