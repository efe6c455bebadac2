// se_devmem.h -- internal: owning handles for the host code's GPU resources.
//
//   DevBuf<T>    one hipMalloc allocation of size() elements of T
//   PinnedBuf<T> one hipHostMalloc allocation of size() elements of T
//   Stream       one hipStream_t        Event   one hipEvent_t
//
// All four are move-only and free what they hold in their destructor.  Whether a buffer holds secrets (keys,
// seeds, errors, plaintexts, `a`) is fixed where it is declared -- `DevBuf<int8_t> err{Secret::yes};` -- and a
// secret buffer is zeroed (hipMemset / explicit_bzero) before its memory goes back to the allocator, on grow()
// as on release() and destruction.
//
// Precondition of grow(), release() and destruction: nothing still uses the memory.  The owner drains the
// streams that used it first; these types add no synchronisation of their own and never call hipSetDevice (the
// owner has the device of the allocation current).
#pragma once
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <cstddef>
#include <utility>

namespace seamd {

enum class Secret : bool { no = false, yes = true };

struct DeviceMem
{
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void wipe(void *p, size_t bytes) { (void)hipMemset(p, 0, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};

struct PinnedMem
{
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void wipe(void *p, size_t bytes) { explicit_bzero(p, bytes); }
    static void free(void *p) { (void)hipHostFree(p); }
};

template <typename T, typename Mem>
class Buf
{
public:
    explicit Buf(Secret s = Secret::no) : secret_(s == Secret::yes) {}
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)), secret_(o.secret_) {}
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o)
        {
            release();
            p_      = std::exchange(o.p_, nullptr);
            n_      = std::exchange(o.n_, 0);
            secret_ = o.secret_;
        }
        return *this;
    }
    ~Buf() { release(); }

    // Room for at least `count` elements.  Growing drops the old contents (wiped first if secret).  On failure
    // the buffer is left empty and the error is returned.
    hipError_t grow(size_t count)
    {
        if (count <= n_) return hipSuccess;
        release();
        void *p      = nullptr;
        hipError_t e = Mem::alloc(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p);
        n_ = count;
        return hipSuccess;
    }

    void release()
    {
        if (!p_) return;
        if (secret_) Mem::wipe(p_, n_ * sizeof(T));
        Mem::free(p_);
        p_ = nullptr;
        n_ = 0;
    }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t size() const { return n_; }

private:
    T *p_   = nullptr;
    size_t n_ = 0;
    bool secret_;
};

template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using PinnedBuf = Buf<T, PinnedMem>;

// A default-constructed handle holds nothing; create() makes one if none is held yet (lazy creation).
template <typename H, hipError_t (*Create)(H *, unsigned), hipError_t (*Destroy)(H)>
class Handle
{
public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept
    {
        if (this != &o)
        {
            if (h_) (void)Destroy(h_);
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle()
    {
        if (h_) (void)Destroy(h_);
    }

    hipError_t create(unsigned flags) { return h_ ? hipSuccess : Create(&h_, flags); }
    operator H() const { return h_; }

private:
    H h_ = nullptr;
};

using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event  = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

}  // namespace seamd
