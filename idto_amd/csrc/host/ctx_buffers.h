// ctx_buffers.h — the owners of a context's staging and grown buffers: one pinned host buffer (Pinned) or one device buffer
// (Grown) each, made on first use, grown on demand, freed by its destructor.  A new entry adds a member and calls Ensure;
// nothing in idto_hip_destroy.  An owner, not an allocator: no pooling, no reuse.
//
// Host-only (tests/cpp/ctx_buffers_check.cc runs it over a counting fake): the four memory calls come from a policy M,
//   static int  PinAlloc(void** p, size_t bytes);   static void PinFree(void* p);
//   static int  DevAlloc(void** p, size_t bytes);   static void DevFree(void* p);
// where an allocation returns 0, or a negative status after writing the error text, and DevAlloc's memory is zero-filled
// with the fill finished on return.  idto_hip.hip supplies the HIP one.
#pragma once

#include <cstddef>
#include <utility>

namespace idto_host {

template <class T, class M, bool kDevice>
class OwnedBuffer {
 public:
  OwnedBuffer() = default;
  OwnedBuffer(OwnedBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  OwnedBuffer& operator=(OwnedBuffer&& o) noexcept {
    if (this != &o) {
      Reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~OwnedBuffer() { Reset(); }

  // Room for `count` elements (at least `at_least` when it has to be made): nothing happens while the capacity suffices - a
  // smaller request after a larger one allocates nothing.  Otherwise the superseded buffer is freed and the larger one
  // made - what the old one held is gone.  alloc_first: made, then the old one freed - for a device buffer that enqueued
  // work may still read: DevAlloc's wait behind its fill has drained that work by then, no wait of its own is needed.
  // After a failed allocation the buffer is empty (null, capacity 0); the next Ensure tries again.
  int Ensure(size_t count, size_t at_least = 0, bool alloc_first = false) {
    if (cap_ >= count) return 0;
    const size_t n = count > at_least ? count : at_least;
    if (!alloc_first) Reset();
    void* p = nullptr;
    const int rc = kDevice ? M::DevAlloc(&p, n * sizeof(T)) : M::PinAlloc(&p, n * sizeof(T));
    Reset();
    if (rc) return rc;
    p_ = static_cast<T*>(p);
    cap_ = n;
    return 0;
  }
  void Reset() {
    if (p_) kDevice ? M::DevFree(p_) : M::PinFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  operator T*() const { return p_; }   // (read where the bare pointer was read)
  size_t cap() const { return cap_; }  // elements

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <class T, class M> using Pinned = OwnedBuffer<T, M, false>;
template <class T, class M> using Grown = OwnedBuffer<T, M, true>;

// A device buffer with its pinned mirror: both or neither - a call whose device side grew while its pinned side failed
// reports the failure, and the next call makes what is missing.
template <class M>
struct GrownPair {
  Grown<double, M> dev;
  Pinned<double, M> pin;
  int Ensure(size_t dev_count, size_t pin_count) {
    if (int rc = dev.Ensure(dev_count)) return rc;
    return pin.Ensure(pin_count);
  }
};

}  // namespace idto_host
