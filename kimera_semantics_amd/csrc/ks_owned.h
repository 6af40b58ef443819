// ks_owned.h — the owners of what the host side holds of the HIP runtime: one device block (DevBuf), one pinned host block
// (PinnedBuf), one event, one stream.  An owner is a member (or a local) that frees its resource when it goes away and cannot
// be copied; everything a kernel takes by value (TileTable, Pool, MeshArena, BoCtx, the *View structs, FrameParams) stays plain
// data whose raw pointers are VIEWS of a block some owner holds.  DESIGN.md, "Ownership".
#pragma once
#include <stddef.h>
#include <utility>

#include <hip/hip_runtime.h>

#include "../../include/ks_hip.h"

// ctx->err = "<what>: <the runtime's text>"; returns KS_ERR_HIP (ks_hip.hip, beside HIPCHK)
int ks_hip_failed(ks_ctx* ctx, const char* what, hipError_t e);

// One hipMalloc block of T and its element count.  Move-only; converts to T*, so launches, copies and view structs take it as it is.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
      n_ = std::exchange(o.n_, 0);
    }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }

  // Replaces the block by one of n elements (n == 0: one element).  On failure the owner is empty, {nullptr, 0}.
  hipError_t try_alloc(size_t n) {
    release();
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
    if (e == hipSuccess) n_ = n;
    else p_ = nullptr;
    return e;
  }
  // ... with the failure reported in ctx->err, as HIPCHK does
  int alloc(ks_ctx* ctx, size_t n) {
    const hipError_t e = try_alloc(n);
    return e == hipSuccess ? KS_OK : ks_hip_failed(ctx, "hipMalloc", e);
  }
  // Grow-only: nothing when n elements fit (one compare), else a NEW block of cap_if_grown elements — the call site's growth rule.
  int reserve(ks_ctx* ctx, size_t n, size_t cap_if_grown) { return n <= n_ ? KS_OK : alloc(ctx, cap_if_grown); }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// One hipHostMalloc block of n elements of T (pinned, device-visible).  Allocated once, never handed on.
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
  int alloc(ks_ctx* ctx, size_t n) {
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    const hipError_t e = hipHostMalloc((void**)&p_, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    return e == hipSuccess ? KS_OK : ks_hip_failed(ctx, "hipHostMalloc", e);
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }

 private:
  T* p_ = nullptr;
};

// One event / one stream.  They live in slots and arrays of the context and never change hands.
class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  int create(ks_ctx* ctx, unsigned flags) {
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    return e == hipSuccess ? KS_OK : ks_hip_failed(ctx, "hipEventCreateWithFlags", e);
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  int create(ks_ctx* ctx, unsigned flags) {
    const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
    return e == hipSuccess ? KS_OK : ks_hip_failed(ctx, "hipStreamCreateWithFlags", e);
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};
