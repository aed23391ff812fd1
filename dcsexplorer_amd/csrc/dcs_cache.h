// dcs_cache.h -- CacheBuf, the one owner of a buffer borrowed from a context's buffer cache (dcs_runtime.hip: cacheAlloc /
// cacheFree).  The cache knows the real size of every buffer it handed out, so the owner keeps only what it asked for.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct DcsCtx;
hipError_t dcsCtxAlloc(DcsCtx *ctx, bool pinned, void **out, size_t bytes);
void dcsCtxFree(DcsCtx *ctx, bool pinned, void *p);

// Move-only.  An owner that goes gives its buffer back; an owner whose buffer must go back at a given moment (the cache evicts its
// oldest entries first, so the order of releases is part of what it keeps) calls release() there.
class CacheBuf
{
public:
    CacheBuf() = default;
    CacheBuf(const CacheBuf &) = delete;
    CacheBuf &operator=(const CacheBuf &) = delete;
    CacheBuf(CacheBuf &&o) noexcept : ctx_(o.ctx_), p_(o.p_), bytes_(o.bytes_), pinned_(o.pinned_) { o.p_ = nullptr; o.bytes_ = 0; }
    ~CacheBuf() { release(); }

    // `bytes` of pinned host or device memory from the cache of `ctx` (what this owner held goes back first); on failure it owns nothing
    hipError_t alloc(DcsCtx *ctx, bool pinned, size_t bytes)
    {
        release();
        void *p = nullptr;
        const hipError_t e = dcsCtxAlloc(ctx, pinned, &p, bytes);
        if (e == hipSuccess)
        {
            ctx_ = ctx; p_ = p; bytes_ = bytes; pinned_ = pinned;
        }
        return e;
    }
    void release()
    {
        if (p_ != nullptr)
            dcsCtxFree(ctx_, pinned_, p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    template <class T = void> T *as() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }        // what was asked for
    explicit operator bool() const { return p_ != nullptr; }

private:
    DcsCtx *ctx_ = nullptr;
    void *p_ = nullptr;
    size_t bytes_ = 0;
    bool pinned_ = false;
};
