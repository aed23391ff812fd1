// dcs_cache.h -- CacheBuf, the one owner of a buffer borrowed from a context's buffer cache (dcs_runtime.hip: cacheAlloc /
// cacheFree).  The cache knows the real size of every buffer it handed out, so the owner keeps only what it asked for.
// CacheArena, the owner of all the buffers that one call borrows for work on the context's stream.
// GrowBuf, the one owner of a buffer that lives OUTSIDE the cache: one that is kept and only ever grows (the live decoder's
// arenas, an indexer's tables, the resident index inputs), or a diagnostic entry's temporary that the cache should not keep.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <vector>

struct DcsCtx;
hipStream_t dcsCtxStream(DcsCtx *ctx);
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

// The device buffers of one call.  Move-only.  What the type is for is how they go back: an arena that still holds
// something when it goes waits for the context's stream (kernels and copies queued there may be using them) and then gives
// them back in the order they were taken, which is the order the cache will evict them in.  clear() gives them back at
// once, for buffers nothing was queued on; an owner of several arenas that must go back after ONE wait calls wait() and
// then clear() on each, in the order it wants them back.
class CacheArena
{
public:
    explicit CacheArena(DcsCtx *ctx) : ctx_(ctx), stream_(dcsCtxStream(ctx)) {}
    CacheArena(const CacheArena &) = delete;
    CacheArena &operator=(const CacheArena &) = delete;
    CacheArena(CacheArena &&) = default;            // (what it is moved from holds nothing, and goes without a wait)
    ~CacheArena()
    {
        if (!bufs_.empty())
            wait();
        clear();
    }

    // `count` objects of T in device memory, the byte count rounded up to 256; *p is null on failure
    template <class T> hipError_t alloc(T **p, size_t count)
    {
        bufs_.emplace_back();
        const hipError_t e = bufs_.back().alloc(ctx_, false, (sizeof(T) * count + 255) & ~size_t(255));
        *p = bufs_.back().as<T>();
        return e;
    }
    void wait() const { (void)hipStreamSynchronize(stream_); }
    void clear()
    {
        for (CacheBuf &b : bufs_)
            b.release();
        bufs_.clear();
    }
    bool empty() const { return bufs_.empty(); }
    DcsCtx *ctx() const { return ctx_; }
    hipStream_t stream() const { return stream_; }

private:
    DcsCtx *ctx_;
    hipStream_t stream_;
    std::vector<CacheBuf> bufs_;
};

// One allocation of pinned host or device memory made with the runtime directly, never through the context's cache (whose byte
// counts it leaves alone).  Move-only; an owner that goes frees.  Nothing here waits: whoever lets a buffer go or grow while work
// queued on a stream may still use it waits for that stream first.
class GrowBuf
{
public:
    explicit GrowBuf(bool pinned = false) : pinned_(pinned) {}
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    GrowBuf(GrowBuf &&o) noexcept : p_(o.p_), cap_(o.cap_), pinned_(o.pinned_) { o.p_ = nullptr; o.cap_ = 0; }
    ~GrowBuf() { release(); }

    // room for `bytes`: nothing happens when the capacity suffices; else the old allocation is freed -- what it held is NOT kept --
    // and one of `bytes` rounded up to 64 KiB is made; on failure it owns nothing.  `first`: the least a buffer that holds nothing
    // yet starts with (a decoder's look-ahead grows 64 -> 512 -> 4 096 frames within its first three calls, and every step used to
    // free and pin the live arenas again -- 0.7-1.5 ms of a new context's first stream, NOTES 44).
    hipError_t room(size_t bytes, size_t first = 0)
    {
        if (bytes <= cap_)
            return hipSuccess;
        const size_t want = ((p_ == nullptr && bytes < first ? first : bytes) + 65535) & ~size_t(65535);
        release();
        const hipError_t e = pinned_ ? hipHostMalloc(&p_, want, hipHostMallocDefault) : hipMalloc(&p_, want);
        if (e == hipSuccess)
            cap_ = want;
        else
            p_ = nullptr;
        return e;
    }
    void release()
    {
        if (p_ != nullptr)
            (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    template <class T = void> T *as() const { return static_cast<T *>(p_); }
    size_t capacity() const { return cap_; }        // what it really holds

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
    bool pinned_;
};
