// plba_batch_call.h — the host protocol of a batched front-end call (plba_relative_pose, plba_track_pose, plba_match_descriptors,
// plba_verify_loop_candidates, plba_bow_transform, plba_bow_insert_keyframes): ONE device block laid out by a Layout, one staged copy up,
// the entry point's own launches, one copy down and the call's one counted wait.
//
// An entry point reads: validate; declare the sections (Layout); open(); fill the up image (put / up<T>); upload(); fill the kernels'
// argument blocks from dev<T>(); launch; download(); copy out from down<T>().  The up span is [0, up_end) of the block and the down
// span [down_begin, down_end): they may overlap (masks that go up and come back), the down span may end before the block does
// (workspace behind it, columns nobody asked for) and sections between the two belong to the device alone.
#pragma once
#include "plba_batch_conv.h"
#include "plba_problem.h"

// leave the entry point with the code of a step that failed (the step has written the text)
#define PLBA_TRY(step)                  \
    do {                                \
        if (int rc__ = (step)) return rc__; \
    } while (0)

namespace plba {

struct BatchCall {
    plba_problem* p;
    hipStream_t s;
    DArr<char> blk;      // the device block; back to the pool when the call object goes

    explicit BatchCall(plba_problem* p_) : p(p_), s(p_->stream), scope_(s, p_->have_ctx ? p_->ctx.stage : nullptr) {}

    // the device block of `total` bytes and the staging pair: the pinned area where it is there and large enough, pageable stand-ins
    // otherwise (up is taken first: which of the two still fits depends on it)
    int open(size_t total, size_t up_end, size_t down_begin, size_t down_end) {
        PLBA_HIPCK(p, hipSetDevice(p->device));
        up_end_ = up_end; down_begin_ = down_begin; down_bytes_ = down_end - down_begin;
        hu_ = (char*)stage_take(up_end_);
        hd_ = (char*)stage_take(down_bytes_);
        if (!hu_) { h_up_.resize(up_end_); hu_ = h_up_.data(); }
        if (!hd_) { h_down_.resize(down_bytes_); hd_ = h_down_.data(); }
        PLBA_HIPCK(p, blk.alloc(total, false));
        return PLBA_OK;
    }
    // `bytes` of the caller's into the up image at a 16-byte boundary `off`, the gap up to the next boundary cleared
    void put(size_t off, const void* src, size_t bytes) {
        if (bytes) memcpy(hu_ + off, src, bytes);
        memset(hu_ + off + bytes, 0, (0 - bytes) & 15);
    }
    int upload() {
        PLBA_HIPCK(p, hipMemcpyAsync(blk.p, hu_, up_end_, hipMemcpyHostToDevice, s));
        return PLBA_OK;
    }
    int download() {
        PLBA_HIPCK(p, hipMemcpyAsync(hd_, blk.p + down_begin_, down_bytes_, hipMemcpyDeviceToHost, s));
        PLBA_HIPCK(p, plba_stream_wait(p, s));      // the call's one blocking wait
        return PLBA_OK;
    }
    // a section by its offset in the block: in the up image, on the device, in what came back
    template <class T> T* up(size_t off) const { return reinterpret_cast<T*>(hu_ + off); }
    template <class T> T* dev(size_t off) const { return reinterpret_cast<T*>(blk.p + off); }
    template <class T> const T* down(size_t off) const { return reinterpret_cast<const T*>(hd_ + (off - down_begin_)); }

private:
    DArrStreamScope scope_;
    std::vector<char> h_up_, h_down_;
    char *hu_ = nullptr, *hd_ = nullptr;
    size_t up_end_ = 0, down_begin_ = 0, down_bytes_ = 0;
};

}  // namespace plba
