// stream_lane.hpp -- the owners of what the orchestrator creates on the device (events, streams, buffers) and the fork /
// join protocol of a hook that runs on a stream of its own beside the frame.  Host code only; textually included by
// mmf_hip.hip in front of redetect_host.hpp, the first file that uses the owners (the view store's buffers).
#pragma once

// What the owners share: one handle, move-only, released through Free when it goes.  An empty one owns nothing.
template <typename H, hipError_t (*Free)(H)>
struct Owned {
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) reset(), h_ = o.h_, o.h_ = nullptr;
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (h_) (void)Free(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

protected:
    H h_ = nullptr;
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {  // no timing
    hipError_t create() { return reset(), hipEventCreateWithFlags(&h_, hipEventDisableTiming); }
};
// Destroying a stream does not wait for its work: whoever owns buffers that work reads lets the stream run dry first.
struct Stream : Owned<hipStream_t, hipStreamDestroy> {  // non-blocking
    hipError_t create() { return reset(), hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
    void drain() const {
        if (h_) (void)hipStreamSynchronize(h_);
    }
};
using DeviceMem = Owned<void*, hipFree>;  // device memory, whatever it holds
template <typename T>
struct DeviceBuf : DeviceMem {  // `count` elements of device memory
    hipError_t create(size_t count) { return reset(), hipMalloc(&h_, count * sizeof(T)); }
    T* get() const { return static_cast<T*>(h_); }
};
template <typename T>
struct PinnedBuf : Owned<void*, hipHostFree> {  // ... of page-locked host memory
    hipError_t create(size_t count, unsigned flags = hipHostMallocDefault) { return reset(), hipHostMalloc(&h_, count * sizeof(T), flags); }
    T* get() const { return static_cast<T*>(h_); }
};

// what is enqueued on `to` from here on runs behind what `from` holds now
static inline hipError_t order(hipStream_t from, hipEvent_t ev, hipStream_t to) {
    const hipError_t e = hipEventRecord(ev, from);
    return e != hipSuccess ? e : hipStreamWaitEvent(to, ev, 0);
}

// A stream beside the frame's main stream: work that depends on the frame's inputs only forks off the main stream (open,
// enter), runs on the lane, and the main stream takes it in again later (close, join).  `pending`: `done` is recorded and
// nothing has waited for it -- a frame that fails between close and join leaves it set, and the next open waits first.
struct SideLane {
    Stream stream;
    Event begin;  // main stream: the lane's inputs are there, the readers of its last result are done
    Event done;   // lane: this frame's result is complete
    bool pending = false;

    hipError_t create() {
        hipError_t e = stream.create();
        if (e == hipSuccess) e = begin.create();
        if (e == hipSuccess) e = done.create();
        if (e != hipSuccess) reset();
        return e;
    }
    void reset() {  // (the stream runs dry first)
        stream.drain();
        begin.reset(), done.reset(), stream.reset();
        pending = false;
    }
    ~SideLane() { reset(); }

    hipError_t open(hipStream_t main) {
        if (pending) {
            const hipError_t e = hipStreamWaitEvent(main, done.get(), 0);
            if (e != hipSuccess) return e;
            pending = false;
        }
        return hipEventRecord(begin.get(), main);
    }
    hipError_t enter() { return hipStreamWaitEvent(stream.get(), begin.get(), 0); }
    hipError_t close() {
        const hipError_t e = hipEventRecord(done.get(), stream.get());
        if (e == hipSuccess) pending = true;
        return e;
    }
    hipError_t join(hipStream_t into) {
        const hipError_t e = hipStreamWaitEvent(into, done.get(), 0);
        if (e == hipSuccess) pending = false;
        return e;
    }
};
