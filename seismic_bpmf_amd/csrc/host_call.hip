// The scope of one host-pointer call and the day of data arriving in it: see host_call.h.
#include "host_call.h"

namespace bpmf {

// Streams, events, pinned pieces and the device working set are the device's (context.h): created once, reused by
// every call, one call per device at a time -- nothing is created or destroyed per call, nothing runs on the null
// stream.  Every call binds its thread to `device` first (a fresh host thread starts on device 0).
HostCall::HostCall(const char* name, int device, FanoutScope& fan_)
    : fan(fan_), t0(host_now_ms()), name_(name), bind_(device)
{
    t_call_stats = HostCallStats();
    if (bind_.error() != hipSuccess) {
        set_error("%s: binding device %d failed: %s", name_, device, hipGetErrorString(bind_.error()));
        rc = -2;
        return;
    }
    ctx = device_context(device);
    if (!ctx) {
        rc = -2;
        return;
    }
    // (the hand-over is adopted behind the lock: a source waits for its peers before another call may touch its data)
    lock_ = std::unique_lock<std::mutex>(ctx->call_mutex);
}

char* HostCall::reserve(size_t pinned_bytes)
{
    if (!ok()) return nullptr;
    const double t = host_now_ms();
    char* base = ctx->reserve_device(total_);
    if (!base || (pinned_bytes && ctx->reserve_pinned(pinned_bytes))) {
        rc = -2;
        return nullptr;
    }
    t_call_stats.reserve_ms = host_now_ms() - t;
    return base;
}

void HostCall::fail(hipError_t e, const char* what)
{
    if (!rc) set_error("%s: %s failed: %s", name_, what, hipGetErrorString(e));
    note(-2);
}

void HostCall::finish()
{
    if (finished_) return;
    finished_ = true;
    if (lock_.owns_lock()) {
        // (always drained, also after a failure: the working set goes back to its cache)
        const hipError_t es = hipStreamSynchronize(ctx->s_run);
        (void)hipStreamSynchronize(ctx->s_copy);
        if (also_drain) (void)hipStreamSynchronize(also_drain);
        if (wait_since != 0.0) t_call_stats.device_wait_ms = host_now_ms() - wait_since;
        t_call_stats.total_ms = host_now_ms() - t0;
        if (es != hipSuccess) fail(es, "synchronize");
    }
    // No host thread of the copy pool still reads the caller's arrays or writes into a pinned piece (a straggler of
    // an idempotent fill, context.hip: CopyPool::run) when the call returns.
    copy_pool_quiesce();
    // A SOURCE's peers copy from the buffer it published until they report peer_done: they are through with its
    // copy of the day BEFORE anything may free the working set -- the trim below under option host.cache_limit_mb.
    fan.finish();
    if (lock_.owns_lock()) ctx->trim_after_call();
}

bool DayFeed::from_peer(void* d_dst, size_t bytes, hipStream_t stream)
{
    if (!hc_.ok()) return false;
    const char* what = "";
    hipError_t e = hipSuccess;
    const bool peer = fanout_peer_copy(hc_.fan, hc_.ctx, d_dst, bytes, stream, &e, &what);
    if (peer && e != hipSuccess) hc_.fail(e, what);
    return peer;
}

hipEvent_t DayFeed::next_event()
{
    return hc_.ctx->ev_chunk[n_events_++ % DeviceContext::CHUNK_EVENTS];
}

void DayFeed::fork_from(hipStream_t run_stream)
{
    if (!hc_.ok()) return;
    hipEvent_t ev = next_event();
    hipError_t e;
    if ((e = hipEventRecord(ev, run_stream)) != hipSuccess) return hc_.fail(e, "event record");
    if ((e = hipStreamWaitEvent(hc_.ctx->s_copy, ev, 0)) != hipSuccess) hc_.fail(e, "wait event");
}

void DayFeed::arrive(float* d_dst, const float* host, size_t rows, size_t N, size_t c0, size_t c1, hipStream_t run_stream)
{
    if (!hc_.ok()) return;
    DeviceContext* ctx = hc_.ctx;
    // (through the pinned pieces on the copy stream: the runtime's own path page-locks a host region it has not
    // seen before -- a new day is a new array -- at a third of the rate, context.h)
    hipError_t e = staged_upload_rows(ctx, d_dst, host, rows, N, c0, c1, ctx->s_copy);
    if (e != hipSuccess) return hc_.fail(e, what_);
    hipEvent_t ev = next_event();
    if ((e = hipEventRecord(ev, ctx->s_copy)) != hipSuccess) return hc_.fail(e, "event record");
    if ((e = hipStreamWaitEvent(run_stream, ev, 0)) != hipSuccess) return hc_.fail(e, "wait event");
    if (c1 == N && !published_) {
        published_ = true;              // the whole day is on its way: the other devices may copy it
        if ((e = fanout_publish(hc_.fan, ctx, d_dst, ctx->s_copy)) != hipSuccess) hc_.fail(e, "event record");
    }
}

int guarded_failure(const char* name, const char* what)
{
    copy_pool_quiesce();      // (no pool thread may still read the caller's arrays)
    if (what) set_error("%s: exception: %s", name, what);
    else set_error("%s: unknown exception", name);
    return -3;
}

}  // namespace bpmf
