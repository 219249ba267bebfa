// The scope of one host-pointer call (bpmf_mf_run, bpmf_bp_run, their shares of the *_multi forms,
// bpmf_find_similar_sources) on its device's context (context.h), and the day of data arriving in it.  Every
// ordering rule of such a call lives here, once:
//   - the call binds its device, takes the device's context and holds its call mutex from start to finish;
//   - it adopts its part in a multi-device hand-over of the day BEHIND that lock;
//   - at its end (HostCall::finish): streams drained, then the copy pool quiesced, then the hand-over settled,
//     then the working set trimmed;
//   - nothing leaves it as an exception (guarded()).
#pragma once
#include "context.h"

#include <exception>

namespace bpmf {

class HostCall {
public:
    // `name`: the entry point, as it appears in error texts.  `fan`: the caller's part in a hand-over of the day
    // (a non-participant for a single-device call); it is settled by finish(), and by its owner if this
    // constructor fails.  A failed construction leaves !ok(): return rc.
    HostCall(const char* name, int device, FanoutScope& fan);
    ~HostCall() { finish(); }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

    // The working set: add() gives the offset (256-byte aligned) of the next `bytes` -- 0 bytes take no room --,
    // reserve() then the base of the device block and two pinned pieces of at least `pinned_bytes` each (0: the
    // call stages nothing); nullptr with rc set on failure.  The time goes to HostCallStats::reserve_ms.
    size_t add(size_t bytes)
    {
        const size_t o = align_up(total_, 256);
        total_ = o + bytes;
        return o;
    }
    char* reserve(size_t pinned_bytes);

    bool ok() const { return rc == 0; }
    // status -2 and "<name>: <what> failed: <error string>"; the first error keeps its text
    void fail(hipError_t e, const char* what);
    // a status from elsewhere (a *_dev call that has set its own error text); the first one stays
    void note(int status) { if (!rc) rc = status; }

    // The end of the call, once (the destructor runs it if nobody has): see host_call.hip.
    void finish();

    int rc = 0;
    DeviceContext* ctx = nullptr;
    FanoutScope& fan;
    const double t0;                    // host_now_ms() at the start of the call
    hipStream_t also_drain = nullptr;   // a further stream the call used (a plan's side stream)
    double wait_since = 0.0;            // != 0: device_wait_ms = from here to the end of the drain

private:
    const char* name_;
    DeviceGuard bind_;
    std::unique_lock<std::mutex> lock_;
    size_t total_ = 0;
    bool finished_ = false;
};

// The day of data (rows, N) float32 of a call on its way to the device: from the first device of a multi-device
// call, or from the host -- in one go or in pieces on the copy stream while kernels run on the pieces that have
// arrived.  What is computed behind a piece is the caller's business.  Errors go to HostCall::fail.
class DayFeed {
public:
    // `what`: the name of the upload in error texts ("H2D data")
    DayFeed(HostCall& call, const char* what) : hc_(call), what_(what) {}
    // A PEER of a hand-over that got published: the device-to-device copy, enqueued on `stream` (true; a failure is
    // in the call's status).  false: not a peer, or the hand-over was cancelled or refused: upload from the host.
    bool from_peer(void* d_dst, size_t bytes, hipStream_t stream);
    // the copy stream waits for what `run_stream` has enqueued so far
    void fork_from(hipStream_t run_stream);
    // rows x [c0, c1) through the pinned pieces on the copy stream (staged_upload_rows); `run_stream` waits for
    // them; behind the last piece (c1 == N) a SOURCE publishes the day to its peers, once.
    void arrive(float* d_dst, const float* host, size_t rows, size_t N, size_t c0, size_t c1, hipStream_t run_stream);

private:
    hipEvent_t next_event();            // the ring of DeviceContext::ev_chunk
    HostCall& hc_;
    const char* what_;
    unsigned n_events_ = 0;
    bool published_ = false;
};

// The exception barrier of the C boundary: nothing may cross it as an exception (std::bad_alloc from the host-side
// planning, a std::system_error); it becomes status -3 with its text.
int guarded_failure(const char* name, const char* what);
template <class F>
int guarded(const char* name, F&& f)
{
    try {
        return f();
    } catch (const std::exception& e) {
        return guarded_failure(name, e.what());
    } catch (...) {
        return guarded_failure(name, nullptr);
    }
}

// The host-pointer calls themselves with the caller's part in a hand-over as an argument: bpmf_mf_run / bpmf_bp_run
// pass nobody, *_run_multi the participant of the block (multi.hip).  bp_run_host with `defer_finish` is one device's
// share of bpmf_bp_run_multi under option bp.compat_first_computed -- the share keeps -inf where it computed no beam,
// and the host finishes (0, first id) after the merge of all shares (a finished share could not be told from a
// real 0).
int mf_run_host(const float* templates, const int32_t* moveouts, const float* weights, const float* data, size_t step,
                size_t L, size_t N, size_t T, size_t S, size_t C, size_t n_corr, int network_sum, int flags, int device,
                float* cc_out, FanoutScope& fan);
int bp_run_host(const float* features, const int32_t* moveouts, const float* w_phases, const float* w_sources,
                size_t N, size_t K, size_t S, size_t C, size_t P, int out_of_bounds, int reduce, int device,
                float* beam_out, int32_t* arg_out, bool defer_finish, FanoutScope& fan);

}  // namespace bpmf
