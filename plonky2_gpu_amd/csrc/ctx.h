// ctx.h — what the sources behind the extern "C" boundary share about a `void *ctx`: its streams, its state (ctx.hip), the
// per-device tables and coset-table cache, and the GlError helpers. Internal: nothing here is exported (exports.map).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/plonky2_hip.h"
#include "gate_jit.h"
#include "ntt.h"

namespace plonky2_hip {

struct Streams {  // == CudaInnerContext {stream, stream2} (plonky2/src/fri/oracle.rs:43-47)
    hipStream_t stream;
    hipStream_t stream2;
};

inline Streams *S(void *ctx) { return static_cast<Streams *>(ctx); }
inline hipStream_t ctx_stream(void *ctx) { return S(ctx)->stream; }  // the context's first stream

GlError ok();
GlError fail(int code, const std::string &msg);
GlError hip_fail(hipError_t e, const char *what);

#define HIP_TRY(expr)                                      \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(_e, #expr);  \
    } while (0)

#define TRY(expr)                    \
    do {                             \
        GlError _e = (expr);         \
        if (_e.code != 0) return _e; \
    } while (0)

// Per-device table registry (twiddles are data-independent, a few hundred KiB).
struct CosetEntry {
    CosetTables ct;
    uint64_t last_use = 0;
    uint32_t pins = 0;  // callers between get_coset_tables() and the end of their enqueues
};
struct DeviceState {
    bool have_tables = false;
    NttTables tables;              // twl / twh only: the workspace belongs to a context (CtxState)
    std::list<CosetEntry> cosets;  // LRU cache keyed by (log_n, rate_bits, shift); addresses are stable
    uint64_t coset_tick = 0;
    GateKernel *ed25519_kernel = nullptr;  // the reference symbol compute_quotient_polys' circuit, built on first use
    std::mutex ref_mu;                     // compute_quotient_polys calls on this device take turns (one kernel object, one staging buffer)
    uint64_t *ref_staging = nullptr;       // its column-major staging copy of the three leaf-major inputs
    uint64_t ref_staging_elems = 0;
    bool ref_staging_owned = false;        // false: handed over by gl_reference_quotient_set_staging
};
DeviceState &device_state(int dev);
hipError_t device_tables(int dev, const NttTables **out);  // the device's tables, created on first use

// Everything mutable that a call touches besides the caller's buffers belongs to the CONTEXT: the workspace of the natural-order
// multi-pass transforms (also the scans' totals, the openings' partial sums, the transcript's state), the event pair, the
// low-priority hashing stream of the pipelined commit and its events. Two contexts on one device therefore share only read-only
// tables, and their calls run concurrently — two proofs in flight fill each other's latency-bound phases (transcript, small tree
// layers, openings). Keyed by the context's first stream, so that a caller-built {stream, stream2} pair (the reference's
// CudaInnerContext, fri/oracle.rs:43-47) gets its state on first use; gl_ctx_destroy / gl_ctx_release give it back.
struct CtxState {
    int dev = 0;
    NttTables tb;  // twl / twh of the device, scratch of this context
    bool scratch_owned = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t hash_stream = nullptr;     // pipelined commit: leaf hashing trails the LDE on this lower-priority stream
    std::vector<hipEvent_t> chunk_events;  //   one event per column chunk + one for "tree done"
    bool have_pih = false;                 // gl_reference_set_public_inputs_hash_ctx
    uint64_t pih[4] = {0, 0, 0, 0};
};

// The state of `ctx` on the current device (DeviceCall has made the context's device current), created on first use.
hipError_t ctx_state(void *ctx, CtxState **out);
void ctx_state_release(void *ctx);  // the caller has synchronised the context's streams
hipError_t get_tables(void *ctx, const NttTables **out);
hipError_t get_events(void *ctx, hipEvent_t *a, hipEvent_t *b);
hipError_t get_hash_stream(void *ctx, hipStream_t *hs, std::vector<hipEvent_t> **events, size_t need);

// Holds one cache entry pinned while its owner enqueues the kernels that read it; an unpinned entry may be
// evicted, and eviction synchronises the device first, so work already enqueued on any stream is safe too.
class CosetLease {
public:
    CosetLease() = default;
    CosetLease(const CosetLease &) = delete;
    CosetLease &operator=(const CosetLease &) = delete;
    ~CosetLease() { release(); }
    const CosetTables &operator*() const { return entry_->ct; }
    void acquire(CosetEntry *e) {  // the registry's lock held
        release_locked();
        entry_ = e;
        e->pins++;
    }
    void release();

private:
    void release_locked() {
        if (entry_) entry_->pins--;
        entry_ = nullptr;
    }
    CosetEntry *entry_ = nullptr;
};

hipError_t get_coset_tables(uint32_t log_n, uint32_t rate_bits, uint64_t shift, hipStream_t stream, CosetLease *out);

// Device of a context = device of its first stream; makes it the calling thread's current device.
bool ctx_device(void *ctx, int *dev);

// Every entry point that takes a ctx runs on the device its context's streams belong to, whatever device the calling thread
// has current: tables, workspace and every allocation made inside the call follow it (a context created on device 1 and used
// from a thread whose current device is still 0 must not touch device 0's state). The device comes from the stream itself, so
// a caller-built {stream, stream2} pair (the reference's CudaInnerContext) works too. Nothing is locked and nothing is ordered
// across contexts (up to round 5 the workspace and the event pair existed once per device and contexts took turns): a context
// is used by one host thread at a time, different contexts by different threads at the same time; data shared between two
// contexts is the caller's to order, as with any two streams.
class DeviceCall {
public:
    explicit DeviceCall(void *ctx) {
        int dev = 0;
        if (!ctx_device(ctx, &dev)) (void)hipGetLastError();
    }
    DeviceCall(const DeviceCall &) = delete;
    DeviceCall &operator=(const DeviceCall &) = delete;
};

// makes the device of `ctx` current and returns its tables and workspace (the provers' host logic, prove.hip and stark_prove.hip)
hipError_t ctx_tables(void *ctx, const NttTables **out);

}  // namespace plonky2_hip
