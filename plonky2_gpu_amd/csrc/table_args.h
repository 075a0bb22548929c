// table_args.h — what the tables' C entry points (<table>.hip) share before and around their launches (host code only): the
// refusals of a trace's shape with their message texts, the overlap test of two device ranges, the one read-back of a call's
// status words, and the event clock of the gl_debug_*_stage_ms calls. Each entry point keeps the ORDER of its refusals.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace plonky2_hip {

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte? A null pointer or an empty range overlaps nothing.
inline bool bytes_overlap(const void *a, uint64_t a_bytes, const void *b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// the bytes from the first word of a trace [columns][pitch stride] of n rows to its last
constexpr uint64_t trace_bytes(uint32_t columns, uint64_t stride, uint64_t n) { return ((uint64_t)(columns - 1) * stride + n) * 8; }

// The refusals every table states in the same words; empty: nothing to refuse.
inline std::string degree_bits_error(uint32_t degree_bits, uint32_t max_degree_bits) {
    if (degree_bits == 0 || degree_bits > max_degree_bits) return "degree_bits must be in 1 ..= " + std::to_string(max_degree_bits);
    return "";
}
inline std::string trace_stride_error(uint64_t trace_stride, uint64_t n) {
    if (trace_stride < n) return "trace_stride smaller than 2^degree_bits: the columns would overlap";
    if (trace_stride > (1ull << 40)) return "trace_stride too large";
    return "";
}
inline std::string scratch_alignment_error(const void *d_scratch) { return (uintptr_t)d_scratch & 15 ? "d_scratch must be 16-byte aligned" : ""; }

// what the device decided, copied to the host on `stream`, and the stream awaited: a call's one host wait
inline hipError_t read_status(void *dst, const void *src, size_t bytes, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}

// N events on one stream for a measured call: mark(k) between the enqueues, elapsed() after the caller has awaited the stream.
// `created` is the first error of the constructor; the events are destroyed with the clock.
template <int N>
struct StageClock {
    hipEvent_t ev[N] = {};
    hipStream_t stream;
    hipError_t created = hipSuccess;
    explicit StageClock(hipStream_t s) : stream(s) {
        for (hipEvent_t &x : ev)
            if (created == hipSuccess) created = hipEventCreate(&x);
    }
    ~StageClock() {
        for (hipEvent_t x : ev)
            if (x) (void)hipEventDestroy(x);
    }
    StageClock(const StageClock &) = delete;
    StageClock &operator=(const StageClock &) = delete;
    hipError_t mark(int k) { return hipEventRecord(ev[k], stream); }
    hipError_t elapsed(float *ms, int from, int to) { return hipEventElapsedTime(ms, ev[from], ev[to]); }
};

}  // namespace plonky2_hip
