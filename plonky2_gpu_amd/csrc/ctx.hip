// ctx.hip — owns the per-device and per-context state behind every `void *ctx` (ctx.h).
#include "ctx.h"

#include <map>

#include <string.h>

namespace plonky2_hip {

GlError ok() { return GlError{0, nullptr}; }

GlError fail(int code, const std::string &msg) { return GlError{code, strdup(msg.c_str())}; }

GlError hip_fail(hipError_t e, const char *what) {
    return fail((int)e, std::string(what) + ": " + hipGetErrorString(e));
}

namespace {

constexpr size_t COSET_CACHE_ENTRIES = 64;  // a prover uses a handful (one shift, a few sizes); 80 KiB each at 2^18 x 8
std::mutex g_mu;
DeviceState g_dev[64];
std::map<std::pair<int, hipStream_t>, CtxState *> g_ctx;  // g_mu; keyed by (device, first stream): the null stream exists on every device

hipError_t device_tables_locked(int dev, const NttTables **out) {  // g_mu held
    DeviceState &st = g_dev[dev & 63];
    if (!st.have_tables) {
        hipError_t e = ntt_tables_create(&st.tables);
        if (e != hipSuccess) return e;
        st.have_tables = true;
    }
    *out = &st.tables;
    return hipSuccess;
}

}  // namespace

DeviceState &device_state(int dev) { return g_dev[dev & 63]; }

hipError_t device_tables(int dev, const NttTables **out) {
    std::lock_guard<std::mutex> lk(g_mu);
    return device_tables_locked(dev, out);
}

hipError_t ctx_state(void *ctx, CtxState **out) {
    if (!ctx) return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ctx.find({dev, S(ctx)->stream});
    if (it == g_ctx.end()) {
        const NttTables *dt;
        e = device_tables_locked(dev, &dt);
        if (e != hipSuccess) return e;
        CtxState *c = new CtxState();
        c->dev = dev;
        c->tb = *dt;
        c->tb.scratch_elems = NTT_SCRATCH_ELEMS;
        e = hipMalloc(&c->tb.scratch, NTT_SCRATCH_ELEMS * sizeof(uint64_t));
        if (e != hipSuccess) {
            delete c;
            return e;
        }
        c->scratch_owned = true;
        it = g_ctx.emplace(std::make_pair(dev, S(ctx)->stream), c).first;
    }
    *out = it->second;
    return hipSuccess;
}

void ctx_state_release(void *ctx) {
    if (!ctx) return;
    CtxState *c = nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;  // gl_ctx_release has made the context's device current
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_ctx.find({dev, S(ctx)->stream});
        if (it == g_ctx.end()) return;
        c = it->second;
        g_ctx.erase(it);
    }
    if (c->scratch_owned && c->tb.scratch) (void)hipFree(c->tb.scratch);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->hash_stream) {
        (void)hipStreamSynchronize(c->hash_stream);
        (void)hipStreamDestroy(c->hash_stream);
    }
    for (hipEvent_t e : c->chunk_events) (void)hipEventDestroy(e);
    delete c;
}

hipError_t get_tables(void *ctx, const NttTables **out) {
    CtxState *c;
    hipError_t e = ctx_state(ctx, &c);
    if (e != hipSuccess) return e;
    *out = &c->tb;
    return hipSuccess;
}

hipError_t get_events(void *ctx, hipEvent_t *a, hipEvent_t *b) {
    CtxState *c;
    hipError_t e = ctx_state(ctx, &c);
    if (e != hipSuccess) return e;
    if (!c->ev[0]) {  // only the context's own caller thread gets here
        for (int i = 0; i < 2; i++) {
            e = hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
    }
    *a = c->ev[0];
    *b = c->ev[1];
    return hipSuccess;
}

hipError_t get_hash_stream(void *ctx, hipStream_t *hs, std::vector<hipEvent_t> **events, size_t need) {
    CtxState *c;
    hipError_t e = ctx_state(ctx, &c);
    if (e != hipSuccess) return e;
    if (!c->hash_stream) {
        int lo = 0, hi = 0;  // numerically lower = higher priority; the hashing takes the LOWEST so that the LDE runs ahead
        e = hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (e != hipSuccess) return e;
        e = hipStreamCreateWithPriority(&c->hash_stream, hipStreamNonBlocking, lo);
        if (e != hipSuccess) return e;
    }
    while (c->chunk_events.size() < need) {
        hipEvent_t ev;
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        c->chunk_events.push_back(ev);
    }
    *hs = c->hash_stream;
    *events = &c->chunk_events;
    return hipSuccess;
}

void CosetLease::release() {
    if (!entry_) return;
    std::lock_guard<std::mutex> lk(g_mu);
    release_locked();
}

hipError_t get_coset_tables(uint32_t log_n, uint32_t rate_bits, uint64_t shift, hipStream_t stream, CosetLease *out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceState &st = g_dev[dev & 63];
    for (auto &c : st.cosets)
        if (c.ct.log_n == log_n && c.ct.rate_bits == rate_bits && c.ct.shift == shift) {
            c.last_use = ++st.coset_tick;
            out->acquire(&c);
            return hipSuccess;
        }
    // Miss on a full cache: drop the least recently used entry nobody holds. If every entry is pinned
    // (more concurrent callers than entries) the cache grows instead: a full cache is never an error.
    while (st.cosets.size() >= COSET_CACHE_ENTRIES) {
        auto victim = st.cosets.end();
        for (auto it = st.cosets.begin(); it != st.cosets.end(); ++it)
            if (it->pins == 0 && (victim == st.cosets.end() || it->last_use < victim->last_use)) victim = it;
        if (victim == st.cosets.end()) break;
        e = hipDeviceSynchronize();  // kernels enqueued by earlier, already-returned calls may still read it
        if (e != hipSuccess) return e;
        coset_tables_destroy(&victim->ct);
        st.cosets.erase(victim);
    }
    CosetEntry entry;
    e = coset_tables_create(&entry.ct, log_n, rate_bits, shift, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // built on `stream`; other streams may use them later
    if (e != hipSuccess) {
        coset_tables_destroy(&entry.ct);
        return e;
    }
    entry.last_use = ++st.coset_tick;
    st.cosets.push_back(entry);
    out->acquire(&st.cosets.back());
    return hipSuccess;
}

bool ctx_device(void *ctx, int *dev) {
    if (ctx && S(ctx)->stream) {
        hipDevice_t d;
        if (hipStreamGetDevice(S(ctx)->stream, &d) != hipSuccess) return false;
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) return false;
        if (cur != (int)d && hipSetDevice((int)d) != hipSuccess) return false;
        *dev = (int)d;
        return true;
    }
    return hipGetDevice(dev) == hipSuccess;
}

hipError_t ctx_tables(void *ctx, const NttTables **out) {
    if (!ctx) return hipErrorInvalidValue;
    DeviceCall device_call(ctx);
    return get_tables(ctx, out);
}

}  // namespace plonky2_hip
