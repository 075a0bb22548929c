// lookup.hip — the lookup columns of a STARK trace on the device.
//
// (a) lookup_sort_canonical: a keys-only LSD radix sort of 64-bit keys with 8-bit digits. One first read of the keys writes their
//     canonical values and takes the histogram of all eight digits; a digit in which every key agrees costs nothing more (its pass
//     is skipped: the kernels of that pass return at once, decided on the device, the host never waits). A pass is a per-tile
//     histogram in LDS, one exclusive scan of the tile histograms in digit-major order, and a stable scatter: a wave ranks its 64
//     keys of a round among themselves with eight __ballot masks, the rounds of a wave and the four waves of a tile through counters
//     in LDS.
// (b) lookup_permuted_cols: permuted_cols (evm/src/lookup.rs:67-131) without its serial merge; DESIGN.md §3.7.2 derives the
//     decomposition. With S, T the sorted inputs and table: binary searches flag the unmatched inputs (pops, or post-loop from
//     header[0] on) and the unused table values (pushes); one scan of the flags ranks them and merges them into events by value; one
//     scan of the events under (sum, min) gives every event its stack level and tells the pops on an empty stack; a stable sort of
//     level << 32 | event by the level's digits puts each pop behind the push it takes.
#include <string.h>

#include "lookup.h"

namespace plonky2_hip {

namespace {

constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull;
constexpr uint32_t T = LOOKUP_THREADS;
constexpr uint32_t ITEMS = 8;
static_assert(LOOKUP_SORT_TILE == T * ITEMS && LOOKUP_SCAN_BLOCK == T * ITEMS, "eight elements per thread");
constexpr uint32_t POP = 0x80000000u;
// header words
constexpr uint32_t H_POST_START = 0, H_NUM_DEFERRED = 1, H_PLAN = 16, H_NEEDS_COPY = H_PLAN + 8, H_DIGITS = 64;
static_assert((H_DIGITS + 8 * 256) * 4 <= LOOKUP_HEADER_WORDS * 8, "the header holds the digit histogram");

// ---------------------------------------------------------------- prefix scans
struct AddU32 {
    typedef uint32_t type;
    static __device__ uint32_t identity() { return 0; }
    static __device__ uint32_t op(uint32_t a, uint32_t b) { return a + b; }
};
struct AddU64 {
    typedef uint64_t type;
    static __device__ uint64_t identity() { return 0; }
    static __device__ uint64_t op(uint64_t a, uint64_t b) { return a + b; }
};
// the running sum of +1 / -1 and min(0, its running minimum); (0, 0) is neutral for elements with min <= 0 and min <= sum
struct SumMin {
    int32_t sum, min;
};
struct SumMinOp {
    typedef SumMin type;
    static __device__ SumMin identity() { return SumMin{0, 0}; }
    static __device__ SumMin op(SumMin a, SumMin b) {
        int32_t m = a.sum + b.min;
        return SumMin{a.sum + b.sum, a.min < m ? a.min : m};
    }
};
static_assert(sizeof(SumMin) == 8, "a scan element is one word");

template <typename V>
__device__ __forceinline__ V shfl_up_any(V v, uint32_t delta) {
    if constexpr (sizeof(V) == 4) {
        uint32_t u;
        memcpy(&u, &v, 4);
        u = __shfl_up(u, delta);
        memcpy(&v, &u, 4);
    } else {
        unsigned long long u;
        memcpy(&u, &v, 8);
        u = __shfl_up(u, delta);
        memcpy(&v, &u, 8);
    }
    return v;
}

// exclusive prefix of `v` over the workgroup's threads in thread order and the workgroup's total; `lds` holds one value per wave.
// The caller synchronises before `lds` is used again.
template <typename Op>
__device__ __forceinline__ typename Op::type block_exclusive(typename Op::type v, typename Op::type *lds, typename Op::type *total) {
    typedef typename Op::type V;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        V o = shfl_up_any(v, d);
        if (lane >= d) v = Op::op(o, v);
    }
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    V excl = shfl_up_any(v, 1);
    if (lane == 0) excl = Op::identity();
    V before = Op::identity(), all = Op::identity();
    for (uint32_t w = 0; w < T / 64; ++w) {
        if (w < wave) before = Op::op(before, lds[w]);
        all = Op::op(all, lds[w]);
    }
    *total = all;
    return Op::op(before, excl);
}

// `gate`: null, or a word whose bit 0 says whether this launch has anything to do (the plan of a radix pass)
template <typename Op>
__global__ __launch_bounds__(T) void scan_reduce(const typename Op::type *data, uint64_t len, typename Op::type *totals, const uint32_t *gate) {
    typedef typename Op::type V;
    if (gate && !(*gate & 1)) return;
    __shared__ V lds[T / 64];
    const uint64_t base = (uint64_t)blockIdx.x * LOOKUP_SCAN_BLOCK + threadIdx.x * ITEMS;
    V acc = Op::identity();
    for (uint32_t j = 0; j < ITEMS; ++j)
        if (base + j < len) acc = Op::op(acc, data[base + j]);
    V total;
    block_exclusive<Op>(acc, lds, &total);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// one workgroup: the block totals become their exclusive prefixes
template <typename Op>
__global__ __launch_bounds__(T) void scan_totals(typename Op::type *totals, uint64_t num_blocks, const uint32_t *gate) {
    typedef typename Op::type V;
    if (gate && !(*gate & 1)) return;
    __shared__ V lds[T / 64];
    V carry = Op::identity();
    for (uint64_t base = 0; base < num_blocks; base += T) {
        const uint64_t i = base + threadIdx.x;
        V v = i < num_blocks ? totals[i] : Op::identity(), total;
        V excl = block_exclusive<Op>(v, lds, &total);
        if (i < num_blocks) totals[i] = Op::op(carry, excl);
        carry = Op::op(carry, total);
        __syncthreads();
    }
}

template <typename Op, bool INCLUSIVE>
__global__ __launch_bounds__(T) void scan_apply(typename Op::type *data, uint64_t len, const typename Op::type *totals, const uint32_t *gate) {
    typedef typename Op::type V;
    if (gate && !(*gate & 1)) return;
    __shared__ V lds[T / 64];
    const uint64_t base = (uint64_t)blockIdx.x * LOOKUP_SCAN_BLOCK + threadIdx.x * ITEMS;
    V x[ITEMS], acc = Op::identity();
    for (uint32_t j = 0; j < ITEMS; ++j) {
        x[j] = base + j < len ? data[base + j] : Op::identity();
        acc = Op::op(acc, x[j]);
    }
    V total;
    V run = Op::op(totals[blockIdx.x], block_exclusive<Op>(acc, lds, &total));
    for (uint32_t j = 0; j < ITEMS; ++j) {
        V next = Op::op(run, x[j]);
        if (base + j < len) data[base + j] = INCLUSIVE ? next : run;
        run = next;
    }
}

// in place; `totals` holds ceil(len / LOOKUP_SCAN_BLOCK) elements
template <typename Op, bool INCLUSIVE>
hipError_t scan_in_place(typename Op::type *data, uint64_t len, void *totals, const uint32_t *gate, hipStream_t stream) {
    typedef typename Op::type V;
    const uint64_t blocks = (len + LOOKUP_SCAN_BLOCK - 1) / LOOKUP_SCAN_BLOCK;
    scan_reduce<Op><<<dim3((uint32_t)blocks), dim3(T), 0, stream>>>(data, len, static_cast<V *>(totals), gate);
    scan_totals<Op><<<dim3(1), dim3(T), 0, stream>>>(static_cast<V *>(totals), blocks, gate);
    scan_apply<Op, INCLUSIVE><<<dim3((uint32_t)blocks), dim3(T), 0, stream>>>(data, len, static_cast<const V *>(totals), gate);
    return hipGetLastError();
}

// ---------------------------------------------------------------- the radix sort
// The first read: out[i] = canonical(in[i]) (or in[i] itself for keys that are no field elements) and the histogram of the digits
// first_digit .. 7 of all keys, added into header[H_DIGITS ..] (zeroed before).
__global__ __launch_bounds__(T) void sort_first_read(const uint64_t *in, uint64_t *out, uint64_t n, int canonicalise, uint32_t first_digit,
                                                     uint32_t *header) {
    __shared__ uint32_t hist[8 * 256];
    for (uint32_t i = threadIdx.x; i < 8 * 256; i += T) hist[i] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * LOOKUP_SORT_TILE;
    for (uint32_t j = 0; j < ITEMS; ++j) {
        const uint64_t i = base + j * T + threadIdx.x;
        if (i < n) {
            uint64_t v = in[i];
            if (canonicalise) v = v >= GL_P ? v - GL_P : v;
            out[i] = v;
            for (uint32_t d = first_digit; d < 8; ++d) atomicAdd(&hist[d * 256 + ((v >> (8 * d)) & 255)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 8 * 256; i += T)
        if (hist[i]) atomicAdd(&header[H_DIGITS + i], hist[i]);
}

// One workgroup. plan[d]: bit 0 set where pass d runs (some two keys differ in digit d), bit 1 set where it reads the other buffer
// (`tmp`) and writes `out`; plan[8]: the sorted keys ended in `tmp`.
__global__ __launch_bounds__(T) void sort_plan(uint64_t n, uint32_t first_digit, uint32_t *header) {
    __shared__ uint32_t uniform[8];
    if (threadIdx.x < 8) uniform[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t d = first_digit; d < 8; ++d)
        if (header[H_DIGITS + d * 256 + threadIdx.x] == n) uniform[d] = 1;  // at most one bin holds all n keys
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t passes = 0;
        for (uint32_t d = 0; d < 8; ++d) {
            const bool runs = d >= first_digit && !uniform[d];
            header[H_PLAN + d] = runs ? 1u | ((passes & 1) << 1) : 0u;
            passes += runs;
        }
        header[H_NEEDS_COPY] = passes & 1;
    }
}

// tile_hist[digit value][tile]
__global__ __launch_bounds__(T) void sort_tile_histogram(const uint64_t *out, const uint64_t *tmp, uint64_t n, uint32_t digit, uint32_t *tile_hist,
                                                         uint32_t num_tiles, const uint32_t *header) {
    const uint32_t plan = header[H_PLAN + digit];
    if (!(plan & 1)) return;
    const uint64_t *src = (plan & 2) ? tmp : out;
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * LOOKUP_SORT_TILE;
    for (uint32_t j = 0; j < ITEMS; ++j) {
        const uint64_t i = base + j * T + threadIdx.x;
        if (i < n) atomicAdd(&hist[(src[i] >> (8 * digit)) & 255], 1u);
    }
    __syncthreads();
    tile_hist[(uint64_t)threadIdx.x * num_tiles + blockIdx.x] = hist[threadIdx.x];
}

// tile_offsets: the exclusive scan of tile_hist. Wave w of a tile takes its keys [512 w, 512 w + 512) in eight rounds of 64; a key
// goes to tile_offsets[digit][tile] + (keys of that digit in earlier waves) + (in earlier rounds of its wave) + (in lower lanes of
// its round): the order of equal digits is kept.
__global__ __launch_bounds__(T) void sort_scatter(uint64_t *out, uint64_t *tmp, uint64_t n, uint32_t digit, const uint32_t *tile_offsets,
                                                  uint32_t num_tiles, const uint32_t *header) {
    const uint32_t plan = header[H_PLAN + digit];
    if (!(plan & 1)) return;
    const uint64_t *src = (plan & 2) ? tmp : out;
    uint64_t *dst = (plan & 2) ? out : tmp;
    __shared__ uint32_t counts[T / 64][256];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t w = 0; w < T / 64; ++w) counts[w][threadIdx.x] = 0;
    __syncthreads();
    volatile uint32_t *mine = counts[wave];
    const uint64_t base = (uint64_t)blockIdx.x * LOOKUP_SORT_TILE + wave * (64 * ITEMS) + lane;
    uint64_t key[ITEMS];
    uint32_t rank[ITEMS];
#pragma unroll
    for (uint32_t r = 0; r < ITEMS; ++r) {
        const uint64_t i = base + r * 64;
        const bool valid = i < n;
        key[r] = valid ? src[i] : 0;
        const uint32_t d = (uint32_t)(key[r] >> (8 * digit)) & 255;
        uint64_t same = __ballot(valid);  // the lanes of this round that hold the same digit
#pragma unroll
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1;
            const uint64_t ones = __ballot(valid && one);
            same &= one ? ones : ~ones;
        }
        const uint32_t below = __popcll(same & ((1ull << lane) - 1)), group = __popcll(same);
        uint32_t before = 0;
        if (valid) before = mine[d];
        __builtin_amdgcn_wave_barrier();
        if (valid && below + 1 == group) mine[d] = before + group;  // the group's highest lane
        __builtin_amdgcn_wave_barrier();
        rank[r] = before + below;
    }
    __syncthreads();
    {
        uint32_t run = tile_offsets[(uint64_t)threadIdx.x * num_tiles + blockIdx.x];  // thread t: digit value t
        for (uint32_t w = 0; w < T / 64; ++w) {
            const uint32_t c = counts[w][threadIdx.x];
            counts[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < ITEMS; ++r) {
        const uint64_t i = base + r * 64;
        if (i < n) {
            const uint32_t d = (uint32_t)(key[r] >> (8 * digit)) & 255;
            dst[counts[wave][d] + rank[r]] = key[r];
        }
    }
}

__global__ __launch_bounds__(T) void sort_copy_back(uint64_t *out, const uint64_t *tmp, uint64_t n, const uint32_t *header) {
    if (!header[H_NEEDS_COPY]) return;
    const uint64_t i = (uint64_t)blockIdx.x * T + threadIdx.x;
    if (i < n) out[i] = tmp[i];
}

// stable sort of n keys by their digits first_digit .. 7; canonicalise: the keys are field elements in any representation
hipError_t radix_sort(const uint64_t *in, uint64_t *out, uint64_t n, int canonicalise, uint32_t first_digit, const LookupScratch &s,
                      hipStream_t stream) {
    const uint32_t tiles = (uint32_t)((n + LOOKUP_SORT_TILE - 1) / LOOKUP_SORT_TILE);
    hipError_t e = hipMemsetAsync(s.header + H_DIGITS, 0, 8 * 256 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    sort_first_read<<<dim3(tiles), dim3(T), 0, stream>>>(in, out, n, canonicalise, first_digit, s.header);
    sort_plan<<<dim3(1), dim3(T), 0, stream>>>(n, first_digit, s.header);
    for (uint32_t d = first_digit; d < 8; ++d) {
        sort_tile_histogram<<<dim3(tiles), dim3(T), 0, stream>>>(out, s.tmp, n, d, s.tile_hist, tiles, s.header);
        e = scan_in_place<AddU32, false>(s.tile_hist, 256ull * tiles, s.totals, s.header + H_PLAN + d, stream);
        if (e != hipSuccess) return e;
        sort_scatter<<<dim3(tiles), dim3(T), 0, stream>>>(out, s.tmp, n, d, s.tile_hist, tiles, s.header);
    }
    sort_copy_back<<<dim3((uint32_t)((n + T - 1) / T)), dim3(T), 0, stream>>>(out, s.tmp, n, s.header);
    return hipGetLastError();
}

// ---------------------------------------------------------------- permuted_cols
__device__ __forceinline__ uint32_t lower_bound(const uint64_t *a, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t upper_bound(const uint64_t *a, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// flags[i]: bit 0: s[i] is an unmatched input below the last table value (a pop); bit 32: t[i] is an unused table value (a push).
// A matched input takes its own value. The unmatched inputs from header[H_POST_START] on are the post-loop ones.
__global__ __launch_bounds__(T) void lookup_classify(const uint64_t *s, const uint64_t *t, uint32_t n, uint64_t *permuted_table, uint64_t *flags,
                                                     uint32_t *header) {
    const uint32_t i = blockIdx.x * T + threadIdx.x;
    if (i >= n) return;
    const uint64_t last = t[n - 1];
    uint64_t f = 0, v = s[i];
    if (i - lower_bound(s, n, v) < upper_bound(t, n, v) - lower_bound(t, n, v)) permuted_table[i] = v;
    else if (v < last) f = 1;
    v = t[i];
    if (i - lower_bound(t, n, v) >= upper_bound(s, n, v) - lower_bound(s, n, v)) f |= 1ull << 32;
    flags[i] = f;
    if (i == 0) {
        flags[n] = 0;
        const uint32_t lo = lower_bound(s, n, last), in_s = upper_bound(s, n, last) - lo, in_t = n - lower_bound(t, n, last);
        header[H_POST_START] = lo + (in_s < in_t ? in_s : in_t);
    }
}

// ranks: the exclusive scan of the flags over n + 1 elements. Events are ordered by value (a pop and a push never share one): event
// k gets its source and its element of the (sum, min) scan; the elements behind the last event are neutral. 2 n threads.
__global__ __launch_bounds__(T) void lookup_events(const uint64_t *s, const uint64_t *t, uint32_t n, const uint64_t *ranks, uint32_t *events,
                                                   SumMin *walk) {
    const uint32_t g = blockIdx.x * T + threadIdx.x;
    if (g >= 2 * n) return;
    const uint32_t num_events = (uint32_t)ranks[n] + (uint32_t)(ranks[n] >> 32);
    if (g >= num_events) walk[g] = SumMin{0, 0};
    if (g >= n) return;
    const uint64_t mine = ranks[g], f = ranks[g + 1] - mine;
    if (f & 1) {  // pops before it + pushes of a smaller value
        const uint32_t k = (uint32_t)mine + (uint32_t)(ranks[lower_bound(t, n, s[g])] >> 32);
        events[k] = g | POP;
        walk[k] = SumMin{-1, -1};
    }
    if (f >> 32) {  // pushes before it + pops of a smaller value
        const uint32_t k = (uint32_t)(mine >> 32) + (uint32_t)ranks[lower_bound(s, n, t[g])];
        events[k] = g;
        walk[k] = SumMin{1, 0};
    }
}

// walk: the inclusive (sum, min) scan. A pop that lowers the minimum finds the stack empty: it is deferred, the (-min)-th of them.
// Otherwise the stack's depth is sum - min: a push has the level it reaches, a pop the level it leaves. Deferred pops and the
// keys behind the last event get level 0. 2 n threads.
__global__ __launch_bounds__(T) void lookup_levels(uint32_t n, const uint64_t *ranks, const uint32_t *events, const SumMin *walk, uint64_t *keys,
                                                   uint32_t *deferred, uint32_t *header) {
    const uint32_t k = blockIdx.x * T + threadIdx.x;
    if (k >= 2 * n) return;
    const uint32_t num_events = (uint32_t)ranks[n] + (uint32_t)(ranks[n] >> 32);
    if (k == 0 && num_events == 0) header[H_NUM_DEFERRED] = 0;
    uint32_t level = 0;
    if (k < num_events) {
        const SumMin w = walk[k];
        const int32_t min_before = k ? walk[k - 1].min : 0;
        const uint32_t e = events[k];
        if (k == num_events - 1) header[H_NUM_DEFERRED] = (uint32_t)-w.min;
        if (!(e & POP)) level = (uint32_t)(w.sum - w.min);
        else if (w.min < min_before) deferred[-w.min - 1] = e & ~POP;
        else level = (uint32_t)(w.sum - w.min) + 1;
    }
    keys[k] = (uint64_t)level << 32 | k;
}

// keys: sorted by level, events in order inside a level, where pushes and pops alternate: a pop takes the push before it; a push
// with no pop behind it stays on the stack, at height level - 1. 2 n threads.
__global__ __launch_bounds__(T) void lookup_assign(const uint64_t *t, uint32_t n, const uint64_t *keys, const uint32_t *events,
                                                   uint64_t *permuted_table, uint64_t *stack) {
    const uint32_t q = blockIdx.x * T + threadIdx.x;
    if (q >= 2 * n) return;
    const uint64_t key = keys[q];
    const uint32_t level = (uint32_t)(key >> 32);
    if (level == 0) return;
    const uint32_t e = events[(uint32_t)key];
    if (e & POP) permuted_table[e & ~POP] = t[events[(uint32_t)keys[q - 1]]];
    else if (q + 1 == 2 * n || (uint32_t)(keys[q + 1] >> 32) != level) stack[level - 1] = t[e];
}

// the deferred pops in event order, then the post-loop inputs, take the stack from the bottom
__global__ __launch_bounds__(T) void lookup_fill_deferred(uint32_t n, const uint32_t *deferred, const uint64_t *stack, const uint32_t *header,
                                                          uint64_t *permuted_table) {
    const uint32_t r = blockIdx.x * T + threadIdx.x;
    if (r >= n) return;
    const uint32_t num_deferred = header[H_NUM_DEFERRED], post_start = header[H_POST_START];
    if (r < num_deferred) permuted_table[deferred[r]] = stack[r];
    else if (r - num_deferred < n - post_start) permuted_table[post_start + (r - num_deferred)] = stack[r];
}

uint64_t align_words(uint64_t w) { return (w + 1) & ~1ull; }  // every part starts 16-byte aligned

}  // namespace

LookupScratch lookup_scratch_layout(void *base, uint64_t n) {
    LookupScratch s;
    const uint64_t tiles = (2 * n + LOOKUP_SORT_TILE - 1) / LOOKUP_SORT_TILE;
    const uint64_t longest = 256 * tiles > 2 * n ? 256 * tiles : 2 * n;  // (n + 1 <= 2 n)
    uint64_t words = 0;
    // the part of `size` words that starts where the parts before it end; null without a buffer (the size alone is asked for)
    auto part = [&](uint64_t size) {
        uint64_t *p = base ? static_cast<uint64_t *>(base) + words : nullptr;
        words += size;
        return p;
    };
    s.header = reinterpret_cast<uint32_t *>(part(LOOKUP_HEADER_WORDS));
    s.table = part(align_words(n));
    s.tmp = part(2 * n);
    s.keys = part(2 * n);
    s.ranks = part(align_words(n + 1));
    s.events = reinterpret_cast<uint32_t *>(part(align_words(n)));
    s.stack = part(align_words(n));
    s.deferred = reinterpret_cast<uint32_t *>(part(align_words((n + 1) / 2)));
    s.tile_hist = reinterpret_cast<uint32_t *>(part(128 * tiles));
    s.totals = part(align_words((longest + LOOKUP_SCAN_BLOCK - 1) / LOOKUP_SCAN_BLOCK));
    s.words = words;
    return s;
}

hipError_t lookup_sort_canonical(const uint64_t *in, uint64_t *out, uint64_t n, const LookupScratch &s, hipStream_t stream) {
    return radix_sort(in, out, n, 1, 0, s, stream);
}

hipError_t lookup_sort_by_upper_half(uint64_t *keys, uint64_t n, const LookupScratch &s, hipStream_t stream) {
    return radix_sort(keys, keys, n, 0, 4, s, stream);
}

hipError_t lookup_exclusive_sums(uint64_t *data, uint64_t len, void *totals, hipStream_t stream) {
    return scan_in_place<AddU64, false>(data, len, totals, nullptr, stream);
}

hipError_t lookup_permuted_cols(const uint64_t *inputs, const uint64_t *table, uint64_t n, uint64_t *permuted_inputs, uint64_t *permuted_table,
                                const LookupScratch &s, hipStream_t stream) {
    hipError_t e = radix_sort(inputs, permuted_inputs, n, 1, 0, s, stream);
    if (e != hipSuccess) return e;
    e = radix_sort(table, s.table, n, 1, 0, s, stream);
    if (e != hipSuccess) return e;
    const uint32_t n32 = (uint32_t)n, blocks = (uint32_t)((n + T - 1) / T), blocks2 = (uint32_t)((2 * n + T - 1) / T);
    SumMin *walk = reinterpret_cast<SumMin *>(s.tmp);
    lookup_classify<<<dim3(blocks), dim3(T), 0, stream>>>(permuted_inputs, s.table, n32, permuted_table, s.ranks, s.header);
    e = scan_in_place<AddU64, false>(s.ranks, n + 1, s.totals, nullptr, stream);
    if (e != hipSuccess) return e;
    lookup_events<<<dim3(blocks2), dim3(T), 0, stream>>>(permuted_inputs, s.table, n32, s.ranks, s.events, walk);
    e = scan_in_place<SumMinOp, true>(walk, 2 * n, s.totals, nullptr, stream);
    if (e != hipSuccess) return e;
    lookup_levels<<<dim3(blocks2), dim3(T), 0, stream>>>(n32, s.ranks, s.events, walk, s.keys, s.deferred, s.header);
    e = radix_sort(s.keys, s.keys, 2 * n, 0, 4, s, stream);  // event order is the order of equal levels: only the level's digits
    if (e != hipSuccess) return e;
    lookup_assign<<<dim3(blocks2), dim3(T), 0, stream>>>(s.table, n32, s.keys, s.events, permuted_table, s.stack);
    lookup_fill_deferred<<<dim3(blocks), dim3(T), 0, stream>>>(n32, s.deferred, s.stack, s.header, permuted_table);
    return hipGetLastError();
}

}  // namespace plonky2_hip
