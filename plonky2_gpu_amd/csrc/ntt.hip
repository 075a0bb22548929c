// ntt.hip — batched Goldilocks NTT for gfx950 (MI355X).
//
// What it replaces: fft_dispatch / fft_classic (field/src/fft.rs:37-50, 188-229),
// ifft_with_options (fft.rs:73-103) and, on the reference's GPU side, ifft_kernel / fft_kernel
// (cuda/plonky2_gpu_impl.cuh:214-257), which run one 256-thread block per whole polynomial with
// every radix-2 stage going through global memory.
//
// Design (MI355X-first, not a translation):
//  * A transform of size n = 2^lg is split into at most three "passes" (four-step /
//    Bailey decomposition). One pass = one kernel launch in which every workgroup owns a tile of
//    E = 8192 field elements (64 KiB of the CU's 160 KiB LDS), does an R-point sub-transform on
//    T = E/R interleaved columns entirely in LDS + registers, and touches HBM exactly once for
//    the load and once for the store. HBM traffic per transform is therefore
//    16 B/element/pass (the algorithmic minimum is 16 B/element).
//  * Inside a pass each of the 512 threads (8 wave64) keeps 16 elements in VGPRs and does a
//    radix-16 decimation-in-frequency butterfly. The radix-16 twiddles are powers of
//    w_64 = 2^39 (mod p), so they are shifts (gl::mul_pow2), not multiplies: only the
//    inter-digit twiddles (one per element per digit boundary) cost a 64x64 multiply.
//  * Global accesses are 16 B/lane. "Column" passes read/write T-element (>= 64 B) contiguous
//    segments; "row" passes read whole contiguous rows. LDS uses a +T pad per 16T block so every
//    radix round is bank-conflict free for ds_read_b64 (32 x 8 B slots).
//  * Natural-order output (the fft.rs contract) is produced by the last pass writing the tile
//    transposed (T adjacent outputs per segment); bit-reversed output (what the Merkle leaf order
//    wants, fri/oracle.rs:942-952) falls out of running every pass in place.
//  * The inverse transform is the forward one with the index flip i -> n-i and the n^-1 scale
//    (fft.rs:92-101) folded into the last pass's store addresses.
#include "ntt.h"
#include "knobs.h"

#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "gl_field.h"
#include "ntt_kernels.h"

namespace plonky2_hip {

using namespace nttk;

namespace {

constexpr int NT = 512;            // threads per workgroup (8 wavefronts)
constexpr int LOGE = 13;           // tile = 8192 elements
constexpr int E = 1 << LOGE;
constexpr int LDS_DATA = E + E / 16;  // padded tile

// One radix round over the digit occupying bits [SH, SH+D) of the LDS row index m.
// LOGT = LOGE - LOGR is a compile-time constant, and the padded LDS address of element i of a
// group is (group base) + i * (compile-time stride): bits [SH, SH+D) of m are zero in the base, so
// neither the index nor its pad term (idx >> (4+LOGT)) << LOGT can carry — every ds_read/ds_write
// of the round uses one base VGPR and an immediate offset.
// The tile the round works on has 2^LOGE_ elements and NT_ = 2^LOGE_ / 16 threads: the whole workgroup's tile
// (NT_ = NT = 512) or one wavefront's private tile (NT_ = 64), see ntt_pass_wave_kernel.
template <int LOGE_, int NT_, int LOGR, int D, int SH, bool TWIDDLE>
__device__ __forceinline__ void radix_round(uint64_t *data, const uint64_t *tw, const PassParams &p, uint32_t tid,
                                            uint32_t b, uint32_t z, const uint64_t *chain = nullptr) {
    static_assert((1 << LOGE_) == 16 * NT_, "sixteen elements per thread");
    constexpr int NT = NT_;
    constexpr int RD = 1 << D, G = 16 >> D, LOGT = LOGE_ - LOGR;
    constexpr uint32_t TMASK = (1u << LOGT) - 1;
    static_assert(SH == 0 || SH >= 4, "digits below the top one are radix-16");
    // element stride in the padded image
    constexpr uint32_t STRIDE = (SH >= 4) ? ((1u << (SH + LOGT)) + (1u << (SH - 4 + LOGT))) : (1u << LOGT);
    const bool natural = (SH == 0) && (p.flags & F_NATURAL);
    uint64_t v[16];
    uint32_t base[G];
    static_for<0, G>([&](auto G_) {
        constexpr int g = decltype(G_)::value;
        uint32_t gid = tid + g * NT, l = gid & TMASK, rest = gid >> LOGT;
        uint32_t rest_lo = rest & ((1u << SH) - 1), rest_hi = rest >> SH;
        uint32_t mbase = (rest_hi << (SH + D)) | rest_lo;
        base[g] = phys((mbase << LOGT) + l, LOGT);
        static_for<0, RD>([&](auto I_) {
            constexpr int i = decltype(I_)::value;
            v[g * RD + i] = data[base[g] + i * STRIDE];
        });
    });
    if (natural) tile_sync<NT_>();  // slots are permuted on write-back: everyone must have read
    static_for<0, G>([&](auto G_) { radix_dif<D, decltype(G_)::value * RD>(v); });

    if constexpr (SH > 0) {
        // inter-digit twiddle w_{2^(SH+D)}^(low * k1), k1 = bitrev_D(i), from the LDS table of w_R
        // the G (RD - 1) multiplications as runs of eight with deferred rare paths (ntt_kernels.h mul_run)
        uint32_t rest_lo[G];
        static_for<0, G>([&](auto G_) {
            constexpr int g = decltype(G_)::value;
            rest_lo[g] = ((tid + g * NT) >> LOGT) & ((1u << SH) - 1);
        });
        mul_run<0, G *(RD - 1)>(
            v, [](auto K_) { return (decltype(K_)::value / (RD - 1)) * RD + 1 + decltype(K_)::value % (RD - 1); },
            [&](auto K_) {
                constexpr int g = decltype(K_)::value / (RD - 1), i = 1 + decltype(K_)::value % (RD - 1);
                constexpr int k1 = brev_c(i, D);
                return tw[(rest_lo[g] * k1) << (LOGR - SH - D)];
            },
            [](auto) {});
    } else if constexpr (TWIDDLE) {
        // inter-pass twiddle w_{2^tw_hi}^(L * k1), k1 = bitrev4(i)*(R/16) + kr  (G == 1, D == 4)
        static_assert(D == 4 || !TWIDDLE, "twiddled passes end with a radix-16 round");
        uint64_t c, step;
        if (chain) {
            c = chain[0], step = chain[1];
        } else {
            twiddle_chain<LOGT, LOGR>(p, tid, b, z, c, step);
        }
        static_for<0, 16>([&](auto J_) {
            constexpr int j = decltype(J_)::value;
            constexpr int i = brev_c(j, 4);
            v[i] = gl::mul(v[i], c);
            if constexpr (j < 15) c = gl::mul(c, step);
        });
    }

    if (!natural) {
        static_for<0, G>([&](auto G_) {
            constexpr int g = decltype(G_)::value;
            static_for<0, RD>([&](auto I_) {
                constexpr int i = decltype(I_)::value;
                data[base[g] + i * STRIDE] = v[g * RD + i];
            });
        });
    } else {
        // natural order: slot of frequency k = (bitrev_D(i) << (LOGR-D)) | bitrev(rest). The pad term
        // of the slot index is again separable into a per-thread base and a per-i constant.
        if constexpr (SH == 0) {
            static_for<0, G>([&](auto G_) {
                constexpr int g = decltype(G_)::value;
                uint32_t gid = tid + g * NT, l = gid & TMASK, rest = gid >> LOGT;
                uint32_t kr = brev_rt(rest, LOGR - D);
                uint32_t nb = (kr << LOGT) + l + (((LOGR - D >= 4) ? (kr >> 4) : 0u) << LOGT);
                static_for<0, RD>([&](auto I_) {
                    constexpr int i = decltype(I_)::value;
                    constexpr uint32_t mi = (uint32_t)brev_c(i, D) << (LOGR - D);
                    constexpr uint32_t off = (mi << LOGT) + ((mi >> 4) << LOGT);
                    data[nb + off] = v[g * RD + i];
                });
            });
        }
    }
}

template <int LOGE_, int NT_, int LOGR, int SH, bool TWIDDLE>
__device__ __forceinline__ void radix16_rounds(uint64_t *data, const uint64_t *tw, const PassParams &p, uint32_t tid,
                                               uint32_t b, uint32_t z, const uint64_t *chain) {
    if constexpr (SH >= 0) {
        radix_round<LOGE_, NT_, LOGR, 4, SH, TWIDDLE>(data, tw, p, tid, b, z, chain);
        if constexpr (SH > 0) {
            tile_sync<NT_>();
            radix16_rounds<LOGE_, NT_, LOGR, SH - 4, TWIDDLE>(data, tw, p, tid, b, z, chain);
        }
    }
}

// The R-point DIF of a tile: a short first digit (radix 2/4/8) absorbs LOGR mod 4, radix-16 digits follow.
template <int LOGE_, int NT_, int LOGR, bool TWIDDLE>
__device__ __forceinline__ void tile_transform(uint64_t *data, const uint64_t *tw, const PassParams &p, uint32_t tid, uint32_t b,
                                               uint32_t z, const uint64_t *chain = nullptr) {
    constexpr int D0 = LOGR % 4;
    if constexpr (D0 != 0) {
        radix_round<LOGE_, NT_, LOGR, D0, LOGR - D0, TWIDDLE>(data, tw, p, tid, b, z, chain);
        if constexpr (LOGR - D0 > 0) tile_sync<NT_>();
    }
    radix16_rounds<LOGE_, NT_, LOGR, LOGR - D0 - 4, TWIDDLE>(data, tw, p, tid, b, z, chain);
}

struct alignas(16) u64x2 {
    uint64_t x, y;
};

__device__ __forceinline__ uint64_t flip_index(uint64_t o, uint32_t log_n) {
    uint64_t mask = (1ull << log_n) - 1;
    return (o & ~mask) | (((1ull << log_n) - (o & mask)) & mask);
}

template <int LOGR, bool TWIDDLE>
__global__ __launch_bounds__(NT) void ntt_pass_kernel(const PassParams p) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    uint64_t *data = lds;
    uint64_t *tw = lds + LDS_DATA;
    constexpr int R = 1 << LOGR;
    constexpr uint32_t logt = LOGE - LOGR, T = 1u << logt;
    const uint32_t tid = threadIdx.x;
    const uint32_t a = blockIdx.y, b = blockIdx.x, z = blockIdx.z;

    // local twiddles w_R^e = w_4096^(e * 4096/R)
    if constexpr (LOGR >= 5)
        for (uint32_t e = tid; e < (uint32_t)R; e += NT) tw[e] = p.twh[e << (12 - LOGR)];

    // ---- load tile -------------------------------------------------------------------------
    const uint64_t in_base = a * p.in_sa + b * p.in_sb + z * p.in_sz;
    const bool coset = p.flags & F_COSET;
    if (!(p.flags & F_LOAD_ROWS)) {
        // t contiguous: T/2 lanes x 16 B per row segment
#pragma unroll
        for (int it = 0; it < 8; it++) {
            uint32_t c = tid + it * NT;
            uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
            u64x2 val = {0, 0};
            if (b * T + t < p.t_limit) val = *reinterpret_cast<const u64x2 *>(p.src + in_base + t + (uint64_t)m * p.in_m);
            if (coset) {
                // input scale (s_r^N2)^m = s_r^(m * in_m): in_m is a multiple of 1024 or the
                // two-level split below is still exact because exponents add.
                uint64_t ex = (uint64_t)m * p.in_m;
                uint64_t sc = gl::mul(p.cs_hi[z * p.cs_hi_len + (uint32_t)(ex >> 10)], p.cs_lo[z * 1024 + (uint32_t)(ex & 1023)]);
                val.x = gl::mul(val.x, sc);
                val.y = gl::mul(val.y, sc);
            }
            *reinterpret_cast<u64x2 *>(&data[phys((m << logt) + t, logt)]) = val;
        }
    } else {
        // m contiguous (whole rows): lane = (t, m pair)
#pragma unroll
        for (int it = 0; it < 8; it++) {
            uint32_t c = tid + it * NT;
            uint32_t t = c & (T - 1), m = (c >> logt) * 2;
            u64x2 val = {0, 0};
            if (p.row_shift) {
                uint32_t row = (b * T + t + p.row_shift) & (p.t_limit - 1);
                val = *reinterpret_cast<const u64x2 *>(p.src + a * p.in_sa + z * p.in_sz + (uint64_t)row * p.in_t + m);
            } else if (b * T + t < p.t_limit) {
                val = *reinterpret_cast<const u64x2 *>(p.src + in_base + (uint64_t)t * p.in_t + m);
            }
            data[phys((m << logt) + t, logt)] = val.x;
            data[phys(((m + 1) << logt) + t, logt)] = val.y;
        }
    }
    __syncthreads();

    // ---- R-point DIF in LDS/registers ------------------------------------------------------
    tile_transform<LOGE, NT, LOGR, TWIDDLE>(data, tw, p, tid, b, z);
    __syncthreads();

    // ---- store tile ------------------------------------------------------------------------
    const uint32_t zo = coset ? brev_rt(z, p.rate_bits) : z;
    const uint64_t out_base = a * p.out_sa + b * p.out_sb + zo * p.out_sz;
    const bool inverse = p.flags & F_INVERSE, do_scale = p.scale != 1;
    if (!(p.flags & F_STORE_ROWS)) {
#pragma unroll
        for (int it = 0; it < 8; it++) {
            uint32_t c = tid + it * NT;
            uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
            if (b * T + t >= p.t_limit) continue;
            u64x2 val = *reinterpret_cast<const u64x2 *>(&data[phys((m << logt) + t, logt)]);
            if (do_scale) {
                val.x = gl::mul(val.x, p.scale);
                val.y = gl::mul(val.y, p.scale);
            }
            val.x = gl::canon(val.x);
            val.y = gl::canon(val.y);
            uint64_t o = out_base + t + (uint64_t)m * p.out_m;
            if (!inverse) {
                *reinterpret_cast<u64x2 *>(p.dst + o) = val;
            } else if (p.row_shift) {
                uint64_t ob = a * p.out_sa + zo * p.out_sz + (uint64_t)m * p.out_m;
                uint32_t r0 = (b * T + t + p.row_shift) & (p.t_limit - 1), r1 = (b * T + t + 1 + p.row_shift) & (p.t_limit - 1);
                p.dst[flip_index(ob + r0, p.log_n)] = val.x;
                p.dst[flip_index(ob + r1, p.log_n)] = val.y;
            } else {
                p.dst[flip_index(o, p.log_n)] = val.x;
                p.dst[flip_index(o + 1, p.log_n)] = val.y;
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < 8; it++) {
            uint32_t c = tid + it * NT;
            uint32_t t = c & (T - 1), m = (c >> logt) * 2;
            if (b * T + t >= p.t_limit) continue;
            u64x2 val;
            val.x = data[phys((m << logt) + t, logt)];
            val.y = data[phys(((m + 1) << logt) + t, logt)];
            if (do_scale) {
                val.x = gl::mul(val.x, p.scale);
                val.y = gl::mul(val.y, p.scale);
            }
            val.x = gl::canon(val.x);
            val.y = gl::canon(val.y);
            uint64_t o = out_base + (uint64_t)t * p.out_t + m;
            if (!inverse) {
                *reinterpret_cast<u64x2 *>(p.dst + o) = val;
            } else {
                p.dst[flip_index(o, p.log_n)] = val.x;
                p.dst[flip_index(o + 1, p.log_n)] = val.y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same pass with the tile split into eight wavefront-private sub-tiles (R <= 1024).
//
// ntt_pass_kernel above synchronises its eight wavefronts four or five times per tile, and a CU holds two
// such workgroups: the waves of a workgroup run their load, their rounds and their store in lockstep, and the
// counters show it (rocprofv3, 2^20: vector ALU ~70 % busy, memory ~65 % busy, waves parked 65 % of their
// lifetime — profiles/r02_*). Here a wavefront owns 1024 elements of the tile — TW = 1024/R whole columns
// (rows in a row pass) — in its own padded LDS buffer and runs all radix rounds of its R-point transforms by
// itself: between rounds it needs no barrier at all, because the LDS executes one wavefront's reads and writes in
// program order (tile_sync<64>). Workgroup barriers remain only where the eight waves exchange data through LDS
// to make global accesses wide: a column-pass load (T adjacent columns per row = one T*8-byte segment; the
// segment is spread over the wave buffers on arrival), a column-pass store and the transposed natural-order
// store of a row pass. A row pass that reads and writes whole rows (every pass of the bit-reversed transforms of
// the LDE / commit path) has no barrier after the twiddle table is in place, and its waves drift apart: while
// one waits for its row, the other three of its SIMD compute.
//
// LDS: 8 buffers of 1024 + 64 pad + 2 skew words, + the twiddle table of w_R = 77,952 bytes: two workgroups per CU,
// four waves per SIMD, as before. Grid, tile geometry and PassParams are those of ntt_pass_kernel.
// ---------------------------------------------------------------------------------------------
constexpr int WT = 64;                    // threads of a wave tile
constexpr int LOGEW = 10;                 // wave tile = 1024 elements
constexpr int EW = 1 << LOGEW;
constexpr int WIDE_MIN_LOGR = 7;           // wide (16-wave) tiles are instantiated for R >= 128
constexpr int WBUF = EW + EW / 16 + 2;    // padded wave buffer; the skew of 2 words spreads the eight buffers over
                                          // the banks for the cooperative (cross-buffer) accesses



// LOGW = log2 of the wavefronts per workgroup: 3 (tile of 8192 elements, two workgroups per CU) or 4 (16384 elements, one
// workgroup per CU): the wide tile doubles the segments of the cooperative accesses to 128 bytes — whole cache lines —
// which the memory system moves ~25 % faster than 64-byte halves (tools/ubench_mem.hip, profiles/r02_ubench_mem.txt).
//
// SPLIT (column passes of 2R = 2048 points, LOGR = 10, sixteen waves): a column is twice a wave tile. The first DIF stage —
// a[j] = x[j] + x[j+R], b[j] = (x[j] - x[j+R]) * w_2R^j — is taken while the segments are spread over the wave buffers (the
// thread that loaded row j also loaded row j+R), and the two R-point transforms that remain, of a (even frequencies) and b (odd
// frequencies), are wave tiles like any other: wave 2t holds a of column t, wave 2t+1 holds b. Two passes instead of three
// for 2^21 and 2^22 points.
template <int LOGR, bool TWIDDLE, bool ROWS_IN, bool ROWS_OUT, int LOGW, bool SPLIT = false>
__global__ __launch_bounds__(64 << LOGW) __attribute__((amdgpu_waves_per_eu(4, 4))) void ntt_pass_wave_kernel(const PassParams p, const uint32_t gx, const uint32_t gy, const uint32_t total, const uint32_t xcd_map) {
    static_assert(LOGR <= LOGEW, "a wave tile holds whole R-point columns");
    static_assert(!SPLIT || (LOGR == LOGEW && !ROWS_IN && !ROWS_OUT), "split columns: column passes of 2 * 1024 points");
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    constexpr int R = 1 << LOGR;
    constexpr int NT = 64 << LOGW, WAVES = 1 << LOGW, LOGE = LOGEW + LOGW;  // this kernel's workgroup geometry
    constexpr uint32_t logt = LOGE - LOGR - (SPLIT ? 1 : 0), T = 1u << logt;        // columns of the workgroup tile
    constexpr uint32_t logtw = LOGEW - LOGR, TW = 1u << logtw;    // columns of a wave tile
    static_assert(T >= 2, "16-byte accesses");
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint64_t *data = lds + wave * WBUF;   // this wave's tile
    uint64_t *tw = lds + WAVES * WBUF;
    // slot of element (row m, column t) of the workgroup tile
    auto slot = [&](uint32_t m, uint32_t t) -> uint32_t {
        if constexpr (SPLIT) return ((t << 1) + (m >> LOGR)) * WBUF + phys(m & (R - 1), 0);
        return (t >> logtw) * WBUF + phys((m << logtw) + (t & (TW - 1)), logtw);
    };
    // slot of OUTPUT row m: frequency m of a split column is element m >> 1 of the half m & 1 when the tile is in natural order
    auto slot_out = [&](uint32_t m, uint32_t t) -> uint32_t {
        if constexpr (SPLIT)
            if (p.flags & F_NATURAL) return ((t << 1) + (m & 1)) * WBUF + phys(m >> 1, 0);
        return slot(m, t);
    };
    constexpr bool rows_in = ROWS_IN, rows_out = ROWS_OUT;  // F_LOAD_ROWS / F_STORE_ROWS, fixed at compile time
    const bool coset = p.flags & F_COSET, inverse = p.flags & F_INVERSE, do_scale = p.scale != 1;

    // tile id -> (b, a, z) of the grid the planner describes (b fastest)
    auto decode = [&](uint32_t id, uint32_t &b, uint32_t &a, uint32_t &z) {
        b = id % gx;
        const uint32_t q = id / gx;
        a = q % gy;
        z = q / gy;
    };
    // the tile's global loads, 8 x 16 B per thread, left in flight
    auto issue_loads = [&](uint32_t id, u64x2 (&pre)[8]) {
        uint32_t b, a, z;
        decode(id, b, a, z);
        const uint64_t in_base = a * p.in_sa + b * p.in_sb + z * p.in_sz;
        // Every tile is full (the planner sends ragged ones to ntt_pass_kernel): no bounds checks, straight-line code,
        // all eight loads in flight at once.
        if constexpr (!rows_in) {
            // column pass: T adjacent columns of a row are one segment; 16 B per lane = two columns
#pragma unroll
            for (int it = 0; it < 8; it++) {
                uint32_t c = tid + it * NT;
                uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
                pre[it] = *reinterpret_cast<const u64x2 *>(p.src + in_base + t + (uint64_t)m * p.in_m);
            }
        } else {
            // row pass: a wave reads its own TW rows, 16 B per lane along the row
            const uint64_t az_base = a * p.in_sa + z * p.in_sz;
#pragma unroll
            for (int it = 0; it < 8; it++) {
                uint32_t c = lane + it * WT;
                uint32_t tl = c & (TW - 1), t = wave * TW + tl, m = (c >> logtw) * 2;
                // inverse natural-order row pass: the row tile is rotated by one (t_limit is a power of two there)
                const uint32_t shifted = (b * T + t + p.row_shift) & (p.t_limit - 1);
                const uint64_t off = p.row_shift ? az_base + (uint64_t)shifted * p.in_t : in_base + (uint64_t)t * p.in_t;
                pre[it] = *reinterpret_cast<const u64x2 *>(p.src + off + m);
            }
        }
    };

    if constexpr (LOGR >= 5)
        for (uint32_t e = tid; e < (uint32_t)R; e += NT) tw[e] = p.twh[e << (12 - LOGR)];

    // A workgroup walks the tiles id = blockIdx.x, + gridDim.x, ...; the loads of tile k+1 are issued as soon as
    // tile k sits in LDS and land while its radix rounds run: without this every CU of the chip loads, then
    // computes, then stores in step with all the others, and neither the memory system nor the vector ALU is busy
    // for more than two thirds of the time.
    // registers -> LDS for tile `id` whose loads are in flight in `pre`
    auto land = [&](uint32_t id, u64x2 (&pre)[8]) {
        uint32_t z = id / (gx * gy);
        uint32_t tid_i = tid, lane_i = lane;
        asm volatile("" : "+v"(tid_i), "+v"(lane_i));
        if constexpr (SPLIT) {
#pragma unroll
            for (int it = 0; it < 4; it++) {
                uint32_t c = tid_i + it * NT;
                uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);  // m < R; pre[it + 4] is row m + R of the same columns
                u64x2 x = pre[it], y = pre[it + 4];
                if (coset) {
                    uint64_t ex = (uint64_t)m * p.in_m, ey = (uint64_t)(m + R) * p.in_m;
                    uint64_t sx = gl::mul(p.cs_hi[z * p.cs_hi_len + (uint32_t)(ex >> 10)], p.cs_lo[z * 1024 + (uint32_t)(ex & 1023)]);
                    uint64_t sy = gl::mul(p.cs_hi[z * p.cs_hi_len + (uint32_t)(ey >> 10)], p.cs_lo[z * 1024 + (uint32_t)(ey & 1023)]);
                    x.x = gl::mul(x.x, sx);
                    x.y = gl::mul(x.y, sx);
                    y.x = gl::mul(y.x, sy);
                    y.y = gl::mul(y.y, sy);
                }
                const uint64_t wv = p.twh[m << (12 - (LOGR + 1))];  // w_2R^m
                lds[slot(m, t)] = gl::add(x.x, y.x);
                lds[slot(m, t + 1)] = gl::add(x.y, y.y);
                lds[slot(m + R, t)] = gl::mul(gl::sub(x.x, y.x), wv);
                lds[slot(m + R, t + 1)] = gl::mul(gl::sub(x.y, y.y), wv);
            }
            lds_barrier();
        } else if constexpr (!rows_in) {
#pragma unroll
            for (int it = 0; it < 8; it++) {
                uint32_t c = tid_i + it * NT;
                uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
                u64x2 val = pre[it];
                if (coset) {
                    // input scale (s_r^N2)^m = s_r^(m * in_m), through the two-level table (exponents add)
                    uint64_t ex = (uint64_t)m * p.in_m;
                    uint64_t sc = gl::mul(p.cs_hi[z * p.cs_hi_len + (uint32_t)(ex >> 10)], p.cs_lo[z * 1024 + (uint32_t)(ex & 1023)]);
                    val.x = gl::mul(val.x, sc);
                    val.y = gl::mul(val.y, sc);
                }
                if constexpr (TW >= 2) {
                    *reinterpret_cast<u64x2 *>(&lds[slot(m, t)]) = val;
                } else {
                    lds[slot(m, t)] = val.x;
                    lds[slot(m, t + 1)] = val.y;
                }
            }
            lds_barrier();  // the segments are spread over the wave buffers
        } else {
#pragma unroll
            for (int it = 0; it < 8; it++) {
                uint32_t c = lane_i + it * WT;
                uint32_t tl = c & (TW - 1), m = (c >> logtw) * 2;
                data[phys((m << logtw) + tl, logtw)] = pre[it].x;
                data[phys(((m + 1) << logtw) + tl, logtw)] = pre[it].y;
            }
            tile_sync<WT>();
        }
    };

    // One iteration works on tile k, whose elements sit in LDS, while the loads of tile k+1 (issued at the end of the
    // previous iteration) and the stores of tile k-1 are in flight:
    //     radix rounds of k -> results of k from LDS into registers -> tile k+1: wait for its loads, registers -> LDS,
    //     twiddle-chain look-ups of k+1 -> stores of k -> loads of k+2 issued.
    // Order matters for the waits: vmcnt counts loads and stores together in issue order, and the compiler's counted
    // waits for the prefetched registers do not discount younger stores — so the stores of k are issued only AFTER
    // tile k+1 has landed (its loads are then the youngest operations and the wait is exact), and they have all of the
    // next tile's radix rounds to drain.
    u64x2 pre[8];
    uint64_t chain[2] = {1, 1};
    // Which tiles a workgroup walks. Workgroups are dealt to the eight XCDs round-robin (workgroup w runs on XCD w mod 8) and
    // every XCD has its own L2, so with xcd_map the workgroups of ONE XCD take CONSECUTIVE tiles at every step: the k-th
    // tile of workgroup w is ((k*8 + w%8) * (G/8)) + w/8. Consecutive tiles of a column are the adjacent 64/128-byte
    // pieces of the same rows, so an XCD's L2 and the DRAM pages behind it see whole runs of a row at about the same time
    // instead of one piece in eight. Without it: w, w+G, w+2G, ...
    const uint32_t G = gridDim.x;
    const uint32_t per_xcd = G >> 3;
    auto tile_at = [&](uint32_t k) -> uint32_t {
        const uint64_t t = xcd_map ? ((uint64_t)k * 8 + (blockIdx.x & 7)) * per_xcd + (blockIdx.x >> 3) : (uint64_t)k * G + blockIdx.x;
        return t < total ? (uint32_t)t : 0xFFFFFFFFu;
    };
    uint32_t step = 0;
    uint32_t id = tile_at(0);
    auto chain_of = [&](uint32_t tile) {
        if constexpr (TWIDDLE) {
            uint32_t b, a, z;
            decode(tile, b, a, z);
            uint32_t lane_i = lane;
            asm volatile("" : "+v"(lane_i));
            if constexpr (SPLIT) {
                // output frequency of column L: k1 = 2 * k_inner + h = bitrev4(i) * (2R/16) + (2 * kr + h)
                const uint64_t L = (uint64_t)b * T + (wave >> 1);
                const uint32_t kr = 2 * brev_rt(lane_i, LOGR - 4) + (wave & 1);
                uint64_t c = wpow(p, L * kr);
                if (p.flags & F_COSET)
                    c = gl::mul(c, gl::mul(p.cs_hi[z * p.cs_hi_len + (uint32_t)(L >> 10)], p.cs_lo[z * 1024 + (uint32_t)(L & 1023)]));
                if (p.chain_scale != 1) c = gl::mul(c, p.chain_scale);
                chain[0] = c;
                chain[1] = wpow(p, L << (LOGR - 3));
            } else {
                twiddle_chain<logtw, LOGR>(p, lane_i, b * WAVES + wave, z, chain[0], chain[1]);
            }
        }
    };
    if (id < total) issue_loads(id, pre);
    lds_barrier();  // the twiddle table
    if (id < total) {
        land(id, pre);
        chain_of(id);
        if (tile_at(1) < total) issue_loads(tile_at(1), pre);
    }

    for (; id < total; id = tile_at(++step)) {
        const uint32_t nid = tile_at(step + 1);
        uint32_t b, a, z;
        decode(id, b, a, z);
        // Per-thread slot and address arithmetic is the same for every tile; left to itself the compiler hoists all of it
        // out of this loop and keeps it in registers next to the prefetched tile (128 VGPRs, then scratch). Recomputing
        // it per tile costs a few dozen integer instructions.
        uint32_t tid_i = tid, lane_i = lane;
        asm volatile("" : "+v"(tid_i), "+v"(lane_i));

        // ---- R-point DIFs of this wave's TW columns, no workgroup barrier ------------------------
        tile_transform<LOGEW, WT, LOGR, TWIDDLE>(data, tw, p, lane_i, b * WAVES + wave, z, TWIDDLE ? chain : nullptr);

        // ---- results: LDS -> registers ----------------------------------------------------------------
        u64x2 res[8];
        if constexpr (!rows_out) {
            lds_barrier();  // segments are gathered across the wave buffers
#pragma unroll
            for (int it = 0; it < 8; it++) {
                uint32_t c = tid_i + it * NT;
                uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
                if constexpr (TW >= 2) {
                    res[it] = *reinterpret_cast<const u64x2 *>(&lds[slot(m, t)]);
                } else {
                    res[it].x = lds[slot_out(m, t)];
                    res[it].y = lds[slot_out(m, t + 1)];
                }
            }
        } else {
            tile_sync<WT>();
#pragma unroll
            for (int it = 0; it < 8; it++) {
                uint32_t c = lane_i + it * WT;
                uint32_t tl = c & (TW - 1), m = (c >> logtw) * 2;
                res[it].x = data[phys((m << logtw) + tl, logtw)];
                res[it].y = data[phys(((m + 1) << logtw) + tl, logtw)];
            }
        }
        // the next tile's arrival overwrites buffers that a cooperative load / store lets other waves touch
        if constexpr (!(rows_in && rows_out))
            lds_barrier();
        else
            tile_sync<WT>();

        // ---- tile k+1 lands ---------------------------------------------------------------------------
        if (nid < total) {
            land(nid, pre);
            chain_of(nid);
        }

        // ---- stores of tile k -------------------------------------------------------------------------
        const uint32_t zo = coset ? brev_rt(z, p.rate_bits) : z;
        const uint64_t out_base = a * p.out_sa + b * p.out_sb + zo * p.out_sz;
        auto finish = [&](u64x2 val) {
            if (do_scale) {
                val.x = gl::mul(val.x, p.scale);
                val.y = gl::mul(val.y, p.scale);
            }
            if (!(p.flags & F_RAW_OUT)) {
                val.x = gl::canon(val.x);
                val.y = gl::canon(val.y);
            }
            return val;
        };
        if constexpr (!rows_out) {
            if (!inverse) {
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    uint32_t c = tid_i + it * NT;
                    uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
                    *reinterpret_cast<u64x2 *>(p.dst + out_base + t + (uint64_t)m * p.out_m) = finish(res[it]);
                }
            } else if (p.row_shift) {
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    uint32_t c = tid_i + it * NT;
                    uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
                    u64x2 val = finish(res[it]);
                    uint64_t ob = a * p.out_sa + zo * p.out_sz + (uint64_t)m * p.out_m;
                    uint32_t r0 = (b * T + t + p.row_shift) & (p.t_limit - 1), r1 = (b * T + t + 1 + p.row_shift) & (p.t_limit - 1);
                    p.dst[flip_index(ob + r0, p.log_n)] = val.x;
                    p.dst[flip_index(ob + r1, p.log_n)] = val.y;
                }
            } else {
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    uint32_t c = tid_i + it * NT;
                    uint32_t t = (c & (T / 2 - 1)) * 2, m = c >> (logt - 1);
                    u64x2 val = finish(res[it]);
                    uint64_t o = out_base + t + (uint64_t)m * p.out_m;
                    p.dst[flip_index(o, p.log_n)] = val.x;
                    p.dst[flip_index(o + 1, p.log_n)] = val.y;
                }
            }
        } else {
            if (!inverse) {
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    uint32_t c = lane_i + it * WT;
                    uint32_t tl = c & (TW - 1), t = wave * TW + tl, m = (c >> logtw) * 2;
                    {
                        // whole rows written once and not read again by this kernel: nontemporal stores (bit-reversed
                        // 2^20 transform 0.70 ms against 0.73 with plain stores, profiles/r02_ntt_nontemporal_experiment.jsonl;
                        // nontemporal LOADS of the rows cost 2-3 %)
                        typedef uint64_t v2u64 __attribute__((ext_vector_type(2)));
                        const u64x2 fv = finish(res[it]);
                        v2u64 t2;
                        t2.x = fv.x;
                        t2.y = fv.y;
                        __builtin_nontemporal_store(t2, reinterpret_cast<v2u64 *>(p.dst + out_base + (uint64_t)t * p.out_t + m));
                    }
                }
            } else {
#pragma unroll
                for (int it = 0; it < 8; it++) {
                    uint32_t c = lane_i + it * WT;
                    uint32_t tl = c & (TW - 1), t = wave * TW + tl, m = (c >> logtw) * 2;
                    u64x2 val = finish(res[it]);
                    uint64_t o = out_base + (uint64_t)t * p.out_t + m;
                    p.dst[flip_index(o, p.log_n)] = val.x;
                    p.dst[flip_index(o + 1, p.log_n)] = val.y;
                }
            }
        }
        // ---- loads of tile k+2 ------------------------------------------------------------------------
        if (tile_at(step + 2) < total) issue_loads(tile_at(step + 2), pre);
    }
}

// PLONKY2_NTT_KERNEL=tile selects the workgroup-tile kernel for every size (A/B measurements, tests of both)
static bool use_wave_kernel() {
    static const bool v = [] {
        const char *e = PLONKY2_KNOB("PLONKY2_NTT_KERNEL");
        return !(e && e[0] == 't');
    }();
    return v;
}


// PLONKY2_NTT_DIRECT=0: the wave-tile kernels also where a direct pass exists (A/B measurements)
static bool direct_mode() {
    static const bool v = [] {
        const char *e = PLONKY2_KNOB("PLONKY2_NTT_DIRECT");
        return !(e && e[0] == '0');
    }();
    return v;
}

// PLONKY2_NTT_XCD=0: workgroups walk tiles w, w+G, ... instead of the XCD-aware order (A/B measurements)
static bool xcd_map_enabled() {
    static const bool v = [] {
        const char *e = PLONKY2_KNOB("PLONKY2_NTT_XCD");
        return !(e && e[0] == '0');
    }();
    return v;
}

// Two workgroups per CU (the LDS holds no more), each walking its share of the tiles
static uint32_t persistent_workgroups() {
    static const uint32_t v = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        if (const char *e = PLONKY2_KNOB("PLONKY2_NTT_WG_PER_CU")) {
            int k = atoi(e);
            if (k >= 1 && k <= 8) return (uint32_t)(cus * k);
        }
        return (uint32_t)(2 * cus);
    }();
    return v;
}

template <int LOGR, bool TWIDDLE, bool ROWS_IN, bool ROWS_OUT, int LOGW = 3, bool SPLIT = false>
hipError_t launch_pass_wave_mode(const PassParams &p_in, dim3 grid, hipStream_t stream) {
    size_t lds_bytes = (size_t)((WBUF << LOGW) + (LOGR >= 5 ? (1 << LOGR) : 0)) * sizeof(uint64_t);
    static DynamicLds attr;
    if (hipError_t e = allow_dynamic_lds(attr, reinterpret_cast<const void *>(&ntt_pass_wave_kernel<LOGR, TWIDDLE, ROWS_IN, ROWS_OUT, LOGW, SPLIT>), (uint32_t)lds_bytes);
        e != hipSuccess)
        return e;
    const uint64_t total = (uint64_t)grid.x * grid.y * grid.z;
    if (total > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t resident = persistent_workgroups() >> (LOGW - 3);  // the LDS holds two 8-wave or one 16-wave workgroup per CU
    const uint32_t wgs = (uint32_t)(total < resident ? total : resident);
    const PassParams &p = p_in;
    hipLaunchKernelGGL((ntt_pass_wave_kernel<LOGR, TWIDDLE, ROWS_IN, ROWS_OUT, LOGW, SPLIT>), dim3(wgs), dim3(64 << LOGW), lds_bytes, stream, p,
                       (uint32_t)grid.x, (uint32_t)grid.y, (uint32_t)total, (uint32_t)(xcd_map_enabled() && wgs % 8 == 0 ? 1 : 0));
    return hipGetLastError();
}

// The planner's passes come in three shapes: column pass (segments in, segments out), row pass with transposed
// natural-order output (rows in, segments out), row pass in place (rows in, rows out).
template <int LOGR, bool TWIDDLE>
hipError_t launch_pass_wave(const PassParams &p, dim3 grid, hipStream_t stream) {
    const bool ri = p.flags & F_LOAD_ROWS, ro = p.flags & F_STORE_ROWS;
    if constexpr (LOGR >= WIDE_MIN_LOGR) {
        if (p.flags & F_WIDE) {
            if constexpr (TWIDDLE && LOGR >= 8 && LOGR <= 10)
                if (!ri && !ro && direct_mode() && (p.flags & F_RAW_OUT) && p.scale == 1 && p.in_t == 1 && p.out_t == 1 &&
                    (!(p.flags & F_COSET) || (!(p.flags & F_NATURAL) && p.in_sz == 0 && p.chain_scale == 1 && nttk::col_direct_coset_ok(LOGR - 8, grid))))
                    return nttk::launch_col_direct(LOGR - 8, p, grid, stream);
            if (!ri && !ro) return launch_pass_wave_mode<LOGR, TWIDDLE, false, false, 4>(p, grid, stream);
            if constexpr (!TWIDDLE && LOGR == 10)
                if (ri && !ro && direct_mode() && (p.flags & F_NATURAL) && !(p.flags & F_COSET) && p.scale == 1 && p.in_m == 1 && p.out_t == 1)
                    return nttk::launch_row_natural_direct(p, grid, stream);
            if constexpr (!TWIDDLE)
                if (ri && !ro) return launch_pass_wave_mode<LOGR, false, true, false, 4>(p, grid, stream);
            return hipErrorInvalidValue;
        }
    }
    if (p.flags & F_WIDE) return hipErrorInvalidValue;
    if (!ri && !ro) return launch_pass_wave_mode<LOGR, TWIDDLE, false, false>(p, grid, stream);
    if constexpr (!TWIDDLE) {  // row passes carry no inter-pass twiddle
        if (ri && !ro) return launch_pass_wave_mode<LOGR, false, true, false>(p, grid, stream);
        if constexpr (LOGR == 10)
            if (ri && ro && direct_mode() && !(p.flags & (F_NATURAL | F_INVERSE | F_COSET | F_RAW_OUT)) && p.scale == 1 && p.in_m == 1 && p.out_m == 1 &&
                p.row_shift == 0)
                return nttk::launch_row_inplace_direct(p, grid, stream);
        if (ri && ro) return launch_pass_wave_mode<LOGR, false, true, true>(p, grid, stream);
    }
    return hipErrorInvalidValue;
}

// column pass of 2048 points (ntt_pass_wave_kernel, SPLIT): the planner asks for it with logr = 11 and F_WIDE
template <bool TWIDDLE>
hipError_t launch_pass_wave_split(const PassParams &p, dim3 grid, hipStream_t stream) {
    if (!(p.flags & F_WIDE) || (p.flags & (F_LOAD_ROWS | F_STORE_ROWS))) return hipErrorInvalidValue;
    if constexpr (TWIDDLE)
        if (direct_mode() && (p.flags & F_RAW_OUT) && !(p.flags & F_COSET) && p.scale == 1 && p.in_t == 1 && p.out_t == 1)
            return nttk::launch_col_direct(3, p, grid, stream);   // the direct column pass with eight lane groups (tiles of 2048 rows x 8 columns)
    return launch_pass_wave_mode<LOGEW, TWIDDLE, false, false, 4, true>(p, grid, stream);
}

template <int LOGR, bool TWIDDLE>
hipError_t launch_pass(const PassParams &p, dim3 grid, hipStream_t stream) {
    size_t lds_bytes = (size_t)(LDS_DATA + (LOGR >= 5 ? (1 << LOGR) : 0)) * sizeof(uint64_t);
    static DynamicLds attr;
    if (hipError_t e = allow_dynamic_lds(attr, reinterpret_cast<const void *>(&ntt_pass_kernel<LOGR, TWIDDLE>), (uint32_t)lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL((ntt_pass_kernel<LOGR, TWIDDLE>), grid, dim3(NT), lds_bytes, stream, p);
    return hipGetLastError();
}

template <bool TWIDDLE>
hipError_t dispatch_pass(int logr, const PassParams &p, dim3 grid, hipStream_t stream) {
    const int loge = LOGE + ((p.flags & F_WIDE) ? 1 : 0);
    const bool full_tiles = logr <= loge && (p.t_limit & ((1u << (loge - logr)) - 1)) == 0;  // ragged tiles keep the bounds-checked kernel
    if (!full_tiles && (p.flags & F_WIDE)) return hipErrorInvalidValue;  // the planner checks before it asks for wide tiles
    if (use_wave_kernel() && full_tiles) {
        // a column pass / transposed store of a wave kernel needs >= 2 columns per tile (16-byte accesses): R <= 4096
        // holds for every planned pass; wave tiles exist for R <= 1024
        switch (logr) {
#define CASE(L) \
    case L:     \
        return launch_pass_wave<L, TWIDDLE>(p, grid, stream);
            CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
#undef CASE
            default:
                break;
        }
        if constexpr (TWIDDLE)
            if (logr == LOGEW + 1) return launch_pass_wave_split<true>(p, grid, stream);
        if constexpr (!TWIDDLE) {
            switch (logr) {
                case 1: return launch_pass_wave<1, false>(p, grid, stream);
                case 2: return launch_pass_wave<2, false>(p, grid, stream);
                case 3: return launch_pass_wave<3, false>(p, grid, stream);
                default: break;
            }
        }
    }
    switch (logr) {
#define CASE(L) \
    case L:     \
        return launch_pass<L, TWIDDLE>(p, grid, stream);
        CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
#undef CASE
        default:
            break;
    }
    if constexpr (!TWIDDLE) {
        switch (logr) {
            case 1: return launch_pass<1, false>(p, grid, stream);
            case 2: return launch_pass<2, false>(p, grid, stream);
            case 3: return launch_pass<3, false>(p, grid, stream);
            case 11: return launch_pass<11, false>(p, grid, stream);
            case 12: return launch_pass<12, false>(p, grid, stream);
            default: break;
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Planner
// ---------------------------------------------------------------------------------------------

static void base_params(PassParams &p, const NttTables &tb) {
    p = PassParams{};
    p.twl = tb.twl;
    p.twh = tb.twh;
    p.scale = 1;
    p.chain_scale = 1;
}

// Sweep direction of a plan's passes (PassParams::sweep_down): up, down, up. A pass then starts on the polynomials the pass before it
// wrote last instead of on the ones written longest ago, and a caller's next transform of the same buffer starts where this one's last
// pass ended. 64 x 2^20 natural order is 3-4 % faster for it (profiles/ntt_infinity_cache.jsonl); that the 256 MiB Infinity Cache serves
// those first reads is the hypothesis this was built on (LABNOTES 14 says what is measured and what is not). Only the polynomial index is mirrored,
// and only by the direct column pass and the natural-order row pass (ntt_direct.hip): a pass of any other kernel, and the block index z
// of the three-pass plans' middle pass, walk upwards as before.
static uint32_t sweep_of_pass(int pass) { return (uint32_t)(pass & 1); }

// Passes whose global accesses are segments of T elements (column passes, transposed natural-order stores) use tiles of
// 2^(LOGE+1) elements when the wave kernel can take them: T doubles, and so do the segments (64 -> 128 bytes at 2^20).
// PLONKY2_NTT_WIDE=0 keeps the 8192-element tiles (A/B measurements).
static bool wide_ok(uint32_t logr, uint64_t t_limit) {
    static const bool enabled = [] {
        const char *e = PLONKY2_KNOB("PLONKY2_NTT_WIDE");
        return !(e && e[0] == '0');
    }();
    return enabled && use_wave_kernel() && logr >= (uint32_t)WIDE_MIN_LOGR && logr <= (uint32_t)LOGEW + 1 &&  // LOGEW + 1: split columns
           (t_limit & ((1ull << (LOGE + 1 - logr)) - 1)) == 0;
}

// 2^22 natural-order forward transforms in two passes (round 5). PLONKY2_NTT_TWO_PASS_22=0 in the diagnostic build restores the
// three-pass plan (A/B measurements).
static bool two_pass_2p22() {
    static const bool enabled = [] {
        const char *e = PLONKY2_KNOB("PLONKY2_NTT_TWO_PASS_22");
        return !(e && e[0] == '0');
    }();
    return enabled && direct_mode();
}

hipError_t ntt_batch(const NttTables &tb, const uint64_t *src, uint64_t *dst, uint64_t n_polys, uint32_t log_n,
                     uint64_t src_stride, uint64_t dst_stride, NttOrder order, bool inverse, hipStream_t stream) {
    if (log_n > NTT_MAX_LOG) return hipErrorInvalidValue;
    if (n_polys == 0) return hipSuccess;
    const uint64_t n = 1ull << log_n;
    if (log_n == 0) {
        if (src != dst)
            for (uint64_t i = 0; i < n_polys; i++) {
                hipError_t e = hipMemcpyAsync(dst + i * dst_stride, src + i * src_stride, 8, hipMemcpyDeviceToDevice, stream);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    }
    const bool natural = order == NttOrder::Natural;
    const uint64_t n_inv = inverse ? (glh::P - ((glh::P - 1) >> log_n)) : 1;  // types.rs:227-266
    PassParams p;

    if (log_n <= 12) {
        // one pass: tile rows = T different polynomials
        base_params(p, tb);
        uint32_t logt = LOGE - log_n, T = 1u << logt;
        p.src = src;
        p.dst = dst;
        p.logt = logt;
        p.t_limit = (uint32_t)n_polys;
        p.in_sb = (uint64_t)T * src_stride;
        p.in_t = src_stride;
        p.in_m = 1;
        p.out_sb = (uint64_t)T * dst_stride;
        p.out_t = dst_stride;
        p.out_m = 1;
        p.flags = F_LOAD_ROWS | F_STORE_ROWS | (natural ? F_NATURAL : 0) | (inverse ? F_INVERSE : 0);
        p.log_n = log_n;
        p.scale = n_inv;
        if (inverse && (dst_stride & (n - 1))) return hipErrorInvalidValue;
        if (n_polys > 0xFFFFFFFFull) return hipErrorInvalidValue;
        dim3 grid((unsigned)((n_polys + T - 1) / T), 1, 1);
        return dispatch_pass<false>(log_n, p, grid, stream);
    }

    if (log_n == 22 && natural && two_pass_2p22()) {
        if (inverse && (dst_stride & (n - 1))) return hipErrorInvalidValue;
        // 2^22 = 2048 x 2048 in TWO passes, both the direct column pass with eight lane groups (tiles of 2048 rows x 8 columns,
        // 64-byte segments): pass A takes the columns L of the matrix [m][L] (stride 2048), applies w_n^(L k1) and stores its tile
        // TRANSPOSED into the workspace, mid[L * 2048 + k1]; pass B takes the columns k1 of that matrix [L][k1], has no twiddle left to
        // apply and writes X[k1 + 2048 k2] in natural order. HBM-side traffic 2 x the algorithmic bytes instead of the three-pass
        // plan's 3 x (round 4 priced this plan at the three-pass plan's time from memory-only measurements; round 5 measures it:
        // profiles/r05_ntt_sizes.jsonl). The INVERSE (round 6) is the same plan on the index-reversed input, ifft(x) = fft(x') / n with
        // x'[j] = x[(n - j) mod n]: pass A reads its columns backwards (ntt_direct.hip REVIN) and carries 1 / n on its twiddle chain.
        const uint64_t N1 = 2048, C = 8;
        if (!tb.scratch || tb.scratch_elems < n) return hipErrorInvalidValue;
        const uint64_t chunk = tb.scratch_elems / n;
        for (uint64_t off = 0; off < n_polys; off += chunk) {
            const uint64_t cnt = n_polys - off < chunk ? n_polys - off : chunk;
            base_params(p, tb);
            p.src = src + off * src_stride;
            p.dst = tb.scratch;
            p.logt = 3;
            p.t_limit = (uint32_t)N1;
            p.in_sa = src_stride;
            p.in_sb = C;
            p.in_t = 1;
            p.in_m = N1;
            p.out_sa = n;
            p.out_sb = C * N1;   // column tile b of the input = rows [8 b, 8 b + 8) of the transposed matrix
            p.out_t = 1;
            p.out_m = 1;         // output frequency k1 runs along the row
            p.out_c = N1;        // the tile's columns L are N1 elements apart
            p.flags = F_NATURAL | F_WIDE | F_RAW_OUT;
            p.log_n = log_n;
            p.tw_hi = log_n;
            p.chain_scale = n_inv;
            hipError_t e = inverse ? nttk::launch_col_direct_reversed_input(p, dim3((unsigned)(N1 / C), (unsigned)cnt, 1), stream)
                                   : nttk::launch_col_direct(3, p, dim3((unsigned)(N1 / C), (unsigned)cnt, 1), stream);
            if (e != hipSuccess) return e;
            base_params(p, tb);
            p.src = tb.scratch;
            p.dst = dst + off * dst_stride;
            p.logt = 3;
            p.t_limit = (uint32_t)N1;
            p.in_sa = n;
            p.in_sb = C;
            p.in_t = 1;
            p.in_m = N1;
            p.out_sa = dst_stride;
            p.out_sb = C;
            p.out_t = 1;
            p.out_m = N1;
            p.flags = F_NATURAL | F_WIDE | F_FINAL_COL;
            p.log_n = log_n;
            p.sweep_down = sweep_of_pass(1);
            e = nttk::launch_col_direct_final(p, dim3((unsigned)(N1 / C), (unsigned)cnt, 1), stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }

    // 2^22 bit-reversed as 2048 x 2048 in two passes IN PLACE (round 6): the eight-lane-group column pass, then the in-place row pass
    // over 2048-point rows with two waves per row (ntt_direct.hip, HALVES). PLONKY2_NTT_TWO_PASS_22_INPLACE=0 in the diagnostic build
    // restores the three-pass plan, =generic takes the round-1 kernel for the rows (the first measurement of this plan: slower).
    static const int two_pass_22_inplace = [] {
        const char *e = PLONKY2_KNOB("PLONKY2_NTT_TWO_PASS_22_INPLACE");
        return !direct_mode() ? 0 : (e && e[0] == '0') ? 0 : (e && e[0] == 'g') ? 2 : 1;
    }();
    if (log_n <= 20 || (log_n == 21 && wide_ok(11, 1024)) || (log_n == 22 && !natural && two_pass_22_inplace && wide_ok(11, 2048))) {
        // two passes: n = N1 * N2, N1 = 2^la (strided "column" pass), N2 = 2^lb (row pass); 2^21 = 2048 x 1024 with the
        // column pass on split columns
        uint32_t la = (log_n + 1) / 2, lb = log_n - la;
        // 2^18 = 256 x 1024 and 2^19 = 512 x 1024 instead of 512 x 512 / 1024 x 512: both passes then have a direct kernel (columns of
        // 256 / 512 points, rows of 1024)
        if (direct_mode() && (log_n == 18 || log_n == 19)) lb = 10, la = log_n - 10;
        const uint64_t N1 = 1ull << la, N2 = 1ull << lb;
        // measured at 2^20 on one device: wide tiles make the column pass 6 % faster and the transposed-store row pass 4 % slower
        // the direct row pass (1024-point rows, natural order) works on tiles of sixteen rows
        const bool wideA = wide_ok(la, N2), wideB = natural && lb == 10 && direct_mode() && wide_ok(lb, N1);
        const uint32_t logtA = LOGE + wideA - la, TA = 1u << logtA, logtB = LOGE + wideB - lb, TB = 1u << logtB;
        if (inverse && !natural) return hipErrorInvalidValue;  // bit-reversed inverse is not on the path
        if (inverse && (dst_stride & (n - 1))) return hipErrorInvalidValue;
        // Bit-reversed order: both passes rewrite exactly the addresses they read -> in place.
        // Natural order: pass B writes its tile transposed (k1 + N1*k2), i.e. into rows that other
        // workgroups still have to read, so the intermediate goes through the scratch workspace,
        // a chunk of columns at a time (the chunk's intermediate stays in L2 / Infinity Cache).
        // The two-waves-per-row pass over 2048-point rows (2^22 bit-reversed) is NOT in place either: a row's two waves each read the
        // whole row and each write half of it, with nothing ordering one wave's stores behind the other's loads — its input is the
        // workspace, like the natural-order plans' (found by the 18-column test of round 6: one column passed by timing alone).
        const bool halves_rows = log_n == 22 && !natural && two_pass_22_inplace == 1;
        const bool via_workspace = natural || halves_rows;
        uint64_t chunk = 65535;
        if (via_workspace) {
            if (!tb.scratch || tb.scratch_elems < n) return hipErrorInvalidValue;
            chunk = tb.scratch_elems / n;
            if (chunk > 65535) chunk = 65535;
        }
        if (const char *ev = PLONKY2_KNOB("PLONKY2_NTT_CHUNK_COLS")) {  // tuning knob (tools/ntt_chunk_sweep.py)
            uint64_t c = strtoull(ev, nullptr, 10);
            if (c >= 1 && c < chunk) chunk = c;
        }
        for (uint64_t off = 0; off < n_polys; off += chunk) {
            const uint64_t cnt = n_polys - off < chunk ? n_polys - off : chunk;
            uint64_t *mid = via_workspace ? tb.scratch : dst + off * dst_stride;
            const uint64_t mid_stride = via_workspace ? n : dst_stride;
            // pass A
            base_params(p, tb);
            p.src = src + off * src_stride;
            p.dst = mid;
            p.logt = logtA;
            p.t_limit = (uint32_t)N2;
            p.in_sa = src_stride;
            p.in_sb = TA;
            p.in_t = 1;
            p.in_m = N2;
            p.out_sa = mid_stride;
            p.out_sb = TA;
            p.out_t = 1;
            p.out_m = N2;
            p.flags = (natural ? F_NATURAL : 0) | (wideA ? F_WIDE : 0) | F_RAW_OUT;
            p.log_n = log_n;
            p.tw_hi = log_n;
            p.chain_scale = n_inv;  // the inverse's n^-1 rides on the twiddle chain (1 multiply per thread)
            hipError_t e = dispatch_pass<true>(la, p, dim3((unsigned)(N2 / TA), (unsigned)cnt, 1), stream);
            if (e != hipSuccess) return e;
            // pass B
            base_params(p, tb);
            p.src = mid;
            p.dst = dst + off * dst_stride;
            p.logt = logtB;
            p.t_limit = (uint32_t)N1;
            p.in_sa = mid_stride;
            p.in_sb = (uint64_t)TB * N2;
            p.in_t = N2;
            p.in_m = 1;
            p.out_sa = dst_stride;
            p.log_n = log_n;
            p.sweep_down = sweep_of_pass(1);
            if (natural) {
                p.out_sb = TB;
                p.out_t = 1;
                p.out_m = N1;
                p.flags = F_LOAD_ROWS | F_NATURAL | (inverse ? F_INVERSE : 0) | (wideB ? F_WIDE : 0);
                p.row_shift = inverse ? 1 : 0;
            } else {
                p.out_sb = (uint64_t)TB * N2;
                p.out_t = N2;
                p.out_m = 1;
                p.flags = F_LOAD_ROWS | F_STORE_ROWS;
            }
            if (halves_rows)
                e = nttk::launch_row_inplace_direct_2048(p, dim3((unsigned)(N1 / TB), (unsigned)cnt, 1), stream);
            else
                e = dispatch_pass<false>(lb, p, dim3((unsigned)(N1 / TB), (unsigned)cnt, 1), stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // three passes (2^21 .. 2^24): n = N1*N2*N3, index j = j1*N2N3 + j2*N3 + j3.
    //   pass 1: column pass over the whole polynomial (N1 points, stride N2N3, twiddle w_n^(L*k1))
    //   pass 2: column pass inside each of the N1 blocks (N2 points, stride N3, twiddle w_{N2N3}^(j3*k2))
    //   pass 3: row pass over rows of N3 contiguous points
    // Bit-reversed order runs all three in place; natural order keeps the intermediate in the
    // scratch workspace and lets pass 3 write X[k1 + N1*k2 + N1*N2*k3] (T adjacent k1 per segment).
    {
        uint32_t la = (log_n + 2) / 3, lb = (log_n - la + 1) / 2, lc = log_n - la - lb;
        // the direct column passes take 256-point columns: 2^22 = 256 x 256 x 64 instead of 256 x 128 x 128
        if (direct_mode() && log_n == 22) la = 8, lb = 8, lc = 6;
        const uint64_t N1 = 1ull << la, N2 = 1ull << lb, N3 = 1ull << lc, N23 = N2 * N3;
        const bool wide1 = direct_mode() && wide_ok(la, N23), wide2 = direct_mode() && wide_ok(lb, N3);   // 16384-element tiles: the direct passes' geometry
        const uint32_t logt1 = LOGE + wide1 - la, T1 = 1u << logt1, logt2 = LOGE + wide2 - lb, T2 = 1u << logt2, logt3 = LOGE - lc,
                       T3 = 1u << logt3;
        if (inverse && !natural) return hipErrorInvalidValue;
        if (inverse && (dst_stride & (n - 1))) return hipErrorInvalidValue;
        uint64_t chunk = 65535;
        if (natural) {
            if (!tb.scratch || tb.scratch_elems < n) return hipErrorInvalidValue;
            chunk = tb.scratch_elems / n;
        }
        for (uint64_t off = 0; off < n_polys; off += chunk) {
            const uint64_t cnt = n_polys - off < chunk ? n_polys - off : chunk;
            uint64_t *mid = natural ? tb.scratch : dst + off * dst_stride;
            const uint64_t mid_stride = natural ? n : dst_stride;
            base_params(p, tb);
            p.src = src + off * src_stride;
            p.dst = mid;
            p.logt = logt1;
            p.t_limit = (uint32_t)N23;
            p.in_sa = src_stride;
            p.in_sb = T1;
            p.in_t = 1;
            p.in_m = N23;
            p.out_sa = mid_stride;
            p.out_sb = T1;
            p.out_t = 1;
            p.out_m = N23;
            p.flags = (natural ? F_NATURAL : 0) | F_RAW_OUT | (wide1 ? F_WIDE : 0);
            p.log_n = log_n;
            p.tw_hi = log_n;
            p.chain_scale = n_inv;
            hipError_t e = dispatch_pass<true>(la, p, dim3((unsigned)(N23 / T1), (unsigned)cnt, 1), stream);
            if (e != hipSuccess) return e;
            base_params(p, tb);
            p.src = mid;
            p.dst = mid;
            p.logt = logt2;
            p.t_limit = (uint32_t)N3;
            p.in_sa = mid_stride;
            p.in_sb = T2;
            p.in_sz = N23;
            p.in_t = 1;
            p.in_m = N3;
            p.out_sa = mid_stride;
            p.out_sb = T2;
            p.out_sz = N23;
            p.out_t = 1;
            p.out_m = N3;
            p.flags = (natural ? F_NATURAL : 0) | F_RAW_OUT | (wide2 ? F_WIDE : 0);
            p.log_n = log_n;
            p.tw_hi = lb + lc;
            p.sweep_down = sweep_of_pass(1);
            e = dispatch_pass<true>(lb, p, dim3((unsigned)(N3 / T2), (unsigned)cnt, (unsigned)N1), stream);
            if (e != hipSuccess) return e;
            base_params(p, tb);
            p.src = mid;
            p.dst = dst + off * dst_stride;
            p.logt = logt3;
            p.in_sa = mid_stride;
            p.in_m = 1;
            p.out_sa = dst_stride;
            p.log_n = log_n;
            if (natural) {
                p.row_shift = inverse ? 1 : 0;
                // tile = T3 rows with consecutive k1 at fixed k2 (blockIdx.z): row (k1, k2) starts at (k1*N2 + k2)*N3
                p.t_limit = (uint32_t)N1;
                p.in_sb = (uint64_t)T3 * N23;
                p.in_sz = N3;
                p.in_t = N23;
                p.out_sb = T3;
                p.out_sz = N1;
                p.out_t = 1;
                p.out_m = N1 * N2;
                p.flags = F_LOAD_ROWS | F_NATURAL | (inverse ? F_INVERSE : 0);
                e = dispatch_pass<false>(lc, p, dim3((unsigned)(N1 / T3), (unsigned)cnt, (unsigned)N2), stream);
            } else {
                p.t_limit = (uint32_t)(N1 * N2);
                p.in_sb = (uint64_t)T3 * N3;
                p.in_t = N3;
                p.out_sb = (uint64_t)T3 * N3;
                p.out_t = N3;
                p.out_m = 1;
                p.flags = F_LOAD_ROWS | F_STORE_ROWS;
                e = dispatch_pass<false>(lc, p, dim3((unsigned)(N1 * N2 / T3), (unsigned)cnt, 1), stream);
            }
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
}

// ---------------------------------------------------------------------------------------------
// Tables
// ---------------------------------------------------------------------------------------------

hipError_t ntt_tables_create(NttTables *tb) {
    uint64_t *h = (uint64_t *)malloc(2 * 4096 * sizeof(uint64_t));
    if (!h) return hipErrorOutOfMemory;
    const uint64_t w24 = glh::root_of_unity(24), w12 = glh::root_of_unity(12);
    uint64_t a = 1, b = 1;
    for (int e = 0; e < 4096; e++) {
        h[e] = a;
        h[4096 + e] = b;
        a = glh::mul(a, w24);
        b = glh::mul(b, w12);
    }
    hipError_t e = hipMalloc(&tb->twl, 2 * 4096 * sizeof(uint64_t));
    if (e != hipSuccess) {
        free(h);
        return e;
    }
    tb->twh = tb->twl + 4096;
    e = hipMemcpy(tb->twl, h, 2 * 4096 * sizeof(uint64_t), hipMemcpyHostToDevice);
    free(h);
    // the workspace (`scratch`) belongs to a context, not to the device: ctx.h CtxState
    return e;
}

void ntt_tables_destroy(NttTables *tb) {
    if (tb->twl) (void)hipFree(tb->twl);
    if (tb->scratch) (void)hipFree(tb->scratch);
    tb->twl = tb->twh = tb->scratch = nullptr;
}

namespace {
__global__ void coset_tables_kernel(uint64_t *lo, uint64_t *hi, uint32_t hi_len, uint32_t n_cosets, uint64_t shift,
                                    uint64_t w_ext) {
    uint32_t per = 1024 + hi_len;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cosets * per) return;
    uint32_t r = i / per, e = i % per;
    uint64_t s = gl::mul(shift, gl::pow(w_ext, r));
    if (e < 1024)
        lo[r * 1024 + e] = gl::canon(gl::pow(s, e));
    else
        hi[r * hi_len + (e - 1024)] = gl::canon(gl::pow(s, (uint64_t)(e - 1024) << 10));
}

// dst[(poly, block q, i)] = coeffs[poly, i] * s_{bitrev(q)}^i  (small-n LDE path)
__global__ void coset_scale_kernel(const uint64_t *coeffs, uint64_t *dst, const uint64_t *lo, const uint64_t *hi,
                                   uint32_t hi_len, uint32_t log_n, uint32_t rate_bits, uint64_t src_stride,
                                   uint64_t dst_stride, uint64_t total) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint64_t n = 1ull << log_n;
    uint64_t i = g & (n - 1);
    uint32_t q = (uint32_t)(g >> log_n) & ((1u << rate_bits) - 1);
    uint64_t poly = g >> (log_n + rate_bits);
    uint32_t r = rate_bits ? (__brev(q) >> (32 - rate_bits)) : 0;
    uint64_t sc = gl::mul(hi[r * hi_len + (uint32_t)(i >> 10)], lo[r * 1024 + (uint32_t)(i & 1023)]);
    dst[poly * dst_stride + (uint64_t)q * n + i] = gl::mul(coeffs[poly * src_stride + i], sc);
}
// v[poly*stride + i] *= s^i  (coset_fft_with_options' shift.powers() scaling, polynomial/mod.rs:292-297,
// and coset_ifft's shift^-i, polynomial/mod.rs:64-77); lo/hi are the coset tables of s (one coset).
__global__ void scale_by_powers_kernel(uint64_t *v, const uint64_t *lo, const uint64_t *hi, uint32_t log_n, uint64_t stride,
                                       uint64_t total) {
    uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    uint64_t i = g & ((1ull << log_n) - 1), poly = g >> log_n;
    uint64_t sc = gl::mul(hi[(uint32_t)(i >> 10)], lo[(uint32_t)(i & 1023)]);
    uint64_t *p = v + poly * stride + i;
    *p = gl::canon(gl::mul(*p, sc));
}
}  // namespace

hipError_t scale_by_powers(const CosetTables &ct, uint64_t *values, uint64_t n_polys, uint64_t stride, hipStream_t stream) {
    uint64_t total = n_polys << ct.log_n;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(scale_by_powers_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, values, ct.lo, ct.hi,
                       ct.log_n, stride, total);
    return hipGetLastError();
}

hipError_t coset_tables_create(CosetTables *ct, uint32_t log_n, uint32_t rate_bits, uint64_t shift, hipStream_t stream) {
    if (log_n + rate_bits > 32 || rate_bits > 8) return hipErrorInvalidValue;
    uint32_t n_cosets = 1u << rate_bits;
    uint32_t hi_len = log_n > 10 ? (1u << (log_n - 10)) : 1;
    size_t total = (size_t)n_cosets * (1024 + hi_len);
    hipError_t e = hipMalloc(&ct->lo, total * sizeof(uint64_t));
    if (e != hipSuccess) return e;
    ct->hi = ct->lo + (size_t)n_cosets * 1024;
    ct->hi_len = hi_len;
    ct->log_n = log_n;
    ct->rate_bits = rate_bits;
    ct->shift = shift;
    uint64_t w_ext = glh::root_of_unity(log_n + rate_bits);
    hipLaunchKernelGGL(coset_tables_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ct->lo, ct->hi,
                       hi_len, n_cosets, shift % glh::P, w_ext);
    return hipGetLastError();
}

void coset_tables_destroy(CosetTables *ct) {
    if (ct->lo) (void)hipFree(ct->lo);
    ct->lo = ct->hi = nullptr;
}

hipError_t coset_lde_batch(const NttTables &tb, const CosetTables &ct, const uint64_t *coeffs, uint64_t *dst,
                           uint64_t n_polys, uint64_t src_stride, uint64_t dst_stride, hipStream_t stream) {
    const uint32_t log_n = ct.log_n, rate_bits = ct.rate_bits;
    const uint64_t n = 1ull << log_n, n_cosets = 1ull << rate_bits;
    if (n_polys == 0) return hipSuccess;
    if (log_n > NTT_MAX_LOG) return hipErrorInvalidValue;
    if (log_n <= 12) {
        // small polynomials: scaled copies, then 2^rate_bits * n_polys in-place bit-reversed NTTs
        uint64_t total = n_polys * n_cosets * n;
        hipLaunchKernelGGL(coset_scale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, coeffs, dst,
                           ct.lo, ct.hi, ct.hi_len, log_n, rate_bits, src_stride, dst_stride, total);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (dst_stride == n_cosets * n)
            return ntt_batch(tb, dst, dst, n_polys * n_cosets, log_n, n, n, NttOrder::BitReversed, false, stream);
        for (uint64_t i = 0; i < n_polys; i++) {
            e = ntt_batch(tb, dst + i * dst_stride, dst + i * dst_stride, n_cosets, log_n, n, n, NttOrder::BitReversed,
                          false, stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    if (log_n > 21 || (log_n == 21 && !wide_ok(11, 1024))) {
        // three-pass sizes; passes 2 and 3 enumerate (polynomial, coset block) as one index with stride n, so they need the coset
        // blocks of all polynomials of a launch contiguous (dst_stride = n << rate_bits): with a padded dst_stride the polynomials
        // go one call at a time, as in the small path above (a polynomial's own blocks are always contiguous)
        if (dst_stride != n_cosets * n) {
            for (uint64_t i = 0; i < n_polys; i++) {
                hipError_t e = coset_lde_batch(tb, ct, coeffs + i * src_stride, dst + i * dst_stride, 1, src_stride, n_cosets * n, stream);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        }
        const uint32_t la = (log_n + 2) / 3, lb = (log_n - la + 1) / 2, lc = log_n - la - lb;
        const uint64_t N1 = 1ull << la, N2 = 1ull << lb, N3 = 1ull << lc, N23 = N2 * N3;
        const uint32_t logt1 = LOGE - la, T1 = 1u << logt1, logt2 = LOGE - lb, T2 = 1u << logt2, logt3 = LOGE - lc,
                       T3 = 1u << logt3;
        const uint64_t max_polys = 65535 / n_cosets;
        for (uint64_t off = 0; off < n_polys; off += max_polys) {
            uint64_t cnt = n_polys - off < max_polys ? n_polys - off : max_polys;
            PassParams p;
            base_params(p, tb);
            p.src = coeffs + off * src_stride;
            p.dst = dst + off * dst_stride;
            p.cs_hi = ct.hi;
            p.cs_lo = ct.lo;
            p.cs_hi_len = ct.hi_len;
            p.rate_bits = rate_bits;
            p.logt = logt1;
            p.t_limit = (uint32_t)N23;
            p.in_sa = src_stride;
            p.in_sb = T1;
            p.in_t = 1;
            p.in_m = N23;
            p.out_sa = dst_stride;
            p.out_sb = T1;
            p.out_sz = n;
            p.out_t = 1;
            p.out_m = N23;
            p.flags = F_COSET | F_RAW_OUT;
            p.log_n = log_n;
            p.tw_hi = log_n;
            hipError_t e = dispatch_pass<true>(la, p, dim3((unsigned)(N23 / T1), (unsigned)cnt, (unsigned)n_cosets), stream);
            if (e != hipSuccess) return e;
            base_params(p, tb);  // pass 2: y enumerates (poly, coset block), z = slot m1
            p.src = dst + off * dst_stride;
            p.dst = dst + off * dst_stride;
            p.logt = logt2;
            p.t_limit = (uint32_t)N3;
            p.in_sa = n;
            p.in_sb = T2;
            p.in_sz = N23;
            p.in_t = 1;
            p.in_m = N3;
            p.out_sa = n;
            p.out_sb = T2;
            p.out_sz = N23;
            p.out_t = 1;
            p.out_m = N3;
            p.flags = F_RAW_OUT;
            p.log_n = log_n;
            p.tw_hi = lb + lc;
            e = dispatch_pass<true>(lb, p, dim3((unsigned)(N3 / T2), (unsigned)(cnt * n_cosets), (unsigned)N1), stream);
            if (e != hipSuccess) return e;
            base_params(p, tb);  // pass 3: rows of N3, in place
            p.src = dst + off * dst_stride;
            p.dst = dst + off * dst_stride;
            p.logt = logt3;
            p.t_limit = (uint32_t)(N1 * N2);
            p.in_sa = n;
            p.in_sb = (uint64_t)T3 * N3;
            p.in_t = N3;
            p.in_m = 1;
            p.out_sa = n;
            p.out_sb = (uint64_t)T3 * N3;
            p.out_t = N3;
            p.out_m = 1;
            p.flags = F_LOAD_ROWS | F_STORE_ROWS;
            p.log_n = log_n;
            e = dispatch_pass<false>(lc, p, dim3((unsigned)(N1 * N2 / T3), (unsigned)(cnt * n_cosets), 1), stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // two-pass sizes: the coset scaling is fused into pass A (input scale (s^N2)^j1 on load,
    // s^j2 folded into the inter-pass twiddle chain); coefficients are read once per coset from
    // L2/Infinity Cache and each coset block is written in place by pass B.
    uint32_t la = (log_n + 1) / 2, lb = log_n - la;
    if (direct_mode() && (log_n == 18 || log_n == 19)) lb = 10, la = log_n - 10;  // as ntt_batch: direct kernels for both passes
    const uint64_t N1 = 1ull << la, N2 = 1ull << lb;
    for (uint64_t off = 0; off < n_polys; off += 65535) {
        uint64_t cnt = n_polys - off < 65535 ? n_polys - off : 65535;
        PassParams p;
        base_params(p, tb);
        const bool wideA = wide_ok(la, N2);
        uint32_t logtA = LOGE + wideA - la, TA = 1u << logtA;
        p.src = coeffs + off * src_stride;
        p.dst = dst + off * dst_stride;
        p.cs_hi = ct.hi;
        p.cs_lo = ct.lo;
        p.cs_hi_len = ct.hi_len;
        p.rate_bits = rate_bits;
        p.logt = logtA;
        p.t_limit = (uint32_t)N2;
        p.in_sa = src_stride;
        p.in_sb = TA;
        p.in_sz = 0;
        p.in_t = 1;
        p.in_m = N2;
        p.out_sa = dst_stride;
        p.out_sb = TA;
        p.out_sz = n;
        p.out_t = 1;
        p.out_m = N2;
        p.flags = F_COSET | F_RAW_OUT | (wideA ? F_WIDE : 0);
        p.log_n = log_n;
        p.tw_hi = log_n;
        hipError_t e = dispatch_pass<true>(la, p, dim3((unsigned)(N2 / TA), (unsigned)cnt, (unsigned)n_cosets), stream);
        if (e != hipSuccess) return e;
        base_params(p, tb);
        uint32_t logtB = LOGE - lb, TB = 1u << logtB;
        p.src = dst + off * dst_stride;
        p.dst = dst + off * dst_stride;
        p.logt = logtB;
        p.t_limit = (uint32_t)N1;
        p.in_sa = dst_stride;
        p.in_sb = (uint64_t)TB * N2;
        p.in_sz = n;
        p.in_t = N2;
        p.in_m = 1;
        p.out_sa = dst_stride;
        p.out_sb = (uint64_t)TB * N2;
        p.out_sz = n;
        p.out_t = N2;
        p.out_m = 1;
        p.flags = F_LOAD_ROWS | F_STORE_ROWS;
        p.log_n = log_n;
        e = dispatch_pass<false>(lb, p, dim3((unsigned)(N1 / TB), (unsigned)cnt, (unsigned)n_cosets), stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace plonky2_hip
