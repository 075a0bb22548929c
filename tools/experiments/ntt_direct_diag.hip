// Diagnostic builds of the direct NTT passes (csrc/ntt_direct.hip): this translation unit sets the hook points of that file from
// -DDIRECT_DIAG_* flags and includes it. NEVER the product — the results of most variants are wrong by design; they answer "what
// does this part of the pass cost" (tools/gpu_runs/ntt_direct_variants.sh, profiles/r03_ntt_direct_diagnostic_variants.jsonl):
//   DIRECT_DIAG_SAME_LOADS   every tile loads tile 0's addresses (served by L2)     -> what the load latency costs
//   DIRECT_DIAG_SAME_STORES  every tile stores to tile 0's addresses                 -> what the store traffic costs
//   DIRECT_DIAG_NO_BARRIER   the two workgroup barriers of a tile are dropped        -> what waiting for the slowest wave costs
//   DIRECT_DIAG_TAIL_FRONT   the sixteen tail steps run before the first rounds      -> what spreading the stores buys
//   DIRECT_DIAG_NT_{LOAD,STORE}_{COL,ROW}   nontemporal loads / stores in either pass
//   DIRECT_DIAG_TOUCH_AHEAD=D   touch-ahead (results stay right): behind the first radix stage of the tile in A every lane reads one dword
//                            of one 128-byte line of the tile the workgroup loads D tiles after the one whose register loads close the
//                            iteration (column pass: 1024 lanes = the tile's 1024 lines; row pass: a wave's 64 lines of its row). Measured
//                            and rejected, 8-12 % slower at D = 1 (LABNOTES 14, profiles/ntt_infinity_cache.jsonl)
//   DIRECT_DIAG_NT_TOUCH     ... with nontemporal touches                              -> what a line's second trip into L2 costs
#define DIRECT_DIAG_HOOKS
#ifdef DIRECT_DIAG_NO_BARRIER
#define DIRECT_TILE_BARRIER() tile_sync<64>()
#else
#define DIRECT_TILE_BARRIER() lds_barrier()
#endif
#ifdef DIRECT_DIAG_SAME_LOADS
#define DIRECT_LOAD_TILE(t) 0u
#else
#define DIRECT_LOAD_TILE(t) (t)
#endif
#ifdef DIRECT_DIAG_SAME_STORES
#define DIRECT_STORE_TILE(t) 0u
#define DIRECT_DIAG_SAME_STORES_ON 1
#else
#define DIRECT_STORE_TILE(t) (t)
#define DIRECT_DIAG_SAME_STORES_ON 0
#endif
#ifdef DIRECT_DIAG_TAIL_FRONT
#define DIRECT_DIAG_TAIL_FRONT_ON 1
#else
#define DIRECT_DIAG_TAIL_FRONT_ON 0
#endif
#ifdef DIRECT_DIAG_NT_LOAD_COL
#define DIRECT_NT_LOAD_COL true
#else
#define DIRECT_NT_LOAD_COL false
#endif
#ifdef DIRECT_DIAG_NT_STORE_COL
#define DIRECT_NT_STORE_COL true
#else
#define DIRECT_NT_STORE_COL false
#endif
#ifdef DIRECT_DIAG_NT_LOAD_ROW
#define DIRECT_NT_LOAD_ROW true
#else
#define DIRECT_NT_LOAD_ROW false
#endif
#ifdef DIRECT_DIAG_NT_STORE_ROW
#define DIRECT_NT_STORE_ROW true
#else
#define DIRECT_NT_STORE_ROW false
#endif
#ifdef DIRECT_DIAG_TOUCH_AHEAD
#include <hip/hip_runtime.h>
#include <cstdint>
// One dword of a 128-byte line, for the line's sake. The result is kept in one register and "used" by an empty asm one iteration later,
// where every load issued before it has long been waited for: the compiler may neither drop the load nor wait for it early. The touch
// sits BEHIND the first radix stage because vmcnt counts in order: issued before that stage's waits it would have to be back from HBM
// before the stage could start. The lane's index comes from registers the loop keeps (wave, opaque_lane()), not from threadIdx.x.
__device__ __forceinline__ uint32_t diag_touch(const uint64_t *base, uint32_t byte_off) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(reinterpret_cast<const unsigned char *>(base) + byte_off);
#ifdef DIRECT_DIAG_NT_TOUCH
    return __builtin_nontemporal_load(q);
#else
    return *q;
#endif
}
#define DIRECT_TOUCH_STATE uint32_t touched = 0;
// the tile is one this workgroup loads (guarded by its tile count like issue_loads), the addresses are addresses issue_loads reads
#define DIRECT_TOUCH_COL(t_in_a)                                                                                                   \
    do {                                                                                                                           \
        if constexpr (with_tail && LOGG <= 2 && !COSET && !FINAL && !REVIN) {                                                      \
            asm volatile("" : : "v"(touched));                                                                                     \
            if ((t_in_a) + 1 + DIRECT_DIAG_TOUCH_AHEAD < n_tiles) {                                                                \
                uint32_t tb_, ta_, tz_;                                                                                            \
                tile_of((t_in_a) + 1 + DIRECT_DIAG_TOUCH_AHEAD, tb_, ta_, tz_);                                                    \
                const uint32_t tl_ = wave * 64 + opaque_lane();                                                                    \
                constexpr uint32_t LPR_ = LOGG <= 2 ? 4 >> LOGG : 1; /* 128-byte lines per row of the tile */                      \
                touched = diag_touch(p.src + (ta_ * p.in_sa + tb_ * p.in_sb + tz_ * p.in_sz),                                      \
                                     (uint32_t)(((tl_ & (LPR_ - 1)) * 16 + (uint64_t)(tl_ / LPR_) * p.in_m) * 8));                 \
                __builtin_amdgcn_sched_barrier(0);                                                                                 \
            }                                                                                                                      \
        }                                                                                                                          \
    } while (0)
#define DIRECT_TOUCH_ROW(t_in_a)                                                                                                   \
    do {                                                                                                                           \
        if constexpr (with_tail) {                                                                                                 \
            asm volatile("" : : "v"(touched));                                                                                     \
            if ((t_in_a) + 1 + DIRECT_DIAG_TOUCH_AHEAD < n_tiles) {                                                                \
                uint32_t tb_, ta_, tz_;                                                                                            \
                tile_of((t_in_a) + 1 + DIRECT_DIAG_TOUCH_AHEAD, tb_, ta_, tz_);                                                    \
                const uint32_t trow_ = (tb_ * 16 + wave + p.row_shift) & (p.t_limit - 1);                                          \
                touched = diag_touch(p.src + (ta_ * p.in_sa + tz_ * p.in_sz + (uint64_t)trow_ * p.in_t), opaque_lane() * 128);     \
                __builtin_amdgcn_sched_barrier(0);                                                                                 \
            }                                                                                                                      \
        }                                                                                                                          \
    } while (0)
#else
#define DIRECT_TOUCH_STATE
#define DIRECT_TOUCH_COL(t_in_a)
#define DIRECT_TOUCH_ROW(t_in_a)
#endif
#include "ntt_direct.hip"
