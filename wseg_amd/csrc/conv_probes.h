// conv_probes.h — development probes of the conv forward / data-gradient kernels (conv_igemm.hip includes it behind common.h; one translation unit, like the kernels).
// The product build (no WSEG_PROBES) gets empty macros only.  Probe builds: `WSEG_PROBES=1 bash build.sh` (stamps + timing switches) and `WSEG_PROBES=2`
// (adds WSEG_SLOTS); scripts/conv_tile_breakdown.py reads them through wseg_debug_stamps / wseg_debug_set_diag.
#pragma once
#ifdef WSEG_PROBES
// In-kernel stamps of the 256-tile body (probe builds only: `WSEG_PROBES=1 bash build.sh`): per workgroup 8 x s_memrealtime (100 MHz) — entry, gather
// set-up done, first tiles landed, main loop done (early wave group), tile done; slots 5 / 6: main loop / tile done of the late group (wave 4);
// slot 7: XCC id.  Written to a buffer of their own that no kernel reads (scripts/conv_tile_breakdown.py fetches it).
__device__ unsigned long long g_wseg_stamps[24 * 4096];   // per workgroup: 8 wall-clock stamps, then (WSEG_SLOTS builds) 8 slot sums of wave 0 and 8 of wave 4
#define WSEG_STAMP(slot, wave)                                                                                  \
  do { if (threadIdx.x == (wave) * 64 && bid < 4096) g_wseg_stamps[bid * 24 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int wseg_debug_stamps(void* out, size_t bytes) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wseg_stamps), bytes < sizeof(g_wseg_stamps) ? bytes : sizeof(g_wseg_stamps)) == hipSuccess ? 0 : -1;
}
#define WSEG_CSTAMP(slot, wave)   /* shader-clock stamp (s_memtime): with the wall-clock stamps beside it, the clock the loop ran at */ \
  do { if (threadIdx.x == (wave) * 64 && bid < 4096) g_wseg_stamps[bid * 24 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
// probe-only timing switches (results wrong by design): bit 0 = request the A tile only on every 9th K-tile, bit 1 = no B requests after the prologue,
// bit 2 = no A requests after the prologue, bit 3 = the A pointers never move (every request re-reads the tile's first K-tile: cache-resident), bit 4 = the same for B, bit 5 = the wave-local epilogue stores nothing (its loads and LDS round trips stay), bit 6 = it loads nothing either
__device__ int g_wseg_diag;
extern "C" int wseg_debug_set_diag(int v) { return hipMemcpyToSymbol(HIP_SYMBOL(g_wseg_diag), &v, sizeof(int)) == hipSuccess ? 0 : -1; }
#define WSEG_DIAG_LOAD() const int diag_ = __builtin_amdgcn_readfirstlane(g_wseg_diag)
#define WSEG_DIAG_A_OK(u) (!(diag_ & 4) && (!(diag_ & 1) || (u) % 9 == 8))
#define WSEG_DIAG_B_OK() (!(diag_ & 2))
#define WSEG_DIAG_A_MOVES() (!(diag_ & 8))
#define WSEG_DIAG_B_MOVES() (!(diag_ & 16))
#define WSEG_DIAG_EPI_STORES() (!(__builtin_amdgcn_readfirstlane(g_wseg_diag) & 32))
#define WSEG_DIAG_EPI_LOADS() (!(__builtin_amdgcn_readfirstlane(g_wseg_diag) & 64))
#else
#define WSEG_STAMP(slot, wave) do { } while (0)
#define WSEG_CSTAMP(slot, wave) do { } while (0)
#define WSEG_DIAG_LOAD() do { } while (0)
#define WSEG_DIAG_A_OK(u) true
#define WSEG_DIAG_B_OK() true
#define WSEG_DIAG_A_MOVES() true
#define WSEG_DIAG_B_MOVES() true
#define WSEG_DIAG_EPI_STORES() true
#define WSEG_DIAG_EPI_LOADS() true
#endif
// WSEG_SLOTS (with WSEG_PROBES): cycles (s_memtime) a wave spends in each slot of the main loop, summed over the K-tiles: read slot 1 (fragment reads
// until they have landed + LDS-DMA issue), barrier, MFMA slot 1, barrier, read slot 2 (+ the counted DMA wait), barrier, MFMA slot 2, barrier.
// The stamps serialise what the real kernel overlaps (each waits for lgkmcnt(0)): read the SHARES, not the run time of this build.
#if defined(WSEG_PROBES) && defined(WSEG_SLOTS)
#define WSEG_SLOT_DECL() unsigned long long sl_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp_ = 0
#define WSEG_SLOT_BEGIN() asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tp_) :: "memory")
#define WSEG_SLOT(i)                                                                                            \
  do {                                                                                                          \
    unsigned long long t_;                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                          \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory");                               \
    __builtin_amdgcn_sched_barrier(0);                                                                          \
    sl_[i] += t_ - tp_; tp_ = t_;                                                                               \
  } while (0)
#define WSEG_SLOT_FLUSH()                                                                                       \
  do {                                                                                                          \
    if ((threadIdx.x == 0 || threadIdx.x == 256) && bid < 4096) {                                               \
      _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) g_wseg_stamps[bid * 24 + 8 + (threadIdx.x >> 8) * 8 + i_] = sl_[i_]; \
    }                                                                                                           \
  } while (0)
#else
#define WSEG_SLOT_DECL() do { } while (0)
#define WSEG_SLOT_BEGIN() do { } while (0)
#define WSEG_SLOT(i) do { } while (0)
#define WSEG_SLOT_FLUSH() do { } while (0)
#endif
