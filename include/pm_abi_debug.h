/*
 * Diagnostic entry points of libpm.so (pm_diag.hip): measurements and invariant checks used by bench.py, the
 * tools/ scripts and the tests.  They are exported from the same library as the C-ABI of pm_abi.h but are no
 * part of the interface an integrator binds against; their signatures may change with the kernels they measure.
 */
#ifndef PM_ABI_DEBUG_H_
#define PM_ABI_DEBUG_H_

#include "pm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics: average time of `reps` launches of superstep-0 kernel variant
 * (0 = product kernel; others are ablation builds used by tools/ubench.py). */
int pm_debug_time_lcc_first(pm_ctx* ctx, int variant, int reps, float* ms_out);
/* Diagnostics: a one-rank RCCL collective of `bytes` (op 0 ncclAllGather, 1 ncclAllReduce u64 sum),
   result checked: 0 = right, 1 = wrong, -1 = error (pm_last_error). */
int pm_debug_rccl_selftest(int device, uint64_t bytes, int op);
/* Diagnostics: HBM copy bandwidth of a 16-B nontemporal copy kernel over two `bytes` buffers (read + write
   bytes per second / 1e9), the measured ceiling beside the datasheet peak. */
int pm_debug_copy_gbs(int device, uint64_t bytes, int reps, double* gbs);
/* Diagnostics: the floor of the first later superstep's neighbour-T_pub gathers: superstep 0
   runs, its light survivors' alive M entries are collected as code indices in record order, and gather-only
   kernels are timed over them (variant 0 record order, 1 index stream only, 2 XCD-sliced buckets, 3 the buckets
   spread over every XCD, 4 uniformly random, 5 sorted, 6 distinct-line misses of a 4 GiB buffer (FETCH_SIZE calibration),
   7 the bucketing pass).  info[0] entries, [1] checksum of the gathered codes, [2] code array bytes. */
int pm_debug_gather_floor(pm_ctx* ctx, int variant, int reps, float* ms_out, uint64_t* info);
/* Diagnostics: superstep-0 tiling statistics, the first n of: [0] real entries, [1] loaded slots, [2] rows,
   [3] tiles, [4] ranges, [5] heavy rows, [6] microseconds of the last layout + tiling build; then which
   specialisations the tiling selects, over its ranges with rows: [7] max nrel (relevant label runs),
   [8] max nadm (merged runs), [9] max nkeep (template vertices of one label), [10] k1_wide (some nrel > 4:
   k_lcc_first<0, true> runs), [11] mask of the phase-A cases the light ranges take (bit 0 nadm <= 1, 1 nadm == 2,
   2 nadm 3..4, 3 the full label test: nadm > 4, and every range when k1_wide); [12] pull supersteps of the last
   search's first LCC call that listed long rows for k_lcc_step_pieces (0 before the first search). */
int pm_debug_layout_stats(pm_ctx* ctx, uint64_t* out, uint64_t n);

/* Diagnostics: T_pub census (both ping-pong buffers) -- out[0], out[1]: nonzero entries of buffer 0 / 1,
   out[2]: positions with a nonzero entry in either buffer that are not in the current slist (the invariant
   the search-start clear relies on: 0).  deferred_reset != 0 first runs the search start's reset as a search
   does (deferred, then flushed in one launch), so out[0..2] must all be 0 afterwards. */
int pm_debug_tpub_census(pm_ctx* ctx, int deferred_reset, uint64_t* out);

#ifdef __cplusplus
}
#endif

#endif /* PM_ABI_DEBUG_H_ */
