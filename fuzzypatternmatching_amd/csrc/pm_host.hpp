// Host-side declarations shared by the context set-up (pm_context.hip), the search driver (pm_driver.hip),
// the diagnostics (pm_diag.hip) and the C-ABI entry points (pm_api.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <exception>
#include <string>
#include <vector>

#include "../../include/pm_abi.h"
#include "pm_internal.hpp"

struct pm_ctx : public pm::Ctx {};

namespace pm {

// per thread: the shards of one process (pm_run_beta_local_shards, the CLI's one-thread-per-GPU mode) fail
// independently
extern thread_local std::string g_last_error;

// The C-ABI's error convention.  A call without a context: a thrown message goes to pm_last_error(NULL) and the
// call returns `fail` (-1 or nullptr).
template <typename R, typename F>
R api_call(R fail, F&& body) {
  try {
    return body();
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return fail;
  }
}

// A call on a context: its device is made current, and a thrown message is kept on the context as well.
template <typename F>
int ctx_call(pm_ctx* ctx, F&& body) {
  if (!ctx) return -1;
  try {
    (void)hipSetDevice(ctx->device);
    body();
    return 0;
  } catch (const std::exception& e) {
    ctx->err = e.what();
    g_last_error = e.what();
    return -1;
  }
}

template <typename T>
T* dalloc(uint64_t n) {
  T* p = nullptr;
  PM_HIP_CHECK(hipMalloc(&p, std::max<uint64_t>(1, n) * sizeof(T)));
  return p;
}

// --- pm_context.hip: one-time set-up -----------------------------------------------------------------------------

// Graph of one context: the whole graph (nshards == 1) or one shard's rows.
struct CtxInput {
  uint64_t n = 0;
  const uint64_t* off = nullptr;   // n + 1 offsets of the rows this context scans
  const uint32_t* col = nullptr;
  const uint32_t* gdeg = nullptr;  // global degrees (null: from off)
  bool symmetric = true;
  uint32_t nranks = 1;
  uint64_t hub_threshold = 1048576;
  uint32_t nshards = 1, shard = 0;
  Comm* comm = nullptr;            // ownership passes to the context
  bool col_on_device = false;      // col is device memory (GPU-built graph); off stays host
  bool col_release = false;        // ... and the context frees it once copied (the caller must not)
  uint32_t inprocess_shards = 1;   // shards of this process on the same device (ThreadComm groups)
  const uint64_t* in_off = nullptr;  // directed graphs: in-rows built by the caller (host offsets,
  const uint32_t* in_col = nullptr;  // columns where col lives), e.g. by the GPU ingest
};

void require_gfx950(int device);
void set_degree_labels(Ctx& c);
pm_ctx* create_ctx(const CtxInput& in, const char* pattern_dir, int device);
pm_ctx* create_ctx(const pm_graph_desc* g, const char* pattern_dir, int device);
void destroy_ctx(pm_ctx* c);
// pm_push_shard.hip: the in-rows of the vertices this shard of a directed graph owns, from every shard's
// out-rows (collective; see there).  Fills in_off (n + 1, host), *d_in_col (device, the caller frees it) and
// c.rdeg_host (every vertex's in-degree); a failure on any shard leaves a message in err on every shard.
void build_shard_in_rows(Ctx& c, const CtxInput& in, std::string& err, std::vector<uint64_t>& in_off,
                         uint32_t** d_in_col);
void relayout(Ctx& c);

// --- pm_driver.hip: what a search executes -----------------------------------------------------------------------

// defer: the fills stay queued for the search's first launch (flush_zero batches them into one)
void reset_state(Ctx& c, bool defer = false);

// Per-superstep outputs of one LCC call.
struct LccOut {
  std::vector<std::vector<uint64_t>> vcount, ecount;  // [superstep][rank]
  std::vector<uint64_t> trav;
  std::vector<double> seconds;
  bool not_finished = false;
  uint64_t matching_rows = 0;  // vertices with a label match (superstep 0 of the first call)
  // this shard's counts: per rank after the last superstep; superstep-0 survivors and M entries
  std::vector<uint64_t> loc_vc, loc_ec;
  uint64_t loc_surv = 0, loc_edges = 0;
};

void ensure_counts(Ctx& c, size_t slots);
LccOut lcc_call(Ctx& c, bool init_step);
uint32_t owner_host(const Ctx& c, uint64_t v);
void export_state_all(Ctx& c, std::vector<uint16_t>& tpub, std::vector<uint32_t>& mdeg, std::vector<uint32_t>& nbrs);
void run_beta(Ctx& c, const std::string& out_dir, uint64_t max_iterations, pm_run_stats* st);

// --- pm_diag.hip -------------------------------------------------------------------------------------------------

void gather_floor_forget(const void* owner);  // the gather-floor cache of a destroyed context
void install_segv_trace();                    // PM_SEGV_TRACE=1: backtrace of a host crash in the shard threads

}  // namespace pm
