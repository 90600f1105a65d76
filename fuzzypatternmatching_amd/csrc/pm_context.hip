// One-time set-up of a context: device check, graph upload, label-major layout and tiling (create_ctx),
// its release (destroy_ctx) and the layout of new labels (relayout).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "host/graph_store.hpp"
#include "pm_device.hpp"
#include "pm_host.hpp"

namespace pm {

void require_gfx950(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= device)
    throw std::runtime_error("no HIP device " + std::to_string(device) + " available (the HIP path has no CPU fallback)");
  hipDeviceProp_t prop;
  PM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    throw std::runtime_error(std::string("device arch ") + prop.gcnArchName + " is not gfx950 (MI355X)");
  // the driver loop waits on a few small read-backs per search: spin instead of
  // yielding, so the next launch follows the device at once (PM_SPIN=0: runtime
  // default; refused once the device's context is active, which then keeps its flags)
  static const bool spin = !std::getenv("PM_SPIN") || std::string(std::getenv("PM_SPIN")) != "0";
  if (spin && hipSetDevice(device) == hipSuccess && hipSetDeviceFlags(hipDeviceScheduleSpin) != hipSuccess)
    (void)hipGetLastError();
}

// In-rows of a directed CSR (rows sorted by source id, duplicates adjacent):
// superstep 0 pulls along in-edges, i.e. exactly the messages the reference
// pushes along out-edges (nonunique_ee.hpp:555-560, SURVEY A.6 hazard 10).
static void transpose_csr(uint64_t n, const uint64_t* off, const uint32_t* col, std::vector<uint64_t>& toff,
                          std::vector<uint32_t>& tcol) {
  toff.assign(n + 1, 0);
  for (uint64_t e = 0; e < off[n]; ++e) {
    if (col[e] >= n) throw std::runtime_error("edge target out of range");
    ++toff[col[e] + 1];
  }
  for (uint64_t v = 0; v < n; ++v) toff[v + 1] += toff[v];
  tcol.resize(off[n]);
  std::vector<uint64_t> at(toff.begin(), toff.end() - 1);
  for (uint64_t v = 0; v < n; ++v)
    for (uint64_t e = off[v]; e < off[v + 1]; ++e) tcol[at[col[e]]++] = static_cast<uint32_t>(v);
}

// Degree labels (vertex_data_db_degree.hpp:109) from the global out-degrees (host: the layout uploads them).
void set_degree_labels(Ctx& c) {
  c.labels_host.assign(c.n, 0);
  for (uint64_t v = 0; v < c.n; ++v) c.labels_host[v] = degree_label(c.deg_host[v]);
}

// Host pages registered with the runtime for the lifetime of the object (large
// uploads only; a range the runtime refuses, e.g. memory that is already
// pinned, is copied as pageable memory).
struct PinnedRange {
  void* base = nullptr;
  PinnedRange(const void* p, size_t bytes) {
    if (!p || bytes < (size_t(16) << 20)) return;
    const size_t page = 4096;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p) & ~(page - 1);
    const size_t len = ((reinterpret_cast<uintptr_t>(p) + bytes + page - 1) & ~(page - 1)) - a;
    if (hipHostRegister(reinterpret_cast<void*>(a), len, hipHostRegisterDefault) == hipSuccess)
      base = reinterpret_cast<void*>(a);
    else
      (void)hipGetLastError();
  }
  ~PinnedRange() {
    if (base) (void)hipHostUnregister(base);
  }
  PinnedRange(const PinnedRange&) = delete;
  PinnedRange& operator=(const PinnedRange&) = delete;
};

pm_ctx* create_ctx(const CtxInput& in, const char* pattern_dir, int device) {
  std::unique_ptr<Comm> comm(in.comm);
  // a device-resident input the caller handed over (col_release) is freed as soon as it is copied
  struct ColRelease {
    const uint32_t* p;
    void now() {
      if (p) (void)hipFree(const_cast<uint32_t*>(p));
      p = nullptr;
    }
    ~ColRelease() { now(); }
  } col_release{in.col_on_device && in.col_release ? in.col : nullptr};
  if (!in.off || !in.col) throw std::runtime_error("pm_create: null graph");
  if (in.nshards == 0 || in.shard >= in.nshards) throw std::runtime_error("pm_create: bad shard index");
  if (in.nshards > 1 && !comm) throw std::runtime_error("pm_create: sharded context without a communicator");
  require_gfx950(device);
  // a construction that throws releases what it allocated (device buffers, stream, communicator)
  std::unique_ptr<pm_ctx, void (*)(pm_ctx*)> c(new pm_ctx(), destroy_ctx);
  c->device = device;
  PM_HIP_CHECK(hipSetDevice(device));
  PM_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->n = in.n;
  c->nnz = in.off[in.n];
  c->symmetric = in.symmetric;
  c->nranks = in.nranks ? in.nranks : 1;
  c->hub_threshold = in.hub_threshold;
  c->nshards = in.nshards;
  c->shard = in.shard;
  c->comm = comm.get();
  c->comm_owned = comm.release();
  if (c->n >= (1ull << 30)) throw std::runtime_error("more than 2^30 vertices (30-bit positions in M entries)");
  // the rows superstep 0 scans: the CSR itself, or its in-rows for a directed graph
  std::vector<uint64_t> tin_off;
  std::vector<uint32_t> tin_col;
  const uint64_t* soff = in.off;
  const uint32_t* scol = in.col;
  bool scol_on_device = in.col_on_device;
  uint64_t snnz = c->nnz;
  size_t arena = 0;
  bool any_sv = false;
  std::string build_err;
  // a shard of a directed graph holds out-rows: the in-rows of the vertices it owns come from every shard's
  // (collective; a shard that fails in it reports through build_err and still takes part in the agreement below)
  struct InCol {
    uint32_t* p = nullptr;
    void now() {
      if (p) (void)hipFree(p);
      p = nullptr;
    }
    ~InCol() { now(); }
  } in_col;
  if (!c->symmetric && in.nshards > 1) build_shard_in_rows(*c, in, build_err, tin_off, &in_col.p);
  try {
    if (!build_err.empty()) throw std::runtime_error(build_err);
    if (!c->symmetric && in.nshards > 1) {
      soff = tin_off.data();
      scol = in_col.p;
      scol_on_device = true;
      snnz = tin_off[c->n];
    } else if (!c->symmetric) {
      if (in.in_off && in.in_col) {
        soff = in.in_off;
        scol = in.in_col;
      } else {
        if (in.col_on_device) throw std::runtime_error("directed device-resident graphs need their in-rows");
        transpose_csr(c->n, in.off, in.col, tin_off, tin_col);
        soff = tin_off.data();
        scol = tin_col.data();
      }
      c->rdeg_host.resize(c->n);
      for (uint64_t v = 0; v < c->n; ++v) c->rdeg_host[v] = static_cast<uint32_t>(soff[v + 1] - soff[v]);
    }
    c->pattern = load_pattern_dir(pattern_dir);
    const PatternGraph& pg = c->pattern.graph;
    if (pg.diameter == 0) throw std::runtime_error("pattern_stat: diameter is 0 or missing");
    for (int t = 0; t < kMaxTemplateVertices; ++t) c->pa.adj[t] = pg.adj[t];
    c->pa.K = static_cast<int32_t>(pg.vertex_data.size());
    for (int t = 0; t < c->pa.K; ++t) c->pa.plabel[t] = pg.vertex_data[t];
    // a label of more than two template vertices: its 2-bit code cannot carry T_pub (tpub_code)
    for (int t = 0; t < c->pa.K; ++t) {
      int k = 0;
      for (int u = 0; u < c->pa.K; ++u) k += c->pa.plabel[u] == c->pa.plabel[t];
      if (k > 2) c->xcode_wide = true;
    }
    any_sv = false;
    for (size_t pl = 0; pl < c->pattern.lines.size(); ++pl) {
      const auto& l = c->pattern.lines[pl];
      if (!l.selected_vertices) continue;
      any_sv = true;
      if (pl >= 4 || l.valid_cycle)  // the reference applies it in nem_1 path checks only
        throw std::runtime_error("pattern_nlc selected_vertices=1 is supported on path lines (index < 4, valid_cycle 0)");
    }
    // global degrees (labels, hubs, layout order) and the lengths of the rows held here
    c->deg_host.resize(c->n);
    if (in.gdeg) c->ldeg_host.reserve(c->n);
    for (uint64_t v = 0; v < c->n; ++v) {
      const uint64_t d = in.gdeg ? in.gdeg[v] : in.off[v + 1] - in.off[v];
      if (d > 0xFFFFFFFFull) throw std::runtime_error("degree above 2^32");
      const uint64_t ld = in.off[v + 1] - in.off[v];
      // a shard holds the whole rows it owns, and of a delegate (degree >= -d) the entries whose target it owns
      if (in.gdeg && ld && (d >= c->hub_threshold && c->nshards > 1 ? ld > d
                                                                     : (ld != d || v % c->nshards != c->shard)))
        throw std::runtime_error("shard rows must be the owned rows (v % nshards == shard) with their full degree, "
                                 "and delegate rows (degree >= hub threshold) split by target owner");
      c->deg_host[v] = static_cast<uint32_t>(d);
      if (d >= c->hub_threshold) c->hubs_host.push_back(v);
      if (in.gdeg) c->ldeg_host.push_back(static_cast<uint32_t>(ld));
      c->held_rows += ld != 0;
      if (ld && d >= c->hub_threshold && c->nshards > 1) c->held_hub_entries += ld;
    }
    // (a directed graph's in-rows are whole on their owners, delegates' too: nothing to combine)
    c->split_hubs = c->nshards > 1 && c->symmetric && !c->hubs_host.empty();
    // a shard context of a directed graph (one shard with a communicator included): the rows held here, which
    // the layout copies and pads, are the in-rows -- not the out-rows the shard was given
    if (!c->symmetric && (c->nshards > 1 || !c->ldeg_host.empty())) {
      c->ldeg_host.resize(c->n);
      for (uint64_t v = 0; v < c->n; ++v) c->ldeg_host[v] = static_cast<uint32_t>(soff[v + 1] - soff[v]);
    }
    for (uint64_t j = c->shard; c->split_hubs && j < c->hubs_host.size(); j += c->nshards)
      c->hub_area += c->deg_host[c->hubs_host[j]];
    // device graph + state; padded slot count of the rows scanned here (label independent)
    c->nq = 0;
    for (uint64_t v = 0; v < c->n; ++v) c->nq += padded_degree(soff[v + 1] - soff[v]);
    c->mcap = c->nq;
    c->d_offp = dalloc<uint64_t>(c->n + 1);
    c->d_offr = dalloc<uint64_t>(c->n + 1);
    // slot buffers carry kTileEntries entries of tail padding (superstep-0 tile loads read whole tiles)
    // dense superstep-0 M region behind the tail padding (both buffers: relayout swaps them)
    if (c->symmetric && c->nq)
      c->dcap = std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>(uint64_t(1) << 16, c->nq / 8));
    c->dbase = c->nq + kTileEntries;
    c->d_colp = dalloc<uint32_t>(c->nq + kTileEntries + c->dcap + c->hub_area);
    c->d_perm = dalloc<uint32_t>(c->n);
    c->d_pos = dalloc<uint32_t>(c->n);
    if (!c->hubs_host.empty()) {
      c->d_hubs = dalloc<uint64_t>(c->hubs_host.size());
      PM_HIP_CHECK(hipMemcpy(c->d_hubs, c->hubs_host.data(), c->hubs_host.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    c->d_tpub[0] = dalloc<uint16_t>(c->n);
    c->d_tpub[1] = dalloc<uint16_t>(c->n);
    c->d_tst = dalloc<uint16_t>(c->n);
    c->d_mcol = dalloc<uint32_t>(c->nq + kTileEntries + c->dcap + c->hub_area);
    c->d_mlen = dalloc<uint32_t>(c->n);
    c->d_malive = dalloc<uint32_t>(c->n);
    c->d_slist = dalloc<uint32_t>(c->n);
    c->d_smask[0] = dalloc<uint64_t>((c->n + 63) / 64 + 1);
    c->d_smask[1] = dalloc<uint64_t>((c->n + 63) / 64 + 1);
    c->d_sources = dalloc<uint32_t>(c->n);
    c->d_nS = dalloc<uint32_t>(2);  // [1]: long-row stamp (launch_compact_rows)
    PM_HIP_CHECK(hipMemset(c->d_nS, 0, 2 * sizeof(uint32_t)));
    c->d_flags = dalloc<uint32_t>(4);
    c->d_tsm = dalloc<uint8_t>(c->n);
    c->d_tcode = dalloc<uint32_t>((c->n + 15) / 16 + 1);
    if (c->nranks > 64) throw std::runtime_error("more than 64 ranks for result-file attribution");
    c->d_part = dalloc<uint64_t>(uint64_t(kPartGridMax) * slot_words(*c));
    size_t free_b = 0, total_b = 0;
    PM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    arena = std::min<size_t>(free_b / 2, size_t(32) << 30);
    if (in.inprocess_shards > 1)  // in-process shard groups share one device
      arena = std::min<size_t>(arena, std::max<size_t>(size_t(1) << 30, free_b / (2 * in.inprocess_shards)));
    arena = std::max<size_t>(arena, size_t(64) << 20);
    // PM_ARENA_MB=<MiB> (tests): a smaller arena (the exact path lines' source batches)
    if (const char* e = std::getenv("PM_ARENA_MB"))
      arena = std::min<size_t>(arena, std::max<size_t>(1, std::strtoull(e, nullptr, 10)) << 20);
  } catch (const std::exception& e) {
    build_err = e.what();
    arena = 0;
  }
  // one size on every shard: the replicated lines' walk storage and TDS chunk caps come from it, and a line
  // that overflowed on some shards only would send those into collectives the others never make
  // -- and construction is collective: a shard that failed above still takes part (arena 0), so the others
  // are not left in a collective it never makes, and every shard then fails
  arena = static_cast<size_t>(shard_agree_min(*c, arena));
  if (!build_err.empty()) throw std::runtime_error(build_err);
  if (arena == 0) throw std::runtime_error("another shard failed while building its context");
  c->arena.base = dalloc<char>(arena);
  c->arena.cap = arena;
  if (const char* e = std::getenv("PM_FUSED_LINES")) c->fused_lines = std::string(e) != "0";
  if (const char* e = std::getenv("PM_ROW_COMPACTION")) c->no_row_compaction = std::string(e) == "0";
  if (const char* e = std::getenv("PM_PULL_PIECES")) c->long_seen_off = std::string(e) == "0";
  if (const char* e = std::getenv("PM_PULL_LONG")) c->pull_long = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
  if (const char* e = std::getenv("PM_DIAG_STEP")) c->diag_step = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
  if (any_sv) c->fused_lines = false;  // token-source sets across lines: the per-position path keeps them
  c->any_sv = any_sv;
  // Grid-barrier kernels (k_lines, the list compaction's scan) need every block resident.  A cooperative launch
  // guarantees it but costs ~28 us per launch (85 us per S=28 step for three launches, tools/gpu_coop_ab.sh); with one
  // context on the device the grids are sized to fit and nothing else that waits on them runs beside them, so an
  // ordinary launch is used.  Shards sharing a device (in-process shards, host-collective ranks) could hold each
  // other's blocks out with their spinning grids: cooperative.  PM_COOP=1 / PM_LINES_NOCOOP=1 force either.
  c->coop = in.inprocess_shards > 1 || (c->comm && c->comm->transport() != PM_TRANSPORT_RCCL);
  // (host collectives: the ranks may share the device -- several processes on one GPU; RCCL never puts two ranks
  // on one device.  A caller running two unrelated contexts concurrently on one GPU sets PM_COOP=1.)
  if (const char* e = std::getenv("PM_COOP")) c->coop = std::string(e) == "1";
  if (const char* e = std::getenv("PM_LINES_NOCOOP")) if (std::string(e) == "1") c->coop = false;
  if (const char* e = std::getenv("PM_SPLIT_LINES")) c->split_min = std::strtoull(e, nullptr, 10);
  if (const char* e = std::getenv("PM_HASH_SLOTS")) c->hash_slots = std::strtoull(e, nullptr, 10);
  if (const char* e = std::getenv("PM_HANDOFF")) c->handoff_ss = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
  if (const char* e = std::getenv("PM_DEBUG_NOGROW_SHARD")) c->nogrow_shard = std::strtoll(e, nullptr, 10);
  if (const char* e = std::getenv("PM_DEBUG_OVERFLOW_SHARD")) c->overflow_shard = std::strtoll(e, nullptr, 10);
  // diagnostics: PM_FORCE_PULL=1 keeps the pull form in every LCC call (an
  // asymmetric M then aborts the search: tests use it to find such inputs)
  if (const char* e = std::getenv("PM_FORCE_PULL")) c->force_pull = std::string(e) == "1" && c->symmetric;
  // default labels = degree labels; the id-major adjacency is staged in the
  // M column buffer and permuted into the label-major d_colp
  if (snnz) {
    if (scol_on_device) {
      PM_HIP_CHECK(hipMemcpy(c->d_mcol, scol, snnz * sizeof(uint32_t), hipMemcpyDeviceToDevice));
      col_release.now();
      in_col.now();
    } else {
      // pinned staging: the caller's pages are registered for the copy, so the
      // adjacency moves by DMA without a bounce through driver staging buffers
      PinnedRange pin(scol, snnz * sizeof(uint32_t));
      PM_HIP_CHECK(hipMemcpy(c->d_mcol, scol, snnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
  }
  set_degree_labels(*c);
  const auto t_lay = std::chrono::steady_clock::now();
  build_label_layout(*c, c->d_mcol, false, c->d_colp);
  build_tiling(*c);
  PM_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->layout_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_lay).count();
  return c.release();
}

pm_ctx* create_ctx(const pm_graph_desc* g, const char* pattern_dir, int device) {
  if (!g || !g->off || !g->col) throw std::runtime_error("pm_create: null graph");
  CtxInput in;
  in.n = g->n;
  in.off = g->off;
  in.col = g->col;
  in.symmetric = g->symmetric != 0;
  in.nranks = g->nranks;
  in.hub_threshold = g->hub_threshold;
  return create_ctx(in, pattern_dir, device);
}

void destroy_ctx(pm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  void* ptrs[] = {c->d_offp, c->d_offr, c->d_colp, c->d_perm, c->d_pos, c->d_labs, c->d_hubs,
                  c->d_ktab, c->d_ttab, c->d_hseg, c->d_hscr, c->d_tpub[0], c->d_tpub[1], c->d_tst, c->d_mcol,
                  c->d_mlen, c->d_malive, c->d_slist, c->d_slist2, c->d_nS2, c->d_ccnt, c->d_cbase, c->d_ctmp, c->d_smask[0], c->d_smask[1], c->d_kmask, c->d_sources, c->d_nS, c->d_flags, c->d_tsm,
                  c->d_counts, c->d_part, c->d_tmask, c->d_tbase, c->d_scan_tmp, c->arena.base, c->d_tn, c->d_pseen,
                  c->d_tcode, c->d_rarea, c->d_rbase, c->d_rcnt, c->d_rofs, c->d_hrec, c->d_srec, c->d_rscan_tmp, c->d_cdesc,
                  c->d_xsend, c->d_xrecv, c->d_xent_send,
                  c->d_xent_recv, c->d_xcnt, c->d_rmoff, c->d_rmcol, c->d_xred, c->d_hubinfo, c->d_moff, c->d_hubpart, c->d_xsplit, c->d_push,
                  c->d_lrows, c->d_lscr, c->d_clstat, c->d_lsrc, c->d_ldels, c->d_pushx,
                  };
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete c->comm_owned;
  if (c->h_pin) (void)hipHostFree(c->h_pin);
  if (c->h_pin_lines) (void)hipHostFree(c->h_pin_lines);
  free_line_buffers(*c);
  for (auto e : c->events) (void)hipEventDestroy(e);
  if (c->ev_handoff) (void)hipEventDestroy(c->ev_handoff);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->rstream) (void)hipStreamDestroy(c->rstream);
  if (c->ev_rb) (void)hipEventDestroy(c->ev_rb);
  if (c->ev_tz0) (void)hipEventDestroy(c->ev_tz0);
  if (c->ev_tz) (void)hipEventDestroy(c->ev_tz);
  delete c;
}

// New labels: rebuild the label-major layout from the current one (the M
// column buffer is free between searches and receives the new adjacency).
void relayout(Ctx& c) {
  const auto t_lay = std::chrono::steady_clock::now();
  build_label_layout(c, c.d_colp, true, c.d_mcol);
  std::swap(c.d_colp, c.d_mcol);
  c.mcap = c.nq;  // d_mcol is the former d_colp (nq entries, no remote region)
  build_tiling(c);
  PM_HIP_CHECK(hipStreamSynchronize(c.stream));
  c.layout_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_lay).count();
  c.lcc_started = false;
  c.tpub_clean = false;  // positions changed: the next reset clears T_pub entirely
  c.long_seen.clear();   // (new labels: where long rows survive is not known)
  c.tcode_zeroed = false;  // (new labels: more code words than the last clear covered)
  // the line grid of a search's prelaunched lines is sized by the previous search's |S| (identical for repeated
  // searches of one layout); new labels: the full grid until a search has run
  c.live_hint = ~0ull;
}

}  // namespace pm
