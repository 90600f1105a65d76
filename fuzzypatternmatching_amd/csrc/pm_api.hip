// C-ABI (include/pm_abi.h) of the MI355X pattern-matching path: the extern "C" entry points over the context
// set-up (pm_context.hip) and the search driver (pm_driver.hip), the in-process shard driver and the input
// builders (R-MAT, text ingest, graph files, text writers).  The pm_debug_* entry points are in pm_diag.hip.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "host/graph_store.hpp"
#include "host/mt_jump.hpp"
#include "pm_host.hpp"
#include "pm_ingest.hpp"
#include "pm_rmat.hpp"
#include "pm_shard.hpp"

namespace pm {
thread_local std::string g_last_error;
}

namespace {

using pm::api_call;
using pm::ctx_call;

// Device resources of an entry point that builds its input on the device, released on every exit.
struct Stream {
  hipStream_t s = nullptr;
  Stream() { PM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ~Stream() { (void)hipStreamDestroy(s); }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  explicit DevBuf(uint64_t n) : p(pm::dalloc<T>(n)) {}
  ~DevBuf() { (void)hipFree(p); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

void free_dev_csr(pm::DevCsr& g) {
  if (g.d_off) (void)hipFree(g.d_off);
  if (g.d_col) (void)hipFree(g.d_col);
  g.d_off = nullptr;
  g.d_col = nullptr;
}

struct CsrGuard {  // frees what the CSR still holds (an array handed on is set to null first)
  pm::DevCsr& g;
  ~CsrGuard() { free_dev_csr(g); }
};

// malloc'ed output arrays (pm_free_host), released unless handed to the caller
template <typename T>
std::unique_ptr<T, void (*)(void*)> host_alloc(uint64_t n, const char* who) {
  std::unique_ptr<T, void (*)(void*)> p(static_cast<T*>(std::malloc(std::max<uint64_t>(1, n) * sizeof(T))), std::free);
  if (!p) throw std::runtime_error(std::string(who) + ": out of host memory");
  return p;
}

std::vector<std::string> file_list(const char* const* files, uint32_t nfiles) {
  if (nfiles && !files) throw std::runtime_error("null file list");
  std::vector<std::string> v;
  for (uint32_t i = 0; i < nfiles; ++i) {
    if (!files[i]) throw std::runtime_error("null file name");
    v.emplace_back(files[i]);
  }
  return v;
}

// -v files basename(prefix).* parsed on the current device (stream s), kept on the host: the layout's input
std::vector<uint64_t> labels_from_files(const char* prefix, uint64_t n, hipStream_t s) {
  const std::vector<std::string> files = pm::vertex_label_files(prefix);
  DevBuf<uint64_t> d_labels(n);
  pm::labels_from_files_device(files, n, d_labels.p, s);
  std::vector<uint64_t> labels(n);
  if (n) PM_HIP_CHECK(hipMemcpyAsync(labels.data(), d_labels.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PM_HIP_CHECK(hipStreamSynchronize(s));
  return labels;
}

// The graph of a shard context as the caller describes it (the communicator is the caller's to add).
pm::CtxInput shard_input(const pm_shard_desc& d, const char* who) {
  pm::CtxInput in;
  in.n = d.n;
  in.off = d.off;
  in.col = d.col;
  in.gdeg = d.degree;
  if (!in.gdeg) throw std::runtime_error(std::string(who) + ": null degree array");
  in.symmetric = d.symmetric != 0;
  in.nranks = d.nranks;
  in.hub_threshold = d.hub_threshold;
  in.nshards = d.nshards;
  in.shard = d.shard;
  return in;
}

// One shard of the R-MAT graph built on the device (pm_rmat.hip rmat_shard_device) and its context;
// the communicator passes to the context.
pm_ctx* create_rmat_shard_ctx(uint64_t scale, uint64_t p_gen, const char* pattern_dir, int device, uint32_t nranks,
                              uint64_t hub_threshold, uint32_t nshards, uint32_t shard, pm::Comm* comm,
                              uint32_t inprocess, double* gen_seconds) {
  std::unique_ptr<pm::Comm> owned(comm);
  pm::require_gfx950(device);
  PM_HIP_CHECK(hipSetDevice(device));
  Stream s;
  pm::DevCsr g;
  CsrGuard hold{g};
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> gdeg;
  g = pm::rmat_shard_device(scale, p_gen, hub_threshold, *comm, nshards, shard, gdeg, s.s);
  if (gen_seconds) *gen_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::vector<uint64_t> off(g.n + 1);
  PM_HIP_CHECK(hipMemcpy(off.data(), g.d_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  (void)hipFree(g.d_off);
  g.d_off = nullptr;
  pm::CtxInput in;
  in.n = g.n;
  in.off = off.data();
  in.col = g.d_col;
  in.col_on_device = true;
  in.col_release = true;  // freed by the context once copied (in-process shards: before the next shard builds)
  g.d_col = nullptr;
  in.gdeg = gdeg.data();
  in.symmetric = true;
  in.nranks = nranks;
  in.hub_threshold = hub_threshold;
  in.nshards = nshards;
  in.shard = shard;
  in.comm = owned.release();
  in.inprocess_shards = inprocess;
  return pm::create_ctx(in, pattern_dir, device);
}

// Every failed shard's message (a device fault is seen by whichever shard calls the runtime next; the shard
// whose work faulted names it in its own message).
void throw_shard_errors(const std::vector<std::string>& errs) {
  std::string msg;
  for (size_t q = 0; q < errs.size(); ++q)
    if (!errs[q].empty() && errs[q] != "another shard failed")
      msg += (msg.empty() ? "" : " | ") + ("shard " + std::to_string(q) + ": " + errs[q]);
  if (msg.empty())
    for (size_t q = 0; q < errs.size() && msg.empty(); ++q)
      if (!errs[q].empty()) msg = "shard " + std::to_string(q) + ": " + errs[q];
  if (!msg.empty()) throw std::runtime_error(msg);
}

// nshards shards of one search, each driven by a thread of this process, all on one device.  make_ctx(q, grp,
// dev) builds shard q's context: it may first work on the host beside the other shards, then takes the device
// lock `dev` before its first runtime call and returns holding it -- the shard keeps the lock from there to the
// release of its context (the collectives let go of it while they wait).  Labels (may be null: degree labels)
// are shared by the shards; the search runs `repeats` times, result files from the first run.
template <typename MakeCtx>
void run_local_shards(uint32_t nshards, const uint64_t* labels, const char* result_dir, uint64_t max_iterations,
                      uint32_t repeats, pm_run_stats* per_shard, const MakeCtx& make_ctx) {
  pm::install_segv_trace();
  pm::ThreadGroup grp(static_cast<int>(nshards));
  std::vector<pm_run_stats> st(nshards);
  std::vector<std::string> errs(nshards);
  const std::string dir = result_dir ? result_dir : "";
  auto work = [&](uint32_t q) {
    pm_ctx* ctx = nullptr;
    try {
      std::unique_lock<std::mutex> dev(grp.device, std::defer_lock);
      ctx = make_ctx(q, grp, dev);
      if (labels) {
        ctx->labels_host.assign(labels, labels + ctx->n);
        pm::relayout(*ctx);
      }
      for (uint32_t r = 0; r < std::max<uint32_t>(repeats, 1); ++r)
        pm::run_beta(*ctx, r == 0 ? dir : std::string(), max_iterations, &st[q]);
      pm::destroy_ctx(ctx);  // (the device lock still held)
      ctx = nullptr;
    } catch (const std::exception& e) {
      errs[q] = e.what();
      grp.abort();
    }
    if (ctx) {
      std::lock_guard<std::mutex> dev(grp.device);
      pm::destroy_ctx(ctx);
    }
  };
  std::vector<std::thread> pool;
  for (uint32_t q = 0; q < nshards; ++q) pool.emplace_back(work, q);
  for (auto& t : pool) t.join();
  throw_shard_errors(errs);
  if (per_shard) std::copy(st.begin(), st.end(), per_shard);
}

// Decimal text of x at p (no terminator); returns the end.
inline char* put_u64(char* p, uint64_t x) {
  char tmp[20];
  int k = 0;
  do {
    tmp[k++] = static_cast<char>('0' + x % 10);
    x /= 10;
  } while (x);
  while (k) *p++ = tmp[--k];
  return p;
}

// Lines "a[i] b[i]\n" (b == nullptr: "i a[i]\n") for i in [0, n), formatted by host threads into
// per-chunk buffers and written in order to f.
uint64_t write_pairs_text(std::FILE* f, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t id0) {
  const unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  constexpr uint64_t kChunk = 1ull << 22;  // lines per chunk (<= 42 bytes each)
  uint64_t total = 0;
  std::vector<std::vector<char>> buf(T, std::vector<char>(kChunk * 42));
  std::vector<uint64_t> len(T);
  for (uint64_t c0 = 0; c0 < n; c0 += kChunk * T) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t)
      th.emplace_back([&, t] {
        const uint64_t b0 = c0 + t * kChunk, e0 = std::min(n, b0 + kChunk);
        char* p = buf[t].data();
        for (uint64_t i = b0; i < e0; ++i) {
          p = put_u64(p, b ? a[i] : id0 + i);
          *p++ = ' ';
          p = put_u64(p, b ? b[i] : a[i]);
          *p++ = '\n';
        }
        len[t] = b0 < e0 ? static_cast<uint64_t>(p - buf[t].data()) : 0;
      });
    for (auto& x : th) x.join();
    for (unsigned t = 0; t < T; ++t) {
      if (len[t] && std::fwrite(buf[t].data(), 1, len[t], f) != len[t]) throw std::runtime_error("text write failed");
      total += len[t];
    }
  }
  return total;
}

// One text file of write_pairs_text lines; returns its bytes.
uint64_t write_pairs_file(const std::string& path, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t id0) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  uint64_t bytes = 0;
  try {
    bytes = write_pairs_text(f, a, b, n, id0);
  } catch (...) {
    std::fclose(f);
    throw;
  }
  if (std::fclose(f) != 0) throw std::runtime_error("cannot close " + path);
  return bytes;
}

}  // namespace

extern "C" {

// --- contexts and searches ---------------------------------------------------------------------------------------

pm_ctx* pm_create(const pm_graph_desc* graph, const char* pattern_dir, int device) {
  return api_call<pm_ctx*>(nullptr, [&] { return pm::create_ctx(graph, pattern_dir, device); });
}

void pm_destroy(pm_ctx* ctx) {
  pm::gather_floor_forget(ctx ? static_cast<const void*>(static_cast<pm::Ctx*>(ctx)) : nullptr);
  pm::destroy_ctx(ctx);
}

const char* pm_last_error(const pm_ctx* ctx) {
  if (ctx && !ctx->err.empty()) return ctx->err.c_str();
  return pm::g_last_error.c_str();
}

int pm_vertex_data_degree(pm_ctx* ctx) {
  return ctx_call(ctx, [&] {
    pm::set_degree_labels(*ctx);
    pm::relayout(*ctx);
  });
}

int pm_vertex_data_set(pm_ctx* ctx, const uint64_t* labels) {
  return ctx_call(ctx, [&] {
    if (!labels) throw std::runtime_error("null labels");
    ctx->labels_host.assign(labels, labels + ctx->n);
    pm::relayout(*ctx);
  });
}

int pm_vertex_data_files(pm_ctx* ctx, const char* prefix) {
  return ctx_call(ctx, [&] {
    if (!prefix) throw std::runtime_error("null label prefix");
    ctx->labels_host = labels_from_files(prefix, ctx->n, ctx->stream);
    pm::relayout(*ctx);
  });
}

int pm_reset(pm_ctx* ctx) {
  return ctx_call(ctx, [&] { pm::reset_state(*ctx); });
}

int pm_lcc_bsp(pm_ctx* ctx, int init_step, uint64_t itr, pm_lcc_stats* out) {
  (void)itr;
  return ctx_call(ctx, [&] {
    pm::LccOut lo = pm::lcc_call(*ctx, init_step != 0);
    if (out) {
      *out = pm_lcc_stats{};
      out->supersteps = lo.seconds.size();
      for (auto t : lo.trav) out->edges_traversed += t;
      for (auto x : lo.vcount.back()) out->active_vertices += x;
      for (auto x : lo.ecount.back()) out->active_edges += x;
      out->not_finished = lo.not_finished ? 1 : 0;
    }
  });
}

int pm_token_passing(pm_ctx* ctx, uint32_t pl, pm_tp_stats* out) {
  return ctx_call(ctx, [&] {
    if (ctx->comm) throw std::runtime_error("pm_token_passing: sharded contexts run lines through pm_run_beta");
    if (pl >= ctx->pattern.lines.size()) throw std::runtime_error("NLC line index out of range");
    const auto& line = ctx->pattern.lines[pl];
    pm::TpResult r;
    if (pl >= 4) {
      std::vector<uint32_t> walks;
      uint32_t stride = 0;
      r = pm::run_tds_line(*ctx, line, walks, stride);
    } else {
      r = pm::run_path_line(*ctx, line);
    }
    if (out) {
      out->sources = r.sources;
      out->acked_sources = 0;
      out->edges_traversed = r.edges;
      out->tokens = r.tokens;
      out->walks = r.walks;
    }
  });
}

int pm_tds(pm_ctx* ctx, uint32_t pl, pm_path_sink sink, void* user, pm_tp_stats* out) {
  return ctx_call(ctx, [&] {
    if (ctx->comm) throw std::runtime_error("pm_tds: sharded contexts run lines through pm_run_beta");
    if (pl >= ctx->pattern.lines.size()) throw std::runtime_error("NLC line index out of range");
    if (pl < 4) throw std::runtime_error("pm_tds: line index below 4 is a path / cycle line (pm_token_passing)");
    // kept walks reach the sink chunk by chunk, in the enumeration's order
    uint32_t stride = 0;
    std::vector<uint32_t> ids;
    const pm::TpResult r = pm::run_tds_line(*ctx, ctx->pattern.lines[pl], stride,
                                            [&](const uint32_t* w, uint64_t n) {
                                              if (!sink) return;
                                              ids.resize(stride);
                                              for (uint64_t i = 0; i < n; ++i) {
                                                for (uint32_t p = 0; p < stride; ++p)
                                                  ids[p] = ctx->perm_host[w[i * stride + p]];
                                                sink(user, pm::owner_host(*ctx, ids[stride - 1]), ids.data(), stride);
                                              }
                                            });
    if (out) {
      out->sources = r.sources;
      out->acked_sources = 0;
      out->edges_traversed = r.edges;
      out->tokens = r.tokens;
      out->walks = r.walks;
    }
  });
}

int pm_post_token_passing(pm_ctx* ctx, uint32_t pl, uint32_t* deleted) {
  return ctx_call(ctx, [&] {
    if (pl >= ctx->pattern.lines.size()) throw std::runtime_error("NLC line index out of range");
    const uint32_t d = pm::launch_post_tp(*ctx, ctx->pattern.lines[pl]);
    if (deleted) *deleted = d;
  });
}

int pm_run_beta(pm_ctx* ctx, const char* result_dir, uint64_t max_iterations, pm_run_stats* out) {
  return ctx_call(ctx, [&] { pm::run_beta(*ctx, result_dir ? result_dir : "", max_iterations, out); });
}

int pm_export_state(pm_ctx* ctx, uint16_t* tpub, uint32_t* mdeg, uint32_t* nbrs, uint64_t* n_edges) {
  return ctx_call(ctx, [&] {
    std::vector<uint16_t> t;
    std::vector<uint32_t> d, nb;
    pm::export_state_all(*ctx, t, d, nb);
    if (tpub) std::copy(t.begin(), t.end(), tpub);
    if (mdeg) std::copy(d.begin(), d.end(), mdeg);
    if (nbrs) std::copy(nb.begin(), nb.end(), nbrs);
    if (n_edges) *n_edges = nb.size();
  });
}

int pm_graph_size(const pm_ctx* ctx, uint64_t* n, uint64_t* nnz, int* symmetric) {
  if (!ctx) return -1;
  if (n) *n = ctx->n;
  if (nnz) *nnz = ctx->nnz;
  if (symmetric) *symmetric = ctx->symmetric ? 1 : 0;
  return 0;
}

int pm_comm_info(const pm_ctx* ctx, uint32_t* nshards, uint32_t* shard, int32_t* comm_ranks, int32_t* transport) {
  if (!ctx) return -1;
  return api_call(-1, [&] {
    if (nshards) *nshards = ctx->nshards;
    if (shard) *shard = ctx->shard;
    if (comm_ranks) *comm_ranks = ctx->comm ? ctx->comm->ranks() : 0;
    if (transport) *transport = ctx->comm ? ctx->comm->transport() : PM_TRANSPORT_NONE;
    return 0;
  });
}

int pm_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}

const char* pm_build_arch(void) { return "gfx950"; }

void pm_free_host(void* p) { std::free(p); }

// --- sharded searches --------------------------------------------------------------------------------------------

int pm_comm_unique_id(uint8_t* out, uint64_t len) {
  return api_call(-1, [&] { return static_cast<int>(pm::rccl_unique_id(out, len)); });
}

pm_ctx* pm_create_shard(const pm_shard_desc* d, const char* pattern_dir, int device, const uint8_t* unique_id) {
  return api_call<pm_ctx*>(nullptr, [&] {
    if (!d || !unique_id) throw std::runtime_error("pm_create_shard: null argument");
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    pm::CtxInput in = shard_input(*d, "pm_create_shard");
    // the exchanges run whenever a communicator is present (also for one shard)
    in.comm = pm::make_rccl_comm(unique_id, static_cast<int>(d->nshards), static_cast<int>(d->shard));
    return pm::create_ctx(in, pattern_dir, device);
  });
}

pm_ctx* pm_create_shard_host_comm(const pm_shard_desc* d, const char* pattern_dir, int device,
                                  const pm_host_comm* comm) {
  return api_call<pm_ctx*>(nullptr, [&] {
    if (!d || !comm) throw std::runtime_error("pm_create_shard_host_comm: null argument");
    if (comm->nshards != d->nshards || comm->shard != d->shard)
      throw std::runtime_error("pm_create_shard_host_comm: communicator and shard disagree on nshards / shard");
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    pm::CtxInput in = shard_input(*d, "pm_create_shard_host_comm");
    in.comm = pm::make_host_comm(*comm);
    return pm::create_ctx(in, pattern_dir, device);
  });
}

int pm_run_beta_local_shards(const pm_graph_desc* g, const char* pattern_dir, int device, uint32_t nshards,
                             const uint64_t* labels, const char* label_prefix, const char* result_dir,
                             uint64_t max_iterations, uint32_t repeats, pm_run_stats* per_shard) {
  return api_call(-1, [&] {
    if (!g || !g->off || !g->col) throw std::runtime_error("pm_run_beta_local_shards: null graph");
    if (nshards == 0 || nshards > 64) throw std::runtime_error("pm_run_beta_local_shards: 1..64 shards");
    pm::require_gfx950(device);
    const uint64_t n = g->n;
    std::vector<uint32_t> gdeg(n);
    for (uint64_t v = 0; v < n; ++v) {
      const uint64_t d = g->off[v + 1] - g->off[v];
      if (d > 0xFFFFFFFFull) throw std::runtime_error("degree above 2^32");
      gdeg[v] = static_cast<uint32_t>(d);
    }
    // -v files: parsed on the device once, the same labels for every shard
    std::vector<uint64_t> file_labels;
    if (label_prefix) {
      PM_HIP_CHECK(hipSetDevice(device));
      Stream s;
      file_labels = labels_from_files(label_prefix, n, s.s);
      labels = file_labels.data();
    }
    run_local_shards(nshards, labels, result_dir, max_iterations, repeats, per_shard,
                     [&](uint32_t q, pm::ThreadGroup& grp, std::unique_lock<std::mutex>& dev) {
      // this shard's rows, built on the host by every shard thread at once: shard q holds the rows of ids
      // v % nshards == q; a delegate's row (degree >= the hub threshold) is split by target owner -- shard q
      // holds its entries u with u % nshards == q (delegate_partitioned_graph.ipp:818-969, 1402-1648)
      std::vector<uint64_t> off(n + 1, 0);
      const bool split = nshards > 1;
      for (uint64_t v = 0; v < n; ++v) {
        uint64_t k = 0;
        if (split && gdeg[v] >= g->hub_threshold) {
          for (uint64_t e = g->off[v]; e < g->off[v + 1]; ++e) k += g->col[e] % nshards == q;
        } else if (v % nshards == q) {
          k = gdeg[v];
        }
        off[v + 1] = off[v] + k;
      }
      std::vector<uint32_t> col(std::max<uint64_t>(off[n], 1), 0);
      for (uint64_t v = 0; v < n; ++v) {
        if (off[v + 1] == off[v]) continue;
        uint32_t* out = col.data() + off[v];
        if (split && gdeg[v] >= g->hub_threshold) {
          for (uint64_t e = g->off[v]; e < g->off[v + 1]; ++e)
            if (g->col[e] % nshards == q) *out++ = g->col[e];
        } else {
          std::copy(g->col + g->off[v], g->col + g->off[v + 1], out);
        }
      }
      dev.lock();
      PM_HIP_CHECK(hipSetDevice(device));
      pm::CtxInput in;
      in.n = n;
      in.off = off.data();
      in.col = col.data();
      in.gdeg = gdeg.data();
      in.symmetric = g->symmetric != 0;
      in.nranks = g->nranks;
      in.hub_threshold = g->hub_threshold;
      in.nshards = nshards;
      in.shard = q;
      in.comm = pm::make_thread_comm(&grp, static_cast<int>(q));
      in.inprocess_shards = nshards;
      return pm::create_ctx(in, pattern_dir, device);  // (the context holds its copy of the rows)
    });
    return 0;
  });
}

pm_ctx* pm_create_rmat_shard(uint64_t scale, uint64_t p_gen, const char* pattern_dir, int device, uint32_t nranks,
                             uint64_t hub_threshold, uint32_t nshards, uint32_t shard, const uint8_t* unique_id,
                             double* gen_seconds) {
  return api_call<pm_ctx*>(nullptr, [&] {
    if (!unique_id) throw std::runtime_error("pm_create_rmat_shard: null communicator id");
    PM_HIP_CHECK(hipSetDevice(device));
    pm::Comm* comm = pm::make_rccl_comm(unique_id, static_cast<int>(nshards), static_cast<int>(shard));
    return create_rmat_shard_ctx(scale, p_gen, pattern_dir, device, nranks, hub_threshold, nshards, shard, comm, 1,
                                 gen_seconds);
  });
}

int pm_run_rmat_local_shards(uint64_t scale, uint64_t p_gen, const char* pattern_dir, int device, uint32_t nshards,
                             uint32_t nranks, uint64_t hub_threshold, const uint64_t* labels, const char* result_dir,
                             uint64_t max_iterations, uint32_t repeats, pm_run_stats* per_shard) {
  return api_call(-1, [&] {
    if (nshards == 0 || nshards > 64) throw std::runtime_error("pm_run_rmat_local_shards: 1..64 shards");
    run_local_shards(nshards, labels, result_dir, max_iterations, repeats, per_shard,
                     [&](uint32_t q, pm::ThreadGroup& grp, std::unique_lock<std::mutex>& dev) {
      dev.lock();  // (generated on the device: no host phase)
      PM_HIP_CHECK(hipSetDevice(device));
      return create_rmat_shard_ctx(scale, p_gen, pattern_dir, device, nranks, hub_threshold, nshards, q,
                                   pm::make_thread_comm(&grp, static_cast<int>(q)), nshards, nullptr);
    });
    return 0;
  });
}

// --- input builders ----------------------------------------------------------------------------------------------

int pm_rmat_edges(uint64_t scale, uint64_t p_gen, uint64_t first, uint64_t stride, uint32_t** src, uint32_t** dst,
                  uint64_t* m) {
  return api_call(-1, [&] {
    if (stride == 0) throw std::runtime_error("pm_rmat_edges: stride 0");
    std::vector<uint64_t> vr;
    for (uint64_t r = first; r < p_gen; r += stride) vr.push_back(r);
    if (p_gen == 0) throw std::runtime_error("P_gen must be positive");
    const uint64_t total = 2 * pm::rmat_edges_per_rank(scale, p_gen) * vr.size();
    auto s = host_alloc<uint32_t>(total, "pm_rmat_edges"), d = host_alloc<uint32_t>(total, "pm_rmat_edges");
    *m = pm::rmat_stream_of(scale, p_gen, vr, [&](uint64_t i, uint32_t u, uint32_t v) {
      s.get()[i] = u;
      d.get()[i] = v;
    });
    *src = s.release();
    *dst = d.release();
    return 0;
  });
}

int pm_rmat_csr(uint64_t scale, uint64_t p_gen, uint64_t** off, uint32_t** col, uint64_t* n) {
  return api_call(-1, [&] {
    pm::Csr g = pm::build_rmat_csr(scale, p_gen);
    *n = g.n;
    *off = static_cast<uint64_t*>(std::malloc(g.off.size() * sizeof(uint64_t)));
    *col = static_cast<uint32_t*>(std::malloc(std::max<size_t>(1, g.col.size()) * sizeof(uint32_t)));
    std::memcpy(*off, g.off.data(), g.off.size() * sizeof(uint64_t));
    std::memcpy(*col, g.col.data(), g.col.size() * sizeof(uint32_t));
    return 0;
  });
}

// GPU generator (pm_rmat.hip): the same CSR as pm_rmat_csr, built on `device`.
int pm_rmat_csr_gpu(uint64_t scale, uint64_t p_gen, int device, uint64_t** off, uint32_t** col, uint64_t* n) {
  return api_call(-1, [&] {
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    Stream s;
    pm::DevCsr g;
    CsrGuard hold{g};
    g = pm::rmat_csr_device(scale, p_gen, s.s);
    auto o = host_alloc<uint64_t>(g.n + 1, "pm_rmat_csr_gpu");
    auto c = host_alloc<uint32_t>(g.nnz, "pm_rmat_csr_gpu");
    PM_HIP_CHECK(hipMemcpy(o.get(), g.d_off, (g.n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (g.nnz) PM_HIP_CHECK(hipMemcpy(c.get(), g.d_col, g.nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *off = o.release();
    *col = c.release();
    *n = g.n;
    return 0;
  });
}

// Context over an R-MAT graph generated on the device itself (no host copy of
// the adjacency): the north_star S=28 one-GPU configuration.
pm_ctx* pm_create_rmat(uint64_t scale, uint64_t p_gen, const char* pattern_dir, int device, uint32_t nranks,
                       uint64_t hub_threshold, double* gen_seconds) {
  return api_call<pm_ctx*>(nullptr, [&] {
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    Stream s;
    pm::DevCsr g;
    CsrGuard hold{g};
    const auto t0 = std::chrono::steady_clock::now();
    g = pm::rmat_csr_device(scale, p_gen, s.s);
    if (gen_seconds) *gen_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<uint64_t> off(g.n + 1);
    PM_HIP_CHECK(hipMemcpy(off.data(), g.d_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    (void)hipFree(g.d_off);
    g.d_off = nullptr;
    pm::CtxInput in;
    in.n = g.n;
    in.off = off.data();
    in.col = g.d_col;
    in.col_on_device = true;
    in.col_release = true;  // the context frees the generated adjacency once it holds its copy
    g.d_col = nullptr;
    in.symmetric = true;
    in.nranks = nranks;
    in.hub_threshold = hub_threshold;
    return pm::create_ctx(in, pattern_dir, device);
  });
}

// GPU text ingest (pm_ingest.hip): the CSR ingest_edge_list builds, returned to the host.
int pm_ingest_edge_list_gpu(const char* const* files, uint32_t nfiles, int undirected, int device, uint64_t** off,
                            uint32_t** col, uint64_t* n, int* symmetric) {
  return api_call(-1, [&] {
    if (!off || !col || !n) throw std::runtime_error("null output");
    const std::vector<std::string> fl = file_list(files, nfiles);
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    Stream s;
    pm::IngestCsr g;
    CsrGuard hold_fwd{g.fwd}, hold_rev{g.rev};
    g = pm::ingest_edges_device(fl, undirected != 0, false, s.s);
    auto o = host_alloc<uint64_t>(g.fwd.n + 1, "pm_ingest_edge_list_gpu");
    auto c = host_alloc<uint32_t>(g.fwd.nnz, "pm_ingest_edge_list_gpu");
    PM_HIP_CHECK(hipMemcpy(o.get(), g.fwd.d_off, (g.fwd.n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (g.fwd.nnz)
      PM_HIP_CHECK(hipMemcpy(c.get(), g.fwd.d_col, g.fwd.nnz * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *off = o.release();
    *col = c.release();
    *n = g.fwd.n;
    if (symmetric) *symmetric = g.symmetric ? 1 : 0;
    return 0;
  });
}

// Context over a graph ingested from text on the device (the adjacency never
// leaves HBM; a directed graph's in-rows come from the same sort).
pm_ctx* pm_create_edge_list(const char* const* files, uint32_t nfiles, int undirected, const char* pattern_dir,
                            int device, uint32_t nranks, uint64_t hub_threshold, double* ingest_seconds) {
  return api_call<pm_ctx*>(nullptr, [&] {
    const std::vector<std::string> fl = file_list(files, nfiles);
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    Stream s;
    pm::IngestCsr g;
    CsrGuard hold_fwd{g.fwd}, hold_rev{g.rev};
    const auto t0 = std::chrono::steady_clock::now();
    g = pm::ingest_edges_device(fl, undirected != 0, true, s.s);
    if (ingest_seconds)
      *ingest_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<uint64_t> off(g.fwd.n + 1), roff;
    PM_HIP_CHECK(hipMemcpy(off.data(), g.fwd.d_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    pm::CtxInput in;
    in.n = g.fwd.n;
    in.off = off.data();
    in.col = g.fwd.d_col;
    in.col_on_device = true;
    in.symmetric = g.symmetric;
    in.nranks = nranks;
    in.hub_threshold = hub_threshold;
    if (!g.symmetric) {
      roff.resize(g.rev.n + 1);
      PM_HIP_CHECK(hipMemcpy(roff.data(), g.rev.d_off, roff.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
      in.in_off = roff.data();
      in.in_col = g.rev.d_col;
    }
    return pm::create_ctx(in, pattern_dir, device);
  });
}

// Host check of the MT19937 jump-ahead machinery (host/mt_jump.hpp): the
// first `count` outputs of std::mt19937(seed) after skipping `skip` outputs,
// obtained by one polynomial jump instead of stepping.
int pm_mt19937_jump_outputs(uint32_t seed, uint64_t skip, uint32_t* out, uint64_t count) {
  return api_call(-1, [&] {
    uint32_t w[pm::mtj::kN], wj[pm::mtj::kN];
    pm::mtj::seed_window(seed, w);
    pm::mtj::apply(pm::mtj::jump_poly(skip), w, wj);
    std::vector<uint32_t> seq(pm::mtj::kN + count);
    pm::mtj::extend(wj, seq.data(), seq.size());
    for (uint64_t i = 0; i < count; ++i) out[i] = pm::mtj::temper(seq[pm::mtj::kN + i]);
    return 0;
  });
}

int pm_write_graph(const char* base, uint64_t n, const uint64_t* off, const uint32_t* col, int symmetric,
                   uint32_t nranks, uint64_t hub_threshold) {
  return api_call(-1, [&] {
    pm::Csr g;
    g.n = n;
    g.off.assign(off, off + n + 1);
    g.col.assign(col, col + off[n]);
    g.symmetric = symmetric != 0;
    pm::write_graph_files(base, g, nranks, hub_threshold);
    return 0;
  });
}

int pm_read_graph(const char* base, uint64_t** off, uint32_t** col, uint64_t* n, int* symmetric, uint32_t* nranks,
                  uint64_t* hub_threshold) {
  return api_call(-1, [&] {
    uint32_t p = 1;
    uint64_t h = 0;
    pm::Csr g = pm::read_graph_files(base, &p, &h);
    *n = g.n;
    *off = static_cast<uint64_t*>(std::malloc(g.off.size() * sizeof(uint64_t)));
    *col = static_cast<uint32_t*>(std::malloc(std::max<size_t>(1, g.col.size()) * sizeof(uint32_t)));
    std::memcpy(*off, g.off.data(), g.off.size() * sizeof(uint64_t));
    std::memcpy(*col, g.col.data(), g.col.size() * sizeof(uint32_t));
    if (symmetric) *symmetric = g.symmetric ? 1 : 0;
    if (nranks) *nranks = p;
    if (hub_threshold) *hub_threshold = h;
    return 0;
  });
}

int pm_graph_partitions(const char* base) {
  return api_call(-1, [&] {
    if (!base) throw std::runtime_error("pm_graph_partitions: null base");
    const uint32_t p = pm::graph_file_partitions(base);
    if (p == 0) throw std::runtime_error(std::string("no graph files found for base ") + base);
    return static_cast<int>(p);
  });
}

int pm_read_graph_shard(const char* base, uint32_t nshards, uint32_t shard, uint64_t** off, uint32_t** col,
                        uint32_t** degree, uint64_t* n, int* symmetric, uint32_t* nranks, uint64_t* hub_threshold) {
  return api_call(-1, [&] {
    if (!base || !off || !col || !degree || !n) throw std::runtime_error("pm_read_graph_shard: null argument");
    pm::ShardCsr s = pm::read_graph_shard(base, nshards, shard);
    auto o = host_alloc<uint64_t>(s.off.size(), "pm_read_graph_shard");
    auto c = host_alloc<uint32_t>(s.col.size(), "pm_read_graph_shard");
    auto d = host_alloc<uint32_t>(s.degree.size(), "pm_read_graph_shard");
    std::memcpy(o.get(), s.off.data(), s.off.size() * sizeof(uint64_t));
    std::memcpy(c.get(), s.col.data(), s.col.size() * sizeof(uint32_t));
    std::memcpy(d.get(), s.degree.data(), s.degree.size() * sizeof(uint32_t));
    *off = o.release();
    *col = c.release();
    *degree = d.release();
    *n = s.n;
    if (symmetric) *symmetric = s.symmetric ? 1 : 0;
    if (nranks) *nranks = s.nranks;
    if (hub_threshold) *hub_threshold = s.hub_threshold;
    return 0;
  });
}

int pm_write_rmat_text(uint64_t scale, uint64_t p_gen, int device, const char* base, uint64_t* bytes_out) {
  return api_call(-1, [&] {
    if (!base || !p_gen || scale == 0 || scale > 32) throw std::runtime_error("pm_write_rmat_text: bad arguments");
    pm::require_gfx950(device);
    PM_HIP_CHECK(hipSetDevice(device));
    Stream s;
    const pm::RmatPlan plan = pm::rmat_plan(scale, p_gen);
    DevBuf<uint64_t> d_keys(2 * plan.per_rank);
    std::vector<uint64_t> keys(2 * plan.per_rank), u(plan.per_rank), v(plan.per_rank);
    const uint64_t mask = (uint64_t(1) << scale) - 1;
    uint64_t total = 0;
    for (uint64_t r = 0; r < p_gen; ++r) {
      pm::rmat_keys_device(plan, {r}, d_keys.p, s.s);  // keys 2k = (u << S | v), 2k + 1 = (v << S | u)
      PM_HIP_CHECK(hipMemcpy(keys.data(), d_keys.p, keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
      for (uint64_t k = 0; k < plan.per_rank; ++k) {
        u[k] = keys[2 * k] >> scale;
        v[k] = keys[2 * k] & mask;
      }
      total += write_pairs_file(std::string(base) + "." + std::to_string(r), u.data(), v.data(), plan.per_rank, 0);
    }
    if (bytes_out) *bytes_out = total;
    return 0;
  });
}

int pm_write_label_text(const uint64_t* labels, uint64_t n, const char* prefix, uint32_t nfiles, uint64_t* bytes_out) {
  return api_call(-1, [&] {
    if (!labels || !prefix || !nfiles) throw std::runtime_error("pm_write_label_text: bad arguments");
    uint64_t total = 0;
    const uint64_t per = (n + nfiles - 1) / nfiles;
    for (uint32_t i = 0; i < nfiles; ++i) {
      const uint64_t b = std::min<uint64_t>(n, uint64_t(i) * per), e = std::min<uint64_t>(n, b + per);
      total += write_pairs_file(std::string(prefix) + "." + std::to_string(i), labels + b, nullptr, e - b, b);
    }
    if (bytes_out) *bytes_out = total;
    return 0;
  });
}

int pm_pattern_summary(const char* pattern_dir, char* buf, uint64_t buflen) {
  return api_call(-1, [&] {
    const pm::Pattern p = pm::load_pattern_dir(pattern_dir);
    std::ostringstream o;
    auto vec = [&o](const std::vector<uint64_t>& v) {
      o << "[";
      for (size_t i = 0; i < v.size(); ++i) o << (i ? "," : "") << v[i];
      o << "]";
    };
    o << "{\"vertex_count\":" << p.graph.vertex_count << ",\"edge_count\":" << p.graph.edge_count
      << ",\"diameter\":" << p.graph.diameter << ",\"vertices\":";
    vec(p.graph.vertices);
    o << ",\"edges\":";
    vec(p.graph.edges);
    o << ",\"vertex_data\":";
    vec(p.graph.vertex_data);
    o << ",\"adj\":[";
    for (size_t t = 0; t < p.graph.vertex_data.size(); ++t) o << (t ? "," : "") << p.graph.adj[t];
    o << "],\"lines\":[";
    for (size_t i = 0; i < p.lines.size(); ++i) {
      const auto& l = p.lines[i];
      o << (i ? "," : "") << "{\"labels\":";
      vec(l.labels);
      o << ",\"indices\":";
      vec(l.indices);
      o << ",\"C\":" << l.cycle_length << ",\"VC\":" << l.valid_cycle << ",\"IL\":" << l.interleave_lp
        << ",\"SV\":" << l.selected_vertices << ",\"enumeration\":";
      vec(l.enumeration);
      o << "}";
    }
    o << "]}";
    const std::string s = o.str();
    if (s.size() + 1 > buflen) throw std::runtime_error("summary buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return 0;
  });
}

}  // extern "C"
