// Host driver of a search on the MI355X pattern-matching path.
//
// run_beta restates the driver loop of src/run_pattern_matching_beta.cpp
// (:539-1425) on top of the device kernels in pm_kernels.hip and writes the
// same result directory layout.  Everything the timed
// path calls on the host (reset_state, lcc_call, the count / export helpers)
// lives in this one translation unit.

#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <algorithm>
#include <bitset>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "pm_device.hpp"
#include "pm_host.hpp"

namespace pm {

static void mkdir_p(const std::string& path) {
  std::string cur;
  for (size_t i = 0; i < path.size(); ++i) {
    cur += path[i];
    if (path[i] == '/' && cur.size() > 1) ::mkdir(cur.c_str(), 0755);
  }
  ::mkdir(path.c_str(), 0755);
}

static std::string fmt_double(double x) {
  std::ostringstream o;
  o << x;
  return o.str();
}

void reset_state(Ctx& c, bool defer) {
  if (c.tpub_clean && c.lcc_started) {
    c.clear_pending = true;  // nonzero T_pub only at (every shard's) slist entries; d_nS zeroed after the clear
    c.clear_cap = c.nS_host;
  } else {
    if (!c.tpub_clean) {
      PM_HIP_CHECK(hipMemsetAsync(c.d_tpub[0], 0, c.n * sizeof(uint16_t), c.stream));
      PM_HIP_CHECK(hipMemsetAsync(c.d_tpub[1], 0, c.n * sizeof(uint16_t), c.stream));
    }
    zero_later(c, c.d_nS, sizeof(uint32_t));
  }
  c.tpub_clean = true;
  c.lines_prelaunched = false;  // (a failed search may leave one behind; the stream has run it)
  // d_tsm needs no reset: only sources are read, and selecting a source resets its entry
  c.smask_valid = false;
  zero_later(c, c.d_flags, 4 * sizeof(uint32_t));
  queue_lines_ctl_clear(c);
  if (!defer) flush_zero(c);
  c.cur = 0;
  c.nS_host = 0;
  c.push_long = true;  // full-length rows until the first row compaction
  c.lcc_started = false;
  c.replicated = false;
  c.k1_dense = false;
  c.nsources = 0;
  c.npseen = 0;
}

void debug_point(Ctx& c, const char* where) {
  static const int level = std::getenv("PM_DEBUG_SYNC") ? std::atoi(std::getenv("PM_DEBUG_SYNC")) : 0;
  if (!level) return;
  hipError_t e = hipStreamSynchronize(c.stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess)
    throw std::runtime_error(std::string("device fault before debug point '") + where + "' (shard " +
                             std::to_string(c.shard) + "): " + hipGetErrorString(e));
  if (level >= 2) std::fprintf(stderr, "[pm dbg] shard %u: %s ok\n", c.shard, where);
}

// PM_DEBUG_WATCH_ID=<vertex id> (diagnostics): the vertex's state on this shard at the named point.
static void debug_watch(Ctx& c, const char* where) {
  static const char* e = std::getenv("PM_DEBUG_WATCH_ID");
  if (!e || c.perm_host.empty()) return;
  const uint64_t id = std::strtoull(e, nullptr, 10);
  uint32_t p = 0;
  PM_HIP_CHECK(hipMemcpy(&p, c.d_pos + id, 4, hipMemcpyDeviceToHost));
  PM_HIP_CHECK(hipStreamSynchronize(c.stream));
  uint16_t t0 = 0, t1 = 0, ts = 0;
  uint32_t ml = 0, ma = 0, ns = 0;
  PM_HIP_CHECK(hipMemcpy(&t0, c.d_tpub[0] + p, 2, hipMemcpyDeviceToHost));
  PM_HIP_CHECK(hipMemcpy(&t1, c.d_tpub[1] + p, 2, hipMemcpyDeviceToHost));
  PM_HIP_CHECK(hipMemcpy(&ts, c.d_tst + p, 2, hipMemcpyDeviceToHost));
  PM_HIP_CHECK(hipMemcpy(&ml, c.d_mlen + p, 4, hipMemcpyDeviceToHost));
  PM_HIP_CHECK(hipMemcpy(&ma, c.d_malive + p, 4, hipMemcpyDeviceToHost));
  PM_HIP_CHECK(hipMemcpy(&ns, c.d_nS, 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> sl(ns);
  if (ns) PM_HIP_CHECK(hipMemcpy(sl.data(), c.d_slist, ns * 4, hipMemcpyDeviceToHost));
  int at = -1;
  for (uint32_t i = 0; i < ns; ++i)
    if (sl[i] == p) at = static_cast<int>(i);
  std::fprintf(stderr, "[pm watch] shard %u %-22s id %llu pos %u: tpub %u/%u (cur %d) tst %u mlen %u malive %u, slist[%d] of %u\n",
               c.shard, where, static_cast<unsigned long long>(id), p, t0, t1, c.cur, ts, ml, ma, at, ns);
}

// Pinned host staging of at least `words` u64 (read-backs of the driver loop).
uint64_t* pinned(Ctx& c, size_t words) {
  if (c.h_pin_words < words) {
    if (c.h_pin) (void)hipHostFree(c.h_pin);
    c.h_pin = nullptr;
    const size_t w = std::max<size_t>(words, 1 << 15);
    PM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c.h_pin), w * sizeof(uint64_t), hipHostMallocDefault));
    c.h_pin_words = w;
  }
  return c.h_pin;
}

void ensure_counts(Ctx& c, size_t slots) {
  if (c.counts_slots >= slots) return;
  if (c.d_counts) (void)hipFree(c.d_counts);
  c.d_counts = dalloc<uint64_t>(slots * slot_words(c));
  c.counts_slots = slots;
}

// label_propagation_pattern_matching_bsp (nonunique_ee.hpp:1033-1153).
LccOut lcc_call(Ctx& c, bool init_step) {
  const uint64_t D = c.pattern.graph.diameter;
  const uint64_t W = slot_words(c);
  const uint64_t P = c.nranks <= 1 ? 1 : c.nranks;
  ensure_counts(c, D);
  while (c.events.size() < D + 3) {
    hipEvent_t e;
    PM_HIP_CHECK(hipEventCreate(&e));
    c.events.push_back(e);
  }
  std::vector<hipEvent_t>& ev = c.events;  // [0..D] superstep bounds, [D+1], [D+2] superstep-0 kernel
  // (a dense superstep-0 state is never packed: with D >= 2 the hand-off follows a later superstep; a directed
  // graph's state is never dense, so PM_HANDOFF=0 replicates it straight after superstep 0)
  const uint64_t handoff_ss =
      D == 1 ? 0 : std::max<uint64_t>(c.symmetric ? 1 : 0, std::min<uint64_t>(c.handoff_ss, D - 1));
  if (init_step) c.push_msgs.clear();
  zero_later(c, c.d_counts, D * W * sizeof(uint64_t));  // kernels add into the slots
  // the search's reset fills go with superstep 0's own (one launch, before the call's timing event)
  if (init_step) queue_lcc_first_fills(c);
  flush_zero(c);
  c.probe("zero flushed");
  PM_HIP_CHECK(hipEventRecord(ev[0], c.stream));
  bool k_timed = false, handed_off = false;
  // diagnostics: PM_DEBUG_LCC_STOP=k -- the first call runs supersteps 0..k-1 only
  static const uint64_t stop_at = std::getenv("PM_DEBUG_LCC_STOP") ? std::strtoull(std::getenv("PM_DEBUG_LCC_STOP"), nullptr, 10) : 0;
  // sharded: the state became the replica (the sharded part of the search ends here)
  auto handoff = [&] {
    if (!c.comm) return;
    if (!c.ev_handoff) PM_HIP_CHECK(hipEventCreate(&c.ev_handoff));
    PM_HIP_CHECK(hipEventRecord(c.ev_handoff, c.stream));
    c.comm_wall_handoff = c.comm->wall;
    handed_off = true;
  };
  for (uint64_t ss = 0; ss < D; ++ss) {
    if (init_step && stop_at && ss >= stop_at) {
      PM_HIP_CHECK(hipEventRecord(ev[D], c.stream));
      break;
    }
    uint64_t* slot = c.d_counts + ss * W;
    if (ss == 0 && init_step) {
      if (c.lcc_started) throw std::runtime_error("init_step LCC after the state map was built");
      // (the call's start event ev[0] directly precedes the kernel -- the search's fills were flushed before it --
      // so it also opens the kernel's own interval: one event record less before superstep 0)
      launch_lcc_first(c, slot, nullptr, ev[D + 2]);
      c.probe("superstep 0 launched");
      debug_point(c, "superstep 0"); debug_watch(c, "superstep 0");
      k_timed = true;
      // |slist| is read back with the counters at the end of the call; until
      // then later supersteps size their grids by its upper bound
      c.nS_host = static_cast<uint32_t>(std::min<uint64_t>(c.ss0_rows, 0xFFFFFFFFull));
      c.lcc_started = true;
      // sharded: the delegates' shares meet at their controllers; the survivors' codes of every shard
      // for the next superstep's pulls; a one-superstep pattern goes to the replica at once
      if (c.split_hubs) shard_hub_combine(c, slot);
      debug_point(c, "delegate combine"); debug_watch(c, "delegate combine");
      // (the codes serve the pull form; a directed graph's push-form supersteps carry T_pub in their messages)
      if (handoff_ss > 0) {
        if (c.symmetric) shard_codes_after_first(c);
      } else {
        shard_replicate(c);
        handoff();
      }
      debug_point(c, "code exchange / replica"); debug_watch(c, "code exchange / replica");
    } else {
      if (!c.lcc_started) throw std::runtime_error("LCC without an initial step: state map is empty");
      // pull form while M is known symmetric (the first call on a symmetric
      // graph: no cycle flag set yet); push form otherwise
      if (!c.force_pull && (!c.symmetric || !init_step)) {
        // a sharded directed search before the replica: the receivers of other shards get messages
        if (c.comm && !c.replicated) launch_lcc_push_sharded(c, slot);
        else launch_lcc_push(c, slot);
        debug_point(c, "push superstep"); debug_watch(c, "push superstep");
      } else {
        // S collapses in the first later supersteps (S=28 tree: 9.8 M -> 0.8 M -> 26 k): the next
        // supersteps, the NLC lines and the next reset walk the live entries only.  (Appending the live
        // entries inside the superstep, one counter reservation per 64-entry chunk, measured 1.2 ms slower
        // at S=28: 153 k atomics on one address serialise.)
        c.cur_ss = init_step ? ss : 0;
        launch_lcc_step(c, slot, init_step && ss == 1, ss + 1 == D, init_step);
        debug_point(c, "pull superstep"); debug_watch(c, "pull superstep");
        if (init_step && (ss == 1 || ss == 2) && ss + 1 < D) launch_compact_slist(c);
        // the codes' clear for the next search (their last reader was the first later superstep), beside the
        // latency-bound small supersteps after the second compaction rather than beside the first
        if (init_step && (ss == 2 || (ss == 1 && D == 2))) side_clear_codes(c);
        debug_point(c, "list compaction"); debug_watch(c, "list compaction");
      }
      // sharded: the state of S goes to the replica after superstep handoff_ss; before, the supersteps run
      // over each shard's own rows, and after the first the shards' new T_pub are exchanged
      if (init_step && ss == handoff_ss) {
        shard_replicate(c);
        handoff();
      } else if (init_step && ss < handoff_ss && c.symmetric) {
        shard_tpub_exchange(c);
      }
      debug_point(c, "superstep end"); debug_watch(c, "superstep end");
    }
    if (c.fine_timing || ss + 1 == D) PM_HIP_CHECK(hipEventRecord(ev[ss + 1], c.stream));
  }
  // rows with dead entries compacted for the lines and the next call (k_compact_rows)
  const uint32_t stamp = ++c.lcc_calls;
  if (!c.no_row_compaction) launch_compact_rows(c, stamp);
  debug_point(c, "row compaction");
  c.probe("lcc issued");
  // read-back through pinned memory: [nS | local counts | summed counts]
  uint64_t* pin = pinned(c, 1 + 2 * D * W);
  // sharded: the supersteps before the replica counted this shard's rows only: their slots are summed
  // over the shards (the replica's supersteps count the whole state on every shard)
  const uint64_t sharded_slots = c.comm && init_step ? handoff_ss + 1 : 0;
  // one context with prelaunched lines: the read-back copies go on a side stream ordered after the call's last
  // kernel, so they run beside the lines instead of in front of them (the lines read neither the list count nor
  // the counters, and the host waits for both)
  const bool side = c.prelaunch_lines && !sharded_slots;
  hipStream_t rs = c.stream;
  if (side) {
    if (!c.rstream) {
      PM_HIP_CHECK(hipStreamCreateWithFlags(&c.rstream, hipStreamNonBlocking));
      PM_HIP_CHECK(hipEventCreateWithFlags(&c.ev_rb, hipEventDisableTiming));
    }
    PM_HIP_CHECK(hipEventRecord(c.ev_rb, c.stream));
    PM_HIP_CHECK(hipStreamWaitEvent(c.rstream, c.ev_rb, 0));
    rs = c.rstream;
    prelaunch_lines_fused(c);  // the device goes on with the lines while the host parses
  }
  PM_HIP_CHECK(hipMemcpyAsync(pin, c.d_nS, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, rs));  // + stamp
  if (sharded_slots) {  // this shard's counts, then the sums over the shards
    PM_HIP_CHECK(hipMemcpyAsync(pin + 1, c.d_counts, D * W * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
    c.comm->allreduce_sum_u64(c.d_counts, sharded_slots * W, c.stream);
  }
  PM_HIP_CHECK(hipMemcpyAsync(pin + 1 + D * W, c.d_counts, D * W * sizeof(uint64_t), hipMemcpyDeviceToHost, rs));
  if (c.prelaunch_lines && !side) prelaunch_lines_fused(c);
  // (with the read-back on the side stream the host parses the counters while the prelaunched lines run; the
  // lines' own read-back waits for the stream in run_lines_fused)
  if (side) stream_wait(c.rstream);
  debug_point(c, "counters + prelaunched lines");
  if (!side) stream_wait(c.stream);
  c.probe("lcc synced");
  std::vector<uint64_t> host(pin + 1 + D * W, pin + 1 + 2 * D * W);
  std::vector<uint64_t> local = sharded_slots ? std::vector<uint64_t>(pin + 1, pin + 1 + D * W) : host;
  const uint32_t nS = static_cast<uint32_t>(pin[0] & 0xFFFFFFFFull);
  c.nS_host = nS;
  c.push_long = c.no_row_compaction || !nS || static_cast<uint32_t>(pin[0] >> 32) == stamp;
  LccOut out;
  bool asym = false;
  {
    const uint64_t* h = local.data() + (D - 1) * W;
    out.loc_vc.assign(h, h + c.nranks);
    out.loc_ec.assign(h + P, h + P + c.nranks);
  }
  for (uint64_t ss = 0; ss < D; ++ss) {
    const uint64_t* h = host.data() + ss * W;
    std::vector<uint64_t> vc(c.nranks), ec(c.nranks);
    for (uint32_t r = 0; r < c.nranks; ++r) {
      vc[r] = h[r];
      ec[r] = h[P + r];
    }
    out.vcount.push_back(vc);
    out.ecount.push_back(ec);
    out.trav.push_back(h[2 * P]);
    if (ss == 0 && init_step) {
      // superstep 0 visits only label-matching rows; their adjacency size is
      // a property of the layout (build_tiling), identical to the reference's count
      out.trav.back() = c.ss0_trav_all;
      out.matching_rows = c.ss0_rows;
      for (uint32_t r = 0; r < c.nranks; ++r) {  // this shard's survivors (roofline bytes)
        out.loc_surv += local[r];
        out.loc_edges += local[P + r];
      }
    }
    if (init_step && ss > 0) {  // pull supersteps that deferred long rows (the next search's pieces launches)
      if (c.long_seen.size() < D) c.long_seen.assign(D, 1);
      c.long_seen[ss] = h[2 * P + 4] != 0;
    }
    if (init_step) {  // the survivors' mean |M| per superstep (the next search's entries in flight)
      uint64_t v = 0, e = 0;
      for (uint32_t r = 0; r < c.nranks; ++r) {
        v += h[r];
        e += h[P + r];
      }
      if (c.m_per_row.size() < D) c.m_per_row.resize(D, 0.0);
      c.m_per_row[ss] = v ? double(e) / double(v) : 0.0;
    }
    if (h[2 * P + 2]) out.not_finished = true;
    if (h[2 * P + 3]) asym = true;
    float ms = 0.f;
    if (c.fine_timing) PM_HIP_CHECK(hipEventElapsedTime(&ms, ev[ss], ev[ss + 1]));
    out.seconds.push_back(ms * 1e-3);
    c.device_seconds += ms * 1e-3;
  }
  if (!c.fine_timing) {  // one interval for the whole call
    float ms = 0.f;
    PM_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[D]));
    c.device_seconds += ms * 1e-3;
  }
  if (k_timed) {
    float ms = 0.f;
    PM_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[D + 2]));
    c.lcc_first_ms = ms;
  }
  if (handed_off) {  // minus the collectives' host time, during which the stream idles (in-process shards wait
                     // for each other there): the shard's own device work and launch gaps
    float ms = 0.f;
    PM_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], c.ev_handoff));
    c.sharded_ms = static_cast<float>(std::max(0.0, ms - (c.comm_wall_handoff - c.comm_wall0) * 1e3));
  }
  c.probe("lcc parsed");
  if (asym)
    throw std::runtime_error(
        "active-edge map became asymmetric (a cycle-marked edge outlived its neighbour's message) in a pull-form "
        "superstep (PM_FORCE_PULL=1)");
  return out;
}

// Algorithmic bytes of the fused superstep-0 kernel (DESIGN.md
// roofline): 4 B neighbour id per scanned adjacency entry, 12 B per scanned
// (label-matching) row (8 B row offset + 2 B T + 2 B TN), 12 B of state per
// survivor (T_state, T_pub, |M| written, mlen) and 4 B per kept M entry.  The
// 2 B neighbour-T gather of the survey's model is not counted: the label-major
// layout derives a neighbour's template bits from its position, no load.
static uint64_t lcc_first_bytes(const Ctx& c, uint64_t scanned, uint64_t survivors, uint64_t edges,
                                uint64_t matching_rows) {
  (void)c;
  return scanned * 4 + matching_rows * 12 + survivors * 12 + edges * 4;
}

struct DriverFiles {
  std::vector<std::string> superstep, step, iteration;
  std::vector<std::vector<std::string>> vcount, ecount, mcount;  // per rank
};

static void add_count_lines(Ctx& c, DriverFiles& f, uint64_t itr, const char* tag, uint64_t idx,
                            const std::vector<uint64_t>& vc, const std::vector<uint64_t>& ec, uint64_t msgs) {
  for (uint32_t r = 0; r < c.nranks; ++r) {
    const std::string pre = std::to_string(itr) + ", " + tag + ", " + std::to_string(idx) + ", ";
    f.vcount[r].push_back(pre + std::to_string(vc[r]));
    f.ecount[r].push_back(pre + std::to_string(ec[r]));
    f.mcount[r].push_back(pre + std::to_string(r == 0 ? msgs : 0));
  }
}

static void count_state(Ctx& c, std::vector<uint64_t>& vc, std::vector<uint64_t>& ec) {
  ensure_counts(c, 1);
  const uint64_t W = slot_words(c);
  const uint64_t P = c.nranks <= 1 ? 1 : c.nranks;
  PM_HIP_CHECK(hipMemsetAsync(c.d_counts, 0, W * sizeof(uint64_t), c.stream));
  if (c.nS_host) launch_count_state(c, c.d_counts);
  std::vector<uint64_t> host(W);
  PM_HIP_CHECK(hipMemcpyAsync(host.data(), c.d_counts, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
  PM_HIP_CHECK(hipStreamSynchronize(c.stream));
  vc.assign(c.nranks, 0);
  ec.assign(c.nranks, 0);
  for (uint32_t r = 0; r < c.nranks; ++r) {
    vc[r] = host[r];
    ec[r] = host[P + r];
  }
}

uint32_t owner_host(const Ctx& c, uint64_t v) {
  if (c.nranks <= 1) return 0;
  if (!c.hubs_host.empty()) {
    auto it = std::lower_bound(c.hubs_host.begin(), c.hubs_host.end(), v);
    if (it != c.hubs_host.end() && *it == v) return static_cast<uint32_t>((it - c.hubs_host.begin()) % c.nranks);
  }
  return static_cast<uint32_t>(v % c.nranks);
}

// State by vertex id: T_pub, |M[v]| and the alive M entries (neighbour ids,
// rows in vertex-id order, entries in the row's order: neighbour-id order).
// The rows of S are packed on the device (pack_state: every member of S is an
// slist entry with T_pub != 0), so only the state map crosses PCIe.  A sharded
// context holds the replica of the whole state after its first superstep pair,
// so every shard exports everything.
static void export_state(Ctx& c, std::vector<uint16_t>& tpub, std::vector<uint32_t>& mdeg,
                         std::vector<uint32_t>& nbrs) {
  const uint64_t n = c.n;
  tpub.assign(n, 0);
  mdeg.assign(n, 0);
  nbrs.clear();
  if (!c.lcc_started || !c.nS_host) return;
  if (c.comm && !c.replicated) throw std::runtime_error("pm_export_state: the sharded state is not replicated yet");
  const uint64_t ne = pack_state_entry_bound(c);
  const uint64_t nr = pinned(c, 2)[0];
  uint32_t *d_rec = nullptr, *d_ent = nullptr;
  PM_HIP_CHECK(hipMalloc(&d_rec, std::max<uint64_t>(c.nS_host, 1) * 16));
  if (hipMalloc(&d_ent, std::max<uint64_t>(ne, 1) * 4) != hipSuccess) {
    (void)hipFree(d_rec);
    throw std::runtime_error("pm_export_state: out of device memory");
  }
  std::vector<uint32_t> rec(nr * 4), ent(ne);
  try {
    pack_state(c, d_rec, d_ent, ne, c.d_xcnt + 2);
    if (nr) PM_HIP_CHECK(hipMemcpyAsync(rec.data(), d_rec, nr * 16, hipMemcpyDeviceToHost, c.stream));
    if (ne) PM_HIP_CHECK(hipMemcpyAsync(ent.data(), d_ent, ne * 4, hipMemcpyDeviceToHost, c.stream));
    PM_HIP_CHECK(hipStreamSynchronize(c.stream));
  } catch (...) {
    (void)hipFree(d_rec);
    (void)hipFree(d_ent);
    throw;
  }
  (void)hipFree(d_rec);
  (void)hipFree(d_ent);
  std::vector<uint64_t> at(n, ~0ull);
  for (uint64_t i = 0; i < nr; ++i) {
    const uint32_t v = c.perm_host[rec[4 * i]];
    tpub[v] = static_cast<uint16_t>(rec[4 * i + 1]);
    mdeg[v] = rec[4 * i + 2];
    at[v] = i;
  }
  for (uint64_t v = 0; v < n; ++v) {
    if (at[v] == ~0ull) continue;
    const uint32_t* r = rec.data() + 4 * at[v];
    for (uint32_t k = 0; k < r[2]; ++k) nbrs.push_back(c.perm_host[ent[r[3] + k] & kPosMask]);
  }
}

void export_state_all(Ctx& c, std::vector<uint16_t>& tpub, std::vector<uint32_t>& mdeg,
                      std::vector<uint32_t>& nbrs) {
  export_state(c, tpub, mdeg, nbrs);
}

static void write_lines(const std::string& path, const std::vector<std::string>& lines) {
  std::ofstream f(path, std::ofstream::out);
  if (!f) throw std::runtime_error("cannot write " + path);
  for (const auto& l : lines) f << l << "\n";
}

// Subgraph lines "[r], w0, ..., wk, [wk]" of kept TDS walks (positions, `stride` per walk), into the file of
// the owner of the last vertex (tds_batch_1.hpp:739-743).
static void add_walk_lines(const Ctx& c, std::vector<std::vector<std::string>>& files, const uint32_t* walks,
                           uint64_t n, uint32_t stride) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t* w = walks + i * stride;
    const uint32_t last = c.perm_host[w[stride - 1]];
    const uint32_t r = owner_host(c, last);
    std::string l = "[" + std::to_string(r) + "], ";
    for (uint32_t p = 0; p < stride; ++p) l += std::to_string(c.perm_host[w[p]]) + ", ";
    l += "[" + std::to_string(last) + "]";
    files[r].push_back(std::move(l));
  }
}

// run_pattern_matching_beta.cpp:539-1425
// (diagnostics, PM_HOST_PROBES=1: the host's time between searches -- from the previous run_beta's return to
// this one's entry, its setup before the first launch, and its end after the last sync -- on stderr)
static std::chrono::steady_clock::time_point g_last_return{};
static double g_last_tail_us = 0;  // the previous search: its last probe ("end") to its return
void run_beta(Ctx& c, const std::string& out_dir, uint64_t max_iterations, pm_run_stats* st) {
  const auto t_entry = std::chrono::steady_clock::now();
  static const bool host_probes = std::getenv("PM_HOST_PROBES") != nullptr;
  c.probes.clear();
  c.probing = host_probes || std::getenv("PM_PHASE_TIMES") != nullptr;
  c.probe("entry");
  const Pattern& P = c.pattern;
  const bool files = !out_dir.empty();
  static const bool build_lines_anyway = std::getenv("PM_BUILD_LINES") != nullptr;  // diagnostics (A/B)
  const bool lines_on = files || build_lines_anyway;
  reset_state(c, true);  // flushed with superstep 0's fills
  c.probe("reset");
  DriverFiles f;
  f.vcount.assign(c.nranks, {});
  f.ecount.assign(c.nranks, {});
  f.mcount.assign(c.nranks, {});
  std::vector<std::vector<std::vector<std::string>>> subgraphs(P.lines.size(),
                                                               std::vector<std::vector<std::string>>(c.nranks));
  pm_run_stats s{};
  const uint64_t comm_calls0 = c.comm ? c.comm->calls : 0, comm_bytes0 = c.comm ? c.comm->bytes : 0;
  if (c.comm) c.comm_wall0 = c.comm->wall;
  c.device_seconds = 0.0;
  c.lines_seconds = 0.0;
  // pattern_time_start (beta.cpp:539): the reset above is only enqueued; the
  // search's kernels follow it on the stream without a host round trip
  const auto t_pattern = std::chrono::steady_clock::now();
  c.probe("start");
  auto since = [](std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
  };
  bool init_step = true, nf = false, terminated = true;
  // PM_PHASE_TIMES=1: per-phase host wall time on stderr (diagnostics)
  const bool phase_times = std::getenv("PM_PHASE_TIMES") != nullptr;
  c.fine_timing = files || phase_times;
  c.probing = phase_times || host_probes;
  double ph_lcc = 0, ph_tp = 0, ph_post = 0, ph_count = 0;
  auto tick = [] { return std::chrono::steady_clock::now(); };
  uint64_t itr = 0;
  uint64_t first_scanned = 0, first_surv = 0, first_edges = 0, first_matching = 0;
  uint64_t last_v = 0, last_e = 0;
  auto totals = [&](const std::vector<uint64_t>& vc, const std::vector<uint64_t>& ec) {
    last_v = 0;
    last_e = 0;
    for (auto x : vc) last_v += x;
    for (auto x : ec) last_e += x;
  };
  // active vertex / edge counts per rank after the latest step
  std::vector<uint64_t> cur_vc(c.nranks, 0), cur_ec(c.nranks, 0);
  std::vector<uint64_t> loc_vc(c.nranks, 0), loc_ec(c.nranks, 0);  // this shard's share (sharded)
  auto record_lcc = [&](const LccOut& lo, uint64_t itr_) {
    loc_vc = lo.loc_vc;
    loc_ec = lo.loc_ec;
    c.live_hint = 0;
    for (auto x : loc_vc) c.live_hint += x;
    for (size_t ss = 0; ss < lo.seconds.size(); ++ss) {
      if (lines_on) {  // (result-file lines are built only when they are written)
        f.superstep.push_back(std::to_string(itr_) + ", LP, " + std::to_string(ss) + ", " + fmt_double(lo.seconds[ss]));
        add_count_lines(c, f, itr_, "LP", ss, lo.vcount[ss], lo.ecount[ss], lo.trav[ss]);
      }
      if (phase_times) {
        uint64_t sv = 0, se = 0;
        for (auto x : lo.vcount[ss]) sv += x;
        for (auto x : lo.ecount[ss]) se += x;
        std::fprintf(stderr, "[pm] LP itr %llu superstep %zu: |S| %llu, |M| %llu, traversed %llu, %.1f us\n",
                     static_cast<unsigned long long>(itr_), ss, static_cast<unsigned long long>(sv),
                     static_cast<unsigned long long>(se), static_cast<unsigned long long>(lo.trav[ss]),
                     lo.seconds[ss] * 1e6);
      }
      s.lcc_edges += lo.trav[ss];
      totals(lo.vcount[ss], lo.ecount[ss]);
      cur_vc = lo.vcount[ss];
      cur_ec = lo.ecount[ss];
    }
  };
  do {
    if (max_iterations && itr >= max_iterations) {
      terminated = false;
      break;
    }
    nf = false;
    const auto t_itr = std::chrono::steady_clock::now();
    const auto t_lp = std::chrono::steady_clock::now();
    const bool was_init = init_step;
    auto t0 = tick();
    // iteration 0 always runs the lines (beta.cpp:686-688): one shard enqueues them behind the LCC
    c.prelaunch_lines = itr == 0 && c.fused_lines && !P.lines.empty();
    LccOut lo = lcc_call(c, init_step);
    c.prelaunch_lines = false;
    ph_lcc += since(t0);
    if (was_init) {  // this shard's superstep-0 kernel (roofline bytes)
      first_scanned = c.ss0_trav;
      first_matching = lo.matching_rows;
      first_surv = lo.loc_surv;
      first_edges = lo.loc_edges;
    }
    record_lcc(lo, itr);
    if (was_init && c.shard == 0 && std::getenv("PM_DEBUG_STATE_DUMP")) {  // diagnostics: the state after it
      std::vector<uint16_t> tp;
      std::vector<uint32_t> md, nb;
      export_state(c, tp, md, nb);
      std::ofstream f(std::getenv("PM_DEBUG_STATE_DUMP"));
      uint64_t at = 0;
      for (uint64_t v = 0; v < c.n; ++v) {
        if (!tp[v]) continue;
        std::vector<uint32_t> row(nb.begin() + at, nb.begin() + at + md[v]);
        std::sort(row.begin(), row.end());
        f << v << " " << tp[v] << " :";
        for (auto x : row) f << " " << x;
        f << "\n";
        at += md[v];
      }
    }
    nf = nf || lo.not_finished;
    if (lines_on) f.step.push_back(std::to_string(itr) + ", LP, " + fmt_double(since(t_lp)));
    init_step = false;
    if (itr == 0) nf = true;  // forced token passing (beta.cpp:686-688)
    if (nf) {
      nf = false;
      // fused lines run in batches (one launch for consecutive lines, see
      // run_lines_fused); a line whose batch overflowed runs on the exact path
      std::vector<FusedLineOut> batch;
      size_t batch_pl0 = 0, exact_at = SIZE_MAX;
      for (size_t pl = 0; pl < P.lines.size(); ++pl) {
        const NlcLine& line = P.lines[pl];
        for (auto& r : subgraphs[pl]) r.clear();  // reopened with truncation (beta.cpp:713-717)
        const auto t_tp = std::chrono::steady_clock::now();
        TpResult tr;
        uint32_t deleted = 0;
        std::vector<uint64_t> vc, ec;
        std::vector<uint32_t> walks;
        uint32_t stride = 0;
        FusedLineOut fo;
        bool fused = false;
        auto t1 = tick();
        if (c.comm && !c.replicated) throw std::runtime_error("internal: NLC line before the sharded state was replicated");
        if (c.fused_lines && pl != exact_at) {
          if (pl < batch_pl0 || pl >= batch_pl0 + batch.size()) {
            for (;;) {
              bool overflow = false;
              const size_t n = run_lines_fused(c, pl, files, batch, overflow);
              s.line_overflows += overflow ? 1 : 0;
              batch_pl0 = pl;
              const bool regrown = c.hash_regrown;
              c.hash_regrown = false;
              if (overflow && !regrown) {  // (walk storage, or no room to grow the table)
                // one context: the line's sources in parts on the fused kernel (local_split_line), else the
                // exact path
                FusedLineOut lo;
                static const bool no_local = std::getenv("PM_LOCAL_SPLIT") && std::string(std::getenv("PM_LOCAL_SPLIT")) == "0";
                if (!no_local && !c.comm && pl + n < P.lines.size() && local_split_line(c, pl + n, files, lo)) {
                  if (phase_times)
                    std::fprintf(stderr, "[pm] line %zu: local split in %u parts\n", pl + n, c.local_split_parts);
                  batch.push_back(std::move(lo));
                } else {
                  exact_at = pl + n;
                }
              }
              if (!(overflow && regrown && n == 0)) break;   // the overflowed line reruns with the grown table
            }
          }
          if (pl >= batch_pl0 && pl < batch_pl0 + batch.size()) {
            fo = std::move(batch[pl - batch_pl0]);
            fused = true;
          }
        }
        if (fused) {
          tr = fo.tr;
          deleted = fo.deleted;
          s.split_lines += fo.split ? 1 : 0;
          vc = cur_vc;
          ec = cur_ec;
          for (uint32_t r = 0; r < c.nranks; ++r) {
            vc[r] -= fo.rm_v[r];
            ec[r] -= fo.rm_e[r];
          }
          walks.swap(fo.walks);
          stride = fo.stride;
          ph_tp += since(t1);
        } else {
          // exact-count path (one launch + sync per position)
          ++s.exact_lines;
          if (pl >= 4) {  // beta.cpp:762-767
            // the kept walks become subgraph lines chunk by chunk (the chunked enumeration bounds the device
            // memory, the lines are all the host keeps)
            tr = run_tds_line(c, line, stride, [&](const uint32_t* w, uint64_t nk) {
              if (lines_on) add_walk_lines(c, subgraphs[pl], w, nk, stride);
            });
            s.tds_chunks += c.last_tds_chunks;
          } else {
            tr = run_path_line(c, line);
            s.path_batches += tr.batches;
          }
          ph_tp += since(t1);
          auto t2 = tick();
          deleted = launch_post_tp(c, line);
          ph_post += since(t2);
          auto t3 = tick();
          count_state(c, vc, ec);
          ph_count += since(t3);
          c.lines_seconds += since(t1);
        }
        if (pl >= 4) {
          s.tds_edges += tr.edges;
          s.walks = tr.walks;
          if (stride) add_walk_lines(c, subgraphs[pl], walks.data(), walks.size() / stride, stride);
        } else {
          s.nlcc_edges += tr.edges;
        }
        if (deleted) nf = true;
        if (lines_on) {
          f.superstep.push_back(std::to_string(itr) + ", TP, " + std::to_string(pl) + ", " + fmt_double(since(t_tp)));
          add_count_lines(c, f, itr, "TP", pl, vc, ec, tr.edges);
        }
        totals(vc, ec);
        cur_vc = vc;
        cur_ec = ec;
        if (deleted && line.interleave_lp) {  // beta.cpp:1163-1197
          const auto t_lpi = std::chrono::steady_clock::now();
          LccOut li = lcc_call(c, false);
          record_lcc(li, itr);
          nf = nf || li.not_finished;
          if (lines_on) f.step.push_back(std::to_string(itr) + ", LP, " + fmt_double(since(t_lpi)));
        }
      }
    } else {
      nf = false;
    }
    if (lines_on) f.iteration.push_back(std::to_string(itr) + ", " + fmt_double(since(t_itr)));
    ++itr;
  } while (nf);
  c.probe("iterations done");
  stream_wait(c.stream);
  c.probe("end");
  const double secs = since(t_pattern);
  if (phase_times)
    std::fprintf(stderr, "[pm] run_beta %.3f ms: lcc %.3f, token passing %.3f, post %.3f, counts %.3f, device %.3f\n",
                 secs * 1e3, ph_lcc * 1e3, ph_tp * 1e3, ph_post * 1e3, ph_count * 1e3, c.device_seconds * 1e3);
  if ((phase_times || host_probes) && !c.probes.empty()) {
    std::string line = "[pm] host:";
    if (g_last_return.time_since_epoch().count()) {
      char buf[128];
      std::snprintf(buf, sizeof(buf), " (previous end to return %.1f, return to entry %.1f, entry to start %.1f)",
                    g_last_tail_us, std::chrono::duration<double>(t_entry - g_last_return).count() * 1e6,
                    (c.probes[0].second - std::chrono::duration<double>(t_entry.time_since_epoch()).count()) * 1e6);
      line += buf;
    }
    double prev = c.probes[0].second;
    for (const auto& pr : c.probes) {
      char buf[96];
      std::snprintf(buf, sizeof(buf), " %s +%.1f", pr.first, (pr.second - prev) * 1e6);
      line += buf;
      prev = pr.second;
    }
    std::fprintf(stderr, "%s us\n", line.c_str());
  }
  s.iterations = itr;
  s.terminated = terminated ? 1 : 0;
  s.hubs = static_cast<uint32_t>(c.hubs_host.size());
  s.nlcc_seconds = c.lines_seconds;
  s.seconds = secs;
  s.device_seconds = c.device_seconds;
  s.lcc_first_kernel_ms = c.lcc_first_ms;
  c.lcc_first_bytes = lcc_first_bytes(c, first_scanned, first_surv, first_edges, first_matching);
  s.lcc_first_bytes = c.lcc_first_bytes;
  s.final_vertices = last_v;
  s.final_edges = last_e;
  s.shard_entries = c.nnz;
  s.shard_rows = c.held_rows;
  s.shard_hub_entries = c.held_hub_entries;
  for (uint64_t j = c.shard; c.split_hubs && j < c.hubs_host.size(); j += c.nshards) ++s.shard_hubs_controlled;
  s.shard_ss0_entries = first_scanned;
  s.shard_ss0_survivors = first_surv;
  s.shard_sharded_ms = c.comm ? c.sharded_ms : 0.0;
  s.shard_in_entries = c.in_entries;
  s.shard_push_supersteps = c.push_msgs.size();
  for (uint64_t m : c.push_msgs) s.shard_push_messages += m;
  if (c.comm) {
    s.comm_calls = c.comm->calls - comm_calls0;
    s.comm_bytes = c.comm->bytes - comm_bytes0;
    s.comm_seconds = c.comm->wall - c.comm_wall0;
  }
  s.replica_rows = c.replica_rows;
  s.replica_entries = c.replica_entries;
  if (files) {
    // result dump (beta.cpp:1370-1425) -- after pattern_time_end, as in the reference
    std::vector<uint16_t> tpub;
    std::vector<uint32_t> mdeg, nbrs;
    export_state_all(c, tpub, mdeg, nbrs);
    if (c.shard != 0) {  // shard 0 writes every rank's files
      if (st) *st = s;
      return;
    }
    const std::string d = out_dir + "/0";
    const char* subdirs[] = {"all_ranks_active_vertices_count", "all_ranks_active_edges_count", "all_ranks_messages",
                             "all_ranks_active_vertices", "all_ranks_active_edges", "all_ranks_subgraphs",
                             "all_ranks_vertex_data"};
    for (auto sd : subdirs) mkdir_p(d + "/" + sd);
    write_lines(out_dir + "/result_pattern_set",
                {"0, " + std::to_string(c.nranks) + ", " + std::to_string(itr) + ", " + fmt_double(secs) + ", " +
                 std::to_string(P.graph.edge_count) + ", " + std::to_string(P.graph.vertex_count) + ", " +
                 std::to_string(P.lines.size())});
    write_lines(d + "/result_iteration", f.iteration);
    write_lines(d + "/result_step", f.step);
    write_lines(d + "/result_superstep", f.superstep);
    std::vector<std::vector<std::string>> av(c.nranks), ae(c.nranks);
    uint64_t pos = 0;
    for (uint64_t v = 0; v < c.n; ++v) {
      if (!tpub[v]) continue;
      const uint32_t r = owner_host(c, v);
      av[r].push_back(std::to_string(r) + ", " + std::to_string(v) + ", 0, " + std::to_string(c.labels_host[v]) + ", " +
                      std::bitset<16>(tpub[v]).to_string());
      for (uint32_t k = 0; k < mdeg[v]; ++k)
        ae[r].push_back(std::to_string(r) + ", " + std::to_string(v) + ", " + std::to_string(nbrs[pos + k]));
      pos += mdeg[v];
    }
    for (uint32_t r = 0; r < c.nranks; ++r) {
      const std::string rs = std::to_string(r);
      write_lines(d + "/all_ranks_active_vertices_count/active_vertices_" + rs, f.vcount[r]);
      write_lines(d + "/all_ranks_active_edges_count/active_edges_" + rs, f.ecount[r]);
      write_lines(d + "/all_ranks_messages/messages_" + rs, f.mcount[r]);
      write_lines(d + "/all_ranks_active_vertices/active_vertices_" + rs, av[r]);
      write_lines(d + "/all_ranks_active_edges/active_edges_" + rs, ae[r]);
      for (size_t pl = 0; pl < P.lines.size(); ++pl)
        write_lines(d + "/all_ranks_subgraphs/subgraphs_" + std::to_string(pl) + "_" + rs, subgraphs[pl][r]);
    }
  }
  if (st) *st = s;
  if (host_probes) {
    g_last_return = std::chrono::steady_clock::now();
    g_last_tail_us = c.probes.empty() ? 0.0
                                      : (std::chrono::duration<double>(g_last_return.time_since_epoch()).count() -
                                         c.probes.back().second) * 1e6;
  }
}

}  // namespace pm
