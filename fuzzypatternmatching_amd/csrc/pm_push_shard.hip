// Sharded search of a directed graph.
//
// A shard of a directed graph is given its owned OUT-rows (ids v % nshards == shard; a delegate's out-row split
// by target owner), as a shard of a symmetric graph is.  Superstep 0 pulls over IN-rows, so construction first
// moves every out-entry (v -> u) to the owner of its target, u % nshards, and builds the in-row CSR of the owned
// vertices there (build_shard_in_rows: collective, untimed).  The later supersteps of the first LCC call run in
// push form over the received-from map M: what a sender delivers to a receiver of another shard travels as a
// 12-byte message in one all-to-all per superstep (launch_lcc_push_sharded), until the state of S is replicated
// (shard_replicate) after superstep PM_HANDOFF.

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "pm_device.hpp"
#include "pm_host.hpp"

namespace pm {

namespace {

// Device allocations of one call, freed with the object (keep() hands one over to the caller).
struct Owned {
  std::vector<void*> ps;
  ~Owned() {
    for (void* p : ps) (void)hipFree(p);
  }
  template <typename T>
  T* get(uint64_t n) {
    void* p = nullptr;
    PM_HIP_CHECK(hipMalloc(&p, std::max<uint64_t>(n, 1) * sizeof(T)));
    ps.push_back(p);
    return static_cast<T*>(p);
  }
  void keep(void* p) { ps.erase(std::remove(ps.begin(), ps.end(), p), ps.end()); }
};

unsigned grid_of(uint64_t items, unsigned per, unsigned cap) {
  const uint64_t g = (items + per - 1) / per;
  return static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>(g, cap)));
}

// ---------------------------------------------------------------------------
// In-rows of the owned vertices.
static constexpr int kInBlock = 256;
static constexpr uint32_t kInPer = 8;                       // entries per thread
static constexpr uint32_t kInChunk = kInBlock * kInPer;     // entries per block
static constexpr uint32_t kMaxShards = 64;

// Row of out-entry e: the last v with off[v] <= e (empty rows skipped).
__device__ __forceinline__ uint64_t row_of_entry(const uint64_t* __restrict__ off, uint64_t n, uint64_t e) {
  uint64_t lo = 0, hi = n;  // first v with off[v + 1] > e
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > e) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Count: the entries of each block's chunk per target owner, bcnt[g * nblocks + block] (LDS histogram, no
// global atomic).  A target outside [0, n) is reported and counted nowhere.
__global__ __launch_bounds__(kInBlock) void k_in_count(const uint32_t* __restrict__ col, uint64_t nnz, uint64_t n,
                                                       uint32_t G, uint32_t nblocks, uint64_t* __restrict__ bcnt,
                                                       unsigned* __restrict__ bad) {
  __shared__ uint32_t s_h[kMaxShards];
  if (threadIdx.x < kMaxShards) s_h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = uint64_t(blockIdx.x) * kInChunk;
  for (uint32_t k = 0; k < kInPer; ++k) {
    const uint64_t e = base + uint64_t(k) * kInBlock + threadIdx.x;
    if (e >= nnz) continue;
    const uint32_t u = col[e];
    if (u >= n) {
      *bad = 1u;
      continue;
    }
    atomicAdd(&s_h[u % G], 1u);
  }
  __syncthreads();
  if (threadIdx.x < G) bcnt[uint64_t(threadIdx.x) * nblocks + blockIdx.x] = s_h[threadIdx.x];
}

// Scatter: bbase = exclusive scan of bcnt (owner-major, so the entries of one owner are consecutive in `out`);
// an entry's slot is its block's base plus its rank inside the block (LDS counter).  Keys (u << 32 | v).
__global__ __launch_bounds__(kInBlock) void k_in_scatter(const uint64_t* __restrict__ off, const uint32_t* __restrict__ col,
                                                         uint64_t nnz, uint64_t n, uint32_t G, uint32_t nblocks,
                                                         const uint64_t* __restrict__ bbase, uint64_t cap,
                                                         uint64_t* __restrict__ out) {
  __shared__ uint32_t s_h[kMaxShards];
  if (threadIdx.x < kMaxShards) s_h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t base = uint64_t(blockIdx.x) * kInChunk;
  for (uint32_t k = 0; k < kInPer; ++k) {
    const uint64_t e = base + uint64_t(k) * kInBlock + threadIdx.x;
    if (e >= nnz) continue;
    const uint32_t u = col[e];
    if (u >= n) continue;
    const uint32_t g = u % G;
    const uint64_t at = bbase[uint64_t(g) * nblocks + blockIdx.x] + atomicAdd(&s_h[g], 1u);
    if (at < cap) out[at] = (uint64_t(u) << 32) | row_of_entry(off, n, e);
  }
}

// Sorted keys (u << 32 | v) -> the in-row offsets (n + 1), the sources, and the in-degree of every row (u32).
// A key whose target is outside [0, n) or not owned here is reported (nothing of it is written).
__global__ void k_in_rows(const uint64_t* __restrict__ keys, uint64_t m, uint64_t n, uint32_t G, uint32_t me,
                          uint64_t* __restrict__ off, uint32_t* __restrict__ col, unsigned* __restrict__ bad) {
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < m; i += uint64_t(gridDim.x) * blockDim.x) {
    const uint64_t k = keys[i], u = k >> 32, v = k & 0xFFFFFFFFull;
    const uint64_t last = keys[m - 1] >> 32;
    if (last >= n) {  // (sorted: the largest target bounds every write below)
      *bad = 1u;
      return;
    }
    if (u % G != me || v >= n) *bad = 1u;
    col[i] = static_cast<uint32_t>(v);
    const uint64_t first = i ? (keys[i - 1] >> 32) + 1 : 0;
    for (uint64_t w = first; w <= u; ++w) off[w] = i;
    if (i == m - 1)
      for (uint64_t w = u + 1; w <= n; ++w) off[w] = m;
  }
}

__global__ void k_row_lengths(const uint64_t* __restrict__ off, uint64_t n, uint32_t* __restrict__ len) {
  for (uint64_t v = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; v < n; v += uint64_t(gridDim.x) * blockDim.x)
    len[v] = static_cast<uint32_t>(off[v + 1] - off[v]);
}

}  // namespace

// Collective.  Every shard makes the same four collectives whatever fails locally (a failed shard contributes
// nothing and reports through `err`); after the first and the second, every shard knows whether all are well and
// the ones that follow are skipped by all or by none.
void build_shard_in_rows(Ctx& c, const CtxInput& in, std::string& err, std::vector<uint64_t>& in_off,
                         uint32_t** d_in_col) {
  const uint32_t G = c.nshards, me = c.shard;
  const uint64_t n = c.n, nnz = in.off[n];
  hipStream_t s = c.stream;
  Owned mem;
  uint64_t* d_keys = nullptr;
  uint64_t* d_cnt = nullptr;  // [0, G): to each owner, [G]: failed; then the gather, G x (G + 1)
  std::vector<uint64_t> sb(G, 0), rb(G, 0);
  uint64_t sent = 0, recvd = 0;
  auto fail = [&](const std::exception& e) {
    if (err.empty()) err = e.what();
  };
  // A: this shard's out-entries bucketed by the owner of their target
  std::vector<uint64_t> cnt(G + 1, 0);
  try {
    d_cnt = mem.get<uint64_t>(uint64_t(G + 1) * (G + 1));
    if (G > kMaxShards) throw std::runtime_error("more than 64 shards");
    if (in.col_on_device) throw std::runtime_error("sharded directed graphs take host-resident shard rows");
    if (in.off[0] != 0) throw std::runtime_error("shard rows: off[0] != 0");
    for (uint64_t v = 0; v < n; ++v)
      if (in.off[v] > in.off[v + 1]) throw std::runtime_error("shard rows: offsets decrease");
    const uint32_t nblocks = static_cast<uint32_t>(std::max<uint64_t>(1, (nnz + kInChunk - 1) / kInChunk));
    if ((nnz + kInChunk - 1) / kInChunk > 0x7FFFFFFFull) throw std::runtime_error("shard rows: too many entries");
    auto* d_off = mem.get<uint64_t>(n + 1);
    auto* d_col = mem.get<uint32_t>(nnz);
    auto* d_bcnt = mem.get<uint64_t>(uint64_t(G) * nblocks + 1);
    auto* d_bbase = mem.get<uint64_t>(uint64_t(G) * nblocks + 1);
    auto* d_bad = mem.get<unsigned>(1);
    d_keys = mem.get<uint64_t>(nnz);
    PM_HIP_CHECK(hipMemcpyAsync(d_off, in.off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (nnz) PM_HIP_CHECK(hipMemcpyAsync(d_col, in.col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    PM_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(unsigned), s));
    PM_HIP_CHECK(hipMemsetAsync(d_bcnt, 0, (uint64_t(G) * nblocks + 1) * sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_in_count, dim3(nblocks), dim3(kInBlock), 0, s, d_col, nnz, n, G, nblocks, d_bcnt, d_bad);
    size_t tb = 0;
    const size_t items = size_t(G) * nblocks + 1;  // (+ 1: the total lands behind the last base)
    PM_HIP_CHECK(rocprim::exclusive_scan(nullptr, tb, d_bcnt, d_bbase, uint64_t(0), items, rocprim::plus<uint64_t>(), s));
    void* d_tmp = mem.get<char>(tb);
    PM_HIP_CHECK(rocprim::exclusive_scan(d_tmp, tb, d_bcnt, d_bbase, uint64_t(0), items, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(k_in_scatter, dim3(nblocks), dim3(kInBlock), 0, s, d_off, d_col, nnz, n, G, nblocks, d_bbase,
                       nnz, d_keys);
    PM_HIP_CHECK(hipGetLastError());
    // the owners' first slots (bbase at g * nblocks) and the total
    std::vector<uint64_t> first(G + 1, 0);
    unsigned bad = 0;
    for (uint32_t g = 0; g <= G; ++g)
      PM_HIP_CHECK(hipMemcpyAsync(&first[g], d_bbase + uint64_t(g) * nblocks, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PM_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    PM_HIP_CHECK(hipStreamSynchronize(s));
    if (bad) throw std::runtime_error("edge target out of range");
    if (first[G] != nnz) throw std::runtime_error("internal: in-row buckets hold " + std::to_string(first[G]) +
                                                   " of " + std::to_string(nnz) + " entries");
    for (uint32_t g = 0; g < G; ++g) cnt[g] = first[g + 1] - first[g];
  } catch (const std::exception& e) {
    fail(e);
    std::fill(cnt.begin(), cnt.end(), 0);
  }
  cnt[G] = err.empty() ? 0 : 1;
  // a shard that could not even allocate the count words cannot take part: nothing to agree with (it throws)
  if (!d_cnt) throw std::runtime_error(err);
  PM_HIP_CHECK(hipMemcpyAsync(d_cnt, cnt.data(), (G + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  c.comm->allgather(d_cnt, d_cnt + (G + 1), (G + 1) * sizeof(uint64_t), s);  // collective 1
  std::vector<uint64_t> all(uint64_t(G) * (G + 1));
  PM_HIP_CHECK(hipMemcpyAsync(all.data(), d_cnt + (G + 1), all.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PM_HIP_CHECK(hipStreamSynchronize(s));
  bool any_failed = false;
  for (uint32_t g = 0; g < G; ++g) any_failed |= all[uint64_t(g) * (G + 1) + G] != 0;
  if (any_failed) {
    if (err.empty()) err = "another shard failed while building its in-rows";
    return;
  }
  for (uint32_t g = 0; g < G; ++g) {
    sb[g] = cnt[g] * sizeof(uint64_t);
    rb[g] = all[uint64_t(g) * (G + 1) + me] * sizeof(uint64_t);
    sent += cnt[g];
    recvd += all[uint64_t(g) * (G + 1) + me];
  }
  // B: room for what arrives
  uint64_t *d_recv = nullptr, *d_alt = nullptr, *d_ioff = nullptr;
  uint32_t *d_icol = nullptr, *d_len = nullptr;
  unsigned* d_bad2 = nullptr;
  void* d_stmp = nullptr;
  size_t stb = 0;
  unsigned bits = 32;  // sort key: the source's 32 bits and the target's (targets < n)
  while (bits < 64 && (n >> (bits - 32))) ++bits;
  try {
    if (recvd >= (1ull << 36)) throw std::runtime_error("more than 2^36 in-row entries on one shard");
    d_recv = mem.get<uint64_t>(recvd);
    d_alt = mem.get<uint64_t>(recvd);
    d_ioff = mem.get<uint64_t>(n + 1);
    d_icol = mem.get<uint32_t>(recvd);
    d_len = mem.get<uint32_t>(n);
    d_bad2 = mem.get<unsigned>(1);
    if (recvd > 1) {
      rocprim::double_buffer<uint64_t> db(d_recv, d_alt);
      PM_HIP_CHECK(rocprim::radix_sort_keys(nullptr, stb, db, size_t(recvd), 0u, bits, s));
      d_stmp = mem.get<char>(stb);
    }
    PM_HIP_CHECK(hipMemsetAsync(d_len, 0, std::max<uint64_t>(n, 1) * sizeof(uint32_t), s));
    PM_HIP_CHECK(hipMemsetAsync(d_ioff, 0, (n + 1) * sizeof(uint64_t), s));
    PM_HIP_CHECK(hipMemsetAsync(d_bad2, 0, sizeof(unsigned), s));
    PM_HIP_CHECK(hipStreamSynchronize(s));
  } catch (const std::exception& e) {
    fail(e);
  }
  if (shard_agree_min(c, err.empty() ? 1 : 0) == 0) {  // collective 2
    if (err.empty()) err = "another shard failed while building its in-rows";
    return;
  }
  c.comm->alltoallv(d_keys, sb.data(), d_recv, rb.data(), s);  // collective 3: 8 bytes per out-entry
  // C: the received (target, source) pairs sorted into the in-row CSR: rows in source-id order, duplicates and
  // self loops with their multiplicity (as the one-context transpose keeps them)
  try {
    const uint64_t* sorted = d_recv;
    if (recvd > 1) {
      rocprim::double_buffer<uint64_t> db(d_recv, d_alt);
      PM_HIP_CHECK(rocprim::radix_sort_keys(d_stmp, stb, db, size_t(recvd), 0u, bits, s));
      sorted = db.current();
    }
    if (recvd) {
      hipLaunchKernelGGL(k_in_rows, dim3(grid_of(recvd, 256, 1u << 16)), dim3(256), 0, s, sorted, recvd, n, G, me,
                         d_ioff, d_icol, d_bad2);
      hipLaunchKernelGGL(k_row_lengths, dim3(grid_of(n, 256, 1u << 16)), dim3(256), 0, s, d_ioff, n, d_len);
      PM_HIP_CHECK(hipGetLastError());
    }
    unsigned bad = 0;
    PM_HIP_CHECK(hipMemcpyAsync(&bad, d_bad2, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    in_off.assign(n + 1, 0);
    PM_HIP_CHECK(hipMemcpyAsync(in_off.data(), d_ioff, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PM_HIP_CHECK(hipStreamSynchronize(s));
    if (bad) {
      // (the row lengths of a bad exchange are not added to the other shards' degrees)
      PM_HIP_CHECK(hipMemsetAsync(d_len, 0, std::max<uint64_t>(n, 1) * sizeof(uint32_t), s));
      throw std::runtime_error("in-row exchange: an entry whose target this shard does not own, or a source out of range");
    }
  } catch (const std::exception& e) {
    fail(e);
  }
  // the in-degree of every vertex on every shard (the label-major layout's sort key): each row is held by one
  // shard, so the sum over the shards is its length
  c.comm->allreduce_sum_u32(d_len, n, s);  // collective 4
  if (!err.empty()) return;
  c.rdeg_host.assign(n, 0);
  if (n) PM_HIP_CHECK(hipMemcpyAsync(c.rdeg_host.data(), d_len, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  PM_HIP_CHECK(hipStreamSynchronize(s));
  c.in_entries = recvd;
  (void)sent;
  mem.keep(d_icol);
  *d_in_col = d_icol;
}

// ---------------------------------------------------------------------------
// Sharded push-form superstep.
namespace {

static constexpr uint32_t kMsgWords = 3;  // {receiver position, sender position, T_pub(sender)}: 12 bytes

struct ShardPush {
  uint32_t G, me;
  unsigned long long* cnt;  // count pass: messages per destination shard
  unsigned long long* cur;  // scatter pass: next free message of each destination's bucket
  uint32_t* out;            // the buckets, destination after destination
  uint64_t cap;             // messages `out` holds
};

// One entry per lane (valid: the lane has one); every lane of the wave must call.  Count pass (SCATTER = 0):
// a receiver this shard owns is served in place (push_send_entry), a remote one counted in the block's LDS
// histogram.  Scatter pass: the remote entries are written to their buckets -- one reservation per wave and
// destination (the lanes of one destination are ranked by a ballot), never one per message.
template <int SCATTER>
__device__ __forceinline__ void shard_send_entry(const PushArgs& a, const ShardPush& sp, const uint16_t* s_adj,
                                                 uint32_t* s_dst, bool valid, uint32_t v, uint32_t vid, uint16_t Tv,
                                                 uint32_t m) {
  const uint32_t u = m & kPosMask;
  const bool alive = valid && (m & kAlive);
  const uint32_t g = alive ? a.perm[u] % sp.G : sp.me;
  const bool remote = alive && g != sp.me;
  if (!SCATTER) {
    if (alive && !remote) push_receive(a, s_adj, u, v, vid, Tv);
    if (remote) atomicAdd(&s_dst[g], 1u);
    return;
  }
  const int lane = lane_id();
  uint64_t rem = __ballot(remote);
  while (rem) {
    const int l = __ffsll(static_cast<long long>(rem)) - 1;
    const uint32_t gg = static_cast<uint32_t>(__shfl(static_cast<int>(g), l, kWave));
    const uint64_t same = __ballot(remote && g == gg);
    unsigned long long base = 0;
    if (lane == l) base = atomicAdd(&sp.cur[gg], static_cast<unsigned long long>(__builtin_popcountll(same)));
    base = __shfl(base, l, kWave);
    if (remote && g == gg) {
      const uint64_t at = base + __builtin_popcountll(same & ((1ull << lane) - 1));
      if (at < sp.cap) {
        uint32_t* o = sp.out + at * kMsgWords;
        o[0] = u;
        o[1] = v;
        o[2] = Tv;
      }
    }
    rem &= ~same;
  }
}

// The senders of this shard's rows of S (k_lcc_push_rows<0>'s walk: short rows flattened over the wave, long
// rows cut into pieces for k_push_shard_pieces).
template <int SCATTER>
__global__ __launch_bounds__(kBlock) void k_push_shard_rows(PushArgs a, ShardPush sp, PatArgs pa,
                                                           unsigned long long* __restrict__ trav_out) {
  __shared__ uint16_t s_adj[16];
  __shared__ uint32_t s_dst[kMaxShards];
  __shared__ uint64_t s_beg[kWpb][kWave];
  __shared__ uint32_t s_end[kWpb][kWave], s_v[kWpb][kWave], s_vid[kWpb][kWave];
  __shared__ uint16_t s_T[kWpb][kWave];
  if (threadIdx.x < kMaxShards) s_dst[threadIdx.x] = 0;
  load_adj(s_adj, pa);
  __syncthreads();
  uint64_t trav = 0;
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t nS = *a.nS;
  const uint64_t nch = (nS + kWave - 1) / kWave;
  for (uint64_t ch = uint64_t(blockIdx.x) * kWpb + w; ch < nch; ch += uint64_t(gridDim.x) * kWpb) {
    const uint64_t i = ch * kWave + lane;
    uint32_t v = 0, vid = 0, len = 0;
    uint64_t beg = 0;
    uint16_t T = 0;
    if (i < nS) {
      v = a.slist[i];
      const uint16_t Tv = a.tcur[v];
      if (Tv) {
        T = Tv;
        vid = a.perm[v];
        beg = a.offp[v];
        len = a.mlen[v];
        trav += a.malive[v];
      }
      if (len > kPushLong && push_pieces(a, i, len)) len = 0;
    }
    const uint32_t incl = static_cast<uint32_t>(wave_incl_scan(len));
    const uint32_t total = static_cast<uint32_t>(__shfl(incl, kWave - 1, kWave));
    if (!total) continue;
    s_end[w][lane] = incl;
    s_beg[w][lane] = beg;
    s_v[w][lane] = v;
    s_vid[w][lane] = vid;
    s_T[w][lane] = T;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t t0 = 0; t0 < total; t0 += kWave) {
      const uint32_t t = t0 + lane;
      const bool valid = t < total;
      int lo = 0;
      uint32_t m = 0;
      if (valid) {
        int hi = kWave - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_end[w][mid] > t) hi = mid; else lo = mid + 1;
        }
        m = a.mcol[s_beg[w][lo] + (t - (lo ? s_end[w][lo - 1] : 0u))];
      }
      shard_send_entry<SCATTER>(a, sp, s_adj, s_dst, valid, s_v[w][lo], s_vid[w][lo], s_T[w][lo], m);
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (!SCATTER) {
    __syncthreads();
    if (threadIdx.x < sp.G && s_dst[threadIdx.x])
      atomicAdd(&sp.cnt[threadIdx.x], static_cast<unsigned long long>(s_dst[threadIdx.x]));
    block_atomic_add(trav_out, trav);  // the superstep's traversed-entries word (this shard's senders)
  }
}

// The long rows' pieces: one wave per piece.
template <int SCATTER>
__global__ __launch_bounds__(kBlock) void k_push_shard_pieces(PushArgs a, ShardPush sp, PatArgs pa) {
  __shared__ uint16_t s_adj[16];
  __shared__ uint32_t s_dst[kMaxShards];
  if (threadIdx.x < kMaxShards) s_dst[threadIdx.x] = 0;
  load_adj(s_adj, pa);
  __syncthreads();
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const uint64_t np = min<uint64_t>(*a.npieces, a.piece_cap);
  for (uint64_t k = uint64_t(blockIdx.x) * kWpb + w; k < np; k += uint64_t(gridDim.x) * kWpb) {
    const unsigned long long pc = a.pieces[k];
    if (pc == ~0ull) continue;  // (a slot of a row that did not fit: wave-uniform)
    const uint32_t v = a.slist[pc >> 32];
    const uint32_t q = static_cast<uint32_t>(pc);
    const uint64_t b = a.offp[v] + uint64_t(q) * kPushLong;
    const uint32_t len = min(kPushLong, a.mlen[v] - q * kPushLong);
    const uint16_t Tv = a.tcur[v];
    const uint32_t vid = a.perm[v];
#pragma unroll
    for (int r = 0; r < static_cast<int>(kPushLong / kWave); ++r) {
      const uint32_t j = r * kWave + lane;
      const bool valid = j < len;
      const uint32_t m = valid ? a.mcol[b + j] : 0u;
      shard_send_entry<SCATTER>(a, sp, s_adj, s_dst, valid, v, vid, Tv, m);
    }
  }
  if (!SCATTER) {
    __syncthreads();
    if (threadIdx.x < sp.G && s_dst[threadIdx.x])
      atomicAdd(&sp.cnt[threadIdx.x], static_cast<unsigned long long>(s_dst[threadIdx.x]));
  }
}

// The receivers of the messages that arrived: push_send_entry's receiver half, in its order (the filter,
// TN(u) |= Tv before the edge check, then the flag on M[u][v]).  A position outside [0, n) is reported.
__global__ __launch_bounds__(kBlock) void k_push_apply(PushArgs a, PatArgs pa, const uint32_t* __restrict__ msg,
                                                      uint64_t nmsg, uint64_t n, unsigned* __restrict__ bad) {
  __shared__ uint16_t s_adj[16];
  load_adj(s_adj, pa);
  __syncthreads();
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < nmsg; i += uint64_t(gridDim.x) * blockDim.x) {
    const uint32_t u = msg[i * kMsgWords], v = msg[i * kMsgWords + 1];
    const uint16_t Tv = static_cast<uint16_t>(msg[i * kMsgWords + 2]);
    if (u >= n || v >= n) {
      *bad = 1u;
      continue;
    }
    push_receive(a, s_adj, u, v, a.perm[v], Tv);
  }
}

template <typename T>
T* grow_to(void*& p, size_t& cap, size_t bytes) {
  if (cap < bytes || !p) {
    if (p) (void)hipFree(p);
    p = nullptr;
    const size_t b = std::max<size_t>(bytes + bytes / 8, 4096);
    PM_HIP_CHECK(hipMalloc(&p, b));
    cap = b;
  }
  return static_cast<T*>(p);
}

}  // namespace

void launch_lcc_push_sharded(Ctx& c, uint64_t* d_slot) {
  if (!c.comm) throw std::runtime_error("internal: sharded push superstep without a communicator");
  const uint32_t G = c.nshards, me = c.shard;
  if (G > kMaxShards) throw std::runtime_error("more than 64 shards");
  hipStream_t s = c.stream;
  PushArgs a, av;
  push_prepare(c, a, av);
  const bool pieces = c.push_long;
  const uint32_t P = c.nranks <= 1 ? 1 : c.nranks;
  // [0, 64): counts, [64, 128): cursors, [128]: the apply's error word, [192, 192 + 64 * 64): the gathered counts
  if (!c.d_pushx) PM_HIP_CHECK(hipMalloc(&c.d_pushx, (192 + 64 * 64) * sizeof(unsigned long long)));
  auto* x = static_cast<unsigned long long*>(c.d_pushx);
  PM_HIP_CHECK(hipMemsetAsync(x, 0, 192 * sizeof(unsigned long long), s));
  ShardPush sp{G, me, x, x + 64, nullptr, 0};
  const unsigned grid = grid_of((uint64_t(c.nS_host) + kWave - 1) / kWave, kWpb, 16384);
  auto* trav = reinterpret_cast<unsigned long long*>(d_slot + 2 * P);
  // 1. count pass: the receivers this shard owns are served in place, the remote ones counted per destination
  hipLaunchKernelGGL(k_push_shard_rows<0>, dim3(grid), dim3(kBlock), 0, s, a, sp, c.pa, trav);
  if (pieces) hipLaunchKernelGGL(k_push_shard_pieces<0>, dim3(kMaxGrid), dim3(kBlock), 0, s, a, sp, c.pa);
  PM_HIP_CHECK(hipGetLastError());
  // 2. every shard's counts (one host sync)
  c.comm->allgather(x, x + 192, uint64_t(G) * sizeof(unsigned long long), s);
  uint64_t* pin = pinned(c, uint64_t(G) * G);
  PM_HIP_CHECK(hipMemcpyAsync(pin, x + 192, uint64_t(G) * G * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PM_HIP_CHECK(hipStreamSynchronize(s));
  std::vector<uint64_t> sb(G), rb(G), cur(G);
  uint64_t nsend = 0, nrecv = 0;
  for (uint32_t g = 0; g < G; ++g) {
    const uint64_t to = pin[uint64_t(me) * G + g], from = pin[uint64_t(g) * G + me];
    cur[g] = nsend;
    sb[g] = to * kMsgWords * sizeof(uint32_t);
    rb[g] = from * kMsgWords * sizeof(uint32_t);
    nsend += to;
    nrecv += from;
  }
  auto* send = grow_to<uint32_t>(c.d_xsend, c.xsend_cap, std::max<uint64_t>(nsend, 1) * kMsgWords * sizeof(uint32_t));
  auto* recv = grow_to<uint32_t>(c.d_xrecv, c.xrecv_cap, std::max<uint64_t>(nrecv, 1) * kMsgWords * sizeof(uint32_t));
  // 3. scatter pass into the destinations' buckets
  if (nsend) {
    uint64_t* pc = pinned(c, G);  // (the counts above are consumed)
    for (uint32_t g = 0; g < G; ++g) pc[g] = cur[g];
    PM_HIP_CHECK(hipMemcpyAsync(x + 64, pc, G * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (pieces) PM_HIP_CHECK(hipMemsetAsync(a.npieces, 0, sizeof(unsigned long long), s));
    sp.out = send;
    sp.cap = nsend;
    hipLaunchKernelGGL(k_push_shard_rows<1>, dim3(grid), dim3(kBlock), 0, s, a, sp, c.pa, trav);
    if (pieces) hipLaunchKernelGGL(k_push_shard_pieces<1>, dim3(kMaxGrid), dim3(kBlock), 0, s, a, sp, c.pa);
    PM_HIP_CHECK(hipGetLastError());
    PM_HIP_CHECK(hipStreamSynchronize(s));  // (the pinned cursors are reused by the next read-back)
  }
  // 4. one all-to-all carries the messages; 5. the receivers
  c.comm->alltoallv(send, sb.data(), recv, rb.data(), s);
  if (nrecv) {
    hipLaunchKernelGGL(k_push_apply, dim3(grid_of(nrecv, kBlock, 16384)), dim3(kBlock), 0, s, a, c.pa, recv, nrecv,
                       c.n, reinterpret_cast<unsigned*>(x + 128));
    PM_HIP_CHECK(hipGetLastError());
    uint64_t* pb = pinned(c, 1);
    PM_HIP_CHECK(hipMemcpyAsync(pb, x + 128, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PM_HIP_CHECK(hipStreamSynchronize(s));
    if (pb[0]) throw std::runtime_error("sharded push superstep: a message names a position outside the graph");
  }
  c.push_msgs.push_back(nsend);
  // 6. the verify, unchanged, over this shard's rows
  launch_push_verify(c, av, d_slot);
}

}  // namespace pm
