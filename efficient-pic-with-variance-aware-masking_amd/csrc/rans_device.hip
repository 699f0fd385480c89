// The rANS coder on the device: rans_core.h's steps driven by one wave per stream.
//
// A stream is an (image, slice) pair of an NHWC int32 window; stream id = slice * B + image.  What is parallel: all
// streams of a launch, and inside a stream everything that does not depend on the coder state — addressing, the layer
// selection, the index / size / offset / start / frequency look-ups and the escape classification, staged 64 elements
// at a time, one per lane.  What is serial: the state update, which every lane of the wave carries redundantly (the
// values are wave-uniform), so a staged record is fetched with v_readlane and the decoder's symbol search is a wave-wide
// compare (one ballot per 64 table entries) instead of a scan.  One lane stores.  Plain C++ only.
//
// Lane-split streams turn that around: one thread per (stream, lane), see the second half.
//
// Layered launches: every kernel takes n_sel consecutive layer selectors sel .. sel + n_sel - 1 over the
// same window; stream id = (k * n_slices + slice) * B + image codes / decodes the elements of layer sel + k.  The
// single-selector entry points are n_sel = 1.
#include "common.h"
#include "rans_core.h"
#include <cstring>

using namespace vam;
namespace R = vam_rans;

namespace {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_get(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct Geometry {
  int B, h, w, ld, c0, C, n_slices;
  int n_sel;           // layer selectors of the launch; the level is the slowest dimension of the stream id
  __device__ int streams() const { return B * n_slices * n_sel; }
  __device__ long hw() const { return (long)h * w; }
  // Stream str = (level * n_slices + slice) * B + image: its level, and where its (image, slice) window begins.
  __device__ long origin(int str, int& lvl) const {
    const int per = B * n_slices;
    lvl = str / per;
    const int sid = str - lvl * per, s = sid / B, b = sid - s * B;
    return (long)b * hw() * ld + c0 + (long)s * C;
  }
};

// The arguments of the four kernels over a window; K is the lanes of a stream, which the wave-per-stream kernels ignore.
struct EncArgs {
  const int32_t* sym;
  const int32_t* idx;
  const uint8_t* layer;
  int sel;
  Geometry g;
  int K;
  vam_rans_tables t;
  uint32_t* out;
  long cap;
  int32_t* lengths;
  int32_t* status;
};

__global__ __launch_bounds__(kWave) void rans_encode_kernel(EncArgs a) {
  const int gid = blockIdx.x, lane = threadIdx.x;
  int lvl;
  const long img = a.g.origin(gid, lvl), hw = a.g.hw(), n = hw * a.g.C;
  const int sel = a.sel + lvl;
  const R::Nhwc at{hw, a.g.ld};
  uint32_t* region = a.out + (long)gid * a.cap;
  R::Enc e;
  R::enc_init(e, region, region + a.cap, lane == 0);
  int fail = 0;
  for (long base = (n - 1) / kWave * kWave; base >= 0 && n > 0; base -= kWave) {
    const long i = base + lane;
    R::Put u{0, 0, 0, -1};
    int st = 0;
    if (i < n) {                                      // staging: one element per lane
      const long o = img + at.off(i);
      const bool keep = !a.layer || a.layer[o] == sel;
      const int ci = keep ? (a.idx ? a.idx[o] : at.chan(i)) : 0;
      st = R::classify(keep ? a.sym[o] : 0, ci, a.t.cdf, a.t.stride, a.t.sizes, a.t.offsets, a.t.n_cdfs, u);
    }
    const unsigned long long bad = __ballot(st != 0);
    if (bad) {                                        // the element nearest the stream's end decides, as good as any
      fail = lane_get(st, 63 - __clzll(bad));
      break;
    }
    const int cnt = (int)(n - base < kWave ? n - base : kWave);
    for (int k = cnt - 1; k >= 0; --k) {              // serial: wave-uniform state, records by v_readlane
      const R::Put uk{(uint32_t)lane_get((int)u.start_freq, k), (uint32_t)lane_get((int)u.rcp, k),
                      (uint32_t)lane_get((int)u.raw, k), lane_get(u.n_bypass, k)};
      R::enc_element(e, uk);
    }
    fail = uniform(e.status);
    if (fail) break;
  }
  long words = 0;
  if (!fail) {
    words = R::enc_finish(e, region + a.cap);
    fail = uniform(e.status);
  }
  if (lane == 0) {
    a.lengths[gid] = fail ? 0 : (int32_t)words;
    a.status[gid] = fail;
  }
}

// offsets[s] = sum of lengths[0 .. s), offsets[n] = the total; stream s's tail words go to packed + offsets[s].  A scan in
// two levels, with offsets itself as the workspace: (1) every block of 256 regions scans its own lengths, offsets[i + 1] =
// the inclusive sum inside i's block, so offsets[256 (j + 1)] (offsets[n] for the last block) is block j's total; (2) one
// workgroup turns those totals into running sums in place, which is their final value; (3) region i adds its block's base
// offsets[i - i % 256] and copies.  Nothing in (3) writes an entry another workgroup of (3) reads: bases are multiples of 256.
constexpr int kPackBlock = 256;

__global__ __launch_bounds__(kPackBlock) void rans_pack_local_kernel(const int32_t* lengths, int n, int64_t* offsets) {
  __shared__ long part[kPackBlock];
  const int t = threadIdx.x, i = blockIdx.x * kPackBlock + t;
  part[t] = i < n ? lengths[i] : 0;
  __syncthreads();
  for (int d = 1; d < kPackBlock; d <<= 1) {
    const long add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  if (i < n) offsets[i + 1] = part[t];
  if (i == 0) offsets[0] = 0;
}

// Block totals -> running sums, in place.  Thread t takes the blocks [t * per, (t + 1) * per).
__global__ __launch_bounds__(kPackBlock) void rans_pack_blocks_kernel(int n, int64_t* offsets) {
  __shared__ long part[kPackBlock];
  const int t = threadIdx.x, n_blocks = (n + kPackBlock - 1) / kPackBlock, per = (n_blocks + kPackBlock - 1) / kPackBlock;
  const int j0 = t * per < n_blocks ? t * per : n_blocks, j1 = j0 + per < n_blocks ? j0 + per : n_blocks;
  auto total_at = [&](int j) -> long { const long e = (long)(j + 1) * kPackBlock; return e < n ? e : n; };
  long sum = 0;
  for (int j = j0; j < j1; ++j) sum += offsets[total_at(j)];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kPackBlock; d <<= 1) {
    const long add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long run = part[t] - sum;                                    // the total of every block before j0
  for (int j = j0; j < j1; ++j) {
    run += offsets[total_at(j)];
    offsets[total_at(j)] = run;
  }
}

__global__ __launch_bounds__(kPackBlock) void rans_pack_kernel(const uint32_t* regions, long cap, const int32_t* lengths, int n_streams,
                                                               uint32_t* packed, long packed_cap, int64_t* offsets) {
  const int sid = blockIdx.x, t = threadIdx.x, in_block = sid % kPackBlock;
  const long off = in_block ? offsets[sid - in_block] + offsets[sid] : offsets[sid], len = lengths[sid];
  __syncthreads();                                            // every thread has read offsets[sid] before it is replaced
  if (t == 0) {
    if (in_block) offsets[sid] = off;
    if (sid == n_streams - 1) offsets[n_streams] = off + (len > 0 ? len : 0);
  }
  if (len <= 0 || len > cap || off + len > packed_cap) return;
  const uint32_t* src = regions + (long)sid * cap + (cap - len);
  for (long j = t; j < len; j += kPackBlock) packed[off + j] = src[j];
}

// The decoder's symbol search across the wave: entries e[1 .. n_ent] of an increasing table, 64 at a time.  Above 64
// entries the lanes first sample every step-th one to find the bucket.  Returns what the host's linear scan returns.
template <class E>
struct WaveSearch {
  const E* e;          // e[0] = the table's first entry
  int sz;              // cdf_sizes of the table
  bool implied_last;   // packed tables: entry sz-1 is not stored, it is 65536
  __device__ int operator()(uint32_t cum, uint32_t& start, uint32_t& freq) const {
    const int lane = threadIdx.x & (kWave - 1);
    int lo = 0, len = implied_last ? sz - 2 : sz - 1;        // searchable entries e[1 + lo .. 1 + lo + len)
    while (len > kWave) {
      const int step = (len + kWave - 1) / kWave;
      const int pos = lo + (lane + 1) * step - 1;
      const bool le = pos < lo + len && (uint32_t)e[1 + pos] <= cum;
      const int full = __popcll(__ballot(le));                 // buckets that lie wholly at or below cum
      const int end = lo + len;
      lo += full * step;
      len = end - lo < step ? (end - lo > 0 ? end - lo : 0) : step;
    }
    const bool le = lane < len && (uint32_t)e[1 + lo + lane] <= cum;
    int s = lo + __popcll(__ballot(le));
    if (s > sz - 2) s = sz - 2;
    start = (uint32_t)e[s];
    freq = (implied_last && s == sz - 2 ? (1u << R::kPrecision) : (uint32_t)e[s + 1]) - start;
    return s;
  }
};

// The decode kernels' tables.  Packed: every thread of the workgroup (kThreads of them, also those with no stream) copies
// the ragged 16-bit tables into LDS, 16 bytes per thread and step, and waits at the barrier; the LDS copy is what returns.
// Otherwise the tables are read as int32 rows from global memory and nothing is copied.
template <bool kPacked, int kThreads>
__device__ __forceinline__ const uint16_t* stage_tables(const vam_rans_tables& t) {
  extern __shared__ uint4 lds_raw[];
  if (kPacked) {
    const uint4* src = reinterpret_cast<const uint4*>(t.packed);
    for (int j = threadIdx.x; j < t.packed_entries / 8; j += kThreads) lds_raw[j] = src[j];
    __syncthreads();
  }
  return reinterpret_cast<const uint16_t*>(lds_raw);
}

// The rows a thread of its own searches (rans_core.h's TableSearch): in the LDS copy, or in the int32 tables.
template <bool kPacked>
__device__ __forceinline__ auto table_rows(const uint16_t* tab, const vam_rans_tables& t) {
  if constexpr (kPacked) return R::PackedRows{tab, t.packed_start};
  else return R::Int32Rows{t.cdf, t.stride};
}

// Where a row begins for the wave-wide search: an offset into the LDS copy, or into the int32 tables.
template <bool kPacked>
struct RowStarts {
  const int32_t* starts;
  int stride;
  __device__ int operator()(int ci, int) const { return kPacked ? starts[ci] : ci * stride; }
  __device__ int none() const { return 0; }
};

// What a kernel stages per element: the row of T and the table's offset, read side by side so that neither load waits for
// the other.
template <class T>
struct Staged {
  T rows;
  const int32_t* offsets;
  struct Row {
    decltype(T{}(0, 2)) where;   // T's row: a TableSearch, or the row's start
    int offv;
  };
  __device__ Row operator()(int ci, int sz) const { return {rows(ci, sz), offsets[ci]}; }
  __device__ Row none() const { return {rows.none(), 0}; }
};
template <class T>
__device__ __forceinline__ Staged<T> staged(const T& rows, const vam_rans_tables& t) { return {rows, t.offsets}; }

// A stream's bytes lie inside the launch's: a whole-word offset and a length within [0, total].
__device__ __forceinline__ bool span_ok(int64_t boff, long len, long total) {
  return boff >= 0 && !(boff & 3) && len >= 0 && boff <= total && len <= total - boff;
}

struct DecArgs {
  const uint8_t* bytes;
  const int64_t* byte_offsets;
  const int32_t* byte_lengths;
  const int32_t* idx;
  const uint8_t* layer;
  int sel;
  Geometry g;
  int K;
  vam_rans_tables t;
  int32_t* out;
  int32_t* status;
};

// kWaves streams per workgroup, one wave each, share one LDS copy of the packed tables (the layered launches: 8 waves;
// the single-selector entry point: 1).  A wave whose stream id is past the end leaves after the barrier.
template <bool kPacked, int kWaves>
__global__ __launch_bounds__(kWave * kWaves) void rans_decode_kernel(DecArgs a) {
  const uint16_t* tab = stage_tables<kPacked, kWave * kWaves>(a.t);
  const int lane = threadIdx.x & (kWave - 1);
  const int gid = blockIdx.x * kWaves + uniform((int)threadIdx.x / kWave);
  if (gid >= a.g.streams()) return;
  int lvl;
  const long img = a.g.origin(gid, lvl), hw = a.g.hw(), n = hw * a.g.C;
  const int sel = a.sel + lvl;
  const R::Nhwc at{hw, a.g.ld};
  R::Dec d;
  const int64_t boff = a.byte_offsets[gid];
  R::dec_init(d, (boff & 3) ? nullptr : reinterpret_cast<const uint32_t*>(a.bytes + boff), a.byte_lengths[gid]);
  int fail = uniform(d.status);
  for (long base = 0; base < n; base += kWave) {
    const long i = base + lane;
    bool keep = false;
    long o = 0;
    int st = 0, sz = 2, offv = 0, t0 = 0;
    if (i < n) {                                              // staging: one element per lane
      o = img + at.off(i);
      keep = !a.layer || a.layer[o] == sel;
      const int ci = keep ? (a.idx ? a.idx[o] : at.chan(i)) : 0;
      const auto t = R::table_row(staged(RowStarts<kPacked>{a.t.packed_start, a.t.stride}, a.t), ci, a.t.stride, a.t.sizes, a.t.n_cdfs);
      st = t.status; sz = t.sz; t0 = t.row.where; offv = t.row.offv;
    }
    int32_t mine = 0;
    bool have = false;
    const int cnt = (int)(n - base < kWave ? n - base : kWave);
    for (int k = 0; k < cnt && !fail; ++k) {                  // serial: wave-uniform state, records by v_readlane
      fail = lane_get(st, k);
      if (fail) break;
      const int szk = lane_get(sz, k), tk = lane_get(t0, k);
      int32_t v;
      if (kPacked) v = R::dec_element(d, WaveSearch<uint16_t>{tab + tk, szk, true}, szk);
      else v = R::dec_element(d, WaveSearch<int32_t>{a.t.cdf + tk, szk, false}, szk);
      fail = uniform(d.status);
      if (fail) break;
      if (lane == k) { mine = v; have = true; }
    }
    if (keep) a.out[o] = have ? (int32_t)((uint32_t)mine + (uint32_t)offv) : 0;   // after a failure: zeros
  }
  if (lane == 0) a.status[gid] = fail;
}

// ---------------------------------------------------------------- lane-split streams
// One thread per (stream, lane): thread id = stream id * K + lane, so 64 / K streams share a wave and a wave is full for
// every K.  Nothing crosses a lane: each thread runs rans_core.h's lane_encode / lane_decode on its own state, its own
// words and its own elements (stream elements lane, lane + K, ...), and is its own writer.
__global__ __launch_bounds__(kWave) void rans_lanes_encode_kernel(EncArgs a) {
  const int gid = blockIdx.x * kWave + threadIdx.x;
  if (gid >= a.g.streams() * a.K) return;
  const int str = gid / a.K, lane = gid - str * a.K;
  int lvl;
  const long img = a.g.origin(str, lvl), hw = a.g.hw(), n = hw * a.g.C;
  long words = 0;
  const int32_t st = R::lane_encode(a.sym + img, a.idx ? a.idx + img : nullptr, a.layer ? a.layer + img : nullptr, a.sel + lvl, n,
                                    R::Nhwc{hw, a.g.ld}, a.K, lane, a.t.cdf, a.t.stride, a.t.sizes, a.t.offsets, a.t.n_cdfs,
                                    a.out + (long)gid * a.cap, a.cap, &words);
  a.lengths[gid] = st ? 0 : (int32_t)words;
  a.status[gid] = st;
}

// 256 threads share one LDS copy of the packed tables (54 KB for the Gaussian tables: two workgroups, eight waves, per
// CU); stage_tables has every thread of the workgroup copy, also those past the last lane.  The symbol search is a
// per-thread binary search (table_rows: rans_core.h's TableSearch) over the LDS copy, or over the int32 tables in global memory.
constexpr int kLaneBlock = 256;

template <bool kPacked>
__global__ __launch_bounds__(kLaneBlock) void rans_lanes_decode_kernel(DecArgs a) {
  const uint16_t* tab = stage_tables<kPacked, kLaneBlock>(a.t);
  const int gid = blockIdx.x * kLaneBlock + threadIdx.x;
  if (gid >= a.g.streams() * a.K) return;
  const int str = gid / a.K, lane = gid - str * a.K;
  int lvl;
  const long img = a.g.origin(str, lvl), hw = a.g.hw(), n = hw * a.g.C;
  const int64_t boff = a.byte_offsets[str];
  const uint32_t* words = (boff & 3) ? nullptr : reinterpret_cast<const uint32_t*>(a.bytes + boff);
  a.status[gid] = R::lane_decode(words, a.byte_lengths[str], a.K, lane, a.idx ? a.idx + img : nullptr, a.layer ? a.layer + img : nullptr,
                                 a.sel + lvl, n, R::Nhwc{hw, a.g.ld}, table_rows<kPacked>(tab, a.t), a.t.stride, a.t.sizes, a.t.offsets,
                                 a.t.n_cdfs, a.out + img);
}

// ---------------------------------------------------------------- interleaved lanes
// One thread per (stream, lane) as above, thread id = stream id * K + lane, but the K lanes of a stream share ONE word
// stream: in every round the lanes that flush (encode) or fetch (decode) are a ballot, a stream's K bits of it are cut out
// with the stream's first wave lane (StreamLanes), and a lane's word position is the stream's position plus the popcount of the
// flushing / fetching lanes above (encode: words are stored backwards) or below it (decode).  Every lane of a stream
// carries the stream's position itself, so nothing but the ballot crosses a lane.  All streams of a launch have the same
// n, so the group loop is wave-uniform; the rounds of a group run until no lane of the wave has a put / get left.
// No thread leaves early: a lane past the last stream stays, inactive, so that the wave stays converged at the ballots.
//
// Where a stream's elements lie is a base of the argument structs: FlatRows, the ranked buffers of the
// embedded streams, or NhwcWindow, the (image, slice) windows of the first half of this file, for z and the base slices
// of an "embedded-4" container.  What a window adds is compiled only for it (kWindow); the decoder's group step is one
// function, wave_group, for both forms and for the resume kernel.
struct FlatRows {                                            // stream s = elements [s * n, (s + 1) * n) in place, idx given
  static constexpr bool kWindow = false;
  __device__ long origin(int) const { return 0; }
  __device__ long off(long i) const { return i; }
  __device__ int chan(long) const { return 0; }
};
struct NhwcWindow {                                          // stream s * B + image = channels [c0 + s C, c0 + (s + 1) C) of an image
  static constexpr bool kWindow = true;
  int B, hw, ld, c0, C;
  __device__ long origin(int str) const {
    const int s = str / B, b = str - s * B;
    return (long)b * hw * ld + c0 + (long)s * C;
  }
  __device__ long off(long i) const {                        // n <= 2^28: 32-bit division
    const uint32_t c = (uint32_t)i / (uint32_t)hw;
    return (long)((uint32_t)i - c * (uint32_t)hw) * ld + c;
  }
  __device__ int chan(long i) const { return (int)((uint32_t)i / (uint32_t)hw); }
};

typedef unsigned long long u64;

// Thread gid of a launch as lane `lane` of stream `str`, and that stream's part of a wave ballot.
struct StreamLanes {
  int K, str, lane, shift;   // shift: the wave lane of the stream's lane 0
  u64 kmask, below, above;   // the stream's lanes; those below and above this one
  __device__ StreamLanes(int gid, int K_)
      : K(K_), str(gid / K_), lane(gid - str * K_), shift((int)(threadIdx.x & (kWave - 1)) - lane),
        kmask(K_ == kWave ? ~0ull : (1ull << K_) - 1), below((1ull << lane) - 1), above(kmask & ~((2ull << lane) - 1)) {}
  __device__ u64 mine(u64 ballot) const { return (ballot >> shift) & kmask; }
};

template <class A>
struct IlvEncArgs : A {
  const int32_t* sym;
  const int32_t* idx;
  int n_streams;
  long n;
  int K;
  vam_rans_tables t;
  uint32_t* out;
  long cap;
  int32_t* lengths;
  int32_t* status;
  const int32_t* counts;     // [n_marks][n_streams], non-decreasing in the mark
  int n_marks;
  int32_t* mark_bytes;       // [n_marks][n_streams]
};

template <class A>
__global__ __launch_bounds__(kWave) void rans_interleaved_encode_kernel(IlvEncArgs<A> a) {
  const StreamLanes L(blockIdx.x * kWave + threadIdx.x, a.K);
  const int K = L.K, str = L.str, lane = L.lane;
  const bool valid = str < a.n_streams;
  const long n = a.n, base = A::kWindow ? a.origin(valid ? str : 0) : (long)(valid ? str : 0) * n;
  uint32_t* region = a.out + (long)(valid ? str : 0) * a.cap;
  uint32_t* top = region + a.cap;                            // the stream's next word goes below top
  R::Enc e;
  R::enc_init(e, region, top);
  long emitted = 0;                                          // words of the stream so far
  int m_hi = valid ? a.n_marks : 0;                          // marks 0 .. m_hi - 1 have seen no flush of theirs yet
  long c_top = m_hi > 0 ? a.counts[(long)(m_hi - 1) * a.n_streams + str] : 0;
  int32_t st = 0;
  bool alive = valid;
  for (long g = (n + K - 1) / K - 1; g >= 0; --g) {
    const long i = g * K + lane;
    R::Put u{0, 0, 0, -1};
    int gets = 0;
    if (alive && i < n) {
      if constexpr (A::kWindow) {
        const long o = base + a.off(i);
        st = R::classify(a.sym[o], a.idx ? a.idx[o] : a.chan(i), a.t.cdf, a.t.stride, a.t.sizes, a.t.offsets, a.t.n_cdfs, u);
      } else {
        st = R::classify(a.sym[base + i], a.idx[base + i], a.t.cdf, a.t.stride, a.t.sizes, a.t.offsets, a.t.n_cdfs, u);
      }
      gets = st ? 0 : R::put_gets(u);
    }
    if (L.mine(__ballot(st != 0))) alive = false;
    if (!alive) gets = 0;
    for (int t = R::kMaxGets - 1; t >= 0; --t) {
      const bool act = gets > t;
      if (!__ballot(act)) continue;
      const bool fl = act && R::put_flushes(e, u, t);
      const u64 sub = L.mine(__ballot(fl));
      while (m_hi > 0 && sub) {                               // the first flush on behalf of an element below a mark's count
        const long c = c_top > 0 ? c_top : 0, gq = c / K;
        const u64 mine = g < gq ? sub : g == gq ? sub & ((1ull << (int)(c - gq * K)) - 1) : 0;
        if (!mine) break;
        const int hi = 63 - __clzll(mine);                    // descending lanes: the highest flushes first
        if (lane == 0) a.mark_bytes[(long)(m_hi - 1) * a.n_streams + str] = (int32_t)(emitted + __popcll(sub & ~((2ull << hi) - 1)));
        --m_hi;
        c_top = m_hi > 0 ? a.counts[(long)(m_hi - 1) * a.n_streams + str] : 0;
      }
      if (fl) e.p = top - __popcll(sub & L.above);            // enc_flush_word stores at --p
      if (act) R::enc_put_step(e, u, t);
      top -= __popcll(sub);
      emitted += __popcll(sub);
    }
    if (L.mine(__ballot(e.status != 0))) alive = false;
  }
  const int32_t own = st ? st : e.status;
  const u64 bad = L.mine(__ballot(own != 0));
  int32_t sst = __shfl(own, bad ? L.shift + __ffsll(bad) - 1 : L.shift);    // the stream's status: its lowest failing lane's
  if (!bad) sst = 0;
  long words = 0;
  if (valid && !sst) {
    if (top - region < 2l * K) sst = R::kOverflow;
    else {
      uint32_t* s = top - 2l * K;
      s[2 * lane] = (uint32_t)e.x;
      s[2 * lane + 1] = (uint32_t)(e.x >> 32);
      words = (long)(region + a.cap - s);
    }
  }
  if (valid && lane == 0) {
    a.lengths[str] = sst ? 0 : (int32_t)words;
    a.status[str] = sst;
    for (int m = 0; m < a.n_marks; ++m) {                     // words before the mark's first flush -> the prefix's bytes
      const long at = (long)m * a.n_streams + str;
      if (sst) a.mark_bytes[at] = 0;
      else if (m < m_hi) a.mark_bytes[at] = a.counts[at] > 0 ? 8 * K : 0;
      else a.mark_bytes[at] = (int32_t)(4 * (words - a.mark_bytes[at]));
    }
  }
}

// ---------------------------------------------------------------- cut table
// cut[s][c], 0 <= c <= n: vam_rans_interleaved_prefix_bytes of count c on the string the kernel above writes for stream s,
// for EVERY count, from one dry walk of the encoder: the same thread geometry, groups and rounds descending, the same
// ballots, but no word is stored, so there is no region and no overflow.  The decoder reads an element's LAST word where
// the encoder flushes for it FIRST; with e_i the stream's words before that flush in encoder order (+inf when element i
// never flushes) and `words` the string's length, the prefix that decodes c elements ends at 4 (words - min over i < c of
// e_i), or at 8 K when that minimum is +inf.  Inside a group a high lane may flush in a later round than a low one, hence
// a minimum and not "the last flushing element".
// Phase 1, the walk: every thread stores e_i (kNoFlush: none) into cut[s][i + 1] for its own elements i = g K + lane.
// Phase 2: the stream's lanes rewrite their row ascending, K entries at a time, with a prefix minimum over the stream's
// lanes and a carry.  A thread reads back only entries it stored itself, so nothing but shuffles and ballots crosses a
// lane and nothing leaves the wave.  A stream that ends with a status gets a row of zeros.  No thread leaves early.
constexpr int32_t kNoFlush = 0x7fffffff;

struct CutArgs {
  const int32_t* sym;
  const int32_t* idx;
  int n_streams;
  long n;
  int K;
  vam_rans_tables t;
  int32_t* cut;              // [n_streams][n + 1]
  int32_t* status;           // [n_streams]
};

__global__ __launch_bounds__(kWave) void rans_interleaved_cut_table_kernel(CutArgs a) {
  const StreamLanes L(blockIdx.x * kWave + threadIdx.x, a.K);
  const int K = L.K, str = L.str, lane = L.lane, wl = (int)(threadIdx.x & (kWave - 1));
  const bool valid = str < a.n_streams;
  const long n = a.n, base = (long)(valid ? str : 0) * n;
  int32_t* row = a.cut + (long)(valid ? str : 0) * (n + 1);
  R::Enc e;
  R::enc_init(e, nullptr, nullptr, false);                    // a dry run: the flush below is the state's half of enc_flush_word
  int32_t emitted = 0;                                        // words of the stream so far: at most 2 n <= 2^29
  int32_t st = 0;
  bool alive = valid;
  for (long g = (n + K - 1) / K - 1; g >= 0; --g) {
    const long i = g * K + lane;
    R::Put u{0, 0, 0, -1};
    int gets = 0;
    if (alive && i < n) {
      st = R::classify(a.sym[base + i], a.idx[base + i], a.t.cdf, a.t.stride, a.t.sizes, a.t.offsets, a.t.n_cdfs, u);
      gets = st ? 0 : R::put_gets(u);
    }
    if (L.mine(__ballot(st != 0))) alive = false;
    if (!alive) gets = 0;
    int32_t first = kNoFlush;                                 // e_i of this thread's element
    for (int t = R::kMaxGets - 1; t >= 0; --t) {
      const bool act = gets > t;
      if (!__ballot(act)) continue;
      const bool fl = act && R::put_flushes(e, u, t);
      const u64 sub = L.mine(__ballot(fl));
      if (fl) {
        if (first == kNoFlush) first = emitted + __popcll(sub & L.above);
        e.x >>= 32;                                           // after it no bound of enc_put / enc_put_bits is reached again
      }
      if (act) R::enc_put_step(e, u, t);
      emitted += __popcll(sub);
    }
    if (valid && i < n) row[i + 1] = first;
  }
  const u64 bad = L.mine(__ballot(st != 0));
  int32_t sst = __shfl(st, bad ? L.shift + __ffsll(bad) - 1 : L.shift);     // the stream's status: its lowest failing lane's
  if (!bad) sst = 0;
  const int32_t words = emitted + 2 * K;
  int32_t carry = kNoFlush;                                   // min of e_i over the groups below
  for (long g = 0; g * K < n; ++g) {
    const long i = g * K + lane;
    const bool has = valid && i < n;
    int32_t v = has && !sst ? row[i + 1] : kNoFlush;
    for (int d = 1; d < K; d <<= 1) {                         // inclusive prefix minimum over the stream's lanes
      const int32_t o = __shfl(v, lane >= d ? wl - d : wl);
      if (lane >= d && o < v) v = o;
    }
    if (carry < v) v = carry;
    carry = __shfl(v, L.shift + K - 1);                       // lanes past n hold kNoFlush: the last lane's is the group's
    if (has) row[i + 1] = sst ? 0 : v == kNoFlush ? 8 * K : 4 * (words - v);
  }
  if (valid && lane == 0) {
    row[0] = 0;
    a.status[str] = sst;
  }
}

template <class A>
struct IlvDecArgs : A {
  const uint8_t* bytes;
  long bytes_total;
  const int64_t* byte_offsets;
  const int32_t* byte_lengths;
  const int32_t* idx;
  int n_streams;
  long n;
  int K;
  vam_rans_tables t;
  int32_t* out;
  int32_t* available;
  int32_t* status;
};

// One group of the tolerant decode on the wave, the counterpart of rans_core.h's interleaved_group: a lane that `has` an
// element runs its gets on the staged row t (a refused row fails the lane at once) from the state in gt, and in every
// round the lanes that need a word take the stream's words from `pos` on in lane order.  The string's word p is
// words[p - first_word] and it holds the words below W; a request past them fails the lane.  The rounds are wave-uniform:
// every lane of the wave calls this together, the lanes without an element take no part but stay at the ballots.
// What comes back is the stream's: the lanes that failed and those that failed with a status (bits of the stream), the
// lowest failed lane (K when none) and the status of the lowest lane that has one.
struct GroupEnd {
  u64 fsub, esub;
  int first;
  int32_t err;
};

template <class S>
__device__ __forceinline__ GroupEnd wave_group(const StreamLanes& L, bool has, const R::TableRow<S>& t, R::Get& gt, long& pos,
                                               const uint32_t* words, long first_word, long W) {
  int32_t lst = t.status;                                     // what failed this lane, when it is an error
  bool failed = lst != 0, act = has && !failed;
  if (has) {
    gt.phase = R::kGetSymbol;
    gt.status = 0;
    gt.value = 0;
  }
  while (__ballot(act)) {                                     // one round: the updates, then the words in lane order
    bool need = false;
    if (act) {
      need = R::get_step(gt, t.row.where, t.sz);
      if (gt.status) { lst = gt.status; failed = true; need = false; }
    }
    const u64 sub = L.mine(__ballot(need));
    if (need) {
      const long p = pos + __popcll(sub & L.below);
      if (p < W) gt.x = (gt.x << 32) | words[p - first_word];
      else failed = true;                                     // past the words held: so is every later request
    }
    pos += __popcll(sub);
    if (failed || gt.phase == R::kGetDone) act = false;
  }
  const u64 fsub = L.mine(__ballot(failed)), esub = L.mine(__ballot(lst != 0));
  return {fsub, esub, fsub ? __ffsll(fsub) - 1 : L.K, __shfl(lst, esub ? L.shift + __ffsll(esub) - 1 : L.shift)};
}

// The flat form is tolerant (rans_core.h's interleaved_decode).  A window is decoded STRICTLY: the base of a container is
// needed whole.  A stream whose words end early gets kTruncated, its elements from the failing group on are written as 0,
// and a refused stream (kBadStream) is neither read nor written; there are no available counts.
template <bool kPacked, class A>
__global__ __launch_bounds__(kLaneBlock) void rans_interleaved_decode_kernel(IlvDecArgs<A> a) {
  const auto rows = staged(table_rows<kPacked>(stage_tables<kPacked, kLaneBlock>(a.t), a.t), a.t);
  const StreamLanes L(blockIdx.x * kLaneBlock + threadIdx.x, a.K);
  const int K = L.K, str = L.str, lane = L.lane;
  const bool valid = str < a.n_streams;
  const long n = a.n, base = A::kWindow ? a.origin(valid ? str : 0) : (long)(valid ? str : 0) * n;
  const uint32_t* words = nullptr;
  long W = 0;
  int32_t sst = 0;
  if (valid) {
    const int64_t boff = a.byte_offsets[str];
    const long len = a.byte_lengths[str];
    if (!span_ok(boff, len, a.bytes_total)) sst = R::kBadStream;
    else { words = reinterpret_cast<const uint32_t*>(a.bytes + boff); W = len / 4; }
  }
  bool alive = valid && !sst && W >= 2l * K;
  bool refused = false;
  if constexpr (A::kWindow) {
    refused = sst != 0;
    if (valid && !sst && !alive) sst = R::kTruncated;         // not even the states
  }
  long avail = alive ? n : 0, pos = 2l * K;
  R::Get gt{0, 0, 0, 0, 0, R::kGetDone, 0};
  if (alive) gt.x = (uint64_t)words[2 * lane] | ((uint64_t)words[2 * lane + 1] << 32);
  for (long g = 0; g * K < n; ++g) {
    const long i = g * K + lane;
    const bool has = valid && i < n, was_alive = alive;
    R::TableRow<decltype(rows.none())> t{R::kOk, 2, rows.none()};
    if (alive && has) {
      int ci;
      if constexpr (A::kWindow) ci = a.idx ? a.idx[base + a.off(i)] : a.chan(i);
      else ci = a.idx[base + i];
      t = R::table_row(rows, ci, a.t.stride, a.t.sizes, a.t.n_cdfs);
    }
    const GroupEnd e = wave_group(L, alive && has, t, gt, pos, words, 0, W);
    if constexpr (A::kWindow) {                               // strict: a failing group is zeros as a whole
      if (has && !refused) a.out[base + a.off(i)] = was_alive && !e.fsub ? (int32_t)((uint32_t)gt.value + (uint32_t)t.row.offv) : 0;
    } else {
      if (has) a.out[base + i] = was_alive && lane < e.first ? (int32_t)((uint32_t)gt.value + (uint32_t)t.row.offv) : 0;
    }
    if (was_alive && e.fsub) {
      alive = false;
      avail = g * K + e.first;
      if constexpr (A::kWindow) sst = e.esub ? e.err : (int32_t)R::kTruncated;
      else sst = e.esub ? e.err : 0;
    }
  }
  if (valid && lane == 0) {
    if constexpr (!A::kWindow) a.available[str] = (int32_t)avail;
    a.status[str] = sst;
  }
}

// ---------------------------------------------------------------- resumable decode
// The flat decode from a checkpoint (rans_core.h's interleaved_resume): the same geometry and, through wave_group, the same
// group step as the kernel above, with a policy of its own around it.  The streams of a launch stand at
// different groups, so every stream counts its own group g and the loop runs while any stream of the wave still decodes:
// that test is a ballot, wave-uniform, and so are the rounds inside, where the lanes of a stream that has ended take no
// part.  A wave therefore leaves after the groups its bytes reach, not after n / K.  Every lane carries the state and the
// word position it had when the current group began; they are what a failing group leaves as the checkpoint.
struct IlvResArgs {
  const uint8_t* bytes;
  long bytes_total;
  const int64_t* byte_offsets;
  const int32_t* byte_lengths;
  const int32_t* idx;
  int n_streams;
  long n;
  int K;
  vam_rans_tables t;
  int32_t* out;
  uint64_t* states;          // [n_streams][K]
  int32_t* done;             // [n_streams]
  int32_t* pos;              // [n_streams]: the uploaded bytes of stream s begin at the string's word pos[s]
  int32_t* available;
  int32_t* status;
};

template <bool kPacked>
__global__ __launch_bounds__(kLaneBlock) void rans_interleaved_resume_kernel(IlvResArgs a) {
  const auto rows = staged(table_rows<kPacked>(stage_tables<kPacked, kLaneBlock>(a.t), a.t), a.t);
  const StreamLanes L(blockIdx.x * kLaneBlock + threadIdx.x, a.K);
  const int K = L.K, str = L.str, lane = L.lane;
  const bool valid = str < a.n_streams;
  const long n = a.n, base = (long)(valid ? str : 0) * n;
  const uint32_t* words = nullptr;                            // the string's word p is words[p - first_word]
  long W = 0, pos = 0, first_word = 0, g = 0;
  int32_t sst = 0;
  bool alive = false;
  long avail = 0;
  R::Get gt{0, 0, 0, 0, 0, R::kGetDone, 0};
  if (valid) {
    const int64_t boff = a.byte_offsets[str];
    const long len = a.byte_lengths[str], done = a.done[str];
    pos = a.pos[str];
    if (!span_ok(boff, len, a.bytes_total) || !R::checkpoint_valid(done, pos, n, K)) sst = R::kBadStream;
    else if (done == n) avail = n;                            // finished: nothing is read or written
    else {
      words = reinterpret_cast<const uint32_t*>(a.bytes + boff);
      first_word = pos;
      W = pos + len / 4;
      g = done / K;
      if (done == 0 && pos == 0) {                            // fresh: the states stand in front of the string
        if (W >= 2l * K) {
          alive = true;
          gt.x = (uint64_t)words[2 * lane] | ((uint64_t)words[2 * lane + 1] << 32);
          pos = 2l * K;
        }
      } else {
        alive = true;
        gt.x = a.states[(long)str * K + lane];
      }
    }
  }
  const bool ran = alive;
  uint64_t ck_x = gt.x;                                       // the checkpoint this lane will leave
  long ck_pos = pos, ck_done = 0;
  while (__ballot(alive)) {
    const long i = g * K + lane;
    const bool has = alive && i < n;
    if (alive) { ck_x = gt.x; ck_pos = pos; ck_done = g * K; }
    R::TableRow<decltype(rows.none())> t{R::kOk, 2, rows.none()};
    if (has) t = R::table_row(rows, a.idx[base + i], a.t.stride, a.t.sizes, a.t.n_cdfs);
    const GroupEnd e = wave_group(L, has, t, gt, pos, words, first_word, W);
    if (has && lane < e.first) a.out[base + i] = (int32_t)((uint32_t)gt.value + (uint32_t)t.row.offv);
    if (alive) {
      if (e.fsub) {                                           // the group failed: its start is the checkpoint
        alive = false;
        avail = g * K + e.first;
        sst = e.esub ? e.err : 0;
      } else if ((++g) * K >= n) {                            // the stream is complete
        alive = false;
        avail = n;
        ck_x = gt.x; ck_pos = pos; ck_done = n;
      }
    }
  }
  if (ran) {
    a.states[(long)str * K + lane] = ck_x;
    if (lane == 0) {
      a.done[str] = (int32_t)ck_done;
      a.pos[str] = (int32_t)ck_pos;
    }
  }
  if (valid && lane == 0) {
    a.available[str] = (int32_t)avail;
    a.status[str] = sst;
  }
}

int check_geometry(const char* what, int B, int h, int w, int ld, int c0, int C, int n_slices, int n_sel = 1) {
  VAM_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0 && n_slices > 0 && c0 >= 0, "%s: B, h, w, C, n_slices must be > 0 and c0 >= 0", what);
  VAM_REQUIRE((long)c0 + (long)C * n_slices <= ld, "%s: window [%d, %ld) does not fit ld = %d", what, c0, (long)c0 + (long)C * n_slices, ld);
  VAM_REQUIRE(n_sel > 0, "%s: n_sel must be > 0, got %d", what, n_sel);
  VAM_REQUIRE((long)h * w * C <= (1l << 28) && (long)n_sel * B * n_slices <= (1l << 20), "%s: stream of %ld symbols or %ld streams is too large",
              what, (long)h * w * C, (long)n_sel * B * n_slices);
  return VAM_OK;
}

int check_tables(const char* what, const vam_rans_tables* t) {
  VAM_REQUIRE(t && t->cdf && t->sizes && t->offsets && t->n_cdfs > 0 && t->stride >= 2, "%s: tables need cdf, sizes, offsets, n_cdfs > 0, stride >= 2", what);
  VAM_REQUIRE((long)t->n_cdfs * t->stride < (1l << 31), "%s: tables too large", what);
  VAM_REQUIRE(!t->packed || (t->packed_start && t->packed_entries > 0 && t->packed_entries % 8 == 0),
              "%s: packed tables need their start offsets and a multiple of 8 entries", what);
  return VAM_OK;
}

const char* status_text(int st) {
  switch (st) {
    case R::kTruncated: return "bitstream truncated";
    case R::kBadIndex: return "index out of range";
    case R::kBadTable: return "cdf size invalid";
    case R::kOverflow: return "output buffer too small";
    case R::kZeroFreq: return "zero-frequency symbol (cdf table not normalised)";
    case R::kBadStream: return "bad arguments (a stream is at least 8 bytes, in whole words)";
    default: return "unknown status";
  }
}

template <class A>
long core_encode(const char* what, const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at,
                 const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out,
                 long out_cap) {
  std::vector<uint32_t> region((size_t)(2 * n + 16));       // 8 n + 64 bytes, the host coder's budget
  long words = 0;
  const int32_t st = R::encode_stream(sym, idx, layer, sel, n, at, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, region.data(),
                                      (long)region.size(), &words);
  VAM_REQUIRE(st == 0, "%s: %s", what, status_text(st));
  VAM_REQUIRE(words * 4 <= out_cap, "%s: output buffer too small (%ld > %ld)", what, words * 4, out_cap);
  std::memcpy(out, region.data() + region.size() - words, (size_t)words * 4);
  return words * 4;
}

template <class A>
int core_decode(const uint8_t* in, long n_bytes, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at,
                const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* out) {
  std::vector<uint32_t> words((size_t)(n_bytes / 4));       // aligned copy of the whole words
  if (!words.empty()) std::memcpy(words.data(), in, words.size() * 4);
  return R::decode_stream(words.empty() ? nullptr : words.data(), n_bytes, idx, layer, sel, n, at, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out);
}

template <class A>
long core_lanes_encode(const char* what, const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at,
                       int K, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs,
                       uint8_t* out, long out_cap, int32_t* lane_status) {
  VAM_REQUIRE(R::lanes_valid(K), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, K);
  const long cap = R::lane_cap_words(n, K);
  std::vector<uint32_t> regions((size_t)(cap * K));
  long words[R::kMaxLanes];
  int32_t status[R::kMaxLanes];
  const int32_t st = R::lanes_encode_stream(sym, idx, layer, sel, n, at, K, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, regions.data(),
                                            cap, words, status);
  if (lane_status) std::memcpy(lane_status, status, sizeof(int32_t) * (size_t)K);
  if (st) {
    int bad = 0;
    while (!status[bad]) ++bad;
    VAM_REQUIRE(false, "%s: lane %d: %s", what, bad, status_text(st));
  }
  long total = K > 1 ? K : 0;                                // K == 1: the stream itself, no header
  for (int j = 0; j < K; ++j) total += words[j];
  VAM_REQUIRE(total * 4 <= out_cap, "%s: output buffer too small (%ld > %ld)", what, total * 4, out_cap);
  uint8_t* p = out;
  if (K > 1)
    for (int j = 0; j < K; ++j, p += 4) {
      const uint32_t len = (uint32_t)words[j];
      std::memcpy(p, &len, 4);
    }
  for (int j = 0; j < K; p += words[j] * 4, ++j)
    std::memcpy(p, regions.data() + (size_t)(j + 1) * cap - words[j], (size_t)words[j] * 4);
  return total * 4;
}

template <class A>
int core_lanes_decode(const char* what, const uint8_t* in, long n_bytes, int K, const int32_t* idx, const uint8_t* layer, int sel,
                      long n, const A& at, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                      int n_cdfs, int32_t* out, int32_t* lane_status) {
  VAM_REQUIRE(R::lanes_valid(K), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, K);
  std::vector<uint32_t> words((size_t)(n_bytes / 4));       // aligned copy of the whole words
  if (!words.empty()) std::memcpy(words.data(), in, words.size() * 4);
  int32_t status[R::kMaxLanes];
  const int32_t st = R::lanes_decode_stream(words.empty() ? nullptr : words.data(), n_bytes, K, idx, layer, sel, n, at, cdfs, cdf_stride,
                                            cdf_sizes, offsets, n_cdfs, out, status);
  if (lane_status) std::memcpy(lane_status, status, sizeof(int32_t) * (size_t)K);
  return st;
}

// ---------------------------------------------------------------- launches, shared by the single-selector and the layered entry points
int launch_encode(const char* what, const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int n_sel, int B, int h, int w,
                  int ld, int c0, int C, int n_slices, const vam_rans_tables* tables, uint32_t* out_words, long out_cap_words,
                  int32_t* lengths, int32_t* status, void* stream) {
  VAM_REQUIRE(sym && out_words && lengths && status, "%s: need sym, out_words, lengths, status", what);
  if (int rc = check_geometry(what, B, h, w, ld, c0, C, n_slices, n_sel)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  VAM_REQUIRE(out_cap_words >= 2 && out_cap_words < (1l << 31), "%s: a region is 2 .. 2^31 words, got %ld", what, out_cap_words);
  EncArgs a{sym, idx, layer, sel, {B, h, w, ld, c0, C, n_slices, n_sel}, 1, *tables, out_words, out_cap_words, lengths, status};
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  hipLaunchKernelGGL(rans_encode_kernel, dim3(n_sel * B * n_slices), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch("rans_encode_kernel");
}

// The launch of a decode kernel: its <true> form with the packed tables a.t in LDS (refused when a workgroup may not have
// that much), its <false> form over the int32 tables otherwise.  `kernel` is the name a failed launch is reported under.
template <class Args>
int launch_with_tables(const char* what, const char* kernel, void (*packed)(Args), void (*plain)(Args), int blocks, int threads,
                       const Args& a, void* stream) {
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  if (a.t.packed) {
    const int lds = a.t.packed_entries * 2;
    const int limit = vam_rans_lds_table_bytes();
    if (limit < 0) return limit;
    VAM_REQUIRE(lds <= limit, "%s: packed tables of %d bytes exceed the %d bytes of LDS a workgroup may use", what, lds, limit);
    VAM_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(packed), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(packed, dim3(blocks), dim3(threads), lds, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(plain, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, a);
  }
  return check_launch(kernel);
}

template <int kWaves>
int launch_decode(const char* what, const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                  const uint8_t* layer, int sel, int n_sel, int B, int h, int w, int ld, int c0, int C, int n_slices,
                  const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream) {
  VAM_REQUIRE(bytes && byte_offsets && byte_lengths && sym_out && status, "%s: need bytes, offsets, lengths, sym_out, status", what);
  if (int rc = check_geometry(what, B, h, w, ld, c0, C, n_slices, n_sel)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  DecArgs a{bytes, byte_offsets, byte_lengths, idx, layer, sel, {B, h, w, ld, c0, C, n_slices, n_sel}, 1, *tables, sym_out, status};
  return launch_with_tables(what, "rans_decode_kernel", rans_decode_kernel<true, kWaves>, rans_decode_kernel<false, kWaves>,
                            (n_sel * B * n_slices + kWaves - 1) / kWaves, kWave * kWaves, a, stream);
}

int launch_lanes_encode(const char* what, const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int n_sel, int B, int h,
                        int w, int ld, int c0, int C, int n_slices, int lanes, const vam_rans_tables* tables, uint32_t* out_words,
                        long out_cap_words, int32_t* lengths, int32_t* status, void* stream) {
  VAM_REQUIRE(sym && out_words && lengths && status, "%s: need sym, out_words, lengths, status", what);
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  if (int rc = check_geometry(what, B, h, w, ld, c0, C, n_slices, n_sel)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  VAM_REQUIRE(out_cap_words >= 2 && out_cap_words < (1l << 31), "%s: a region is 2 .. 2^31 words, got %ld", what, out_cap_words);
  EncArgs a{sym, idx, layer, sel, {B, h, w, ld, c0, C, n_slices, n_sel}, lanes, *tables, out_words, out_cap_words, lengths, status};
  const int threads = n_sel * B * n_slices * lanes;         // at most 2^20 streams of 64 lanes
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  hipLaunchKernelGGL(rans_lanes_encode_kernel, dim3((threads + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch("rans_lanes_encode_kernel");
}

int launch_lanes_decode(const char* what, const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                        const uint8_t* layer, int sel, int n_sel, int B, int h, int w, int ld, int c0, int C, int n_slices, int lanes,
                        const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream) {
  VAM_REQUIRE(bytes && byte_offsets && byte_lengths && sym_out && status, "%s: need bytes, offsets, lengths, sym_out, status", what);
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  if (int rc = check_geometry(what, B, h, w, ld, c0, C, n_slices, n_sel)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  DecArgs a{bytes, byte_offsets, byte_lengths, idx, layer, sel, {B, h, w, ld, c0, C, n_slices, n_sel}, lanes, *tables, sym_out, status};
  return launch_with_tables(what, "rans_lanes_decode_kernel", rans_lanes_decode_kernel<true>, rans_lanes_decode_kernel<false>,
                            (n_sel * B * n_slices * lanes + kLaneBlock - 1) / kLaneBlock, kLaneBlock, a, stream);
}

// The layered launches select by layer id: a uint8, so the selectors stay within 0 .. 255.
int check_layers(const char* what, const uint8_t* layer, int sel0, int n_sel) {
  VAM_REQUIRE(layer, "%s: need the layer ids", what);
  VAM_REQUIRE(sel0 >= 0 && n_sel > 0 && (long)sel0 + n_sel <= 256, "%s: selectors [%d, %ld) outside the layer ids 0 .. 255", what, sel0,
              (long)sel0 + n_sel);
  return VAM_OK;
}

constexpr int kLayerWaves = 8;       // streams per workgroup of the layered K = 1 decode

template <class A>
int launch_interleaved_decode(const char* what, const IlvDecArgs<A>& a, void* stream) {
  return launch_with_tables(what, "rans_interleaved_decode_kernel", rans_interleaved_decode_kernel<true, A>,
                            rans_interleaved_decode_kernel<false, A>, (a.n_streams * a.K + kLaneBlock - 1) / kLaneBlock, kLaneBlock, a, stream);
}

// What the flat interleaved entry points refuse alike: the lanes of a stream, and the streams and symbols of a launch.
int check_streams(const char* what, int lanes, int n_streams, long n) {
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  VAM_REQUIRE(n_streams > 0 && n_streams <= (1 << 20) && n >= 0 && n <= (1l << 28), "%s: 1 .. 2^20 streams of 0 .. 2^28 symbols, got %d of %ld",
              what, n_streams, n);
  return VAM_OK;
}

}  // namespace

extern "C" {

long vam_rans_core_encode(const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                          const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long out_cap,
                          const uint8_t* layer, int sel) {
  VAM_REQUIRE(symbols && indexes && cdfs && cdf_sizes && offsets && out && n >= 0 && n <= (1l << 28) && n_cdfs >= 1,
              "vam_rans_core_encode: bad arguments");
  return core_encode("vam_rans_core_encode", symbols, indexes, layer, sel, n, R::Flat{}, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                     out, out_cap);
}

int vam_rans_core_decode(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                         const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* out, const uint8_t* layer, int sel) {
  VAM_REQUIRE((in || n_bytes == 0) && indexes && cdfs && cdf_sizes && offsets && out && n >= 0 && n_bytes >= 0 && n_cdfs >= 1,
              "vam_rans_core_decode: bad arguments");
  return core_decode(in, n_bytes, indexes, layer, sel, n, R::Flat{}, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out);
}

long vam_rans_core_encode_nhwc(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int image, int h, int w, int ld,
                               int c0, int C, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                               int n_cdfs, uint8_t* out, long out_cap) {
  VAM_REQUIRE(sym && cdfs && cdf_sizes && offsets && out && n_cdfs >= 1 && image >= 0, "vam_rans_core_encode_nhwc: bad arguments");
  if (int rc = check_geometry("vam_rans_core_encode_nhwc", 1, h, w, ld, c0, C, 1)) return rc;
  const long hw = (long)h * w, img = (long)image * hw * ld + c0;
  return core_encode("vam_rans_core_encode_nhwc", sym + img, idx ? idx + img : nullptr, layer ? layer + img : nullptr, sel, hw * C,
                     R::Nhwc{hw, ld}, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out, out_cap);
}

int vam_rans_core_decode_nhwc(const uint8_t* in, long n_bytes, const int32_t* idx, const uint8_t* layer, int sel, int image, int h,
                              int w, int ld, int c0, int C, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                              const int32_t* offsets, int n_cdfs, int32_t* sym_out) {
  VAM_REQUIRE((in || n_bytes == 0) && cdfs && cdf_sizes && offsets && sym_out && n_bytes >= 0 && n_cdfs >= 1 && image >= 0,
              "vam_rans_core_decode_nhwc: bad arguments");
  if (int rc = check_geometry("vam_rans_core_decode_nhwc", 1, h, w, ld, c0, C, 1)) return rc;
  const long hw = (long)h * w, img = (long)image * hw * ld + c0;
  return core_decode(in, n_bytes, idx ? idx + img : nullptr, layer ? layer + img : nullptr, sel, hw * C, R::Nhwc{hw, ld}, cdfs,
                     cdf_stride, cdf_sizes, offsets, n_cdfs, sym_out + img);
}

int vam_rans_encode_device(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int B, int h, int w, int ld, int c0,
                           int C, int n_slices, const vam_rans_tables* tables, uint32_t* out_words, long out_cap_words,
                           int32_t* lengths, int32_t* status, void* stream) {
  return launch_encode("vam_rans_encode_device", sym, idx, layer, sel, 1, B, h, w, ld, c0, C, n_slices, tables, out_words, out_cap_words,
                       lengths, status, stream);
}

int vam_rans_pack_device(const uint32_t* regions, long cap_words, const int32_t* lengths, int n_streams, uint32_t* packed,
                         long packed_cap_words, int64_t* offsets, void* stream) {
  VAM_REQUIRE(regions && lengths && packed && offsets && n_streams > 0 && cap_words >= 2 && packed_cap_words >= 0,
              "vam_rans_pack_device: bad arguments");
  const int n_blocks = (n_streams + kPackBlock - 1) / kPackBlock;
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  hipLaunchKernelGGL(rans_pack_local_kernel, dim3(n_blocks), dim3(kPackBlock), 0, (hipStream_t)stream, lengths, n_streams, offsets);
  if (n_blocks > 1)
    hipLaunchKernelGGL(rans_pack_blocks_kernel, dim3(1), dim3(kPackBlock), 0, (hipStream_t)stream, n_streams, offsets);
  hipLaunchKernelGGL(rans_pack_kernel, dim3(n_streams), dim3(kPackBlock), 0, (hipStream_t)stream, regions, cap_words, lengths, n_streams,
                     packed, packed_cap_words, offsets);
  return check_launch("rans_pack_kernel");
}

int vam_rans_lds_table_bytes(void) {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) {
    set_error("vam_rans_lds_table_bytes: no HIP device");
    return VAM_ENOGPU;
  }
  return v;
}

int vam_rans_decode_device(const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                           const uint8_t* layer, int sel, int B, int h, int w, int ld, int c0, int C, int n_slices,
                           const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream) {
  return launch_decode<1>("vam_rans_decode_device", bytes, byte_offsets, byte_lengths, idx, layer, sel, 1, B, h, w, ld, c0, C, n_slices,
                          tables, sym_out, status, stream);
}

long vam_rans_lanes_encode(const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                           const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long out_cap,
                           const uint8_t* layer, int sel, int lanes, int32_t* lane_status) {
  VAM_REQUIRE(symbols && indexes && cdfs && cdf_sizes && offsets && out && n >= 0 && n <= (1l << 28) && n_cdfs >= 1,
              "vam_rans_lanes_encode: bad arguments");
  return core_lanes_encode("vam_rans_lanes_encode", symbols, indexes, layer, sel, n, R::Flat{}, lanes, cdfs, cdf_stride, cdf_sizes,
                           offsets, n_cdfs, out, out_cap, lane_status);
}

int vam_rans_lanes_decode(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                          const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* out, const uint8_t* layer, int sel,
                          int lanes, int32_t* lane_status) {
  VAM_REQUIRE((in || n_bytes == 0) && indexes && cdfs && cdf_sizes && offsets && out && n >= 0 && n_bytes >= 0 && n_cdfs >= 1,
              "vam_rans_lanes_decode: bad arguments");
  return core_lanes_decode("vam_rans_lanes_decode", in, n_bytes, lanes, indexes, layer, sel, n, R::Flat{}, cdfs, cdf_stride, cdf_sizes,
                           offsets, n_cdfs, out, lane_status);
}

long vam_rans_lanes_encode_nhwc(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int image, int h, int w, int ld,
                                int c0, int C, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                int n_cdfs, uint8_t* out, long out_cap, int lanes, int32_t* lane_status) {
  VAM_REQUIRE(sym && cdfs && cdf_sizes && offsets && out && n_cdfs >= 1 && image >= 0, "vam_rans_lanes_encode_nhwc: bad arguments");
  if (int rc = check_geometry("vam_rans_lanes_encode_nhwc", 1, h, w, ld, c0, C, 1)) return rc;
  const long hw = (long)h * w, img = (long)image * hw * ld + c0;
  return core_lanes_encode("vam_rans_lanes_encode_nhwc", sym + img, idx ? idx + img : nullptr, layer ? layer + img : nullptr, sel,
                           hw * C, R::Nhwc{hw, ld}, lanes, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out, out_cap, lane_status);
}

int vam_rans_lanes_decode_nhwc(const uint8_t* in, long n_bytes, const int32_t* idx, const uint8_t* layer, int sel, int image, int h,
                               int w, int ld, int c0, int C, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                               const int32_t* offsets, int n_cdfs, int32_t* sym_out, int lanes, int32_t* lane_status) {
  VAM_REQUIRE((in || n_bytes == 0) && cdfs && cdf_sizes && offsets && sym_out && n_bytes >= 0 && n_cdfs >= 1 && image >= 0,
              "vam_rans_lanes_decode_nhwc: bad arguments");
  if (int rc = check_geometry("vam_rans_lanes_decode_nhwc", 1, h, w, ld, c0, C, 1)) return rc;
  const long hw = (long)h * w, img = (long)image * hw * ld + c0;
  return core_lanes_decode("vam_rans_lanes_decode_nhwc", in, n_bytes, lanes, idx ? idx + img : nullptr, layer ? layer + img : nullptr,
                           sel, hw * C, R::Nhwc{hw, ld}, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, sym_out + img, lane_status);
}

int vam_rans_lanes_encode_device(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, int B, int h, int w, int ld,
                                 int c0, int C, int n_slices, int lanes, const vam_rans_tables* tables, uint32_t* out_words,
                                 long out_cap_words, int32_t* lengths, int32_t* status, void* stream) {
  return launch_lanes_encode("vam_rans_lanes_encode_device", sym, idx, layer, sel, 1, B, h, w, ld, c0, C, n_slices, lanes, tables, out_words,
                             out_cap_words, lengths, status, stream);
}

int vam_rans_lanes_decode_device(const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                                 const uint8_t* layer, int sel, int B, int h, int w, int ld, int c0, int C, int n_slices, int lanes,
                                 const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream) {
  return launch_lanes_decode("vam_rans_lanes_decode_device", bytes, byte_offsets, byte_lengths, idx, layer, sel, 1, B, h, w, ld, c0, C,
                             n_slices, lanes, tables, sym_out, status, stream);
}

// ---------------------------------------------------------------- layered launches
int vam_rans_layers_encode_device(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel0, int n_sel, int B, int h, int w,
                                  int ld, int c0, int C, int n_slices, int lanes, const vam_rans_tables* tables, uint32_t* out_words,
                                  long out_cap_words, int32_t* lengths, int32_t* status, void* stream) {
  const char* what = "vam_rans_layers_encode_device";
  if (int rc = check_layers(what, layer, sel0, n_sel)) return rc;
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  if (lanes == 1)
    return launch_encode(what, sym, idx, layer, sel0, n_sel, B, h, w, ld, c0, C, n_slices, tables, out_words, out_cap_words, lengths, status,
                         stream);
  return launch_lanes_encode(what, sym, idx, layer, sel0, n_sel, B, h, w, ld, c0, C, n_slices, lanes, tables, out_words, out_cap_words,
                             lengths, status, stream);
}

int vam_rans_layers_decode_device(const uint8_t* bytes, const int64_t* byte_offsets, const int32_t* byte_lengths, const int32_t* idx,
                                  const uint8_t* layer, int sel0, int n_sel, int B, int h, int w, int ld, int c0, int C, int n_slices,
                                  int lanes, const vam_rans_tables* tables, int32_t* sym_out, int32_t* status, void* stream) {
  const char* what = "vam_rans_layers_decode_device";
  if (int rc = check_layers(what, layer, sel0, n_sel)) return rc;
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  if (lanes == 1)
    return launch_decode<kLayerWaves>(what, bytes, byte_offsets, byte_lengths, idx, layer, sel0, n_sel, B, h, w, ld, c0, C, n_slices, tables,
                                      sym_out, status, stream);
  return launch_lanes_decode(what, bytes, byte_offsets, byte_lengths, idx, layer, sel0, n_sel, B, h, w, ld, c0, C, n_slices, lanes, tables,
                             sym_out, status, stream);
}

// ---------------------------------------------------------------- interleaved lanes
int vam_rans_interleaved_encode_device(const int32_t* sym, const int32_t* idx, int n_streams, long n, int lanes,
                                       const vam_rans_tables* tables, uint32_t* out_words, long out_cap_words, int32_t* lengths,
                                       int32_t* status, const int32_t* counts, int n_marks, int32_t* mark_bytes, void* stream) {
  const char* what = "vam_rans_interleaved_encode_device";
  VAM_REQUIRE(sym && idx && out_words && lengths && status, "%s: need sym, idx, out_words, lengths, status", what);
  if (int rc = check_streams(what, lanes, n_streams, n)) return rc;
  VAM_REQUIRE(n_marks >= 0 && n_marks <= 4096 && (n_marks == 0 || (counts && mark_bytes)), "%s: marks need counts and mark_bytes", what);
  if (int rc = check_tables(what, tables)) return rc;
  VAM_REQUIRE(out_cap_words >= 2l * lanes && out_cap_words < (1l << 31), "%s: a region is 2 * lanes .. 2^31 words, got %ld", what,
              out_cap_words);
  IlvEncArgs<FlatRows> a{{}, sym, idx, n_streams, n, lanes, *tables, out_words, out_cap_words, lengths, status, counts, n_marks, mark_bytes};
  const int threads = n_streams * lanes;
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  hipLaunchKernelGGL(rans_interleaved_encode_kernel<FlatRows>, dim3((threads + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch("rans_interleaved_encode_kernel");
}

int vam_rans_interleaved_cut_table_device(const int32_t* sym, const int32_t* idx, int n_streams, long n, int lanes,
                                          const vam_rans_tables* tables, int32_t* cut, int32_t* status, void* stream) {
  const char* what = "vam_rans_interleaved_cut_table_device";
  VAM_REQUIRE(sym && idx && cut && status, "%s: need sym, idx, cut, status", what);
  VAM_REQUIRE(n >= 1, "%s: a row has n + 1 >= 2 entries, got n = %ld", what, n);
  if (int rc = check_streams(what, lanes, n_streams, n)) return rc;      // n <= 2^28: n + 1 and every entry fit an int32
  if (int rc = check_tables(what, tables)) return rc;
  CutArgs a{sym, idx, n_streams, n, lanes, *tables, cut, status};
  const int threads = n_streams * lanes;
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  hipLaunchKernelGGL(rans_interleaved_cut_table_kernel, dim3((threads + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch("rans_interleaved_cut_table_kernel");
}

int vam_rans_interleaved_decode_device(const uint8_t* bytes, long bytes_total, const int64_t* byte_offsets,
                                       const int32_t* byte_lengths, const int32_t* idx, int n_streams, long n, int lanes,
                                       const vam_rans_tables* tables, int32_t* sym_out, int32_t* available, int32_t* status,
                                       void* stream) {
  const char* what = "vam_rans_interleaved_decode_device";
  VAM_REQUIRE(bytes && byte_offsets && byte_lengths && idx && sym_out && available && status && bytes_total >= 0 &&
              ((uintptr_t)bytes & 3) == 0, "%s: need word-aligned bytes, offsets, lengths, idx, sym_out, available, status", what);
  if (int rc = check_streams(what, lanes, n_streams, n)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  IlvDecArgs<FlatRows> a{{}, bytes, bytes_total, byte_offsets, byte_lengths, idx, n_streams, n, lanes, *tables, sym_out, available, status};
  return launch_interleaved_decode(what, a, stream);
}

// The window forms: z and the base slices of an "embedded-4" container.
int vam_rans_interleaved_encode_nhwc_device(const int32_t* sym, const int32_t* idx, int B, int h, int w, int ld, int c0, int C,
                                            int n_slices, int lanes, const vam_rans_tables* tables, uint32_t* out_words,
                                            long out_cap_words, int32_t* lengths, int32_t* status, void* stream) {
  const char* what = "vam_rans_interleaved_encode_nhwc_device";
  VAM_REQUIRE(sym && out_words && lengths && status, "%s: need sym, out_words, lengths, status", what);
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  if (int rc = check_geometry(what, B, h, w, ld, c0, C, n_slices)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  VAM_REQUIRE(out_cap_words >= 2l * lanes && out_cap_words < (1l << 31), "%s: a region is 2 * lanes .. 2^31 words, got %ld", what,
              out_cap_words);
  const int n_streams = B * n_slices;                       // at most 2^20, each of at most 2^28 elements
  IlvEncArgs<NhwcWindow> a{{B, h * w, ld, c0, C}, sym, idx, n_streams, (long)h * w * C, lanes, *tables, out_words, out_cap_words,
                           lengths, status, nullptr, 0, nullptr};
  const int threads = n_streams * lanes;
  ProfScope prof(VAM_FAM_MISC, (hipStream_t)stream, 0.0, 0.0);
  hipLaunchKernelGGL(rans_interleaved_encode_kernel<NhwcWindow>, dim3((threads + kWave - 1) / kWave), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch("rans_interleaved_encode_kernel");
}

int vam_rans_interleaved_decode_nhwc_device(const uint8_t* bytes, long bytes_total, const int64_t* byte_offsets,
                                            const int32_t* byte_lengths, const int32_t* idx, int B, int h, int w, int ld, int c0,
                                            int C, int n_slices, int lanes, const vam_rans_tables* tables, int32_t* sym_out,
                                            int32_t* status, void* stream) {
  const char* what = "vam_rans_interleaved_decode_nhwc_device";
  VAM_REQUIRE(bytes && byte_offsets && byte_lengths && sym_out && status && bytes_total >= 0 && ((uintptr_t)bytes & 3) == 0,
              "%s: need word-aligned bytes, offsets, lengths, sym_out, status", what);
  VAM_REQUIRE(R::lanes_valid(lanes), "%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
  if (int rc = check_geometry(what, B, h, w, ld, c0, C, n_slices)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  IlvDecArgs<NhwcWindow> a{{B, h * w, ld, c0, C}, bytes, bytes_total, byte_offsets, byte_lengths, idx, B * n_slices, (long)h * w * C,
                           lanes, *tables, sym_out, nullptr, status};
  return launch_interleaved_decode(what, a, stream);
}

// ---------------------------------------------------------------- resumable decode
int vam_rans_interleaved_resume_device(const uint8_t* bytes, long bytes_total, const int64_t* byte_offsets,
                                       const int32_t* byte_lengths, const int32_t* idx, int n_streams, long n, int lanes,
                                       const vam_rans_tables* tables, int32_t* sym_out, uint64_t* states, int32_t* done, int32_t* pos,
                                       int32_t* available, int32_t* status, void* stream) {
  const char* what = "vam_rans_interleaved_resume_device";
  VAM_REQUIRE(bytes && byte_offsets && byte_lengths && idx && sym_out && available && status && bytes_total >= 0 &&
              ((uintptr_t)bytes & 3) == 0, "%s: need word-aligned bytes, offsets, lengths, idx, sym_out, available, status", what);
  VAM_REQUIRE(states && done && pos && ((uintptr_t)states & 7) == 0, "%s: need the checkpoints: 64-bit aligned states, done, pos", what);
  if (int rc = check_streams(what, lanes, n_streams, n)) return rc;
  if (int rc = check_tables(what, tables)) return rc;
  IlvResArgs a{bytes, bytes_total, byte_offsets, byte_lengths, idx, n_streams, n, lanes, *tables, sym_out, states, done, pos, available,
               status};
  return launch_with_tables(what, "rans_interleaved_resume_kernel", rans_interleaved_resume_kernel<true>,
                            rans_interleaved_resume_kernel<false>, (n_streams * lanes + kLaneBlock - 1) / kLaneBlock, kLaneBlock, a, stream);
}

}  // extern "C"
