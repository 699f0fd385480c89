// The rANS coder of rans.cpp as one core for host and device: the same wire format — 64-bit state,
// 32-bit renormalisation words, 16-bit precision, 4-bit bypass nibbles (count nibbles, then up to 8 raw nibbles), the
// final state as two words — restated so that one stream is coded without an expansion buffer and decoded without
// trusting its input.  rans.cpp is the yardstick: tests/test_rans_core_cpu.py holds this header to its bytes.
//
// Layers:   steps     enc_put / enc_put_bits / enc_element, dec_init / dec_bits / dec_element: one symbol's state update;
//                     the device kernels (rans_device.hip) call these between their parallel staging phases
//           streams   encode_stream / decode_stream: one whole stream on one thread (host exports, sanitizer program)
//           lanes     a stream as K independent lanes, each a stream of its own: the header check,
//                     lane_encode / lane_decode for one thread per lane, lanes_*_stream for all lanes on one thread
//           interleaved  K lanes on ONE word stream: interleaved_encode / _decode, and the decode from a
//                     checkpoint at a group boundary, interleaved_resume
// Addressing goes through a functor (Flat, Nhwc), the symbol search through another (TableSearch here, the wave-wide
// search of rans_device.hip), so the steps never see a pointer they could walk off.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VAM_RANS_HD __host__ __device__ inline
#else
#define VAM_RANS_HD inline
#endif

namespace vam_rans {

constexpr int kPrecision = 16;
constexpr int kBypassBits = 4;
constexpr uint32_t kMaxBypass = (1u << kBypassBits) - 1;
constexpr int kMaxRawNibbles = 32 / kBypassBits;
constexpr uint64_t kRansL = 1ull << 31;

// Per-stream status codes (0 = ok); bitstream.py words them like the host coder's errors.
enum Status : int32_t {
  kOk = 0,
  kTruncated = 1,      // decode: a word was needed past the end of the stream
  kBadIndex = 2,       // a table index outside [0, n_cdfs)
  kBadTable = 3,       // a cdf_sizes entry the coder refuses, or a table that is not increasing where it was read
  kOverflow = 4,       // encode: the output region is too small
  kZeroFreq = 5,       // encode: zero-frequency symbol (cdf table not normalised)
  kBadStream = 6       // decode: fewer than 8 bytes, not whole words, or misaligned
};

// ---------------------------------------------------------------- addressing
// Stream element i -> offset into a buffer, and the channel it belongs to (the table index when there is no index buffer).
struct Flat {
  VAM_RANS_HD long off(long i) const { return i; }
  VAM_RANS_HD int chan(long) const { return 0; }
};
// An NHWC window: element i = (c * h + y) * w + x of one image reads buf[(y * w + x) * ld + c], buf pointing at the
// image's first pixel and the window's first channel.  That is the [C, h, w] order the host coder gets after transpose.
struct Nhwc {
  long hw, ld;
  VAM_RANS_HD long off(long i) const { const long c = i / hw; return (i - c * hw) * ld + c; }
  VAM_RANS_HD int chan(long i) const { return (int)(i / hw); }
};

// ---------------------------------------------------------------- encode steps
// Exact x / f and x % f for f < 2^16 from m = floor((2^32 - 1) / f), one multiply-high and one correction per 32-bit
// step: m = 2^32 / f - e with 0 <= e <= 1, so floor(t * m / 2^32) lies in (t / f - 2, t / f]: it is q or q - 1.
VAM_RANS_HD uint32_t reciprocal(uint32_t f) { return 0xFFFFFFFFu / (f ? f : 1u); }

VAM_RANS_HD uint32_t div_step(uint32_t t, uint32_t f, uint32_t m, uint32_t& r) {
  uint32_t q = (uint32_t)(((uint64_t)t * m) >> 32);
  r = t - q * f;
  if (r >= f) { ++q; r -= f; }
  return q;
}

struct Enc {
  uint64_t x;
  uint32_t* p;         // next word is stored at --p
  uint32_t* lo;        // the region is [lo, end)
  int32_t status;
  bool writer;         // device: every lane of the wave carries the state, one lane stores
};

VAM_RANS_HD void enc_init(Enc& e, uint32_t* lo, uint32_t* end, bool writer = true) {
  e.x = kRansL; e.p = end; e.lo = lo; e.status = kOk; e.writer = writer;
}

VAM_RANS_HD void enc_flush_word(Enc& e) {
  if (e.p <= e.lo) { e.status = kOverflow; return; }
  --e.p;
  if (e.writer) *e.p = (uint32_t)e.x;
  e.x >>= 32;
}

// enc_put of rans.cpp: x = ((x / freq) << 16) + x % freq + start.  After renormalisation x < freq * 2^47, so the high
// word is below freq * 2^15 and the quotient comes from three 32-bit steps (high word, then 16 bits at a time).
VAM_RANS_HD void enc_put(Enc& e, uint32_t start, uint32_t freq, uint32_t rcp) {
  if (e.x >= ((uint64_t)freq << (31 - kPrecision + 32))) enc_flush_word(e);
  if (e.status) return;
  const uint32_t hi = (uint32_t)(e.x >> 32), lw = (uint32_t)e.x;
  uint32_t r;
  const uint64_t q0 = div_step(hi, freq, rcp, r);
  const uint64_t q1 = div_step((r << 16) | (lw >> 16), freq, rcp, r);
  const uint64_t q2 = div_step((r << 16) | (lw & 0xFFFFu), freq, rcp, r);
  e.x = (((q0 << 32) | (q1 << 16) | q2) << kPrecision) + r + start;
}

VAM_RANS_HD void enc_put_bits(Enc& e, uint32_t val) {
  if (e.x >= (1ull << (31 - kPrecision + 32 + kPrecision - kBypassBits))) enc_flush_word(e);
  if (e.status) return;
  e.x = (e.x << kBypassBits) | val;
}

// One element, looked up: the table symbol and, when it is the escape, the raw value behind it.
struct Put {
  uint32_t start_freq;  // start | freq << 16 (both < 2^16)
  uint32_t rcp;
  uint32_t raw;
  int32_t n_bypass;     // -1: no escape
};

// The look-ups of encode_one for one element (value already masked by the layer selection).  Returns a status.
VAM_RANS_HD int32_t classify(int32_t symbol, int ci, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                             const int32_t* offsets, int n_cdfs, Put& u) {
  u.start_freq = 0; u.rcp = 0; u.raw = 0; u.n_bypass = -1;
  if (ci < 0 || ci >= n_cdfs) return kBadIndex;
  const int32_t* cdf = cdfs + (long)ci * cdf_stride;
  const int max_value = cdf_sizes[ci] - 2;
  if (max_value < 0 || max_value + 1 >= cdf_stride) return kBadTable;
  int64_t value = (int64_t)symbol - offsets[ci];
  uint32_t raw = 0;
  if (value < 0) {
    raw = (uint32_t)(-2 * value - 1);
    value = max_value;
  } else if (value >= max_value) {
    raw = (uint32_t)(2 * (value - max_value));
    value = max_value;
  }
  const uint32_t start = (uint16_t)cdf[value], freq = (uint16_t)(cdf[value + 1] - cdf[value]);
  if (freq == 0) return kZeroFreq;
  u.start_freq = start | (freq << 16);
  u.rcp = reciprocal(freq);
  if (value == max_value) {
    int nb = 0;
    while (nb < kMaxRawNibbles && (raw >> (nb * kBypassBits)) != 0) ++nb;
    u.raw = raw;
    u.n_bypass = nb;
  }
  return kOk;
}

// The puts of one element in reverse: raw nibbles n_bypass-1 .. 0, the count nibbles backwards, then the table symbol
// (the decoder reads symbol, count, raw nibbles 0 .. n_bypass-1).
VAM_RANS_HD void enc_element(Enc& e, const Put& u) {
  if (u.n_bypass >= 0) {
    for (int j = u.n_bypass - 1; j >= 0; --j) enc_put_bits(e, (u.raw >> (j * kBypassBits)) & kMaxBypass);
    enc_put_bits(e, (uint32_t)u.n_bypass % kMaxBypass);                  // forward: [15] * (n / 15), then n % 15
    for (int k = u.n_bypass / (int)kMaxBypass; k > 0; --k) enc_put_bits(e, kMaxBypass);
  }
  enc_put(e, u.start_freq & 0xFFFFu, u.start_freq >> 16, u.rcp);
}

// The final state as two words; returns the stream length in words (the stream is the region's tail).
VAM_RANS_HD long enc_finish(Enc& e, uint32_t* end) {
  if (e.status) return 0;
  if (e.p - e.lo < 2) { e.status = kOverflow; return 0; }
  e.p -= 2;
  if (e.writer) { e.p[0] = (uint32_t)e.x; e.p[1] = (uint32_t)(e.x >> 32); }
  return (long)(end - e.p);
}

// One stream on one thread.  sym / idx / layer are addressed through A; idx == NULL means "index = channel".
// Words are written backwards from region + cap_words; *n_words receives the length, the stream is the tail.
template <class A>
VAM_RANS_HD int32_t encode_stream(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at,
                                  const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                  int n_cdfs, uint32_t* region, long cap_words, long* n_words) {
  *n_words = 0;
  Enc e;
  enc_init(e, region, region + cap_words);
  for (long i = n - 1; i >= 0; --i) {
    const long o = at.off(i);
    const bool keep = !layer || layer[o] == sel;
    const int ci = keep ? (idx ? idx[o] : at.chan(i)) : 0;
    Put u;
    const int32_t st = classify(keep ? sym[o] : 0, ci, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, u);
    if (st) return st;
    enc_element(e, u);
    if (e.status) return e.status;
  }
  *n_words = enc_finish(e, region + cap_words);
  return e.status;
}

// ---------------------------------------------------------------- decode steps
struct Dec {
  uint64_t x;
  const uint32_t* p;
  const uint32_t* end;
  int32_t status;
};

VAM_RANS_HD void dec_init(Dec& d, const uint32_t* words, long n_bytes) {
  d.x = 0; d.p = d.end = words; d.status = kOk;
  if (!words || n_bytes < 8 || (n_bytes & 3) || ((uintptr_t)words & 3)) { d.status = kBadStream; return; }
  d.end = words + n_bytes / 4;
  d.x = (uint64_t)words[0] | ((uint64_t)words[1] << 32);
  d.p = words + 2;
}

VAM_RANS_HD void dec_renorm(Dec& d) {
  if (d.x < kRansL) {
    if (d.p >= d.end) { d.status = kTruncated; return; }
    d.x = (d.x << 32) | *d.p++;
  }
}

VAM_RANS_HD uint32_t dec_bits(Dec& d) {
  const uint32_t val = (uint32_t)(d.x & kMaxBypass);
  d.x >>= kBypassBits;
  dec_renorm(d);
  return val;
}

// One element of a table with `sz` entries.  find(cum, start, freq) returns the host's scan result s = the number of
// entries 1 .. sz-1 that are <= cum (at most sz - 2), and that entry's start and frequency.  Returns the value relative
// to the table's offset; d.status != 0 afterwards means the element is incomplete and the value is not to be used.
template <class F>
VAM_RANS_HD int32_t dec_element(Dec& d, const F& find, int sz) {
  const uint32_t cum = (uint32_t)(d.x & ((1u << kPrecision) - 1));
  uint32_t start, freq;
  const int s = find(cum, start, freq);
  if (freq == 0 || freq > (1u << kPrecision) || start > cum) { d.status = kBadTable; return 0; }
  d.x = (uint64_t)freq * (d.x >> kPrecision) + cum - start;
  dec_renorm(d);
  if (d.status) return 0;
  const int max_value = sz - 2;
  if (s != max_value) return s;
  uint32_t val = dec_bits(d);
  uint32_t n_bypass = val;
  while (!d.status && val == kMaxBypass) {        // every nibble eats 4 bits of the stream: bounded by its length
    val = dec_bits(d);
    n_bypass += val;
  }
  uint32_t raw = 0;
  for (uint32_t j = 0; !d.status && j < n_bypass; ++j) {
    const uint32_t nib = dec_bits(d);
    if (j < (uint32_t)kMaxRawNibbles) raw |= nib << (j * kBypassBits);
  }
  if (d.status) return 0;
  const uint32_t half = raw >> 1;                 // unsigned: a corrupt stream may not overflow an int
  return (int32_t)((raw & 1) ? ~half : half + (uint32_t)max_value);
}

// The host's linear scan as a binary search: entries 1 .. sz-1 are increasing on every table the coder accepts, so the
// count of entries <= cum is the scan's stopping point.  E = int32_t reads a row of the [n_cdfs][stride] tables;
// E = uint16_t with implied_last reads a packed table, whose entry sz-1 is not stored: it is 65536, above every cum.
template <class E>
struct TableSearch {
  const E* cdf;
  int sz;
  bool implied_last;
  VAM_RANS_HD int operator()(uint32_t cum, uint32_t& start, uint32_t& freq) const {
    int lo = 0, hi = implied_last ? sz - 2 : sz - 1;  // s in [lo, hi]: cdf[1 .. lo] <= cum
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if ((uint32_t)cdf[mid] <= cum) lo = mid; else hi = mid - 1;
    }
    if (lo > sz - 2) lo = sz - 2;                 // only on a table without its terminal 65536: stay inside it
    start = (uint32_t)cdf[lo];
    freq = (implied_last && lo == sz - 2 ? (1u << kPrecision) : (uint32_t)cdf[lo + 1]) - start;
    return lo;
  }
};

// Where table ci lives: the int32 rows, or the packed 16-bit tables at their start offsets (rans_device.hip's LDS copy).
// none() is the row of no table: what a refused index is given, never searched.
struct Int32Rows {
  const int32_t* cdfs;
  int stride;
  VAM_RANS_HD TableSearch<int32_t> operator()(int ci, int sz) const { return {cdfs + (long)ci * stride, sz, false}; }
  VAM_RANS_HD TableSearch<int32_t> none() const { return {nullptr, 2, false}; }
};
struct PackedRows {
  const uint16_t* packed;
  const int32_t* starts;
  VAM_RANS_HD TableSearch<uint16_t> operator()(int ci, int sz) const { return {packed + starts[ci], sz, true}; }
  VAM_RANS_HD TableSearch<uint16_t> none() const { return {nullptr, 2, true}; }
};

// The one check of a table index: table ci of `rows` with its size, or the status that refuses it (kBadIndex, kBadTable)
// with the row of no table and the smallest size, so that a caller may carry the row on without a branch.  The nested
// form, one assignment in the innermost branch, is what keeps the device kernels' registers where they were.
template <class F>
struct TableRow {
  int32_t status;
  int sz;
  F row;
};
template <class T>
VAM_RANS_HD auto table_row(const T& rows, int ci, int cdf_stride, const int32_t* cdf_sizes, int n_cdfs) -> TableRow<decltype(rows(0, 2))> {
  TableRow<decltype(rows(0, 2))> t{kBadIndex, 2, rows.none()};
  if (ci >= 0 && ci < n_cdfs) {
    const int sz = cdf_sizes[ci];
    if (sz - 2 < 0 || sz - 1 >= cdf_stride) t.status = kBadTable;
    else t = {kOk, sz, rows(ci, sz)};
  }
  return t;
}

// The n elements of a stream whose state is initialised (or refused: d.status) in d.  Only elements with layer == sel
// are written; after a failure every remaining selected element is written as 0.
template <class A, class T>
VAM_RANS_HD int32_t decode_elements(Dec& d, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at, const T& rows,
                                    int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* out) {
  for (long i = 0; i < n; ++i) {
    const long o = at.off(i);
    const bool keep = !layer || layer[o] == sel;
    int32_t value = 0;
    if (!d.status) {
      const int ci = keep ? (idx ? idx[o] : at.chan(i)) : 0;
      const auto t = table_row(rows, ci, cdf_stride, cdf_sizes, n_cdfs);
      d.status = t.status;
      if (!d.status) {
        const int32_t v = dec_element(d, t.row, t.sz);
        if (!d.status) value = (int32_t)((uint32_t)v + (uint32_t)offsets[ci]);
      }
    }
    if (keep) out[o] = value;
  }
  return d.status;
}

// One stream on one thread; idx == NULL means "index = channel".
template <class A>
VAM_RANS_HD int32_t decode_stream(const uint32_t* words, long n_bytes, const int32_t* idx, const uint8_t* layer, int sel,
                                  long n, const A& at, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                                  const int32_t* offsets, int n_cdfs, int32_t* out) {
  Dec d;
  dec_init(d, words, n_bytes);
  return decode_elements(d, idx, layer, sel, n, at, Int32Rows{cdfs, cdf_stride}, cdf_stride, cdf_sizes, offsets, n_cdfs, out);
}

// ---------------------------------------------------------------- lane-split streams
// A stream of n elements as K independent lanes, K a power of two in 1 .. 64: lane j is the stream above of the
// elements j, j + K, j + 2K, ...  K == 1 is that stream itself, with no header.  For K > 1 the string is K uint32 lane
// lengths in words (each >= 2), then the lanes' words back to back: 4 K + 4 sum(L_j) bytes, exactly.  K is not stored.
constexpr int kMaxLanes = 64;

VAM_RANS_HD bool lanes_valid(int K) { return K >= 1 && K <= kMaxLanes && (K & (K - 1)) == 0; }
VAM_RANS_HD long lane_elements(long n, int j, int K) { return n > j ? (n - j + K - 1) / K : 0; }
// Words a lane's region needs: 8 m + 64 bytes for the m = ceil(n / K) elements of the longest lane, the host's budget.
VAM_RANS_HD long lane_cap_words(long n, int K) { return 2 * ((n + K - 1) / K) + 16; }

// Element i of lane j is element j + i K of the stream.
template <class A>
struct Lane {
  A at;
  long j, K;
  VAM_RANS_HD long off(long i) const { return at.off(j + i * K); }
  VAM_RANS_HD int chan(long i) const { return at.chan(j + i * K); }
};

// The header check: lane `lane` of the string is the n_words words from word `first` on.  kBadStream for a string
// that is misaligned, not whole words or shorter than its header, for a lane shorter than a final state, and for
// lengths that do not add up to the string's; the sums are 64-bit, so no header wraps them.  K == 1 has no header:
// dec_init checks that string itself.
VAM_RANS_HD int32_t lanes_header(const uint32_t* words, long n_bytes, int K, int lane, long& first, long& n_words) {
  first = 0; n_words = 0;
  if (!lanes_valid(K) || lane < 0 || lane >= K) return kBadStream;
  if (K == 1) { n_words = n_bytes / 4; return kOk; }
  if (!words || ((uintptr_t)words & 3) || n_bytes < 4l * K || (n_bytes & 3)) return kBadStream;
  uint64_t total = (uint64_t)K, before = (uint64_t)K;
  for (int j = 0; j < K; ++j) {
    const uint32_t len = words[j];
    if (len < 2) return kBadStream;
    total += len;
    if (j < lane) before += len;
  }
  if (total != (uint64_t)(n_bytes / 4)) return kBadStream;
  first = (long)before; n_words = (long)words[lane];
  return kOk;
}

// One lane of a string: its own state, word pointer and end.  T finds the tables (Int32Rows, PackedRows).
template <class A, class T>
VAM_RANS_HD int32_t lane_decode(const uint32_t* words, long n_bytes, int K, int lane, const int32_t* idx, const uint8_t* layer,
                                int sel, long n, const A& at, const T& rows, int cdf_stride, const int32_t* cdf_sizes,
                                const int32_t* offsets, int n_cdfs, int32_t* out) {
  long first, n_words;
  Dec d;
  const int32_t st = lanes_header(words, n_bytes, K, lane, first, n_words);
  if (st) { d.x = 0; d.p = d.end = words; d.status = st; }
  else dec_init(d, words + first, K == 1 ? n_bytes : 4 * n_words);
  return decode_elements(d, idx, layer, sel, lane_elements(n, lane, K), Lane<A>{at, lane, K}, rows, cdf_stride, cdf_sizes, offsets,
                         n_cdfs, out);
}

// One lane into its own region of cap_words words (the lane is the region's tail).
template <class A>
VAM_RANS_HD int32_t lane_encode(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at, int K,
                                int lane, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                int n_cdfs, uint32_t* region, long cap_words, long* n_words) {
  return encode_stream(sym, idx, layer, sel, lane_elements(n, lane, K), Lane<A>{at, lane, K}, cdfs, cdf_stride, cdf_sizes, offsets,
                       n_cdfs, region, cap_words, n_words);
}

// All lanes of one stream on one thread.  Lane j is coded into regions + j * cap_words; lane_words[j] and lane_status[j]
// receive its length and status.  Returns the status of the lowest-numbered failing lane.
template <class A>
VAM_RANS_HD int32_t lanes_encode_stream(const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n, const A& at,
                                        int K, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets,
                                        int n_cdfs, uint32_t* regions, long cap_words, long* lane_words, int32_t* lane_status) {
  int32_t first_bad = kOk;
  for (int j = 0; j < K; ++j) {
    lane_status[j] = lane_encode(sym, idx, layer, sel, n, at, K, j, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                                 regions + (long)j * cap_words, cap_words, lane_words + j);
    if (lane_status[j] && !first_bad) first_bad = lane_status[j];
  }
  return first_bad;
}

// A failing lane zeroes its own elements from the failure on; the other lanes are still decoded.  A refused header
// fails every lane, so every selected element is 0.  Returns the status of the lowest-numbered failing lane.
template <class A>
VAM_RANS_HD int32_t lanes_decode_stream(const uint32_t* words, long n_bytes, int K, const int32_t* idx, const uint8_t* layer, int sel,
                                        long n, const A& at, const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes,
                                        const int32_t* offsets, int n_cdfs, int32_t* out, int32_t* lane_status) {
  int32_t first_bad = kOk;
  for (int j = 0; j < K; ++j) {
    lane_status[j] = lane_decode(words, n_bytes, K, j, idx, layer, sel, n, at, Int32Rows{cdfs, cdf_stride}, cdf_stride, cdf_sizes,
                                 offsets, n_cdfs, out);
    if (lane_status[j] && !first_bad) first_bad = lane_status[j];
  }
  return first_bad;
}

// ---------------------------------------------------------------- interleaved lanes
// A stream of n elements on K interleaved lanes, K as above: element i belongs to lane i % K and group i / K, and the K
// coder states share ONE word stream.  The string is the K final states in lane order (two words each, as enc_finish
// writes one), then the renormalisation words in the order the decoder reads them: groups ascending; inside a group the
// rounds t = 0, 1, ..; in round t every lane that still has a get t updates its state, then the lanes whose state fell
// below 2^31 take one word each in ascending lane order.  Get 0 of an element is the table symbol, the count nibbles and
// the raw nibbles follow when it is the escape (dec_element's order).  The encoder is the mirror: groups, rounds and lanes
// descending, words stored backwards.  So a prefix of the words decodes a prefix of the elements, and K == 1 is the
// stream above byte for byte.
//
// The steps here split an element into its gets / puts so that a driver can renormalise between them: the host drivers
// below run all lanes on one thread, rans_device.hip runs one thread per lane and finds a lane's word by a wave ballot.

// Put t of an element, numbered like the decoder's gets: 0 = the table symbol, 1 .. = the count nibbles ([15] * (n / 15),
// then n % 15), then the raw nibbles 0 .. n_bypass - 1.  An element has put_gets(u) <= kMaxGets of them.
constexpr int kMaxGets = 2 + kMaxRawNibbles;                // classify gives n_bypass <= 8: one count nibble
VAM_RANS_HD int put_gets(const Put& u) { return u.n_bypass < 0 ? 1 : 2 + u.n_bypass / (int)kMaxBypass + u.n_bypass; }

VAM_RANS_HD uint32_t put_nibble(const Put& u, int t) {
  const int nc = u.n_bypass / (int)kMaxBypass + 1;          // count nibbles
  if (t < nc) return kMaxBypass;
  if (t == nc) return (uint32_t)u.n_bypass % kMaxBypass;
  return (u.raw >> ((t - nc - 1) * kBypassBits)) & kMaxBypass;
}

// Whether put t flushes a word first: the bounds of enc_put and enc_put_bits.
VAM_RANS_HD bool put_flushes(const Enc& e, const Put& u, int t) {
  return t == 0 ? e.x >= ((uint64_t)(u.start_freq >> 16) << (31 - kPrecision + 32))
                : e.x >= (1ull << (31 - kPrecision + 32 + kPrecision - kBypassBits));
}

VAM_RANS_HD void enc_put_step(Enc& e, const Put& u, int t) {
  if (t == 0) enc_put(e, u.start_freq & 0xFFFFu, u.start_freq >> 16, u.rcp);
  else enc_put_bits(e, put_nibble(u, t));
}

// Words that hold any string: the K states and at most two words per element (16 + 4 * 9 bits), with the host's slack.
VAM_RANS_HD long interleaved_cap_words(long n, int K) { return 2 * n + 2 * K + 16; }

// All lanes on one thread.  Words are written backwards from region + cap_words; the string is the region's tail.
template <class A>
VAM_RANS_HD int32_t interleaved_encode(const int32_t* sym, const int32_t* idx, long n, const A& at, int K, const int32_t* cdfs,
                                       int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs,
                                       uint32_t* region, long cap_words, long* n_words) {
  *n_words = 0;
  if (!lanes_valid(K) || n < 0) return kBadStream;
  Enc e;
  enc_init(e, region, region + cap_words);
  uint64_t xs[kMaxLanes];
  Put us[kMaxLanes];
  for (int l = 0; l < K; ++l) xs[l] = kRansL;
  for (long g = (n + K - 1) / K - 1; g >= 0; --g) {
    const int m = (int)(n - g * K < K ? n - g * K : K);      // lanes with an element in this group
    int rounds = 0;
    for (int l = 0; l < m; ++l) {
      const long o = at.off(g * K + l);
      const int32_t st = classify(sym[o], idx ? idx[o] : at.chan(g * K + l), cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, us[l]);
      if (st) return st;
      if (put_gets(us[l]) > rounds) rounds = put_gets(us[l]);
    }
    for (int t = rounds - 1; t >= 0; --t)
      for (int l = m - 1; l >= 0; --l) {
        if (put_gets(us[l]) <= t) continue;
        e.x = xs[l];
        enc_put_step(e, us[l], t);
        if (e.status) return e.status;
        xs[l] = e.x;
      }
  }
  if (e.p - e.lo < 2l * K) return kOverflow;
  e.p -= 2l * K;
  for (int l = 0; l < K; ++l) { e.p[2 * l] = (uint32_t)xs[l]; e.p[2 * l + 1] = (uint32_t)(xs[l] >> 32); }
  *n_words = (long)(region + cap_words - e.p);
  return kOk;
}

// One lane's element in flight: dec_element cut into its gets.  get_step does one get's state update (dec_element's
// arithmetic) and says whether a renormalisation word is due; the driver supplies it (x = x << 32 | word) or fails the lane.
enum GetPhase : int32_t { kGetSymbol = 0, kGetCount = 1, kGetRaw = 2, kGetDone = 3 };
struct Get {
  uint64_t x;
  uint32_t n_bypass, raw, j;
  int32_t value;       // relative to the table's offset; valid once phase == kGetDone with status == 0
  int32_t phase;
  int32_t status;
};

template <class F>
VAM_RANS_HD bool get_step(Get& g, const F& find, int sz) {
  const int max_value = sz - 2;
  if (g.phase == kGetSymbol) {
    const uint32_t cum = (uint32_t)(g.x & ((1u << kPrecision) - 1));
    uint32_t start, freq;
    const int s = find(cum, start, freq);
    if (freq == 0 || freq > (1u << kPrecision) || start > cum) { g.status = kBadTable; g.phase = kGetDone; return false; }
    g.x = (uint64_t)freq * (g.x >> kPrecision) + cum - start;
    g.value = s;
    g.n_bypass = 0; g.raw = 0; g.j = 0;
    g.phase = s != max_value ? kGetDone : kGetCount;
  } else {
    const uint32_t nib = (uint32_t)(g.x & kMaxBypass);
    g.x >>= kBypassBits;
    if (g.phase == kGetCount) {
      g.n_bypass += nib;
      if (nib != kMaxBypass) g.phase = g.n_bypass ? kGetRaw : kGetDone;
    } else {
      if (g.j < (uint32_t)kMaxRawNibbles) g.raw |= nib << (g.j * kBypassBits);
      if (++g.j >= g.n_bypass) g.phase = kGetDone;
    }
    if (g.phase == kGetDone) {
      const uint32_t half = g.raw >> 1;                      // unsigned: a corrupt stream may not overflow an int
      g.value = (int32_t)((g.raw & 1) ? ~half : half + (uint32_t)max_value);
    }
  }
  return g.x < kRansL;
}

// One group of the tolerant decode, all lanes on one thread: the m lanes of group g run their gets from the states in gs,
// taking words from position pos on.  The string's word p is words[p - first_word] and it holds the words below W.  Returns
// the lowest failed lane (m when none failed); status = that of the lowest lane from there on that failed with one, kOk when
// the group only ran out of words.  ci and last (m entries each) receive the lanes' table indexes and the read position
// after each lane's last word (0: it read none).
template <class A, class T>
VAM_RANS_HD int interleaved_group(const uint32_t* words, long first_word, long W, int K, long g, int m, const int32_t* idx, const A& at,
                                  const T& rows, int cdf_stride, const int32_t* cdf_sizes, int n_cdfs, Get* gs, long& pos, int* ci,
                                  long* last, int32_t& status) {
  using Find = decltype(rows(0, 2));
  Find find[kMaxLanes];
  int sz[kMaxLanes];
  bool active[kMaxLanes], failed[kMaxLanes], need[kMaxLanes];
  int n_active = 0;
  for (int l = 0; l < m; ++l) {
    Get& t = gs[l];
    t.status = kOk; t.phase = kGetSymbol; t.value = 0;
    last[l] = 0;
    ci[l] = idx ? idx[at.off(g * K + l)] : at.chan(g * K + l);
    const auto row = table_row(rows, ci[l], cdf_stride, cdf_sizes, n_cdfs);
    t.status = row.status; sz[l] = row.sz; find[l] = row.row;
    failed[l] = t.status != 0;
    active[l] = !failed[l];
    n_active += active[l];
  }
  while (n_active > 0) {                                      // one round: the updates, then the words in lane order
    for (int l = 0; l < m; ++l) {
      need[l] = active[l] && get_step(gs[l], find[l], sz[l]);
      if (active[l] && gs[l].status) { failed[l] = true; need[l] = false; }
    }
    for (int l = 0; l < m; ++l) {
      if (!active[l]) continue;
      if (need[l]) {
        if (pos < W) { gs[l].x = (gs[l].x << 32) | words[pos - first_word]; last[l] = ++pos; }
        else failed[l] = true;
      }
      if (failed[l] || gs[l].phase == kGetDone) { active[l] = false; --n_active; }
    }
  }
  int first = 0;
  while (first < m && !failed[first]) ++first;
  status = kOk;
  for (int l = first; l < m && !status; ++l) status = gs[l].status;
  return first;
}

// Tolerant prefix decode, all lanes on one thread: `words` are the first floor(n_bytes / 4) words of a string.  With fewer
// than 2 K words nothing decodes.  A lane that needs a word past the prefix fails, and so does every later request; the
// other lanes of that group finish the gets that need no word, and decoding ends with that group:
// *available = g K + the lowest failed lane of group g (n when no lane failed).  out (may be NULL) receives the elements
// below *available, the rest of it is left untouched.  A bad index or table fails its lane the same way and is the status
// returned (that of the lowest such lane of the last group); running out of words is no error.
// marks (may be NULL): n_marks sorted counts; mark_bytes[m] = 4 * the read position after the last word any of the
// elements 0 .. marks[m] - 1 reads (8 K when they read none, 0 for a count of 0), -1 for a count beyond *available.
template <class A, class T>
VAM_RANS_HD int32_t interleaved_decode(const uint32_t* words, long n_bytes, int K, const int32_t* idx, long n, const A& at,
                                       const T& rows, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs,
                                       int32_t* out, long* available, const long* marks, int n_marks, long* mark_bytes) {
  *available = 0;
  int mk = 0;
  for (int q = 0; q < n_marks; ++q) mark_bytes[q] = -1;
  while (mk < n_marks && marks[mk] <= 0) mark_bytes[mk++] = 0;
  if (!lanes_valid(K) || n < 0 || n_bytes < 0) return kBadStream;
  const long W = n_bytes / 4;
  if (W > 0 && (!words || ((uintptr_t)words & 3))) return kBadStream;
  if (W < 2l * K) return kOk;
  Get gs[kMaxLanes];
  for (int l = 0; l < K; ++l) gs[l].x = (uint64_t)words[2 * l] | ((uint64_t)words[2 * l + 1] << 32);
  long pos = 2l * K, reach = 2l * K;                        // next word; read position after the last word of the elements so far
  for (long g = 0; g * K < n; ++g) {
    const int m = (int)(n - g * K < K ? n - g * K : K);
    int ci[kMaxLanes];
    long last[kMaxLanes];
    int32_t status;
    const int first = interleaved_group(words, 0, W, K, g, m, idx, at, rows, cdf_stride, cdf_sizes, n_cdfs, gs, pos, ci, last, status);
    for (int l = 0; l < first; ++l) {
      if (out) out[at.off(g * K + l)] = (int32_t)((uint32_t)gs[l].value + (uint32_t)offsets[ci[l]]);
      if (last[l] > reach) reach = last[l];
      while (mk < n_marks && marks[mk] <= g * K + l + 1) mark_bytes[mk++] = 4 * reach;
    }
    *available = g * K + first;
    if (first < m) return status;
  }
  return kOk;
}

// ---------------------------------------------------------------- resumable decode
// The checkpoint of a stream is the decoder at the start of a group: `done` elements lie before that group (a multiple of
// K, or n once the stream is finished), `pos` is the index in the whole string of the next word to read, and states holds
// the K lane states there.  done = 0, pos = 0 is the fresh checkpoint: its states are read from the string's first 2 K words.
VAM_RANS_HD bool checkpoint_valid(long done, long pos, long n, int K) {
  return done >= 0 && done <= n && (done == n || done % K == 0) && pos >= 0 && (done == 0 || pos >= 2l * K);
}

// interleaved_decode from a checkpoint: `words` are the string's whole words FROM WORD pos ON, n_bytes their bytes, so the
// string is known up to the absolute word count W = pos + floor(n_bytes / 4).  Decoding proceeds as interleaved_decode's
// does from group done / K and writes out[i] (out may be NULL) for done_in <= i < *available only.  When a lane of group g
// fails, for want of a word or with a status, the checkpoint becomes the start of that group: done = g K, pos and states
// as they were when it began; a complete stream gets done = n and reads and writes nothing on later calls.  With a fresh
// checkpoint and W < 2 K nothing decodes and the checkpoint stays fresh.  For successive prefixes of one string,
// *available, the elements below it and the status returned equal interleaved_decode's on the whole prefix: a group that
// completed read only words the shorter prefix held.  The status is recomputed on every call.  An impossible checkpoint
// is kBadStream, with nothing read or written.
template <class A, class T>
VAM_RANS_HD int32_t interleaved_resume(const uint32_t* words, long n_bytes, int K, const int32_t* idx, long n, const A& at,
                                       const T& rows, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs,
                                       int32_t* out, long* available, long* done, long* pos, uint64_t* states) {
  *available = 0;
  if (!lanes_valid(K) || n < 0 || n_bytes < 0 || !checkpoint_valid(*done, *pos, n, K)) return kBadStream;
  if (*done == n) { *available = n; return kOk; }
  const long first_word = *pos, W = first_word + n_bytes / 4;
  if (W > first_word && (!words || ((uintptr_t)words & 3))) return kBadStream;
  Get gs[kMaxLanes];
  long p = first_word;
  if (*done == 0 && *pos == 0) {
    if (W < 2l * K) return kOk;
    for (int l = 0; l < K; ++l) gs[l].x = (uint64_t)words[2 * l] | ((uint64_t)words[2 * l + 1] << 32);
    p = 2l * K;
  } else {
    for (int l = 0; l < K; ++l) gs[l].x = states[l];
  }
  for (long g = *done / K; g * K < n; ++g) {
    const int m = (int)(n - g * K < K ? n - g * K : K);
    int ci[kMaxLanes];
    long last[kMaxLanes];
    uint64_t begin[kMaxLanes];
    const long p_begin = p;
    for (int l = 0; l < K; ++l) begin[l] = gs[l].x;
    int32_t status;
    const int first = interleaved_group(words, first_word, W, K, g, m, idx, at, rows, cdf_stride, cdf_sizes, n_cdfs, gs, p, ci, last,
                                        status);
    for (int l = 0; l < first; ++l)
      if (out) out[at.off(g * K + l)] = (int32_t)((uint32_t)gs[l].value + (uint32_t)offsets[ci[l]]);
    *available = g * K + first;
    if (first < m) {
      for (int l = 0; l < K; ++l) states[l] = begin[l];
      *done = g * K; *pos = p_begin;
      return status;
    }
  }
  for (int l = 0; l < K; ++l) states[l] = gs[l].x;
  *done = n; *pos = p;
  return kOk;
}

}  // namespace vam_rans
