// Bitstream layer: CDF quantisation and the rANS entropy coder that the
// reference reaches through compressai 1.2.4 (`_CXX.pmf_to_quantized_cdf`, `ans.RansEncoder` /
// `ans.RansDecoder`; call sites reference entropy_models.py:61-64,175-183,206-294).
//
// compressai is absent offline, so this is a restatement of its PUBLISHED algorithm (which itself
// ports ryg_rans' rans64): 64-bit state, 32-bit renormalisation words, 16-bit CDF precision,
// 4-bit bypass chunks for out-of-range symbols, symbols pushed in order and encoded in reverse.
// Wire compatibility with compressai cannot be checked here (no vectors, no library) — DESIGN.md
// marks it "unpinned"; what IS tested is: round trip, agreement with the independent pure-Python
// restatement in oracle/rans_oracle.py, and the rate against -sum(log2 p).
//
// Host code by nature (bit-serial, one stream per image and slice); it runs beside the GPU path,
// exactly where the reference runs it (SURVEY §1 "sits beside the path").
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/vampic.h"
#include "rans_core.h"

namespace vam {
void set_error(const char* fmt, ...);
}
using vam::set_error;

namespace {

constexpr int kPrecision = 16;
constexpr int kBypassBits = 4;
constexpr uint32_t kMaxBypass = (1u << kBypassBits) - 1;
constexpr uint64_t kRansL = 1ull << 31;

struct Sym {
  uint16_t start;
  uint16_t range;   // 0 means 65536 is impossible here: ranges are < 2^16 by construction
  bool bypass;
};

inline void enc_put(uint64_t& x, uint32_t*& p, uint32_t start, uint32_t freq, uint32_t scale_bits) {
  const uint64_t x_max = ((kRansL >> scale_bits) << 32) * freq;
  if (x >= x_max) {
    *--p = (uint32_t)x;
    x >>= 32;
  }
  x = ((x / freq) << scale_bits) + (x % freq) + start;
}

inline void enc_put_bits(uint64_t& x, uint32_t*& p, uint32_t val, uint32_t nbits) {
  const uint32_t freq = 1u << (16 - nbits);
  const uint64_t x_max = ((kRansL >> 16) << 32) * freq;
  if (x >= x_max) {
    *--p = (uint32_t)x;
    x >>= 32;
  }
  x = (x << nbits) | val;
}

inline uint32_t dec_get_bits(uint64_t& x, const uint32_t*& p, const uint32_t* end, uint32_t nbits, bool& ok) {
  const uint32_t val = (uint32_t)(x & ((1u << nbits) - 1));
  x >>= nbits;
  if (x < kRansL) {
    if (p >= end) { ok = false; return 0; }
    x = (x << 32) | *p++;
  }
  return val;
}

}  // namespace

extern "C" {

int vam_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out) {
  if (!pmf || !cdf_out || n < 1 || precision < 1 || precision > 16) {
    set_error("vam_pmf_to_quantized_cdf: bad arguments");
    return VAM_EINVAL;
  }
  for (int i = 0; i < n; ++i)
    if (!(pmf[i] >= 0.f) || !std::isfinite(pmf[i])) {
      set_error("vam_pmf_to_quantized_cdf: invalid pmf value at %d", i);
      return VAM_EINVAL;
    }
  std::vector<uint32_t> cdf(n + 1);
  cdf[0] = 0;
  for (int i = 0; i < n; ++i) cdf[i + 1] = (uint32_t)std::round(pmf[i] * (float)(1 << precision));
  uint32_t total = 0;
  for (uint32_t v : cdf) total += v;
  if (total == 0) {
    set_error("vam_pmf_to_quantized_cdf: pmf sums to zero");
    return VAM_EINVAL;
  }
  for (auto& v : cdf) v = (uint32_t)((((uint64_t)1 << precision) * v) / total);
  for (int i = 1; i <= n; ++i) cdf[i] += cdf[i - 1];
  cdf[n] = 1u << precision;
  for (int i = 0; i < n; ++i) {
    if (cdf[i] == cdf[i + 1]) {
      // steal one count from the least frequent symbol that can spare it
      uint32_t best_freq = ~0u;
      int best = -1;
      for (int j = 0; j < n; ++j) {
        uint32_t f = cdf[j + 1] - cdf[j];
        if (f > 1 && f < best_freq) { best_freq = f; best = j; }
      }
      if (best < 0) {
        set_error("vam_pmf_to_quantized_cdf: cannot give every symbol a non-zero frequency");
        return VAM_EINVAL;
      }
      if (best < i) for (int j = best + 1; j <= i; ++j) cdf[j]--;
      else for (int j = i + 1; j <= best; ++j) cdf[j]++;
    }
  }
  for (int i = 0; i <= n; ++i) cdf_out[i] = (int32_t)cdf[i];
  return VAM_OK;
}

}  // extern "C"

namespace {

// One stream.  layer != NULL: element i is coded as symbol 0 with table 0 unless layer[i] == sel (the reference's
// `r_sym * delta`, `idx * delta`, src/test/functions_encode.py:190-192, without building the masked copies).
long encode_one(const int32_t* symbols, const int32_t* indexes, const uint8_t* layer, int sel, long n, const int32_t* cdfs,
                int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long out_cap) {
  if (!symbols || !indexes || !cdfs || !cdf_sizes || !offsets || !out || n < 0 || n_cdfs < 1) {
    set_error("vam_rans_encode: bad arguments");
    return VAM_EINVAL;
  }
  std::vector<Sym> syms;
  syms.reserve((size_t)n + 16);
  for (long i = 0; i < n; ++i) {
    const bool keep = !layer || layer[i] == sel;
    const int ci = keep ? indexes[i] : 0;
    if (ci < 0 || ci >= n_cdfs) {
      set_error("vam_rans_encode: index %d out of range at %ld", ci, i);
      return VAM_EINVAL;
    }
    const int32_t* cdf = cdfs + (long)ci * cdf_stride;
    const int max_value = cdf_sizes[ci] - 2;
    if (max_value < 0 || max_value + 1 >= cdf_stride) {
      set_error("vam_rans_encode: cdf size %d invalid for table %d", cdf_sizes[ci], ci);
      return VAM_EINVAL;
    }
    int32_t value = (keep ? symbols[i] : 0) - offsets[ci];
    uint32_t raw = 0;
    if (value < 0) {
      raw = (uint32_t)(-2 * (int64_t)value - 1);
      value = max_value;
    } else if (value >= max_value) {
      raw = (uint32_t)(2 * ((int64_t)value - max_value));
      value = max_value;
    }
    syms.push_back({(uint16_t)cdf[value], (uint16_t)(cdf[value + 1] - cdf[value]), false});
    if (value == max_value) {                      // bypass mode: Golomb-like count + raw 4-bit chunks
      int n_bypass = 0;
      while (n_bypass < 32 / kBypassBits && (raw >> (n_bypass * kBypassBits)) != 0) ++n_bypass;   // no shift by 32
      int32_t val = n_bypass;
      while (val >= (int32_t)kMaxBypass) {
        syms.push_back({(uint16_t)kMaxBypass, (uint16_t)(kMaxBypass + 1), true});
        val -= kMaxBypass;
      }
      syms.push_back({(uint16_t)val, (uint16_t)(val + 1), true});
      for (int j = 0; j < n_bypass; ++j) {
        const uint32_t v = (raw >> (j * kBypassBits)) & kMaxBypass;
        syms.push_back({(uint16_t)v, (uint16_t)(v + 1), true});
      }
    }
  }
  std::vector<uint32_t> buf(syms.size() + 4);
  uint32_t* p = buf.data() + buf.size();
  uint64_t x = kRansL;
  for (size_t k = syms.size(); k-- > 0;) {
    const Sym& s = syms[k];
    if (s.bypass) enc_put_bits(x, p, s.start, kBypassBits);
    else {
      if (s.range == 0) {
        set_error("vam_rans_encode: zero-frequency symbol (cdf table not normalised)");
        return VAM_EINVAL;
      }
      enc_put(x, p, s.start, s.range, kPrecision);
    }
  }
  *--p = (uint32_t)(x >> 32);
  *--p = (uint32_t)x;
  const long nbytes = (long)((buf.data() + buf.size()) - p) * 4;
  if (nbytes > out_cap) {
    set_error("vam_rans_encode: output buffer too small (%ld > %ld)", nbytes, out_cap);
    return VAM_EINVAL;
  }
  std::memcpy(out, p, (size_t)nbytes);
  return nbytes;
}

// One stream.  layer != NULL: element i is decoded with table 0 unless layer[i] == sel, and only the elements with
// layer[i] == sel are written to out (the layers of a container fill one symbol array).
int decode_one(const uint8_t* in, long n_bytes, const int32_t* indexes, const uint8_t* layer, int sel, long n,
               const int32_t* cdfs, int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs,
               int32_t* out) {
  if (!in || !indexes || !cdfs || !cdf_sizes || !offsets || !out || n < 0 || n_bytes < 8 || (n_bytes & 3)) {
    set_error("vam_rans_decode: bad arguments (stream of %ld bytes)", n_bytes);
    return VAM_EINVAL;
  }
  std::vector<uint32_t> words((size_t)n_bytes / 4);
  std::memcpy(words.data(), in, (size_t)n_bytes);
  const uint32_t* p = words.data();
  const uint32_t* end = p + words.size();
  uint64_t x = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
  p += 2;
  bool ok = true;
  for (long i = 0; i < n; ++i) {
    const bool keep = !layer || layer[i] == sel;
    const int ci = keep ? indexes[i] : 0;
    if (ci < 0 || ci >= n_cdfs) {
      set_error("vam_rans_decode: index %d out of range at %ld", ci, i);
      return VAM_EINVAL;
    }
    const int32_t* cdf = cdfs + (long)ci * cdf_stride;
    const int sz = cdf_sizes[ci];
    const int max_value = sz - 2;
    const uint32_t cum = (uint32_t)(x & ((1u << kPrecision) - 1));
    int s = 0;                                   // first entry > cum, minus one
    while (s + 1 < sz && (uint32_t)cdf[s + 1] <= cum) ++s;
    const uint32_t start = (uint32_t)cdf[s], freq = (uint32_t)(cdf[s + 1] - cdf[s]);
    x = (uint64_t)freq * (x >> kPrecision) + cum - start;
    if (x < kRansL) {
      if (p >= end) { ok = false; break; }
      x = (x << 32) | *p++;
    }
    int32_t value = s;
    if (value == max_value) {
      int32_t val = (int32_t)dec_get_bits(x, p, end, kBypassBits, ok);
      int32_t n_bypass = val;
      while (ok && val == (int32_t)kMaxBypass) {
        val = (int32_t)dec_get_bits(x, p, end, kBypassBits, ok);
        n_bypass += val;
      }
      uint32_t raw = 0;
      for (int j = 0; ok && j < n_bypass; ++j) raw |= dec_get_bits(x, p, end, kBypassBits, ok) << (j * kBypassBits);
      value = (int32_t)(raw >> 1);
      if (raw & 1) value = -value - 1;
      else value += max_value;
    }
    if (!ok) break;
    if (keep) out[i] = value + offsets[ci];
  }
  if (!ok) {
    set_error("vam_rans_decode: bitstream truncated");
    return VAM_EINVAL;
  }
  return VAM_OK;
}

// Tolerant prefix decode (embedded streams).  The decoder reads the words of a stream front to back
// and symbol i depends only on the words consumed up to it, so the first floor(n_bytes / 4) words of a stream decode its
// leading symbols.  A symbol counts when its whole step fits the prefix: the table symbol, its renormalisation word and
// every bypass nibble with theirs (what decode_one needs before it writes the symbol).  Returns the number of leading
// symbols (< 0 on bad arguments); out (may be NULL) receives them, the rest of out is left untouched.  marks (may be
// NULL): n_marks sorted symbol counts; mark_bytes[m] = the bytes consumed when marks[m] symbols were complete (0 for a
// count of 0) = the shortest prefix, in whole words, that still decodes that many; marks the prefix does not reach stay
// at -1.
long decode_prefix_one(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                       const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* out, const long* marks,
                       int n_marks, long* mark_bytes) {
  if ((!in && n_bytes > 0) || (!indexes && n > 0) || !cdfs || !cdf_sizes || !offsets || n < 0 || n_bytes < 0 || n_cdfs < 1 ||
      n_marks < 0 || (n_marks > 0 && (!marks || !mark_bytes))) {
    set_error("vam_rans_decode_prefix: bad arguments (prefix of %ld bytes)", n_bytes);
    return VAM_EINVAL;
  }
  int m = 0;
  for (int q = 0; q < n_marks; ++q) {
    if (marks[q] < 0 || (q > 0 && marks[q] < marks[q - 1])) {
      set_error("vam_rans_prefix_bytes: counts must be >= 0 and sorted, got %ld at %d", marks[q], q);
      return VAM_EINVAL;
    }
    mark_bytes[q] = -1;
  }
  while (m < n_marks && marks[m] == 0) mark_bytes[m++] = 0;
  if (n_bytes < 8) return 0;
  std::vector<uint32_t> words((size_t)n_bytes / 4);
  std::memcpy(words.data(), in, words.size() * 4);
  const uint32_t* p = words.data();
  const uint32_t* end = p + words.size();
  uint64_t x = (uint64_t)p[0] | ((uint64_t)p[1] << 32);
  p += 2;
  long count = 0;
  for (long i = 0; i < n; ++i) {
    const int ci = indexes[i];
    if (ci < 0 || ci >= n_cdfs) {
      set_error("vam_rans_decode_prefix: index %d out of range at %ld", ci, i);
      return VAM_EINVAL;
    }
    const int32_t* cdf = cdfs + (long)ci * cdf_stride;
    const int sz = cdf_sizes[ci];
    const int max_value = sz - 2;
    if (max_value < 0 || max_value + 1 >= cdf_stride) {
      set_error("vam_rans_decode_prefix: cdf size %d invalid for table %d", sz, ci);
      return VAM_EINVAL;
    }
    const uint32_t cum = (uint32_t)(x & ((1u << kPrecision) - 1));
    int s = 0;
    while (s + 1 < sz && (uint32_t)cdf[s + 1] <= cum) ++s;
    const uint32_t start = (uint32_t)cdf[s], freq = (uint32_t)(cdf[s + 1] - cdf[s]);
    x = (uint64_t)freq * (x >> kPrecision) + cum - start;
    if (x < kRansL) {
      if (p >= end) break;
      x = (x << 32) | *p++;
    }
    bool ok = true;
    int32_t value = s;
    if (value == max_value) {
      int32_t val = (int32_t)dec_get_bits(x, p, end, kBypassBits, ok);
      int32_t n_bypass = val;
      while (ok && val == (int32_t)kMaxBypass) {
        val = (int32_t)dec_get_bits(x, p, end, kBypassBits, ok);
        n_bypass += val;
      }
      uint32_t raw = 0;
      for (int j = 0; ok && j < n_bypass; ++j) {
        const uint32_t nib = dec_get_bits(x, p, end, kBypassBits, ok);
        if (j < 32 / kBypassBits) raw |= nib << (j * kBypassBits);
      }
      value = (int32_t)(raw >> 1);
      if (raw & 1) value = -value - 1;
      else value += max_value;
    }
    if (!ok) break;
    if (out) out[i] = value + offsets[ci];
    count = i + 1;
    while (m < n_marks && marks[m] <= count) mark_bytes[m++] = (long)(p - words.data()) * 4;
  }
  return count;
}

// Runs job(i) for i in [0, n_jobs) on min(n_threads, n_jobs) threads (the caller's thread included).  Jobs write
// disjoint memory.  The first failure (lowest job index) becomes this thread's vam_last_error.
template <class F>
int run_jobs(int n_jobs, int n_threads, const char* what, F&& job) {
  if (n_jobs < 0 || n_threads < 1) {
    set_error("%s: bad arguments (%d streams, %d threads)", what, n_jobs, n_threads);
    return VAM_EINVAL;
  }
  const int nt = std::min(std::min(n_threads, VAM_RANS_MAX_THREADS), std::max(n_jobs, 1));
  std::atomic<int> next{0};
  std::mutex mu;
  int bad = -1;
  std::string msg;
  auto worker = [&]() {
    for (int i = next++; i < n_jobs; i = next++) {
      if (job(i) >= 0) continue;
      std::lock_guard<std::mutex> g(mu);
      if (bad < 0 || i < bad) { bad = i; msg = vam_last_error(); }
    }
  };
  std::vector<std::thread> pool;
  pool.reserve(nt - 1);
  for (int t = 1; t < nt; ++t) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
  if (bad >= 0) {
    set_error("%s: stream %d: %s", what, bad, msg.c_str());
    return VAM_EINVAL;
  }
  return VAM_OK;
}

}  // namespace

extern "C" {

long vam_rans_encode(const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                     const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long out_cap) {
  return encode_one(symbols, indexes, nullptr, 0, n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out, out_cap);
}

int vam_rans_decode(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs,
                    int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int32_t* out) {
  return decode_one(in, n_bytes, indexes, nullptr, 0, n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out);
}

int vam_rans_encode_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs, int cdf_stride,
                            const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int n_threads) {
  if (n_streams > 0 && !streams) {
    set_error("vam_rans_encode_streams: bad arguments");
    return VAM_EINVAL;
  }
  return run_jobs(n_streams, n_threads, "vam_rans_encode_streams", [&](int i) -> long {
    vam_rans_stream& s = streams[i];
    s.n_bytes = encode_one(s.symbols, s.indexes, s.layer, s.sel, s.n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                           s.bytes, s.capacity);
    return s.n_bytes;
  });
}

int vam_rans_decode_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs, int cdf_stride,
                            const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int n_threads) {
  if (n_streams > 0 && !streams) {
    set_error("vam_rans_decode_streams: bad arguments");
    return VAM_EINVAL;
  }
  return run_jobs(n_streams, n_threads, "vam_rans_decode_streams", [&](int i) -> long {
    const vam_rans_stream& s = streams[i];
    return decode_one(s.bytes, s.n_bytes, s.indexes, s.layer, s.sel, s.n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                      s.symbols_out);
  });
}

int vam_rans_decode_prefix_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs, int cdf_stride,
                                   const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int n_threads,
                                   long* counts_out) {
  if (n_streams > 0 && (!streams || !counts_out)) {
    set_error("vam_rans_decode_prefix_streams: bad arguments");
    return VAM_EINVAL;
  }
  return run_jobs(n_streams, n_threads, "vam_rans_decode_prefix_streams", [&](int i) -> long {
    const vam_rans_stream& s = streams[i];
    if (s.layer) {
      set_error("vam_rans_decode_prefix_streams: an embedded stream carries no layer selection");
      return VAM_EINVAL;
    }
    return counts_out[i] = decode_prefix_one(s.bytes, s.n_bytes, s.indexes, s.n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                                             s.symbols_out, nullptr, 0, nullptr);
  });
}

int vam_rans_prefix_bytes(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                          const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, const long* counts, int n_counts,
                          long* bytes_out) {
  const long got = decode_prefix_one(in, n_bytes, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, nullptr, counts,
                                     n_counts, bytes_out);
  if (got < 0) return (int)got;
  for (int q = 0; q < n_counts; ++q)
    if (bytes_out[q] < 0) {
      set_error("vam_rans_prefix_bytes: %ld symbols asked for, the %ld bytes given decode %ld of %ld", counts[q], n_bytes, got, n);
      return VAM_EINVAL;
    }
  return VAM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- interleaved lanes (rans_core.h)
// The host exports of the interleaved format drive rans_core.h's one-thread functions; K = 1 gives the strings, counts
// and byte marks of the functions above.
namespace {

namespace R = vam_rans;

const char* ilv_status_text(int st) {
  switch (st) {
    case R::kBadIndex: return "index out of range";
    case R::kBadTable: return "cdf size invalid";
    case R::kOverflow: return "output buffer too small";
    case R::kZeroFreq: return "zero-frequency symbol (cdf table not normalised)";
    case R::kBadStream: return "bad arguments (lanes is a power of two in 1 .. 64, the string word-aligned)";
    default: return "unknown status";
  }
}

long ilv_encode_one(const char* what, const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                    const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long out_cap, int lanes) {
  if (!symbols || !indexes || !cdfs || !cdf_sizes || !offsets || !out || n < 0 || n > (1l << 28) || n_cdfs < 1) {
    set_error("%s: bad arguments", what);
    return VAM_EINVAL;
  }
  if (!R::lanes_valid(lanes)) {
    set_error("%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
    return VAM_EINVAL;
  }
  std::vector<uint32_t> region((size_t)R::interleaved_cap_words(n, lanes));
  long words = 0;
  const int32_t st = R::interleaved_encode(symbols, indexes, n, R::Flat{}, lanes, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                                           region.data(), (long)region.size(), &words);
  if (st) {
    set_error("%s: %s", what, ilv_status_text(st));
    return VAM_EINVAL;
  }
  if (words * 4 > out_cap) {
    set_error("%s: output buffer too small (%ld > %ld)", what, words * 4, out_cap);
    return VAM_EINVAL;
  }
  std::memcpy(out, region.data() + region.size() - words, (size_t)words * 4);
  return words * 4;
}

// Returns the count (< 0: bad arguments, or a status when status_out is NULL).
long ilv_decode_one(const char* what, const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs,
                    int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes, int32_t* out,
                    int32_t* status_out, const long* marks, int n_marks, long* mark_bytes) {
  if (status_out) *status_out = 0;
  if ((!in && n_bytes > 0) || (!indexes && n > 0) || !cdfs || !cdf_sizes || !offsets || n < 0 || n_bytes < 0 || n_cdfs < 1 ||
      n_marks < 0 || (n_marks > 0 && (!marks || !mark_bytes))) {
    set_error("%s: bad arguments (prefix of %ld bytes)", what, n_bytes);
    return VAM_EINVAL;
  }
  if (!R::lanes_valid(lanes)) {
    set_error("%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
    return VAM_EINVAL;
  }
  for (int q = 0; q < n_marks; ++q)
    if (marks[q] < 0 || (q > 0 && marks[q] < marks[q - 1])) {
      set_error("%s: counts must be >= 0 and sorted, got %ld at %d", what, marks[q], q);
      return VAM_EINVAL;
    }
  std::vector<uint32_t> words((size_t)n_bytes / 4);         // aligned copy of the whole words
  if (!words.empty()) std::memcpy(words.data(), in, words.size() * 4);
  long available = 0;
  const int32_t st = R::interleaved_decode(words.empty() ? nullptr : words.data(), (long)words.size() * 4, lanes, indexes, n, R::Flat{},
                                           R::Int32Rows{cdfs, cdf_stride}, cdf_stride, cdf_sizes, offsets, n_cdfs, out, &available,
                                           marks, n_marks, mark_bytes);
  if (status_out) *status_out = st;
  else if (st) {
    set_error("%s: %s after %ld symbols", what, ilv_status_text(st), available);
    return VAM_EINVAL;
  }
  return available;
}

// The resumable decode of one stream: `in` holds the string from byte 4 * ck->pos on.  Returns the count
// (< 0: refused by message, nothing written); *status_out receives the status that ended the stream.
long ilv_resume_one(const char* what, const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs,
                    int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes, int32_t* out,
                    vam_rans_checkpoint* ck, int32_t* status_out) {
  if (n_bytes < 0 || n < 0) {
    set_error("%s: bad arguments (%ld bytes for %ld symbols)", what, n_bytes, n);
    return VAM_EINVAL;
  }
  if ((!in && n_bytes > 0) || (!indexes && n > 0) || !cdfs || !cdf_sizes || !offsets || n_cdfs < 1 || !ck || !ck->states) {
    set_error("%s: bad arguments (need the bytes, indexes, tables and a checkpoint with its states)", what);
    return VAM_EINVAL;
  }
  if (!R::lanes_valid(lanes)) {
    set_error("%s: lanes is a power of two in 1 .. %d, got %d", what, R::kMaxLanes, lanes);
    return VAM_EINVAL;
  }
  if ((uintptr_t)ck->states & 7) {
    set_error("%s: the checkpoint's states are 64-bit words, the pointer is misaligned", what);
    return VAM_EINVAL;
  }
  if (!R::checkpoint_valid(ck->done, ck->pos, n, lanes)) {
    set_error("%s: impossible checkpoint (done = %ld, pos = %ld for %ld symbols on %d lanes: done is a multiple of lanes or n, "
              "and pos >= 2 * lanes once done > 0)", what, ck->done, ck->pos, n, lanes);
    return VAM_EINVAL;
  }
  std::vector<uint32_t> words((size_t)n_bytes / 4);         // aligned copy of the whole words
  if (!words.empty()) std::memcpy(words.data(), in, words.size() * 4);
  long available = 0, done = ck->done, pos = ck->pos;
  const int32_t st = R::interleaved_resume(words.empty() ? nullptr : words.data(), (long)words.size() * 4, lanes, indexes, n, R::Flat{},
                                           R::Int32Rows{cdfs, cdf_stride}, cdf_stride, cdf_sizes, offsets, n_cdfs, out, &available,
                                           &done, &pos, ck->states);
  ck->done = done;
  ck->pos = pos;
  *status_out = st;
  return available;
}

}  // namespace

extern "C" {

long vam_rans_interleaved_resume(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                                 const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes, int32_t* out,
                                 vam_rans_checkpoint* checkpoint, int32_t* status_out) {
  const char* what = "vam_rans_interleaved_resume";
  int32_t st = 0;
  const long got = ilv_resume_one(what, in, n_bytes, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, lanes, out, checkpoint, &st);
  if (got < 0) return got;
  if (status_out) *status_out = st;
  else if (st) {
    set_error("%s: %s after %ld symbols", what, ilv_status_text(st), got);
    return VAM_EINVAL;
  }
  return got;
}

int vam_rans_interleaved_resume_streams(vam_rans_stream* streams, vam_rans_checkpoint* checkpoints, int n_streams, const int32_t* cdfs,
                                        int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes,
                                        int n_threads, long* counts_out, int32_t* status_out) {
  const char* what = "vam_rans_interleaved_resume_streams";
  if (n_streams > 0 && (!streams || !checkpoints || !counts_out || !status_out)) {
    set_error("%s: bad arguments", what);
    return VAM_EINVAL;
  }
  return run_jobs(n_streams, n_threads, what, [&](int i) -> long {
    const vam_rans_stream& s = streams[i];
    if (s.layer) {
      set_error("%s: an embedded stream carries no layer selection", what);
      return VAM_EINVAL;
    }
    const long got = ilv_resume_one("vam_rans_interleaved_resume", s.bytes, s.n_bytes, s.indexes, s.n, cdfs, cdf_stride, cdf_sizes,
                                    offsets, n_cdfs, lanes, s.symbols_out, checkpoints + i, status_out + i);
    if (got < 0) return got;
    counts_out[i] = got;
    if (status_out[i]) {
      set_error("vam_rans_interleaved_resume: %s after %ld symbols", ilv_status_text(status_out[i]), got);
      return VAM_EINVAL;
    }
    return got;
  });
}

long vam_rans_interleaved_encode(const int32_t* symbols, const int32_t* indexes, long n, const int32_t* cdfs, int cdf_stride,
                                 const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, uint8_t* out, long out_cap, int lanes) {
  return ilv_encode_one("vam_rans_interleaved_encode", symbols, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs, out, out_cap,
                        lanes);
}

int vam_rans_interleaved_encode_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs, int cdf_stride,
                                        const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes, int n_threads) {
  if (n_streams > 0 && !streams) {
    set_error("vam_rans_interleaved_encode_streams: bad arguments");
    return VAM_EINVAL;
  }
  return run_jobs(n_streams, n_threads, "vam_rans_interleaved_encode_streams", [&](int i) -> long {
    vam_rans_stream& s = streams[i];
    if (s.layer) {
      set_error("vam_rans_interleaved_encode_streams: an embedded stream carries no layer selection");
      return s.n_bytes = VAM_EINVAL;
    }
    return s.n_bytes = ilv_encode_one("vam_rans_interleaved_encode", s.symbols, s.indexes, s.n, cdfs, cdf_stride, cdf_sizes, offsets,
                                      n_cdfs, s.bytes, s.capacity, lanes);
  });
}

long vam_rans_interleaved_decode_prefix(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs,
                                        int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes,
                                        int32_t* out, int32_t* status_out) {
  return ilv_decode_one("vam_rans_interleaved_decode_prefix", in, n_bytes, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets, n_cdfs,
                        lanes, out, status_out, nullptr, 0, nullptr);
}

int vam_rans_interleaved_decode_prefix_streams(vam_rans_stream* streams, int n_streams, const int32_t* cdfs, int cdf_stride,
                                               const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes, int n_threads,
                                               long* counts_out) {
  if (n_streams > 0 && (!streams || !counts_out)) {
    set_error("vam_rans_interleaved_decode_prefix_streams: bad arguments");
    return VAM_EINVAL;
  }
  return run_jobs(n_streams, n_threads, "vam_rans_interleaved_decode_prefix_streams", [&](int i) -> long {
    const vam_rans_stream& s = streams[i];
    if (s.layer) {
      set_error("vam_rans_interleaved_decode_prefix_streams: an embedded stream carries no layer selection");
      return VAM_EINVAL;
    }
    return counts_out[i] = ilv_decode_one("vam_rans_interleaved_decode_prefix", s.bytes, s.n_bytes, s.indexes, s.n, cdfs, cdf_stride,
                                          cdf_sizes, offsets, n_cdfs, lanes, s.symbols_out, nullptr, nullptr, 0, nullptr);
  });
}

int vam_rans_interleaved_prefix_bytes(const uint8_t* in, long n_bytes, const int32_t* indexes, long n, const int32_t* cdfs,
                                      int cdf_stride, const int32_t* cdf_sizes, const int32_t* offsets, int n_cdfs, int lanes,
                                      const long* counts, int n_counts, long* bytes_out) {
  const long got = ilv_decode_one("vam_rans_interleaved_prefix_bytes", in, n_bytes, indexes, n, cdfs, cdf_stride, cdf_sizes, offsets,
                                  n_cdfs, lanes, nullptr, nullptr, counts, n_counts, bytes_out);
  if (got < 0) return (int)got;
  for (int q = 0; q < n_counts; ++q)
    if (bytes_out[q] < 0) {
      set_error("vam_rans_interleaved_prefix_bytes: %ld symbols asked for, the %ld bytes given decode %ld of %ld", counts[q], n_bytes,
                got, n);
      return VAM_EINVAL;
    }
  return VAM_OK;
}

}  // extern "C"
