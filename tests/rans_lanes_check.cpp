// Stand-alone check of the lane-split streams of csrc/rans_core.h for a sanitizer build
// (tests/test_rans_lanes_cpu.py compiles it with -fsanitize=address,undefined and runs it as its own process): round
// trips over the n x K grid through flat and NHWC addressing, every truncation length of a K = 8 string, every
// single-word corruption of its header, strings of random bytes, and the packed 16-bit table search against a linear
// scan.  Every buffer is a heap block of exactly the size the core is told, so a read or write outside one stops the
// program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "rans_core.h"

namespace R = vam_rans;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) { std::printf("rans_lanes_check: FAILED %s (line %d)\n", #cond, __LINE__); std::exit(1); } \
  } while (0)

struct Tables {
  int n_cdfs, stride;
  std::vector<int32_t> cdf, sizes, offsets;
};

// n tables of 3 .. max_syms symbols plus the escape, random increasing CDFs from 0 to 65536
static Tables make_tables(int n, int max_syms) {
  Tables t{n, max_syms + 2, {}, {}, {}};
  t.cdf.assign((size_t)n * t.stride, 0);
  for (int k = 0; k < n; ++k) {
    const int syms = 3 + (int)(rnd() % (uint32_t)(max_syms - 2));
    uint32_t left = 65536 - syms;
    int32_t c = 0;
    for (int j = 0; j < syms; ++j) {
      const uint32_t extra = j == syms - 1 ? left : rnd() % (left / 2 + 1);
      t.cdf[(size_t)k * t.stride + j] = c;
      c += (int32_t)(1 + extra);
      left -= extra;
    }
    t.cdf[(size_t)k * t.stride + syms] = c;
    CHECK(c == 65536);
    t.sizes.push_back(syms + 1);
    t.offsets.push_back(-(syms / 2));
  }
  return t;
}

template <class T>
static std::unique_ptr<T[]> exact(const T* src, size_t n) {
  std::unique_ptr<T[]> p(new T[n ? n : 1]);
  if (n) std::memcpy(p.get(), src, n * sizeof(T));
  return p;
}

static void fill_symbols(const Tables& t, long n, std::vector<int32_t>& sym, std::vector<int32_t>& idx) {
  sym.resize(n); idx.resize(n);
  for (long i = 0; i < n; ++i) {
    const int ci = (int)(rnd() % (uint32_t)t.n_cdfs);
    idx[i] = ci;
    const int mx = t.sizes[ci] - 2;
    int32_t v = (int32_t)(rnd() % (uint32_t)(mx > 0 ? mx : 1));
    const uint32_t r = rnd() % 16;
    if (r == 0) v = mx + (int32_t)((rnd() >> 2) >> (rnd() % 30));      // escapes of every nibble count, both signs
    if (r == 1) v = -1 - (int32_t)((rnd() >> 2) >> (rnd() % 30));
    if (r == 2) v = mx;
    sym[i] = v + t.offsets[ci];
  }
}

// The string of a stream: the header (K > 1) and the lanes, each from a region of exactly the budgeted size.
template <class A>
static std::vector<uint32_t> encode(const Tables& t, const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n,
                                    const A& at, int K) {
  const long cap = R::lane_cap_words(n, K);
  std::unique_ptr<uint32_t[]> regions(new uint32_t[cap * K]);
  std::unique_ptr<long[]> words(new long[K]);
  std::unique_ptr<int32_t[]> status(new int32_t[K]);
  CHECK(R::lanes_encode_stream(sym, idx, layer, sel, n, at, K, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs,
                               regions.get(), cap, words.get(), status.get()) == R::kOk);
  std::vector<uint32_t> out;
  for (int j = 0; j < K && K > 1; ++j) out.push_back((uint32_t)words[j]);
  for (int j = 0; j < K; ++j) {
    CHECK(status[j] == R::kOk && words[j] >= 2 && words[j] <= cap);
    if (R::lane_elements(n, j, K) == 0) CHECK(words[j] == 2);
    out.insert(out.end(), regions.get() + (j + 1) * cap - words[j], regions.get() + (j + 1) * cap);
  }
  return out;
}

template <class A>
static int32_t decode(const Tables& t, const uint32_t* words, long n_bytes, int K, const int32_t* idx, const uint8_t* layer, int sel,
                      long n, const A& at, int32_t* out, int32_t* lane_status) {
  auto w = exact(words, (size_t)(n_bytes / 4));              // whole words only: what the kernels may touch
  return R::lanes_decode_stream(n_bytes >= 4 ? w.get() : nullptr, n_bytes, K, idx, layer, sel, n, at, t.cdf.data(), t.stride,
                                t.sizes.data(), t.offsets.data(), t.n_cdfs, out, lane_status);
}

static const int kLanes[] = {1, 2, 8, 64};

static void round_trips(const Tables& t) {
  const long lengths[] = {0, 1, 2, 63, 64, 65, 512, 4097};
  for (long n : lengths)
    for (int K : kLanes) {
      std::vector<int32_t> sym, idx;
      fill_symbols(t, n, sym, idx);
      auto s = exact(sym.data(), (size_t)n);
      auto ix = exact(idx.data(), (size_t)n);
      std::vector<uint8_t> layer(n);
      for (auto& l : layer) l = (uint8_t)(rnd() % 3);
      auto ly = exact(layer.data(), (size_t)n);
      for (int pass = 0; pass < 2; ++pass) {
        const uint8_t* lp = pass ? ly.get() : nullptr;
        const auto words = encode(t, s.get(), ix.get(), lp, 1, n, R::Flat{}, K);
        if (K == 1) {                                        // the existing stream, byte for byte
          const long cap = 2 * n + 16;
          std::unique_ptr<uint32_t[]> region(new uint32_t[cap]);
          long nw = 0;
          CHECK(R::encode_stream(s.get(), ix.get(), lp, 1, n, R::Flat{}, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(),
                                 t.n_cdfs, region.get(), cap, &nw) == R::kOk);
          CHECK(nw == (long)words.size() && !std::memcmp(region.get() + cap - nw, words.data(), (size_t)nw * 4));
        }
        std::unique_ptr<int32_t[]> out(new int32_t[n ? n : 1]), st(new int32_t[K]);
        for (long i = 0; i < n; ++i) out[i] = -77;
        CHECK(decode(t, words.data(), (long)words.size() * 4, K, ix.get(), lp, 1, n, R::Flat{}, out.get(), st.get()) == R::kOk);
        for (int j = 0; j < K; ++j) CHECK(st[j] == R::kOk);
        for (long i = 0; i < n; ++i) CHECK(out[i] == (!lp || layer[i] == 1 ? sym[i] : -77));
      }
    }
  // an NHWC window, with and without an index buffer: [2, 3, 5, 7], c0 = 2, C = 4
  const int h = 3, w = 5, ld = 7, c0 = 2, C = 4;
  const long hw = h * w, n = hw * C, total = 2 * hw * ld;
  for (int K : kLanes)
    for (int image = 0; image < 2; ++image)
      for (int with_idx = 0; with_idx < 2; ++with_idx) {
        std::unique_ptr<int32_t[]> sym(new int32_t[total]), idx(new int32_t[total]), out(new int32_t[total]), st(new int32_t[K]);
        for (long i = 0; i < total; ++i) {
          idx[i] = (int32_t)(rnd() % (uint32_t)t.n_cdfs);
          sym[i] = t.offsets[with_idx ? idx[i] : 0] + (int32_t)(rnd() % 5) - 1;
          out[i] = -77;
        }
        const long img = image * hw * ld + c0;
        const R::Nhwc at{hw, ld};
        const int32_t* ip = with_idx ? idx.get() + img : nullptr;
        const auto words = encode(t, sym.get() + img, ip, nullptr, 0, n, at, K);
        CHECK(decode(t, words.data(), (long)words.size() * 4, K, ip, nullptr, 0, n, at, out.get() + img, st.get()) == R::kOk);
        for (long i = 0; i < total; ++i) {
          const long pix = i / ld, c = i % ld;
          const bool inside = pix / hw == image && c >= c0 && c < c0 + C;
          CHECK(out[i] == (inside ? sym[i] : -77));
        }
      }
}

// The decoded prefix of every lane is right, and from a lane's failure on its elements are 0.
static void check_lanes_output(const std::vector<int32_t>& sym, const int32_t* out, const int32_t* st, long n, int K) {
  for (int j = 0; j < K; ++j) {
    long i = j;
    while (i < n && out[i] == sym[i]) i += K;
    if (st[j] == R::kOk) CHECK(i >= n);
    for (; i < n; i += K) CHECK(out[i] == 0);
  }
}

static void truncations_and_headers(const Tables& t) {
  const int K = 8;
  const long n = 1000;
  std::vector<int32_t> sym, idx;
  fill_symbols(t, n, sym, idx);
  auto ix = exact(idx.data(), (size_t)n);
  const auto words = encode(t, sym.data(), ix.get(), nullptr, 0, n, R::Flat{}, K);
  const long full = (long)words.size() * 4;
  std::unique_ptr<int32_t[]> out(new int32_t[n]), st(new int32_t[K]);
  // every length with the header as it is: the lengths no longer add up, every lane is refused, all zeros
  for (long cut = 0; cut < full; ++cut) {
    if (cut > 64 && (cut & 3) && cut % 101) continue;         // unaligned lengths: all near the header, a sample beyond
    for (long i = 0; i < n; ++i) out[i] = -77;
    CHECK(decode(t, words.data(), cut, K, ix.get(), nullptr, 0, n, R::Flat{}, out.get(), st.get()) == R::kBadStream);
    for (int j = 0; j < K; ++j) CHECK(st[j] == R::kBadStream);
    for (long i = 0; i < n; ++i) CHECK(out[i] == 0);
  }
  // every word-aligned length with the header adjusted so the sum matches: the lanes before the cut decode, the cut lane
  // is truncated (or too short for a final state: the header is refused), the lanes after it are empty streams
  for (long cut_words = K; cut_words < (long)words.size(); ++cut_words) {
    std::vector<uint32_t> part(words.begin(), words.begin() + cut_words);
    long at = K;
    int cut_lane = -1;
    bool refused = false;
    for (int j = 0; j < K; ++j) {
      const long len = words[j], have = cut_words - at < 0 ? 0 : (cut_words - at < len ? cut_words - at : len);
      if (have < len && cut_lane < 0) cut_lane = j;
      part[j] = (uint32_t)have;
      if (have < 2) refused = true;
      at += len;
    }
    for (long i = 0; i < n; ++i) out[i] = -77;
    const int32_t rc = decode(t, part.data(), cut_words * 4, K, ix.get(), nullptr, 0, n, R::Flat{}, out.get(), st.get());
    if (refused) {
      CHECK(rc == R::kBadStream);
      for (long i = 0; i < n; ++i) CHECK(out[i] == 0);
      continue;
    }
    CHECK(cut_lane == K - 1 && rc == R::kTruncated && st[cut_lane] == R::kTruncated);
    for (int j = 0; j < cut_lane; ++j) CHECK(st[j] == R::kOk);
    check_lanes_output(sym, out.get(), st.get(), n, K);
  }
  // every single-word corruption of the header
  const uint32_t values[] = {0u, 1u, 2u, 3u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
  for (int j = 0; j < K; ++j)
    for (int v = 0; v < 12; ++v) {
      std::vector<uint32_t> bad(words);
      bad[j] = v < 8 ? values[v] : v == 8 ? words[j] + 1 : v == 9 ? words[j] - 1 : rnd();
      if (bad[j] == words[j]) continue;
      for (long i = 0; i < n; ++i) out[i] = -77;
      CHECK(decode(t, bad.data(), full, K, ix.get(), nullptr, 0, n, R::Flat{}, out.get(), st.get()) == R::kBadStream);
      for (long i = 0; i < n; ++i) CHECK(out[i] == 0);
    }
  // two header words changed so that the sum still matches: the lanes are cut in the wrong places, a status or wrong
  // symbols, never a read outside the string
  for (int j = 0; j + 1 < K; ++j) {
    std::vector<uint32_t> bad(words);
    const uint32_t d = 1 + rnd() % (bad[j] - 2 > 0 ? bad[j] - 2 : 1);
    if (bad[j] - d < 2) continue;
    bad[j] -= d; bad[j + 1] += d;
    const int32_t rc = decode(t, bad.data(), full, K, ix.get(), nullptr, 0, n, R::Flat{}, out.get(), st.get());
    CHECK(rc >= 0 && rc <= R::kBadStream);
  }
  // a wrong K on a good string
  for (int k2 : kLanes) {
    std::unique_ptr<int32_t[]> st2(new int32_t[k2]);
    const int32_t rc = decode(t, words.data(), full, k2, ix.get(), nullptr, 0, n, R::Flat{}, out.get(), st2.get());
    CHECK(rc >= 0 && rc <= R::kBadStream && (k2 != K || rc == R::kOk));
  }
}

static void random_bytes(const Tables& t) {
  for (int trial = 0; trial < 600; ++trial) {
    const int K = kLanes[rnd() % 4];
    const long n = 1 + rnd() % 4096, n_words = rnd() % 600;
    std::vector<uint32_t> words((size_t)n_words);
    for (auto& v : words) v = rnd() ^ (rnd() << 16);
    if (trial % 3 == 0) for (auto& v : words) v |= 0xFFFF0000u >> (rnd() % 16);   // long runs of escapes and count nibbles
    if (trial % 2 == 0 && K > 1 && n_words >= 3l * K) {      // a header that is accepted, random lanes behind it
      long left = n_words - K;
      for (int j = 0; j < K; ++j) {
        const long len = j == K - 1 ? left : 2 + (long)(rnd() % (uint32_t)(left - 2 * (K - j) + 1));
        words[j] = (uint32_t)len;
        left -= len;
      }
    }
    std::vector<int32_t> idx(n);
    for (auto& v : idx) v = (int32_t)(rnd() % (uint32_t)t.n_cdfs);
    auto ix = exact(idx.data(), (size_t)n);
    std::unique_ptr<int32_t[]> out(new int32_t[n]), st(new int32_t[K]);
    const long n_bytes = n_words * 4 + (trial % 7 == 0 ? rnd() % 4 : 0);          // also lengths that are not whole words
    auto padded = words;
    padded.push_back(0);
    const int32_t rc = decode(t, padded.data(), n_bytes, K, ix.get(), nullptr, 0, n, R::Flat{}, out.get(), st.get());
    CHECK(rc >= 0 && rc <= R::kBadStream);
  }
}

// TableSearch over a packed 16-bit table (terminal implied) and over the int32 row against the host's linear scan.
static void searches(const Tables& t) {
  for (int k = 0; k < t.n_cdfs; ++k) {
    const int sz = t.sizes[k];
    const int32_t* row = t.cdf.data() + (size_t)k * t.stride;
    std::unique_ptr<uint16_t[]> packed(new uint16_t[sz - 1]);
    for (int j = 0; j < sz - 1; ++j) packed[j] = (uint16_t)row[j];
    auto exact_row = exact(row, (size_t)sz);
    for (int trial = 0; trial < 2000; ++trial) {
      const uint32_t cum = trial < sz ? (uint32_t)row[trial] - (trial && (trial & 1)) : rnd() & 0xFFFFu;
      if (cum > 0xFFFFu) continue;
      int s = 0;
      while (s + 1 < sz - 1 && (uint32_t)row[s + 1] <= cum) ++s;             // the scan of rans.cpp, clamped to sz - 2
      uint32_t s0, f0, s1, f1;
      CHECK((R::TableSearch<uint16_t>{packed.get(), sz, true})(cum, s0, f0) == s);
      CHECK((R::TableSearch<int32_t>{exact_row.get(), sz, false})(cum, s1, f1) == s);
      CHECK(s0 == (uint32_t)row[s] && f0 == (uint32_t)(row[s + 1] - row[s]) && s1 == s0 && f1 == f0);
    }
  }
}

int main() {
  for (int round = 0; round < 3; ++round) {
    const Tables t = make_tables(round == 0 ? 5 : 64, round == 2 ? 3000 : 40);
    round_trips(t);
    truncations_and_headers(t);
    random_bytes(t);
    searches(t);
  }
  std::printf("rans_lanes_check: ok\n");
  return 0;
}
