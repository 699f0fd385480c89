// Stand-alone check of the interleaved-lanes streams of csrc/rans_core.h for a sanitizer build
// (tests/test_rans_interleaved_cpu.py compiles it with -fsanitize=address,undefined and runs it as its own process):
// encode, tolerant decode and marks over the n x K grid, K = 1 against encode_stream, every byte length of two strings,
// corrupted indexes and states, strings of random bytes.  Every buffer is a heap block of exactly the size the core is
// told, so a read or write outside one stops the program.
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
    if (!(cond)) { std::printf("rans_interleaved_check: FAILED %s (line %d)\n", #cond, __LINE__); std::exit(1); } \
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
    const uint32_t r = rnd() % 8;
    if (r == 0) v = mx + (int32_t)((rnd() >> 2) >> (rnd() % 30));      // escapes of every nibble count, both signs
    if (r == 1) v = -1 - (int32_t)((rnd() >> 2) >> (rnd() % 30));
    if (r == 2) v = mx;
    sym[i] = v + t.offsets[ci];
  }
}

static std::vector<uint32_t> encode(const Tables& t, const std::vector<int32_t>& sym, const std::vector<int32_t>& idx, int K) {
  const long n = (long)sym.size(), cap = R::interleaved_cap_words(n, K);
  auto s = exact(sym.data(), (size_t)n);
  auto i = exact(idx.data(), (size_t)n);
  std::unique_ptr<uint32_t[]> region(new uint32_t[cap]);
  long words = 0;
  CHECK(R::interleaved_encode(s.get(), i.get(), n, R::Flat{}, K, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs,
                              region.get(), cap, &words) == R::kOk);
  CHECK(words >= 2 * K && words <= cap);
  return std::vector<uint32_t>(region.get() + cap - words, region.get() + cap);
}

// The tolerant decode of the first n_bytes bytes; out has exactly n entries.
static int32_t decode(const Tables& t, const std::vector<uint32_t>& str, long n_bytes, int K, const std::vector<int32_t>& idx,
                      int32_t* out, long* available, const long* marks = nullptr, int n_marks = 0, long* mark_bytes = nullptr) {
  auto w = exact(str.data(), (size_t)(n_bytes / 4));           // whole words only: what the core may touch
  auto i = exact(idx.data(), idx.size());
  return R::interleaved_decode(n_bytes >= 4 ? w.get() : nullptr, n_bytes, K, i.get(), (long)idx.size(), R::Flat{},
                               R::Int32Rows{t.cdf.data(), t.stride}, t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs, out, available,
                               marks, n_marks, mark_bytes);
}

static const int kLanes[] = {1, 2, 8, 64};
static const int32_t kFill = -777777;

static void grid(const Tables& t) {
  const long lengths[] = {0, 1, 12, 63, 64, 65, 1000};
  for (long n : lengths)
    for (int K : kLanes) {
      std::vector<int32_t> sym, idx;
      fill_symbols(t, n, sym, idx);
      const auto str = encode(t, sym, idx, K);
      if (K == 1) {                                            // the stream of encode_stream, word for word
        const long cap = 2 * n + 16;
        std::unique_ptr<uint32_t[]> region(new uint32_t[cap]);
        long words = 0;
        CHECK(R::encode_stream(sym.data(), idx.data(), nullptr, 0, n, R::Flat{}, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(),
                               t.n_cdfs, region.get(), cap, &words) == R::kOk);
        CHECK(words == (long)str.size() && std::memcmp(region.get() + cap - words, str.data(), (size_t)words * 4) == 0);
      }
      std::unique_ptr<int32_t[]> out(new int32_t[n ? n : 1]);
      long avail = -1;
      long marks[4] = {0, n > 0 ? 1 : 0, n / 3, n};
      if (marks[2] < marks[1]) marks[2] = marks[1];            // sorted
      long mb[4];
      CHECK(decode(t, str, (long)str.size() * 4, K, idx, out.get(), &avail, marks, 4, mb) == R::kOk);
      CHECK(avail == n && (n == 0 || std::memcmp(out.get(), sym.data(), (size_t)n * 4) == 0));
      for (int q = 0; q < 4; ++q) {                            // a mark decodes its count, four bytes fewer do not
        CHECK(mb[q] >= 0 && mb[q] <= (long)str.size() * 4 && (marks[q] == 0) == (mb[q] == 0));
        long a2 = -1;
        CHECK(decode(t, str, mb[q], K, idx, out.get(), &a2) == R::kOk && a2 >= marks[q]);
        if (marks[q] > 0) CHECK(mb[q] >= 8 * K && decode(t, str, mb[q] - 4, K, idx, out.get(), &a2) == R::kOk && a2 < marks[q]);
      }
    }
}

static void every_prefix(const Tables& t) {
  for (long n : {12l, 65l})
    for (int K : kLanes) {
      std::vector<int32_t> sym, idx;
      fill_symbols(t, n, sym, idx);
      const auto str = encode(t, sym, idx, K);
      long before = 0;
      for (long L = 0; L <= (long)str.size() * 4; ++L) {
        std::unique_ptr<int32_t[]> out(new int32_t[n]);
        for (long i = 0; i < n; ++i) out[i] = kFill;
        long avail = -1;
        CHECK(decode(t, str, L, K, idx, out.get(), &avail) == R::kOk);
        CHECK(avail >= before && avail <= n && (L / 4 >= 2 * K || avail == 0));
        for (long i = 0; i < n; ++i) CHECK(out[i] == (i < avail ? sym[i] : kFill));
        before = avail;
      }
      CHECK(before == n);
    }
}

static void corrupted(const Tables& t) {
  for (int K : kLanes) {
    std::vector<int32_t> sym, idx;
    fill_symbols(t, 300, sym, idx);
    const auto str = encode(t, sym, idx, K);
    std::unique_ptr<int32_t[]> out(new int32_t[300]);
    long avail = -1;
    for (int32_t bad : {-1, t.n_cdfs, 1 << 30}) {            // an index outside the tables ends the stream with a status
      auto idx2 = idx;
      idx2[100] = bad;
      CHECK(decode(t, str, (long)str.size() * 4, K, idx2, out.get(), &avail) == R::kBadIndex);
      CHECK(avail <= 100 && avail >= 100 / K * K);
    }
    Tables t2 = t;                                           // a table size the coder refuses
    t2.sizes[idx[7]] = t.stride + 5;
    CHECK(decode(t2, str, (long)str.size() * 4, K, idx, out.get(), &avail) == R::kBadTable && avail <= 7);
    for (int rep = 0; rep < 200; ++rep) {                    // corrupted states and words: any count, no status but a table's
      auto s2 = str;
      s2[rnd() % s2.size()] = rnd() * 65537u;
      const int32_t st = decode(t, s2, (long)s2.size() * 4, K, idx, out.get(), &avail);
      CHECK((st == R::kOk || st == R::kBadTable) && avail >= 0 && avail <= 300);
    }
    for (int rep = 0; rep < 200; ++rep) {                    // strings of random bytes of any length
      std::vector<uint32_t> junk(rnd() % 200);
      for (auto& w : junk) w = rnd() * 65537u;
      const long nb = junk.empty() ? 0 : (long)junk.size() * 4 - (long)(rnd() % 4);
      const int32_t st = decode(t, junk, nb, K, idx, out.get(), &avail);
      CHECK((st == R::kOk || st == R::kBadTable) && avail >= 0 && avail <= 300);
    }
    long words = 0;                                          // a region too small is an overflow, not a write outside it
    for (long cap : {0l, 1l, 2l * K - 1, 2l * K, 2l * K + 20}) {
      std::unique_ptr<uint32_t[]> region(new uint32_t[cap ? cap : 1]);
      CHECK(R::interleaved_encode(sym.data(), idx.data(), 300, R::Flat{}, K, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(),
                                  t.n_cdfs, region.get(), cap, &words) == R::kOverflow && words == 0);
    }
    auto idx2 = idx;
    idx2[299] = t.n_cdfs;
    std::unique_ptr<uint32_t[]> region(new uint32_t[R::interleaved_cap_words(300, K)]);
    CHECK(R::interleaved_encode(sym.data(), idx2.data(), 300, R::Flat{}, K, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(),
                                t.n_cdfs, region.get(), R::interleaved_cap_words(300, K), &words) == R::kBadIndex);
  }
  std::vector<int32_t> none;
  long avail = -1, words = 0;
  uint32_t w[4] = {0, 0, 0, 0};
  CHECK(R::interleaved_decode(w, 16, 3, none.data(), 0, R::Flat{}, R::Int32Rows{t.cdf.data(), t.stride}, t.stride, t.sizes.data(),
                              t.offsets.data(), t.n_cdfs, nullptr, &avail, nullptr, 0, nullptr) == R::kBadStream);
  CHECK(R::interleaved_encode(none.data(), none.data(), 0, R::Flat{}, 128, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(),
                              t.n_cdfs, w, 4, &words) == R::kBadStream);
}

int main() {
  const Tables small = make_tables(5, 40), wide = make_tables(64, 600);
  for (const Tables* t : {&small, &wide}) {
    grid(*t);
    every_prefix(*t);
    corrupted(*t);
  }
  std::printf("rans_interleaved_check: ok\n");
  return 0;
}
