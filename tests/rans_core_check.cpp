// Stand-alone check of csrc/rans_core.h for a sanitizer build (tests/test_rans_core_cpu.py compiles it with
// -fsanitize=address,undefined and runs it as its own process): round trips through flat and NHWC addressing, every
// word-aligned truncation of a stream plus the lengths 0, 4 and 7, and streams of random bytes.  Every buffer is a
// heap block of exactly the size the core is told, so a read or write outside one stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "rans_core.h"

namespace R = vam_rans;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) { std::printf("rans_core_check: FAILED %s (line %d)\n", #cond, __LINE__); std::exit(1); } \
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
    const int syms = 3 + (int)(rnd() % (uint32_t)(max_syms - 2));      // pmf length, escape included
    std::vector<uint32_t> f(syms);
    uint32_t left = 65536 - syms;
    for (int j = 0; j < syms; ++j) {
      const uint32_t extra = j == syms - 1 ? left : rnd() % (left / 2 + 1);
      f[j] = 1 + extra;
      left -= extra;
    }
    int32_t c = 0;
    for (int j = 0; j < syms; ++j) { t.cdf[(size_t)k * t.stride + j] = c; c += (int32_t)f[j]; }
    t.cdf[(size_t)k * t.stride + syms] = c;
    CHECK(c == 65536);
    t.sizes.push_back(syms + 1);
    t.offsets.push_back(-(syms / 2));
  }
  return t;
}

// exact-size heap copies, so the sanitizer sees the true bounds
template <class T>
static std::unique_ptr<T[]> exact(const T* src, size_t n) {
  std::unique_ptr<T[]> p(new T[n ? n : 1]);
  if (n) std::memcpy(p.get(), src, n * sizeof(T));
  return p;
}

template <class A>
static std::vector<uint32_t> encode(const Tables& t, const int32_t* sym, const int32_t* idx, const uint8_t* layer, int sel, long n,
                                    const A& at) {
  const long cap = 2 * n + 16;
  std::unique_ptr<uint32_t[]> region(new uint32_t[cap]);
  long words = 0;
  const int32_t st = R::encode_stream(sym, idx, layer, sel, n, at, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs,
                                      region.get(), cap, &words);
  CHECK(st == R::kOk && words >= 2 && words <= cap);
  return std::vector<uint32_t>(region.get() + cap - words, region.get() + cap);
}

template <class A>
static int32_t decode(const Tables& t, const uint32_t* words, long n_bytes, const int32_t* idx, const uint8_t* layer, int sel, long n,
                      const A& at, int32_t* out) {
  auto w = exact(words, (size_t)(n_bytes / 4));              // whole words only: what the kernels may touch
  return R::decode_stream(n_bytes >= 4 ? w.get() : nullptr, n_bytes, idx, layer, sel, n, at, t.cdf.data(), t.stride, t.sizes.data(),
                          t.offsets.data(), t.n_cdfs, out);
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

static void round_trips(const Tables& t) {
  const long lengths[] = {0, 1, 2, 63, 64, 65, 512, 4096};
  for (long n : lengths) {
    std::vector<int32_t> sym, idx;
    fill_symbols(t, n, sym, idx);
    auto s = exact(sym.data(), (size_t)n);
    auto ix = exact(idx.data(), (size_t)n);
    std::vector<uint8_t> layer(n);
    for (auto& l : layer) l = (uint8_t)(rnd() % 3);
    auto ly = exact(layer.data(), (size_t)n);
    for (int pass = 0; pass < 2; ++pass) {
      const uint8_t* lp = pass ? ly.get() : nullptr;
      const auto words = encode(t, s.get(), ix.get(), lp, 1, n, R::Flat{});
      std::unique_ptr<int32_t[]> out(new int32_t[n ? n : 1]);
      for (long i = 0; i < n; ++i) out[i] = -77;
      CHECK(decode(t, words.data(), (long)words.size() * 4, ix.get(), lp, 1, n, R::Flat{}, out.get()) == R::kOk);
      for (long i = 0; i < n; ++i) CHECK(out[i] == (!lp || layer[i] == 1 ? sym[i] : -77));
    }
  }
  // an NHWC window, with and without an index buffer: [2, 3, 5, 7], c0 = 2, C = 4
  const int h = 3, w = 5, ld = 7, c0 = 2, C = 4;
  const long hw = h * w, n = hw * C, total = 2 * hw * ld;
  for (int image = 0; image < 2; ++image)
    for (int with_idx = 0; with_idx < 2; ++with_idx) {
      std::unique_ptr<int32_t[]> sym(new int32_t[total]), idx(new int32_t[total]), out(new int32_t[total]);
      for (long i = 0; i < total; ++i) {
        idx[i] = (int32_t)(rnd() % (uint32_t)t.n_cdfs);
        sym[i] = t.offsets[with_idx ? idx[i] : 0] + (int32_t)(rnd() % 5) - 1;
        out[i] = -77;
      }
      const long img = image * hw * ld + c0;
      const R::Nhwc at{hw, ld};
      const int32_t* ip = with_idx ? idx.get() + img : nullptr;
      const auto words = encode(t, sym.get() + img, ip, nullptr, 0, n, at);
      CHECK(decode(t, words.data(), (long)words.size() * 4, ip, nullptr, 0, n, at, out.get() + img) == R::kOk);
      for (long i = 0; i < total; ++i) {
        const long pix = i / ld, c = i % ld;
        const bool inside = pix / hw == image && c >= c0 && c < c0 + C;
        CHECK(out[i] == (inside ? sym[i] : -77));
      }
    }
}

static void truncations(const Tables& t) {
  const long n = 2000;
  std::vector<int32_t> sym, idx;
  fill_symbols(t, n, sym, idx);
  auto ix = exact(idx.data(), (size_t)n);
  const auto words = encode(t, sym.data(), ix.get(), nullptr, 0, n, R::Flat{});
  const long full = (long)words.size() * 4;
  std::vector<long> cuts = {0, 4, 7};
  for (long c = 8; c <= full; c += 4) cuts.push_back(c);
  long failures = 0;
  for (long cut : cuts) {
    std::unique_ptr<int32_t[]> out(new int32_t[n]);
    for (long i = 0; i < n; ++i) out[i] = -77;
    const int32_t st = decode(t, words.data(), cut, ix.get(), nullptr, 0, n, R::Flat{}, out.get());
    if (cut < 8 || (cut & 3)) CHECK(st == R::kBadStream);
    if (cut == full) CHECK(st == R::kOk);
    if (st == R::kOk) continue;
    ++failures;
    long k = 0;
    while (k < n && out[k] == sym[k]) ++k;                    // the decoded prefix, then zeros to the end
    for (; k < n; ++k) CHECK(out[k] == 0);
  }
  CHECK(failures > (long)cuts.size() / 2);
  // a table index out of range, and a size the stride cannot hold, are statuses
  std::unique_ptr<int32_t[]> out(new int32_t[n]);
  ix[n / 2] = t.n_cdfs + 95;
  CHECK(decode(t, words.data(), full, ix.get(), nullptr, 0, n, R::Flat{}, out.get()) == R::kBadIndex);
  for (long k = n / 2; k < n; ++k) CHECK(out[k] == 0);
  ix[n / 2] = -1;
  CHECK(decode(t, words.data(), full, ix.get(), nullptr, 0, n, R::Flat{}, out.get()) == R::kBadIndex);
  Tables bad = t;
  bad.sizes[idx[0]] = t.stride + 1;
  ix[n / 2] = idx[n / 2];
  CHECK(decode(bad, words.data(), full, ix.get(), nullptr, 0, n, R::Flat{}, out.get()) == R::kBadTable);
  bad.sizes[idx[0]] = 1;
  CHECK(decode(bad, words.data(), full, ix.get(), nullptr, 0, n, R::Flat{}, out.get()) == R::kBadTable);
  // an output region that is too small is a status, not a write
  std::unique_ptr<uint32_t[]> region(new uint32_t[8]);
  long nw = -1;
  CHECK(R::encode_stream(sym.data(), ix.get(), nullptr, 0, n, R::Flat{}, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(),
                         t.n_cdfs, region.get(), 8, &nw) == R::kOverflow && nw == 0);
}

static void random_bytes(const Tables& t) {
  for (int trial = 0; trial < 400; ++trial) {
    const long n = 1 + rnd() % 4096, n_bytes = 4 * (rnd() % 600);
    std::vector<uint32_t> words((size_t)n_bytes / 4);
    for (auto& v : words) v = rnd() ^ (rnd() << 16);
    if (trial % 3 == 0) for (auto& v : words) v |= 0xFFFF0000u >> (rnd() % 16);   // long runs of escapes and count nibbles
    if (trial % 5 == 0 && words.size() > 1) words[1] = 0x7FFFFFFFu;              // the largest valid initial state
    std::vector<int32_t> idx(n);
    for (auto& v : idx) v = (int32_t)(rnd() % (uint32_t)t.n_cdfs);
    auto ix = exact(idx.data(), (size_t)n);
    std::unique_ptr<int32_t[]> out(new int32_t[n]);
    const int32_t st = decode(t, words.data(), n_bytes, ix.get(), nullptr, 0, n, R::Flat{}, out.get());
    CHECK(st >= 0 && st <= R::kBadStream);
  }
}

int main() {
  for (int round = 0; round < 3; ++round) {
    const Tables t = make_tables(round == 0 ? 5 : 64, round == 2 ? 3000 : 40);
    round_trips(t);
    truncations(t);
    random_bytes(t);
  }
  std::printf("rans_core_check: ok\n");
  return 0;
}
