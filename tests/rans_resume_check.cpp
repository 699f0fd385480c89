// Stand-alone check of the resumable decode of csrc/rans_core.h for a sanitizer build
// (tests/test_rans_resume_cpu.py compiles it with -fsanitize=address,undefined and runs it as its own process): the pairs
// of byte lengths L1 <= L2 (all of a short string, an odd stride over a long one) at K = 1, 8, 64 and a chain through every
// length, each call seeing only the words from the checkpoint's position on, against the one-shot interleaved_decode on
// the first L2 bytes; a corrupted index in an earlier group, in the checkpointed group and in a later one; impossible
// checkpoints.  Every buffer is a heap block of exactly the size the core is told, so a read or write outside one stops
// the program.
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
    if (!(cond)) { std::printf("rans_resume_check: FAILED %s (line %d)\n", #cond, __LINE__); std::exit(1); } \
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
  std::unique_ptr<uint32_t[]> region(new uint32_t[cap]);
  long words = 0;
  CHECK(R::interleaved_encode(sym.data(), idx.data(), n, R::Flat{}, K, t.cdf.data(), t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs,
                              region.get(), cap, &words) == R::kOk);
  return std::vector<uint32_t>(region.get() + cap - words, region.get() + cap);
}

static const int32_t kFill = -777777;

// The one-shot decode of the first n_bytes bytes into a kFill-ed array of n.
static int32_t one_shot(const Tables& t, const std::vector<uint32_t>& str, long n_bytes, int K, const std::vector<int32_t>& idx,
                        std::vector<int32_t>& out, long* available) {
  auto w = exact(str.data(), (size_t)(n_bytes / 4));
  auto i = exact(idx.data(), idx.size());
  out.assign(idx.size(), kFill);
  return R::interleaved_decode(n_bytes >= 4 ? w.get() : nullptr, n_bytes, K, i.get(), (long)idx.size(), R::Flat{},
                               R::Int32Rows{t.cdf.data(), t.stride}, t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs, out.data(),
                               available, nullptr, 0, nullptr);
}

// A receiver: the checkpoint and the symbols so far.  step() hands the core ONLY the whole words of the first n_bytes bytes
// from the checkpoint's position on, in a block of exactly that size, and checks what it wrote.
struct Receiver {
  long done = 0, pos = 0;
  std::unique_ptr<uint64_t[]> states;
  std::unique_ptr<int32_t[]> out;
  long n;
  int K;
  Receiver(long n_, int K_) : states(new uint64_t[K_]), out(new int32_t[n_ ? n_ : 1]), n(n_), K(K_) {
    for (int l = 0; l < K; ++l) states[l] = 0;
    for (long i = 0; i < n; ++i) out[i] = kFill;
  }
  int32_t step(const Tables& t, const std::vector<uint32_t>& str, long n_bytes, const std::vector<int32_t>& idx, long* available) {
    const long W = n_bytes / 4, have = W > pos ? W - pos : 0, done_in = done;
    auto w = exact(str.data() + (have ? pos : 0), (size_t)have);
    auto i = exact(idx.data(), idx.size());
    std::vector<int32_t> before(out.get(), out.get() + n);
    const int32_t st = R::interleaved_resume(have ? w.get() : nullptr, have * 4 + (W >= pos ? n_bytes % 4 : 0), K, i.get(), n, R::Flat{},
                                             R::Int32Rows{t.cdf.data(), t.stride}, t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs,
                                             out.get(), available, &done, &pos, states.get());
    for (long e = 0; e < n; ++e)
      if (e < done_in || e >= *available) CHECK(out[e] == before[e]);      // nothing outside [done_in, available) is touched
    CHECK(done >= done_in && (done == n || done % K == 0) && done <= *available);
    return st;
  }
};

struct Want {
  int32_t status;
  long available;
  std::vector<int32_t> sym;
};

static Want want_of(const Tables& t, const std::vector<uint32_t>& str, long L, int K, const std::vector<int32_t>& idx) {
  Want w;
  w.status = one_shot(t, str, L, K, idx, w.sym, &w.available);
  return w;
}

static void agrees(const Tables& t, const std::vector<uint32_t>& str, long L, int K, const std::vector<int32_t>& idx, Receiver& r,
                   const Want& w) {
  long a2 = -1;
  const int32_t s2 = r.step(t, str, L, idx, &a2);
  CHECK(w.status == s2 && w.available == a2);
  for (long e = 0; e < a2; ++e) CHECK(r.out[e] == w.sym[e]);
  CHECK(r.done == (a2 == r.n ? r.n : a2 / K * K));
}

static void agrees(const Tables& t, const std::vector<uint32_t>& str, long L, int K, const std::vector<int32_t>& idx, Receiver& r) {
  agrees(t, str, L, K, idx, r, want_of(t, str, L, K, idx));
}

static void split_pairs(const Tables& t) {
  for (long n : {1l, 50l, 130l})
    for (int K : {1, 8, 64}) {
      std::vector<int32_t> sym, idx;
      fill_symbols(t, n, sym, idx);
      const auto str = encode(t, sym, idx, K);
      const long total = (long)str.size() * 4;
      std::vector<Want> want;                                // the one-shot decode of every byte length, once
      for (long L = 0; L <= total; ++L) want.push_back(want_of(t, str, L, K, idx));
      const long step = total <= 160 ? 1 : (total / 80) | 1;   // every pair of the short strings; an odd stride over the long
      for (long L1 = 0; L1 <= total; L1 += step)
        for (long L2 = L1; L2 <= total; L2 += step) {
          Receiver r(n, K);
          agrees(t, str, L1, K, idx, r, want[L1]);
          agrees(t, str, L2, K, idx, r, want[L2]);
          if (L2 + step > total) {                           // the whole string, and a call after the end
            agrees(t, str, total, K, idx, r, want[total]);
            CHECK(r.done == n);
            agrees(t, str, total, K, idx, r, want[total]);
            for (long e = 0; e < n; ++e) CHECK(r.out[e] == sym[e]);
          }
        }
      Receiver chain(n, K);                                  // one receiver through every byte length
      for (long L = 0; L <= total; ++L) agrees(t, str, L, K, idx, chain, want[L]);
      CHECK(chain.done == n);
    }
}

static void corrupted(const Tables& t) {
  for (int K : {1, 8, 64}) {
    const long n = 300;
    std::vector<int32_t> sym, idx;
    fill_symbols(t, n, sym, idx);
    const auto str = encode(t, sym, idx, K);
    const long total = (long)str.size() * 4;
    for (long where : {70l, 150l, 290l})                     // before, in and after the group a cut in the middle leaves
      for (int32_t bad : {-1, t.n_cdfs, 1 << 30}) {
        auto idx2 = idx;
        idx2[where] = bad;
        Receiver r(n, K);
        for (long L : {0l, total / 2 + 1, total - 2, total, total}) {
          agrees(t, str, L, K, idx2, r);                     // the status is recomputed on every call
        }
        long avail = -1;
        CHECK(r.step(t, str, total, idx2, &avail) == R::kBadIndex && avail <= where && avail >= where / K * K);
        CHECK(r.done == where / K * K);
      }
  }
}

static void refusals(const Tables& t) {
  std::vector<int32_t> sym, idx;
  fill_symbols(t, 50, sym, idx);
  const auto str = encode(t, sym, idx, 8);
  std::unique_ptr<uint64_t[]> states(new uint64_t[8]);
  std::unique_ptr<int32_t[]> out(new int32_t[50]);
  for (int l = 0; l < 8; ++l) states[l] = 0x5555555555555555ull;
  for (long e = 0; e < 50; ++e) out[e] = kFill;
  const long bad[][2] = {{3, 16}, {51, 16}, {56, 16}, {8, 15}, {8, 0}, {-8, 16}, {0, -1}};
  for (const auto& b : bad) {
    long done = b[0], pos = b[1], avail = -1;
    CHECK(R::interleaved_resume(str.data(), (long)str.size() * 4, 8, idx.data(), 50, R::Flat{}, R::Int32Rows{t.cdf.data(), t.stride},
                                t.stride, t.sizes.data(), t.offsets.data(), t.n_cdfs, out.get(), &avail, &done, &pos,
                                states.get()) == R::kBadStream);
    CHECK(avail == 0 && done == b[0] && pos == b[1]);
    for (int l = 0; l < 8; ++l) CHECK(states[l] == 0x5555555555555555ull);
    for (long e = 0; e < 50; ++e) CHECK(out[e] == kFill);
  }
  long done = 0, pos = 0, avail = -1;
  CHECK(R::interleaved_resume(str.data(), 16, 3, idx.data(), 50, R::Flat{}, R::Int32Rows{t.cdf.data(), t.stride}, t.stride,
                              t.sizes.data(), t.offsets.data(), t.n_cdfs, out.get(), &avail, &done, &pos, states.get()) == R::kBadStream);
  CHECK(R::interleaved_resume(str.data(), -4, 8, idx.data(), 50, R::Flat{}, R::Int32Rows{t.cdf.data(), t.stride}, t.stride,
                              t.sizes.data(), t.offsets.data(), t.n_cdfs, out.get(), &avail, &done, &pos, states.get()) == R::kBadStream);
}

int main() {
  const Tables small = make_tables(5, 40), wide = make_tables(64, 600);
  for (const Tables* t : {&small, &wide}) {
    split_pairs(*t);
    corrupted(*t);
    refusals(*t);
  }
  std::printf("rans_resume_check: ok\n");
  return 0;
}
