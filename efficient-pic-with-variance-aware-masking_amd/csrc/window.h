// The channel-window idiom of the element-wise kernels, once.  A window is C channels of an NHWC buffer whose pixels lie
// `ld` elements apart (and, for the levels forms, whose levels lie `ls` elements apart); a kernel walks it as n_pix * C/4
// vectors of 16 bytes, grid-stride.  Device side: the split of a vector index and the 16-byte loads and stores.  Host side:
// the launch grid, the alignment predicate and one checker for the rules every entry point applies to its windows.
#pragma once
#include <cstdint>
#include <initializer_list>
#include "common.h"

namespace vam {

// vector i of a window of C4 = C/4 vectors per pixel: pixel p, first channel c
__device__ __forceinline__ void vec_at(long i, int C4, long& p, int& c) {
  p = i / C4;
  c = (int)(i - p * C4) * 4;
}

__device__ __forceinline__ float4 ld4(const float* base, long p, int ld, int c) {
  return *reinterpret_cast<const float4*>(base + p * ld + c);
}
__device__ __forceinline__ void ld4(const float* base, long p, int ld, int c, float* v) {
  const float4 t = ld4(base, p, ld, c);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void st4(float* base, long p, int ld, int c, const float* v) {
  *reinterpret_cast<float4*>(base + p * ld + c) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void ldi4(const int32_t* base, long p, int ld, int c, int* v) {
  const int4 t = *reinterpret_cast<const int4*>(base + p * ld + c);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void sti4(int32_t* base, long p, int ld, int c, const int* v) {
  *reinterpret_cast<int4*>(base + p * ld + c) = make_int4(v[0], v[1], v[2], v[3]);
}
// four uint8 layer ids in one 4-byte load; id k is (word >> 8k) & 255
__device__ __forceinline__ unsigned ldb4(const uint8_t* base, long p, int ld, int c) {
  return *reinterpret_cast<const unsigned*>(base + p * ld + c);
}
__device__ __forceinline__ int layer_id(unsigned word, int k) { return (int)((word >> (8 * k)) & 255u); }

// ------------------------------------------------------------------ host
// grid of a grid-stride launch over n work items: at least one block, at most `cap`
static inline unsigned stream_grid(long n, int block, int cap) {
  long g = (n + block - 1) / block;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

static inline bool aligned(const void* p, int bytes) { return (((uintptr_t)p) & (uintptr_t)(bytes - 1)) == 0; }

// One window (or plain array) of an entry point and what the entry demands of it.  An absent optional window is not
// looked at.  align = 16 / 8 / 4 bytes; the strides must be multiples of 4.  A stride the kernel does not use, or that an
// array does not have, is passed as 0.
struct Win {
  const char* name;
  const void* ptr;
  long ld;            // pixel stride
  long ls;            // level stride, 0 where there is none
  bool required;
  int align;
  bool at_least_C;    // the entry demands ld >= C
};

// What an entry says when a rule fires: "<who>: <prefix><phrase> (<window>)".
struct WinWords {
  const char* null = "bad arguments";
  const char* align = "alignment";
  const char* stride = "strides";
  const char* prefix = "";
};

static inline int check_windows(const char* who, int C, std::initializer_list<Win> wins, const WinWords& w = WinWords()) {
  for (const Win& x : wins) {
    if (!x.ptr) {
      VAM_REQUIRE(!x.required, "%s: %s%s (%s)", who, w.prefix, w.null, x.name);
      continue;
    }
    VAM_REQUIRE(aligned(x.ptr, x.align), "%s: %s%s (%s)", who, w.prefix, w.align, x.name);
    VAM_REQUIRE(x.ld % 4 == 0 && x.ls % 4 == 0 && (!x.at_least_C || x.ld >= C), "%s: %s%s (%s)", who,
                w.prefix, w.stride, x.name);
  }
  return VAM_OK;
}

#define VAM_CHECK_WINDOWS(...)                              \
  do {                                                      \
    if (int rc_ = vam::check_windows(__VA_ARGS__)) return rc_; \
  } while (0)

}  // namespace vam
