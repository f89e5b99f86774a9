// What the stand-alone AddressSanitizer programs (tests/emul/*_asan_main.cpp) share: the two checking macros, the case
// generator, exact-size heap blocks, bit comparison, the 16-bit conversions and a hand-built ggl_segplan_t.  Plain C++17 on
// ggl_mpops.h alone, nothing of csrc/: the programs restate what the library documents, they do not borrow its code.
// NOTHING here may add slack: a block is a malloc of exactly the bytes asked for, so that the sanitizer's redzone starts
// where the documented size ends.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "ggl_mpops.h"

// both return 1 from the enclosing function (a run or main) after one line on stderr
#define CHECK(call)                                                                \
  do {                                                                             \
    const int rc_ = (call);                                                        \
    if (rc_ != GGL_OK) {                                                           \
      std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, ggl_last_error());        \
      return 1;                                                                    \
    }                                                                              \
  } while (0)
#define EXPECT(cond)                                                               \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond);             \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

// one LCG draws every case; a program that wants another sequence sets rnd_state first thing in main
inline uint32_t rnd_state = 2463534242u;
inline uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }
inline float rndf() { return (float)((int)(rnd() >> 8) % 4001 - 2000) / 1024.0f; }

// exactly n elements (one for n = 0: never a zero-byte block's NULL)
template <typename T>
inline T *block(size_t n) { return static_cast<T *>(std::malloc((n ? n : 1) * sizeof(T))); }

// n elements, bit for bit
template <typename T>
inline bool same(const T *a, const T *b, size_t n) { return std::memcmp(a, b, n * sizeof(T)) == 0; }

// 16-bit <-> f32 as the library documents them: exact widening, round-to-nearest-even narrowing
inline float widen(int dtype, uint16_t b) {
  if (dtype == GGL_BF16) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  }
  _Float16 h;
  std::memcpy(&h, &b, 2);
  return (float)h;
}
inline uint16_t narrow(int dtype, float f) {
  if (dtype == GGL_BF16) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    return (uint16_t)((x + (((x >> 16) & 1u) + 0x7fffu)) >> 16);   // (no NaNs in these programs)
  }
  const _Float16 h = (_Float16)f;
  uint16_t b;
  std::memcpy(&b, &h, 2);
  return b;
}

// A ggl_segplan_t (c) and the blocks it points into.  A program fills rowptr ([N + 1]) — make_plan does it from ids — and
// finish_plan derives the rest.
struct Plan {
  ggl_segplan_t c{};
  int64_t *rowptr = nullptr, *chunk_ptr = nullptr;
  int32_t *long_rows = nullptr, *perm = nullptr;
  // the hub partial of the next walk: exactly `bytes` bytes (NULL for 0) in place of the one attached before
  void set_partial(size_t bytes) {
    std::free(c.partial);
    c.partial = bytes ? std::malloc(bytes) : nullptr;
    c.partial_bytes = bytes;
  }
  void release() { set_partial(0); std::free(rowptr); std::free(chunk_ptr); std::free(long_rows); std::free(perm); }
};

// the long-row table of p.rowptr as ggl_plan_long_count / _fill build it (a row is long when it holds MORE than `chunk`
// elements and is walked as ceil(len / chunk) chunks; chunk_ptr is the exclusive prefix of the chunk counts), then p.c
inline void finish_plan(Plan &p, int64_t N, int64_t E, int64_t chunk) {
  std::vector<int32_t> lr;
  std::vector<int64_t> cp{0};
  for (int64_t r = 0; r < N; ++r) {
    const int64_t len = p.rowptr[r + 1] - p.rowptr[r];
    if (len > chunk) {
      lr.push_back((int32_t)r);
      cp.push_back(cp.back() + (len + chunk - 1) / chunk);
    }
  }
  p.c.rowptr = p.rowptr;
  p.c.perm = p.perm;
  p.c.N = N;
  p.c.E = E;
  p.c.chunk = chunk;
  p.c.n_long = (int64_t)lr.size();
  p.c.n_chunks = cp.back();
  if (!lr.empty()) {
    p.long_rows = block<int32_t>(lr.size());
    p.chunk_ptr = block<int64_t>(cp.size());
    std::memcpy(p.long_rows, lr.data(), lr.size() * sizeof(int32_t));
    std::memcpy(p.chunk_ptr, cp.data(), cp.size() * sizeof(int64_t));
    p.c.long_rows = p.long_rows;
    p.c.chunk_ptr = p.chunk_ptr;
  }
}

// rowptr / perm / long-row table of `ids` (stable sort; perm stays NULL when the ids arrive sorted)
inline void make_plan(Plan &p, const std::vector<int32_t> &ids, int64_t N, int64_t chunk) {
  const int64_t E = (int64_t)ids.size();
  p.rowptr = block<int64_t>(N + 1);
  std::fill(p.rowptr, p.rowptr + N + 1, 0);
  for (int32_t d : ids) ++p.rowptr[d + 1];
  for (int64_t r = 0; r < N; ++r) p.rowptr[r + 1] += p.rowptr[r];
  if (!std::is_sorted(ids.begin(), ids.end())) {
    p.perm = block<int32_t>(E);
    std::iota(p.perm, p.perm + E, 0);
    std::stable_sort(p.perm, p.perm + E, [&](int32_t a, int32_t b) { return ids[a] < ids[b]; });
  }
  finish_plan(p, N, E, chunk);
}
