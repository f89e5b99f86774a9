// A stand-alone AddressSanitizer check of the multi-statistic segment aggregate (ggl_segment_multi_fwd / _bwd) on the
// host-emulated kernel sources: every buffer is a heap block of exactly the documented size — x and gx exactly E * K floats,
// out and g exactly N * A * K, mean exactly N * K, the witnesses exactly N * K int32, plan->partial exactly
// ggl_segment_multi_partial_bytes(...) — so a read or write past an end aborts the run.  Two plans: one built from UNSORTED ids
// (a non-NULL perm) with long rows (chunk 16: pieces, partials, the merge), one from ids that arrive sorted (NULL perm, no
// long rows).  Shapes (K, C) = (20, 5) (one column per lane) and (48, 16) (16-byte lanes), four sets of aggregates, empty_zero
// both ways.  Built and run by tests/test_segment_multi_sanitized.py; exits 0 when every output has the bits of the serial
// loop below.
#include <cfloat>
#include <cmath>

#include "asan_common.hpp"

static float rndq() { return (float)((int)(rnd() >> 8) % 17 - 8) / 4.0f; }       // many equal values, +0.0 among them

struct Acc { float S, Q, mn, mx; int32_t an, ax; };

// the documented arithmetic, one (row, column) at a time; volatile keeps every step a rounded f32 operation
static void serial(const Plan &p, const float *x, int64_t K, int64_t C, const int *aggs, int A, int empty_zero, const float *g,
                   float *out, float *mean_o, int32_t *amin, int32_t *amax, float *gx) {
  const int64_t E = p.c.E;
  int at[6] = {-1, -1, -1, -1, -1, -1};
  for (int s = 0; s < A; ++s) at[aggs[s]] = s;
  const bool sq = at[GGL_AGG_VAR] >= 0 || at[GGL_AGG_STD] >= 0;
  auto piece = [&](int64_t b, int64_t stop, int64_t k) {
    Acc a{0.0f, 0.0f, FLT_MAX, -FLT_MAX, (int32_t)E, (int32_t)E};
    for (int64_t q = b; q < stop; ++q) {
      const int32_t e = p.perm ? p.perm[q] : (int32_t)q;
      const float v = x[(int64_t)e * K + k];
      volatile float s = a.S + v, vv = v * v;
      a.S = s;
      volatile float qq = a.Q + vv;
      a.Q = qq;
      if (a.mx < v) { a.mx = v; a.ax = e; }
      if (v < a.mn) { a.mn = v; a.an = e; }
    }
    return a;
  };
  volatile float s0 = std::sqrt(1e-5f);
  for (int64_t r = 0; r < p.c.N; ++r)
    for (int64_t k = 0; k < K; ++k) {
      const int64_t beg = p.rowptr[r], end = p.rowptr[r + 1], n = end - beg;
      Acc t{0.0f, 0.0f, FLT_MAX, -FLT_MAX, (int32_t)E, (int32_t)E};
      if (n > p.c.chunk) {
        for (int64_t b = beg; b < end; b += p.c.chunk) {   // partials merged in ascending order
          const Acc a = piece(b, std::min(b + p.c.chunk, end), k);
          volatile float s = t.S + a.S, q = t.Q + a.Q;
          t.S = s; t.Q = q;
          if (t.mx < a.mx) { t.mx = a.mx; t.ax = a.ax; }
          if (a.mn < t.mn) { t.mn = a.mn; t.an = a.an; }
        }
      } else {
        t = piece(beg, end, k);
      }
      const float nf = (float)n;
      volatile float mean = n > 1 ? t.S / nf : t.S, msq = n > 1 ? t.Q / nf : t.Q;
      volatile float mm = mean * mean;
      volatile float var = msq - mm;
      volatile float vp = std::fmax((float)var, 0.0f) + 1e-5f;
      volatile float sd = std::sqrt((float)vp);
      const float mn = (n == 0 && empty_zero) ? 0.0f : t.mn, mx = (n == 0 && empty_zero) ? 0.0f : t.mx;
      const float vals[6] = {t.S, mean, mn, mx, var, sd};
      const int64_t base = r * A * K + (k / C) * A * C + k % C;
      for (int s = 0; s < A; ++s) out[base + (int64_t)s * C] = vals[aggs[s]];
      mean_o[r * K + k] = mean;
      amin[r * K + k] = t.an;
      amax[r * K + k] = t.ax;
      if (n == 0) continue;
      // backward coefficients, then every position of the row
      auto gof = [&](int code) { return g[base + (int64_t)at[code] * C]; };
      volatile float gv = at[GGL_AGG_VAR] >= 0 ? gof(GGL_AGG_VAR) : 0.0f;
      if (at[GGL_AGG_STD] >= 0) {
        volatile float two_sd = 2.0f * sd;
        volatile float tt = sd > s0 ? gof(GGL_AGG_STD) / two_sd : 0.0f;
        if (at[GGL_AGG_VAR] >= 0) gv = gv + tt; else gv = tt;
      }
      volatile float two_gv = 2.0f * gv;
      volatile float c1 = sq ? two_gv / nf : 0.0f;
      volatile float c0 = 0.0f;
      if (at[GGL_AGG_SUM] >= 0) c0 = c0 + gof(GGL_AGG_SUM);
      if (at[GGL_AGG_MEAN] >= 0) { volatile float d = gof(GGL_AGG_MEAN) / nf; c0 = c0 + d; }
      if (sq) { volatile float d = c1 * mean; c0 = c0 - d; }
      for (int64_t q = beg; q < end; ++q) {
        const int32_t e = p.perm ? p.perm[q] : (int32_t)q;
        volatile float tv = c0;
        if (sq) { volatile float d = c1 * x[(int64_t)e * K + k]; tv = c0 + d; }
        if (at[GGL_AGG_MAX] >= 0 && t.ax == e) tv = tv + gof(GGL_AGG_MAX);
        if (at[GGL_AGG_MIN] >= 0 && t.an == e) tv = tv + gof(GGL_AGG_MIN);
        gx[(int64_t)e * K + k] = tv;
      }
    }
}

static int run_case(Plan &p, int64_t K, int64_t C, const std::vector<int> &aggs, int empty_zero) {
  const int64_t N = p.c.N, E = p.c.E;
  const int A = (int)aggs.size();
  bool sq = false, mn = false, mx = false;
  for (int c : aggs) { sq |= c >= GGL_AGG_VAR; mn |= c == GGL_AGG_MIN; mx |= c == GGL_AGG_MAX; }
  float *x = block<float>(E * K), *g = block<float>(N * A * K);
  for (int64_t i = 0; i < E * K; ++i) x[i] = rndq();
  for (int64_t i = 0; i < N * A * K; ++i) g[i] = rndf();
  const size_t pb = ggl_segment_multi_partial_bytes(p.c.n_chunks, K, aggs.data(), A);
  EXPECT((pb > 0) == (p.c.n_long > 0));
  p.set_partial(pb);
  float *out = block<float>(N * A * K);                                  // exactly N * A * K floats
  float *mean = sq ? block<float>(N * K) : nullptr;
  int32_t *amin = mn ? block<int32_t>(N * K) : nullptr, *amax = mx ? block<int32_t>(N * K) : nullptr;   // exactly N * K int32
  float *gx = block<float>(E * K);
  CHECK(ggl_segment_multi_fwd(x, &p.c, K, C, aggs.data(), A, empty_zero, out, mean, amin, amax, nullptr));
  p.set_partial(0);                    // the backward needs no partial buffer
  // (x, mean, out and the witnesses are handed over only where the aggs read them)
  CHECK(ggl_segment_multi_bwd(g, sq ? x : nullptr, aggs.end() != std::find(aggs.begin(), aggs.end(), (int)GGL_AGG_STD) ? out : nullptr,
                              mean, amin, amax, &p.c, K, C, aggs.data(), A, gx, nullptr));
  float *w_out = block<float>(N * A * K), *w_mean = block<float>(N * K), *w_gx = block<float>(E * K);
  int32_t *w_amin = block<int32_t>(N * K), *w_amax = block<int32_t>(N * K);
  serial(p, x, K, C, aggs.data(), A, empty_zero, g, w_out, w_mean, w_amin, w_amax, w_gx);
  EXPECT(same(out, w_out, N * A * K));
  if (mean) EXPECT(same(mean, w_mean, N * K));
  if (amin) EXPECT(same(amin, w_amin, N * K));
  if (amax) EXPECT(same(amax, w_amax, N * K));
  EXPECT(same(gx, w_gx, E * K));
  for (void *b : {(void *)x, (void *)g, (void *)out, (void *)mean, (void *)amin, (void *)amax, (void *)gx, (void *)w_out,
                  (void *)w_mean, (void *)w_gx, (void *)w_amin, (void *)w_amax})
    std::free(b);
  return 0;
}

int main() {
  const int64_t N = 60, E = 1500;
  const int64_t shapes[2][2] = {{20, 5}, {48, 16}};
  const std::vector<std::vector<int>> sets = {{GGL_AGG_MEAN, GGL_AGG_MIN, GGL_AGG_MAX, GGL_AGG_STD},
                                              {GGL_AGG_SUM, GGL_AGG_MEAN, GGL_AGG_MIN, GGL_AGG_MAX, GGL_AGG_VAR, GGL_AGG_STD},
                                              {GGL_AGG_MIN}, {GGL_AGG_STD, GGL_AGG_MEAN}};
  int cases = 0;
  for (int pass = 0; pass < 2; ++pass) {   // 0: unsorted ids (perm) + long rows; 1: sorted ids (NULL perm), short rows
    std::vector<int32_t> ids(E);
    for (int64_t e = 0; e < E; ++e) ids[e] = (e % 3 == 0) ? 5 : (int32_t)(rnd() % (N - 2));   // a hub; rows N-2, N-1 empty
    if (pass == 1) std::sort(ids.begin(), ids.end());
    Plan p;
    make_plan(p, ids, N, pass == 0 ? 16 : 4096);
    if ((p.perm == nullptr) != (pass == 1) || (p.c.n_long > 0) != (pass == 0)) {
      std::fprintf(stderr, "plan of pass %d is not what the case needs\n", pass);
      return 1;
    }
    for (const auto &s : shapes)
      for (const auto &aggs : sets)
        for (int ez = 0; ez < 2; ++ez) {
          if (run_case(p, s[0], s[1], aggs, ez)) {
            std::fprintf(stderr, "failed: pass %d, K %d, C %d, %d aggs, empty_zero %d\n", pass, (int)s[0], (int)s[1],
                         (int)aggs.size(), ez);
            return 1;
          }
          ++cases;
        }
    p.release();
  }
  std::printf("segment_multi sanitized: %d cases ok\n", cases);
  return 0;
}
