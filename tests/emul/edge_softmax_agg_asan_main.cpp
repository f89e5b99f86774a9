// A stand-alone AddressSanitizer check of the edge-softmax aggregate (ggl_edge_softmax_agg_{fwd,bwd_dst,bwd_src}) on the
// host-emulated kernel sources: every buffer is a heap block of exactly the documented size — z and gz hold exactly E * H
// floats, alpha exactly E * H — so a read or write past an end aborts the run.  Two plans: one built from UNSORTED ids (a
// non-NULL perm) with long rows both ways (chunk 16: hub chunks, partials, merges), one from ids that arrive sorted (NULL
// perm, no long rows).  Shapes 1 x 1, 3 x 5 (element form), 2 x 12 and 8 x 8 (16-byte loads), with and without attention
// dropout.  Built and run by tests/test_edge_softmax_agg_sanitized.py; exits 0 when, on z = LeakyReLU(el[src] + er[dst]),
// out / rowmax / rowden / alpha / gx have the bits of ggl_gat_fused_* and gz is their de in the caller's edge order.
#include "asan_common.hpp"

static int run(int64_t N, int64_t E, int64_t chunk, bool sorted, int64_t H, int64_t C, float p_drop) {
  const int64_t K = H * C;
  // the caller's edge list: a heavy destination (N - 1) and a heavy source (0)
  std::vector<int32_t> src(E), dst(E);
  for (int64_t e = 0; e < E; ++e) {
    src[e] = (e % 5 == 0) ? 0 : (int32_t)(rnd() % N);
    dst[e] = (e % 7 == 0) ? (int32_t)(N - 1) : (int32_t)(rnd() % N);
  }
  if (sorted) std::sort(dst.begin(), dst.end());
  Plan f, t;
  make_plan(f, dst, N, chunk);
  make_plan(t, src, N, chunk);
  EXPECT((f.perm == nullptr) == sorted);
  if (chunk < 64) EXPECT(f.c.n_long > 0 && t.c.n_long > 0);
  // col[p] = source of sorted position p; colT / posT: destination and forward position of every transposed position
  int32_t *col = block<int32_t>(E), *colT = block<int32_t>(E), *posT = block<int32_t>(E);
  std::vector<int32_t> pos_of(E);
  for (int64_t p = 0; p < E; ++p) {
    const int32_t e = f.perm ? f.perm[p] : (int32_t)p;
    col[p] = src[e];
    pos_of[e] = (int32_t)p;
  }
  for (int64_t q = 0; q < E; ++q) {
    const int32_t e = t.perm ? t.perm[q] : (int32_t)q;
    colT[q] = dst[e];
    posT[q] = pos_of[e];
  }

  const float slope = 0.2f;
  float *el = block<float>(N * H), *er = block<float>(N * H), *x = block<float>(N * K), *g = block<float>(N * K);
  for (int64_t i = 0; i < N * H; ++i) { el[i] = rndf(); er[i] = rndf(); }
  for (int64_t i = 0; i < N * K; ++i) { x[i] = rndf(); g[i] = rndf(); }
  float *z = block<float>(E * H);                 // exactly E * H floats, the caller's order
  std::vector<char> positive(E * H);
  for (int64_t e = 0; e < E; ++e)
    for (int64_t h = 0; h < H; ++h) {
      const float raw = el[src[e] * H + h] + er[dst[e] * H + h];
      const float neg = raw * slope;
      positive[e * H + h] = raw > 0.0f;
      z[e * H + h] = raw > 0.0f ? raw : neg;
    }
  int64_t *rng = block<int64_t>(2), *rng_f = block<int64_t>(2), *rng_used = block<int64_t>(2);
  rng[0] = rng_f[0] = rng_used[0] = 0x1234567;
  rng[1] = rng_f[1] = rng_used[1] = 3;

  // ---- forward
  f.set_partial(ggl_gat_partial_bytes(f.c.n_chunks, H, C));
  float *out_f = block<float>(N * K), *rmax_f = block<float>(N * H), *rden_f = block<float>(N * H);
  float *out = block<float>(N * K), *rmax = block<float>(N * H), *rden = block<float>(N * H);
  CHECK(ggl_gat_fused_fwd(&f.c, col, el, er, x, slope, H, C, p_drop, p_drop > 0 ? rng_f : nullptr, out_f, rmax_f, rden_f,
                          nullptr));
  CHECK(ggl_edge_softmax_agg_fwd(&f.c, col, z, x, H, C, p_drop, p_drop > 0 ? rng : nullptr, out, rmax, rden, nullptr));
  if (p_drop > 0) EXPECT(rng[1] == 4 && rng_f[1] == 4);
  EXPECT(same(out, out_f, N * K) && same(rmax, rmax_f, N * H) && same(rden, rden_f, N * H));

  // ---- backward
  f.set_partial(ggl_partial_bytes(GGL_F32, f.c.n_chunks, H, 0));
  t.set_partial(ggl_partial_bytes(GGL_F32, t.c.n_chunks, K + H, 0));
  float *alpha_f = block<float>(E * H), *de_f = block<float>(E * H), *ger_f = block<float>(N * H), *gel_f = block<float>(N * H);
  float *gx_f = block<float>(N * K);
  float *alpha = block<float>(E * H), *gz = block<float>(E * H), *gx = block<float>(N * K);
  const int64_t *ru = p_drop > 0 ? rng_used : nullptr;
  CHECK(ggl_gat_fused_bwd_dst(&f.c, col, nullptr, el, er, x, g, out_f, rmax_f, rden_f, slope, H, C, p_drop, ru, alpha_f, de_f,
                              ger_f, nullptr, nullptr));
  CHECK(ggl_gat_fused_bwd_src(&t.c, colT, posT, alpha_f, de_f, g, H, C, gx_f, gel_f, nullptr));
  CHECK(ggl_edge_softmax_agg_bwd_dst(&f.c, col, z, x, g, out, rmax, rden, H, C, p_drop, ru, alpha, gz, nullptr));
  CHECK(ggl_edge_softmax_agg_bwd_src(&t.c, colT, posT, alpha, g, H, C, gx, nullptr));
  EXPECT(same(alpha, alpha_f, E * H) && same(gx, gx_f, N * K));
  for (int64_t p = 0; p < E; ++p) {   // gz[e] is the GAT call's ds at position p: its de is ds where raw > 0, ds * slope elsewhere
    const int64_t e = f.perm ? f.perm[p] : p;
    for (int64_t h = 0; h < H; ++h) {
      const float ds = gz[e * H + h];
      const float want = positive[e * H + h] ? ds : ds * slope;
      EXPECT(same(&want, &de_f[p * H + h], 1));
    }
  }
  // either gradient alone: the other buffer is not touched (NULL)
  float *gz2 = block<float>(E * H), *alpha2 = block<float>(E * H);
  CHECK(ggl_edge_softmax_agg_bwd_dst(&f.c, col, z, x, g, out, rmax, rden, H, C, p_drop, ru, nullptr, gz2, nullptr));
  CHECK(ggl_edge_softmax_agg_bwd_dst(&f.c, col, z, x, g, out, rmax, rden, H, C, p_drop, ru, alpha2, nullptr, nullptr));
  EXPECT(same(gz2, gz, E * H) && same(alpha2, alpha, E * H));
  for (void *b : {(void *)col, (void *)colT, (void *)posT, (void *)el, (void *)er, (void *)x, (void *)g, (void *)z, (void *)rng,
                  (void *)rng_f, (void *)rng_used, (void *)out_f, (void *)rmax_f, (void *)rden_f, (void *)out, (void *)rmax,
                  (void *)rden, (void *)alpha_f, (void *)de_f, (void *)ger_f, (void *)gel_f, (void *)gx_f, (void *)alpha,
                  (void *)gz, (void *)gx, (void *)gz2, (void *)alpha2})
    std::free(b);
  f.release();
  t.release();
  return 0;
}

int main() {
  const int64_t shapes[4][2] = {{1, 1}, {3, 5}, {2, 12}, {8, 8}};
  int cases = 0;
  for (int pass = 0; pass < 2; ++pass)   // 0: unsorted ids (perm), long rows both ways; 1: sorted ids (NULL perm), short rows
    for (const auto &s : shapes)
      for (float p : {0.0f, 0.5f}) {
        if (run(120, 2500, pass == 0 ? 16 : 4096, pass == 1, s[0], s[1], p)) {
          std::fprintf(stderr, "failed: pass %d, %d x %d, p %g\n", pass, (int)s[0], (int)s[1], p);
          return 1;
        }
        ++cases;
      }
  std::printf("edge_softmax_agg sanitized: %d cases ok\n", cases);
  return 0;
}
