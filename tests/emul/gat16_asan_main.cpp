// A stand-alone AddressSanitizer check of the fused GAT on 16-bit rows (ggl_gat_fused_{fwd,bwd_dst,bwd_src}_x16) on the
// host-emulated kernel sources: every buffer is a heap block of exactly the documented size, so a read or write past an end
// aborts the run.  Shapes 3 x 5 (element form), 2 x 12 (8-byte loads) and 8 x 8 (16-byte loads), bf16 and f16, 16-bit and f32
// out, with and without attention dropout; once on a plan with long rows both ways (hub chunks, f32 partials, the merges) and
// once with x, g and out starting ONE element into their blocks (2-byte aligned panels: the element form).
// Built and run by tests/test_gat16_sanitized.py; exits 0 when every result has the bits of the f32 entry points on the
// widened rows.
#include "asan_common.hpp"

// shift = 1: the 16-bit panels start one element into their blocks
static int run(int64_t N, int64_t E_want, int64_t chunk, int64_t H, int64_t C, int dtype, int out_f32, float p_drop, int shift) {
  const int64_t K = H * C;
  // a random graph with a heavy destination (row N - 1) and a heavy source (node 0), as a CSR and its transpose
  std::vector<std::vector<int32_t>> in(N), out_pos(N);
  for (int64_t e = 0; e < E_want; ++e) {
    const int32_t s = (e % 5 == 0) ? 0 : (int32_t)(rnd() % N), d = (e % 7 == 0) ? (int32_t)(N - 1) : (int32_t)(rnd() % N);
    in[d].push_back(s);
  }
  const int64_t E = E_want;
  Plan f, t;
  f.rowptr = block<int64_t>(N + 1);
  t.rowptr = block<int64_t>(N + 1);
  int32_t *col = block<int32_t>(E), *colT = block<int32_t>(E), *posT = block<int32_t>(E);
  std::vector<int32_t> dst_of(E);
  int64_t p = 0;
  for (int64_t d = 0; d < N; ++d) {
    f.rowptr[d] = p;
    for (int32_t s : in[d]) {
      col[p] = s;
      dst_of[p] = (int32_t)d;
      out_pos[s].push_back((int32_t)p);
      ++p;
    }
  }
  f.rowptr[N] = p;
  p = 0;
  for (int64_t s = 0; s < N; ++s) {
    t.rowptr[s] = p;
    for (int32_t q : out_pos[s]) {
      colT[p] = dst_of[q];
      posT[p] = q;
      ++p;
    }
  }
  t.rowptr[N] = p;
  finish_plan(f, N, E, chunk);
  finish_plan(t, N, E, chunk);
  if (chunk < 64) EXPECT(f.c.n_long > 0 && t.c.n_long > 0);

  float *el = block<float>(N * H), *er = block<float>(N * H);
  for (int64_t i = 0; i < N * H; ++i) { el[i] = rndf(); er[i] = rndf(); }
  // 16-bit panels (exactly N * K elements, + the one skipped in front when shifted) and their widened copies
  uint16_t *x16b = block<uint16_t>(N * K + shift), *g16b = block<uint16_t>(N * K + shift);
  uint16_t *x16 = x16b + shift, *g16 = g16b + shift;
  float *xf = block<float>(N * K), *gf = block<float>(N * K);
  for (int64_t i = 0; i < N * K; ++i) {
    x16[i] = narrow(dtype, rndf());
    g16[i] = narrow(dtype, rndf());
    xf[i] = widen(dtype, x16[i]);
    gf[i] = widen(dtype, g16[i]);
  }
  int64_t *rng = block<int64_t>(2), *rng_f = block<int64_t>(2), *rng_used = block<int64_t>(2);
  rng[0] = rng_f[0] = rng_used[0] = 0x1234567;
  rng[1] = rng_f[1] = rng_used[1] = 3;
  const float slope = 0.2f;

  // ---- forward: F, then the 16-bit entry point
  f.set_partial(ggl_gat_partial_bytes(f.c.n_chunks, H, C));
  float *out_f = block<float>(N * K), *rmax_f = block<float>(N * H), *rden_f = block<float>(N * H);
  CHECK(ggl_gat_fused_fwd(&f.c, col, el, er, xf, slope, H, C, p_drop, p_drop > 0 ? rng_f : nullptr, out_f, rmax_f, rden_f,
                          nullptr));
  const int odt = out_f32 ? GGL_F32 : dtype;
  const size_t osz = out_f32 ? 4 : 2;
  const int64_t oshift = out_f32 ? 0 : shift;
  char *outb = block<char>((N * K + oshift) * osz);
  void *out = outb + oshift * osz;
  float *rmax = block<float>(N * H), *rden = block<float>(N * H);
  CHECK(ggl_gat_fused_fwd_x16(&f.c, col, el, er, dtype, x16, slope, H, C, p_drop, p_drop > 0 ? rng : nullptr, odt, out, rmax,
                              rden, nullptr));
  if (p_drop > 0) EXPECT(rng[1] == 4 && rng_f[1] == 4);
  EXPECT(same(rmax, rmax_f, N * H) && same(rden, rden_f, N * H));
  float *seen = block<float>(N * K);      // the widened output the backward reads
  for (int64_t i = 0; i < N * K; ++i) {
    if (out_f32) {
      EXPECT(same(&static_cast<float *>(out)[i], &out_f[i], 1));
      seen[i] = out_f[i];
    } else {
      EXPECT(static_cast<uint16_t *>(out)[i] == narrow(dtype, out_f[i]));
      seen[i] = widen(dtype, static_cast<uint16_t *>(out)[i]);
    }
  }

  // ---- backward: destination walk then source walk, F on (xf, gf, seen), then the 16-bit entry points
  f.set_partial(ggl_partial_bytes(GGL_F32, f.c.n_chunks, H, 0));
  t.set_partial(ggl_partial_bytes(GGL_F32, t.c.n_chunks, K + H, 0));
  float *ad_f = block<float>(E * H * 2), *ad = block<float>(E * H * 2);
  float *ger_f = block<float>(N * H), *ger = block<float>(N * H), *gel_f = block<float>(N * H), *gel = block<float>(N * H);
  float *gx_f = block<float>(N * K);
  uint16_t *gxb = block<uint16_t>(N * K + shift), *gx = gxb + shift;
  const int64_t *ru = p_drop > 0 ? rng_used : nullptr;
  CHECK(ggl_gat_fused_bwd_dst(&f.c, col, nullptr, el, er, xf, gf, seen, rmax_f, rden_f, slope, H, C, p_drop, ru, ad_f, ad_f + 1,
                              ger_f, nullptr, nullptr));
  CHECK(ggl_gat_fused_bwd_src(&t.c, colT, posT, ad_f, ad_f + 1, gf, H, C, gx_f, gel_f, nullptr));
  const void *g_in = out_f32 ? static_cast<const void *>(gf) : static_cast<const void *>(g16);
  CHECK(ggl_gat_fused_bwd_dst_x16(&f.c, col, el, er, dtype, x16, odt, g_in, odt, out, rmax, rden, slope, H, C, p_drop, ru, ad,
                                  ad + 1, ger, nullptr));
  CHECK(ggl_gat_fused_bwd_src_x16(&t.c, colT, posT, ad, ad + 1, odt, g_in, H, C, dtype, gx, gel, nullptr));
  EXPECT(same(ad, ad_f, E * H * 2));
  EXPECT(same(ger, ger_f, N * H) && same(gel, gel_f, N * H));
  for (int64_t i = 0; i < N * K; ++i) EXPECT(gx[i] == narrow(dtype, gx_f[i]));
  for (void *b : {(void *)col, (void *)colT, (void *)posT, (void *)el, (void *)er, (void *)x16b, (void *)g16b, (void *)xf,
                  (void *)gf, (void *)rng, (void *)rng_f, (void *)rng_used, (void *)out_f, (void *)rmax_f, (void *)rden_f,
                  (void *)outb, (void *)rmax, (void *)rden, (void *)seen, (void *)ad_f, (void *)ad, (void *)ger_f, (void *)ger,
                  (void *)gel_f, (void *)gel, (void *)gx_f, (void *)gxb})
    std::free(b);
  f.release();
  t.release();
  return 0;
}

int main() {
  const int64_t shapes[3][2] = {{3, 5}, {2, 12}, {8, 8}};
  int cases = 0;
  for (int pass = 0; pass < 2; ++pass)          // 0: long rows both ways (chunk 16), aligned panels; 1: short rows, shifted panels
    for (const auto &s : shapes)
      for (int dtype : {GGL_BF16, GGL_F16})
        for (int out_f32 = 0; out_f32 < 2; ++out_f32)
          for (float p : {0.0f, 0.5f}) {
            if (run(120, 2500, pass == 0 ? 16 : 4096, s[0], s[1], dtype, out_f32, p, pass)) {
              std::fprintf(stderr, "failed: pass %d, %d x %d, dtype %d, out_f32 %d, p %g\n", pass, (int)s[0], (int)s[1], dtype,
                           out_f32, p);
              return 1;
            }
            ++cases;
          }
  std::printf("gat16 sanitized: %d cases ok\n", cases);
  return 0;
}
