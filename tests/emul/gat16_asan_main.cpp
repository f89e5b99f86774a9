// A stand-alone AddressSanitizer check of the fused GAT on 16-bit rows (ggl_gat_fused_{fwd,bwd_dst,bwd_src}_x16) on the
// host-emulated kernel sources: every buffer is a heap block of exactly the documented size, so a read or write past an end
// aborts the run.  Shapes 3 x 5 (element form), 2 x 12 (8-byte loads) and 8 x 8 (16-byte loads), bf16 and f16, 16-bit and f32
// out, with and without attention dropout; once on a plan with long rows both ways (hub chunks, f32 partials, the merges) and
// once with x, g and out starting ONE element into their blocks (2-byte aligned panels: the element form).
// Built and run by tests/test_gat16_sanitized.py; exits 0 when every result has the bits of the f32 entry points on the
// widened rows.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ggl_mpops.h"

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

static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }
static float rndf() { return (float)((int)(rnd() >> 8) % 4001 - 2000) / 1024.0f; }

template <typename T>
static T *block(size_t n) { return static_cast<T *>(std::malloc((n ? n : 1) * sizeof(T))); }

// 16-bit <-> f32 as the library documents them: exact widening, round-to-nearest-even narrowing
static float widen(int dtype, uint16_t b) {
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
static uint16_t narrow(int dtype, float f) {
  if (dtype == GGL_BF16) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    return (uint16_t)((x + (((x >> 16) & 1u) + 0x7fffu)) >> 16);   // (no NaNs in this program)
  }
  const _Float16 h = (_Float16)f;
  uint16_t b;
  std::memcpy(&b, &h, 2);
  return b;
}

struct Plan {
  ggl_segplan_t c{};
  int64_t *rowptr = nullptr, *chunk_ptr = nullptr;
  int32_t *long_rows = nullptr;
  void release() { std::free(rowptr); std::free(chunk_ptr); std::free(long_rows); }
};

static void finish_plan(Plan &p, int64_t N, int64_t E, int64_t chunk) {
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
  const size_t pfb = ggl_gat_partial_bytes(f.c.n_chunks, H, C);
  f.c.partial = pfb ? std::malloc(pfb) : nullptr;
  f.c.partial_bytes = pfb;
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
  EXPECT(std::memcmp(rmax, rmax_f, N * H * 4) == 0 && std::memcmp(rden, rden_f, N * H * 4) == 0);
  float *seen = block<float>(N * K);      // the widened output the backward reads
  for (int64_t i = 0; i < N * K; ++i) {
    if (out_f32) {
      EXPECT(std::memcmp(&static_cast<float *>(out)[i], &out_f[i], 4) == 0);
      seen[i] = out_f[i];
    } else {
      EXPECT(static_cast<uint16_t *>(out)[i] == narrow(dtype, out_f[i]));
      seen[i] = widen(dtype, static_cast<uint16_t *>(out)[i]);
    }
  }
  std::free(f.c.partial);

  // ---- backward: destination walk then source walk, F on (xf, gf, seen), then the 16-bit entry points
  const size_t pdb = ggl_partial_bytes(GGL_F32, f.c.n_chunks, H, 0), psb = ggl_partial_bytes(GGL_F32, t.c.n_chunks, K + H, 0);
  f.c.partial = pdb ? std::malloc(pdb) : nullptr;
  t.c.partial = psb ? std::malloc(psb) : nullptr;
  f.c.partial_bytes = pdb;
  t.c.partial_bytes = psb;
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
  EXPECT(std::memcmp(ad, ad_f, E * H * 2 * 4) == 0);
  EXPECT(std::memcmp(ger, ger_f, N * H * 4) == 0 && std::memcmp(gel, gel_f, N * H * 4) == 0);
  for (int64_t i = 0; i < N * K; ++i) EXPECT(gx[i] == narrow(dtype, gx_f[i]));
  std::free(f.c.partial);
  std::free(t.c.partial);
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
