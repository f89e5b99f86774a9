// A stand-alone AddressSanitizer check of GATv2's backward walk (ggl_gatv2_logit_bwd) on the host-emulated kernel sources:
// every buffer is a heap block of exactly the documented size — gz exactly E * H floats, the node arrays exactly N * H * C,
// att exactly H * C, plan->partial exactly ggl_gatv2_logit_bwd_partial_bytes(...) — so a read or write past an end aborts the
// run.  Two plan pairs: one built from UNSORTED ids (a non-NULL perm) with long rows both ways (chunk 16: hub chunks,
// partials, the merge), one from ids that arrive sorted (NULL perm on the forward plan, no long rows).  Each pair is walked
// as the backward walks it: the forward plan with self = xr, other = xl and att_rows, and without att_rows; the transposed
// plan with self = xl, other = xr, with and without add.  Shapes 1 x 1, 3 x 5 (element form), 2 x 12 and 8 x 8 (16-byte
// loads).  Built and run by tests/test_gatv2_sanitized.py; exits 0 when every output has the bits of the serial loop below.
#include "asan_common.hpp"

// the documented arithmetic, one (row, head, channel) at a time; volatile keeps every step a rounded f32 operation
static void serial(const Plan &p, const int32_t *col, const float *other, const float *self, const float *gz, const float *att,
                   float slope, int64_t H, int64_t C, const float *add, float *g_self, float *rows) {
  const int64_t K = H * C;
  for (int64_t r = 0; r < p.c.N; ++r)
    for (int64_t k = 0; k < K; ++k) {
      const int64_t h = k / C, beg = p.rowptr[r], end = p.rowptr[r + 1];
      const bool lng = end - beg > p.c.chunk;
      volatile float totD = 0.0f, totA = 0.0f;
      auto piece = [&](int64_t b, int64_t stop, volatile float &accD, volatile float &accA) {
        accD = 0.0f; accA = 0.0f;
        for (int64_t q = b; q < stop; ++q) {
          const int64_t e = p.perm ? p.perm[q] : q;
          volatile float s = other[col[q] * K + k] + self[r * K + k];
          const float w = gz[e * H + h];
          volatile float ws = w * slope, ss = s * slope;
          accD = accD + (s > 0.0f ? w : ws);
          volatile float t = w * (s > 0.0f ? s : ss);
          accA = accA + t;
        }
      };
      if (!lng) {
        piece(beg, end, totD, totA);
      } else {
        for (int64_t b = beg; b < end; b += p.c.chunk) {   // partials merged in ascending order from 0.0f
          volatile float accD, accA;
          piece(b, std::min(b + p.c.chunk, end), accD, accA);
          totD = totD + accD; totA = totA + accA;
        }
      }
      volatile float gs = att[k] * totD;
      if (add) gs = add[r * K + k] + gs;
      g_self[r * K + k] = gs;
      rows[r * K + k] = totA;
    }
}

static int walk(Plan &p, const int32_t *col, const float *other, const float *self, const float *gz, const float *att,
                float slope, int64_t N, int64_t H, int64_t C, const float *add, bool with_rows) {
  const int64_t K = H * C;
  const size_t pb = ggl_gatv2_logit_bwd_partial_bytes(p.c.n_chunks, H, C, with_rows ? 1 : 0);
  EXPECT((pb > 0) == (p.c.n_long > 0));
  p.set_partial(pb);
  float *g_self = block<float>(N * K), *rows = with_rows ? block<float>(N * K) : nullptr;
  float *w_self = block<float>(N * K), *w_rows = block<float>(N * K);
  CHECK(ggl_gatv2_logit_bwd(&p.c, col, other, self, gz, att, slope, H, C, add, g_self, rows, nullptr));
  serial(p, col, other, self, gz, att, slope, H, C, add, w_self, w_rows);
  EXPECT(same(g_self, w_self, N * K));
  if (with_rows) EXPECT(same(rows, w_rows, N * K));
  std::free(g_self); std::free(rows); std::free(w_self); std::free(w_rows);
  return 0;
}

static int run(int64_t N, int64_t E, int64_t chunk, bool sorted, int64_t H, int64_t C) {
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
  else EXPECT(f.c.n_long == 0 && t.c.n_long == 0);
  // col[p] = source of sorted position p; colT[q] = destination of transposed position q; each plan's perm is the caller's
  // edge number of its positions
  int32_t *col = block<int32_t>(E), *colT = block<int32_t>(E);
  for (int64_t p = 0; p < E; ++p) col[p] = src[f.perm ? f.perm[p] : p];
  for (int64_t q = 0; q < E; ++q) colT[q] = dst[t.perm ? t.perm[q] : q];

  const float slope = 0.2f;
  float *xl = block<float>(N * K), *xr = block<float>(N * K), *gv = block<float>(N * K), *att = block<float>(K);
  float *gz = block<float>(E * H);                 // exactly E * H floats, the caller's order
  for (int64_t i = 0; i < N * K; ++i) { xl[i] = rndf(); xr[i] = rndf(); gv[i] = rndf(); }
  for (int64_t i = 0; i < K; ++i) att[i] = rndf();
  for (int64_t i = 0; i < E * H; ++i) gz[i] = rndf();

  if (walk(f, col, xl, xr, gz, att, slope, N, H, C, nullptr, true)) return 1;    // g_xr and R
  if (walk(f, col, xl, xr, gz, att, slope, N, H, C, nullptr, false)) return 1;   // g_xr alone
  if (walk(t, colT, xr, xl, gz, att, slope, N, H, C, nullptr, false)) return 1;  // the logit part of g_xl
  if (walk(t, colT, xr, xl, gz, att, slope, N, H, C, gv, false)) return 1;       // g_xl with add = gv
  for (void *b : {(void *)col, (void *)colT, (void *)xl, (void *)xr, (void *)gv, (void *)att, (void *)gz}) std::free(b);
  f.release();
  t.release();
  return 0;
}

int main() {
  const int64_t shapes[4][2] = {{1, 1}, {3, 5}, {2, 12}, {8, 8}};
  int cases = 0;
  for (int pass = 0; pass < 2; ++pass)   // 0: unsorted ids (perm), long rows both ways; 1: sorted ids (NULL perm), short rows
    for (const auto &s : shapes) {
      if (run(120, 2500, pass == 0 ? 16 : 4096, pass == 1, s[0], s[1])) {
        std::fprintf(stderr, "failed: pass %d, %d x %d\n", pass, (int)s[0], (int)s[1]);
        return 1;
      }
      ++cases;
    }
  std::printf("gatv2 logit backward sanitized: %d cases ok\n", cases);
  return 0;
}
