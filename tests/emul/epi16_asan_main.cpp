// A stand-alone AddressSanitizer check of the fused epilogue on 16-bit rows (ggl_spmm_epi_x16, ggl_bias_act_{fwd,bwd}_x16) on
// the host-emulated kernel sources: x, add, out, y, ga, gbias and the workspace are heap blocks of exactly the documented
// sizes, so a read or write past an end aborts the run.  Widths 7 (one element per lane), 8, 44 (ragged lanes) and 264 (more
// than one pass of a lane group), bf16 and f16, 16-bit and f32 out, sum and mean, with and without dropout; once on a plan
// with long rows and once with x / out / add rows ld > K elements apart (the last row is K long: no slack behind it).
// Built and run by tests/test_epi16_sanitized.py; exits 0 when every result has the bits of the f32 entry points on the
// widened rows, rounded once.
#include "asan_common.hpp"

// rows `ld` elements apart, the last one K long: (N - 1) * ld + K elements exactly
static size_t panel(int64_t N, int64_t K, int64_t ld) { return N > 0 ? (size_t)((N - 1) * ld + K) : 0; }

static int run_epi(int64_t N, int64_t E, int64_t chunk, int64_t K, int dtype, int out_f32, int mean, int has_add, float p_drop,
                   int64_t pad) {
  // a random CSR with a heavy destination (row N - 1), already in destination order (perm = NULL)
  std::vector<std::vector<int32_t>> in(N);
  for (int64_t e = 0; e < E; ++e) in[(e % 3 == 0) ? N - 1 : (int64_t)(rnd() % N)].push_back((int32_t)(rnd() % N));
  Plan plan;
  plan.rowptr = block<int64_t>(N + 1);
  int32_t *col = block<int32_t>(E);
  float *w = block<float>(E);
  int64_t p = 0;
  for (int64_t d = 0; d < N; ++d) {
    plan.rowptr[d] = p;
    for (int32_t s : in[d]) { col[p] = s; w[p] = (float)(rnd() % 1000) / 1000.0f; ++p; }
  }
  plan.rowptr[N] = p;
  finish_plan(plan, N, E, chunk);
  plan.set_partial(ggl_partial_bytes(GGL_F32, plan.c.n_chunks, K, 0));
  const int64_t ld = K + pad;
  const size_t n_el = panel(N, K, ld);
  uint16_t *x16 = block<uint16_t>(n_el), *add16 = has_add ? block<uint16_t>(n_el) : nullptr;
  float *x32 = block<float>(n_el), *add32 = has_add ? block<float>(n_el) : nullptr, *bias = block<float>(K);
  for (size_t i = 0; i < n_el; ++i) {
    x16[i] = narrow(dtype, rndf()); x32[i] = widen(dtype, x16[i]);
    if (has_add) { add16[i] = narrow(dtype, rndf()); add32[i] = widen(dtype, add16[i]); }
  }
  for (int64_t k = 0; k < K; ++k) bias[k] = rndf();
  float *want = block<float>(n_el), *got32 = block<float>(n_el);
  uint16_t *got16 = block<uint16_t>(n_el);
  int64_t *rng = block<int64_t>(2);
  rng[0] = 99; rng[1] = 5;
  CHECK(ggl_spmm_epi_ex(&plan.c, col, w, 1, x32, ld, K, want, ld, 0, mean, add32, has_add ? ld : 0, bias, 1, p_drop,
                        p_drop > 0 ? rng : nullptr, 0, 0, 1, nullptr));
  const int64_t moved = rng[1];
  EXPECT(moved == (p_drop > 0 ? 6 : 5));
  rng[1] = 5;
  void *out = out_f32 ? (void *)got32 : (void *)got16;
  CHECK(ggl_spmm_epi_x16(&plan.c, col, w, 1, dtype, x16, ld, K, out_f32 ? GGL_F32 : dtype, out, ld, mean, add16, has_add ? ld : 0,
                         bias, 1, p_drop, p_drop > 0 ? rng : nullptr, 0, 0, 1, nullptr));
  EXPECT(rng[1] == moved);
  for (int64_t r = 0; r < N; ++r)
    for (int64_t k = 0; k < K; ++k) {
      const size_t i = (size_t)(r * ld + k);
      if (out_f32) EXPECT(same(&got32[i], &want[i], 1));
      else EXPECT(got16[i] == narrow(dtype, want[i]));
    }
  plan.release(); std::free(col); std::free(w);
  std::free(x16); std::free(add16); std::free(x32); std::free(add32); std::free(bias); std::free(want); std::free(got32);
  std::free(got16); std::free(rng);
  return 0;
}

static int run_bias_act(int64_t N, int64_t K, int dtype, int relu, float p_drop, int redraw) {
  const size_t n = (size_t)(N * K);
  uint16_t *a16 = block<uint16_t>(n), *y16 = block<uint16_t>(n), *g16 = block<uint16_t>(n), *ga16 = block<uint16_t>(n);
  float *a32 = block<float>(n), *y32 = block<float>(n), *g32 = block<float>(n), *ga32 = block<float>(n), *yw = block<float>(n);
  float *bias = block<float>(K), *gb16 = block<float>(K), *gb32 = block<float>(K);
  for (size_t i = 0; i < n; ++i) {
    a16[i] = narrow(dtype, rndf()); a32[i] = widen(dtype, a16[i]);
    g16[i] = narrow(dtype, rndf()); g32[i] = widen(dtype, g16[i]);
  }
  for (int64_t k = 0; k < K; ++k) bias[k] = rndf();
  int64_t *rng = block<int64_t>(2), *used = block<int64_t>(2);
  rng[0] = used[0] = 7; rng[1] = used[1] = 11;
  CHECK(ggl_bias_act_fwd(a32, bias, N, K, relu, p_drop, p_drop > 0 ? rng : nullptr, y32, nullptr));
  const int64_t moved = rng[1];
  rng[1] = 11;
  CHECK(ggl_bias_act_fwd_x16(dtype, a16, bias, N, K, relu, p_drop, p_drop > 0 ? rng : nullptr, y16, nullptr));
  EXPECT(rng[1] == moved);
  for (size_t i = 0; i < n; ++i) { EXPECT(y16[i] == narrow(dtype, y32[i])); yw[i] = widen(dtype, y16[i]); }
  const size_t wsb = ggl_bias_act_bwd_workspace_bytes(N, K);
  void *ws = std::malloc(wsb ? wsb : 1);
  const int64_t *ru = (p_drop > 0 && redraw) ? used : nullptr;
  CHECK(ggl_bias_act_bwd(g32, yw, N, K, relu, p_drop, ru, ga32, gb32, ws, wsb, nullptr));
  CHECK(ggl_bias_act_bwd_x16(dtype, g16, y16, N, K, relu, p_drop, ru, ga16, gb16, ws, wsb, nullptr));
  for (size_t i = 0; i < n; ++i) EXPECT(ga16[i] == narrow(dtype, ga32[i]));
  EXPECT(same(gb16, gb32, (size_t)K));
  std::free(a16); std::free(y16); std::free(g16); std::free(ga16); std::free(a32); std::free(y32); std::free(g32);
  std::free(ga32); std::free(yw); std::free(bias); std::free(gb16); std::free(gb32); std::free(rng); std::free(used); std::free(ws);
  return 0;
}

int main() {
  int cases = 0;
  const int dtypes[2] = {GGL_BF16, GGL_F16};
  const int64_t widths[4] = {7, 8, 44, 264};
  for (int dtype : dtypes)
    for (int64_t K : widths)
      for (int out_f32 = 0; out_f32 < 2; ++out_f32)
        for (int mean = 0; mean < 2; ++mean) {
          // short rows only; a plan with long rows (chunk 16); strided rows (ld = K + 3: 2-byte aligned rows)
          if (run_epi(40, 500, 1 << 20, K, dtype, out_f32, mean, mean, mean ? 0.0f : 0.5f, 0)) return 1;
          if (run_epi(40, 500, 16, K, dtype, out_f32, mean, 1, 0.5f, 0)) return 1;
          if (run_epi(23, 300, 16, K, dtype, out_f32, mean, 1, mean ? 0.5f : 0.0f, 3)) return 1;
          cases += 3;
        }
  for (int dtype : dtypes)
    for (int64_t K : widths)
      for (int64_t N : {37, 300}) {
        if (run_bias_act(N, K, dtype, 1, 0.0f, 0)) return 1;
        if (run_bias_act(N, K, dtype, 1, 0.5f, 1)) return 1;
        if (run_bias_act(N, K, dtype, 0, 0.5f, 1)) return 1;
        if (run_bias_act(N, K, dtype, 0, 0.5f, 0)) return 1;
        cases += 4;
      }
  // the refusals: f32 rows, bf16 -> f16, f64
  ggl_segplan_t plan{};
  int64_t rowptr[2] = {0, 0};
  plan.rowptr = rowptr; plan.N = 1; plan.chunk = 16;
  uint16_t one[8] = {0};
  EXPECT(ggl_spmm_epi_x16(&plan, nullptr, nullptr, 0, GGL_F32, one, 0, 8, GGL_F32, one, 0, 0, nullptr, 0, nullptr, 0, 0.0f, nullptr,
                          0, 0, 1, nullptr) == GGL_EDTYPE);
  EXPECT(ggl_spmm_epi_x16(&plan, nullptr, nullptr, 0, GGL_BF16, one, 0, 8, GGL_F16, one, 0, 0, nullptr, 0, nullptr, 0, 0.0f, nullptr,
                          0, 0, 1, nullptr) == GGL_EDTYPE);
  EXPECT(ggl_spmm_epi_x16(&plan, nullptr, nullptr, 0, GGL_F64, one, 0, 8, GGL_F64, one, 0, 0, nullptr, 0, nullptr, 0, 0.0f, nullptr,
                          0, 0, 1, nullptr) == GGL_EDTYPE);
  EXPECT(ggl_bias_act_fwd_x16(GGL_F32, one, nullptr, 1, 8, 0, 0.0f, nullptr, one, nullptr) == GGL_EDTYPE);
  EXPECT(ggl_bias_act_bwd_x16(GGL_F64, one, one, 1, 8, 0, 0.0f, nullptr, one, nullptr, nullptr, 0, nullptr) == GGL_EDTYPE);
  std::printf("%d cases ok\n", cases);
  return 0;
}
