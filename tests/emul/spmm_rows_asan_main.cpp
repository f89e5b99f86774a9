// A stand-alone AddressSanitizer check of the restricted plan pair (ggl_plan_rows_*) and ggl_bias_grad_rows on the host-emulated
// kernel sources: every buffer is a heap block of exactly the documented size, so a read or write past an end aborts the run.
// Built and run by tests/test_spmm_rows_sanitized.py; exits 0 when every result equals a plain serial restatement.
#include "asan_common.hpp"

static int run(int64_t N, int64_t E_want, const std::vector<int64_t> &rows_v, bool weighted, int64_t K) {
  // a random graph as a CSR pair: forward (grouped by destination) and transposed (grouped by source), ascending inside a row
  std::vector<std::vector<int32_t>> in(N), out(N);
  for (int64_t e = 0; e < E_want; ++e) {
    const int32_t s = rnd() % N, d = (e % 7 == 0) ? (int32_t)(N - 1) : (int32_t)(rnd() % N);   // row N - 1 is heavy
    in[d].push_back(s);
  }
  const int64_t R = (int64_t)rows_v.size();
  int64_t E = 0;
  for (auto &v : in) E += (int64_t)v.size();
  int64_t *rowptr = block<int64_t>(N + 1), *rowptrT = block<int64_t>(N + 1);
  int32_t *col = block<int32_t>(E), *colT = block<int32_t>(E), *wperm = block<int32_t>(E), *wpermT = block<int32_t>(E);
  float *w = weighted ? block<float>(E) : nullptr;
  // the caller's edge order is the forward order here (wperm = identity); the transposed plan permutes it
  int64_t p = 0;
  for (int64_t d = 0; d < N; ++d) {
    rowptr[d] = p;
    for (int32_t s : in[d]) {
      col[p] = s;
      wperm[p] = (int32_t)p;
      if (w) w[p] = (float)(rnd() % 1000) / 1000.0f;
      out[s].push_back((int32_t)p);
      ++p;
    }
  }
  rowptr[N] = p;
  std::vector<int32_t> dst_of(E);
  for (int64_t d = 0; d < N; ++d)
    for (int64_t q = rowptr[d]; q < rowptr[d + 1]; ++q) dst_of[q] = (int32_t)d;
  p = 0;
  for (int64_t s = 0; s < N; ++s) {
    rowptrT[s] = p;
    for (int32_t q : out[s]) {
      colT[p] = dst_of[q];
      wpermT[p] = q;
      ++p;
    }
  }
  rowptrT[N] = p;

  int64_t *rows = block<int64_t>(R);
  for (int64_t i = 0; i < R; ++i) rows[i] = rows_v[i];
  const size_t wsb = ggl_plan_rows_workspace_bytes(E, N, R);
  void *ws = std::malloc(wsb);
  int32_t *rank = block<int32_t>(N);
  CHECK(ggl_plan_rows_rank(rows, R, N, rank, ws, wsb, nullptr));
  for (int64_t i = 0, r = 0; i < N; ++i) {
    const bool listed = r < R && rows[r] == i;
    EXPECT(rank[i] == (listed ? (int32_t)r : -1));
    r += listed;
  }
  // forward: a segmented copy
  int64_t *rowptr_r = block<int64_t>(R + 1);
  int64_t E_r = -1, E_t = -1;
  CHECK(ggl_plan_rows_fwd_rowptr(rowptr, rows, R, rowptr_r, ws, wsb, nullptr, &E_r));
  int32_t *col_r = block<int32_t>(E_r);
  float *w_r = weighted ? block<float>(E_r) : nullptr;
  CHECK(ggl_plan_rows_fwd_fill(rowptr, col, w, wperm, rows, R, rowptr_r, E_r, col_r, w_r, nullptr));
  int64_t q = 0;
  for (int64_t r = 0; r < R; ++r) {
    EXPECT(rowptr_r[r] == q);
    for (int64_t e = rowptr[rows[r]]; e < rowptr[rows[r] + 1]; ++e, ++q) {
      EXPECT(col_r[q] == col[e]);
      if (w) EXPECT(w_r[q] == w[e]);
    }
  }
  EXPECT(rowptr_r[R] == q && E_r == q);
  // transposed: a filter
  int32_t *pos = block<int32_t>(E + 1);
  int64_t *rowptrT_r = block<int64_t>(N + 1);
  CHECK(ggl_plan_rows_bwd_rowptr(rowptrT, colT, N, E, rank, pos, rowptrT_r, ws, wsb, nullptr, &E_t));
  EXPECT(E_t == E_r);
  int32_t *colT_r = block<int32_t>(E_r);
  float *wT_r = weighted ? block<float>(E_r) : nullptr;
  CHECK(ggl_plan_rows_bwd_fill(colT, w, wpermT, E, rank, pos, colT_r, wT_r, nullptr));
  q = 0;
  for (int64_t s = 0; s < N; ++s) {
    EXPECT(rowptrT_r[s] == q);
    for (int64_t e = rowptrT[s]; e < rowptrT[s + 1]; ++e) {
      if (rank[colT[e]] < 0) continue;
      EXPECT(colT_r[q] == rank[colT[e]]);
      if (w) EXPECT(wT_r[q] == w[wpermT[e]]);
      ++q;
    }
  }
  EXPECT(rowptrT_r[N] == q && q == E_r);
  // the bias gradient over the listed rows against the full pass over the scattered gradient
  float *g = block<float>(R * K), *gfull = block<float>(N * K), *ga = block<float>(N * K);
  for (int64_t i = 0; i < N * K; ++i) gfull[i] = 0.0f;
  for (int64_t r = 0; r < R; ++r)
    for (int64_t k = 0; k < K; ++k) gfull[rows[r] * K + k] = g[r * K + k] = (float)((int)(rnd() % 2001) - 1000) / 512.0f;
  const size_t bwb = ggl_bias_act_bwd_workspace_bytes(N, K);
  void *bws = std::malloc(bwb ? bwb : 1);
  float *gb = block<float>(K), *gb_full = block<float>(K);
  CHECK(ggl_bias_grad_rows(g, rows, R, N, K, gb, bws, bwb, nullptr));
  CHECK(ggl_bias_act_bwd(gfull, nullptr, N, K, 0, 0.0f, nullptr, ga, gb_full, bws, bwb, nullptr));
  for (int64_t k = 0; k < K; ++k) EXPECT(gb[k] == gb_full[k]);
  for (void *b : {(void *)rowptr, (void *)rowptrT, (void *)col, (void *)colT, (void *)wperm, (void *)wpermT, (void *)w, (void *)rows,
                  ws, (void *)rank, (void *)rowptr_r, (void *)col_r, (void *)w_r, (void *)pos, (void *)rowptrT_r, (void *)colT_r,
                  (void *)wT_r, (void *)g, (void *)gfull, (void *)ga, bws, (void *)gb, (void *)gb_full})
    std::free(b);
  return 0;
}

int main() {
  rnd_state = 12345u;   // this program's own sequence
  const int64_t N = 300;
  std::vector<int64_t> every, some;
  for (int64_t i = 0; i < N; ++i) {
    every.push_back(i);
    if (i == 0 || i == N - 1 || rnd() % 12 == 0) some.push_back(i);
  }
  const std::vector<std::vector<int64_t>> lists = {{}, {17}, {N - 1}, some, every};
  int cases = 0;
  for (const auto &rows : lists)
    for (int weighted = 0; weighted < 2; ++weighted)
      for (int64_t K : {4, 8, 48}) {
        if (run(N, 6000, rows, weighted != 0, K)) return 1;
        ++cases;
      }
  if (run(1, 0, {0}, true, 4) || run(5, 0, {1, 3}, false, 8)) return 1;   // no edges at all
  // bad lists are errors, not writes through a bad rank
  int64_t bad[3][2] = {{5, 3}, {4, 4}, {2, 300}};
  int32_t *rank = block<int32_t>(N);
  void *ws = std::malloc(ggl_plan_rows_workspace_bytes(0, N, 2));
  for (auto &b : bad)
    if (ggl_plan_rows_rank(b, 2, N, rank, ws, ggl_plan_rows_workspace_bytes(0, N, 2), nullptr) == GGL_OK) {
      std::fprintf(stderr, "a bad row list was accepted\n");
      return 1;
    }
  std::free(rank);
  std::free(ws);
  std::printf("spmm_rows sanitized: %d cases ok\n", cases + 2);
  return 0;
}
