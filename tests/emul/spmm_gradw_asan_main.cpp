// A stand-alone AddressSanitizer check of gspmm's weight gradient (ggl_spmm_grad_w, sum and mean, every pair of f32 / bf16 /
// f16 panels) on the host-emulated kernel sources: gw, the scratch and the 16-bit panels are heap blocks of exactly the
// documented sizes, so a read or write past an end aborts the run.  Built and run by tests/test_spmm_gradw_sanitized.py;
// exits 0 when every result equals a plain serial restatement, bit for bit.
#include "asan_common.hpp"

// exactly n bytes (never a zero-byte block's NULL)
static void *bytes(size_t n) { return std::malloc(n ? n : 1); }

// a panel of `n` elements of `dtype` in a block of exactly n * size bytes, and its widened values
static void *panel(int dtype, int64_t n, std::vector<float> &wide) {
  wide.resize((size_t)n);
  if (dtype == GGL_F32) {
    float *p = block<float>((size_t)n);
    for (int64_t i = 0; i < n; ++i) wide[i] = p[i] = rndf();
    return p;
  }
  uint16_t *p = block<uint16_t>((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    p[i] = narrow(dtype, rndf());
    wide[i] = widen(dtype, p[i]);
  }
  return p;
}

static int run(int64_t N_src, int64_t N_dst, int64_t E, int64_t K, int xd, int gd, bool mean, bool permuted) {
  // destination-sorted positions; the caller's edge order is a rotation of them when `permuted`
  std::vector<std::vector<int32_t>> in((size_t)N_dst);
  for (int64_t e = 0; e < E; ++e) in[(e % 7 == 0) ? N_dst - 1 : rnd() % N_dst].push_back((int32_t)(rnd() % N_src));
  int64_t *rowptr = block<int64_t>((size_t)N_dst + 1);
  int32_t *col = block<int32_t>((size_t)E), *rowidx = block<int32_t>((size_t)E), *perm = permuted ? block<int32_t>((size_t)E) : nullptr;
  int64_t p = 0;
  for (int64_t d = 0; d < N_dst; ++d) {
    rowptr[d] = p;
    for (int32_t s : in[(size_t)d]) {
      col[p] = s;
      rowidx[p] = (int32_t)d;
      if (perm) perm[p] = (int32_t)((p + 17) % E);
      ++p;
    }
  }
  rowptr[N_dst] = p;
  EXPECT(p == E);
  ggl_segplan_t plan{};
  plan.rowptr = rowptr;
  plan.perm = perm;
  plan.N = N_dst;
  plan.E = E;
  plan.chunk = 1 << 20;
  std::vector<float> xf, gf;
  void *x = panel(xd, N_src * K, xf), *g = panel(gd, N_dst * K, gf);
  const size_t sb = ggl_spmm_grad_w_scratch_bytes(E, N_dst, K, xd, mean ? 1 : 0);
  EXPECT(!mean || E == 0 || sb >= (size_t)(N_dst * K) * sizeof(float));   // (no edges: nothing runs, no scratch)
  void *scratch = sb ? bytes(sb) : nullptr;
  float *gw = block<float>((size_t)E);
  CHECK(ggl_spmm_grad_w(&plan, col, rowidx, xd, x, gd, g, mean ? rowptr : nullptr, K, gw, scratch, nullptr));
  for (int64_t q = 0; q < E; ++q) {
    const int64_t d = rowidx[q];
    const float cnt = (float)(rowptr[d + 1] - rowptr[d]);
    float acc = 0.0f;
    for (int64_t k = 0; k < K; ++k) {
      const float gv = mean ? gf[(size_t)(d * K + k)] / cnt : gf[(size_t)(d * K + k)];
      const float prod = xf[(size_t)((int64_t)col[q] * K + k)] * gv;
      acc = acc + prod;
    }
    const float got = gw[perm ? perm[q] : q];
    EXPECT(same(&got, &acc, 1));
  }
  for (void *b : {(void *)rowptr, (void *)col, (void *)rowidx, (void *)perm, x, g, scratch, (void *)gw}) std::free(b);
  return 0;
}

int main() {
  int cases = 0;
  const int dts[3] = {GGL_F32, GGL_BF16, GGL_F16};
  for (int xd : dts)
    for (int gd : dts)
      for (int mean = 0; mean < 2; ++mean)
        for (int64_t K : {1, 7, 8, 12, 40, 264}) {
          if (run(500, 200, 5000, K, xd, gd, mean != 0, (K & 1) == 0)) return 1;
          ++cases;
        }
  for (int64_t E : {0, 1, 255, 256, 257}) {
    if (run(300, 300, E, 8, GGL_BF16, GGL_F32, true, E > 1)) return 1;
    ++cases;
  }
  // refusals: another dtype, mean without its scratch
  {
    ggl_segplan_t plan{};
    int64_t rowptr[2] = {0, 1};
    int32_t col[1] = {0}, rowidx[1] = {0};
    plan.rowptr = rowptr;
    plan.N = 1;
    plan.E = 1;
    double x[4] = {0}, gw[1];
    if (ggl_spmm_grad_w(&plan, col, rowidx, GGL_F64, x, GGL_F32, x, nullptr, 4, (float *)gw, nullptr, nullptr) != GGL_EDTYPE ||
        ggl_spmm_grad_w(&plan, col, rowidx, GGL_F32, x, GGL_F32, x, rowptr, 4, (float *)gw, nullptr, nullptr) != GGL_EINVAL) {
      std::fprintf(stderr, "a bad call was accepted\n");
      return 1;
    }
  }
  std::printf("spmm_grad_w sanitized: %d cases ok\n", cases);
  return 0;
}
