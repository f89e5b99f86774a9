// libggl_torch.so — TORCH_LIBRARY(ggl, ...): the seven operators of gammagl/mpops/torch_ext registered with the
// PyTorch dispatcher FROM C++, the style the reference names as intended (docs/.../register_cpp_ops.md:29-31) but does
// not use (src/operators.cpp:51-59 binds pybind11 free functions).  An op call is dispatcher -> this file -> C ABI
// (include/ggl_mpops.h) -> kernel: no Python frame on the path, callable from C++ / TorchScript / torch.compile.
//
//   ggl::segment_sum / segment_mean (Tensor x, Tensor index, int N) -> Tensor         src/segment_{sum,mean}.cpp
//   ggl::segment_max                (Tensor x, Tensor index, int N) -> (Tensor, Tensor)  src/segment_max.cpp (+ argmax)
//   ggl::segment_softmax            (Tensor x, Tensor index, int N) -> Tensor         utils/softmax.py:10-36 as one op
//   ggl::spmm_sum / spmm_mean / spmm_max (Tensor index, Tensor? weight, Tensor x) -> Tensor   src/gspmm.cpp:26-202
//   ggl::bspmm_sum                  (Tensor index, Tensor weight, Tensor x) -> Tensor   src/gspmm.cpp:204-260
//
// Backend keys: CUDA (= HIP on ROCm) -> libggl_mpops_hip.so, CPU -> libggl_mpops_host.so (the host build of the same
// kernel sources), both resolved with dlopen from the directory this library sits in — a missing kernel library is a
// loud error at the first call of that device, nothing is computed anywhere else.  Autograd: torch::autograd::Function
// per op, same formulas as the reference's (segment_sum.cpp:43-54, segment_mean.cpp:44-63, segment_max.cpp:48-61,
// gspmm.cpp:57-80,...).  Meta: shapes only.
//
// What lives here besides the registrations is the host side of the op library, the same one gammagl_amd/ops.py
// implements (the two are checked against each other bit for bit, tests/test_torch_cpp.py).  The launch DECISIONS —
// thresholds, padded widths, which walk a gradient takes — are not written twice: both hosts ask the kernel library
// (ggl_policy_*, include/ggl_mpops.h); what each host owns is the plumbing around them:
//   * plan cache keyed on (storage, offset, shape, version, N) of the id tensor, entries die with the storage;
//   * long-row threshold = f(E) (auto_chunk), row hand-out order in id windows, XCD runs for graphs with locality;
//   * rows of K % 4 != 0 / K > 256 && K % 64 != 0 floats aggregate on one padded copy;
//   * edge weights seen twice on a plan are kept in sorted order (w_by_pos);
//   * f16 / bf16 sums walk rows in one piece, hub rows through ggl_segment_hub16 where the build has it;
//   * spmm-mean backward = rows pre-divided by their count + the plain transposed SpMM-sum.
#include <ATen/ATen.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPGraphsC10Utils.h>
#include <c10/hip/HIPStream.h>
#include <dlfcn.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <list>
#include <memory>
#include <mutex>
#include <string>

#include "ggl_mpops.h"

namespace ggl_torch {

using at::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

// ---------------------------------------------------------------------------------------------------------------
// The C ABI of one build of the kernel library, resolved at run time (both builds export the same names).
// ---------------------------------------------------------------------------------------------------------------
#define GGL_FNS(X)                                                                                                  \
  X(ggl_abi_version) X(ggl_last_error) X(ggl_plan_workspace_bytes) X(ggl_plan_build) X(ggl_plan_long_workspace_bytes) \
  X(ggl_plan_long_count) X(ggl_plan_long_fill) X(ggl_partial_bytes) X(ggl_gather_i64_to_i32) X(ggl_gather_rows_f32)  \
  X(ggl_segment_sum) X(ggl_segment_mean) X(ggl_segment_max) X(ggl_segment_hub16_supported) X(ggl_segment_hub16)      \
  X(ggl_segment_sum_bwd) X(ggl_segment_mean_bwd) X(ggl_segment_max_bwd) X(ggl_spmm_sum) X(ggl_spmm_mean)             \
  X(ggl_spmm_max) X(ggl_spmm_mean_bwd) X(ggl_spmm_max_bwd) X(ggl_bspmm_sum) X(ggl_bspmm_grad_w)                      \
  X(ggl_bspmm_grad_w_sorted_scratch_bytes) X(ggl_bspmm_grad_w_sorted)                                                \
  X(ggl_spmm_grad_w_scratch_bytes) X(ggl_spmm_grad_w)                                                                \
  X(ggl_gat_partial_bytes) X(ggl_gat_bwd_dst_partial_bytes) X(ggl_gat_bwd_src_partial_bytes)                          \
  X(ggl_gat_fast_bwd_dst_partial_bytes) X(ggl_gat_fused_fwd) X(ggl_gat_fused_bwd_dst) X(ggl_gat_fused_bwd_src)         \
  X(ggl_gat_fused_fwd_x16) X(ggl_gat_fused_bwd_dst_x16) X(ggl_gat_fused_bwd_src_x16)                                    \
  X(ggl_edge_softmax_agg_fwd) X(ggl_edge_softmax_agg_bwd_dst) X(ggl_edge_softmax_agg_bwd_src)                          \
  X(ggl_dot_attn_supported) X(ggl_policy_dot_attn_fused) X(ggl_dot_attn_fwd)                                           \
  X(ggl_gatv2_supported) X(ggl_policy_gatv2_fused) X(ggl_gatv2_fwd) X(ggl_gatv2_logit_bwd_partial_bytes)                \
  X(ggl_gatv2_logit_bwd) X(ggl_colsum_workspace_bytes) X(ggl_colsum_f32)                                               \
  X(ggl_gat_fast_supported) X(ggl_gat_fast_fwd) X(ggl_gat_fast_bwd) X(ggl_bias_act_fwd)                                \
  X(ggl_bias_act_bwd_workspace_bytes) X(ggl_bias_act_bwd) X(ggl_spmm_epi_ex) X(ggl_segment_epi)                        \
  X(ggl_sample_hop_workspace_bytes) X(ggl_sample_hop)                                                                \
  X(ggl_policy_chunk) X(ggl_policy_spmm_width) X(ggl_policy_head_channels) X(ggl_policy_mean_bwd_prescale)            \
  X(ggl_policy_gradw_sorted) X(ggl_policy_xcd_run_rows) X(ggl_policy_row_order)                                     \
  X(ggl_spmm_max_mask_bytes) X(ggl_spmm_max_mask) X(ggl_spmm_max_bwd_mask) X(ggl_get_option)                         \
  X(ggl_spmm_max_bwd32) X(ggl_policy_maxbwd_form)                                                                   \
  X(ggl_segment_softmax_supported) X(ggl_segment_softmax_partial_bytes) X(ggl_segment_softmax_fwd) X(ggl_segment_softmax_bwd) \
  X(ggl_policy_softmax_sublanes) X(ggl_spmm_sum_x16) X(ggl_spmm_mean_x16) X(ggl_spmm_mean_bwd_x16)                    \
  X(ggl_plan_rows_workspace_bytes) X(ggl_plan_rows_rank) X(ggl_plan_rows_fwd_rowptr) X(ggl_plan_rows_fwd_fill)        \
  X(ggl_plan_rows_bwd_rowptr) X(ggl_plan_rows_bwd_fill) X(ggl_bias_grad_rows)                                          \
  X(ggl_spmm_epi_x16) X(ggl_bias_act_fwd_x16) X(ggl_bias_act_bwd_x16)                                                \
  X(ggl_linear_bias_act_bwd) X(ggl_policy_linear_epi_bwd)                                                             \
  X(ggl_segment_multi_partial_bytes) X(ggl_segment_multi_fwd) X(ggl_segment_multi_bwd)

struct Api {
  void *handle = nullptr;
  std::string path;
#define X(n) decltype(&::n) n = nullptr;
  GGL_FNS(X)
#undef X
};

static std::string here() {
  Dl_info info;
  if (dladdr(reinterpret_cast<void *>(&here), &info) == 0 || info.dli_fname == nullptr) return ".";
  std::string p(info.dli_fname);
  auto slash = p.rfind('/');
  return slash == std::string::npos ? "." : p.substr(0, slash);
}

static Api load(const char *env, const char *file, const char *what) {
  Api a;
  const char *over = std::getenv(env);
  a.path = over != nullptr ? std::string(over) : here() + "/" + file;
  a.handle = dlopen(a.path.c_str(), RTLD_NOW | RTLD_LOCAL);
  TORCH_CHECK(a.handle != nullptr, "gammagl_amd: cannot load ", a.path, " (", dlerror(), "): ", what,
              " tensors are served by this library only — build it with `make -C gammagl_amd/csrc`");
#define X(n)                                                                     \
  a.n = reinterpret_cast<decltype(a.n)>(dlsym(a.handle, #n));                    \
  TORCH_CHECK(a.n != nullptr, "gammagl_amd: ", a.path, " does not export " #n);
  GGL_FNS(X)
#undef X
  TORCH_CHECK(a.ggl_abi_version() == GGL_ABI_VERSION, "gammagl_amd: ", a.path, " has C ABI version ",
              a.ggl_abi_version(), ", this binding was built against ", GGL_ABI_VERSION);
  return a;
}

static const Api &api_for(const c10::Device &d) {
  if (d.is_cuda()) {
    static const Api hip = load("GGL_TORCH_HIP_LIB", "libggl_mpops_hip.so", "GPU");
    return hip;
  }
  TORCH_CHECK(d.is_cpu(), "gammagl_amd: no kernels for device ", d);
  static const Api host = load("GGL_TORCH_HOST_LIB", "libggl_mpops_host.so", "CPU");
  return host;
}

static void check(const Api &a, int rc) {
  if (rc == GGL_OK) return;
  const char *m = a.ggl_last_error();
  std::string msg(m != nullptr ? m : "");
  TORCH_CHECK_INDEX(rc != GGL_EINDEX, msg);
  TORCH_CHECK(false, "ggl_mpops error ", rc, ": ", msg);
}

static void *stream_of(const c10::Device &d) {
  return d.is_cuda() ? static_cast<void *>(c10::hip::getCurrentHIPStream(d.index()).stream()) : nullptr;
}

static int dtype_code(const Tensor &t) {
  switch (t.scalar_type()) {
    case at::kByte: return GGL_U8;
    case at::kChar: return GGL_I8;
    case at::kShort: return GGL_I16;
    case at::kInt: return GGL_I32;
    case at::kLong: return GGL_I64;
    case at::kHalf: return GGL_F16;
    case at::kBFloat16: return GGL_BF16;
    case at::kFloat: return GGL_F32;
    case at::kDouble: return GGL_F64;
    default: TORCH_CHECK(false, "unsupported dtype ", t.scalar_type());
  }
}

static void same_device(std::initializer_list<const Tensor *> ts) {
  const Tensor *first = nullptr;
  for (const Tensor *t : ts) {
    if (t == nullptr || !t->defined()) continue;
    if (first == nullptr) first = t;
    TORCH_CHECK(t->device() == first->device(), "Tensor device inconsistent error.");   // segment_sum.cpp:31
  }
}

static int64_t env_int(const char *name, int64_t dflt) {
  const char *v = std::getenv(name);
  return v != nullptr ? std::strtoll(v, nullptr, 10) : dflt;
}

// ---------------------------------------------------------------------------------------------------------------
// Plans (struct ggl_segplan + the tensors that own its arrays)
// ---------------------------------------------------------------------------------------------------------------
static int64_t auto_chunk(const Api &a, int64_t E) { return a.ggl_policy_chunk(E); }   // (GGL_LONG_ROW is read there)

static Tensor row_order_of(const Tensor &counts);

static bool capturing(const c10::Device &d) {
  if (!d.is_cuda()) return false;
  c10::OptionalDeviceGuard guard(d);
  return c10::hip::currentStreamCaptureStatusMayInitCtx() != c10::hip::CaptureStatus::None;
}

struct SegPlan {
  int64_t N = 0, E = 0, chunk = 0, n_long = 0, n_chunks = 0, max_len = 0, xcd_run = 0;
  bool hub_first = false;   // the long rows lead the id range (a degree-sorted node order): ggl_segplan.xcd_run_rows = -1
  bool sorted = false;
  uint64_t uid = 0;
  Tensor rowptr, perm, long_rows, chunk_ptr, long_order;
  // the row hand-out order is a scheduling aid worth ~100 us of sorting: computed when the plan is launched a SECOND
  // time, so a plan used once (a fresh edge list per mini-batch) never pays for it (plans.py SegPlan.c_struct)
  mutable Tensor row_order;
  mutable std::mutex order_mu;
  mutable int uses = 0;

  // `unsplit`: every row walked in one piece; `skip_long`: rows longer than chunk left to ggl_segment_hub16
  ggl_segplan_t c(const Tensor &partial, bool unsplit = false, bool skip_long = false) const {
    ggl_segplan_t s{};
    const bool lng = n_long > 0 && !unsplit && !skip_long;
    s.rowptr = rowptr.data_ptr<int64_t>();
    s.perm = perm.defined() ? perm.data_ptr<int32_t>() : nullptr;
    s.long_rows = lng ? long_rows.data_ptr<int32_t>() : nullptr;
    s.chunk_ptr = lng ? chunk_ptr.data_ptr<int64_t>() : nullptr;
    s.n_long = lng ? n_long : 0;
    s.n_chunks = lng ? n_chunks : 0;
    s.chunk = unsplit ? (int64_t(1) << 62) : chunk;
    s.partial = partial.defined() ? partial.data_ptr() : nullptr;
    s.partial_bytes = partial.defined() ? partial.nbytes() : 0;
    s.N = N;
    s.E = E;
    if (N > 1) {
      std::lock_guard<std::mutex> g(order_mu);
      // (not while a hipGraph is being recorded: the sort would be allocated in the capture pool and filled on replay only)
      if (!row_order.defined() && ++uses >= 2 && !capturing(rowptr.device())) row_order = row_order_of(counts());
    }
    s.row_order = row_order.defined() ? row_order.data_ptr<int32_t>() : nullptr;
    s.xcd_run_rows = xcd_run > 0 ? xcd_run : ((lng && hub_first) ? -1 : 0);
    s.long_order = (lng && long_order.defined()) ? long_order.data_ptr<int32_t>() : nullptr;
    s.max_len = max_len;
    return s;
  }
  Tensor counts() const { return rowptr.slice(0, 1) - rowptr.slice(0, 0, N); }
};

static std::atomic<uint64_t> g_plans_built{0}, g_plan_hits{0};

// rows by descending length inside windows of consecutive ids, the heavy ones first (ops.py Engine._row_order)
static Tensor row_order_of(const Tensor &counts) {
  int64_t W = 2048, heavy = 1024;
  api_for(counts.device()).ggl_policy_row_order(&W, &heavy);
  const int64_t N = counts.size(0);
  if (W <= 0 || N <= W) return at::argsort(counts, /*stable=*/true, 0, /*descending=*/true).to(at::kInt);
  Tensor ar = at::arange(N, counts.options());
  Tensor group = at::where(counts >= heavy, at::zeros_like(ar), at::floor_divide(ar, W) + 1);
  Tensor key = at::bitwise_or(at::bitwise_left_shift(group, 32),
                              (int64_t(1) << 31) - counts.clamp_max((int64_t(1) << 31) - 1));
  return at::argsort(key, /*stable=*/true).to(at::kInt);
}

static void fill_long_rows(const Api &a, SegPlan &p, void *st) {
  if (p.max_len <= p.chunk) return;
  auto bytes = p.rowptr.options().dtype(at::kByte);
  const size_t lwb = a.ggl_plan_long_workspace_bytes(p.N);
  Tensor lws = at::empty({static_cast<int64_t>(lwb)}, bytes);
  int64_t nl = 0, nc = 0;
  check(a, a.ggl_plan_long_count(p.rowptr.data_ptr<int64_t>(), p.N, p.chunk, lws.data_ptr(), lwb, st, &nl, &nc));
  p.n_long = nl;
  p.n_chunks = nc;
  p.long_rows = at::empty({nl}, p.rowptr.options().dtype(at::kInt));
  p.chunk_ptr = at::empty({nl + 1}, p.rowptr.options());
  check(a, a.ggl_plan_long_fill(p.rowptr.data_ptr<int64_t>(), p.N, p.chunk, nl, p.long_rows.data_ptr<int32_t>(),
                                p.chunk_ptr.data_ptr<int64_t>(), lws.data_ptr(), lwb, st));
  if (nl >= 8)  // do the long rows lead the id range (degree-sorted order)?  one host read, at plan build only (ops.py)
    p.hub_first = p.long_rows.select(0, nl - 1).item<int32_t>() < 4 * nl;
  if (nl > 0)   // the serial hub walk starts its longest rows first (ggl_segplan.long_order; ops.py Engine._long_order)
    p.long_order = at::argsort(p.counts().index_select(0, p.long_rows.to(at::kLong)), /*stable=*/true, 0, /*descending=*/true).to(at::kInt);
}

static std::shared_ptr<SegPlan> build_plan(const Tensor &ids_in, int64_t N) {
  const auto dev = ids_in.device();
  const Api &a = api_for(dev);
  Tensor ids = ids_in.contiguous();
  void *st = stream_of(dev);
  auto p = std::make_shared<SegPlan>();
  p->N = N;
  p->E = ids.size(0);
  p->chunk = auto_chunk(a, p->E);
  auto i64 = ids.options().dtype(at::kLong);
  p->rowptr = at::empty({N + 1}, i64);
  Tensor perm = at::empty({std::max<int64_t>(p->E, 1)}, i64.dtype(at::kInt));
  const size_t wsb = a.ggl_plan_workspace_bytes(p->E, N);
  Tensor ws = at::empty({static_cast<int64_t>(wsb)}, i64.dtype(at::kByte));
  int32_t is_sorted = 0;
  int64_t max_len = 0;
  check(a, a.ggl_plan_build(ids.data_ptr<int64_t>(), p->E, N, perm.data_ptr<int32_t>(), p->rowptr.data_ptr<int64_t>(),
                            ws.data_ptr(), wsb, st, &is_sorted, &max_len));
  p->sorted = is_sorted != 0;
  p->max_len = max_len;
  if (!p->sorted) p->perm = perm.slice(0, 0, p->E);
  fill_long_rows(a, *p, st);
  p->uid = ++g_plans_built;
  return p;
}

// LRU keyed on the identity + version of a tensor; an entry dies with the tensor's storage (plans.py _PlanCache)
struct TensorKey {
  const void *storage = nullptr;
  int64_t offset = 0, numel = 0, version = 0, a = 0, b = 0;
  std::vector<int64_t> shape, stride;
  c10::Device dev = c10::Device(c10::kCPU);
  bool operator==(const TensorKey &o) const {
    return storage == o.storage && offset == o.offset && numel == o.numel && version == o.version && a == o.a &&
           b == o.b && dev == o.dev && shape == o.shape && stride == o.stride;
  }
  static TensorKey of(const Tensor &t, int64_t a, int64_t b) {
    TensorKey k;
    k.storage = t.storage().unsafeGetStorageImpl();
    k.offset = t.storage_offset();
    k.numel = t.numel();
    k.version = t.is_inference() ? 0 : static_cast<int64_t>(t._version());
    k.a = a;
    k.b = b;
    k.shape = t.sizes().vec();
    k.stride = t.strides().vec();
    k.dev = t.device();
    return k;
  }
};

template <typename V>
class Cache {
 public:
  explicit Cache(size_t cap) : cap_(cap) {}
  std::shared_ptr<V> get(const TensorKey &k) {
    std::lock_guard<std::mutex> g(mu_);
    for (auto it = items_.begin(); it != items_.end(); ++it) {
      if (!(it->key == k)) continue;
      if (it->ref.expired()) {   // the storage is gone and its address was recycled: not the same tensor
        items_.erase(it);
        return nullptr;
      }
      items_.splice(items_.begin(), items_, it);
      return items_.front().val;
    }
    return nullptr;
  }
  void put(const Tensor &t, const TensorKey &k, std::shared_ptr<V> v) {
    std::lock_guard<std::mutex> g(mu_);
    items_.remove_if([&](const Item &i) { return i.key == k || i.ref.expired(); });
    items_.push_front(Item{k, t.storage().getWeakStorageImpl(), std::move(v)});
    while (items_.size() > cap_) items_.pop_back();
  }
  void clear() {
    std::lock_guard<std::mutex> g(mu_);
    items_.clear();
  }

 private:
  struct Item {
    TensorKey key;
    c10::weak_intrusive_ptr<c10::StorageImpl> ref;
    std::shared_ptr<V> val;
  };
  size_t cap_;
  std::mutex mu_;
  std::list<Item> items_;
};

static Cache<SegPlan> &seg_cache() {
  static Cache<SegPlan> c(16);
  return c;
}

static std::shared_ptr<SegPlan> seg_plan(const Tensor &ids, int64_t N) {
  TensorKey k = TensorKey::of(ids, N, 0);
  if (auto hit = seg_cache().get(k)) {
    ++g_plan_hits;
    return hit;
  }
  auto p = build_plan(ids, N);
  seg_cache().put(ids, k, p);
  return p;
}

static Tensor gather_i32(const Api &a, const Tensor &src_i64, const Tensor &perm) {
  Tensor src = src_i64.contiguous();
  Tensor out = at::empty({src.size(0)}, src.options().dtype(at::kInt));
  check(a, a.ggl_gather_i64_to_i32(src.data_ptr<int64_t>(), perm.defined() ? perm.data_ptr<int32_t>() : nullptr,
                                   src.size(0), out.data_ptr<int32_t>(), stream_of(src.device())));
  return out;
}

struct SortedW {   // edge weights in a plan's sorted order, once they have been seen twice
  int sightings = 0;
  Tensor sorted;
};

struct GraphPlan {
  int64_t N_dst = 0, N_src = 0, E = 0;
  std::shared_ptr<SegPlan> fwd, bwd;
  Tensor col, colT, rowidx;
  std::mutex mu;
  Cache<SortedW> weights{8};

  // share of the (sampled) edges whose endpoints lie within N / 64 ids of each other (plans.py GraphPlan.locality)
  double locality() const {
    const int64_t N = std::max(N_dst, N_src);
    if (E == 0 || N_dst != N_src) return 0.0;
    const int64_t S = std::min<int64_t>(int64_t(1) << 16, E);
    Tensor pos = at::arange(S, fwd->rowptr.options()) * (E / S);
    Tensor rows = at::searchsorted(fwd->rowptr, pos, /*out_int32=*/false, /*right=*/true) - 1;
    Tensor near = (col.index_select(0, pos).to(at::kLong) - rows).abs() < std::max<int64_t>(N / 64, 4096);
    return near.to(at::kFloat).mean().item<double>();
  }
  void schedule() {   // XCD runs where the node order carries locality (plans.py GraphPlan._schedule)
    const Api &a = api_for(fwd->rowptr.device());
    const bool need = a.ggl_policy_xcd_run_rows(E, 1.0) > 0 || a.ggl_policy_xcd_run_rows(E, 0.0) > 0;
    const int64_t run = a.ggl_policy_xcd_run_rows(E, need ? locality() : 0.0);   // (locality() is one host read)
    fwd->xcd_run = run;
    if (bwd) bwd->xcd_run = run;
  }
  void need_bwd(const Tensor &index) {   // CSC side, built on the first backward
    std::lock_guard<std::mutex> g(mu);
    if (bwd) return;
    const Api &a = api_for(index.device());
    auto b = seg_plan(index.select(0, 0), N_src);
    colT = gather_i32(a, index.select(0, 1), b->perm);
    b->xcd_run = fwd->xcd_run;
    bwd = b;
  }
  void need_rowidx(const Tensor &index) {
    std::lock_guard<std::mutex> g(mu);
    if (rowidx.defined()) return;
    rowidx = gather_i32(api_for(index.device()), index.select(0, 1), fwd->perm);
  }
  // transposed sorted position -> forward sorted position (int32 [E]; plans.py GraphPlan.posT)
  Tensor posT;
  void need_posT(const Tensor &index) {
    need_bwd(index);
    std::lock_guard<std::mutex> g(mu);
    if (posT.defined()) return;
    auto i32 = fwd->rowptr.options().dtype(at::kInt);
    Tensor ar = at::arange(E, i32);
    Tensor pf = fwd->perm.defined() ? fwd->perm : ar, pt = bwd->perm.defined() ? bwd->perm : ar;
    Tensor inv = at::empty({E}, i32);
    inv.index_put_({pf.to(at::kLong)}, ar);
    posT = inv.index_select(0, pt.to(at::kLong)).contiguous();
  }
};

static Cache<GraphPlan> &graph_cache() {
  static Cache<GraphPlan> c(16);
  return c;
}

static void check_range(const Tensor &ids, int64_t n) {   // one host read per plan
  if (ids.numel() == 0) return;
  auto mm = at::aminmax(ids);
  Tensor both = at::stack({std::get<0>(mm), std::get<1>(mm)}).cpu();   // one host read
  TORCH_CHECK_INDEX(both[0].item<int64_t>() >= 0 && both[1].item<int64_t>() < n, "node id out of range [0, ", n, ")");
}

static std::shared_ptr<GraphPlan> graph_plan(const Tensor &index, int64_t n_dst, int64_t n_src) {
  TORCH_CHECK_INDEX(index.dim() == 2 && index.size(0) == 2, "edge index must have shape [2, E]");
  TORCH_CHECK(index.scalar_type() == at::kLong, "expected scalar type Long but found ", index.scalar_type());
  TensorKey k = TensorKey::of(index, n_dst, n_src);
  if (auto hit = graph_cache().get(k)) return hit;
  const Api &a = api_for(index.device());
  auto gp = std::make_shared<GraphPlan>();
  gp->N_dst = n_dst;
  gp->N_src = n_src;
  gp->E = index.size(1);
  gp->fwd = seg_plan(index.select(0, 1), n_dst);   // shared with segment ops on edge_index[1]
  check_range(index.select(0, 0), n_src);
  gp->col = gather_i32(a, index.select(0, 0), gp->fwd->perm);
  gp->schedule();
  graph_cache().put(index, k, gp);
  return gp;
}

// ---------------------------------------------------------------------------------------------------------------
// Forward launches
// ---------------------------------------------------------------------------------------------------------------
// the partial buffer of a plan's long rows: nbytes(n_chunks) bytes + 16 of slack on like's device, undefined for a plan without
// long rows.  It must outlive the launch that is handed it.
template <typename Bytes>
static Tensor hub_partial(const SegPlan &p, const Tensor &like, Bytes nbytes) {
  if (p.n_long == 0) return Tensor();
  return at::empty({static_cast<int64_t>(nbytes(p.n_chunks)) + 16}, like.options().dtype(at::kByte));
}
// One sizer per export: a call site names the walk it launches; the library owns the layout and checks plan->partial_bytes.
// ... of the segment reductions, gspmm / bspmm and their backward walks, partials of like's dtype
static Tensor partial_for(const Api &a, const SegPlan &p, const Tensor &like, int64_t K, bool with_arg) {
  return hub_partial(p, like, [&](int64_t n) { return a.ggl_partial_bytes(dtype_code(like), n, K, with_arg ? 1 : 0); });
}
// ... of the _x16 aggregates: f32 partials under 16-bit rows
static Tensor partial_f32_for(const Api &a, const SegPlan &p, const Tensor &like, int64_t K) {
  return hub_partial(p, like, [&](int64_t n) { return a.ggl_partial_bytes(GGL_F32, n, K, 0); });
}
// ... of the GAT forward walks: gat_fused, edge_softmax_aggregate and the ops that form their logits inside that walk
static Tensor gat_fwd_partial(const Api &a, const SegPlan &p, int64_t H, int64_t C, const Tensor &like) {
  return hub_partial(p, like, [&](int64_t n) { return a.ggl_gat_partial_bytes(n, H, C); });
}
// ... of their destination walks (fast: ggl_gat_fast_bwd's forward plan) and of the source walk
static Tensor gat_bwd_dst_partial(const Api &a, const SegPlan &p, int64_t H, bool fast, const Tensor &like) {
  return hub_partial(p, like, [&](int64_t n) {
    return fast ? a.ggl_gat_fast_bwd_dst_partial_bytes(n, H) : a.ggl_gat_bwd_dst_partial_bytes(n, H);
  });
}
static Tensor gat_bwd_src_partial(const Api &a, const SegPlan &p, int64_t H, int64_t C, const Tensor &like) {
  return hub_partial(p, like, [&](int64_t n) { return a.ggl_gat_bwd_src_partial_bytes(n, H, C); });
}

static std::vector<int64_t> out_shape(const Tensor &x, int64_t N) {
  auto s = x.sizes().vec();
  s[0] = N;
  return s;
}

enum class Red { Sum, Mean, Max };

static std::pair<Tensor, Tensor> segment_fwd(Red op, const Tensor &x, const SegPlan &p) {
  const auto dev = x.device();
  const Api &a = api_for(dev);
  const int64_t E = x.size(0);
  TORCH_CHECK_INDEX(E == p.E, "fisrt dimension of x and index should be same");   // segment_sum_cpu.cpp:17-19
  int64_t K = 1;
  for (int64_t d = 1; d < x.dim(); ++d) K *= x.size(d);
  Tensor out = at::empty(out_shape(x, p.N), x.options());
  void *st = stream_of(dev);
  const int code = dtype_code(x);
  const bool half = x.scalar_type() == at::kHalf || x.scalar_type() == at::kBFloat16;
  // f16 / bf16 sums accumulate in the storage type: chunk partials would not reproduce the serial result
  const bool unsplit = op != Red::Max && half;
  const bool hubs = unsplit && p.n_long > 0 && a.ggl_segment_hub16_supported(code, K, x.data_ptr(), out.data_ptr()) != 0;
  Tensor part = unsplit ? Tensor() : partial_for(a, p, x, K, op == Red::Max);
  ggl_segplan_t cs = p.c(part, unsplit && !hubs, hubs);
  if (op == Red::Max) {
    Tensor arg = at::empty(out_shape(x, p.N), x.options().dtype(at::kLong));
    check(a, a.ggl_segment_max(code, x.data_ptr(), &cs, K, out.data_ptr(), arg.data_ptr<int64_t>(), E, st));
    return {out, arg};
  }
  check(a, (op == Red::Sum ? a.ggl_segment_sum : a.ggl_segment_mean)(code, x.data_ptr(), &cs, K, out.data_ptr(), st));
  if (hubs) {
    ggl_segplan_t full = p.c(Tensor());
    check(a, a.ggl_segment_hub16(code, op == Red::Mean ? 1 : 0, x.data_ptr(), &full, K, out.data_ptr(), st));
  }
  return {out, Tensor()};
}

static std::pair<const float *, int> weights_for(const Api &a, GraphPlan &gp, const SegPlan &p, const Tensor &w,
                                                 Tensor &keep) {
  if (!w.defined()) return {nullptr, 0};
  if (!p.perm.defined()) return {w.data_ptr<float>(), 0};
  TensorKey k = TensorKey::of(w, static_cast<int64_t>(p.uid), 0);
  auto hit = gp.weights.get(k);
  if (!hit) {   // first sight: remember it, the kernel reads w[perm[p]] itself
    auto s = std::make_shared<SortedW>();
    s->sightings = 1;
    gp.weights.put(w, k, s);
    return {w.data_ptr<float>(), 0};
  }
  if (!hit->sorted.defined()) {
    const int64_t H = p.E > 0 ? std::max<int64_t>(w.numel() / p.E, 1) : 1;
    Tensor ws = at::empty_like(w);
    check(a, a.ggl_gather_rows_f32(w.data_ptr<float>(), p.perm.data_ptr<int32_t>(), p.E, H, ws.data_ptr<float>(),
                                   stream_of(w.device())));
    hit->sorted = ws;
  }
  keep = hit->sorted;
  return {keep.data_ptr<float>(), 1};
}

enum class SpOp { Sum, Mean, Max, MeanBwd, MaxBwd };

static bool is_x16(const Tensor &t) { return t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16; }

// sum / mean / mean backward on rows STORED as f16 / bf16 (ggl_spmm_*_x16): widened at the load, the f32 op's products and adds
// in its order, rounded once at the store — or not at all with out_f32.  Any width, nothing padded; f32 partials.
static Tensor spmm_fwd16(SpOp op, GraphPlan &gp, const SegPlan &p, const Tensor &col, const Tensor &w, const Tensor &x,
                         int64_t n_out, const Tensor &aux, bool out_f32) {
  const auto dev = x.device();
  const Api &a = api_for(dev);
  int64_t K = 1;
  for (int64_t d = 1; d < x.dim(); ++d) K *= x.size(d);
  Tensor out = at::empty(out_shape(x, n_out), out_f32 ? x.options().dtype(at::kFloat) : x.options());
  void *st = stream_of(dev);
  Tensor part = partial_f32_for(a, p, x, K);
  ggl_segplan_t cs = p.c(part);
  Tensor keep;
  auto [wp, by_pos] = weights_for(a, gp, p, w, keep);
  const int32_t *c = col.data_ptr<int32_t>();
  const int xc = dtype_code(x), oc = out_f32 ? GGL_F32 : xc;
  switch (op) {
    case SpOp::Sum: check(a, a.ggl_spmm_sum_x16(&cs, c, wp, by_pos, xc, x.data_ptr(), 0, K, oc, out.data_ptr(), 0, st)); break;
    case SpOp::Mean: check(a, a.ggl_spmm_mean_x16(&cs, c, wp, by_pos, xc, x.data_ptr(), 0, K, oc, out.data_ptr(), 0, st)); break;
    case SpOp::MeanBwd:
      check(a, a.ggl_spmm_mean_bwd_x16(&cs, c, wp, by_pos, xc, x.data_ptr(), aux.data_ptr<int64_t>(), K, oc, out.data_ptr(), st));
      break;
    default: TORCH_CHECK(false, "expected scalar type Float but found ", x.scalar_type(), " (gspmm max is f32 only)");
  }
  return out;
}

static std::pair<Tensor, Tensor> spmm_fwd(SpOp op, GraphPlan &gp, const SegPlan &p, const Tensor &col, const Tensor &w,
                                          const Tensor &x, int64_t n_out, const Tensor &aux = Tensor(),
                                          const Tensor &posT = Tensor(), bool out_f32 = false) {
  if (is_x16(x) && (op == SpOp::Sum || op == SpOp::Mean || op == SpOp::MeanBwd))
    return {spmm_fwd16(op, gp, p, col, w, x, n_out, aux, out_f32), Tensor()};
  const auto dev = x.device();
  const Api &a = api_for(dev);
  int64_t K = 1;
  for (int64_t d = 1; d < x.dim(); ++d) K *= x.size(d);
  if ((op == SpOp::Sum || op == SpOp::Mean || op == SpOp::Max) && x.dim() == 2) {
    // one zero-padded copy where the kernels want whole cache lines / 16-byte rows (ggl_policy_spmm_width; ops.py _spmm_fwd)
    const int64_t Kp = a.ggl_policy_spmm_width(op == SpOp::Max ? 1 : 0, K, p.E, x.size(0));
    if (Kp != K) {
      Tensor xp = at::constant_pad_nd(x, {0, Kp - K});
      auto r = spmm_fwd(op, gp, p, col, w, xp, n_out, aux);
      return {r.first.slice(1, 0, K).contiguous(), r.second.defined() ? r.second.slice(1, 0, K).contiguous() : Tensor()};
    }
  }
  Tensor out = at::empty(out_shape(x, n_out), x.options());
  void *st = stream_of(dev);
  Tensor part = partial_for(a, p, x, K, op == SpOp::Max);
  ggl_segplan_t cs = p.c(part);
  Tensor keep;
  auto [wp, by_pos] = weights_for(a, gp, p, w, keep);
  const int32_t *c = col.data_ptr<int32_t>();
  const float *xp = x.data_ptr<float>();
  float *op_ = out.data_ptr<float>();
  switch (op) {
    case SpOp::Sum: check(a, a.ggl_spmm_sum(&cs, c, wp, by_pos, xp, K, op_, st)); break;
    case SpOp::Mean: check(a, a.ggl_spmm_mean(&cs, c, wp, by_pos, xp, K, op_, st)); break;
    case SpOp::Max: {
      Tensor arg = at::empty(out.sizes(), out.options().dtype(at::kLong));
      check(a, a.ggl_spmm_max(&cs, c, wp, by_pos, xp, K, op_, arg.data_ptr<int64_t>(), st));
      return {out, arg};
    }
    case SpOp::MeanBwd:
      if (x.dim() == 2 && a.ggl_policy_mean_bwd_prescale(p.E, x.size(0))) {
        // the division depends on the destination row only: once per row, then the plain transposed SpMM-sum
        Tensor cnt = (aux.slice(0, 1) - aux.slice(0, 0, aux.size(0) - 1)).clamp_min(1).to(at::kFloat).unsqueeze(1);
        Tensor xs = x / cnt;
        check(a, a.ggl_spmm_sum(&cs, c, wp, by_pos, xs.data_ptr<float>(), K, op_, st));
      } else {
        check(a, a.ggl_spmm_mean_bwd(&cs, c, wp, by_pos, xp, aux.data_ptr<int64_t>(), K, op_, st));
      }
      break;
    case SpOp::MaxBwd: {
      // the form is the library's decision (ggl_policy_maxbwd_form: the winner mask only where its E x K/8-byte transient
      // pays); `posT` is defined iff the caller found the mask form chosen.  An allocation failure falls back to the int32 copy.
      Tensor mask;
      if (posT.defined()) {
        try {
          mask = at::empty({static_cast<int64_t>(a.ggl_spmm_max_mask_bytes(p.E, K) / 4) + 4}, x.options().dtype(at::kInt));
        } catch (const c10::Error &) {
          mask = Tensor();
        }
      }
      if (mask.defined()) {
        // a 1-bit winner mask built in destination order; records in forward order, read at posT[t] (ops.py _spmm_fwd)
        ggl_segplan_t fs = gp.fwd->c(Tensor());
        check(a, a.ggl_spmm_max_mask(&fs, gp.col.data_ptr<int32_t>(), aux.data_ptr<int64_t>(), K,
                                     reinterpret_cast<uint32_t *>(mask.data_ptr<int32_t>()), st));
        check(a, a.ggl_spmm_max_bwd_mask(&cs, c, wp, by_pos, xp, reinterpret_cast<const uint32_t *>(mask.data_ptr<int32_t>()),
                                         posT.data_ptr<int32_t>(), K, op_, st));
      } else if (posT.defined() || a.ggl_get_option("maxbwd_arg32") != 0) {   // witnesses from a compact int32 copy (one [N, K] pass)
        Tensor aux32 = aux.to(at::kInt);
        check(a, a.ggl_spmm_max_bwd32(&cs, c, wp, by_pos, xp, aux32.data_ptr<int32_t>(), K, op_, st));
      } else {
        check(a, a.ggl_spmm_max_bwd(&cs, c, wp, by_pos, xp, aux.data_ptr<int64_t>(), K, op_, st));
      }
      break;
    }
  }
  return {out, Tensor()};
}

static Tensor bspmm_fwd(GraphPlan &gp, const SegPlan &p, const Tensor &col, const Tensor &w, const Tensor &x,
                        int64_t n_out) {
  const Api &a = api_for(x.device());
  const int64_t H = x.size(1), C = x.size(2);
  Tensor out = at::empty({n_out, H, C}, x.options());
  Tensor part = partial_for(a, p, x, H * C, false);
  ggl_segplan_t cs = p.c(part);
  Tensor keep;
  auto [wp, by_pos] = weights_for(a, gp, p, w, keep);
  check(a, a.ggl_bspmm_sum(&cs, col.data_ptr<int32_t>(), wp, by_pos, x.data_ptr<float>(), H, C, out.data_ptr<float>(),
                           stream_of(x.device())));
  return out;
}

// ---------------------------------------------------------------------------------------------------------------
// Argument checks (the reference's predicates and exception types: segment_sum_cpu.cpp:13-19, spmm_sum_cpu.cpp:22)
// ---------------------------------------------------------------------------------------------------------------
static void seg_args(const Tensor &x, const Tensor &index) {
  same_device({&x, &index});
  TORCH_CHECK_INDEX(index.dim() == 1, "index dimension should be 1, but got ", index.dim());
  TORCH_CHECK_INDEX(x.dim() >= 1 && x.size(0) == index.size(0), "fisrt dimension of x and index should be same");
  TORCH_CHECK(index.scalar_type() == at::kLong, "expected scalar type Long but found ", index.scalar_type());
}

static void f32(const char *name, const Tensor &t) {
  TORCH_CHECK(t.scalar_type() == at::kFloat, "expected scalar type Float but found ", t.scalar_type(), " (", name, ")");
}

using OptT_ = c10::optional<Tensor>;
static Tensor opt(const c10::optional<Tensor> &t) { return t.has_value() ? *t : Tensor(); }
// the kernels read weight.data_ptr() as E dense floats (spmm_sum_cpu.cpp:48-50 makes it contiguous in backward too)
static Tensor opt_dense(const c10::optional<Tensor> &t) { return t.has_value() && t->defined() ? t->contiguous() : Tensor(); }

// ---------------------------------------------------------------------------------------------------------------
// Backend kernels (forward only; these are what the CUDA / CPU keys run, e.g. under no_grad)
// ---------------------------------------------------------------------------------------------------------------
static Tensor segment_sum_kernel(const Tensor &x, const Tensor &index, int64_t N) {
  seg_args(x, index);
  c10::OptionalDeviceGuard guard(x.device());
  return segment_fwd(Red::Sum, x.contiguous(), *seg_plan(index, N)).first;
}
static Tensor segment_mean_kernel(const Tensor &x, const Tensor &index, int64_t N) {
  seg_args(x, index);
  c10::OptionalDeviceGuard guard(x.device());
  return segment_fwd(Red::Mean, x.contiguous(), *seg_plan(index, N)).first;
}
static std::tuple<Tensor, Tensor> segment_max_kernel(const Tensor &x, const Tensor &index, int64_t N) {
  seg_args(x, index);
  c10::OptionalDeviceGuard guard(x.device());
  auto r = segment_fwd(Red::Max, x.contiguous(), *seg_plan(index, N));
  return {r.first, r.second};
}

// Edge softmax (utils/softmax.py:29-35) as one op each way: ggl_segment_softmax_fwd / _bwd over the id vector's cached plan.
// y and gx come back in the caller's element order; the backward needs y and grad only.
static Tensor softmax_partial(const Api &a, const SegPlan &p, const Tensor &like, int64_t K) {
  return hub_partial(p, like, [&](int64_t n) { return a.ggl_segment_softmax_partial_bytes(n, K); });
}
static int64_t softmax_width(const Api &a, const Tensor &x, const SegPlan &p) {
  TORCH_CHECK_INDEX(x.size(0) == p.E, "fisrt dimension of x and index should be same");
  f32("x", x);
  int64_t K = 1;
  for (int64_t d = 1; d < x.dim(); ++d) K *= x.size(d);
  TORCH_CHECK(a.ggl_segment_softmax_supported(K) != 0, "segment_softmax: no kernel for rows of ", K,
              " columns (ggl_segment_softmax_supported); gammagl_amd.utils.segment_softmax composes such rows from the segment ops");
  return K;
}
static Tensor segment_softmax_kernel(const Tensor &x_, const Tensor &index, int64_t N) {
  seg_args(x_, index);
  c10::OptionalDeviceGuard guard(x_.device());
  const Api &a = api_for(x_.device());
  Tensor x = x_.contiguous();
  auto plan = seg_plan(index, N);
  const int64_t K = softmax_width(a, x, *plan);
  Tensor y = at::empty_like(x);
  Tensor part = softmax_partial(a, *plan, x, K);
  ggl_segplan_t cs = plan->c(part);
  check(a, a.ggl_segment_softmax_fwd(x.data_ptr<float>(), &cs, K, y.data_ptr<float>(), stream_of(x.device())));
  return y;
}
static Tensor segment_softmax_backward_kernel(const Tensor &grad, const Tensor &y_, const Tensor &index, int64_t N) {
  same_device({&grad, &y_, &index});
  c10::OptionalDeviceGuard guard(y_.device());
  const Api &a = api_for(y_.device());
  Tensor y = y_.contiguous(), g = grad.contiguous();
  TORCH_CHECK(g.sizes() == y.sizes(), "segment_softmax backward: grad and y differ in shape");
  f32("grad", g);
  auto plan = seg_plan(index, N);    // (the forward's plan: a cache hit)
  const int64_t K = softmax_width(a, y, *plan);
  Tensor gx = at::empty_like(y);
  Tensor part = softmax_partial(a, *plan, y, K);
  ggl_segplan_t cs = plan->c(part);
  check(a, a.ggl_segment_softmax_bwd(y.data_ptr<float>(), g.data_ptr<float>(), &cs, K, gx.data_ptr<float>(),
                                     stream_of(y.device())));
  return gx;
}

struct SpArgs {
  std::shared_ptr<GraphPlan> gp;
  Tensor w, x;
};
// x16: the op also takes rows stored as f16 / bf16 (sum and mean: an extension over the reference, which is f32 only)
static SpArgs spmm_args(const Tensor &index, const c10::optional<Tensor> &weight, const Tensor &x, bool x16 = false) {
  Tensor w = opt(weight);
  same_device({&index, &w, &x});
  if (!(x16 && is_x16(x))) f32("x", x);
  if (w.defined()) f32("weight", w);
  TORCH_CHECK(x.dim() >= 1, "x must have a node dimension");
  SpArgs s;
  s.gp = graph_plan(index, x.size(0), x.size(0));   // gspmm.cpp:16 out = zeros_like(x): square
  if (w.defined()) TORCH_CHECK(w.numel() % std::max<int64_t>(s.gp->E, 1) == 0 && w.size(0) == s.gp->E,
                               "edge weight must hold one row per edge: got ", w.sizes(), " for ", s.gp->E, " edges");
  s.w = w.defined() ? w.contiguous() : w;
  s.x = x.contiguous();
  return s;
}

static Tensor spmm_kernel(SpOp op, const Tensor &index, const c10::optional<Tensor> &weight, const Tensor &x,
                          Tensor *arg = nullptr, bool out_f32 = false) {
  c10::OptionalDeviceGuard guard(x.device());
  SpArgs s = spmm_args(index, weight, x, op != SpOp::Max);
  TORCH_CHECK(!out_f32 || is_x16(s.x), "out_f32 is for f16 / bf16 rows (x is ", x.scalar_type(), ")");
  auto r = spmm_fwd(op, *s.gp, *s.gp->fwd, s.gp->col, s.w, s.x, s.gp->N_dst, Tensor(), Tensor(), out_f32);
  if (arg != nullptr) *arg = r.second;
  return r.first;
}
static Tensor spmm_sum_kernel(const Tensor &i, const c10::optional<Tensor> &w, const Tensor &x) {
  return spmm_kernel(SpOp::Sum, i, w, x);
}
static Tensor spmm_mean_kernel(const Tensor &i, const c10::optional<Tensor> &w, const Tensor &x) {
  return spmm_kernel(SpOp::Mean, i, w, x);
}
static Tensor spmm_max_kernel(const Tensor &i, const c10::optional<Tensor> &w, const Tensor &x) {
  return spmm_kernel(SpOp::Max, i, w, x);
}
// f16 / bf16 rows, the f32 sums as they are (out_f32) or rounded once to x's dtype (= spmm_sum / spmm_mean on such rows)
static Tensor spmm_sum_x16_kernel(const Tensor &i, const c10::optional<Tensor> &w, const Tensor &x, bool out_f32) {
  TORCH_CHECK(is_x16(x), "spmm_sum_x16 takes f16 / bf16 rows (x is ", x.scalar_type(), ")");
  return spmm_kernel(SpOp::Sum, i, w, x, nullptr, out_f32);
}
static Tensor spmm_mean_x16_kernel(const Tensor &i, const c10::optional<Tensor> &w, const Tensor &x, bool out_f32) {
  TORCH_CHECK(is_x16(x), "spmm_mean_x16 takes f16 / bf16 rows (x is ", x.scalar_type(), ")");
  return spmm_kernel(SpOp::Mean, i, w, x, nullptr, out_f32);
}

static int64_t head_pad(const GraphPlan &gp, const Tensor &x) {   // channels to append per head (ggl_policy_head_channels)
  return api_for(x.device()).ggl_policy_head_channels(x.size(2), gp.E, x.size(0)) - x.size(2);
}
static void bspmm_check(const Tensor &w, const Tensor &x) {
  TORCH_CHECK(x.dim() == 3, "bspmm expects x of shape [num_nodes, heads, channels]");
  TORCH_CHECK(w.defined() && w.dim() == 2 && w.size(1) == x.size(1), "bspmm expects weight of shape [num_edges, heads]");
}
static Tensor bspmm_sum_kernel(const Tensor &index, const Tensor &weight, const Tensor &x) {
  c10::OptionalDeviceGuard guard(x.device());
  TORCH_CHECK(x.dim() == 3, "bspmm expects x of shape [num_nodes, heads, channels]");
  SpArgs s = spmm_args(index, weight, x);
  bspmm_check(s.w, s.x);
  const int64_t C = s.x.size(2);
  const int64_t hp = head_pad(*s.gp, s.x);
  Tensor xin = hp > 0 ? at::constant_pad_nd(s.x, {0, hp}) : s.x;
  Tensor out = bspmm_fwd(*s.gp, *s.gp->fwd, s.gp->col, s.w, xin, s.gp->N_dst);
  return xin.size(2) == C ? out : out.slice(2, 0, C).contiguous();
}

// ---------------------------------------------------------------------------------------------------------------
// Backward passes as dispatcher ops of their own (backend + Meta kernels): the autograd formulas below only CALL ops,
// so a graph that contains them traces end to end under FakeTensor / torch.compile (AOTAutograd), forward and backward
// ---------------------------------------------------------------------------------------------------------------
static int64_t width_of(c10::IntArrayRef shape) {
  int64_t K = 1;
  for (size_t d = 1; d < shape.size(); ++d) K *= shape[d];
  return K;
}

// gin[e, :] = gout[ids[e], :]                                            (segment_sum.cpp:43-54)
static Tensor segment_sum_backward_kernel(const Tensor &grad, const Tensor &index, c10::IntArrayRef x_shape) {
  Tensor g = grad.contiguous();
  c10::OptionalDeviceGuard guard(g.device());
  const Api &a = api_for(g.device());
  Tensor gin = at::empty(x_shape, g.options());
  Tensor ids = index.contiguous();
  check(a, a.ggl_segment_sum_bwd(dtype_code(g), g.data_ptr(), ids.data_ptr<int64_t>(), x_shape[0], width_of(x_shape),
                                 gin.data_ptr(), stream_of(g.device())));
  return gin;
}
// gin[e, :] = gout[ids[e], :] / count[ids[e]]                             (segment_mean.cpp:44-63)
static Tensor segment_mean_backward_kernel(const Tensor &grad, const Tensor &index, int64_t N, c10::IntArrayRef x_shape) {
  Tensor g = grad.contiguous();
  TORCH_CHECK(g.is_floating_point(), "segment_mean backward needs a floating dtype");
  c10::OptionalDeviceGuard guard(g.device());
  const Api &a = api_for(g.device());
  Tensor gin = at::empty(x_shape, g.options());
  Tensor ids = index.contiguous();
  auto plan = seg_plan(index, N);    // (the forward's plan: a cache hit)
  check(a, a.ggl_segment_mean_bwd(dtype_code(g), g.data_ptr(), ids.data_ptr<int64_t>(), plan->rowptr.data_ptr<int64_t>(),
                                  x_shape[0], width_of(x_shape), gin.data_ptr(), stream_of(g.device())));
  return gin;
}
// gin = 0; gin[arg[s, k], k] = gout[s, k] where the segment is not empty   (segment_max.cpp:48-61)
static Tensor segment_max_backward_kernel(const Tensor &grad, const Tensor &arg, c10::IntArrayRef x_shape) {
  Tensor g = grad.contiguous();
  c10::OptionalDeviceGuard guard(g.device());
  const Api &a = api_for(g.device());
  Tensor gin = at::empty(x_shape, g.options());
  Tensor ar = arg.contiguous();
  check(a, a.ggl_segment_max_bwd(dtype_code(g), g.data_ptr(), ar.data_ptr<int64_t>(), x_shape[0], ar.size(0),
                                 width_of(x_shape), gin.data_ptr(), stream_of(g.device())));
  return gin;
}

static std::shared_ptr<GraphPlan> bwd_plan(const Tensor &index, int64_t n) {
  auto gp = graph_plan(index, n, n);
  gp->need_bwd(index);
  return gp;
}
// gx[src] += w[e] * g[dst]: the same walk on the transposed plan          (spmm_sum_cpu.cpp:43-80)
static Tensor spmm_sum_backward_kernel(const Tensor &index, const c10::optional<Tensor> &weight, const Tensor &grad) {
  Tensor g = grad.contiguous(), w = opt_dense(weight);
  if (!is_x16(g)) f32("grad", g);
  if (w.defined()) f32("weight", w);
  c10::OptionalDeviceGuard guard(g.device());
  auto gp = bwd_plan(index, g.size(0));
  return spmm_fwd(SpOp::Sum, *gp, *gp->bwd, gp->colT, w, g, gp->N_src).first;
}
static Tensor spmm_mean_backward_kernel(const Tensor &index, const c10::optional<Tensor> &weight, const Tensor &grad) {
  Tensor g = grad.contiguous(), w = opt_dense(weight);
  if (!is_x16(g)) f32("grad", g);
  if (w.defined()) f32("weight", w);
  c10::OptionalDeviceGuard guard(g.device());
  auto gp = bwd_plan(index, g.size(0));
  return spmm_fwd(SpOp::MeanBwd, *gp, *gp->bwd, gp->colT, w, g, gp->N_src, gp->fwd->rowptr).first;
}
static Tensor spmm_max_backward_kernel(const Tensor &index, const c10::optional<Tensor> &weight, const Tensor &grad,
                                       const Tensor &arg) {
  Tensor g = grad.contiguous(), w = opt_dense(weight);
  c10::OptionalDeviceGuard guard(g.device());
  auto gp = bwd_plan(index, g.size(0));
  Tensor posT;
  const int64_t Kw = g.dim() >= 2 ? g.numel() / std::max<int64_t>(g.size(0), 1) : 1;
  // (the inverse-permutation passes and the cached int32[E] only where the mask form is the one chosen for this K)
  if (api_for(g.device()).ggl_policy_maxbwd_form(gp->E, g.size(0), Kw) == 2) {
    gp->need_posT(index.contiguous());
    posT = gp->posT;
  }
  return spmm_fwd(SpOp::MaxBwd, *gp, *gp->bwd, gp->colT, w, g, gp->N_src, arg.contiguous(), posT).first;
}
static std::tuple<Tensor, Tensor> spmm_max_arg_kernel(const Tensor &i, const c10::optional<Tensor> &w, const Tensor &x) {
  Tensor arg;
  Tensor out = spmm_kernel(SpOp::Max, i, w, x, &arg);
  return {out, arg};
}
// gw[e] = sum_k x[src_e, k] * grad[dst_e, k] (mean: grad / the destination row's edge count first): gspmm's gradient with
// respect to its edge weights, f32 [E] whatever x and grad are stored as (ggl_spmm_grad_w; an extension, gspmm.cpp:79)
static Tensor spmm_grad_w_kernel(const Tensor &index, const Tensor &x_in, const Tensor &grad, bool mean) {
  same_device({&index, &x_in, &grad});
  Tensor x = x_in.contiguous(), g = grad.contiguous();
  if (!is_x16(x)) f32("x", x);
  if (!is_x16(g)) f32("grad", g);
  TORCH_CHECK(x.dim() >= 1 && g.dim() >= 1 && width_of(x.sizes()) == width_of(g.sizes()),
              "spmm_grad_w: x ", x.sizes(), " and grad ", g.sizes(), " differ in row width");
  c10::OptionalDeviceGuard guard(g.device());
  const Api &a = api_for(g.device());
  auto gp = graph_plan(index, g.size(0), x.size(0));
  const int64_t K = width_of(x.sizes());
  if (gp->E == 0 || K == 0) return at::zeros({gp->E}, g.options().dtype(at::kFloat));
  Tensor gw = at::empty({gp->E}, g.options().dtype(at::kFloat));   // every entry is written (through perm)
  gp->need_rowidx(index);
  const size_t sb = a.ggl_spmm_grad_w_scratch_bytes(gp->E, gp->N_dst, K, dtype_code(x), mean ? 1 : 0);
  Tensor scratch = sb > 0 ? at::empty({static_cast<int64_t>(sb / 4)}, gw.options()) : Tensor();
  ggl_segplan_t cs = gp->fwd->c(Tensor());
  check(a, a.ggl_spmm_grad_w(&cs, gp->col.data_ptr<int32_t>(), gp->rowidx.data_ptr<int32_t>(), dtype_code(x), x.data_ptr(),
                             dtype_code(g), g.data_ptr(), mean ? gp->fwd->rowptr.data_ptr<int64_t>() : nullptr, K,
                             gw.data_ptr<float>(), scratch.defined() ? scratch.data_ptr() : nullptr, stream_of(g.device())));
  return gw;
}
// (gw, gx): gx = the transposed walk; gw[e, h] = sum_c x[src, h, c] * g[dst, h, c]   (bspmm_sum_cpu.cpp:58-113)
static std::tuple<Tensor, Tensor> bspmm_sum_backward_kernel(const Tensor &index, const Tensor &weight, const Tensor &x_in,
                                                            const Tensor &grad) {
  c10::OptionalDeviceGuard guard(grad.device());
  const Api &a = api_for(grad.device());
  Tensor w = weight.contiguous();
  auto gp = bwd_plan(index, x_in.size(0));
  const int64_t C0 = x_in.size(2), H = x_in.size(1);
  const int64_t pad = head_pad(*gp, x_in);
  Tensor x = (pad > 0 ? at::constant_pad_nd(x_in, {0, pad}) : x_in).contiguous();
  Tensor g = (pad > 0 ? at::constant_pad_nd(grad, {0, pad}) : grad).contiguous();
  const int64_t C = C0 + pad;
  Tensor gx = bspmm_fwd(*gp, *gp->bwd, gp->colT, w, g, gp->N_src);
  Tensor gw = at::empty_like(w);
  void *st = stream_of(g.device());
  if (a.ggl_policy_gradw_sorted(H, C)) {   // along the destination-sorted plan, strips staged through LDS (edgedot.hip)
    gp->need_rowidx(index);
    const size_t sb = a.ggl_bspmm_grad_w_sorted_scratch_bytes(gp->E, gp->N_dst, H, C);
    Tensor scratch = sb > 0 ? at::empty({static_cast<int64_t>(sb / 4)}, g.options()) : Tensor();
    ggl_segplan_t cs = gp->fwd->c(Tensor());
    check(a, a.ggl_bspmm_grad_w_sorted(&cs, gp->col.data_ptr<int32_t>(), gp->rowidx.data_ptr<int32_t>(),
                                       x.data_ptr<float>(), g.data_ptr<float>(), H, C, gw.data_ptr<float>(),
                                       scratch.defined() ? scratch.data_ptr<float>() : nullptr, st));
  } else {
    Tensor idx = index.contiguous();
    check(a, a.ggl_bspmm_grad_w(idx.data_ptr<int64_t>(), x.data_ptr<float>(), g.data_ptr<float>(), gp->E, H, C,
                                gw.data_ptr<float>(), st));
  }
  if (pad > 0) gx = gx.slice(2, 0, C0).contiguous();
  return {gw, gx};
}

// ---------------------------------------------------------------------------------------------------------------
// The fused route: edge-softmax + aggregate, the layer epilogue in the aggregate's
// store, one static-shape sampler hop — registered like the seven operators above: forward and backward passes are
// dispatcher ops of their own, the autograd formulas only call ops.  (Until round 4 these existed as Python-registered
// ops only, gammagl_amd/torch_ops.py: 20-30 us of Python + ctypes per call.)
// ---------------------------------------------------------------------------------------------------------------
// device-resident {seed, offset} of the fused dropouts, seeded from torch's CPU generator on first use (follows
// torch.manual_seed, like ops.py Engine._rng_state); ggl::reseed() forgets it
static std::mutex g_rng_mu;
static std::vector<std::pair<c10::Device, Tensor>> g_rng;
static Tensor rng_state(const c10::Device &d) {
  std::lock_guard<std::mutex> g(g_rng_mu);
  for (auto &e : g_rng)
    if (e.first == d) return e.second;
  const int64_t seed = at::randint(0, int64_t(1) << 62, {1}, at::TensorOptions().dtype(at::kLong)).item<int64_t>();
  Tensor st = at::tensor({seed, int64_t(0)}, at::TensorOptions().dtype(at::kLong)).to(d);
  g_rng.emplace_back(d, st);
  return st;
}
static void reseed() {
  std::lock_guard<std::mutex> g(g_rng_mu);
  g_rng.clear();
}
// One fused-dropout draw: `rng` is the device state the launch reads and then advances by one, `used` a clone of the
// {seed, offset} it reads, which the op returns for its backward to redraw the mask.  At rate 0 nothing is drawn: rng is
// undefined and `used` the EMPTY tensor that stands for "no dropout" wherever an op returns or takes a rng_used.
struct Draw {
  Tensor rng, used;
  int64_t *ptr() const { return rng.defined() ? rng.data_ptr<int64_t>() : nullptr; }
};
static Draw draw(const c10::Device &dev, double p) {
  if (p > 0) {
    Tensor rng = rng_state(dev);
    return {rng, rng.clone()};
  }
  return {Tensor(), at::empty({0}, at::TensorOptions().dtype(at::kLong).device(dev))};
}
// the {seed, offset} a backward hands its kernel: the forward's `used`, or NULL without dropout
static const int64_t *used_ptr(double p, const Tensor &rng_used) {
  return (p > 0 && rng_used.numel() == 2) ? rng_used.data_ptr<int64_t>() : nullptr;
}

// x may be STORED as f16 / bf16 (an extension: ggl_gat_fused_*_x16, the general kernels with f32 softmax and sums); el / er are f32
static void gat_check(const Tensor &el, const Tensor &er, const Tensor &x) {
  same_device({&el, &er, &x});
  f32("el", el); f32("er", er);
  if (!is_x16(x)) f32("x", x);
  TORCH_CHECK(x.dim() == 3 && el.dim() == 2 && er.dim() == 2 && el.size(1) == x.size(1) && er.size(1) == x.size(1) &&
              el.size(0) == x.size(0), "gat_fused expects el [N_src, H], er [N_dst, H], x [N_src, H, C]");
}

// (out, rowmax, rowden, rng_used, fast): one launch (+ the hub-chunk combine inside the library)
static std::tuple<Tensor, Tensor, Tensor, Tensor, bool> gat_forward(GraphPlan &gp, const Tensor &el_, const Tensor &er_,
                                                                    const Tensor &x_, double slope, double p,
                                                                    bool out_f32 = false) {
  const auto dev = x_.device();
  const Api &a = api_for(dev);
  Tensor el = el_.contiguous(), er = er_.contiguous(), x = x_.contiguous();
  TORCH_CHECK(er.size(0) == gp.N_dst && x.size(0) == gp.N_src, "gat_fused: er has ", er.size(0), " rows for ", gp.N_dst,
              " destinations, x ", x.size(0), " for ", gp.N_src, " sources");
  const int64_t N = gp.N_dst, H = x.size(1), C = x.size(2);
  const bool x16 = is_x16(x);
  TORCH_CHECK(!out_f32 || x16, "out_f32 is for f16 / bf16 rows (x is ", x.scalar_type(), ")");
  Tensor out = at::empty({N, H, C}, out_f32 ? x.options().dtype(at::kFloat) : x.options());
  Tensor rmax = at::empty({N, H}, el.options()), rden = at::empty({N, H}, el.options());
  Tensor part = gat_fwd_partial(a, *gp.fwd, H, C, x);
  ggl_segplan_t cs = gp.fwd->c(part);
  const Draw d = draw(dev, p);
  static const bool want_fast = env_int("GGL_GAT_FAST", 1) != 0;
  const bool fast = !x16 && want_fast && a.ggl_gat_fast_supported(H, C) != 0;   // 16-bit rows: the general kernels
  void *st = stream_of(dev);
  int64_t *rp = d.ptr();
  if (x16)
    check(a, a.ggl_gat_fused_fwd_x16(&cs, gp.col.data_ptr<int32_t>(), el.data_ptr<float>(), er.data_ptr<float>(), dtype_code(x),
                                     x.data_ptr(), static_cast<float>(slope), H, C, static_cast<float>(p), rp, dtype_code(out),
                                     out.data_ptr(), rmax.data_ptr<float>(), rden.data_ptr<float>(), st));
  else if (fast)
    check(a, a.ggl_gat_fast_fwd(&cs, gp.col.data_ptr<int32_t>(), el.data_ptr<float>(), er.data_ptr<float>(),
                                x.data_ptr<float>(), x.size(0), static_cast<float>(slope), H, C, static_cast<float>(p), rp,
                                out.data_ptr<float>(), rmax.data_ptr<float>(), rden.data_ptr<float>(), st));
  else
    check(a, a.ggl_gat_fused_fwd(&cs, gp.col.data_ptr<int32_t>(), el.data_ptr<float>(), er.data_ptr<float>(),
                                 x.data_ptr<float>(), static_cast<float>(slope), H, C, static_cast<float>(p), rp,
                                 out.data_ptr<float>(), rmax.data_ptr<float>(), rden.data_ptr<float>(), st));
  return {out, rmax, rden, d.used, fast};
}

// (gel, ger, gx): the destination walk and the source walk
static std::tuple<Tensor, Tensor, Tensor> gat_backward(GraphPlan &gp, const Tensor &colT, const Tensor &posT,
                                                       const Tensor &el, const Tensor &er, const Tensor &x, const Tensor &g_,
                                                       const Tensor &out, const Tensor &rmax, const Tensor &rden,
                                                       const Tensor &rng_used, double slope, double p, bool fast) {
  const auto dev = x.device();
  const Api &a = api_for(dev);
  const bool x16 = is_x16(x);
  TORCH_CHECK(!(x16 && fast), "gat_fused_backward: f16 / bf16 rows take the general kernels (fast must be false)");
  // 16-bit rows: out is what the forward returned (x's dtype or f32) and the gradient is read in that dtype
  Tensor g = x16 && g_.scalar_type() != out.scalar_type() ? g_.to(out.scalar_type()).contiguous() : g_.contiguous();
  const int64_t H = x.size(1), C = x.size(2);
  void *st = stream_of(dev);
  const SegPlan &fw = *gp.fwd, &bw = *gp.bwd;
  Tensor ger = at::empty_like(er), gx = at::empty({gp.N_src, H, C}, x.options()), gel = at::empty({gp.N_src, H}, el.options());
  // (the fast destination walk keeps four DOUBLE sums per chunk and head: 8 H floats' worth per chunk, include/ggl_mpops.h;
  //  el is f32: the partials are, whatever x is stored as)
  Tensor part_f = gat_bwd_dst_partial(a, fw, H, fast, el), part_t = gat_bwd_src_partial(a, bw, H, C, el);
  ggl_segplan_t cs = fw.c(part_f), csT = bw.c(part_t);
  const int64_t *ru = used_ptr(p, rng_used);
  if (fast) {
    Tensor stats = at::empty({gp.N_dst, H, 4}, x.options());
    check(a, a.ggl_gat_fast_bwd(&cs, gp.col.data_ptr<int32_t>(), &csT, colT.data_ptr<int32_t>(),
                                p > 0 ? posT.data_ptr<int32_t>() : nullptr, el.data_ptr<float>(), er.data_ptr<float>(),
                                x.data_ptr<float>(), g.data_ptr<float>(), out.data_ptr<float>(), rmax.data_ptr<float>(),
                                rden.data_ptr<float>(), static_cast<float>(slope), H, C, static_cast<float>(p), ru,
                                stats.data_ptr<float>(), gx.data_ptr<float>(), gel.data_ptr<float>(), ger.data_ptr<float>(), st));
    return {gel, ger, gx};
  }
  // alpha and de interleaved [E, H, 2]: the source-side walk fetches both with one 64-byte line
  Tensor ad = at::empty({std::max<int64_t>(gp.E, 1), H, 2}, el.options());
  float *alpha = ad.data_ptr<float>(), *de = alpha + 1;
  if (x16) {
    TORCH_CHECK(out.scalar_type() == x.scalar_type() || out.scalar_type() == at::kFloat,
                "gat_fused_backward: out must have x's dtype or Float (got ", out.scalar_type(), " for ", x.scalar_type(), ")");
    Tensor oc = out.contiguous();
    const int xc = dtype_code(x), gc = dtype_code(g);
    check(a, a.ggl_gat_fused_bwd_dst_x16(&cs, gp.col.data_ptr<int32_t>(), el.data_ptr<float>(), er.data_ptr<float>(), xc,
                                         x.data_ptr(), gc, g.data_ptr(), gc, oc.data_ptr(), rmax.data_ptr<float>(),
                                         rden.data_ptr<float>(), static_cast<float>(slope), H, C, static_cast<float>(p), ru,
                                         alpha, de, ger.data_ptr<float>(), st));
    check(a, a.ggl_gat_fused_bwd_src_x16(&csT, colT.data_ptr<int32_t>(), posT.data_ptr<int32_t>(), alpha, de, gc, g.data_ptr(),
                                         H, C, xc, gx.data_ptr(), gel.data_ptr<float>(), st));
    return {gel, ger, gx};
  }
  check(a, a.ggl_gat_fused_bwd_dst(&cs, gp.col.data_ptr<int32_t>(), nullptr, el.data_ptr<float>(), er.data_ptr<float>(),
                                   x.data_ptr<float>(), g.data_ptr<float>(), out.data_ptr<float>(), rmax.data_ptr<float>(),
                                   rden.data_ptr<float>(), static_cast<float>(slope), H, C, static_cast<float>(p), ru, alpha,
                                   de, ger.data_ptr<float>(), nullptr, st));
  check(a, a.ggl_gat_fused_bwd_src(&csT, colT.data_ptr<int32_t>(), posT.data_ptr<int32_t>(), alpha, de, g.data_ptr<float>(),
                                   H, C, gx.data_ptr<float>(), gel.data_ptr<float>(), st));
  return {gel, ger, gx};
}

static std::shared_ptr<GraphPlan> gat_plan(const Tensor &index, int64_t n_dst, int64_t n_src) {
  TORCH_CHECK(index.scalar_type() == at::kLong, "expected scalar type Long but found ", index.scalar_type());
  return graph_plan(index.contiguous(), n_dst, n_src);
}

// out[i, h, :] = sum_{j -> i} dropout(softmax_i(LeakyReLU(el[j, h] + er[i, h]))) x[j, h, :]   (gat_conv.py:103-112)
static std::tuple<Tensor, Tensor, Tensor, Tensor, bool> gat_fused_forward_kernel(const Tensor &index, const Tensor &el,
                                                                                const Tensor &er, const Tensor &x,
                                                                                double slope, int64_t num_nodes, double p) {
  gat_check(el, er, x);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  c10::OptionalDeviceGuard guard(x.device());
  auto gp = gat_plan(index, num_nodes, x.size(0));
  return gat_forward(*gp, el, er, x, slope, p);
}
// gat_fused on f16 / bf16 rows with the choice of an f32 result (a last layer's logits); (out, rowmax, rowden, rng_used)
static std::tuple<Tensor, Tensor, Tensor, Tensor> gat_x16_forward_kernel(const Tensor &index, const Tensor &el, const Tensor &er,
                                                                         const Tensor &x, double slope, int64_t num_nodes,
                                                                         double p, bool out_f32) {
  gat_check(el, er, x);
  TORCH_CHECK(is_x16(x), "gat_fused_x16 takes f16 / bf16 rows (x is ", x.scalar_type(), ")");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  c10::OptionalDeviceGuard guard(x.device());
  auto gp = gat_plan(index, num_nodes, x.size(0));
  auto r = gat_forward(*gp, el, er, x, slope, p, out_f32);
  return {std::get<0>(r), std::get<1>(r), std::get<2>(r), std::get<3>(r)};
}
static std::tuple<Tensor, Tensor, Tensor> gat_fused_backward_kernel(const Tensor &index, const Tensor &el, const Tensor &er,
                                                                    const Tensor &x, const Tensor &grad, const Tensor &out,
                                                                    const Tensor &rmax, const Tensor &rden,
                                                                    const Tensor &rng_used, double slope, int64_t num_nodes,
                                                                    double p, bool fast) {
  c10::OptionalDeviceGuard guard(x.device());
  Tensor idx = index.contiguous();
  auto gp = gat_plan(idx, num_nodes, x.size(0));
  gp->need_bwd(idx);
  if (p > 0 || !fast) gp->need_posT(idx);
  return gat_backward(*gp, gp->colT, gp->posT, el.contiguous(), er.contiguous(), x.contiguous(), grad, out, rmax, rden,
                      rng_used, slope, p, fast);
}

// Edge softmax + aggregate on per-edge logits (ggl_edge_softmax_agg_*, include/ggl_mpops.h): the general GAT walks with the
// logit read from z [E, H] in the caller's edge order.  out[i, h, :] = sum_{e -> i} dropout(softmax_i(z[:, h]))[e] x[src_e, h, :]
static void esa_check(const Tensor &index, const Tensor &z, const Tensor &x) {
  same_device({&z, &x});
  f32("logits", z); f32("x", x);
  TORCH_CHECK(index.dim() == 2 && index.size(0) == 2, "edge_softmax_aggregate expects index [2, E]");
  TORCH_CHECK(x.dim() == 3 && z.dim() == 2 && z.size(1) == x.size(1) && z.size(0) == index.size(1),
              "edge_softmax_aggregate expects logits [E, H] and x [N_src, H, C] (got logits ", z.sizes(), ", x ", x.sizes(),
              " for ", index.size(1), " edges)");
}
// The two host cores under edge_softmax_aggregate, dot_attention and gatv2_attention (contiguous f32 tensors on v's device).
// A fused forward of the same walk, which forms its logits itself and stores them to z unless z is NULL:
using FusedFwd = std::function<int(const ggl_segplan_t *cs, int64_t *rng, float *out, float *rmax, float *rden, float *z, void *st)>;
// (out, rowmax, rowden, rng_used): the outputs, the hub partial and the rng draw, then ggl_edge_softmax_agg_fwd on the logits z —
// or `fused`, handed the same plan struct, draw and outputs, and z (which may be undefined) to write
static std::tuple<Tensor, Tensor, Tensor, Tensor> esa_forward(GraphPlan &gp, const Tensor &z, const Tensor &v, double p,
                                                              const FusedFwd &fused = nullptr) {
  const auto dev = v.device();
  const Api &a = api_for(dev);
  const int64_t N = gp.N_dst, H = v.size(1), C = v.size(2);
  Tensor out = at::empty({N, H, C}, v.options()), rmax = at::empty({N, H}, v.options()), rden = at::empty({N, H}, v.options());
  Tensor part = gat_fwd_partial(a, *gp.fwd, H, C, v);
  ggl_segplan_t cs = gp.fwd->c(part);
  const Draw d = draw(dev, p);
  float *zp = z.defined() ? z.data_ptr<float>() : nullptr;
  if (fused)
    check(a, fused(&cs, d.ptr(), out.data_ptr<float>(), rmax.data_ptr<float>(), rden.data_ptr<float>(), zp, stream_of(dev)));
  else
    check(a, a.ggl_edge_softmax_agg_fwd(&cs, gp.col.data_ptr<int32_t>(), zp, v.data_ptr<float>(), H, C, static_cast<float>(p),
                                        d.ptr(), out.data_ptr<float>(), rmax.data_ptr<float>(), rden.data_ptr<float>(),
                                        stream_of(dev)));
  return {out, rmax, rden, d.used};
}
// (gz, gv) on the logits z the forward used: the destination walk (alpha by sorted position, gz in the caller's edge order only
// with need_gz), then — only with need_gv — the source walk.  A gradient that is not needed is not computed and comes back
// UNDEFINED.
static std::pair<Tensor, Tensor> esa_backward(GraphPlan &gp, const Tensor &idx, const Tensor &z, const Tensor &v, const Tensor &grad,
                                              const Tensor &out, const Tensor &rmax, const Tensor &rden, const Tensor &rng_used,
                                              double p, bool need_gz, bool need_gv) {
  const auto dev = v.device();
  const Api &a = api_for(dev);
  Tensor g = grad.contiguous(), oc = out.contiguous();
  const int64_t H = v.size(1), C = v.size(2);
  void *st = stream_of(dev);
  Tensor alpha = need_gv ? at::empty({std::max<int64_t>(gp.E, 1), H}, v.options()) : Tensor();
  Tensor gz = need_gz ? at::empty_like(z) : Tensor(), gv;
  Tensor part_f = gat_bwd_dst_partial(a, *gp.fwd, H, false, z);
  ggl_segplan_t cs = gp.fwd->c(part_f);
  check(a, a.ggl_edge_softmax_agg_bwd_dst(&cs, gp.col.data_ptr<int32_t>(), z.data_ptr<float>(), v.data_ptr<float>(),
                                          g.data_ptr<float>(), oc.data_ptr<float>(), rmax.data_ptr<float>(),
                                          rden.data_ptr<float>(), H, C, static_cast<float>(p), used_ptr(p, rng_used),
                                          need_gv ? alpha.data_ptr<float>() : nullptr,
                                          need_gz ? gz.data_ptr<float>() : nullptr, st));
  if (need_gv) {
    gp.need_bwd(idx);
    gp.need_posT(idx);
    gv = at::empty({gp.N_src, H, C}, v.options());
    Tensor part_t = gat_bwd_src_partial(a, *gp.bwd, H, C, z);
    ggl_segplan_t csT = gp.bwd->c(part_t);
    check(a, a.ggl_edge_softmax_agg_bwd_src(&csT, gp.colT.data_ptr<int32_t>(), gp.posT.data_ptr<int32_t>(),
                                            alpha.data_ptr<float>(), g.data_ptr<float>(), H, C, gv.data_ptr<float>(), st));
  }
  return {gz, gv};
}
// what an op returns for a gradient nobody needs: EMPTY (a fresh tensor each: outputs of an op may not alias one another)
static Tensor or_empty(const Tensor &t, const Tensor &like) { return t.defined() ? t : at::empty({0}, like.options()); }
// (out, rowmax, rowden, rng_used, logits) of an op that forms its logits from its inputs (dot_attention, gatv2_attention):
// fused, its kernel `launch` forms them in the aggregate's walk and stores them only with keep_logits; otherwise compose(z)
// fills z [E, H] in front of ggl_edge_softmax_agg_fwd.  logits come back EMPTY without keep_logits.
template <typename Compose>
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> logit_attention_forward(GraphPlan &gp, const Tensor &v, double p,
                                                                                  bool keep_logits, bool fused, Compose compose,
                                                                                  const FusedFwd &launch) {
  Tensor z = (keep_logits || !fused) ? at::empty({gp.E, v.size(1)}, v.options()) : Tensor();
  if (!fused) compose(z);
  static const FusedFwd composed;   // empty: ggl_edge_softmax_agg_fwd on z
  auto r = esa_forward(gp, z, v, p, fused ? launch : composed);
  return {std::get<0>(r), std::get<1>(r), std::get<2>(r), std::get<3>(r), keep_logits ? z : at::empty({0}, v.options())};
}

// (out, rowmax, rowden, rng_used)
static std::tuple<Tensor, Tensor, Tensor, Tensor> esa_forward_kernel(const Tensor &index, const Tensor &z_, const Tensor &x_,
                                                                     int64_t num_nodes, double p) {
  esa_check(index, z_, x_);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  c10::OptionalDeviceGuard guard(x_.device());
  auto gp = gat_plan(index, num_nodes, x_.size(0));
  return esa_forward(*gp, z_.contiguous(), x_.contiguous(), p);
}
// (gz, gx); a gradient that is not needed is not computed and comes back EMPTY: need_x = false skips the source walk,
// need_z = false the gz stores
static std::tuple<Tensor, Tensor> esa_backward_kernel(const Tensor &index, const Tensor &z_, const Tensor &x_, const Tensor &grad,
                                                      const Tensor &out, const Tensor &rmax, const Tensor &rden,
                                                      const Tensor &rng_used, int64_t num_nodes, double p, bool need_z,
                                                      bool need_x) {
  c10::OptionalDeviceGuard guard(x_.device());
  Tensor idx = index.contiguous(), z = z_.contiguous(), x = x_.contiguous();
  auto gp = gat_plan(idx, num_nodes, x.size(0));
  std::pair<Tensor, Tensor> r;
  if (need_z || need_x) r = esa_backward(*gp, idx, z, x, grad, out, rmax, rden, rng_used, p, need_z, need_x);
  return {or_empty(r.first, z), or_empty(r.second, x)};
}

// Scaled dot-product graph attention (hgt_conv.py:115-153): z[e, h] = scale * <q[dst_e, h, :], k[src_e, h, :]>, then the op above on
// (z, v).  Fused route (ggl_dot_attn_fwd, GPU build, where ggl_dot_attn_supported and the policy say so): the dot is formed in
// the aggregate's walk and z is stored — by that walk, in the caller's edge order — only with keep_logits.  Composed route (any
// other shape, CPU tensors): z = scale * edge dot (chosen as bspmm_sum_backward_kernel chooses), then ggl_edge_softmax_agg_fwd.
static void dot_check(const Tensor &index, const Tensor &q, const Tensor &k, const Tensor &v) {
  same_device({&q, &k, &v});
  f32("q", q); f32("k", k); f32("v", v);
  TORCH_CHECK(index.dim() == 2 && index.size(0) == 2, "dot_attention expects index [2, E]");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3 && k.size(0) == v.size(0) && k.size(1) == q.size(1) &&
                  k.size(2) == q.size(2) && v.size(1) == q.size(1),
              "dot_attention expects q [N_dst, H, C] and k, v [N_src, H, C]: got q ", q.sizes(), ", k ", k.sizes(), ", v ", v.sizes());
  TORCH_CHECK(v.size(2) == q.size(2), "dot_attention needs v of k's head width (Cv == C): got C = ", q.size(2), ", Cv = ", v.size(2));
}
// out[e, h] = <x[src_e, h, :], g[dst_e, h, :]> in the caller's edge order
static void edge_dot(const Api &a, GraphPlan &gp, const Tensor &index, const Tensor &x, const Tensor &g, Tensor &out) {
  const int64_t H = x.size(1), C = x.size(2);
  void *st = stream_of(g.device());
  if (a.ggl_policy_gradw_sorted(H, C)) {
    gp.need_rowidx(index);
    const size_t sb = a.ggl_bspmm_grad_w_sorted_scratch_bytes(gp.E, gp.N_dst, H, C);
    Tensor scratch = sb > 0 ? at::empty({static_cast<int64_t>(sb / 4)}, g.options()) : Tensor();
    ggl_segplan_t cs = gp.fwd->c(Tensor());
    check(a, a.ggl_bspmm_grad_w_sorted(&cs, gp.col.data_ptr<int32_t>(), gp.rowidx.data_ptr<int32_t>(), x.data_ptr<float>(),
                                       g.data_ptr<float>(), H, C, out.data_ptr<float>(),
                                       scratch.defined() ? scratch.data_ptr<float>() : nullptr, st));
  } else {
    check(a, a.ggl_bspmm_grad_w(index.data_ptr<int64_t>(), x.data_ptr<float>(), g.data_ptr<float>(), gp.E, H, C,
                                out.data_ptr<float>(), st));
  }
}
// bspmm_sum with the weights read through the plan's perm in the kernel (w_by_pos = 0): one-launch weights stay out of the
// sorted-weight cache
static Tensor bspmm_by_perm(const SegPlan &p, const Tensor &col, const Tensor &w, const Tensor &x, int64_t n_out) {
  const Api &a = api_for(x.device());
  const int64_t H = x.size(1), C = x.size(2);
  Tensor out = at::empty({n_out, H, C}, x.options());
  Tensor part = partial_for(a, p, x, H * C, false);
  ggl_segplan_t cs = p.c(part);
  check(a, a.ggl_bspmm_sum(&cs, col.data_ptr<int32_t>(), w.data_ptr<float>(), 0, x.data_ptr<float>(), H, C,
                           out.data_ptr<float>(), stream_of(x.device())));
  return out;
}
// (out, rowmax, rowden, rng_used, logits); logits [E, H] in the caller's edge order, or EMPTY when they were not formed
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> dot_forward_kernel(const Tensor &index, const Tensor &q_, const Tensor &k_,
                                                                             const Tensor &v_, int64_t num_nodes, double scale,
                                                                             double p, bool keep_logits) {
  dot_check(index, q_, k_, v_);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  const auto dev = v_.device();
  c10::OptionalDeviceGuard guard(dev);
  Tensor idx = index.contiguous();
  auto gp = gat_plan(idx, num_nodes, k_.size(0));
  TORCH_CHECK(gp->N_dst == q_.size(0), "dot_attention: the graph has ", gp->N_dst, " destinations, q has ", q_.size(0), " rows");
  const Api &a = api_for(dev);
  Tensor q = q_.contiguous(), k = k_.contiguous(), v = v_.contiguous();
  const int64_t H = v.size(1), C = v.size(2);
  const bool fused = dev.is_cuda() && a.ggl_dot_attn_supported(H, C) && a.ggl_policy_dot_attn_fused(H, C, gp->E, gp->N_src);
  return logit_attention_forward(
      *gp, v, p, keep_logits, fused,
      [&](Tensor &z) {
        edge_dot(a, *gp, idx, k, q, z);
        z.mul_(static_cast<float>(scale));   // one rounded f32 multiply per element
      },
      [&](const ggl_segplan_t *cs, int64_t *rng, float *out, float *rmax, float *rden, float *z, void *st) {
        return a.ggl_dot_attn_fwd(cs, gp->col.data_ptr<int32_t>(), q.data_ptr<float>(), k.data_ptr<float>(), v.data_ptr<float>(),
                                  static_cast<float>(scale), H, C, static_cast<float>(p), rng, out, rmax, rden, z, st);
      });
}
// (gq, gk, gv) from the saved logits: the edge-softmax aggregate's two backward walks, gs = gz * scale, gq = bspmm_sum(plan, gs, k),
// gk = bspmm_sum(planT, gs, q).  A gradient that is not needed is not computed and comes back EMPTY.
static std::tuple<Tensor, Tensor, Tensor> dot_backward_kernel(const Tensor &index, const Tensor &q_, const Tensor &k_, const Tensor &v_,
                                                              const Tensor &z_, const Tensor &grad, const Tensor &out,
                                                              const Tensor &rmax, const Tensor &rden, const Tensor &rng_used,
                                                              int64_t num_nodes, double scale, double p, bool need_q, bool need_k,
                                                              bool need_v) {
  c10::OptionalDeviceGuard guard(v_.device());
  Tensor idx = index.contiguous(), q = q_.contiguous(), k = k_.contiguous(), v = v_.contiguous(), z = z_.contiguous();
  auto gp = gat_plan(idx, num_nodes, k.size(0));
  Tensor gq, gk, gs, gv;
  if (need_q || need_k || need_v) {
    TORCH_CHECK(z.dim() == 2 && z.size(0) == gp->E && z.size(1) == v.size(1),
                "dot_attention_backward needs the forward's logits [E, H]");
    std::tie(gs, gv) = esa_backward(*gp, idx, z, v, grad, out, rmax, rden, rng_used, p, need_q || need_k, need_v);
    if (gs.defined()) gs.mul_(static_cast<float>(scale));
    if (need_q) gq = bspmm_by_perm(*gp->fwd, gp->col, gs, k, gp->N_dst);
    if (need_k) {
      gp->need_bwd(idx);
      gk = bspmm_by_perm(*gp->bwd, gp->colT, gs, q, gp->N_src);
    }
  }
  return {or_empty(gq, v), or_empty(gk, v), or_empty(gv, v)};
}

// GATv2's additive graph attention: z[e, h] = sum_c att[h, c] * LeakyReLU(xl[src_e, h, c] + xr[dst_e, h, c]), then
// edge_softmax_aggregate on (z, xl).  Fused route (ggl_gatv2_fwd, GPU build, where ggl_gatv2_supported and the policy say so):
// the logit is formed in the aggregate's walk from the value row and z is stored — by that walk, in the caller's edge order —
// only with keep_logits.  Composed route (any other shape, CPU tensors): z by torch in edge blocks of at most 256 MiB of
// [E_block, H, C], then ggl_edge_softmax_agg_fwd.
static void gatv2_check(const Tensor &index, const Tensor &xl, const Tensor &xr, const Tensor &att) {
  same_device({&xl, &xr, &att});
  f32("xl", xl); f32("xr", xr); f32("att", att);
  TORCH_CHECK(index.dim() == 2 && index.size(0) == 2, "gatv2_attention expects index [2, E]");
  TORCH_CHECK(xl.dim() == 3 && xr.dim() == 3 && xl.size(1) == xr.size(1) && xl.size(2) == xr.size(2),
              "gatv2_attention expects xl [N_src, H, C] and xr [N_dst, H, C]: got xl ", xl.sizes(), ", xr ", xr.sizes());
  TORCH_CHECK(att.dim() == 2 && att.size(0) == xl.size(1) && att.size(1) == xl.size(2), "gatv2_attention expects att [H, C] = [",
              xl.size(1), ", ", xl.size(2), "]: got ", att.sizes());
}
static void gatv2_logits(const Tensor &index, const Tensor &xl, const Tensor &xr, const Tensor &att, double slope, Tensor &z) {
  at::NoGradGuard no_grad;
  const int64_t E = index.size(1), H = xl.size(1), C = xl.size(2);
  const int64_t block = std::max<int64_t>(1, (int64_t(256) << 20) / (4 * H * C));
  Tensor src = index.select(0, 0), dst = index.select(0, 1);
  for (int64_t b = 0; b < E; b += block) {
    const int64_t n = std::min(block, E - b);
    Tensor s = xl.index_select(0, src.narrow(0, b, n)) + xr.index_select(0, dst.narrow(0, b, n));
    z.narrow(0, b, n).copy_((att * at::leaky_relu(s, slope)).sum(-1));
  }
}
// (g_self, att_rows) of ggl_gatv2_logit_bwd over plan p; gz is read through p's perm in the kernel
static std::pair<Tensor, Tensor> gatv2_logit_bwd(const SegPlan &p, const Tensor &col, const Tensor &other, const Tensor &self,
                                                 const Tensor &gz, const Tensor &att, double slope, const Tensor &add,
                                                 bool want_rows) {
  const Api &a = api_for(self.device());
  const int64_t H = self.size(1), C = self.size(2);
  Tensor g_self = at::empty_like(self), rows = want_rows ? at::empty_like(self) : Tensor();
  Tensor part = hub_partial(p, self, [&](int64_t n) { return a.ggl_gatv2_logit_bwd_partial_bytes(n, H, C, want_rows ? 1 : 0); });
  ggl_segplan_t cs = p.c(part);
  check(a, a.ggl_gatv2_logit_bwd(&cs, col.data_ptr<int32_t>(), other.data_ptr<float>(), self.data_ptr<float>(),
                                 gz.data_ptr<float>(), att.data_ptr<float>(), static_cast<float>(slope), H, C,
                                 add.defined() ? add.data_ptr<float>() : nullptr, g_self.data_ptr<float>(),
                                 want_rows ? rows.data_ptr<float>() : nullptr, stream_of(self.device())));
  return {g_self, rows};
}
// (out, rowmax, rowden, rng_used, logits); logits [E, H] in the caller's edge order, or EMPTY when they were not formed
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> gatv2_forward_kernel(const Tensor &index, const Tensor &xl_, const Tensor &xr_,
                                                                               const Tensor &att_, int64_t num_nodes, double slope,
                                                                               double p, bool keep_logits) {
  gatv2_check(index, xl_, xr_, att_);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  const auto dev = xl_.device();
  c10::OptionalDeviceGuard guard(dev);
  Tensor idx = index.contiguous();
  auto gp = gat_plan(idx, num_nodes, xl_.size(0));
  TORCH_CHECK(gp->N_dst == xr_.size(0), "gatv2_attention: the graph has ", gp->N_dst, " destinations, xr has ", xr_.size(0), " rows");
  const Api &a = api_for(dev);
  Tensor xl = xl_.contiguous(), xr = xr_.contiguous(), att = att_.contiguous();
  const int64_t H = xl.size(1), C = xl.size(2);
  const bool fused = dev.is_cuda() && a.ggl_gatv2_supported(H, C) && a.ggl_policy_gatv2_fused(H, C, gp->E, gp->N_src);
  return logit_attention_forward(
      *gp, xl, p, keep_logits, fused, [&](Tensor &z) { gatv2_logits(idx, xl, xr, att, slope, z); },
      [&](const ggl_segplan_t *cs, int64_t *rng, float *out, float *rmax, float *rden, float *z, void *st) {
        return a.ggl_gatv2_fwd(cs, gp->col.data_ptr<int32_t>(), xl.data_ptr<float>(), xr.data_ptr<float>(), att.data_ptr<float>(),
                               static_cast<float>(slope), H, C, static_cast<float>(p), rng, out, rmax, rden, z, st);
      });
}
// (g_xl, g_xr, g_att) from the saved logits: the edge-softmax aggregate's two backward walks (alpha, gz, gv), then
// ggl_gatv2_logit_bwd on the plan (g_xr, R; g_att = ggl_colsum_f32(R)) and on its transpose with add = gv (g_xl).  A gradient
// that is not needed is not computed and comes back EMPTY.
static std::tuple<Tensor, Tensor, Tensor> gatv2_backward_kernel(const Tensor &index, const Tensor &xl_, const Tensor &xr_,
                                                                const Tensor &att_, const Tensor &z_, const Tensor &grad,
                                                                const Tensor &out, const Tensor &rmax, const Tensor &rden,
                                                                const Tensor &rng_used, int64_t num_nodes, double slope, double p,
                                                                bool need_l, bool need_r, bool need_a) {
  const auto dev = xl_.device();
  c10::OptionalDeviceGuard guard(dev);
  const Api &a = api_for(dev);
  Tensor idx = index.contiguous(), xl = xl_.contiguous(), xr = xr_.contiguous(), att = att_.contiguous(), z = z_.contiguous();
  auto gp = gat_plan(idx, num_nodes, xl.size(0));
  const int64_t H = xl.size(1), C = xl.size(2);
  Tensor gl, gr, ga;
  if (need_l || need_r || need_a) {
    TORCH_CHECK(z.dim() == 2 && z.size(0) == gp->E && z.size(1) == H,
                "gatv2_attention_backward needs the forward's logits [E, H]");
    Tensor gz, gv;
    std::tie(gz, gv) = esa_backward(*gp, idx, z, xl, grad, out, rmax, rden, rng_used, p, true, need_l);
    if (need_r || need_a) {
      auto r = gatv2_logit_bwd(*gp->fwd, gp->col, xl, xr, gz, att, slope, Tensor(), need_a);
      if (need_r) gr = r.first;
      if (need_a) {
        ga = at::empty({H, C}, xl.options());
        const size_t wsb = a.ggl_colsum_workspace_bytes(gp->N_dst, H * C);
        Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(wsb, 4))}, xl.options().dtype(at::kByte));
        check(a, a.ggl_colsum_f32(r.second.data_ptr<float>(), gp->N_dst, H * C, ga.data_ptr<float>(), ws.data_ptr(), wsb,
                                  stream_of(dev)));
      }
    }
    if (need_l) gl = gatv2_logit_bwd(*gp->bwd, gp->colT, xr, xl, gz, att, slope, gv, false).first;
  }
  return {or_empty(gl, xl), or_empty(gr, xl), or_empty(ga, xl)};
}

// The same op over a CSR the caller already holds — the argument list of dgNN's GATConvFuse
// (layers/conv/fusedgat_conv.py:121): rows of the CSR aggregate, no sort.  The plan is cached on row_ptr.
struct CsrExtra {   // what besides row_ptr identifies the five-tensor structure
  const void *p[4];
  int64_t v[4];
  bool operator==(const CsrExtra &o) const { return std::memcmp(this, &o, sizeof(CsrExtra)) == 0; }
};
static Cache<GraphPlan> &csr_cache() {
  static Cache<GraphPlan> c(8);
  return c;
}
static std::mutex g_csr_mu;
static std::list<std::pair<std::weak_ptr<GraphPlan>, CsrExtra>> g_csr_extra;

static Tensor own_i32(const Tensor &t) { return t.scalar_type() == at::kInt ? t.clone().contiguous() : t.to(at::kInt).contiguous(); }
static std::shared_ptr<SegPlan> plan_from_rowptr(const Tensor &rowptr, int64_t E) {
  const Api &a = api_for(rowptr.device());
  auto p = std::make_shared<SegPlan>();
  p->N = rowptr.size(0) - 1;
  p->E = E;
  p->chunk = auto_chunk(a, E);
  p->rowptr = rowptr.to(at::kLong).contiguous();
  if (p->rowptr.data_ptr() == rowptr.data_ptr()) p->rowptr = p->rowptr.clone();   // the plan keeps its OWN copy
  p->sorted = true;
  p->max_len = p->N > 0 ? p->counts().max().item<int64_t>() : 0;
  fill_long_rows(a, *p, stream_of(rowptr.device()));
  p->uid = ++g_plans_built;
  return p;
}
static std::shared_ptr<GraphPlan> csr_plan(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &col_ptr,
                                           const Tensor &row_ind, const Tensor &permute) {
  same_device({&row_ptr, &col_ind, &col_ptr, &row_ind, &permute});
  const int64_t n_rows = row_ptr.size(0) - 1, n_cols = col_ptr.size(0) - 1, E = col_ind.size(0);
  for (const Tensor *t : {&row_ptr, &col_ind, &col_ptr, &row_ind, &permute})
    TORCH_CHECK(t->dim() == 1 && (t->scalar_type() == at::kInt || t->scalar_type() == at::kLong),
                "GATConvFuse: the CSR / CSC tensors must be 1-D int32 / int64");
  TORCH_CHECK(row_ind.size(0) == E && permute.size(0) == E, "GATConvFuse: col_ind, row_ind and permute must have one entry per edge");
  TensorKey k = TensorKey::of(row_ptr, n_rows, n_cols);
  CsrExtra ex{};
  const Tensor *others[4] = {&col_ind, &col_ptr, &row_ind, &permute};
  for (int i = 0; i < 4; ++i) {
    ex.p[i] = others[i]->data_ptr();
    ex.v[i] = static_cast<int64_t>(others[i]->_version());
  }
  if (auto hit = csr_cache().get(k)) {
    std::lock_guard<std::mutex> g(g_csr_mu);
    for (auto &e : g_csr_extra)
      if (e.first.lock() == hit && e.second == ex) return hit;
  }
  check_range(col_ind, n_cols);
  check_range(row_ind, n_rows);
  check_range(permute, std::max<int64_t>(E, 1));
  for (const Tensor *ptr : {&row_ptr, &col_ptr}) {   // one-off (per plan) host reads
    Tensor p64 = ptr->to(at::kLong);
    TORCH_CHECK(p64[0].item<int64_t>() == 0 && p64[-1].item<int64_t>() == E &&
                    (p64.size(0) < 2 || !(p64.slice(0, 1) < p64.slice(0, 0, p64.size(0) - 1)).any().item<bool>()),
                "GATConvFuse: a row pointer must rise from 0 to the number of edges (", E, ")");
  }
  auto gp = std::make_shared<GraphPlan>();
  gp->N_dst = n_rows;
  gp->N_src = n_cols;
  gp->E = E;
  gp->fwd = plan_from_rowptr(row_ptr, E);
  gp->col = own_i32(col_ind);
  gp->bwd = plan_from_rowptr(col_ptr, E);
  gp->colT = own_i32(row_ind);
  gp->posT = own_i32(permute);
  gp->schedule();
  csr_cache().put(row_ptr, k, gp);
  {
    std::lock_guard<std::mutex> g(g_csr_mu);
    g_csr_extra.remove_if([](const std::pair<std::weak_ptr<GraphPlan>, CsrExtra> &e) { return e.first.expired(); });
    g_csr_extra.emplace_back(gp, ex);
  }
  return gp;
}
static std::tuple<Tensor, Tensor, Tensor, Tensor, bool> gat_csr_forward_kernel(const Tensor &row_ptr, const Tensor &col_ind,
                                                                              const Tensor &col_ptr, const Tensor &row_ind,
                                                                              const Tensor &permute, const Tensor &el,
                                                                              const Tensor &er, const Tensor &x, double slope,
                                                                              double p) {
  gat_check(el, er, x);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  c10::OptionalDeviceGuard guard(x.device());
  auto gp = csr_plan(row_ptr, col_ind, col_ptr, row_ind, permute);
  return gat_forward(*gp, el, er, x, slope, p);
}
static std::tuple<Tensor, Tensor, Tensor> gat_csr_backward_kernel(const Tensor &row_ptr, const Tensor &col_ind,
                                                                  const Tensor &col_ptr, const Tensor &row_ind,
                                                                  const Tensor &permute, const Tensor &el, const Tensor &er,
                                                                  const Tensor &x, const Tensor &grad, const Tensor &out,
                                                                  const Tensor &rmax, const Tensor &rden,
                                                                  const Tensor &rng_used, double slope, double p, bool fast) {
  c10::OptionalDeviceGuard guard(x.device());
  auto gp = csr_plan(row_ptr, col_ind, col_ptr, row_ind, permute);
  return gat_backward(*gp, gp->colT, gp->posT, el.contiguous(), er.contiguous(), x.contiguous(), grad, out, rmax, rden,
                      rng_used, slope, p, fast);
}

// y = dropout(relu(a + bias))                                                      (gcn_conv.py:105-106, models/gcn.py:55-59)
// a may be STORED as f16 / bf16 (ggl_bias_act_*_x16: the f32 operations and words, y rounded once); bias and gbias stay f32
static std::tuple<Tensor, Tensor> bias_act_forward_kernel(const Tensor &a_, const OptT_ &bias, bool relu, double p) {
  Tensor a = a_.contiguous(), b = opt(bias);
  same_device({&a, &b});
  if (!is_x16(a)) f32("a", a);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "p_drop must be in [0, 1)");
  c10::OptionalDeviceGuard guard(a.device());
  const Api &api = api_for(a.device());
  const int64_t N = a.dim() > 0 ? a.size(0) : 1, K = N > 0 ? a.numel() / N : width_of(a.sizes());
  if (b.defined()) {
    f32("bias", b);
    b = b.contiguous().reshape({-1});
    TORCH_CHECK(b.numel() == K, "bias must hold one value per column");
  }
  Tensor y = at::empty_like(a);
  const Draw d = draw(a.device(), p);
  if (is_x16(a))
    check(api, api.ggl_bias_act_fwd_x16(dtype_code(a), a.data_ptr(), b.defined() ? b.data_ptr<float>() : nullptr, N, K,
                                        relu ? 1 : 0, static_cast<float>(p), d.ptr(), y.data_ptr(), stream_of(a.device())));
  else
    check(api, api.ggl_bias_act_fwd(a.data_ptr<float>(), b.defined() ? b.data_ptr<float>() : nullptr, N, K, relu ? 1 : 0,
                                    static_cast<float>(p), d.ptr(), y.data_ptr<float>(), stream_of(a.device())));
  return {y, d.used};
}
// (ga, gbias): the mask is rebuilt from y, the bias gradient reduced in the same pass (epilogue.hip)
static std::tuple<Tensor, Tensor> bias_act_backward_kernel(const Tensor &g_, const Tensor &y, bool has_bias, bool relu, double p,
                                                           const Tensor &rng_used) {
  Tensor g = g_.contiguous();
  c10::OptionalDeviceGuard guard(g.device());
  const Api &api = api_for(g.device());
  const int64_t N = g.dim() > 0 ? g.size(0) : 1, K = N > 0 ? g.numel() / N : width_of(g.sizes());
  if (!relu && p <= 0 && !has_bias) return {g, Tensor()};
  if (!is_x16(g)) f32("grad", g);
  TORCH_CHECK(g.scalar_type() == y.scalar_type(), "expected scalar type Float: the gradient (", g.scalar_type(),
              ") must have the output's dtype (", y.scalar_type(), ")");
  const auto f32o = g.options().dtype(at::kFloat);
  Tensor ga = at::empty_like(g), gb = has_bias ? at::empty({K}, f32o) : Tensor();
  const size_t wsb = api.ggl_bias_act_bwd_workspace_bytes(N, K);
  Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(wsb, 4))}, g.options().dtype(at::kByte));
  Tensor yc = y.contiguous();
  if (is_x16(g))
    check(api, api.ggl_bias_act_bwd_x16(dtype_code(g), g.data_ptr(), yc.data_ptr(), N, K, relu ? 1 : 0, static_cast<float>(p),
                                        used_ptr(p, rng_used), ga.data_ptr(), gb.defined() ? gb.data_ptr<float>() : nullptr,
                                        ws.data_ptr(), wsb, stream_of(g.device())));
  else
    check(api, api.ggl_bias_act_bwd(g.data_ptr<float>(), yc.data_ptr<float>(), N, K, relu ? 1 : 0, static_cast<float>(p),
                                    used_ptr(p, rng_used), ga.data_ptr<float>(), gb.defined() ? gb.data_ptr<float>() : nullptr,
                                    ws.data_ptr(), wsb, stream_of(g.device())));
  return {ga, gb.defined() ? gb : at::empty({0}, f32o)};
}

// bias_act_backward on a gradient that is the narrow product grad[:, :J] @ weight (weight [J, K]: the Linear that reads y),
// without that [N, K] product in memory (ggl_linear_bias_act_bwd: serial fmas in ascending j, then bias_act_backward's bits)
static std::tuple<Tensor, Tensor> linear_bias_act_backward_kernel(const Tensor &g_, const Tensor &w_, const Tensor &y, bool has_bias,
                                                                  bool relu, double p, const Tensor &rng_used) {
  Tensor g = g_.contiguous(), w = w_.contiguous(), yc = y.contiguous();
  same_device({&g, &w, &yc});
  f32("grad", g);
  f32("weight", w);
  f32("y", yc);
  TORCH_CHECK(g.dim() == 2 && w.dim() == 2 && yc.dim() == 2 && g.size(1) >= w.size(0) && yc.size(0) == g.size(0) &&
                  yc.size(1) == w.size(1),
              "linear_bias_act_backward: grad ", g.sizes(), ", weight ", w.sizes(), ", y ", yc.sizes(), " do not fit");
  c10::OptionalDeviceGuard guard(g.device());
  const Api &api = api_for(g.device());
  const int64_t N = g.size(0), J = w.size(0), K = w.size(1);
  const auto f32o = g.options().dtype(at::kFloat);
  Tensor ga = at::empty_like(yc), gb = has_bias ? at::empty({K}, f32o) : Tensor();
  const size_t wsb = api.ggl_bias_act_bwd_workspace_bytes(N, K);
  Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(wsb, 4))}, g.options().dtype(at::kByte));
  check(api, api.ggl_linear_bias_act_bwd(g.data_ptr<float>(), g.size(1), w.data_ptr<float>(), yc.data_ptr<float>(), N, J, K,
                                         relu ? 1 : 0, static_cast<float>(p), used_ptr(p, rng_used), ga.data_ptr<float>(),
                                         gb.defined() ? gb.data_ptr<float>() : nullptr, ws.data_ptr(), wsb, stream_of(g.device())));
  return {ga, gb.defined() ? gb : at::empty({0}, f32o)};
}

// y = dropout(relu(reduce_{j -> i} w x_j + add_i + bias)) in ONE kernel (reduce.hip MODE_SPMM_EPI): 2-D x, K % 4 == 0.
// x (and add) may be STORED as f16 / bf16: ggl_spmm_epi_x16, any width, the f32 operations, y rounded once to x's dtype.
static std::tuple<Tensor, Tensor> spmm_epi_forward_kernel(const Tensor &index, const OptT_ &weight, const Tensor &x, bool mean,
                                                          const OptT_ &add_, const OptT_ &bias_, bool relu, double p) {
  c10::OptionalDeviceGuard guard(x.device());
  SpArgs s = spmm_args(index, weight, x, true);
  Tensor add = opt(add_), bias = opt(bias_);
  same_device({&x, &add, &bias});
  const bool x16 = is_x16(s.x);
  TORCH_CHECK(s.x.dim() == 2 && (x16 || s.x.size(1) % 4 == 0), "spmm_epi_forward needs a 2-D x whose width is a multiple of 4");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "p_drop must be in [0, 1)");
  const Api &a = api_for(x.device());
  const int64_t K = s.x.size(1);
  if (add.defined()) {
    if (x16) {
      TORCH_CHECK(add.scalar_type() == s.x.scalar_type(), "expected scalar type Float (add in x's dtype, ", s.x.scalar_type(),
                  ") but found ", add.scalar_type(), " (add)");
    } else {
      f32("add", add);
    }
    TORCH_CHECK(add.dim() == 2 && add.size(0) == s.gp->N_dst && add.size(1) == K, "add must be [destination rows, feature width]");
    add = add.contiguous();
  }
  if (bias.defined()) {
    f32("bias", bias);
    bias = bias.contiguous().reshape({-1});
    TORCH_CHECK(bias.numel() == K, "bias must hold one value per column");
  }
  const SegPlan &p_ = *s.gp->fwd;
  Tensor y = at::empty({s.gp->N_dst, K}, s.x.options());
  Tensor part = x16 ? partial_f32_for(a, p_, s.x, K) : partial_for(a, p_, s.x, K, false);
  ggl_segplan_t cs = p_.c(part);
  Tensor keep;
  auto [wp, by_pos] = weights_for(a, *s.gp, p_, s.w, keep);
  const Draw d = draw(x.device(), p);
  if (x16) {
    const int xc = dtype_code(s.x);
    check(a, a.ggl_spmm_epi_x16(&cs, s.gp->col.data_ptr<int32_t>(), wp, by_pos, xc, s.x.data_ptr(), K, K, xc, y.data_ptr(), K,
                                mean ? 1 : 0, add.defined() ? add.data_ptr() : nullptr, add.defined() ? K : 0,
                                bias.defined() ? bias.data_ptr<float>() : nullptr, relu ? 1 : 0, static_cast<float>(p), d.ptr(),
                                0, 0, 1, stream_of(x.device())));
    return {y, d.used};
  }
  check(a, a.ggl_spmm_epi_ex(&cs, s.gp->col.data_ptr<int32_t>(), wp, by_pos, s.x.data_ptr<float>(), K, K, y.data_ptr<float>(),
                             K, 0, mean ? 1 : 0, add.defined() ? add.data_ptr<float>() : nullptr, add.defined() ? K : 0,
                             bias.defined() ? bias.data_ptr<float>() : nullptr, relu ? 1 : 0, static_cast<float>(p),
                             d.ptr(), 0, 0, 1, stream_of(x.device())));
  return {y, d.used};
}

// ---- spmm_rows: (A x + bias)[rows] on the restricted plan pair (include/ggl_mpops.h ggl_plan_rows_*; ops.py Engine.rows_plan) ----
struct RowsPlan {
  int64_t R = 0, N_dst = 0, N_src = 0;
  Tensor rows, col, colT, w_fwd, w_bwd;
  std::shared_ptr<SegPlan> fwd, bwd;
  bool has_w = false;
  // the weights the pair was built from: storage, offset and version each compared on a hit; an entry whose weights
  // died is a miss (address reuse)
  const void *w_storage = nullptr;
  int64_t w_offset = 0, w_version = 0;
  c10::optional<c10::weak_intrusive_ptr<c10::StorageImpl>> w_ref;
};

static Cache<RowsPlan> &rows_cache() {
  static Cache<RowsPlan> c(8);
  return c;
}

// a plan over elements already grouped by row (ops.py Engine.plan_from_rowptr): one host read for the longest row
// `chunk`: the long-row threshold of the plan the rows were cut from, so the same rows are long in both
static std::shared_ptr<SegPlan> plan_from_rowptr(const Api &a, const Tensor &rowptr, int64_t E, int64_t chunk, void *st) {
  auto p = std::make_shared<SegPlan>();
  p->N = rowptr.size(0) - 1;
  p->E = E;
  p->chunk = chunk;
  p->rowptr = rowptr;
  p->sorted = true;
  p->max_len = p->N > 0 ? p->counts().max().item<int64_t>() : 0;
  fill_long_rows(a, *p, st);
  p->uid = ++g_plans_built;
  return p;
}

static std::shared_ptr<RowsPlan> rows_plan(GraphPlan &gp, const Tensor &index, const Tensor &w, const Tensor &rows_in) {
  TORCH_CHECK(rows_in.dim() == 1 && rows_in.scalar_type() == at::kLong, "rows must be a 1-D int64 tensor, got ", rows_in.sizes(),
              " ", rows_in.scalar_type());
  const void *w_storage = w.defined() ? w.storage().unsafeGetStorageImpl() : nullptr;
  const int64_t w_offset = w.defined() ? w.storage_offset() : 0;
  const int64_t w_version = (w.defined() && !w.is_inference()) ? static_cast<int64_t>(w._version()) : 0;
  TensorKey k = TensorKey::of(rows_in, static_cast<int64_t>(gp.fwd->uid),
                              static_cast<int64_t>(reinterpret_cast<uintptr_t>(w_storage)));
  if (auto hit = rows_cache().get(k)) {
    if (hit->has_w == w.defined() && hit->w_storage == w_storage && hit->w_offset == w_offset && hit->w_version == w_version &&
        (!hit->has_w || !hit->w_ref->expired())) {
      ++g_plan_hits;
      return hit;
    }
  }
  const auto dev = rows_in.device();
  TORCH_CHECK(!capturing(dev), "spmm_rows: the restricted plan of this row list must be built before a hipGraph capture "
                               "(run one eager step first)");
  const Api &a = api_for(dev);
  void *st = stream_of(dev);
  gp.need_bwd(index);
  Tensor rows = rows_in.contiguous();
  const int64_t R = rows.size(0), N = gp.N_dst, E = gp.E;
  auto i64 = rows.options(), i32 = rows.options().dtype(at::kInt), f32o = rows.options().dtype(at::kFloat);
  const size_t wsb = a.ggl_plan_rows_workspace_bytes(E, std::max(gp.N_dst, gp.N_src), R);
  Tensor ws = at::empty({static_cast<int64_t>(wsb)}, rows.options().dtype(at::kByte));
  Tensor rank = at::empty({std::max<int64_t>(N, 1)}, i32);
  check(a, a.ggl_plan_rows_rank(rows.data_ptr<int64_t>(), R, N, rank.data_ptr<int32_t>(), ws.data_ptr(), wsb, st));
  auto rp = std::make_shared<RowsPlan>();
  rp->R = R;
  rp->N_dst = gp.N_dst;
  rp->N_src = gp.N_src;
  rp->rows = rows;
  rp->has_w = w.defined();
  rp->w_storage = w_storage;
  rp->w_offset = w_offset;
  rp->w_version = w_version;
  if (w.defined()) rp->w_ref = w.storage().getWeakStorageImpl();
  const float *wp = w.defined() ? w.data_ptr<float>() : nullptr;
  auto i32p = [](const Tensor &t) { return t.defined() ? t.data_ptr<int32_t>() : nullptr; };
  auto f32p = [](const Tensor &t) { return t.defined() ? t.data_ptr<float>() : nullptr; };
  // forward: a segmented copy of the listed rows' slices
  Tensor rowptr_r = at::empty({R + 1}, i64);
  int64_t E_r = 0, E_t = 0;
  check(a, a.ggl_plan_rows_fwd_rowptr(gp.fwd->rowptr.data_ptr<int64_t>(), rows.data_ptr<int64_t>(), R,
                                      rowptr_r.data_ptr<int64_t>(), ws.data_ptr(), wsb, st, &E_r));
  rp->col = at::empty({E_r}, i32);
  if (w.defined()) rp->w_fwd = at::empty({E_r}, f32o);
  check(a, a.ggl_plan_rows_fwd_fill(gp.fwd->rowptr.data_ptr<int64_t>(), gp.col.data_ptr<int32_t>(), wp, i32p(gp.fwd->perm),
                                    rows.data_ptr<int64_t>(), R, rowptr_r.data_ptr<int64_t>(), E_r, rp->col.data_ptr<int32_t>(),
                                    f32p(rp->w_fwd), st));
  rp->fwd = plan_from_rowptr(a, rowptr_r, E_r, gp.fwd->chunk, st);
  // transposed: the full transposed plan filtered to the listed destinations (flag, scan, compact)
  Tensor pos = at::empty({E + 1}, i32), rowptrT_r = at::empty({gp.N_src + 1}, i64);
  check(a, a.ggl_plan_rows_bwd_rowptr(gp.bwd->rowptr.data_ptr<int64_t>(), gp.colT.data_ptr<int32_t>(), gp.N_src, E,
                                      rank.data_ptr<int32_t>(), pos.data_ptr<int32_t>(), rowptrT_r.data_ptr<int64_t>(),
                                      ws.data_ptr(), wsb, st, &E_t));
  TORCH_CHECK(E_t == E_r, "restricted plans disagree: ", E_r, " forward elements, ", E_t, " transposed");
  rp->colT = at::empty({E_r}, i32);
  if (w.defined()) rp->w_bwd = at::empty({E_r}, f32o);
  check(a, a.ggl_plan_rows_bwd_fill(gp.colT.data_ptr<int32_t>(), wp, i32p(gp.bwd->perm), E, rank.data_ptr<int32_t>(),
                                    pos.data_ptr<int32_t>(), rp->colT.data_ptr<int32_t>(), f32p(rp->w_bwd), st));
  rp->bwd = plan_from_rowptr(a, rowptrT_r, E_r, gp.bwd->chunk, st);
  rows_cache().put(rows_in, k, rp);
  return rp;
}

static Tensor spmm_rows_forward_kernel(const Tensor &index, const OptT_ &weight, const Tensor &x, const Tensor &rows,
                                       const OptT_ &bias_) {
  c10::OptionalDeviceGuard guard(x.device());
  SpArgs s = spmm_args(index, weight, x);
  Tensor bias = opt(bias_);
  same_device({&x, &rows, &bias});
  TORCH_CHECK(s.x.dim() == 2 && s.x.size(1) > 0 && s.x.size(1) % 4 == 0,
              "spmm_rows needs a 2-D f32 x whose width is a multiple of 4, got ", x.sizes());
  const Api &a = api_for(x.device());
  const int64_t K = s.x.size(1);
  if (bias.defined()) {
    f32("bias", bias);
    bias = bias.contiguous().reshape({-1});
    TORCH_CHECK(bias.numel() == K, "bias must hold one value per column");
  }
  auto rp = rows_plan(*s.gp, index, s.w, rows);
  const SegPlan &p_ = *rp->fwd;
  Tensor y = at::empty({rp->R, K}, s.x.options());
  Tensor part = partial_for(a, p_, s.x, K, false);
  ggl_segplan_t cs = p_.c(part);
  check(a, a.ggl_spmm_epi_ex(&cs, rp->col.data_ptr<int32_t>(), rp->has_w ? rp->w_fwd.data_ptr<float>() : nullptr, 1,
                             s.x.data_ptr<float>(), K, K, y.data_ptr<float>(), K, 0, 0, nullptr, 0,
                             bias.defined() ? bias.data_ptr<float>() : nullptr, 0, 0.0f, nullptr, 0, 0, 1, stream_of(x.device())));
  return y;
}

// (gx [N_src, K], gbias [K] or empty): the transposed restricted walk over the compact gradient; ggl_bias_grad_rows
static std::tuple<Tensor, Tensor> spmm_rows_backward_kernel(const Tensor &index, const OptT_ &weight, const Tensor &grad,
                                                            const Tensor &rows, int64_t n_src, bool has_bias) {
  Tensor g = grad.contiguous(), w = opt_dense(weight);
  f32("grad", g);
  if (w.defined()) f32("weight", w);
  c10::OptionalDeviceGuard guard(g.device());
  const Api &a = api_for(g.device());
  auto gp = bwd_plan(index, n_src);
  auto rp = rows_plan(*gp, index, w, rows);
  TORCH_CHECK(g.dim() == 2 && g.size(0) == rp->R && g.size(1) % 4 == 0, "grad must be [len(rows), K], K a multiple of 4");
  const int64_t K = g.size(1);
  void *st = stream_of(g.device());
  Tensor gb = at::empty({has_bias ? K : 0}, g.options());
  if (has_bias) {
    const size_t wsb = a.ggl_bias_act_bwd_workspace_bytes(rp->N_dst, K);
    Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(wsb, 4))}, g.options().dtype(at::kByte));
    check(a, a.ggl_bias_grad_rows(g.data_ptr<float>(), rp->rows.data_ptr<int64_t>(), rp->R, rp->N_dst, K, gb.data_ptr<float>(),
                                  ws.data_ptr(), wsb, st));
  }
  const SegPlan &p_ = *rp->bwd;
  Tensor gx = at::empty({rp->N_src, K}, g.options());
  Tensor part = partial_for(a, p_, g, K, false);
  ggl_segplan_t cs = p_.c(part);
  check(a, a.ggl_spmm_sum(&cs, rp->colT.data_ptr<int32_t>(), rp->has_w ? rp->w_bwd.data_ptr<float>() : nullptr, 1,
                          g.data_ptr<float>(), K, gx.data_ptr<float>(), st));
  return {gx, gb};
}

// relu(segment_{sum,mean}(x, ids, N) + add + bias) for f32 messages [E, K] in one kernel (sage_conv.py:100-108)
static Tensor segment_epi_forward_kernel(const Tensor &x_, const Tensor &index, int64_t N, bool mean, const OptT_ &add_,
                                         const OptT_ &bias_, bool relu) {
  seg_args(x_, index);
  Tensor x = x_.contiguous(), add = opt(add_), bias = opt(bias_);
  same_device({&x, &add, &bias});
  f32("msg", x);
  TORCH_CHECK(x.dim() == 2, "segment_epi expects [E, K] messages");
  c10::OptionalDeviceGuard guard(x.device());
  const Api &a = api_for(x.device());
  auto plan = seg_plan(index, N);
  const int64_t K = x.size(1);
  if (add.defined()) {
    f32("add", add);
    TORCH_CHECK(add.dim() == 2 && add.size(0) == N && add.size(1) == K, "add must be [num_segments, feature width]");
    add = add.contiguous();
  }
  if (bias.defined()) {
    f32("bias", bias);
    bias = bias.contiguous().reshape({-1});
    TORCH_CHECK(bias.numel() == K, "bias must hold one value per column");
  }
  Tensor y = at::empty({N, K}, x.options());
  Tensor part = partial_for(a, *plan, x, K, false);
  ggl_segplan_t cs = plan->c(part);
  check(a, a.ggl_segment_epi(x.data_ptr<float>(), &cs, K, mean ? 1 : 0, add.defined() ? add.data_ptr<float>() : nullptr, 0,
                             bias.defined() ? bias.data_ptr<float>() : nullptr, relu ? 1 : 0, 0.0f, nullptr,
                             y.data_ptr<float>(), stream_of(x.device())));
  return y;
}

// One sampled hop with fixed capacities and device-side sizes (sample.hip ggl_sample_hop; ops/sparse/cpu/sample.cpp:10-135):
// nothing is read back, so a mini-batch step captures into one hipGraph.  Returns (rowptr [B_cap + 1], col [E_cap] int32
// local ids, e_id [E_cap], n_id [S_cap], counts [3] = {nodes, edges, overflow}); first_pos is the caller's relabel scratch
// (one int64 per graph node, all 2^62 on entry and on exit).
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> sample_hop_kernel(const Tensor &rowptr, const Tensor &col,
                                                                            const Tensor &seeds, const Tensor &n_seeds,
                                                                            int64_t num_nodes, int64_t fanout, int64_t e_cap,
                                                                            int64_t s_cap, Tensor &first_pos) {
  same_device({&rowptr, &col, &seeds, &n_seeds, &first_pos});
  const Tensor *all5[5] = {&rowptr, &col, &seeds, &n_seeds, &first_pos};
  for (const Tensor *t : all5)
    TORCH_CHECK(t->scalar_type() == at::kLong && t->is_contiguous(), "sample_hop takes contiguous int64 tensors");
  TORCH_CHECK(fanout > 0 && first_pos.numel() >= num_nodes && rowptr.numel() == num_nodes + 1, "bad sample_hop arguments");
  c10::OptionalDeviceGuard guard(rowptr.device());
  const Api &a = api_for(rowptr.device());
  const int64_t b_cap = seeds.size(0);
  auto i64 = rowptr.options();
  Tensor out_rowptr = at::empty({b_cap + 1}, i64), out_col = at::empty({std::max<int64_t>(e_cap, 1)}, i64.dtype(at::kInt));
  Tensor out_eid = at::empty({std::max<int64_t>(e_cap, 1)}, i64), out_nid = at::empty({s_cap}, i64), counts = at::empty({3}, i64);
  const size_t wsb = a.ggl_sample_hop_workspace_bytes(b_cap, e_cap);
  Tensor ws = at::empty({static_cast<int64_t>(wsb)}, i64.dtype(at::kByte));
  Tensor rng = rng_state(rowptr.device());
  check(a, a.ggl_sample_hop(rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), seeds.data_ptr<int64_t>(),
                            n_seeds.data_ptr<int64_t>(), b_cap, num_nodes, fanout, e_cap, s_cap, rng.data_ptr<int64_t>(),
                            first_pos.data_ptr<int64_t>(), out_rowptr.data_ptr<int64_t>(), out_col.data_ptr<int32_t>(),
                            out_eid.data_ptr<int64_t>(), out_nid.data_ptr<int64_t>(), counts.data_ptr<int64_t>(), ws.data_ptr(),
                            wsb, stream_of(rowptr.device())));
  return {out_rowptr, out_col, out_eid, out_nid, counts};
}

// ---------------------------------------------------------------------------------------------------------------
// Autograd: every formula re-dispatches (below the autograd key) to the ops above
// ---------------------------------------------------------------------------------------------------------------
template <typename Sig>
static auto op_handle(const char *name) {
  return c10::Dispatcher::singleton().findSchemaOrThrow(name, "").typed<Sig>();
}
using OptT = c10::optional<Tensor>;
using SegSig = Tensor(const Tensor &, const Tensor &, int64_t);
using SpSig = Tensor(const Tensor &, const OptT &, const Tensor &);

template <Red OP>
struct SegmentFn : public torch::autograd::Function<SegmentFn<OP>> {
  static variable_list forward(AutogradContext *ctx, const Tensor &x, const Tensor &index, int64_t N) {
    at::AutoDispatchBelowADInplaceOrView below;
    ctx->saved_data["x_shape"] = x.sizes().vec();
    ctx->saved_data["N"] = N;
    if (OP == Red::Max) {
      static auto op = op_handle<std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, int64_t)>("ggl::segment_max");
      auto r = op.call(x, index, N);
      ctx->save_for_backward({std::get<1>(r)});
      ctx->mark_non_differentiable({std::get<1>(r)});
      return {std::get<0>(r), std::get<1>(r)};
    }
    static auto op = op_handle<SegSig>(OP == Red::Sum ? "ggl::segment_sum" : "ggl::segment_mean");
    ctx->save_for_backward({index});
    return {op.call(x, index, N)};
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    auto shape = ctx->saved_data["x_shape"].toIntVector();
    Tensor gin;
    if (OP == Red::Sum) {
      static auto op = op_handle<Tensor(const Tensor &, const Tensor &, c10::IntArrayRef)>("ggl::segment_sum_backward");
      gin = op.call(grads[0], saved[0], shape);
    } else if (OP == Red::Mean) {
      static auto op = op_handle<Tensor(const Tensor &, const Tensor &, int64_t, c10::IntArrayRef)>("ggl::segment_mean_backward");
      gin = op.call(grads[0], saved[0], ctx->saved_data["N"].toInt(), shape);
    } else {
      static auto op = op_handle<Tensor(const Tensor &, const Tensor &, c10::IntArrayRef)>("ggl::segment_max_backward");
      gin = op.call(grads[0], saved[0], shape);
    }
    return {gin, Tensor(), Tensor()};
  }
};

struct SegmentSoftmaxFn : public torch::autograd::Function<SegmentSoftmaxFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &x, const Tensor &index, int64_t N) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<SegSig>("ggl::segment_softmax");
    Tensor y = op.call(x, index, N);
    ctx->saved_data["N"] = N;
    ctx->save_for_backward({y, index});
    return y;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    static auto op = op_handle<Tensor(const Tensor &, const Tensor &, const Tensor &, int64_t)>("ggl::segment_softmax_backward");
    return {op.call(grads[0], saved[0], saved[1], ctx->saved_data["N"].toInt()), Tensor(), Tensor()};
  }
};

// gspmm's sum / mean differentiate with respect to a weight that requires grad (an extension: gspmm.cpp:30 marks it
// non-differentiable): such a node saves x as its LAST tensor, a constant weight saves what it always did.  grad_w answers
// the weight's gradient from `saved` (x at `at` when it was kept, else none) in the weight's own shape.
static void save_for_grad_w(AutogradContext *ctx, variable_list keep, const OptT &weight, const Tensor &x) {
  if (opt(weight).defined() && opt(weight).requires_grad()) keep.push_back(x);
  ctx->save_for_backward(keep);
}
static Tensor grad_w(const variable_list &saved, size_t at, const Tensor &g, bool mean) {
  if (saved.size() <= at) return Tensor();
  static auto op = op_handle<Tensor(const Tensor &, const Tensor &, const Tensor &, bool)>("ggl_grad::spmm_grad_w");
  return op.call(saved[0], saved[at], g, mean).view(saved[1].sizes());
}

template <SpOp OP>
struct SpMMFn : public torch::autograd::Function<SpMMFn<OP>> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const OptT &weight, const Tensor &x) {
    at::AutoDispatchBelowADInplaceOrView below;
    // index and weight are not differentiable (gspmm.cpp:30); the arg-max of `max` is a source NODE id
    if (OP == SpOp::Max) {
      static auto op = op_handle<std::tuple<Tensor, Tensor>(const Tensor &, const OptT &, const Tensor &)>("ggl::spmm_max_arg");
      auto r = op.call(index, weight, x);
      ctx->save_for_backward({index, opt(weight), std::get<1>(r)});
      return std::get<0>(r);
    }
    static auto op = op_handle<SpSig>(OP == SpOp::Sum ? "ggl::spmm_sum" : "ggl::spmm_mean");
    save_for_grad_w(ctx, {index, opt(weight)}, weight, x);
    return op.call(index, weight, x);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    OptT w = saved[1].defined() ? OptT(saved[1]) : OptT();
    Tensor gx;
    if (OP == SpOp::Max) {
      static auto op = op_handle<Tensor(const Tensor &, const OptT &, const Tensor &, const Tensor &)>("ggl::spmm_max_backward");
      gx = op.call(saved[0], w, grads[0], saved[2]);
      return {Tensor(), Tensor(), gx};
    }
    static auto op = op_handle<SpSig>(OP == SpOp::Sum ? "ggl::spmm_sum_backward" : "ggl::spmm_mean_backward");
    gx = op.call(saved[0], w, grads[0]);
    return {Tensor(), grad_w(saved, 2, grads[0], OP == SpOp::Mean), gx};
  }
};

struct BSpMMFn : public torch::autograd::Function<BSpMMFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const Tensor &weight, const Tensor &x) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<Tensor(const Tensor &, const Tensor &, const Tensor &)>("ggl::bspmm_sum");
    ctx->save_for_backward({index, weight, x});
    return op.call(index, weight, x);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    static auto op = op_handle<std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &)>(
        "ggl::bspmm_sum_backward");
    auto r = op.call(saved[0], saved[1], saved[2], grads[0]);
    // the reference returns grad_weight although it marked weight non-differentiable (gspmm.cpp:208,259)
    return {Tensor(), std::get<0>(r), std::get<1>(r)};
  }
};

static Tensor segment_sum_autograd(const Tensor &x, const Tensor &i, int64_t N) { return SegmentFn<Red::Sum>::apply(x, i, N)[0]; }
static Tensor segment_mean_autograd(const Tensor &x, const Tensor &i, int64_t N) { return SegmentFn<Red::Mean>::apply(x, i, N)[0]; }
static std::tuple<Tensor, Tensor> segment_max_autograd(const Tensor &x, const Tensor &i, int64_t N) {
  auto r = SegmentFn<Red::Max>::apply(x, i, N);
  return {r[0], r[1]};
}
static Tensor segment_softmax_autograd(const Tensor &x, const Tensor &i, int64_t N) { return SegmentSoftmaxFn::apply(x, i, N); }
// f16 / bf16 rows with an f32 result: the gradient arrives in f32, is walked in f32 and rounded once to x's dtype
template <SpOp OP>
struct SpMMX16Fn : public torch::autograd::Function<SpMMX16Fn<OP>> {
  using Sig16 = Tensor(const Tensor &, const OptT &, const Tensor &, bool);
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const OptT &weight, const Tensor &x, bool out_f32) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<Sig16>(OP == SpOp::Sum ? "ggl::spmm_sum_x16" : "ggl::spmm_mean_x16");
    save_for_grad_w(ctx, {index, opt(weight)}, weight, x);
    ctx->saved_data["x_dtype"] = static_cast<int64_t>(x.scalar_type());
    return op.call(index, weight, x, out_f32);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto saved = ctx->get_saved_variables();
    OptT w = saved[1].defined() ? OptT(saved[1]) : OptT();
    static auto op = op_handle<SpSig>(OP == SpOp::Sum ? "ggl::spmm_sum_backward" : "ggl::spmm_mean_backward");
    Tensor gx = op.call(saved[0], w, grads[0]);
    const auto xt = static_cast<at::ScalarType>(ctx->saved_data["x_dtype"].toInt());
    return {Tensor(), grad_w(saved, 2, grads[0], OP == SpOp::Mean), gx.scalar_type() == xt ? gx : gx.to(xt), Tensor()};
  }
};
static Tensor spmm_sum_x16_autograd(const Tensor &i, const OptT &w, const Tensor &x, bool f) { return SpMMX16Fn<SpOp::Sum>::apply(i, w, x, f); }
static Tensor spmm_mean_x16_autograd(const Tensor &i, const OptT &w, const Tensor &x, bool f) { return SpMMX16Fn<SpOp::Mean>::apply(i, w, x, f); }
static Tensor spmm_sum_autograd(const Tensor &i, const OptT &w, const Tensor &x) { return SpMMFn<SpOp::Sum>::apply(i, w, x); }
static Tensor spmm_mean_autograd(const Tensor &i, const OptT &w, const Tensor &x) { return SpMMFn<SpOp::Mean>::apply(i, w, x); }
static Tensor spmm_max_autograd(const Tensor &i, const OptT &w, const Tensor &x) { return SpMMFn<SpOp::Max>::apply(i, w, x); }
static Tensor bspmm_sum_autograd(const Tensor &i, const Tensor &w, const Tensor &x) { return BSpMMFn::apply(i, w, x); }

// ---- autograd of the fused route --------------------------------------------------------------------------------
using GatFwdSig = std::tuple<Tensor, Tensor, Tensor, Tensor, bool>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                                    double, int64_t, double);
using GatBwdSig = std::tuple<Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                     const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                     const Tensor &, double, int64_t, double, bool);
// f16 / bf16 rows with the choice of an f32 result: the forward of gat_fused_x16, (out, rowmax, rowden, rng_used)
using GatX16FwdSig = std::tuple<Tensor, Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                                double, int64_t, double, bool);
// gat_fused and (x16 = true) gat_fused_x16: the backward of both is gat_fused_backward on the out the forward returned,
// 16-bit rows through the general kernels (fast = false)
struct GatFn : public torch::autograd::Function<GatFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const Tensor &el, const Tensor &er, const Tensor &x,
                        double slope, int64_t n, double p, bool x16, bool out_f32) {
    at::AutoDispatchBelowADInplaceOrView below;
    Tensor out, rmax, rden, used;
    bool fast = false;
    if (x16) {
      static auto op = op_handle<GatX16FwdSig>("ggl::gat_fused_x16_forward");
      std::tie(out, rmax, rden, used) = op.call(index, el, er, x, slope, n, p, out_f32);
    } else {
      static auto op = op_handle<GatFwdSig>("ggl::gat_fused_forward");
      std::tie(out, rmax, rden, used, fast) = op.call(index, el, er, x, slope, n, p);
    }
    ctx->save_for_backward({index, el, er, x, out, rmax, rden, used});
    ctx->saved_data["slope"] = slope;
    ctx->saved_data["n"] = n;
    ctx->saved_data["p"] = p;
    ctx->saved_data["fast"] = fast;
    return out;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    static auto op = op_handle<GatBwdSig>("ggl::gat_fused_backward");
    auto r = op.call(s[0], s[1], s[2], s[3], grads[0], s[4], s[5], s[6], s[7], ctx->saved_data["slope"].toDouble(),
                     ctx->saved_data["n"].toInt(), ctx->saved_data["p"].toDouble(), ctx->saved_data["fast"].toBool());
    return {Tensor(), std::get<0>(r), std::get<1>(r), std::get<2>(r), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};
// apply(x) on x zero-padded to the policy's head width (41 classes per head: one padded copy keeps every walk on 16-byte
// slices, ops.py Engine.gat_fused), the pad channels — they aggregate to zero — sliced off again; pad and slice are ordinary
// differentiable ops.  E < 0: no policy (the index is not an edge list), x as it is.
template <typename Apply>
static Tensor with_head_pad(const Tensor &x, int64_t E, Apply apply) {
  const int64_t C = x.size(2), Cp = E < 0 ? C : api_for(x.device()).ggl_policy_head_channels(C, E, x.size(0));
  if (Cp == C) return apply(x);
  return apply(at::constant_pad_nd(x, {0, Cp - C})).slice(2, 0, C);
}
static Tensor gat_autograd(const Tensor &index, const Tensor &el, const Tensor &er, const Tensor &x, double slope,
                           c10::optional<int64_t> num_nodes, double p, bool x16, bool out_f32) {
  gat_check(el, er, x);
  TORCH_CHECK(!x16 || is_x16(x), "gat_fused_x16 takes f16 / bf16 rows (x is ", x.scalar_type(), ")");
  const int64_t n = num_nodes.has_value() ? *num_nodes : x.size(0);
  return with_head_pad(x, index.dim() == 2 ? index.size(1) : -1,
                       [&](const Tensor &xp) { return GatFn::apply(index, el, er, xp, slope, n, p, x16, out_f32); });
}
static Tensor gat_fused_autograd(const Tensor &index, const Tensor &el, const Tensor &er, const Tensor &x, double slope,
                                 c10::optional<int64_t> num_nodes, double p) {
  return gat_autograd(index, el, er, x, slope, num_nodes, p, false, false);
}
static Tensor gat_fused_x16_autograd(const Tensor &index, const Tensor &el, const Tensor &er, const Tensor &x, double slope,
                                     c10::optional<int64_t> num_nodes, double p, bool out_f32) {
  return gat_autograd(index, el, er, x, slope, num_nodes, p, true, out_f32);
}

// edge_softmax_aggregate: forward and backward are ops of ggl_attn; gz / gx are asked for only where the input requires grad
using EsaFwdSig = std::tuple<Tensor, Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, int64_t, double);
using EsaBwdSig = std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                             const Tensor &, const Tensor &, const Tensor &, int64_t, double, bool, bool);
struct EsaFn : public torch::autograd::Function<EsaFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const Tensor &z, const Tensor &x, int64_t n, double p) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<EsaFwdSig>("ggl_attn::edge_softmax_aggregate_forward");
    Tensor out, rmax, rden, used;
    std::tie(out, rmax, rden, used) = op.call(index, z, x, n, p);
    ctx->save_for_backward({index, z, x, out, rmax, rden, used});
    ctx->saved_data["n"] = n;
    ctx->saved_data["p"] = p;
    return out;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    static auto op = op_handle<EsaBwdSig>("ggl_attn::edge_softmax_aggregate_backward");
    const bool need_z = ctx->needs_input_grad(1), need_x = ctx->needs_input_grad(2);
    auto r = op.call(s[0], s[1], s[2], grads[0], s[3], s[4], s[5], s[6], ctx->saved_data["n"].toInt(),
                     ctx->saved_data["p"].toDouble(), need_z, need_x);
    return {Tensor(), need_z ? std::get<0>(r) : Tensor(), need_x ? std::get<1>(r) : Tensor(), Tensor(), Tensor()};
  }
};
// logits [E] with x [N, K] are one head
static Tensor esa_autograd(const Tensor &index, const Tensor &z, const Tensor &x, c10::optional<int64_t> num_nodes, double p) {
  if (z.dim() == 1 && x.dim() == 2)
    return esa_autograd(index, z.unsqueeze(1), x.unsqueeze(1), num_nodes, p).squeeze(1);
  esa_check(index, z, x);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  const int64_t n = num_nodes.has_value() ? *num_nodes : x.size(0);
  return with_head_pad(x, index.size(1), [&](const Tensor &xp) { return EsaFn::apply(index, z, xp, n, p); });
}

// dot_attention: as edge_softmax_aggregate; the logits are kept by the forward only where q, k or v requires grad
using DotFwdSig = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                                     int64_t, double, double, bool);
using DotBwdSig = std::tuple<Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                     const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                     int64_t, double, double, bool, bool, bool);
// the autograd node of an op with three differentiable tensors a, b, c and one scalar s (dot_attention: q, k, v, scale;
// gatv2_attention: xl, xr, att, slope); Op names its two passes
struct DotOps {
  static constexpr const char *fwd = "ggl_attn::dot_attention_forward", *bwd = "ggl_attn::dot_attention_backward";
};
struct Gatv2Ops {
  static constexpr const char *fwd = "ggl_attn::gatv2_attention_forward", *bwd = "ggl_attn::gatv2_attention_backward";
};
template <typename Op>
struct LogitAttnFn : public torch::autograd::Function<LogitAttnFn<Op>> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const Tensor &a, const Tensor &b, const Tensor &c, int64_t n,
                        double s, double p, bool need) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<DotFwdSig>(Op::fwd);
    Tensor out, rmax, rden, used, z;
    std::tie(out, rmax, rden, used, z) = op.call(index, a, b, c, n, s, p, need);
    if (need) ctx->save_for_backward({index, a, b, c, z, out, rmax, rden, used});
    ctx->saved_data["n"] = n;
    ctx->saved_data["s"] = s;
    ctx->saved_data["p"] = p;
    return out;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    static auto op = op_handle<DotBwdSig>(Op::bwd);
    const bool need_a = ctx->needs_input_grad(1), need_b = ctx->needs_input_grad(2), need_c = ctx->needs_input_grad(3);
    auto r = op.call(s[0], s[1], s[2], s[3], s[4], grads[0], s[5], s[6], s[7], s[8], ctx->saved_data["n"].toInt(),
                     ctx->saved_data["s"].toDouble(), ctx->saved_data["p"].toDouble(), need_a, need_b, need_c);
    return {Tensor(), need_a ? std::get<0>(r) : Tensor(), need_b ? std::get<1>(r) : Tensor(), need_c ? std::get<2>(r) : Tensor(),
            Tensor(), Tensor(), Tensor(), Tensor()};
  }
};
// q [N, C] with k, v [N, C] are one head
static Tensor dot_autograd(const Tensor &index, const Tensor &q, const Tensor &k, const Tensor &v, c10::optional<int64_t> num_nodes,
                           c10::optional<double> scale, double p) {
  if (q.dim() == 2 && k.dim() == 2 && v.dim() == 2)
    return dot_autograd(index, q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1), num_nodes, scale, p).squeeze(1);
  dot_check(index, q, k, v);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  const int64_t n = num_nodes.has_value() ? *num_nodes : q.size(0);
  const double sc = scale.has_value() ? *scale : 1.0 / std::sqrt(static_cast<double>(q.size(2)));
  const bool need = at::GradMode::is_enabled() && (q.requires_grad() || k.requires_grad() || v.requires_grad());
  return LogitAttnFn<DotOps>::apply(index, q, k, v, n, sc, p, need);
}

// gatv2_attention: as dot_attention; the logits are kept by the forward only where xl, xr or att requires grad
// xl [N, C], xr [N, C] with att [C] are one head
static Tensor gatv2_autograd(const Tensor &index, const Tensor &xl, const Tensor &xr, const Tensor &att,
                             c10::optional<int64_t> num_nodes, double slope, double p) {
  if (xl.dim() == 2 && xr.dim() == 2 && att.dim() == 1)
    return gatv2_autograd(index, xl.unsqueeze(1), xr.unsqueeze(1), att.unsqueeze(0), num_nodes, slope, p).squeeze(1);
  gatv2_check(index, xl, xr, att);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_rate must be in [0, 1)");
  const int64_t n = num_nodes.has_value() ? *num_nodes : xr.size(0);
  const bool need = at::GradMode::is_enabled() && (xl.requires_grad() || xr.requires_grad() || att.requires_grad());
  return LogitAttnFn<Gatv2Ops>::apply(index, xl, xr, att, n, slope, p, need);
}

using GatCsrFwdSig = std::tuple<Tensor, Tensor, Tensor, Tensor, bool>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                                       const Tensor &, const Tensor &, const Tensor &,
                                                                       const Tensor &, double, double);
using GatCsrBwdSig = std::tuple<Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                        const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                        const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                        const Tensor &, double, double, bool);
struct GatCsrFn : public torch::autograd::Function<GatCsrFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &rp, const Tensor &ci, const Tensor &cp, const Tensor &ri,
                        const Tensor &pm, const Tensor &el, const Tensor &er, const Tensor &x, double slope, double p) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<GatCsrFwdSig>("ggl::gat_fused_csr_forward");
    auto r = op.call(rp, ci, cp, ri, pm, el, er, x, slope, p);
    ctx->save_for_backward({rp, ci, cp, ri, pm, el, er, x, std::get<0>(r), std::get<1>(r), std::get<2>(r), std::get<3>(r)});
    ctx->saved_data["slope"] = slope;
    ctx->saved_data["p"] = p;
    ctx->saved_data["fast"] = std::get<4>(r);
    return std::get<0>(r);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    static auto op = op_handle<GatCsrBwdSig>("ggl::gat_fused_csr_backward");
    auto r = op.call(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], grads[0], s[8], s[9], s[10], s[11],
                     ctx->saved_data["slope"].toDouble(), ctx->saved_data["p"].toDouble(), ctx->saved_data["fast"].toBool());
    return {Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), std::get<0>(r), std::get<1>(r), std::get<2>(r), Tensor(), Tensor()};
  }
};
static Tensor gat_fused_csr_autograd(const Tensor &rp, const Tensor &ci, const Tensor &cp, const Tensor &ri, const Tensor &pm,
                                     const Tensor &el, const Tensor &er, const Tensor &x, double slope, double p) {
  gat_check(el, er, x);
  return with_head_pad(x, ci.size(0), [&](const Tensor &xp) { return GatCsrFn::apply(rp, ci, cp, ri, pm, el, er, xp, slope, p); });
}

using BiasFwdSig = std::tuple<Tensor, Tensor>(const Tensor &, const OptT_ &, bool, double);
using BiasBwdSig = std::tuple<Tensor, Tensor>(const Tensor &, const Tensor &, bool, bool, double, const Tensor &);
// a node's bias: whether there is one and its shape are kept at the forward; the backward's flat [K] gradient goes back in
// that shape, or undefined without a bias
static void save_bias(AutogradContext *ctx, const OptT_ &bias) {
  const Tensor b = opt(bias);
  ctx->saved_data["has_bias"] = b.defined();
  ctx->saved_data["bias_shape"] = b.defined() ? b.sizes().vec() : std::vector<int64_t>{};
}
static bool has_bias(AutogradContext *ctx) { return ctx->saved_data["has_bias"].toBool(); }
static Tensor bias_grad(AutogradContext *ctx, const Tensor &flat) {
  return has_bias(ctx) ? flat.reshape(ctx->saved_data["bias_shape"].toIntVector()) : Tensor();
}
// (ga, gbias) back through dropout / ReLU / + bias of a node that saved "relu" and its bias (save_bias): y is the output
// it returned, rng_used what its forward op returned (empty and p = 0 for a node without dropout)
static std::tuple<Tensor, Tensor> epi_backward(AutogradContext *ctx, const Tensor &g, const Tensor &y, double p,
                                               const Tensor &rng_used) {
  static auto op = op_handle<BiasBwdSig>("ggl::bias_act_backward");
  auto r = op.call(g, y, has_bias(ctx), ctx->saved_data["relu"].toBool(), p, rng_used);
  return {std::get<0>(r), bias_grad(ctx, std::get<1>(r))};
}
struct BiasActFn : public torch::autograd::Function<BiasActFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &a, const OptT_ &bias, bool relu, double p) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<BiasFwdSig>("ggl::bias_act_forward");
    auto r = op.call(a, bias, relu, p);
    ctx->save_for_backward({std::get<0>(r), std::get<1>(r)});
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["p"] = p;
    save_bias(ctx, bias);
    return std::get<0>(r);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    auto [ga, gb] = epi_backward(ctx, grads[0], s[0], ctx->saved_data["p"].toDouble(), s[1]);
    return {ga, gb, Tensor(), Tensor()};
  }
};
static Tensor bias_act_autograd(const Tensor &a, const OptT_ &bias, bool relu, double p) { return BiasActFn::apply(a, bias, relu, p); }

using EpiFwdSig = std::tuple<Tensor, Tensor>(const Tensor &, const OptT_ &, const Tensor &, bool, const OptT_ &, const OptT_ &, bool, double);
struct SpMMEpiFn : public torch::autograd::Function<SpMMEpiFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const OptT_ &weight, const Tensor &x, bool mean,
                        const OptT_ &add, const OptT_ &bias, bool relu, double p) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<EpiFwdSig>("ggl::spmm_epi_forward");
    auto r = op.call(index, weight, x, mean, add, bias, relu, p);
    save_for_grad_w(ctx, {index, opt(weight), std::get<0>(r), std::get<1>(r)}, weight, x);
    ctx->saved_data["mean"] = mean;
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["p"] = p;
    ctx->saved_data["has_add"] = opt(add).defined();
    save_bias(ctx, bias);
    return std::get<0>(r);
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    auto [ga, gb] = epi_backward(ctx, grads[0], s[2], ctx->saved_data["p"].toDouble(), s[3]);
    OptT_ w = s[1].defined() ? OptT_(s[1]) : OptT_();
    static auto sum_bwd = op_handle<SpSig>("ggl::spmm_sum_backward");
    static auto mean_bwd = op_handle<SpSig>("ggl::spmm_mean_backward");
    const bool mean = ctx->saved_data["mean"].toBool();
    Tensor gx = mean ? mean_bwd.call(s[0], w, ga) : sum_bwd.call(s[0], w, ga);
    // the weight's gradient is the edge-dot of x with the PRE-ACTIVATION gradient
    return {Tensor(), grad_w(s, 4, ga, mean), gx, Tensor(), ctx->saved_data["has_add"].toBool() ? ga : Tensor(), gb, Tensor(),
            Tensor()};
  }
};
// one kernel for 16-byte rows; the reduce op followed by the adds and the epilogue pass otherwise (same values)
static Tensor spmm_epi_autograd(const Tensor &index, const OptT_ &weight, const Tensor &x, bool mean, const OptT_ &add,
                                const OptT_ &bias, bool relu, double p) {
  if (x.dim() == 2 && (x.size(1) % 4 == 0 || is_x16(x))) return SpMMEpiFn::apply(index, weight, x, mean, add, bias, relu, p);
  Tensor out = mean ? spmm_mean_autograd(index, weight, x) : spmm_sum_autograd(index, weight, x);
  if (opt(add).defined()) out = out + *add;
  return BiasActFn::apply(out, bias, relu, p);
}

// (A x + bias)[rows] computed on the listed rows alone; the edge weights carry no gradient here (bspmm_sum is that op)
struct SpMMRowsFn : public torch::autograd::Function<SpMMRowsFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &index, const OptT_ &weight, const Tensor &x, const Tensor &rows,
                        const OptT_ &bias) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<Tensor(const Tensor &, const OptT_ &, const Tensor &, const Tensor &, const OptT_ &)>(
        "ggl::spmm_rows_forward");
    Tensor y = op.call(index, weight, x, rows, bias);
    ctx->save_for_backward({index, opt(weight), rows});
    ctx->saved_data["n_src"] = x.size(0);
    save_bias(ctx, bias);
    return y;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    static auto op = op_handle<std::tuple<Tensor, Tensor>(const Tensor &, const OptT_ &, const Tensor &, const Tensor &, int64_t,
                                                          bool)>("ggl::spmm_rows_backward");
    OptT_ w = s[1].defined() ? OptT_(s[1]) : OptT_();
    auto r = op.call(s[0], w, grads[0], s[2], ctx->saved_data["n_src"].toInt(), has_bias(ctx));
    return {Tensor(), Tensor(), std::get<0>(r), Tensor(), bias_grad(ctx, std::get<1>(r))};
  }
};
static Tensor spmm_rows_autograd(const Tensor &index, const OptT_ &weight, const Tensor &x, const Tensor &rows,
                                 const OptT_ &bias) {
  TORCH_CHECK(!(opt(weight).defined() && opt(weight).requires_grad()),
              "spmm_rows has no gradient for the edge weights: pass detached weights (bspmm_sum is the op with a weight gradient)");
  return SpMMRowsFn::apply(index, weight, x, rows, bias);
}

struct SegEpiFn : public torch::autograd::Function<SegEpiFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &x, const Tensor &index, int64_t N, bool mean, const OptT_ &add,
                        const OptT_ &bias, bool relu) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<Tensor(const Tensor &, const Tensor &, int64_t, bool, const OptT_ &, const OptT_ &, bool)>(
        "ggl::segment_epi_forward");
    Tensor y = op.call(x, index, N, mean, add, bias, relu);
    ctx->save_for_backward({index, y});
    ctx->saved_data["x_shape"] = x.sizes().vec();
    ctx->saved_data["N"] = N;
    ctx->saved_data["mean"] = mean;
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["has_add"] = opt(add).defined();
    save_bias(ctx, bias);
    return y;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    auto [ga, gb] = epi_backward(ctx, grads[0], s[1], 0.0, at::empty({0}, s[0].options()));
    auto shape = ctx->saved_data["x_shape"].toIntVector();
    Tensor gx;
    if (ctx->saved_data["mean"].toBool()) {
      static auto op = op_handle<Tensor(const Tensor &, const Tensor &, int64_t, c10::IntArrayRef)>("ggl::segment_mean_backward");
      gx = op.call(ga, s[0], ctx->saved_data["N"].toInt(), shape);
    } else {
      static auto op = op_handle<Tensor(const Tensor &, const Tensor &, c10::IntArrayRef)>("ggl::segment_sum_backward");
      gx = op.call(ga, s[0], shape);
    }
    return {gx, Tensor(), Tensor(), Tensor(), ctx->saved_data["has_add"].toBool() ? ga : Tensor(), gb, Tensor()};
  }
};
static Tensor segment_epi_autograd(const Tensor &x, const Tensor &index, int64_t N, bool mean, const OptT_ &add,
                                   const OptT_ &bias, bool relu) {
  return SegEpiFn::apply(x, index, N, mean, add, bias, relu);
}

// ---------------------------------------------------------------------------------------------------------------
// Meta (shapes / dtypes only) and housekeeping ops
// ---------------------------------------------------------------------------------------------------------------
static Tensor seg_meta(const Tensor &x, const Tensor &, int64_t N) { return at::empty(out_shape(x, N), x.options()); }
static std::tuple<Tensor, Tensor> seg_max_meta(const Tensor &x, const Tensor &, int64_t N) {
  return {at::empty(out_shape(x, N), x.options()), at::empty(out_shape(x, N), x.options().dtype(at::kLong))};
}
static Tensor like_x_meta(const Tensor &, const OptT &, const Tensor &x) { return at::empty_like(x); }
static Tensor x16_meta(const Tensor &, const OptT &, const Tensor &x, bool out_f32) {
  return out_f32 ? at::empty(x.sizes(), x.options().dtype(at::kFloat)) : at::empty_like(x);
}
static Tensor spmm_grad_w_meta(const Tensor &index, const Tensor &, const Tensor &g, bool) {
  return at::empty({index.size(1)}, g.options().dtype(at::kFloat));
}
static std::tuple<Tensor, Tensor> spmm_max_arg_meta(const Tensor &, const OptT &, const Tensor &x) {
  return {at::empty_like(x), at::empty(x.sizes(), x.options().dtype(at::kLong))};
}
static Tensor bspmm_meta(const Tensor &, const Tensor &, const Tensor &x) { return at::empty_like(x); }
static Tensor softmax_meta(const Tensor &x, const Tensor &, int64_t) { return at::empty_like(x); }
static Tensor softmax_bwd_meta(const Tensor &, const Tensor &y, const Tensor &, int64_t) { return at::empty_like(y); }
static Tensor seg_bwd_meta(const Tensor &g, const Tensor &, c10::IntArrayRef shape) { return at::empty(shape, g.options()); }
static Tensor seg_mean_bwd_meta(const Tensor &g, const Tensor &, int64_t, c10::IntArrayRef shape) {
  return at::empty(shape, g.options());
}
static Tensor spmm_max_bwd_meta(const Tensor &, const OptT &, const Tensor &g, const Tensor &) { return at::empty_like(g); }
static std::tuple<Tensor, Tensor> bspmm_bwd_meta(const Tensor &, const Tensor &w, const Tensor &x, const Tensor &) {
  return {at::empty_like(w), at::empty_like(x)};
}

static std::tuple<Tensor, Tensor, Tensor, Tensor, bool> gat_fwd_meta(const Tensor &, const Tensor &, const Tensor &er,
                                                                     const Tensor &x, double, int64_t n, double) {
  auto o = x.options(), f = er.options();   // the statistics are f32 whatever x is stored as
  return {at::empty({n, x.size(1), x.size(2)}, o), at::empty({n, x.size(1)}, f), at::empty({n, x.size(1)}, f),
          at::empty({0}, o.dtype(at::kLong)), false};
}
static std::tuple<Tensor, Tensor, Tensor, Tensor> gat_x16_fwd_meta(const Tensor &, const Tensor &, const Tensor &er,
                                                                   const Tensor &x, double, int64_t n, double, bool out_f32) {
  auto o = out_f32 ? x.options().dtype(at::kFloat) : x.options(), f = er.options();
  return {at::empty({n, x.size(1), x.size(2)}, o), at::empty({n, x.size(1)}, f), at::empty({n, x.size(1)}, f),
          at::empty({0}, o.dtype(at::kLong))};
}
static Tensor gat_x16_meta(const Tensor &, const Tensor &, const Tensor &, const Tensor &x, double, c10::optional<int64_t> n,
                           double, bool out_f32) {
  return at::empty({n.has_value() ? *n : x.size(0), x.size(1), x.size(2)},
                   out_f32 ? x.options().dtype(at::kFloat) : x.options());
}
static std::tuple<Tensor, Tensor, Tensor> gat_bwd_meta(const Tensor &, const Tensor &el, const Tensor &er, const Tensor &x,
                                                       const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                       const Tensor &, double, int64_t, double, bool) {
  return {at::empty_like(el), at::empty_like(er), at::empty_like(x)};
}
static Tensor gat_meta(const Tensor &, const Tensor &, const Tensor &, const Tensor &x, double, c10::optional<int64_t> n, double) {
  return at::empty({n.has_value() ? *n : x.size(0), x.size(1), x.size(2)}, x.options());
}
static std::tuple<Tensor, Tensor, Tensor, Tensor> esa_fwd_meta(const Tensor &, const Tensor &, const Tensor &x, int64_t n, double) {
  auto o = x.options();
  return {at::empty({n, x.size(1), x.size(2)}, o), at::empty({n, x.size(1)}, o), at::empty({n, x.size(1)}, o),
          at::empty({0}, o.dtype(at::kLong))};
}
static std::tuple<Tensor, Tensor> esa_bwd_meta(const Tensor &, const Tensor &z, const Tensor &x, const Tensor &, const Tensor &,
                                               const Tensor &, const Tensor &, const Tensor &, int64_t, double, bool need_z,
                                               bool need_x) {
  return {need_z ? at::empty_like(z) : at::empty({0}, z.options()), need_x ? at::empty_like(x) : at::empty({0}, x.options())};
}
static Tensor esa_meta(const Tensor &, const Tensor &z, const Tensor &x, c10::optional<int64_t> n, double) {
  const int64_t N = n.has_value() ? *n : x.size(0);
  if (z.dim() == 1 && x.dim() == 2) return at::empty({N, x.size(1)}, x.options());
  return at::empty({N, x.size(1), x.size(2)}, x.options());
}
// the passes of dot_attention (a, b, c = q, k, v) and gatv2_attention (xl, xr, att): every one of q, k, v, xl, xr is [., H, C]
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> logit_attn_fwd_meta(const Tensor &index, const Tensor &a, const Tensor &,
                                                                              const Tensor &, int64_t n, double, double, bool keep) {
  auto o = a.options();
  return {at::empty({n, a.size(1), a.size(2)}, o), at::empty({n, a.size(1)}, o), at::empty({n, a.size(1)}, o),
          at::empty({0}, o.dtype(at::kLong)), keep ? at::empty({index.size(1), a.size(1)}, o) : at::empty({0}, o)};
}
static std::tuple<Tensor, Tensor, Tensor> logit_attn_bwd_meta(const Tensor &, const Tensor &a, const Tensor &b, const Tensor &c,
                                                              const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                              const Tensor &, const Tensor &, int64_t, double, double, bool need_a,
                                                              bool need_b, bool need_c) {
  auto e = [&]() { return at::empty({0}, a.options()); };
  return {need_a ? at::empty_like(a) : e(), need_b ? at::empty_like(b) : e(), need_c ? at::empty_like(c) : e()};
}
static Tensor dot_meta(const Tensor &, const Tensor &q, const Tensor &, const Tensor &v, c10::optional<int64_t> n,
                       c10::optional<double>, double) {
  const int64_t N = n.has_value() ? *n : q.size(0);
  if (v.dim() == 2) return at::empty({N, v.size(1)}, v.options());
  return at::empty({N, v.size(1), v.size(2)}, v.options());
}
static Tensor gatv2_meta(const Tensor &, const Tensor &xl, const Tensor &xr, const Tensor &, c10::optional<int64_t> n, double, double) {
  const int64_t N = n.has_value() ? *n : xr.size(0);
  if (xl.dim() == 2) return at::empty({N, xl.size(1)}, xl.options());
  return at::empty({N, xl.size(1), xl.size(2)}, xl.options());
}
static std::tuple<Tensor, Tensor, Tensor, Tensor, bool> gat_csr_fwd_meta(const Tensor &rp, const Tensor &, const Tensor &,
                                                                         const Tensor &, const Tensor &, const Tensor &,
                                                                         const Tensor &, const Tensor &x, double, double) {
  const int64_t n = rp.size(0) - 1;
  auto o = x.options(), f = x.options().dtype(at::kFloat);
  return {at::empty({n, x.size(1), x.size(2)}, o), at::empty({n, x.size(1)}, f), at::empty({n, x.size(1)}, f),
          at::empty({0}, o.dtype(at::kLong)), false};
}
static std::tuple<Tensor, Tensor, Tensor> gat_csr_bwd_meta(const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                           const Tensor &, const Tensor &el, const Tensor &er, const Tensor &x,
                                                           const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                                                           const Tensor &, double, double, bool) {
  return {at::empty_like(el), at::empty_like(er), at::empty_like(x)};
}
static Tensor gat_csr_meta(const Tensor &rp, const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                           const Tensor &, const Tensor &x, double, double) {
  return at::empty({rp.size(0) - 1, x.size(1), x.size(2)}, x.options());
}
static std::tuple<Tensor, Tensor> bias_fwd_meta(const Tensor &a, const OptT_ &, bool, double) {
  return {at::empty_like(a), at::empty({0}, a.options().dtype(at::kLong))};
}
static std::tuple<Tensor, Tensor> bias_bwd_meta(const Tensor &g, const Tensor &, bool hb, bool, double, const Tensor &) {
  const int64_t N = g.dim() > 0 ? g.size(0) : 1;
  return {at::empty_like(g), at::empty({hb && N > 0 ? g.numel() / N : 0}, g.options().dtype(at::kFloat))};
}
static Tensor bias_meta(const Tensor &a, const OptT_ &, bool, double) { return at::empty_like(a); }
static std::tuple<Tensor, Tensor> lin_bias_bwd_meta(const Tensor &g, const Tensor &w, const Tensor &y, bool hb, bool, double,
                                                    const Tensor &) {
  return {at::empty_like(y), at::empty({hb ? w.size(1) : 0}, g.options().dtype(at::kFloat))};
}
static std::tuple<Tensor, Tensor> epi_fwd_meta(const Tensor &, const OptT_ &, const Tensor &x, bool, const OptT_ &, const OptT_ &,
                                               bool, double) {
  return {at::empty_like(x), at::empty({0}, x.options().dtype(at::kLong))};
}
static Tensor epi_meta(const Tensor &, const OptT_ &, const Tensor &x, bool, const OptT_ &, const OptT_ &, bool, double) {
  return at::empty_like(x);
}
static Tensor rows_meta(const Tensor &, const OptT_ &, const Tensor &x, const Tensor &rows, const OptT_ &) {
  return at::empty({rows.size(0), x.size(1)}, x.options());
}
static std::tuple<Tensor, Tensor> rows_bwd_meta(const Tensor &, const OptT_ &, const Tensor &g, const Tensor &, int64_t n_src,
                                                bool hb) {
  return {at::empty({n_src, g.size(1)}, g.options()), at::empty({hb ? g.size(1) : 0}, g.options())};
}
static Tensor seg_epi_meta(const Tensor &x, const Tensor &, int64_t N, bool, const OptT_ &, const OptT_ &, bool) {
  return at::empty(out_shape(x, N), x.options());
}

static void clear_caches() {
  seg_cache().clear();
  graph_cache().clear();
  csr_cache().clear();
  rows_cache().clear();
}
static std::vector<int64_t> plan_stats() {
  return {static_cast<int64_t>(g_plans_built.load()), static_cast<int64_t>(g_plan_hits.load())};
}

// ---------------------------------------------------------------------------------------------------------------
// ggl_agg::segment_multi — several statistics (GGL_AGG_* codes) of x [E, K] per segment in one walk each way
// (ggl_segment_multi_fwd / _bwd, csrc/multiagg.hpp).  out [N, K / C, A, C] stored as [N, A * K].  The passes hand what was
// not produced / is not needed as tensors of 0 elements.
// ---------------------------------------------------------------------------------------------------------------
struct MultiAggs {
  std::vector<int> codes;
  bool sq = false, mn = false, mx = false, sd = false;
};
static MultiAggs multi_aggs(c10::IntArrayRef aggs) {
  MultiAggs m;
  TORCH_CHECK(aggs.size() >= 1 && aggs.size() <= 6, "segment_multi: between 1 and 6 aggregators");
  for (int64_t c : aggs) {
    TORCH_CHECK(c >= GGL_AGG_SUM && c <= GGL_AGG_STD, "segment_multi: unknown aggregator code ", c);
    TORCH_CHECK(std::find(m.codes.begin(), m.codes.end(), static_cast<int>(c)) == m.codes.end(), "segment_multi: aggregator code ", c,
                " is given twice");
    m.codes.push_back(static_cast<int>(c));
    m.sq = m.sq || c == GGL_AGG_VAR || c == GGL_AGG_STD;
    m.sd = m.sd || c == GGL_AGG_STD;
    m.mn = m.mn || c == GGL_AGG_MIN;
    m.mx = m.mx || c == GGL_AGG_MAX;
  }
  return m;
}
static void multi_check(const Tensor &x, const Tensor &index, int64_t C) {
  seg_args(x, index);
  f32("x", x);
  TORCH_CHECK(x.dim() == 2, "segment_multi expects x [E, K], got ", x.sizes());
  TORCH_CHECK(C > 0 && x.size(1) % C == 0, "segment_multi: C = ", C, " does not divide K = ", x.size(1));
}
template <typename T> static T *ptr_or_null(const Tensor &t) { return t.defined() && t.numel() > 0 ? t.data_ptr<T>() : nullptr; }

static std::tuple<Tensor, Tensor, Tensor, Tensor> multi_forward_kernel(const Tensor &x_, const Tensor &index, int64_t N,
                                                                       c10::IntArrayRef aggs, int64_t C, bool empty_zero,
                                                                       bool want_mean) {
  multi_check(x_, index, C);
  const MultiAggs m = multi_aggs(aggs);
  const auto dev = x_.device();
  c10::OptionalDeviceGuard guard(dev);
  const Api &a = api_for(dev);
  Tensor x = x_.contiguous();
  auto plan = seg_plan(index, N);
  TORCH_CHECK_INDEX(x.size(0) == plan->E, "fisrt dimension of x and index should be same");
  const int64_t K = x.size(1), A = static_cast<int64_t>(m.codes.size());
  auto o = x.options();
  Tensor out = at::empty({N, A * K}, o);
  Tensor mean = want_mean && m.sq ? at::empty({N, K}, o) : at::empty({0}, o);
  Tensor amin = m.mn ? at::empty({N, K}, o.dtype(at::kInt)) : at::empty({0}, o.dtype(at::kInt));
  Tensor amax = m.mx ? at::empty({N, K}, o.dtype(at::kInt)) : at::empty({0}, o.dtype(at::kInt));
  Tensor part = hub_partial(*plan, x, [&](int64_t n) { return a.ggl_segment_multi_partial_bytes(n, K, m.codes.data(), (int)A); });
  ggl_segplan_t cs = plan->c(part);
  check(a, a.ggl_segment_multi_fwd(ptr_or_null<float>(x), &cs, K, C, m.codes.data(), (int)A, empty_zero ? 1 : 0,
                                   ptr_or_null<float>(out), ptr_or_null<float>(mean), ptr_or_null<int32_t>(amin),
                                   ptr_or_null<int32_t>(amax), stream_of(dev)));
  return {out, mean, amin, amax};
}

static Tensor multi_backward_kernel(const Tensor &grad, const Tensor &x_, const Tensor &out, const Tensor &mean, const Tensor &amin,
                                    const Tensor &amax, const Tensor &index, int64_t N, c10::IntArrayRef aggs, int64_t C) {
  same_device({&grad, &index});
  const MultiAggs m = multi_aggs(aggs);
  const auto dev = grad.device();
  c10::OptionalDeviceGuard guard(dev);
  const Api &a = api_for(dev);
  Tensor g = grad.contiguous(), x = x_.contiguous();
  f32("grad", g);
  const int64_t A = static_cast<int64_t>(m.codes.size());
  TORCH_CHECK(g.dim() == 2 && g.size(0) == N && g.size(1) % A == 0, "segment_multi backward: grad must be [N, A * K]");
  const int64_t K = g.size(1) / A;
  auto plan = seg_plan(index, N);    // (the forward's plan: a cache hit)
  Tensor gx = at::empty({plan->E, K}, g.options());
  ggl_segplan_t cs = plan->c(Tensor());
  check(a, a.ggl_segment_multi_bwd(ptr_or_null<float>(g), ptr_or_null<float>(x), ptr_or_null<float>(out), ptr_or_null<float>(mean),
                                   ptr_or_null<int32_t>(amin), ptr_or_null<int32_t>(amax), &cs, K, C, m.codes.data(), (int)A,
                                   ptr_or_null<float>(gx), stream_of(dev)));
  return gx;
}

using MultiFwdSig = std::tuple<Tensor, Tensor, Tensor, Tensor>(const Tensor &, const Tensor &, int64_t, c10::IntArrayRef, int64_t,
                                                               bool, bool);
using MultiBwdSig = Tensor(const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                           const Tensor &, int64_t, c10::IntArrayRef, int64_t);
// saves only what the requested statistics' backward reads: x and mean for var / std, out for std, the witnesses for min / max
struct MultiFn : public torch::autograd::Function<MultiFn> {
  static Tensor forward(AutogradContext *ctx, const Tensor &x, const Tensor &index, int64_t N, std::vector<int64_t> aggs, int64_t C,
                        bool empty_zero) {
    at::AutoDispatchBelowADInplaceOrView below;
    static auto op = op_handle<MultiFwdSig>("ggl_agg::segment_multi_forward");
    const MultiAggs m = multi_aggs(aggs);
    const bool need = x.requires_grad();
    Tensor out, mean, amin, amax;
    std::tie(out, mean, amin, amax) = op.call(x, index, N, aggs, C, empty_zero, need);
    if (need) {
      Tensor none = at::empty({0}, x.options());
      ctx->save_for_backward({m.sq ? x : none, m.sd ? out : none, mean, amin, amax, index});
    }
    ctx->saved_data["N"] = N;
    ctx->saved_data["C"] = C;
    ctx->saved_data["aggs"] = aggs;
    return out;
  }
  static variable_list backward(AutogradContext *ctx, variable_list grads) {
    auto s = ctx->get_saved_variables();
    static auto op = op_handle<MultiBwdSig>("ggl_agg::segment_multi_backward");
    auto aggs = ctx->saved_data["aggs"].toIntVector();
    Tensor gx = op.call(grads[0], s[0], s[1], s[2], s[3], s[4], s[5], ctx->saved_data["N"].toInt(), aggs,
                        ctx->saved_data["C"].toInt());
    return {gx, Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};
static Tensor multi_autograd(const Tensor &x, const Tensor &index, int64_t N, c10::IntArrayRef aggs, int64_t C, bool empty_zero) {
  multi_check(x, index, C);
  multi_aggs(aggs);
  return MultiFn::apply(x, index, N, aggs.vec(), C, empty_zero);
}
static std::tuple<Tensor, Tensor, Tensor, Tensor> multi_fwd_meta(const Tensor &x, const Tensor &, int64_t N, c10::IntArrayRef aggs,
                                                                 int64_t, bool, bool want_mean) {
  const MultiAggs m = multi_aggs(aggs);
  auto o = x.options(), i = x.options().dtype(at::kInt);
  const int64_t K = x.size(1);
  return {at::empty({N, static_cast<int64_t>(aggs.size()) * K}, o), want_mean && m.sq ? at::empty({N, K}, o) : at::empty({0}, o),
          m.mn ? at::empty({N, K}, i) : at::empty({0}, i), m.mx ? at::empty({N, K}, i) : at::empty({0}, i)};
}
static Tensor multi_bwd_meta(const Tensor &grad, const Tensor &, const Tensor &, const Tensor &, const Tensor &, const Tensor &,
                             const Tensor &index, int64_t, c10::IntArrayRef aggs, int64_t) {
  return at::empty({index.size(0), grad.size(1) / static_cast<int64_t>(aggs.size())}, grad.options());
}
static Tensor multi_meta(const Tensor &x, const Tensor &, int64_t N, c10::IntArrayRef aggs, int64_t, bool) {
  return at::empty({N, static_cast<int64_t>(aggs.size()) * x.size(1)}, x.options());
}

}  // namespace ggl_torch

TORCH_LIBRARY(ggl, m) {
  m.def("segment_sum(Tensor x, Tensor index, int N) -> Tensor");
  m.def("segment_mean(Tensor x, Tensor index, int N) -> Tensor");
  m.def("segment_max(Tensor x, Tensor index, int N) -> (Tensor, Tensor)");
  m.def("segment_softmax(Tensor x, Tensor index, int N) -> Tensor");
  m.def("segment_softmax_backward(Tensor grad, Tensor y, Tensor index, int N) -> Tensor");
  m.def("spmm_sum(Tensor index, Tensor? weight, Tensor x) -> Tensor");
  m.def("spmm_mean(Tensor index, Tensor? weight, Tensor x) -> Tensor");
  m.def("spmm_max(Tensor index, Tensor? weight, Tensor x) -> Tensor");
  m.def("bspmm_sum(Tensor index, Tensor weight, Tensor x) -> Tensor");
  // not in the reference: rows stored as f16 / bf16, summed in f32; out_f32 keeps the f32 sums (a last layer's logits)
  m.def("spmm_sum_x16(Tensor index, Tensor? weight, Tensor x, bool out_f32=False) -> Tensor");
  m.def("spmm_mean_x16(Tensor index, Tensor? weight, Tensor x, bool out_f32=False) -> Tensor");
  // backward passes and the arg-returning max (what the autograd formulas call; usable on their own)
  m.def("segment_sum_backward(Tensor grad, Tensor index, int[] x_shape) -> Tensor");
  m.def("segment_mean_backward(Tensor grad, Tensor index, int N, int[] x_shape) -> Tensor");
  m.def("segment_max_backward(Tensor grad, Tensor arg, int[] x_shape) -> Tensor");
  m.def("spmm_sum_backward(Tensor index, Tensor? weight, Tensor grad) -> Tensor");
  m.def("spmm_mean_backward(Tensor index, Tensor? weight, Tensor grad) -> Tensor");
  m.def("spmm_max_arg(Tensor index, Tensor? weight, Tensor x) -> (Tensor, Tensor)");
  m.def("spmm_max_backward(Tensor index, Tensor? weight, Tensor grad, Tensor arg) -> Tensor");
  m.def("bspmm_sum_backward(Tensor index, Tensor weight, Tensor x, Tensor grad) -> (Tensor, Tensor)");
  // the fused route: edge-softmax + aggregate (COO edge list / the caller's CSR = dgNN's GATConvFuse), the layer epilogue
  // alone and inside the aggregate's store, one static-shape sampler hop
  m.def("gat_fused(Tensor index, Tensor el, Tensor er, Tensor x, float negative_slope=0.2, int? num_nodes=None, "
        "float dropout_rate=0.0) -> Tensor");
  m.def("gat_fused_forward(Tensor index, Tensor el, Tensor er, Tensor x, float negative_slope, int num_nodes, "
        "float dropout_rate) -> (Tensor, Tensor, Tensor, Tensor, bool)");
  m.def("gat_fused_backward(Tensor index, Tensor el, Tensor er, Tensor x, Tensor grad, Tensor out, Tensor rowmax, "
        "Tensor rowden, Tensor rng_used, float negative_slope, int num_nodes, float dropout_rate, bool fast) -> "
        "(Tensor, Tensor, Tensor)");
  // not in the reference: x stored as f16 / bf16 (the ops above take such rows too and return x's dtype); out_f32 keeps
  // the f32 result
  m.def("gat_fused_x16(Tensor index, Tensor el, Tensor er, Tensor x, float negative_slope=0.2, int? num_nodes=None, "
        "float dropout_rate=0.0, bool out_f32=False) -> Tensor");
  m.def("gat_fused_x16_forward(Tensor index, Tensor el, Tensor er, Tensor x, float negative_slope, int num_nodes, "
        "float dropout_rate, bool out_f32) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("gat_fused_csr(Tensor row_ptr, Tensor col_ind, Tensor col_ptr, Tensor row_ind, Tensor permute, Tensor el, "
        "Tensor er, Tensor x, float negative_slope=0.2, float dropout_rate=0.0) -> Tensor");
  m.def("gat_fused_csr_forward(Tensor row_ptr, Tensor col_ind, Tensor col_ptr, Tensor row_ind, Tensor permute, Tensor el, "
        "Tensor er, Tensor x, float negative_slope, float dropout_rate) -> (Tensor, Tensor, Tensor, Tensor, bool)");
  m.def("gat_fused_csr_backward(Tensor row_ptr, Tensor col_ind, Tensor col_ptr, Tensor row_ind, Tensor permute, Tensor el, "
        "Tensor er, Tensor x, Tensor grad, Tensor out, Tensor rowmax, Tensor rowden, Tensor rng_used, float negative_slope, "
        "float dropout_rate, bool fast) -> (Tensor, Tensor, Tensor)");
  m.def("bias_act(Tensor a, Tensor? bias, bool relu, float p_drop) -> Tensor");
  m.def("bias_act_forward(Tensor a, Tensor? bias, bool relu, float p_drop) -> (Tensor, Tensor)");
  m.def("bias_act_backward(Tensor grad, Tensor y, bool has_bias, bool relu, float p_drop, Tensor rng_used) -> (Tensor, Tensor)");
  m.def("spmm_epi(Tensor index, Tensor? weight, Tensor x, bool mean=False, Tensor? add=None, Tensor? bias=None, "
        "bool relu=False, float p_drop=0.0) -> Tensor");
  m.def("spmm_epi_forward(Tensor index, Tensor? weight, Tensor x, bool mean, Tensor? add, Tensor? bias, bool relu, "
        "float p_drop) -> (Tensor, Tensor)");
  // (A x + bias)[rows] on the rows alone: rows = a sorted, duplicate-free int64 list of destination rows; K % 4 == 0
  m.def("spmm_rows(Tensor index, Tensor? weight, Tensor x, Tensor rows, Tensor? bias=None) -> Tensor");
  m.def("spmm_rows_forward(Tensor index, Tensor? weight, Tensor x, Tensor rows, Tensor? bias) -> Tensor");
  m.def("spmm_rows_backward(Tensor index, Tensor? weight, Tensor grad, Tensor rows, int n_src, bool has_bias) -> (Tensor, Tensor)");
  m.def("segment_epi(Tensor x, Tensor index, int N, bool mean=True, Tensor? add=None, Tensor? bias=None, bool relu=False) -> Tensor");
  m.def("segment_epi_forward(Tensor x, Tensor index, int N, bool mean, Tensor? add, Tensor? bias, bool relu) -> Tensor");
  m.def("sample_hop(Tensor rowptr, Tensor col, Tensor seeds, Tensor n_seeds, int num_nodes, int fanout, int e_cap, int s_cap, "
        "Tensor(a!) first_pos) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("reseed() -> ()", ggl_torch::reseed);
  m.def("clear_caches() -> ()", ggl_torch::clear_caches);
  m.def("plan_stats() -> int[]", ggl_torch::plan_stats);
}

#define GGL_BACKEND(KEY)                                     \
  TORCH_LIBRARY_IMPL(ggl, KEY, m) {                          \
    m.impl("segment_sum", ggl_torch::segment_sum_kernel);    \
    m.impl("segment_mean", ggl_torch::segment_mean_kernel);  \
    m.impl("segment_max", ggl_torch::segment_max_kernel);    \
    m.impl("segment_softmax", ggl_torch::segment_softmax_kernel);                    \
    m.impl("segment_softmax_backward", ggl_torch::segment_softmax_backward_kernel);  \
    m.impl("spmm_sum", ggl_torch::spmm_sum_kernel);          \
    m.impl("spmm_mean", ggl_torch::spmm_mean_kernel);        \
    m.impl("spmm_max", ggl_torch::spmm_max_kernel);          \
    m.impl("bspmm_sum", ggl_torch::bspmm_sum_kernel);        \
    m.impl("spmm_sum_x16", ggl_torch::spmm_sum_x16_kernel);  \
    m.impl("spmm_mean_x16", ggl_torch::spmm_mean_x16_kernel); \
    m.impl("segment_sum_backward", ggl_torch::segment_sum_backward_kernel);    \
    m.impl("segment_mean_backward", ggl_torch::segment_mean_backward_kernel);  \
    m.impl("segment_max_backward", ggl_torch::segment_max_backward_kernel);    \
    m.impl("spmm_sum_backward", ggl_torch::spmm_sum_backward_kernel);          \
    m.impl("spmm_mean_backward", ggl_torch::spmm_mean_backward_kernel);        \
    m.impl("spmm_max_arg", ggl_torch::spmm_max_arg_kernel);                    \
    m.impl("spmm_max_backward", ggl_torch::spmm_max_backward_kernel);          \
    m.impl("bspmm_sum_backward", ggl_torch::bspmm_sum_backward_kernel);        \
    m.impl("gat_fused_forward", ggl_torch::gat_fused_forward_kernel);          \
    m.impl("gat_fused_backward", ggl_torch::gat_fused_backward_kernel);        \
    m.impl("gat_fused_x16_forward", ggl_torch::gat_x16_forward_kernel);        \
    m.impl("gat_fused_csr_forward", ggl_torch::gat_csr_forward_kernel);        \
    m.impl("gat_fused_csr_backward", ggl_torch::gat_csr_backward_kernel);      \
    m.impl("bias_act_forward", ggl_torch::bias_act_forward_kernel);            \
    m.impl("bias_act_backward", ggl_torch::bias_act_backward_kernel);          \
    m.impl("spmm_epi_forward", ggl_torch::spmm_epi_forward_kernel);            \
    m.impl("segment_epi_forward", ggl_torch::segment_epi_forward_kernel);      \
    m.impl("spmm_rows_forward", ggl_torch::spmm_rows_forward_kernel);          \
    m.impl("spmm_rows_backward", ggl_torch::spmm_rows_backward_kernel);        \
    m.impl("sample_hop", ggl_torch::sample_hop_kernel);                        \
  }
GGL_BACKEND(CPU)
GGL_BACKEND(CUDA)

TORCH_LIBRARY_IMPL(ggl, Autograd, m) {
  m.impl("segment_sum", ggl_torch::segment_sum_autograd);
  m.impl("segment_mean", ggl_torch::segment_mean_autograd);
  m.impl("segment_max", ggl_torch::segment_max_autograd);
  m.impl("segment_softmax", ggl_torch::segment_softmax_autograd);
  m.impl("spmm_sum", ggl_torch::spmm_sum_autograd);
  m.impl("spmm_mean", ggl_torch::spmm_mean_autograd);
  m.impl("spmm_max", ggl_torch::spmm_max_autograd);
  m.impl("bspmm_sum", ggl_torch::bspmm_sum_autograd);
  m.impl("spmm_sum_x16", ggl_torch::spmm_sum_x16_autograd);
  m.impl("spmm_mean_x16", ggl_torch::spmm_mean_x16_autograd);
  m.impl("gat_fused", ggl_torch::gat_fused_autograd);
  m.impl("gat_fused_x16", ggl_torch::gat_fused_x16_autograd);
  m.impl("gat_fused_csr", ggl_torch::gat_fused_csr_autograd);
  m.impl("bias_act", ggl_torch::bias_act_autograd);
  m.impl("spmm_epi", ggl_torch::spmm_epi_autograd);
  m.impl("segment_epi", ggl_torch::segment_epi_autograd);
  m.impl("spmm_rows", ggl_torch::spmm_rows_autograd);
}

TORCH_LIBRARY_IMPL(ggl, Meta, m) {
  m.impl("segment_sum", ggl_torch::seg_meta);
  m.impl("segment_mean", ggl_torch::seg_meta);
  m.impl("segment_max", ggl_torch::seg_max_meta);
  m.impl("segment_softmax", ggl_torch::softmax_meta);
  m.impl("segment_softmax_backward", ggl_torch::softmax_bwd_meta);
  m.impl("spmm_sum", ggl_torch::like_x_meta);
  m.impl("spmm_mean", ggl_torch::like_x_meta);
  m.impl("spmm_max", ggl_torch::like_x_meta);
  m.impl("bspmm_sum", ggl_torch::bspmm_meta);
  m.impl("spmm_sum_x16", ggl_torch::x16_meta);
  m.impl("spmm_mean_x16", ggl_torch::x16_meta);
  m.impl("segment_sum_backward", ggl_torch::seg_bwd_meta);
  m.impl("segment_mean_backward", ggl_torch::seg_mean_bwd_meta);
  m.impl("segment_max_backward", ggl_torch::seg_bwd_meta);
  m.impl("spmm_sum_backward", ggl_torch::like_x_meta);
  m.impl("spmm_mean_backward", ggl_torch::like_x_meta);
  m.impl("spmm_max_arg", ggl_torch::spmm_max_arg_meta);
  m.impl("spmm_max_backward", ggl_torch::spmm_max_bwd_meta);
  m.impl("bspmm_sum_backward", ggl_torch::bspmm_bwd_meta);
  m.impl("gat_fused", ggl_torch::gat_meta);
  m.impl("gat_fused_forward", ggl_torch::gat_fwd_meta);
  m.impl("gat_fused_x16", ggl_torch::gat_x16_meta);
  m.impl("gat_fused_x16_forward", ggl_torch::gat_x16_fwd_meta);
  m.impl("gat_fused_backward", ggl_torch::gat_bwd_meta);
  m.impl("gat_fused_csr", ggl_torch::gat_csr_meta);
  m.impl("gat_fused_csr_forward", ggl_torch::gat_csr_fwd_meta);
  m.impl("gat_fused_csr_backward", ggl_torch::gat_csr_bwd_meta);
  m.impl("bias_act", ggl_torch::bias_meta);
  m.impl("bias_act_forward", ggl_torch::bias_fwd_meta);
  m.impl("bias_act_backward", ggl_torch::bias_bwd_meta);
  m.impl("spmm_epi", ggl_torch::epi_meta);
  m.impl("spmm_epi_forward", ggl_torch::epi_fwd_meta);
  m.impl("segment_epi", ggl_torch::seg_epi_meta);
  m.impl("spmm_rows", ggl_torch::rows_meta);
  m.impl("spmm_rows_forward", ggl_torch::rows_meta);
  m.impl("spmm_rows_backward", ggl_torch::rows_bwd_meta);
  m.impl("segment_epi_forward", ggl_torch::seg_epi_meta);
}

// gspmm's weight gradient as a dispatcher op.  It lives in a namespace of its own: the operator surface under ggl:: is
// pinned name by name (tests/golden/ggl_schemas.txt), and the autograd formulas of spmm_sum / spmm_mean / spmm_*_x16 /
// spmm_epi above need an OP to call so that their backward traces under FakeTensor like the others.
// linear_bias_act_backward — bias_act_backward under a Linear, the [N, K] product formed in registers — lives here for the same
// reason.
TORCH_LIBRARY(ggl_grad, m) {
  m.def("spmm_grad_w(Tensor index, Tensor x, Tensor grad, bool mean) -> Tensor");
  m.def("linear_bias_act_backward(Tensor grad, Tensor weight, Tensor y, bool has_bias, bool relu, float p_drop, Tensor rng_used) "
        "-> (Tensor, Tensor)");
}
TORCH_LIBRARY_IMPL(ggl_grad, CPU, m) {
  m.impl("spmm_grad_w", ggl_torch::spmm_grad_w_kernel);
  m.impl("linear_bias_act_backward", ggl_torch::linear_bias_act_backward_kernel);
}
TORCH_LIBRARY_IMPL(ggl_grad, CUDA, m) {
  m.impl("spmm_grad_w", ggl_torch::spmm_grad_w_kernel);
  m.impl("linear_bias_act_backward", ggl_torch::linear_bias_act_backward_kernel);
}
TORCH_LIBRARY_IMPL(ggl_grad, Meta, m) {
  m.impl("spmm_grad_w", ggl_torch::spmm_grad_w_meta);
  m.impl("linear_bias_act_backward", ggl_torch::lin_bias_bwd_meta);
}

// Edge softmax + aggregate on per-edge logits, a namespace of its own for the same reason: the ggl:: surface is pinned.
TORCH_LIBRARY(ggl_attn, m) {
  m.def("edge_softmax_aggregate(Tensor index, Tensor logits, Tensor x, int? num_nodes=None, float dropout_rate=0.) -> Tensor");
  m.def("edge_softmax_aggregate_forward(Tensor index, Tensor logits, Tensor x, int num_nodes, float dropout_rate) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("edge_softmax_aggregate_backward(Tensor index, Tensor logits, Tensor x, Tensor grad, Tensor out, Tensor rowmax, "
        "Tensor rowden, Tensor rng_used, int num_nodes, float dropout_rate, bool need_logits, bool need_x) -> (Tensor, Tensor)");
  m.def("dot_attention(Tensor index, Tensor q, Tensor k, Tensor v, int? num_nodes=None, float? scale=None, "
        "float dropout_rate=0.) -> Tensor");
  m.def("dot_attention_forward(Tensor index, Tensor q, Tensor k, Tensor v, int num_nodes, float scale, float dropout_rate, "
        "bool keep_logits) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("dot_attention_backward(Tensor index, Tensor q, Tensor k, Tensor v, Tensor logits, Tensor grad, Tensor out, "
        "Tensor rowmax, Tensor rowden, Tensor rng_used, int num_nodes, float scale, float dropout_rate, bool need_q, "
        "bool need_k, bool need_v) -> (Tensor, Tensor, Tensor)");
  m.def("gatv2_attention(Tensor index, Tensor xl, Tensor xr, Tensor att, int? num_nodes=None, float negative_slope=0.2, "
        "float dropout_rate=0.) -> Tensor");
  m.def("gatv2_attention_forward(Tensor index, Tensor xl, Tensor xr, Tensor att, int num_nodes, float negative_slope, "
        "float dropout_rate, bool keep_logits) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("gatv2_attention_backward(Tensor index, Tensor xl, Tensor xr, Tensor att, Tensor logits, Tensor grad, Tensor out, "
        "Tensor rowmax, Tensor rowden, Tensor rng_used, int num_nodes, float negative_slope, float dropout_rate, bool need_xl, "
        "bool need_xr, bool need_att) -> (Tensor, Tensor, Tensor)");
}
#define GGL_ATTN_IMPL(KEY)                                                                          \
  TORCH_LIBRARY_IMPL(ggl_attn, KEY, m) {                                                            \
    m.impl("edge_softmax_aggregate_forward", ggl_torch::esa_forward_kernel);                        \
    m.impl("edge_softmax_aggregate_backward", ggl_torch::esa_backward_kernel);                      \
    m.impl("dot_attention_forward", ggl_torch::dot_forward_kernel);                                 \
    m.impl("dot_attention_backward", ggl_torch::dot_backward_kernel);                               \
    m.impl("gatv2_attention_forward", ggl_torch::gatv2_forward_kernel);                             \
    m.impl("gatv2_attention_backward", ggl_torch::gatv2_backward_kernel);                           \
  }
GGL_ATTN_IMPL(CPU)
GGL_ATTN_IMPL(CUDA)
#undef GGL_ATTN_IMPL
TORCH_LIBRARY_IMPL(ggl_attn, Autograd, m) {
  m.impl("edge_softmax_aggregate", ggl_torch::esa_autograd);
  m.impl("dot_attention", ggl_torch::dot_autograd);
  m.impl("gatv2_attention", ggl_torch::gatv2_autograd);
}
TORCH_LIBRARY_IMPL(ggl_attn, Meta, m) {
  m.impl("edge_softmax_aggregate", ggl_torch::esa_meta);
  m.impl("edge_softmax_aggregate_forward", ggl_torch::esa_fwd_meta);
  m.impl("edge_softmax_aggregate_backward", ggl_torch::esa_bwd_meta);
  m.impl("dot_attention", ggl_torch::dot_meta);
  m.impl("dot_attention_forward", ggl_torch::logit_attn_fwd_meta);
  m.impl("dot_attention_backward", ggl_torch::logit_attn_bwd_meta);
  m.impl("gatv2_attention", ggl_torch::gatv2_meta);
  m.impl("gatv2_attention_forward", ggl_torch::logit_attn_fwd_meta);
  m.impl("gatv2_attention_backward", ggl_torch::logit_attn_bwd_meta);
}

// Several statistics of the same rows in one walk, a namespace of its own for the same reason: the ggl:: surface is pinned.
TORCH_LIBRARY(ggl_agg, m) {
  m.def("segment_multi(Tensor x, Tensor index, int N, int[] aggs, int C, bool empty_zero=False) -> Tensor");
  m.def("segment_multi_forward(Tensor x, Tensor index, int N, int[] aggs, int C, bool empty_zero, bool want_mean) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  m.def("segment_multi_backward(Tensor grad, Tensor x, Tensor out, Tensor mean, Tensor argmin, Tensor argmax, Tensor index, "
        "int N, int[] aggs, int C) -> Tensor");
}
#define GGL_AGG_IMPL(KEY)                                                                           \
  TORCH_LIBRARY_IMPL(ggl_agg, KEY, m) {                                                             \
    m.impl("segment_multi_forward", ggl_torch::multi_forward_kernel);                               \
    m.impl("segment_multi_backward", ggl_torch::multi_backward_kernel);                             \
  }
GGL_AGG_IMPL(CPU)
GGL_AGG_IMPL(CUDA)
#undef GGL_AGG_IMPL
TORCH_LIBRARY_IMPL(ggl_agg, Autograd, m) { m.impl("segment_multi", ggl_torch::multi_autograd); }
TORCH_LIBRARY_IMPL(ggl_agg, Meta, m) {
  m.impl("segment_multi", ggl_torch::multi_meta);
  m.impl("segment_multi_forward", ggl_torch::multi_fwd_meta);
  m.impl("segment_multi_backward", ggl_torch::multi_bwd_meta);
}
