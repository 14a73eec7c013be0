// Bindings of the multi-tensor update kernels (multi_tensor.hip). The tables
// are device tensors owned by a MultiTensorPlan (ops/mt_plan.py): nothing is
// built or uploaded per call.

#include "binding_util.h"
#include "multi_tensor.h"

namespace {

using bf16 = __hip_bfloat16;

// The tables of a plan, checked. `ptrs` holds n_lists pointer tables of
// n_tensors raw addresses each, which is why list() casts: the element type
// behind them is the caller's word (is_bf16, grad_is_f32).
struct PlanTables {
  const long* ptrs;
  const long* sizes;
  const int* ct;
  const long* co;
  long n_tensors;
  int n_chunks;

  PlanTables(const torch::Tensor& ptrs_, const torch::Tensor& sizes_, const torch::Tensor& ct_,
             const torch::Tensor& co_, long n_lists, const char* who)
      : ptrs(in_ptr<long>(ptrs_, "ptrs")), sizes(in_ptr<long>(sizes_, "sizes")),
        ct(in_ptr<int>(ct_, "ct")), co(in_ptr<long>(co_, "co")), n_tensors(sizes_.numel()),
        n_chunks((int)ct_.numel()) {
    TORCH_CHECK(ptrs_.numel() == n_lists * n_tensors, who, ": ptrs must hold ", n_lists,
                " lists of ", n_tensors, " addresses, got ", ptrs_.numel());
    TORCH_CHECK(ct_.numel() == co_.numel(), who, ": ct and co must have one length");
  }
  template <typename T>
  T* const* list(int l) const {
    return reinterpret_cast<T* const*>(ptrs + l * n_tensors);
  }
  // a per-tensor table such as lr_mult
  template <typename T>
  const T* per_tensor(const torch::Tensor& x, const char* who) const {
    TORCH_CHECK(x.numel() == n_tensors, who, " must have one entry per tensor");
    return in_ptr<T>(x, who);
  }
};

at::ScalarType plan_dtype(bool is_bf16) {
  return is_bf16 ? at::ScalarType::BFloat16 : at::ScalarType::Float;
}

// (param dtype, grad dtype) pairs the AdamW kernel is instantiated for
#define DISPATCH_MT_PAIR(is_bf16, grad_is_f32, ...) \
  [&] {                                             \
    if (!(is_bf16)) {                               \
      using param_t = float;                        \
      using grad_t = float;                         \
      return __VA_ARGS__();                         \
    } else if (grad_is_f32) {                       \
      using param_t = bf16;                         \
      using grad_t = float;                         \
      return __VA_ARGS__();                         \
    } else {                                        \
      using param_t = bf16;                         \
      using grad_t = bf16;                          \
      return __VA_ARGS__();                         \
    }                                               \
  }()

void multi_tensor_ema_planned(torch::Tensor ptrs, torch::Tensor sizes, torch::Tensor ct,
                              torch::Tensor co, int64_t n_tensors, double m,
                              bool is_bf16) {
  const PlanTables p(ptrs, sizes, ct, co, 2, "multi_tensor_ema_planned");
  TORCH_CHECK(n_tensors == p.n_tensors, "multi_tensor_ema_planned: sizes must have n_tensors entries");
  if (p.n_chunks == 0) return;
  DISPATCH_FLOAT_BF16(plan_dtype(is_bf16), "multi_tensor_ema_planned", [&] {
    launch_multi_tensor_ema<scalar_t>(p.list<scalar_t>(0), p.list<const scalar_t>(1), p.sizes,
                                      p.ct, p.co, p.n_chunks, (float)m, current_stream());
  });
}

void multi_tensor_adamw_planned(torch::Tensor ptrs, torch::Tensor sizes, torch::Tensor ct,
                                torch::Tensor co, int64_t n_tensors, torch::Tensor lr_mult,
                                torch::Tensor wd_mult, torch::Tensor is_last,
                                torch::Tensor sub_id, torch::Tensor clip, double lr,
                                double last_lr, double wd, double beta1, double beta2,
                                double eps, double bc1, double bc2, bool has_master,
                                bool is_bf16, bool grad_is_f32) {
  const PlanTables p(ptrs, sizes, ct, co, has_master ? 5 : 4, "multi_tensor_adamw_planned");
  TORCH_CHECK(n_tensors == p.n_tensors, "multi_tensor_adamw_planned: sizes must have n_tensors entries");
  TORCH_CHECK(is_bf16 || grad_is_f32, "multi_tensor_adamw_planned: fp32 params take fp32 grads");
  const float* lr_mult_p = p.per_tensor<float>(lr_mult, "lr_mult");
  const float* wd_mult_p = p.per_tensor<float>(wd_mult, "wd_mult");
  const float* is_last_p = p.per_tensor<float>(is_last, "is_last");
  const int* sub_id_p = p.per_tensor<int>(sub_id, "sub_id");
  const float* clip_p = IN_PTR(float, clip);
  if (p.n_chunks == 0) return;
  DISPATCH_MT_PAIR(is_bf16, grad_is_f32, [&] {
    launch_multi_tensor_adamw_planned<param_t, grad_t>(
        p.list<param_t>(0), p.list<const grad_t>(1), p.list<float>(2), p.list<float>(3),
        has_master ? p.list<float>(4) : nullptr, p.sizes, p.ct, p.co, p.n_chunks, lr_mult_p,
        wd_mult_p, is_last_p, sub_id_p, clip_p, (float)lr, (float)last_lr, (float)wd,
        (float)beta1, (float)beta2, (float)eps, (float)bc1, (float)bc2, has_master,
        current_stream());
  });
}

torch::Tensor multi_tensor_l2norm_planned(torch::Tensor ptrs, torch::Tensor sizes,
                                          torch::Tensor ct, torch::Tensor co,
                                          torch::Tensor sub_id, int64_t n_submodels,
                                          bool is_bf16) {
  const PlanTables p(ptrs, sizes, ct, co, 1, "multi_tensor_l2norm_planned");
  const int* sub_id_p = p.per_tensor<int>(sub_id, "sub_id");
  auto out = torch::zeros({n_submodels}, torch::dtype(torch::kFloat).device(ptrs.device()));
  if (p.n_chunks == 0) return out;
  DISPATCH_FLOAT_BF16(plan_dtype(is_bf16), "multi_tensor_l2norm_planned", [&] {
    launch_multi_tensor_l2norm_planned<scalar_t>(p.list<const scalar_t>(0), p.sizes, p.ct, p.co,
                                                 p.n_chunks, sub_id_p, OUT_PTR(float, out),
                                                 current_stream());
  });
  return out;
}

}  // namespace

void register_multi_tensor(pybind11::module_& mod) {
  mod.def("multi_tensor_ema_planned", &multi_tensor_ema_planned);
  mod.def("multi_tensor_adamw_planned", &multi_tensor_adamw_planned);
  mod.def("multi_tensor_l2norm_planned", &multi_tensor_l2norm_planned);
  mod.attr("MT_CHUNK") = MT_CHUNK;
}
