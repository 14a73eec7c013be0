// PyTorch bindings for the dinov3_amd CDNA4 kernel library.
// Compiled by hipcc (PYTORCH_ROCM_ARCH=gfx950) into dinov3_amd/ops/_hip_ops.so.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <vector>

#include "common.h"  // COLRED_MAX_PARTIALS
#include "fmha_rope.h"  // attention layouts and launchers, launch_probe_mfma

#define CHECK_INPUT(x) \
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), #x " must be a contiguous HIP tensor")

// ---- extern launchers (defined in the .hip kernel TUs) ----
template <typename T>
void launch_layernorm_fwd(const T*, const T*, const T*, T*, float*, float*, long, int,
                          float, hipStream_t);
template <typename T>
void launch_layernorm_bwd(const T*, const T*, const T*, const float*, const float*, T*,
                          float*, T*, T*, long, int, hipStream_t);
template <typename T>
void launch_gather_layernorm_fwd(const T*, const long*, const T*, const T*, T*, T*, float*,
                                 float*, long, int, float, hipStream_t);
template <typename T>
void launch_layernorm_bwd_scatter_acc(const T*, const T*, const T*, const float*,
                                      const float*, T*, const long*, float*, T*, T*, long,
                                      int, hipStream_t);
template <typename T>
void launch_rmsnorm_fwd(const T*, const T*, T*, float*, long, int, float, hipStream_t);
template <typename T>
void launch_rmsnorm_bwd(const T*, const T*, const T*, const float*, T*, float*, T*, long,
                        int, hipStream_t);
template <typename T>
void launch_l2norm_fwd(const T*, T*, float*, long, int, float, hipStream_t);
template <typename T>
void launch_l2norm_bwd(const T*, const T*, const float*, T*, long, int, float, hipStream_t);
template <typename T>
void launch_bias_gelu_fwd(const T*, const T*, T*, long, int, hipStream_t);
template <typename T>
void launch_bias_gelu_bwd(const T*, const T*, const T*, T*, float*, T*, long, int,
                          hipStream_t);
template <typename T>
void launch_ls_axpy_fwd(const T*, const T*, const T*, T*, long, int, hipStream_t);
template <typename T>
void launch_ls_axpy_bwd(const T*, const T*, const T*, T*, float*, T*, long, int,
                        hipStream_t);
template <typename T>
void launch_ls_axpy_bias_fwd(const T*, const T*, const T*, const T*, T*, long, int,
                             hipStream_t);
template <typename T>
void launch_ls_axpy_bias_bwd(const T*, const T*, const T*, const T*, T*, float*, T*, T*,
                             long, int, hipStream_t);
template <typename T>
void launch_ls_scatter_add(T*, const long*, const T*, const T*, const T*, const float*,
                           long, int, hipStream_t);
template <typename T>
void launch_ls_scatter_bwd(const T*, const long*, const T*, const T*, const T*,
                           const float*, T*, float*, T*, T*, long, int, hipStream_t);
template <typename T>
void launch_row_gather(const T*, const long*, T*, long, int, hipStream_t);
template <typename T>
void launch_row_scatter_add(T*, const long*, const T*, const float*, long, int,
                            hipStream_t);
template <typename T>
void launch_row_gather_scaled(const T*, const long*, const float*, T*, long, int,
                              hipStream_t);
template <typename T>
void launch_swiglu_fwd(const T*, T*, long, int, hipStream_t);
template <typename T>
void launch_swiglu_bwd(const T*, const T*, T*, long, int, hipStream_t);
template <typename T>
void launch_rope_fwd(const T*, const float*, const float*, T*, long, int, int, int,
                     hipStream_t);
void launch_dino_ce_fwd(const __hip_bfloat16*, const float*, float*, float*, float*, int,
                        int, int, long, float, bool, hipStream_t);
void launch_dino_ce_bwd(const __hip_bfloat16*, const float*, const float*, const float*,
                        const float*, __hip_bfloat16*, int, int, int, long, float, bool,
                        hipStream_t);
void launch_ibot_ce_fwd(const __hip_bfloat16*, const float*, const float*, float*, float*,
                        float*, int, long, float, hipStream_t);
void launch_ibot_ce_bwd(const __hip_bfloat16*, const float*, const float*, const float*,
                        const float*, const float*, __hip_bfloat16*, int, long, float,
                        hipStream_t);
void launch_sinkhorn_exp(const __hip_bfloat16*, float*, float*, long, float, hipStream_t);
void launch_sinkhorn_fact_colsum(const __hip_bfloat16*, const float*, float*, int, long,
                                 float, hipStream_t);
void launch_sinkhorn_fact_rowsum(const __hip_bfloat16*, const float*, float*, int, long,
                                 float, hipStream_t);
void launch_ibot_ce_fact_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                             const float*, const float*, float*, float*, float*, int,
                             long, float, float, hipStream_t);
void launch_ibot_ce_fact_bwd(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                             const float*, const float*, const float*, const float*,
                             const float*, __hip_bfloat16*, int, long, float, float,
                             hipStream_t);
void launch_dino_ce_fact_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                             const float*, float*, float*, float*, int, int, int, long,
                             float, float, bool, hipStream_t);
void launch_dino_ce_fact_bwd(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                             const float*, const float*, const float*, const float*,
                             __hip_bfloat16*, int, int, int, long, float, float, bool,
                             hipStream_t);
void launch_sinkhorn_colsum(const float*, float*, int, long, const float*, hipStream_t);
void launch_sinkhorn_div_row(float*, const float*, int, long, float, const float*, bool,
                             hipStream_t);
void launch_patch_embed_fwd(const __hip_bfloat16*, const __hip_bfloat16*,
                            const __hip_bfloat16*, __hip_bfloat16*, int, int, int, int,
                            int, int, hipStream_t);
void launch_fp8_quant_rows(const __hip_bfloat16*, unsigned char*, float*, long, int, int,
                           hipStream_t);
int fp8_cols_partials(long, int);
void launch_fp8_quant_cols_t(const __hip_bfloat16*, unsigned char*, float*, float*, float*,
                             float*, long, int, int, hipStream_t);
void launch_fp8_gemm_nt(const unsigned char*, const float*, const unsigned char*, const float*,
                        const __hip_bfloat16*, __hip_bfloat16*, long, int, int, int,
                        hipStream_t);
void launch_probe_mfma_fp8(const unsigned char*, const unsigned char*, float*, int, int,
                           hipStream_t);
int probe_ce_row_blocks(long, int, int);
void probe_ce_layout(int, int, bool, int*, int*);
template <typename T>
void launch_probe_ce(T*, const float*, const long*, float*, float*, long, int, int, int, float,
                     bool, int, hipStream_t);
template <typename GT>
void launch_probe_sgd(float*, float*, const GT*, const float*, const float*, __hip_bfloat16*, int,
                      long, float, float, hipStream_t);
int seg_ce_quad_blocks(long, int);
int seg_ce_fin_rows(long);
template <typename T>
void launch_seg_ce(T*, const float*, const unsigned char*, float*, float*, int*, float*, float*,
                   long*, float*, const float*, long, int, int, int, int, int, int, float, bool,
                   int, hipStream_t);
int knn_topk_auto_splits(long, long);
void launch_knn_topk(const __hip_bfloat16*, const __hip_bfloat16*, unsigned long long*, float*,
                     int*, long, long, int, int, int, hipStream_t);
void launch_gram_rnorm(const __hip_bfloat16*, const __hip_bfloat16*, float*, long, int, bool,
                       hipStream_t);
void launch_gram_tiles(const __hip_bfloat16*, const __hip_bfloat16*, const float*, const float*,
                       __hip_bfloat16*, float*, int, int, int, long, int, hipStream_t);
void launch_gram_finish(const float*, float*, long, double, hipStream_t);
void launch_gram_norm_bwd(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                          __hip_bfloat16*, long, int, float, bool, hipStream_t);
template <typename T>
void launch_multi_tensor_ema(T* const*, const T* const*, const long*, const int*,
                             const long*, int, float, hipStream_t);
template <typename T>
void launch_multi_tensor_adamw(T* const*, const T* const*, float* const*, float* const*,
                               float* const*, const long*, const int*, const long*, int,
                               float, float, float, float, float, float, float, float,
                               bool, hipStream_t);
template <typename T>
void launch_multi_tensor_l2norm_sq(const T* const*, const long*, const int*, const long*,
                                   int, float*, hipStream_t);
template <typename T, typename GT>
void launch_multi_tensor_adamw_planned(T* const*, const GT* const*, float* const*,
                                       float* const*, float* const*, const long*,
                                       const int*, const long*, int, const float*,
                                       const float*, const float*, const int*,
                                       const float*, float, float, float, float, float,
                                       float, float, float, bool, hipStream_t);
template <typename T>
void launch_multi_tensor_l2norm_planned(const T* const*, const long*, const int*,
                                        const long*, int, const int*, float*,
                                        hipStream_t);

namespace {

hipStream_t current_stream() { return at::hip::getCurrentHIPStream().stream(); }

#define DISPATCH_FLOAT_BF16(TYPE, NAME, ...)                                   \
  [&] {                                                                        \
    if (TYPE == at::ScalarType::Float) {                                       \
      using scalar_t = float;                                                  \
      return __VA_ARGS__();                                                    \
    } else if (TYPE == at::ScalarType::BFloat16) {                             \
      using scalar_t = __hip_bfloat16;                                         \
      return __VA_ARGS__();                                                    \
    } else {                                                                   \
      TORCH_CHECK(false, NAME ": unsupported dtype ", TYPE);                   \
    }                                                                          \
  }()

// fp32 workspace of the two-stage column reduction (common.h): one row of D
// per block for each of `n_acc` parameter gradients. Uninitialised on purpose:
// the kernels write every row they later read.
torch::Tensor colreduce_workspace(int n_acc, int D, const torch::Tensor& like) {
  return torch::empty({(long)n_acc * COLRED_MAX_PARTIALS, D},
                      like.options().dtype(torch::kFloat));
}

// ------------------------------- norms ---------------------------------

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                                         double eps) {
  CHECK_INPUT(x);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat));
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  DISPATCH_FLOAT_BF16(x.scalar_type(), "layernorm_fwd", [&] {
    launch_layernorm_fwd<scalar_t>(
        (const scalar_t*)x.data_ptr(), (const scalar_t*)w.data_ptr(),
        (const scalar_t*)b.data_ptr(), (scalar_t*)y.data_ptr(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, D, (float)eps,
        current_stream());
  });
  return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                         torch::Tensor mean, torch::Tensor rstd) {
  CHECK_INPUT(dy);
  CHECK_INPUT(x);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({D}, x.options());
  auto db = torch::empty({D}, x.options());
  auto ws = colreduce_workspace(2, D, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "layernorm_bwd", [&] {
    launch_layernorm_bwd<scalar_t>(
        (const scalar_t*)dy.data_ptr(), (const scalar_t*)x.data_ptr(),
        (const scalar_t*)w.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
        (scalar_t*)dx.data_ptr(), ws.data_ptr<float>(), (scalar_t*)dw.data_ptr(),
        (scalar_t*)db.data_ptr(), rows, D, current_stream());
  });
  return {dx, dw, db};
}

// LayerNorm of the rows flat[idx]: (y, sub = flat[idx], mean, rstd), bit-equal
// to row_gather + layernorm_fwd with one pass less over the gathered rows.
std::vector<torch::Tensor> gather_layernorm_fwd(torch::Tensor flat, torch::Tensor idx,
                                                torch::Tensor w, torch::Tensor b, double eps) {
  CHECK_INPUT(flat);
  CHECK_INPUT(idx);
  CHECK_INPUT(w);
  CHECK_INPUT(b);
  TORCH_CHECK(flat.dim() == 2, "gather_layernorm_fwd: flat must be [R, D]");
  TORCH_CHECK(idx.scalar_type() == torch::kLong, "gather_layernorm_fwd: idx must be int64");
  const int D = flat.size(1);
  TORCH_CHECK(D % 8 == 0, "gather_layernorm_fwd needs D % 8 == 0");
  TORCH_CHECK(w.numel() == D && b.numel() == D && w.scalar_type() == flat.scalar_type() &&
                  b.scalar_type() == flat.scalar_type(),
              "gather_layernorm_fwd: w / b must be [D] of flat's dtype");
  const long M = idx.numel();
  auto y = torch::empty({M, D}, flat.options());
  auto sub = torch::empty({M, D}, flat.options());
  auto mean = torch::empty({M}, flat.options().dtype(torch::kFloat));
  auto rstd = torch::empty({M}, flat.options().dtype(torch::kFloat));
  if (M == 0) return {y, sub, mean, rstd};
  DISPATCH_FLOAT_BF16(flat.scalar_type(), "gather_layernorm_fwd", [&] {
    launch_gather_layernorm_fwd<scalar_t>(
        (const scalar_t*)flat.data_ptr(), idx.data_ptr<long>(), (const scalar_t*)w.data_ptr(),
        (const scalar_t*)b.data_ptr(), (scalar_t*)y.data_ptr(), (scalar_t*)sub.data_ptr(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(), M, D, (float)eps, current_stream());
  });
  return {y, sub, mean, rstd};
}

// LayerNorm backward whose dx rows are accumulated into dacc[idx] in place
// (rows of idx disjoint); returns (dw, db), bit-equal to layernorm_bwd's.
std::vector<torch::Tensor> layernorm_bwd_scatter_acc_(torch::Tensor dacc, torch::Tensor idx,
                                                      torch::Tensor dy, torch::Tensor x,
                                                      torch::Tensor w, torch::Tensor mean,
                                                      torch::Tensor rstd) {
  CHECK_INPUT(dacc);
  CHECK_INPUT(idx);
  CHECK_INPUT(dy);
  CHECK_INPUT(x);
  CHECK_INPUT(w);
  CHECK_INPUT(mean);
  CHECK_INPUT(rstd);
  TORCH_CHECK(dacc.dim() == 2 && x.dim() == 2 && dy.dim() == 2,
              "layernorm_bwd_scatter_acc_: dacc, dy, x must be 2-D");
  TORCH_CHECK(idx.scalar_type() == torch::kLong,
              "layernorm_bwd_scatter_acc_: idx must be int64");
  const int D = x.size(1);
  const long M = x.size(0);
  TORCH_CHECK(D % 8 == 0 && D <= 1536,
              "layernorm_bwd_scatter_acc_ supports D % 8 == 0 and D <= 1536, got ", D);
  TORCH_CHECK(dacc.size(1) == D && dy.size(0) == M && dy.size(1) == D && idx.numel() == M &&
                  mean.numel() == M && rstd.numel() == M && w.numel() == D,
              "layernorm_bwd_scatter_acc_: shape mismatch");
  TORCH_CHECK(dacc.scalar_type() == x.scalar_type() && dy.scalar_type() == x.scalar_type() &&
                  w.scalar_type() == x.scalar_type() &&
                  mean.scalar_type() == torch::kFloat && rstd.scalar_type() == torch::kFloat,
              "layernorm_bwd_scatter_acc_: dtype mismatch");
  if (M == 0) return {torch::zeros({D}, x.options()), torch::zeros({D}, x.options())};
  auto dw = torch::empty({D}, x.options());
  auto db = torch::empty({D}, x.options());
  auto ws = colreduce_workspace(2, D, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "layernorm_bwd_scatter_acc_", [&] {
    launch_layernorm_bwd_scatter_acc<scalar_t>(
        (const scalar_t*)dy.data_ptr(), (const scalar_t*)x.data_ptr(),
        (const scalar_t*)w.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
        (scalar_t*)dacc.data_ptr(), idx.data_ptr<long>(), ws.data_ptr<float>(),
        (scalar_t*)dw.data_ptr(), (scalar_t*)db.data_ptr(), M, D, current_stream());
  });
  return {dw, db};
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps) {
  CHECK_INPUT(x);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  DISPATCH_FLOAT_BF16(x.scalar_type(), "rmsnorm_fwd", [&] {
    launch_rmsnorm_fwd<scalar_t>((const scalar_t*)x.data_ptr(), (const scalar_t*)w.data_ptr(),
                                 (scalar_t*)y.data_ptr(), rstd.data_ptr<float>(), rows, D,
                                 (float)eps, current_stream());
  });
  return {y, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                       torch::Tensor rstd) {
  CHECK_INPUT(dy);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({D}, x.options());
  auto ws = colreduce_workspace(1, D, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "rmsnorm_bwd", [&] {
    launch_rmsnorm_bwd<scalar_t>((const scalar_t*)dy.data_ptr(), (const scalar_t*)x.data_ptr(),
                                 (const scalar_t*)w.data_ptr(), rstd.data_ptr<float>(),
                                 (scalar_t*)dx.data_ptr(), ws.data_ptr<float>(),
                                 (scalar_t*)dw.data_ptr(), rows, D, current_stream());
  });
  return {dx, dw};
}

std::vector<torch::Tensor> l2norm_fwd(torch::Tensor x, double eps) {
  CHECK_INPUT(x);
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto s = torch::empty({rows}, x.options().dtype(torch::kFloat));
  DISPATCH_FLOAT_BF16(x.scalar_type(), "l2norm_fwd", [&] {
    launch_l2norm_fwd<scalar_t>((const scalar_t*)x.data_ptr(), (scalar_t*)y.data_ptr(),
                                s.data_ptr<float>(), rows, D, (float)eps, current_stream());
  });
  return {y, s};
}

torch::Tensor l2norm_bwd(torch::Tensor dy, torch::Tensor y, torch::Tensor s, double eps) {
  CHECK_INPUT(dy);
  const int D = y.size(-1);
  const long rows = y.numel() / D;
  auto dx = torch::empty_like(y);
  DISPATCH_FLOAT_BF16(y.scalar_type(), "l2norm_bwd", [&] {
    launch_l2norm_bwd<scalar_t>((const scalar_t*)dy.data_ptr(), (const scalar_t*)y.data_ptr(),
                                s.data_ptr<float>(), (scalar_t*)dx.data_ptr(), rows, D,
                                (float)eps, current_stream());
  });
  return dx;
}

// ----------------------------- elementwise ------------------------------

torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor bias) {
  CHECK_INPUT(x);
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "bias_gelu: H must be a multiple of 8");
  const long rows = x.numel() / H;
  auto y = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "bias_gelu_fwd", [&] {
    launch_bias_gelu_fwd<scalar_t>((const scalar_t*)x.data_ptr(),
                                   (const scalar_t*)bias.data_ptr(), (scalar_t*)y.data_ptr(),
                                   rows, H, current_stream());
  });
  return y;
}

std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor bias) {
  CHECK_INPUT(dy);
  const int H = x.size(-1);
  const long rows = x.numel() / H;
  auto dx = torch::empty_like(x);
  auto dbias = torch::empty({H}, x.options());
  auto ws = colreduce_workspace(1, H, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "bias_gelu_bwd", [&] {
    launch_bias_gelu_bwd<scalar_t>((const scalar_t*)dy.data_ptr(),
                                   (const scalar_t*)x.data_ptr(),
                                   (const scalar_t*)bias.data_ptr(), (scalar_t*)dx.data_ptr(),
                                   ws.data_ptr<float>(), (scalar_t*)dbias.data_ptr(), rows, H,
                                   current_stream());
  });
  return {dx, dbias};
}

torch::Tensor ls_axpy_fwd(torch::Tensor x, torch::Tensor res, torch::Tensor gamma) {
  CHECK_INPUT(x);
  CHECK_INPUT(res);
  const int D = x.size(-1);
  TORCH_CHECK(D % 8 == 0, "ls_axpy: D must be a multiple of 8");
  const long rows = x.numel() / D;
  auto out = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "ls_axpy_fwd", [&] {
    launch_ls_axpy_fwd<scalar_t>((const scalar_t*)x.data_ptr(),
                                 (const scalar_t*)res.data_ptr(),
                                 (const scalar_t*)gamma.data_ptr(),
                                 (scalar_t*)out.data_ptr(), rows, D, current_stream());
  });
  return out;
}

torch::Tensor ls_axpy_bias_fwd(torch::Tensor x, torch::Tensor res, torch::Tensor gamma,
                               torch::Tensor bias) {
  CHECK_INPUT(x);
  CHECK_INPUT(res);
  const int D = x.size(-1);
  TORCH_CHECK(D % 8 == 0, "ls_axpy_bias: D must be a multiple of 8");
  const long rows = x.numel() / D;
  auto out = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "ls_axpy_bias_fwd", [&] {
    launch_ls_axpy_bias_fwd<scalar_t>(
        (const scalar_t*)x.data_ptr(), (const scalar_t*)res.data_ptr(),
        (const scalar_t*)gamma.data_ptr(), (const scalar_t*)bias.data_ptr(),
        (scalar_t*)out.data_ptr(), rows, D, current_stream());
  });
  return out;
}

std::vector<torch::Tensor> ls_axpy_bwd(torch::Tensor dout, torch::Tensor res,
                                       torch::Tensor gamma) {
  CHECK_INPUT(dout);
  const int D = dout.size(-1);
  const long rows = dout.numel() / D;
  auto dres = torch::empty_like(dout);
  auto dgamma = torch::empty({D}, dout.options());
  auto ws = colreduce_workspace(1, D, dout);
  DISPATCH_FLOAT_BF16(dout.scalar_type(), "ls_axpy_bwd", [&] {
    launch_ls_axpy_bwd<scalar_t>((const scalar_t*)dout.data_ptr(),
                                 (const scalar_t*)res.data_ptr(),
                                 (const scalar_t*)gamma.data_ptr(),
                                 (scalar_t*)dres.data_ptr(), ws.data_ptr<float>(),
                                 (scalar_t*)dgamma.data_ptr(), rows, D, current_stream());
  });
  return {dres, dgamma};
}

std::vector<torch::Tensor> ls_axpy_bias_bwd(torch::Tensor dout, torch::Tensor res,
                                            torch::Tensor gamma, torch::Tensor bias) {
  CHECK_INPUT(dout);
  const int D = dout.size(-1);
  const long rows = dout.numel() / D;
  auto dres = torch::empty_like(dout);
  auto dgamma = torch::empty({D}, dout.options());
  auto dbias = torch::empty({D}, dout.options());
  auto ws = colreduce_workspace(2, D, dout);
  DISPATCH_FLOAT_BF16(dout.scalar_type(), "ls_axpy_bias_bwd", [&] {
    launch_ls_axpy_bias_bwd<scalar_t>(
        (const scalar_t*)dout.data_ptr(), (const scalar_t*)res.data_ptr(),
        (const scalar_t*)gamma.data_ptr(), (const scalar_t*)bias.data_ptr(),
        (scalar_t*)dres.data_ptr(), ws.data_ptr<float>(), (scalar_t*)dgamma.data_ptr(),
        (scalar_t*)dbias.data_ptr(), rows, D, current_stream());
  });
  return {dres, dgamma, dbias};
}

torch::Tensor row_gather(torch::Tensor src, torch::Tensor idx) {
  CHECK_INPUT(src);
  const int D = src.size(-1);
  TORCH_CHECK(D % 8 == 0, "row ops need D % 8 == 0");
  const long M = idx.numel();
  auto out = torch::empty({M, D}, src.options());
  DISPATCH_FLOAT_BF16(src.scalar_type(), "row_gather", [&] {
    launch_row_gather<scalar_t>((const scalar_t*)src.data_ptr(), idx.data_ptr<long>(),
                                (scalar_t*)out.data_ptr(), M, D, current_stream());
  });
  return out;
}

void row_scatter_add_(torch::Tensor dst, torch::Tensor idx, torch::Tensor src,
                      torch::Tensor scale) {
  CHECK_INPUT(dst);
  CHECK_INPUT(src);
  const int D = dst.size(-1);
  const long M = idx.numel();
  const float* sp = (scale.defined() && scale.numel() > 0) ? scale.data_ptr<float>() : nullptr;
  DISPATCH_FLOAT_BF16(dst.scalar_type(), "row_scatter_add", [&] {
    launch_row_scatter_add<scalar_t>((scalar_t*)dst.data_ptr(), idx.data_ptr<long>(),
                                     (const scalar_t*)src.data_ptr(), sp, M, D,
                                     current_stream());
  });
}

torch::Tensor row_gather_scaled(torch::Tensor src, torch::Tensor idx, torch::Tensor scale) {
  CHECK_INPUT(src);
  const int D = src.size(-1);
  const long M = idx.numel();
  auto out = torch::empty({M, D}, src.options());
  const float* sp = (scale.defined() && scale.numel() > 0) ? scale.data_ptr<float>() : nullptr;
  DISPATCH_FLOAT_BF16(src.scalar_type(), "row_gather_scaled", [&] {
    launch_row_gather_scaled<scalar_t>((const scalar_t*)src.data_ptr(),
                                       idx.data_ptr<long>(), sp, (scalar_t*)out.data_ptr(),
                                       M, D, current_stream());
  });
  return out;
}

void ls_scatter_add_(torch::Tensor dst, torch::Tensor idx, torch::Tensor src,
                     torch::Tensor gamma, torch::Tensor bias, torch::Tensor scale) {
  CHECK_INPUT(dst);
  CHECK_INPUT(src);
  const int D = dst.size(-1);
  TORCH_CHECK(D % 8 == 0, "ls_scatter: D must be a multiple of 8");
  const long M = idx.numel();
  DISPATCH_FLOAT_BF16(dst.scalar_type(), "ls_scatter_add_", [&] {
    launch_ls_scatter_add<scalar_t>(
        (scalar_t*)dst.data_ptr(), idx.data_ptr<long>(), (const scalar_t*)src.data_ptr(),
        gamma.defined() ? (const scalar_t*)gamma.data_ptr() : nullptr,
        bias.defined() ? (const scalar_t*)bias.data_ptr() : nullptr,
        scale.defined() && scale.numel() > 0 ? scale.data_ptr<float>() : nullptr, M, D,
        current_stream());
  });
}

std::vector<torch::Tensor> ls_scatter_bwd(torch::Tensor dy, torch::Tensor idx,
                                          torch::Tensor src, torch::Tensor gamma,
                                          torch::Tensor bias, torch::Tensor scale) {
  CHECK_INPUT(dy);
  CHECK_INPUT(src);
  const int D = dy.size(-1);
  const long M = idx.numel();
  auto dres = torch::empty_like(src);
  auto dgamma = gamma.defined() ? torch::empty({D}, dy.options()) : torch::Tensor();
  auto dbias = bias.defined() ? torch::empty({D}, dy.options()) : torch::Tensor();
  auto ws = colreduce_workspace(2, D, dy);
  DISPATCH_FLOAT_BF16(dy.scalar_type(), "ls_scatter_bwd", [&] {
    launch_ls_scatter_bwd<scalar_t>(
        (const scalar_t*)dy.data_ptr(), idx.data_ptr<long>(),
        (const scalar_t*)src.data_ptr(),
        gamma.defined() ? (const scalar_t*)gamma.data_ptr() : nullptr,
        bias.defined() ? (const scalar_t*)bias.data_ptr() : nullptr,
        scale.defined() && scale.numel() > 0 ? scale.data_ptr<float>() : nullptr,
        (scalar_t*)dres.data_ptr(), ws.data_ptr<float>(),
        dgamma.defined() ? (scalar_t*)dgamma.data_ptr() : nullptr,
        dbias.defined() ? (scalar_t*)dbias.data_ptr() : nullptr, M, D, current_stream());
  });
  return {dres, dgamma, dbias};
}

torch::Tensor swiglu_fwd(torch::Tensor x12) {
  CHECK_INPUT(x12);
  const int H2 = x12.size(-1);
  const int H = H2 / 2;
  const long rows = x12.numel() / H2;
  auto sizes = x12.sizes().vec();
  sizes.back() = H;
  auto y = torch::empty(sizes, x12.options());
  DISPATCH_FLOAT_BF16(x12.scalar_type(), "swiglu_fwd", [&] {
    launch_swiglu_fwd<scalar_t>((const scalar_t*)x12.data_ptr(), (scalar_t*)y.data_ptr(),
                                rows, H, current_stream());
  });
  return y;
}

torch::Tensor swiglu_bwd(torch::Tensor dy, torch::Tensor x12) {
  CHECK_INPUT(dy);
  const int H2 = x12.size(-1);
  const int H = H2 / 2;
  const long rows = x12.numel() / H2;
  auto dx12 = torch::empty_like(x12);
  DISPATCH_FLOAT_BF16(x12.scalar_type(), "swiglu_bwd", [&] {
    launch_swiglu_bwd<scalar_t>((const scalar_t*)dy.data_ptr(),
                                (const scalar_t*)x12.data_ptr(), (scalar_t*)dx12.data_ptr(),
                                rows, H, current_stream());
  });
  return dx12;
}

torch::Tensor rope_fwd(torch::Tensor x, torch::Tensor sin_t, torch::Tensor cos_t,
                       int64_t prefix) {
  CHECK_INPUT(x);
  TORCH_CHECK(x.dim() == 4, "rope_fwd expects [B, H, N, hd]");
  TORCH_CHECK(sin_t.scalar_type() == at::ScalarType::Float, "rope tables must be fp32");
  const long BH = x.size(0) * x.size(1);
  const int N = x.size(2);
  const int hd = x.size(3);
  const int P = N - (int)prefix;
  TORCH_CHECK(sin_t.size(0) == P && sin_t.size(1) == hd, "rope table shape mismatch");
  auto y = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "rope_fwd", [&] {
    launch_rope_fwd<scalar_t>((const scalar_t*)x.data_ptr(), sin_t.data_ptr<float>(),
                              cos_t.data_ptr<float>(), (scalar_t*)y.data_ptr(), BH, N, P, hd,
                              current_stream());
  });
  return y;
}

// ------------------------------ proto CE --------------------------------

std::vector<torch::Tensor> dino_ce_fwd(torch::Tensor x, torch::Tensor t, double temp,
                                       bool ignore_diag) {
  CHECK_INPUT(x);
  CHECK_INPUT(t);
  TORCH_CHECK(x.dim() == 3 && t.dim() == 3, "dino_ce expects [S,B,K] and [T,B,K]");
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16);
  TORCH_CHECK(t.scalar_type() == at::ScalarType::Float);
  const int S = x.size(0), B = x.size(1);
  const int T = t.size(0);
  const long K = x.size(2);
  auto lse = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_dino_ce_fwd((const __hip_bfloat16*)x.data_ptr(), t.data_ptr<float>(),
                     lse.data_ptr<float>(), st.data_ptr<float>(), loss.data_ptr<float>(),
                     S, T, B, K, (float)(1.0 / temp), ignore_diag, current_stream());
  return {loss, lse, st};
}

torch::Tensor dino_ce_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor t,
                          torch::Tensor lse, torch::Tensor st, double temp,
                          bool ignore_diag) {
  const int S = x.size(0), B = x.size(1);
  const int T = t.size(0);
  const long K = x.size(2);
  auto dx = torch::empty_like(x);
  launch_dino_ce_bwd((const __hip_bfloat16*)x.data_ptr(), t.data_ptr<float>(),
                     lse.data_ptr<float>(), st.data_ptr<float>(), g.data_ptr<float>(),
                     (__hip_bfloat16*)dx.data_ptr(), S, T, B, K, (float)(1.0 / temp),
                     ignore_diag, current_stream());
  return dx;
}

std::vector<torch::Tensor> ibot_ce_fwd(torch::Tensor x, torch::Tensor t, torch::Tensor w,
                                       double temp) {
  CHECK_INPUT(x);
  CHECK_INPUT(t);
  const int M = x.size(0);
  const long K = x.size(1);
  auto lse = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_ibot_ce_fwd((const __hip_bfloat16*)x.data_ptr(), t.data_ptr<float>(),
                     w.data_ptr<float>(), lse.data_ptr<float>(), st.data_ptr<float>(),
                     loss.data_ptr<float>(), M, K, (float)(1.0 / temp), current_stream());
  return {loss, lse, st};
}

torch::Tensor ibot_ce_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor t,
                          torch::Tensor w, torch::Tensor lse, torch::Tensor st,
                          double temp) {
  const int M = x.size(0);
  const long K = x.size(1);
  auto dx = torch::empty_like(x);
  launch_ibot_ce_bwd((const __hip_bfloat16*)x.data_ptr(), t.data_ptr<float>(),
                     w.data_ptr<float>(), lse.data_ptr<float>(), st.data_ptr<float>(),
                     g.data_ptr<float>(), (__hip_bfloat16*)dx.data_ptr(), M, K,
                     (float)(1.0 / temp), current_stream());
  return dx;
}

torch::Tensor sinkhorn_fact_colsum(torch::Tensor x, torch::Tensor u, double temp) {
  CHECK_INPUT(x);
  const int M = x.size(0);
  const long K = x.size(1);
  auto A = torch::empty({K}, x.options().dtype(torch::kFloat));
  const float* up = (u.defined() && u.numel() > 0) ? u.data_ptr<float>() : nullptr;
  launch_sinkhorn_fact_colsum((const __hip_bfloat16*)x.data_ptr(), up,
                              A.data_ptr<float>(), M, K, (float)(1.0 / temp),
                              current_stream());
  return A;
}

torch::Tensor sinkhorn_fact_rowsum(torch::Tensor x, torch::Tensor v, double temp) {
  CHECK_INPUT(x);
  const int M = x.size(0);
  const long K = x.size(1);
  auto u = torch::empty({M}, x.options().dtype(torch::kFloat));
  launch_sinkhorn_fact_rowsum((const __hip_bfloat16*)x.data_ptr(), v.data_ptr<float>(),
                              u.data_ptr<float>(), M, K, (float)(1.0 / temp),
                              current_stream());
  return u;
}

std::vector<torch::Tensor> ibot_ce_fact_fwd(torch::Tensor x, torch::Tensor xt,
                                            torch::Tensor u, torch::Tensor v,
                                            torch::Tensor w, double temp, double tt) {
  CHECK_INPUT(x);
  CHECK_INPUT(xt);
  const int M = x.size(0);
  const long K = x.size(1);
  auto lse = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_ibot_ce_fact_fwd((const __hip_bfloat16*)x.data_ptr(),
                          (const __hip_bfloat16*)xt.data_ptr(), u.data_ptr<float>(),
                          v.data_ptr<float>(), w.data_ptr<float>(), lse.data_ptr<float>(),
                          st.data_ptr<float>(), loss.data_ptr<float>(), M, K,
                          (float)(1.0 / temp), (float)(1.0 / tt), current_stream());
  return {loss, lse, st};
}

torch::Tensor ibot_ce_fact_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor xt,
                               torch::Tensor u, torch::Tensor v, torch::Tensor w,
                               torch::Tensor lse, torch::Tensor st, double temp,
                               double tt) {
  const int M = x.size(0);
  const long K = x.size(1);
  auto dx = torch::empty_like(x);
  launch_ibot_ce_fact_bwd((const __hip_bfloat16*)x.data_ptr(),
                          (const __hip_bfloat16*)xt.data_ptr(), u.data_ptr<float>(),
                          v.data_ptr<float>(), w.data_ptr<float>(), lse.data_ptr<float>(),
                          st.data_ptr<float>(), g.data_ptr<float>(),
                          (__hip_bfloat16*)dx.data_ptr(), M, K, (float)(1.0 / temp),
                          (float)(1.0 / tt), current_stream());
  return dx;
}

std::vector<torch::Tensor> dino_ce_fact_fwd(torch::Tensor x, torch::Tensor xt,
                                            torch::Tensor u, torch::Tensor v, double temp,
                                            double tt, bool ignore_diag) {
  CHECK_INPUT(x);
  CHECK_INPUT(xt);
  const int S = x.size(0), B = x.size(1);
  const int T = xt.size(0);
  const long K = x.size(2);
  auto lse = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_dino_ce_fact_fwd((const __hip_bfloat16*)x.data_ptr(),
                          (const __hip_bfloat16*)xt.data_ptr(), u.data_ptr<float>(),
                          v.data_ptr<float>(), lse.data_ptr<float>(), st.data_ptr<float>(),
                          loss.data_ptr<float>(), S, T, B, K, (float)(1.0 / temp),
                          (float)(1.0 / tt), ignore_diag, current_stream());
  return {loss, lse, st};
}

torch::Tensor dino_ce_fact_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor xt,
                               torch::Tensor u, torch::Tensor v, torch::Tensor lse,
                               torch::Tensor st, double temp, double tt,
                               bool ignore_diag) {
  const int S = x.size(0), B = x.size(1);
  const int T = xt.size(0);
  const long K = x.size(2);
  auto dx = torch::empty_like(x);
  launch_dino_ce_fact_bwd((const __hip_bfloat16*)x.data_ptr(),
                          (const __hip_bfloat16*)xt.data_ptr(), u.data_ptr<float>(),
                          v.data_ptr<float>(), lse.data_ptr<float>(), st.data_ptr<float>(),
                          g.data_ptr<float>(), (__hip_bfloat16*)dx.data_ptr(), S, T, B, K,
                          (float)(1.0 / temp), (float)(1.0 / tt), ignore_diag,
                          current_stream());
  return dx;
}

std::vector<torch::Tensor> sinkhorn_exp(torch::Tensor x, double temp) {
  CHECK_INPUT(x);
  auto Q = torch::empty(x.sizes(), x.options().dtype(torch::kFloat));
  auto total = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_sinkhorn_exp((const __hip_bfloat16*)x.data_ptr(), Q.data_ptr<float>(),
                      total.data_ptr<float>(), x.numel(), (float)(1.0 / temp),
                      current_stream());
  return {Q, total};
}

torch::Tensor sinkhorn_colsum(torch::Tensor Q, torch::Tensor divisor) {
  const int M = Q.size(0);
  const long K = Q.size(1);
  auto out = torch::empty({K}, Q.options());
  launch_sinkhorn_colsum(Q.data_ptr<float>(), out.data_ptr<float>(), M, K,
                         divisor.data_ptr<float>(), current_stream());
  return out;
}

void sinkhorn_div_row(torch::Tensor Q, torch::Tensor col, double k_div, torch::Tensor B,
                      bool scale_back) {
  const int M = Q.size(0);
  const long K = Q.size(1);
  launch_sinkhorn_div_row(Q.data_ptr<float>(), col.data_ptr<float>(), M, K, (float)k_div,
                          B.data_ptr<float>(), scale_back, current_stream());
}

// -------------------------------- fmha ----------------------------------

torch::Tensor probe_mfma(torch::Tensor A, torch::Tensor B) {
  CHECK_INPUT(A);
  CHECK_INPUT(B);
  TORCH_CHECK(A.scalar_type() == at::ScalarType::BFloat16);
  auto C = torch::empty({32, 32}, A.options().dtype(torch::kFloat));
  launch_probe_mfma((const __hip_bfloat16*)A.data_ptr(), (const __hip_bfloat16*)B.data_ptr(),
                    C.data_ptr<float>(), current_stream());
  return C;
}

// Argument checks of the attention wrappers (fmha_*, fmha_rope_*): every tensor
// the kernels dereference is on the device, contiguous, of the expected dtype
// and holds as many elements as its shape implies.
struct AttnDims {
  int B, H, N, HD;
  int64_t numel() const { return (int64_t)B * H * N * HD; }  // of q, k, v, o, dO each
  float scale() const { return 1.0f / std::sqrt((float)HD); }
};

static void check_attn(const torch::Tensor& x, at::ScalarType dtype, int64_t numel,
                       const char* name) {
  TORCH_CHECK(x.defined() && x.is_cuda() && x.is_contiguous(), "fmha: ", name,
              " must be a contiguous HIP tensor");
  TORCH_CHECK(x.scalar_type() == dtype, "fmha: ", name, " must be ", dtype, ", got ",
              x.scalar_type());
  TORCH_CHECK(x.numel() == numel, "fmha: ", name, " must hold ", numel, " elements, got ",
              x.numel());
}

static const __hip_bfloat16* bf16_in(const torch::Tensor& x) {
  return (const __hip_bfloat16*)x.data_ptr();
}
static __hip_bfloat16* bf16_out(torch::Tensor& x) { return (__hip_bfloat16*)x.data_ptr(); }

static AttnDims plain_dims(const torch::Tensor& q, const torch::Tensor& k,
                           const torch::Tensor& v) {
  TORCH_CHECK(q.dim() == 4, "fmha expects [B, H, N, hd]");
  const AttnDims d{(int)q.size(0), (int)q.size(1), (int)q.size(2), (int)q.size(3)};
  TORCH_CHECK(d.HD == 64 || d.HD == 128, "fmha: head_dim must be 64 or 128, got ", d.HD);
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(), "fmha: q, k, v differ in shape");
  check_attn(q, at::kBFloat16, d.numel(), "q");
  check_attn(k, at::kBFloat16, d.numel(), "k");
  check_attn(v, at::kBFloat16, d.numel(), "v");
  return d;
}

static AttnDims packed_dims(const torch::Tensor& qkv) {
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv must be [B, N, 3, H, hd]");
  const AttnDims d{(int)qkv.size(0), (int)qkv.size(3), (int)qkv.size(1), (int)qkv.size(4)};
  TORCH_CHECK(d.HD == 64 || d.HD == 128, "head_dim must be 64 or 128");
  check_attn(qkv, at::kBFloat16, 3 * d.numel(), "qkv");
  return d;
}

// o, lse (forward results) and dout, as the backward wrappers receive them
static void check_bwd_inputs(const AttnDims& d, const torch::Tensor& dout,
                             const torch::Tensor& o, const torch::Tensor& lse) {
  check_attn(dout, at::kBFloat16, d.numel(), "dout");
  check_attn(o, at::kBFloat16, d.numel(), "o");
  check_attn(lse, at::kFloat, (int64_t)d.B * d.H * d.N, "lse");
}

// fp32 [N - prefix, hd] sin / cos tables, or both empty for no RoPE
struct RopeTables {
  const float *sin, *cos;
  int P;
};

static RopeTables rope_tables(const AttnDims& d, const torch::Tensor& sin_t,
                              const torch::Tensor& cos_t, int64_t prefix) {
  const int P = d.N - (int)prefix;
  if (!(sin_t.defined() && sin_t.numel() > 0)) return {nullptr, nullptr, P};
  TORCH_CHECK(sin_t.dim() == 2 && sin_t.size(0) == P, "rope table rows must equal N - prefix");
  TORCH_CHECK(sin_t.size(1) == d.HD, "rope tables must be [N - prefix, hd]");
  check_attn(sin_t, at::kFloat, (int64_t)P * d.HD, "sin_t");
  TORCH_CHECK(cos_t.defined() && cos_t.sizes() == sin_t.sizes(), "cos_t must match sin_t in shape");
  check_attn(cos_t, at::kFloat, (int64_t)P * d.HD, "cos_t");
  return {sin_t.data_ptr<float>(), cos_t.data_ptr<float>(), P};
}

// single-pass backward where one workgroup holds the sequence, unless switched off
static bool use_fused_bwd(const AttnDims& d) {
  return fmha_rope::fused_bwd_supported(d.N, d.HD) && fmha_rope::fused_bwd_enabled();
}

std::vector<torch::Tensor> fmha_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v) {
  using L = fmha_rope::PlainLayout;
  const AttnDims d = plain_dims(q, k, v);
  auto o = torch::empty_like(q);
  auto lse = torch::empty({d.B, d.H, d.N}, q.options().dtype(torch::kFloat));
  fmha_rope::launch_fwd<L>(L::Qkv{bf16_in(q), bf16_in(k), bf16_in(v)}, nullptr, nullptr,
                           bf16_out(o), lse.data_ptr<float>(), d.B, d.H, d.N, d.N, d.HD,
                           d.scale(), current_stream());
  return {o, lse};
}

std::vector<torch::Tensor> fmha_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o, torch::Tensor lse) {
  using L = fmha_rope::PlainLayout;
  const AttnDims d = plain_dims(q, k, v);
  check_bwd_inputs(d, dout, o, lse);
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  const L::Qkv in{bf16_in(q), bf16_in(k), bf16_in(v)};
  const L::DQkv grad{bf16_out(dq), bf16_out(dk), bf16_out(dv)};
  auto stream = current_stream();
  if (use_fused_bwd(d)) {
    fmha_rope::launch_bwd_fused<L>(in, bf16_in(dout), bf16_in(o), nullptr, nullptr,
                                   lse.data_ptr<float>(), grad, d.B, d.H, d.N, d.N, d.HD,
                                   d.scale(), stream);
    return {dq, dk, dv};
  }
  auto D = torch::empty({d.B, d.H, d.N}, q.options().dtype(torch::kFloat));
  fmha_rope::launch_bwd_pre<L>(bf16_in(dout), bf16_in(o), D.data_ptr<float>(), d.B, d.H, d.N,
                               d.HD, stream);
  fmha_rope::launch_bwd_dq<L>(in, bf16_in(dout), nullptr, nullptr, lse.data_ptr<float>(),
                              D.data_ptr<float>(), grad, d.B, d.H, d.N, d.N, d.HD, d.scale(),
                              stream);
  fmha_rope::launch_bwd_dkv<L>(in, bf16_in(dout), nullptr, nullptr, lse.data_ptr<float>(),
                               D.data_ptr<float>(), grad, d.B, d.H, d.N, d.N, d.HD, d.scale(),
                               stream);
  return {dq, dk, dv};
}

// ----------------------------- patch embed ------------------------------

torch::Tensor patch_embed_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor bias,
                              int64_t patch) {
  CHECK_INPUT(x);
  CHECK_INPUT(w);
  TORCH_CHECK(x.dim() == 4 && x.scalar_type() == at::ScalarType::BFloat16);
  const int B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int D = w.size(0);
  TORCH_CHECK(C == 3, "patch_embed_fwd kernel supports C=3 (any patch size)");
  TORCH_CHECK(H % patch == 0 && W % patch == 0, "H/W must be multiples of patch");
  const long rows = (long)B * (H / patch) * (W / patch);
  auto out = torch::empty({(long)B, rows / B, (long)D}, x.options());
  launch_patch_embed_fwd((const __hip_bfloat16*)x.data_ptr(),
                         (const __hip_bfloat16*)w.data_ptr(),
                         (const __hip_bfloat16*)bias.data_ptr(),
                         (__hip_bfloat16*)out.data_ptr(), B, C, H, W, (int)patch, D,
                         current_stream());
  return out;
}

// ----------------------------- fmha + rope ------------------------------

std::vector<torch::Tensor> fmha_rope_fwd_out(torch::Tensor qkv, torch::Tensor sin_t,
                                             torch::Tensor cos_t, int64_t prefix,
                                             torch::Tensor out_o) {
  using L = fmha_rope::PackedLayout;
  const AttnDims d = packed_dims(qkv);
  const RopeTables rope = rope_tables(d, sin_t, cos_t, prefix);
  torch::Tensor o = out_o.defined() && out_o.numel() > 0
                        ? out_o
                        : torch::empty({d.B, d.N, d.H, d.HD}, qkv.options());
  check_attn(o, at::kBFloat16, d.numel(), "out_o");
  auto lse = torch::empty({d.B, d.H, d.N}, qkv.options().dtype(torch::kFloat));
  fmha_rope::launch_fwd<L>(L::Qkv{bf16_in(qkv)}, rope.sin, rope.cos, bf16_out(o),
                           lse.data_ptr<float>(), d.B, d.H, d.N, rope.P, d.HD, d.scale(),
                           current_stream());
  return {o, lse};
}

torch::Tensor fmha_rope_bwd_out(torch::Tensor dout, torch::Tensor qkv, torch::Tensor o,
                                torch::Tensor lse, torch::Tensor sin_t,
                                torch::Tensor cos_t, int64_t prefix,
                                torch::Tensor out_dqkv) {
  using L = fmha_rope::PackedLayout;
  const AttnDims d = packed_dims(qkv);
  check_bwd_inputs(d, dout, o, lse);
  const RopeTables rope = rope_tables(d, sin_t, cos_t, prefix);
  torch::Tensor dqkv = out_dqkv.defined() && out_dqkv.numel() > 0 ? out_dqkv
                                                                  : torch::empty_like(qkv);
  check_attn(dqkv, at::kBFloat16, 3 * d.numel(), "out_dqkv");
  const L::Qkv in{bf16_in(qkv)};
  const L::DQkv grad{bf16_out(dqkv)};
  auto stream = current_stream();
  if (use_fused_bwd(d)) {
    fmha_rope::launch_bwd_fused<L>(in, bf16_in(dout), bf16_in(o), rope.sin, rope.cos,
                                   lse.data_ptr<float>(), grad, d.B, d.H, d.N, rope.P, d.HD,
                                   d.scale(), stream);
    return dqkv;
  }
  auto D = torch::empty({d.B, d.H, d.N}, qkv.options().dtype(torch::kFloat));
  fmha_rope::launch_bwd_pre<L>(bf16_in(dout), bf16_in(o), D.data_ptr<float>(), d.B, d.H, d.N,
                               d.HD, stream);
  fmha_rope::launch_bwd_dq<L>(in, bf16_in(dout), rope.sin, rope.cos, lse.data_ptr<float>(),
                              D.data_ptr<float>(), grad, d.B, d.H, d.N, rope.P, d.HD,
                              d.scale(), stream);
  fmha_rope::launch_bwd_dkv<L>(in, bf16_in(dout), rope.sin, rope.cos, lse.data_ptr<float>(),
                               D.data_ptr<float>(), grad, d.B, d.H, d.N, rope.P, d.HD,
                               d.scale(), stream);
  return dqkv;
}


// planned single-launch variants: tables are prebuilt device tensors owned by
// the Python-side MultiTensorPlan (no per-call table construction/upload).

void multi_tensor_ema_planned(torch::Tensor ptrs, torch::Tensor sizes, torch::Tensor ct,
                              torch::Tensor co, int64_t n_tensors, double m,
                              bool is_bf16) {
  const int n_chunks = (int)ct.numel();
  long* pp = ptrs.data_ptr<long>();
  if (is_bf16) {
    launch_multi_tensor_ema<__hip_bfloat16>(
        (__hip_bfloat16* const*)pp, (const __hip_bfloat16* const*)(pp + n_tensors),
        sizes.data_ptr<long>(), ct.data_ptr<int>(), co.data_ptr<long>(), n_chunks,
        (float)m, current_stream());
  } else {
    launch_multi_tensor_ema<float>(
        (float* const*)pp, (const float* const*)(pp + n_tensors), sizes.data_ptr<long>(),
        ct.data_ptr<int>(), co.data_ptr<long>(), n_chunks, (float)m, current_stream());
  }
}

void multi_tensor_adamw_planned(torch::Tensor ptrs, torch::Tensor sizes, torch::Tensor ct,
                                torch::Tensor co, int64_t n_tensors, torch::Tensor lr_mult,
                                torch::Tensor wd_mult, torch::Tensor is_last,
                                torch::Tensor sub_id, torch::Tensor clip, double lr,
                                double last_lr, double wd, double beta1, double beta2,
                                double eps, double bc1, double bc2, bool has_master,
                                bool is_bf16, bool grad_is_f32) {
  const int n_chunks = (int)ct.numel();
  long* pp = ptrs.data_ptr<long>();
  const long n = n_tensors;
  if (is_bf16 && grad_is_f32) {
    launch_multi_tensor_adamw_planned<__hip_bfloat16, float>(
        (__hip_bfloat16* const*)pp, (const float* const*)(pp + n),
        (float* const*)(pp + 2 * n), (float* const*)(pp + 3 * n),
        has_master ? (float* const*)(pp + 4 * n) : nullptr, sizes.data_ptr<long>(),
        ct.data_ptr<int>(), co.data_ptr<long>(), n_chunks, lr_mult.data_ptr<float>(),
        wd_mult.data_ptr<float>(), is_last.data_ptr<float>(), sub_id.data_ptr<int>(),
        clip.data_ptr<float>(), (float)lr, (float)last_lr, (float)wd, (float)beta1,
        (float)beta2, (float)eps, (float)bc1, (float)bc2, has_master, current_stream());
  } else if (is_bf16) {
    launch_multi_tensor_adamw_planned<__hip_bfloat16, __hip_bfloat16>(
        (__hip_bfloat16* const*)pp, (const __hip_bfloat16* const*)(pp + n),
        (float* const*)(pp + 2 * n), (float* const*)(pp + 3 * n),
        has_master ? (float* const*)(pp + 4 * n) : nullptr, sizes.data_ptr<long>(),
        ct.data_ptr<int>(), co.data_ptr<long>(), n_chunks, lr_mult.data_ptr<float>(),
        wd_mult.data_ptr<float>(), is_last.data_ptr<float>(), sub_id.data_ptr<int>(),
        clip.data_ptr<float>(), (float)lr, (float)last_lr, (float)wd, (float)beta1,
        (float)beta2, (float)eps, (float)bc1, (float)bc2, has_master, current_stream());
  } else {
    launch_multi_tensor_adamw_planned<float, float>(
        (float* const*)pp, (const float* const*)(pp + n), (float* const*)(pp + 2 * n),
        (float* const*)(pp + 3 * n), has_master ? (float* const*)(pp + 4 * n) : nullptr,
        sizes.data_ptr<long>(), ct.data_ptr<int>(), co.data_ptr<long>(), n_chunks,
        lr_mult.data_ptr<float>(), wd_mult.data_ptr<float>(), is_last.data_ptr<float>(),
        sub_id.data_ptr<int>(), clip.data_ptr<float>(), (float)lr, (float)last_lr,
        (float)wd, (float)beta1, (float)beta2, (float)eps, (float)bc1, (float)bc2,
        has_master, current_stream());
  }
}

torch::Tensor multi_tensor_l2norm_planned(torch::Tensor ptrs, torch::Tensor sizes,
                                          torch::Tensor ct, torch::Tensor co,
                                          torch::Tensor sub_id, int64_t n_submodels,
                                          bool is_bf16) {
  const int n_chunks = (int)ct.numel();
  auto out = torch::zeros({n_submodels}, torch::dtype(torch::kFloat).device(ptrs.device()));
  long* pp = ptrs.data_ptr<long>();
  if (is_bf16) {
    launch_multi_tensor_l2norm_planned<__hip_bfloat16>(
        (const __hip_bfloat16* const*)pp, sizes.data_ptr<long>(), ct.data_ptr<int>(),
        co.data_ptr<long>(), n_chunks, sub_id.data_ptr<int>(), out.data_ptr<float>(),
        current_stream());
  } else {
    launch_multi_tensor_l2norm_planned<float>(
        (const float* const*)pp, sizes.data_ptr<long>(), ct.data_ptr<int>(),
        co.data_ptr<long>(), n_chunks, sub_id.data_ptr<int>(), out.data_ptr<float>(),
        current_stream());
  }
  return out;
}

// ---------------------------- multi-tensor ------------------------------

struct MTTables {
  torch::Tensor device_buf;  // holds sizes + chunk tables + ptr arrays
  long* sizes;
  int* chunk_tensor;
  long* chunk_offset;
  long* ptr_arrays;  // base of pointer storage (n_lists * n_tensors int64)
  int n_chunks;
  int n_tensors;
};

constexpr long kMTChunk = 65536;

MTTables build_tables(const std::vector<std::vector<torch::Tensor>>& lists,
                      torch::Device device) {
  const int n_tensors = (int)lists[0].size();
  const int n_lists = (int)lists.size();
  std::vector<long> sizes(n_tensors);
  std::vector<int> chunk_tensor;
  std::vector<long> chunk_offset;
  for (int t = 0; t < n_tensors; ++t) {
    sizes[t] = lists[0][t].numel();
    for (long off = 0; off < sizes[t]; off += kMTChunk) {
      chunk_tensor.push_back(t);
      chunk_offset.push_back(off);
    }
  }
  const int n_chunks = (int)chunk_tensor.size();
  // layout (int64 slots): [sizes n_tensors][chunk_tensor n_chunks (as i64)]
  //                       [chunk_offset n_chunks][ptrs n_lists*n_tensors]
  const long total = n_tensors + n_chunks + n_chunks + (long)n_lists * n_tensors;
  auto host = torch::empty({total}, torch::dtype(torch::kLong).pinned_memory(true));
  long* hp = host.data_ptr<long>();
  long* p_sizes = hp;
  long* p_ct = hp + n_tensors;
  long* p_co = p_ct + n_chunks;
  long* p_ptr = p_co + n_chunks;
  for (int t = 0; t < n_tensors; ++t) p_sizes[t] = sizes[t];
  for (int c = 0; c < n_chunks; ++c) {
    p_ct[c] = chunk_tensor[c];
    p_co[c] = chunk_offset[c];
  }
  for (int l = 0; l < n_lists; ++l)
    for (int t = 0; t < n_tensors; ++t)
      p_ptr[(long)l * n_tensors + t] = (long)(uintptr_t)lists[l][t].data_ptr();
  auto dev = host.to(device, /*non_blocking=*/true);
  MTTables out;
  out.device_buf = dev;
  long* dp = dev.data_ptr<long>();
  out.sizes = dp;
  out.chunk_tensor = nullptr;  // stored as i64; kernel wants int — handled below
  out.chunk_offset = dp + n_tensors + n_chunks;
  out.ptr_arrays = dp + n_tensors + 2 * (long)n_chunks;
  out.n_chunks = n_chunks;
  out.n_tensors = n_tensors;
  return out;
}

// The chunk_tensor table must be int32 for the kernels; build a separate one.
torch::Tensor build_chunk_tensor_i32(const std::vector<long>& sizes, torch::Device device,
                                     int* n_chunks_out) {
  std::vector<int> ct;
  for (int t = 0; t < (int)sizes.size(); ++t)
    for (long off = 0; off < sizes[t]; off += kMTChunk) ct.push_back(t);
  *n_chunks_out = (int)ct.size();
  auto host = torch::from_blob(ct.data(), {(long)ct.size()}, torch::kInt).clone();
  return host.to(device);
}

void multi_tensor_ema(std::vector<torch::Tensor> t_list, std::vector<torch::Tensor> s_list,
                      double m) {
  TORCH_CHECK(!t_list.empty() && t_list.size() == s_list.size());
  auto device = t_list[0].device();
  auto tables = build_tables({t_list, s_list}, device);
  std::vector<long> sizes(tables.n_tensors);
  for (int t = 0; t < tables.n_tensors; ++t) sizes[t] = t_list[t].numel();
  int n_chunks;
  auto ct32 = build_chunk_tensor_i32(sizes, device, &n_chunks);
  auto stream = current_stream();
  DISPATCH_FLOAT_BF16(t_list[0].scalar_type(), "multi_tensor_ema", [&] {
    launch_multi_tensor_ema<scalar_t>(
        (scalar_t* const*)(tables.ptr_arrays),
        (const scalar_t* const*)(tables.ptr_arrays + tables.n_tensors),
        tables.sizes, ct32.data_ptr<int>(), tables.chunk_offset, n_chunks, (float)m, stream);
  });
}

void multi_tensor_adamw(std::vector<torch::Tensor> p, std::vector<torch::Tensor> g,
                        std::vector<torch::Tensor> m, std::vector<torch::Tensor> v,
                        std::vector<torch::Tensor> w, double lr, double beta1, double beta2,
                        double eps, double weight_decay, double bc1, double bc2,
                        double grad_scale) {
  TORCH_CHECK(!p.empty());
  const bool has_master = !w.empty();
  auto device = p[0].device();
  std::vector<std::vector<torch::Tensor>> lists = {p, g, m, v};
  if (has_master) lists.push_back(w);
  auto tables = build_tables(lists, device);
  std::vector<long> sizes(tables.n_tensors);
  for (int t = 0; t < tables.n_tensors; ++t) sizes[t] = p[t].numel();
  int n_chunks;
  auto ct32 = build_chunk_tensor_i32(sizes, device, &n_chunks);
  auto stream = current_stream();
  const int nt = tables.n_tensors;
  DISPATCH_FLOAT_BF16(p[0].scalar_type(), "multi_tensor_adamw", [&] {
    launch_multi_tensor_adamw<scalar_t>(
        (scalar_t* const*)(tables.ptr_arrays),
        (const scalar_t* const*)(tables.ptr_arrays + nt),
        (float* const*)(tables.ptr_arrays + 2L * nt),
        (float* const*)(tables.ptr_arrays + 3L * nt),
        has_master ? (float* const*)(tables.ptr_arrays + 4L * nt) : nullptr,
        tables.sizes, ct32.data_ptr<int>(), tables.chunk_offset, n_chunks, (float)lr,
        (float)beta1, (float)beta2, (float)eps, (float)weight_decay, (float)bc1, (float)bc2,
        (float)grad_scale, has_master, stream);
  });
}

torch::Tensor multi_tensor_l2norm_sq(std::vector<torch::Tensor> g) {
  TORCH_CHECK(!g.empty());
  auto device = g[0].device();
  auto tables = build_tables({g}, device);
  std::vector<long> sizes(tables.n_tensors);
  for (int t = 0; t < tables.n_tensors; ++t) sizes[t] = g[t].numel();
  int n_chunks;
  auto ct32 = build_chunk_tensor_i32(sizes, device, &n_chunks);
  auto out = torch::zeros({}, torch::dtype(torch::kFloat).device(device));
  DISPATCH_FLOAT_BF16(g[0].scalar_type(), "multi_tensor_l2norm_sq", [&] {
    launch_multi_tensor_l2norm_sq<scalar_t>(
        (const scalar_t* const*)(tables.ptr_arrays), tables.sizes, ct32.data_ptr<int>(),
        tables.chunk_offset, n_chunks, out.data_ptr<float>(), current_stream());
  });
  return out;
}

// ------------------------- fp8 forward and backward ---------------------

#define CHECK_FP8_FMT(fmt, who) \
  TORCH_CHECK((fmt) == FP8_FMT_E4M3 || (fmt) == FP8_FMT_E5M2, who ": format must be 0 (e4m3) or 1 (e5m2)")

// bf16 [M,K] -> (fp8 bytes [M,K] as uint8, fp32 power-of-two scales [M]).
// fmt: FP8_FMT_E4M3 (0, default) or FP8_FMT_E5M2 (1).
std::vector<torch::Tensor> fp8_quant_rows(torch::Tensor x, int64_t fmt) {
  CHECK_INPUT(x);
  CHECK_FP8_FMT(fmt, "fp8_quant_rows");
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16, "fp8_quant_rows: x must be bf16");
  TORCH_CHECK(x.dim() == 2, "fp8_quant_rows: x must be [M, K]");
  const long M = x.size(0);
  const long K = x.size(1);
  TORCH_CHECK(K > 0 && K % FP8_QUANT_VEC == 0 && K <= INT_MAX,
              "fp8_quant_rows: K must be a positive multiple of ", FP8_QUANT_VEC);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0, "fp8_quant_rows: x must be 16-byte aligned");
  auto q = torch::empty({M, K}, x.options().dtype(torch::kUInt8));
  auto scale = torch::empty({M}, x.options().dtype(torch::kFloat));
  launch_fp8_quant_rows((const __hip_bfloat16*)x.data_ptr(), q.data_ptr<uint8_t>(),
                        scale.data_ptr<float>(), M, (int)K, (int)fmt, current_stream());
  return {q, scale};
}

// bf16 [R,C] -> (fp8 bytes [C,Rp] as uint8 with Rp = ceil(R/128)*128 and zero
// pad, fp32 scales [C], fp32 column sums [C] or an empty tensor).
std::vector<torch::Tensor> fp8_quant_cols_t(torch::Tensor x, int64_t fmt, bool colsum) {
  CHECK_INPUT(x);
  CHECK_FP8_FMT(fmt, "fp8_quant_cols_t");
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16, "fp8_quant_cols_t: x must be bf16");
  TORCH_CHECK(x.dim() == 2, "fp8_quant_cols_t: x must be [R, C]");
  const long R = x.size(0);
  const long C = x.size(1);
  TORCH_CHECK(R >= 1, "fp8_quant_cols_t: R must be at least 1");
  TORCH_CHECK(C > 0 && C % FP8_QUANT_VEC == 0 && C <= 65535L * FP8_COLS_TC,
              "fp8_quant_cols_t: C must be a positive multiple of ", FP8_QUANT_VEC);
  TORCH_CHECK((R + FP8_COLS_TR - 1) / FP8_COLS_TR <= INT_MAX, "fp8_quant_cols_t: R too large");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0, "fp8_quant_cols_t: x must be 16-byte aligned");
  const long Rp = (R + FP8_COLS_TR - 1) / FP8_COLS_TR * FP8_COLS_TR;
  const int np = fp8_cols_partials(R, (int)C);
  auto fopt = x.options().dtype(torch::kFloat);
  auto q = torch::empty({C, Rp}, x.options().dtype(torch::kUInt8));
  auto scale = torch::empty({C}, fopt);
  auto sums = torch::empty({colsum ? C : 0}, fopt);
  auto part = torch::empty({colsum ? 2 : 1, (long)np, C}, fopt);
  float* part_amax = part.data_ptr<float>();
  launch_fp8_quant_cols_t((const __hip_bfloat16*)x.data_ptr(), q.data_ptr<uint8_t>(),
                          scale.data_ptr<float>(), colsum ? sums.data_ptr<float>() : nullptr,
                          part_amax, colsum ? part_amax + (long)np * C : nullptr, R, (int)C,
                          (int)fmt, current_stream());
  return {q, scale, sums};
}

// fp32 column sums [C] of bf16 [R,C], by pass 1 of the column quantiser alone
// (the bias gradient when no weight gradient is wanted).
torch::Tensor fp8_colsum(torch::Tensor x) {
  CHECK_INPUT(x);
  TORCH_CHECK(x.scalar_type() == at::ScalarType::BFloat16, "fp8_colsum: x must be bf16");
  TORCH_CHECK(x.dim() == 2, "fp8_colsum: x must be [R, C]");
  const long R = x.size(0);
  const long C = x.size(1);
  TORCH_CHECK(R >= 1, "fp8_colsum: R must be at least 1");
  TORCH_CHECK(C > 0 && C % FP8_QUANT_VEC == 0 && C <= 65535L * FP8_COLS_TC,
              "fp8_colsum: C must be a positive multiple of ", FP8_QUANT_VEC);
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0, "fp8_colsum: x must be 16-byte aligned");
  const int np = fp8_cols_partials(R, (int)C);
  auto fopt = x.options().dtype(torch::kFloat);
  auto sums = torch::empty({C}, fopt);
  auto part = torch::empty({2, (long)np, C}, fopt);
  float* part_amax = part.data_ptr<float>();
  launch_fp8_quant_cols_t((const __hip_bfloat16*)x.data_ptr(), nullptr, nullptr,
                          sums.data_ptr<float>(), part_amax, part_amax + (long)np * C, R, (int)C,
                          FP8_FMT_E4M3, current_stream());
  return sums;
}

// y[M,N] = bf16((xq . wq^T) * sx[m] * sw[n] + bias[n]); xq [M,K] fp8 bytes of format
// fmt_x (e4m3 by default; e5m2 for the backward GEMMs, without bias), wq [N,K] e4m3fn bytes.
torch::Tensor fp8_gemm_nt(torch::Tensor xq, torch::Tensor sx, torch::Tensor wq,
                          torch::Tensor sw, c10::optional<torch::Tensor> bias, int64_t fmt_x) {
  CHECK_INPUT(xq);
  CHECK_FP8_FMT(fmt_x, "fp8_gemm_nt");
  TORCH_CHECK(fmt_x == FP8_FMT_E4M3 || !(bias.has_value() && bias->defined()),
              "fp8_gemm_nt: no bias with an e5m2 first operand");
  CHECK_INPUT(sx);
  CHECK_INPUT(wq);
  CHECK_INPUT(sw);
  TORCH_CHECK(xq.scalar_type() == at::ScalarType::Byte && wq.scalar_type() == at::ScalarType::Byte,
              "fp8_gemm_nt: operands are fp8 bytes viewed as uint8");
  TORCH_CHECK(sx.scalar_type() == at::ScalarType::Float && sw.scalar_type() == at::ScalarType::Float,
              "fp8_gemm_nt: scales must be fp32");
  TORCH_CHECK(xq.dim() == 2 && wq.dim() == 2 && xq.size(1) == wq.size(1),
              "fp8_gemm_nt: xq [M,K] and wq [N,K] must share K");
  const long M = xq.size(0);
  const long N = wq.size(0);
  const long K = xq.size(1);
  TORCH_CHECK(K > 0 && K % FP8_GEMM_BK == 0 && K <= INT_MAX,
              "fp8_gemm_nt: K must be a positive multiple of ", FP8_GEMM_BK);
  TORCH_CHECK(N > 0 && N % FP8_GEMM_N_ALIGN == 0 && N <= INT_MAX,
              "fp8_gemm_nt: N must be a positive multiple of ", FP8_GEMM_N_ALIGN);
  TORCH_CHECK(sx.numel() == M && sw.numel() == N, "fp8_gemm_nt: one scale per row");
  TORCH_CHECK((uintptr_t)xq.data_ptr() % 16 == 0 && (uintptr_t)wq.data_ptr() % 16 == 0 &&
                  (uintptr_t)sw.data_ptr() % 16 == 0,
              "fp8_gemm_nt: operands must be 16-byte aligned");
  const __hip_bfloat16* bias_ptr = nullptr;
  torch::Tensor b;
  if (bias.has_value() && bias->defined()) {
    b = *bias;
    CHECK_INPUT(b);
    TORCH_CHECK(b.scalar_type() == at::ScalarType::BFloat16 && b.numel() == N,
                "fp8_gemm_nt: bias must be bf16 [N]");
    if ((uintptr_t)b.data_ptr() % 8 != 0) b = b.clone();
    bias_ptr = (const __hip_bfloat16*)b.data_ptr();
  }
  auto y = torch::empty({M, N}, xq.options().dtype(torch::kBFloat16));
  launch_fp8_gemm_nt(xq.data_ptr<uint8_t>(), sx.data_ptr<float>(), wq.data_ptr<uint8_t>(),
                     sw.data_ptr<float>(), bias_ptr, (__hip_bfloat16*)y.data_ptr(), M, (int)N,
                     (int)K, (int)fmt_x, current_stream());
  return y;
}

// One-wave lane-map probe: c[16,16] = a[16,128] . bt[16,128]^T on fp8 bytes of
// formats fmt_a and fmt_b (e4m3 by default).
torch::Tensor probe_mfma_fp8(torch::Tensor a, torch::Tensor bt, int64_t fmt_a, int64_t fmt_b) {
  CHECK_INPUT(a);
  CHECK_INPUT(bt);
  CHECK_FP8_FMT(fmt_a, "probe_mfma_fp8");
  CHECK_FP8_FMT(fmt_b, "probe_mfma_fp8");
  TORCH_CHECK(a.scalar_type() == at::ScalarType::Byte && bt.scalar_type() == at::ScalarType::Byte);
  TORCH_CHECK(a.dim() == 2 && a.size(0) == 16 && a.size(1) == FP8_GEMM_BK &&
                  bt.dim() == 2 && bt.size(0) == 16 && bt.size(1) == FP8_GEMM_BK,
              "probe_mfma_fp8: a and bt must be [16, ", FP8_GEMM_BK, "]");
  auto c = torch::empty({16, 16}, a.options().dtype(torch::kFloat));
  launch_probe_mfma_fp8(a.data_ptr<uint8_t>(), bt.data_ptr<uint8_t>(), c.data_ptr<float>(),
                        (int)fmt_a, (int)fmt_b, current_stream());
  return c;
}

// ------------------------------- k-NN -----------------------------------

// (val [Q,k] fp32, idx [Q,k] int32): the k largest dot products of every row of
// q [Q,D] with the rows of bank [N,D], ordered by (value descending, bank row
// ascending). splits: slices of the bank along N; 0 lets the kernel choose.
std::vector<torch::Tensor> knn_topk(torch::Tensor q, torch::Tensor bank, int64_t k,
                                    int64_t splits) {
  CHECK_INPUT(q);
  CHECK_INPUT(bank);
  TORCH_CHECK(q.scalar_type() == at::ScalarType::BFloat16 &&
                  bank.scalar_type() == at::ScalarType::BFloat16,
              "knn_topk: q and bank must be bf16");
  TORCH_CHECK(q.dim() == 2 && bank.dim() == 2, "knn_topk: q must be [Q, D] and bank [N, D]");
  TORCH_CHECK(q.device() == bank.device(), "knn_topk: q and bank must be on one device");
  const long Q = q.size(0);
  const long N = bank.size(0);
  const long D = q.size(1);
  TORCH_CHECK(bank.size(1) == D, "knn_topk: q and bank must share D, got ", D, " and ",
              bank.size(1));
  TORCH_CHECK(D > 0 && D % 32 == 0 && D <= INT_MAX, "knn_topk: D must be a positive multiple of 32");
  TORCH_CHECK(N < (1L << 31), "knn_topk: N must be below 2^31");
  TORCH_CHECK(k >= 1 && k <= 256 && k <= N, "knn_topk: need 1 <= k <= min(N, 256), got k = ", k,
              " with N = ", N);
  TORCH_CHECK(splits >= 0 && splits <= 1024, "knn_topk: splits must be in [0, 1024]");
  TORCH_CHECK((uintptr_t)q.data_ptr() % 16 == 0 && (uintptr_t)bank.data_ptr() % 16 == 0,
              "knn_topk: q and bank must be 16-byte aligned");
  auto val = torch::empty({Q, (long)k}, q.options().dtype(torch::kFloat));
  auto idx = torch::empty({Q, (long)k}, q.options().dtype(torch::kInt));
  if (Q == 0) return {val, idx};
  const int ns = splits > 0 ? (int)splits : knn_topk_auto_splits(Q, N);
  torch::Tensor ws;
  unsigned long long* ws_ptr = nullptr;
  if (ns > 1) {
    ws = torch::empty({(long)ns, Q, (long)k}, q.options().dtype(torch::kLong));
    ws_ptr = (unsigned long long*)ws.data_ptr();
  }
  launch_knn_topk((const __hip_bfloat16*)q.data_ptr(), (const __hip_bfloat16*)bank.data_ptr(),
                  ws_ptr, val.data_ptr<float>(), idx.data_ptr<int>(), Q, N, (int)D, (int)k, ns,
                  current_stream());
  return {val, idx};
}

// Softmax cross-entropy of logits [B, G, Cp] (+ bias [G, Cp]) against labels [B]
// over the first C columns, for G heads at once. Returns (loss_sum [G] fp32,
// correct [G] int64) and, with write_grad, dbias [G, Cp] fp32 after the row
// gradients (softmax - onehot) * grad_scale have replaced the logits in place.
// label -1 marks an ignored row. row_blocks: blocks per head, 0 = chosen.
std::vector<torch::Tensor> probe_ce(torch::Tensor logits, c10::optional<torch::Tensor> bias,
                                    torch::Tensor labels, int64_t C, double grad_scale,
                                    bool write_grad, int64_t row_blocks) {
  CHECK_INPUT(logits);
  CHECK_INPUT(labels);
  TORCH_CHECK(logits.dim() == 3, "probe_ce: logits must be [B, G, Cp]");
  TORCH_CHECK(logits.scalar_type() == at::ScalarType::BFloat16 ||
                  logits.scalar_type() == at::ScalarType::Float,
              "probe_ce: logits must be bf16 or fp32");
  TORCH_CHECK(labels.scalar_type() == at::ScalarType::Long && labels.dim() == 1 &&
                  labels.size(0) == logits.size(0),
              "probe_ce: labels must be int64 [B]");
  TORCH_CHECK(labels.device() == logits.device(), "probe_ce: labels and logits must be on one device");
  const long B = logits.size(0);
  const long G = logits.size(1);
  const long Cp = logits.size(2);
  TORCH_CHECK(Cp > 0 && Cp % 8 == 0 && Cp <= 2048,
              "probe_ce: Cp must be a positive multiple of 8 and at most 2048, got ", Cp);
  TORCH_CHECK(C >= 1 && C <= Cp, "probe_ce: need 1 <= C <= Cp, got C = ", C, ", Cp = ", Cp);
  TORCH_CHECK(G >= 1 && G <= 65535, "probe_ce: G must be in [1, 65535], got ", G);
  TORCH_CHECK(B < (1L << 24), "probe_ce: B must be below 2^24 (counts travel as fp32)");
  TORCH_CHECK(row_blocks >= 0, "probe_ce: row_blocks must be >= 0");
  TORCH_CHECK((uintptr_t)logits.data_ptr() % 16 == 0, "probe_ce: logits must be 16-byte aligned");
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    const torch::Tensor& b = *bias;
    CHECK_INPUT(b);
    TORCH_CHECK(b.scalar_type() == at::ScalarType::Float && b.dim() == 2 && b.size(0) == G &&
                    b.size(1) == Cp,
                "probe_ce: bias must be fp32 [G, Cp]");
    TORCH_CHECK(b.device() == logits.device(), "probe_ce: bias and logits must be on one device");
    TORCH_CHECK((uintptr_t)b.data_ptr() % 16 == 0, "probe_ce: bias must be 16-byte aligned");
    bias_ptr = b.data_ptr<float>();
  }
  int ws_cols, tail;
  probe_ce_layout((int)G, (int)Cp, write_grad, &ws_cols, &tail);
  auto fopts = logits.options().dtype(torch::kFloat);
  if (B == 0) {
    std::vector<torch::Tensor> ret = {torch::zeros({G}, fopts),
                                      torch::zeros({G}, fopts.dtype(torch::kLong))};
    if (write_grad) ret.push_back(torch::zeros({G, Cp}, fopts));
    return ret;
  }
  const int nblk = probe_ce_row_blocks(B, (int)G, (int)std::min<int64_t>(row_blocks, INT_MAX));
  auto ws = torch::empty({(long)nblk, (long)ws_cols}, fopts);
  auto out = torch::empty({(long)ws_cols}, fopts);
  if (logits.scalar_type() == at::ScalarType::Float)
    launch_probe_ce<float>(logits.data_ptr<float>(), bias_ptr, labels.data_ptr<long>(),
                           ws.data_ptr<float>(), out.data_ptr<float>(), B, (int)G, (int)Cp, (int)C,
                           (float)grad_scale, write_grad, nblk, current_stream());
  else
    launch_probe_ce<__hip_bfloat16>((__hip_bfloat16*)logits.data_ptr(), bias_ptr,
                                    labels.data_ptr<long>(), ws.data_ptr<float>(),
                                    out.data_ptr<float>(), B, (int)G, (int)Cp, (int)C,
                                    (float)grad_scale, write_grad, nblk, current_stream());
  std::vector<torch::Tensor> ret = {out.narrow(0, tail, G),
                                    out.narrow(0, tail + G, G).to(torch::kLong)};
  if (write_grad) ret.push_back(out.narrow(0, 0, G * Cp).view({G, Cp}));
  return ret;
}

// In-place SGD with momentum on w, mom [G, R] fp32 from grad [G, R] (bf16 | fp32):
// g' = grad + wd[g] w; mom = momentum mom + g'; w -= lr[g] lr_scale mom; with
// w_lp [G, R] bf16 also w_lp = bf16(w).
void probe_sgd_(torch::Tensor w, torch::Tensor mom, torch::Tensor grad, torch::Tensor lr,
                c10::optional<torch::Tensor> wd, double lr_scale, double momentum,
                c10::optional<torch::Tensor> w_lp) {
  CHECK_INPUT(w);
  CHECK_INPUT(mom);
  CHECK_INPUT(grad);
  CHECK_INPUT(lr);
  TORCH_CHECK(w.dim() == 2 && w.scalar_type() == at::ScalarType::Float, "probe_sgd_: w must be fp32 [G, R]");
  TORCH_CHECK(mom.scalar_type() == at::ScalarType::Float && mom.sizes() == w.sizes(),
              "probe_sgd_: mom must be fp32 and shaped like w");
  TORCH_CHECK((grad.scalar_type() == at::ScalarType::Float ||
               grad.scalar_type() == at::ScalarType::BFloat16) && grad.sizes() == w.sizes(),
              "probe_sgd_: grad must be bf16 or fp32 and shaped like w");
  const long G = w.size(0);
  const long R = w.size(1);
  TORCH_CHECK(R % 8 == 0, "probe_sgd_: R must be a multiple of 8, got ", R);
  TORCH_CHECK(G <= 65535, "probe_sgd_: G must be at most 65535, got ", G);
  TORCH_CHECK(lr.scalar_type() == at::ScalarType::Float && lr.dim() == 1 && lr.size(0) == G,
              "probe_sgd_: lr must be fp32 [G]");
  TORCH_CHECK(mom.device() == w.device() && grad.device() == w.device() && lr.device() == w.device(),
              "probe_sgd_: all tensors must be on one device");
  TORCH_CHECK((uintptr_t)w.data_ptr() % 16 == 0 && (uintptr_t)mom.data_ptr() % 16 == 0 &&
                  (uintptr_t)grad.data_ptr() % 16 == 0,
              "probe_sgd_: w, mom and grad must be 16-byte aligned");
  const float* wd_ptr = nullptr;
  if (wd.has_value()) {
    const torch::Tensor& d = *wd;
    CHECK_INPUT(d);
    TORCH_CHECK(d.scalar_type() == at::ScalarType::Float && d.dim() == 1 && d.size(0) == G &&
                    d.device() == w.device(),
                "probe_sgd_: wd must be fp32 [G] on w's device");
    wd_ptr = d.data_ptr<float>();
  }
  __hip_bfloat16* lp_ptr = nullptr;
  if (w_lp.has_value()) {
    const torch::Tensor& l = *w_lp;
    CHECK_INPUT(l);
    TORCH_CHECK(l.scalar_type() == at::ScalarType::BFloat16 && l.sizes() == w.sizes() &&
                    l.device() == w.device(),
                "probe_sgd_: w_lp must be bf16, shaped like w, on w's device");
    TORCH_CHECK((uintptr_t)l.data_ptr() % 16 == 0, "probe_sgd_: w_lp must be 16-byte aligned");
    lp_ptr = (__hip_bfloat16*)l.data_ptr();
  }
  if (G == 0 || R == 0) return;
  if (grad.scalar_type() == at::ScalarType::Float)
    launch_probe_sgd<float>(w.data_ptr<float>(), mom.data_ptr<float>(), grad.data_ptr<float>(),
                            lr.data_ptr<float>(), wd_ptr, lp_ptr, (int)G, R, (float)lr_scale,
                            (float)momentum, current_stream());
  else
    launch_probe_sgd<__hip_bfloat16>(w.data_ptr<float>(), mom.data_ptr<float>(),
                                     (const __hip_bfloat16*)grad.data_ptr(), lr.data_ptr<float>(),
                                     wd_ptr, lp_ptr, (int)G, R, (float)lr_scale, (float)momentum,
                                     current_stream());
}

// Linear segmentation probe: logits [M, h, w, G, Cp] (+ bias [G, Cp]) upsampled
// bilinearly (align_corners = False) by the even factor s = H / h = W / w to the
// labels [M, H, W] uint8, softmax cross-entropy over the first C columns per
// pixel, 255 = ignored. Returns (loss_sum [G] fp32, areas [G, 3, Cp] int64:
// intersection, prediction and label counts) and, with write_grad, dbias [G, Cp]
// fp32 after the gradient with respect to the logits, times grad_scale (times
// scale[0] when the one-element device tensor `scale` is given), has replaced
// them in place.
std::vector<torch::Tensor> seg_ce(torch::Tensor logits, c10::optional<torch::Tensor> bias,
                                  torch::Tensor labels, int64_t C, double grad_scale,
                                  bool write_grad, c10::optional<torch::Tensor> scale) {
  CHECK_INPUT(logits);
  CHECK_INPUT(labels);
  TORCH_CHECK(logits.dim() == 5, "seg_ce: logits must be [M, h, w, G, Cp]");
  TORCH_CHECK(logits.scalar_type() == at::ScalarType::BFloat16 ||
                  logits.scalar_type() == at::ScalarType::Float,
              "seg_ce: logits must be bf16 or fp32");
  TORCH_CHECK(labels.scalar_type() == at::ScalarType::Byte && labels.dim() == 3 &&
                  labels.size(0) == logits.size(0),
              "seg_ce: labels must be uint8 [M, H, W]");
  TORCH_CHECK(labels.device() == logits.device(), "seg_ce: labels and logits must be on one device");
  const long M = logits.size(0), h = logits.size(1), w = logits.size(2);
  const long G = logits.size(3), Cp = logits.size(4);
  const long H = labels.size(1), W = labels.size(2);
  TORCH_CHECK(h >= 1 && w >= 1 && h <= 4096 && w <= 4096, "seg_ce: h and w must be in [1, 4096]");
  const long s = H / h;
  TORCH_CHECK(H == s * h && W == s * w, "seg_ce: need H = s h and W = s w with one integer s, got ",
              H, " x ", W, " labels for ", h, " x ", w, " cells");
  TORCH_CHECK(s % 2 == 0 && s >= 2 && s <= SEG_MAX_SCALE, "seg_ce: the scale must be even and in [2, ",
              SEG_MAX_SCALE, "], got ", s);
  TORCH_CHECK(Cp > 0 && Cp % 8 == 0 && Cp <= SEG_MAX_CP,
              "seg_ce: Cp must be a positive multiple of 8 and at most ", SEG_MAX_CP, ", got ", Cp);
  TORCH_CHECK(C >= 1 && C <= Cp && C <= SEG_MAX_CLASSES, "seg_ce: need 1 <= C <= min(Cp, ",
              SEG_MAX_CLASSES, "), got C = ", C, ", Cp = ", Cp);
  TORCH_CHECK(G >= 1 && G <= 65535, "seg_ce: G must be in [1, 65535], got ", G);
  TORCH_CHECK(M * H * W < (1L << 31), "seg_ce: M H W must be below 2^31 (block counts are int32)");
  TORCH_CHECK(G * Cp <= INT_MAX, "seg_ce: G Cp must fit an int");
  TORCH_CHECK((uintptr_t)logits.data_ptr() % 16 == 0, "seg_ce: logits must be 16-byte aligned");
  // the labels are read a byte at a time: a slice of images needs no alignment
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    const torch::Tensor& b = *bias;
    CHECK_INPUT(b);
    TORCH_CHECK(b.scalar_type() == at::ScalarType::Float && b.dim() == 2 && b.size(0) == G &&
                    b.size(1) == Cp,
                "seg_ce: bias must be fp32 [G, Cp]");
    TORCH_CHECK(b.device() == logits.device(), "seg_ce: bias and logits must be on one device");
    TORCH_CHECK((uintptr_t)b.data_ptr() % 16 == 0, "seg_ce: bias must be 16-byte aligned");
    bias_ptr = b.data_ptr<float>();
  }
  const float* scale_ptr = nullptr;
  if (scale.has_value()) {
    const torch::Tensor& sc = *scale;
    CHECK_INPUT(sc);
    TORCH_CHECK(sc.scalar_type() == at::ScalarType::Float && sc.numel() == 1 &&
                    sc.device() == logits.device(),
                "seg_ce: scale must be one fp32 value on the logits' device");
    scale_ptr = sc.data_ptr<float>();
  }
  auto fopts = logits.options().dtype(torch::kFloat);
  if (M == 0) {
    std::vector<torch::Tensor> ret = {torch::zeros({G}, fopts),
                                      torch::zeros({G, 3, Cp}, fopts.dtype(torch::kLong))};
    if (write_grad) ret.push_back(torch::zeros({G, Cp}, fopts));
    return ret;
  }
  const long quads = M * h * w;
  const int nblk = seg_ce_quad_blocks(quads, (int)G);
  auto loss = torch::empty({G}, fopts);
  auto areas = torch::empty({G, 3, Cp}, fopts.dtype(torch::kLong));
  auto part_loss = torch::empty({(long)nblk, G}, fopts);
  auto part_area = torch::empty({(long)nblk, G, 3, Cp}, fopts.dtype(torch::kInt));
  torch::Tensor ws, part_db, dbias;
  if (write_grad) {
    ws = torch::empty({quads, 4, G, Cp}, fopts);
    part_db = torch::empty({(long)seg_ce_fin_rows(quads), G * Cp}, fopts);
    dbias = torch::empty({G, Cp}, fopts);
  }
  float* ws_ptr = write_grad ? ws.data_ptr<float>() : nullptr;
  float* pdb_ptr = write_grad ? part_db.data_ptr<float>() : nullptr;
  float* db_ptr = write_grad ? dbias.data_ptr<float>() : nullptr;
  if (logits.scalar_type() == at::ScalarType::Float)
    launch_seg_ce<float>(logits.data_ptr<float>(), bias_ptr, labels.data_ptr<uint8_t>(), ws_ptr,
                         part_loss.data_ptr<float>(), part_area.data_ptr<int>(), pdb_ptr,
                         loss.data_ptr<float>(), areas.data_ptr<long>(), db_ptr, scale_ptr, M,
                         (int)h, (int)w, (int)s, (int)G, (int)Cp, (int)C, (float)grad_scale,
                         write_grad, nblk, current_stream());
  else
    launch_seg_ce<__hip_bfloat16>((__hip_bfloat16*)logits.data_ptr(), bias_ptr,
                                  labels.data_ptr<uint8_t>(), ws_ptr, part_loss.data_ptr<float>(),
                                  part_area.data_ptr<int>(), pdb_ptr, loss.data_ptr<float>(),
                                  areas.data_ptr<long>(), db_ptr, scale_ptr, M, (int)h, (int)w,
                                  (int)s, (int)G, (int)Cp, (int)C, (float)grad_scale, write_grad,
                                  nblk, current_stream());
  std::vector<torch::Tensor> ret = {loss, areas};
  if (write_grad) ret.push_back(dbias);
  return ret;
}

// ------------------------------ Gram loss --------------------------------
// The pieces of ops.gram_loss (gram_loss.hip); the panel loop and the P @ S
// GEMM between them are in ops/gram_loss.py.

constexpr long kGramTile = 128;

void check_gram_inputs(const torch::Tensor& student, const torch::Tensor& teacher) {
  CHECK_INPUT(student);
  CHECK_INPUT(teacher);
  TORCH_CHECK(student.scalar_type() == at::ScalarType::BFloat16 &&
                  teacher.scalar_type() == at::ScalarType::BFloat16,
              "gram_loss: student and teacher must be bf16");
  TORCH_CHECK(student.dim() == 3, "gram_loss: student must be [G, M, D]");
  TORCH_CHECK(teacher.sizes() == student.sizes(), "gram_loss: student and teacher must have one "
              "shape, got ", student.sizes(), " and ", teacher.sizes());
  TORCH_CHECK(student.device() == teacher.device(),
              "gram_loss: student and teacher must be on one device");
  const long G = student.size(0), M = student.size(1), D = student.size(2);
  TORCH_CHECK(G >= 1 && M >= 1, "gram_loss: need G >= 1 and M >= 1");
  TORCH_CHECK(D >= 8 && D % 8 == 0 && D <= (1 << 20),
              "gram_loss: D must be a positive multiple of 8, got ", D);
  TORCH_CHECK(M <= (1L << 30) && G * M <= (1L << 40), "gram_loss: M or G M too large");
  TORCH_CHECK((uintptr_t)student.data_ptr() % 16 == 0 && (uintptr_t)teacher.data_ptr() % 16 == 0,
              "gram_loss: student and teacher must be 16-byte aligned");
}

// r [2, G M] fp32: rsqrt of the squared row norms of student (0) and teacher
// (1), or ones without apply_norm.
torch::Tensor gram_rnorm(torch::Tensor student, torch::Tensor teacher, bool apply_norm) {
  check_gram_inputs(student, teacher);
  const long rows = student.size(0) * student.size(1);
  auto r = torch::empty({2, rows}, student.options().dtype(torch::kFloat));
  launch_gram_rnorm((const __hip_bfloat16*)student.data_ptr(),
                    (const __hip_bfloat16*)teacher.data_ptr(), r.data_ptr<float>(), rows,
                    (int)student.size(2), apply_norm, current_stream());
  return r;
}

// Row tiles tile0 .. tile0 + ntiles - 1 (of the G * nT row tiles of 128 rows,
// nT = ceil(M / 128)) of both similarity matrices: their loss partials go to
// partials [G * nT * nT] and, with a panel [>= ntiles * 128, nT * 128] bf16,
// P = e * mask * r_j of those rows to it. mode: 0 plain, 1 remove_neg,
// 2 remove_only_teacher_neg.
void gram_tiles(torch::Tensor student, torch::Tensor teacher, torch::Tensor r, int64_t mode,
                int64_t tile0, int64_t ntiles, c10::optional<torch::Tensor> panel,
                torch::Tensor partials) {
  check_gram_inputs(student, teacher);
  const long G = student.size(0), M = student.size(1), D = student.size(2);
  const long nT = (M + kGramTile - 1) / kGramTile;
  CHECK_INPUT(r);
  CHECK_INPUT(partials);
  TORCH_CHECK(r.scalar_type() == at::ScalarType::Float && r.dim() == 2 && r.size(0) == 2 &&
                  r.size(1) == G * M && r.device() == student.device(),
              "gram_tiles: r must be fp32 [2, G M] on the inputs' device");
  TORCH_CHECK(partials.scalar_type() == at::ScalarType::Float && partials.numel() == G * nT * nT &&
                  partials.device() == student.device(),
              "gram_tiles: partials must be fp32 with G nT nT elements on the inputs' device");
  TORCH_CHECK(mode >= 0 && mode <= 2, "gram_tiles: mode must be 0, 1 or 2");
  TORCH_CHECK(ntiles >= 1 && ntiles <= 65535 && tile0 >= 0 && tile0 + ntiles <= G * nT,
              "gram_tiles: row tiles [", tile0, ", ", tile0 + ntiles, ") are not inside [0, ",
              G * nT, ") or are more than 65535");
  __hip_bfloat16* p_ptr = nullptr;
  if (panel.has_value()) {
    const torch::Tensor& p = panel.value();
    CHECK_INPUT(p);
    TORCH_CHECK(p.scalar_type() == at::ScalarType::BFloat16 && p.dim() == 2 &&
                    p.size(0) >= ntiles * kGramTile && p.size(1) == nT * kGramTile &&
                    p.device() == student.device(),
                "gram_tiles: panel must be bf16 [>= ntiles * 128, nT * 128] on the inputs' device");
    TORCH_CHECK((uintptr_t)p.data_ptr() % 16 == 0, "gram_tiles: panel must be 16-byte aligned");
    p_ptr = (__hip_bfloat16*)p.data_ptr();
  }
  launch_gram_tiles((const __hip_bfloat16*)student.data_ptr(),
                    (const __hip_bfloat16*)teacher.data_ptr(), r.data_ptr<float>(),
                    r.data_ptr<float>() + G * M, p_ptr, partials.data_ptr<float>(), (int)M, (int)D,
                    (int)mode, tile0, (int)ntiles, current_stream());
}

// loss (0-dim fp32) = sum of the partials in a fixed order / count.
torch::Tensor gram_finish(torch::Tensor partials, double count) {
  CHECK_INPUT(partials);
  TORCH_CHECK(partials.scalar_type() == at::ScalarType::Float && partials.numel() >= 1,
              "gram_finish: partials must be fp32 and not empty");
  TORCH_CHECK(count >= 1.0, "gram_finish: count must be at least 1");
  auto loss = torch::empty({}, partials.options());
  launch_gram_finish(partials.data_ptr<float>(), loss.data_ptr<float>(), partials.numel(), count,
                     current_stream());
  return loss;
}

// dS [G, M, D] bf16 from Draw = P @ S: c r_i (Draw_i - s^_i (s^_i . Draw_i)),
// or c Draw_i without apply_norm.
torch::Tensor gram_norm_bwd(torch::Tensor draw, torch::Tensor student, torch::Tensor r, double c,
                            bool apply_norm) {
  check_gram_inputs(student, draw);
  CHECK_INPUT(r);
  const long rows = student.size(0) * student.size(1);
  TORCH_CHECK(r.scalar_type() == at::ScalarType::Float && r.dim() == 2 && r.size(0) == 2 &&
                  r.size(1) == rows && r.device() == student.device(),
              "gram_norm_bwd: r must be fp32 [2, G M] on the inputs' device");
  auto ds = torch::empty_like(student);
  launch_gram_norm_bwd((const __hip_bfloat16*)draw.data_ptr(),
                       (const __hip_bfloat16*)student.data_ptr(), r.data_ptr<float>(),
                       (__hip_bfloat16*)ds.data_ptr(), rows, (int)student.size(2), (float)c,
                       apply_norm, current_stream());
  return ds;
}

}  // namespace

// hipBLASLt fused-epilogue entry points (blaslt_ext.hip)
std::vector<torch::Tensor> blaslt_gemm_bias_gelu_fwd(torch::Tensor x, torch::Tensor w,
                                                     torch::Tensor bias);
std::vector<torch::Tensor> blaslt_gemm_dgelu_bgrad(torch::Tensor dy, torch::Tensor w2,
                                                   torch::Tensor pre);
torch::Tensor blaslt_gemm_bias(torch::Tensor x, torch::Tensor w, torch::Tensor bias);
int64_t blaslt_probe_epilogue(int64_t epi, int64_t aux_type, int64_t bias_type,
                              int64_t m, int64_t n, int64_t k);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("blaslt_gemm_bias_gelu_fwd", &blaslt_gemm_bias_gelu_fwd);
  mod.def("blaslt_gemm_dgelu_bgrad", &blaslt_gemm_dgelu_bgrad);
  mod.def("blaslt_gemm_bias", &blaslt_gemm_bias);
  mod.def("blaslt_probe_epilogue", &blaslt_probe_epilogue);
  mod.def("layernorm_fwd", &layernorm_fwd);
  mod.def("layernorm_bwd", &layernorm_bwd);
  mod.def("gather_layernorm_fwd", &gather_layernorm_fwd);
  mod.def("layernorm_bwd_scatter_acc_", &layernorm_bwd_scatter_acc_);
  mod.def("rmsnorm_fwd", &rmsnorm_fwd);
  mod.def("rmsnorm_bwd", &rmsnorm_bwd);
  mod.def("l2norm_fwd", &l2norm_fwd);
  mod.def("l2norm_bwd", &l2norm_bwd);
  mod.def("bias_gelu_fwd", &bias_gelu_fwd);
  mod.def("bias_gelu_bwd", &bias_gelu_bwd);
  mod.def("row_gather", &row_gather);
  mod.def("row_scatter_add_", &row_scatter_add_);
  mod.def("row_gather_scaled", &row_gather_scaled);
  mod.def("ls_axpy_fwd", &ls_axpy_fwd);
  mod.def("ls_axpy_bias_fwd", &ls_axpy_bias_fwd);
  mod.def("ls_axpy_bias_bwd", &ls_axpy_bias_bwd);
  mod.def("ls_scatter_add_", &ls_scatter_add_);
  mod.def("ls_scatter_bwd", &ls_scatter_bwd);
  mod.def("ls_axpy_bwd", &ls_axpy_bwd);
  mod.def("swiglu_fwd", &swiglu_fwd);
  mod.def("swiglu_bwd", &swiglu_bwd);
  mod.def("rope_fwd", &rope_fwd);
  mod.def("probe_mfma", &probe_mfma);
  mod.def("fp8_quant_rows", &fp8_quant_rows, py::arg("x"), py::arg("fmt") = FP8_FMT_E4M3);
  mod.def("fp8_quant_cols_t", &fp8_quant_cols_t, py::arg("x"), py::arg("fmt") = FP8_FMT_E4M3,
          py::arg("colsum") = false);
  mod.def("fp8_colsum", &fp8_colsum, py::arg("x"));
  mod.def("fp8_gemm_nt", &fp8_gemm_nt, py::arg("xq"), py::arg("sx"), py::arg("wq"), py::arg("sw"),
          py::arg("bias"), py::arg("fmt_x") = FP8_FMT_E4M3);
  mod.def("probe_mfma_fp8", &probe_mfma_fp8, py::arg("a"), py::arg("bt"),
          py::arg("fmt_a") = FP8_FMT_E4M3, py::arg("fmt_b") = FP8_FMT_E4M3);
  mod.def("patch_embed_fwd", &patch_embed_fwd);
  mod.def("dino_ce_fwd", &dino_ce_fwd);
  mod.def("dino_ce_bwd", &dino_ce_bwd);
  mod.def("ibot_ce_fwd", &ibot_ce_fwd);
  mod.def("ibot_ce_bwd", &ibot_ce_bwd);
  mod.def("sinkhorn_exp", &sinkhorn_exp);
  mod.def("sinkhorn_fact_colsum", &sinkhorn_fact_colsum);
  mod.def("sinkhorn_fact_rowsum", &sinkhorn_fact_rowsum);
  mod.def("ibot_ce_fact_fwd", &ibot_ce_fact_fwd);
  mod.def("ibot_ce_fact_bwd", &ibot_ce_fact_bwd);
  mod.def("dino_ce_fact_fwd", &dino_ce_fact_fwd);
  mod.def("dino_ce_fact_bwd", &dino_ce_fact_bwd);
  mod.def("sinkhorn_colsum", &sinkhorn_colsum);
  mod.def("sinkhorn_div_row", &sinkhorn_div_row);
  mod.def("knn_topk", &knn_topk, py::arg("q"), py::arg("bank"), py::arg("k"),
          py::arg("splits") = 0);
  mod.def("probe_ce", &probe_ce, py::arg("logits"), py::arg("bias"), py::arg("labels"),
          py::arg("C"), py::arg("grad_scale"), py::arg("write_grad"), py::arg("row_blocks") = 0);
  mod.def("probe_sgd_", &probe_sgd_, py::arg("w"), py::arg("mom"), py::arg("grad"), py::arg("lr"),
          py::arg("wd"), py::arg("lr_scale"), py::arg("momentum"), py::arg("w_lp"));
  mod.def("seg_ce", &seg_ce, py::arg("logits"), py::arg("bias"), py::arg("labels"), py::arg("C"),
          py::arg("grad_scale"), py::arg("write_grad"), py::arg("scale") = py::none());
  mod.attr("SEG_MAX_CLASSES") = SEG_MAX_CLASSES;
  mod.def("gram_rnorm", &gram_rnorm, py::arg("student"), py::arg("teacher"),
          py::arg("apply_norm"));
  mod.def("gram_tiles", &gram_tiles, py::arg("student"), py::arg("teacher"), py::arg("r"),
          py::arg("mode"), py::arg("tile0"), py::arg("ntiles"), py::arg("panel"),
          py::arg("partials"));
  mod.def("gram_finish", &gram_finish, py::arg("partials"), py::arg("count"));
  mod.def("gram_norm_bwd", &gram_norm_bwd, py::arg("draw"), py::arg("student"), py::arg("r"),
          py::arg("c"), py::arg("apply_norm"));
  mod.def("fmha_fwd", &fmha_fwd);
  mod.def("fmha_rope_fwd", [](torch::Tensor qkv, torch::Tensor sin_t, torch::Tensor cos_t,
                              int64_t prefix) {
    return fmha_rope_fwd_out(qkv, sin_t, cos_t, prefix, torch::Tensor());
  });
  mod.def("fmha_rope_fwd_out", &fmha_rope_fwd_out);
  mod.def("fmha_rope_bwd", [](torch::Tensor dout, torch::Tensor qkv, torch::Tensor o,
                              torch::Tensor lse, torch::Tensor sin_t, torch::Tensor cos_t,
                              int64_t prefix) {
    return fmha_rope_bwd_out(dout, qkv, o, lse, sin_t, cos_t, prefix, torch::Tensor());
  });
  mod.def("fmha_rope_bwd_out", &fmha_rope_bwd_out);
  mod.def("fmha_bwd", &fmha_bwd);
  mod.def("fmha_fused_bwd_supported", [](int64_t N, int64_t hd) {
    return fmha_rope::fused_bwd_supported((int)N, (int)hd);
  });
  mod.def("multi_tensor_ema", &multi_tensor_ema);
  mod.def("multi_tensor_ema_planned", &multi_tensor_ema_planned);
  mod.def("multi_tensor_adamw_planned", &multi_tensor_adamw_planned);
  mod.def("multi_tensor_l2norm_planned", &multi_tensor_l2norm_planned);
  mod.def("multi_tensor_adamw", &multi_tensor_adamw);
  mod.def("multi_tensor_l2norm_sq", &multi_tensor_l2norm_sq);
}
