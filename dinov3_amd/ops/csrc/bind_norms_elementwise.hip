// Bindings of the normalization kernels (norms.hip) and of the elementwise and
// row kernels (elementwise.hip).

#include "binding_util.h"
#include "elementwise.h"
#include "norms.h"

namespace {

// ------------------------------- norms ---------------------------------

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                                         double eps) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat));
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  DISPATCH_FLOAT_BF16(x.scalar_type(), "layernorm_fwd", [&] {
    launch_layernorm_fwd<scalar_t>(IN_PTR(scalar_t, x), IN_PTR(scalar_t, w),
                                   IN_PTR(scalar_t, b), OUT_PTR(scalar_t, y),
                                   OUT_PTR(float, mean), OUT_PTR(float, rstd), rows, D,
                                   (float)eps, current_stream());
  });
  return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                         torch::Tensor mean, torch::Tensor rstd) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({D}, x.options());
  auto db = torch::empty({D}, x.options());
  auto ws = colreduce_workspace(2, D, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "layernorm_bwd", [&] {
    launch_layernorm_bwd<scalar_t>(IN_PTR(scalar_t, dy), IN_PTR(scalar_t, x),
                                   IN_PTR(scalar_t, w), IN_PTR(float, mean),
                                   IN_PTR(float, rstd), OUT_PTR(scalar_t, dx),
                                   OUT_PTR(float, ws), OUT_PTR(scalar_t, dw),
                                   OUT_PTR(scalar_t, db), rows, D, current_stream());
  });
  return {dx, dw, db};
}

// LayerNorm of the rows flat[idx]: (y, sub = flat[idx], mean, rstd), bit-equal
// to row_gather + layernorm_fwd with one pass less over the gathered rows.
std::vector<torch::Tensor> gather_layernorm_fwd(torch::Tensor flat, torch::Tensor idx,
                                                torch::Tensor w, torch::Tensor b, double eps) {
  TORCH_CHECK(flat.dim() == 2, "gather_layernorm_fwd: flat must be [R, D]");
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
        IN_PTR(scalar_t, flat), IN_PTR(long, idx), IN_PTR(scalar_t, w), IN_PTR(scalar_t, b),
        OUT_PTR(scalar_t, y), OUT_PTR(scalar_t, sub), OUT_PTR(float, mean),
        OUT_PTR(float, rstd), M, D, (float)eps, current_stream());
  });
  return {y, sub, mean, rstd};
}

// LayerNorm backward whose dx rows are accumulated into dacc[idx] in place
// (rows of idx disjoint); returns (dw, db), bit-equal to layernorm_bwd's.
std::vector<torch::Tensor> layernorm_bwd_scatter_acc_(torch::Tensor dacc, torch::Tensor idx,
                                                      torch::Tensor dy, torch::Tensor x,
                                                      torch::Tensor w, torch::Tensor mean,
                                                      torch::Tensor rstd) {
  TORCH_CHECK(dacc.dim() == 2 && x.dim() == 2 && dy.dim() == 2,
              "layernorm_bwd_scatter_acc_: dacc, dy, x must be 2-D");
  const int D = x.size(1);
  const long M = x.size(0);
  TORCH_CHECK(D % 8 == 0 && D <= 1536,
              "layernorm_bwd_scatter_acc_ supports D % 8 == 0 and D <= 1536, got ", D);
  TORCH_CHECK(dacc.size(1) == D && dy.size(0) == M && dy.size(1) == D && idx.numel() == M &&
                  mean.numel() == M && rstd.numel() == M && w.numel() == D,
              "layernorm_bwd_scatter_acc_: shape mismatch");
  if (M == 0) return {torch::zeros({D}, x.options()), torch::zeros({D}, x.options())};
  auto dw = torch::empty({D}, x.options());
  auto db = torch::empty({D}, x.options());
  auto ws = colreduce_workspace(2, D, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "layernorm_bwd_scatter_acc_", [&] {
    launch_layernorm_bwd_scatter_acc<scalar_t>(
        IN_PTR(scalar_t, dy), IN_PTR(scalar_t, x), IN_PTR(scalar_t, w), IN_PTR(float, mean),
        IN_PTR(float, rstd), OUT_PTR(scalar_t, dacc), IN_PTR(long, idx), OUT_PTR(float, ws),
        OUT_PTR(scalar_t, dw), OUT_PTR(scalar_t, db), M, D, current_stream());
  });
  return {dw, db};
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w, double eps) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat));
  DISPATCH_FLOAT_BF16(x.scalar_type(), "rmsnorm_fwd", [&] {
    launch_rmsnorm_fwd<scalar_t>(IN_PTR(scalar_t, x), IN_PTR(scalar_t, w), OUT_PTR(scalar_t, y),
                                 OUT_PTR(float, rstd), rows, D, (float)eps, current_stream());
  });
  return {y, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w,
                                       torch::Tensor rstd) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto dx = torch::empty_like(x);
  auto dw = torch::empty({D}, x.options());
  auto ws = colreduce_workspace(1, D, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "rmsnorm_bwd", [&] {
    launch_rmsnorm_bwd<scalar_t>(IN_PTR(scalar_t, dy), IN_PTR(scalar_t, x), IN_PTR(scalar_t, w),
                                 IN_PTR(float, rstd), OUT_PTR(scalar_t, dx), OUT_PTR(float, ws),
                                 OUT_PTR(scalar_t, dw), rows, D, current_stream());
  });
  return {dx, dw};
}

std::vector<torch::Tensor> l2norm_fwd(torch::Tensor x, double eps) {
  const int D = x.size(-1);
  const long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  auto s = torch::empty({rows}, x.options().dtype(torch::kFloat));
  DISPATCH_FLOAT_BF16(x.scalar_type(), "l2norm_fwd", [&] {
    launch_l2norm_fwd<scalar_t>(IN_PTR(scalar_t, x), OUT_PTR(scalar_t, y), OUT_PTR(float, s),
                                rows, D, (float)eps, current_stream());
  });
  return {y, s};
}

torch::Tensor l2norm_bwd(torch::Tensor dy, torch::Tensor y, torch::Tensor s, double eps) {
  const int D = y.size(-1);
  const long rows = y.numel() / D;
  auto dx = torch::empty_like(y);
  DISPATCH_FLOAT_BF16(y.scalar_type(), "l2norm_bwd", [&] {
    launch_l2norm_bwd<scalar_t>(IN_PTR(scalar_t, dy), IN_PTR(scalar_t, y), IN_PTR(float, s),
                                OUT_PTR(scalar_t, dx), rows, D, (float)eps, current_stream());
  });
  return dx;
}

// ----------------------------- elementwise ------------------------------

torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor bias) {
  const int H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "bias_gelu: H must be a multiple of 8");
  const long rows = x.numel() / H;
  auto y = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "bias_gelu_fwd", [&] {
    launch_bias_gelu_fwd<scalar_t>(IN_PTR(scalar_t, x), IN_PTR(scalar_t, bias),
                                   OUT_PTR(scalar_t, y), rows, H, current_stream());
  });
  return y;
}

std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor bias) {
  const int H = x.size(-1);
  const long rows = x.numel() / H;
  auto dx = torch::empty_like(x);
  auto dbias = torch::empty({H}, x.options());
  auto ws = colreduce_workspace(1, H, x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "bias_gelu_bwd", [&] {
    launch_bias_gelu_bwd<scalar_t>(IN_PTR(scalar_t, dy), IN_PTR(scalar_t, x),
                                   IN_PTR(scalar_t, bias), OUT_PTR(scalar_t, dx),
                                   OUT_PTR(float, ws), OUT_PTR(scalar_t, dbias), rows, H,
                                   current_stream());
  });
  return {dx, dbias};
}

torch::Tensor ls_axpy_fwd(torch::Tensor x, torch::Tensor res, torch::Tensor gamma) {
  const int D = x.size(-1);
  TORCH_CHECK(D % 8 == 0, "ls_axpy: D must be a multiple of 8");
  const long rows = x.numel() / D;
  auto out = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "ls_axpy_fwd", [&] {
    launch_ls_axpy_fwd<scalar_t>(IN_PTR(scalar_t, x), IN_PTR(scalar_t, res),
                                 IN_PTR(scalar_t, gamma), OUT_PTR(scalar_t, out), rows, D,
                                 current_stream());
  });
  return out;
}

torch::Tensor ls_axpy_bias_fwd(torch::Tensor x, torch::Tensor res, torch::Tensor gamma,
                               torch::Tensor bias) {
  const int D = x.size(-1);
  TORCH_CHECK(D % 8 == 0, "ls_axpy_bias: D must be a multiple of 8");
  const long rows = x.numel() / D;
  auto out = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "ls_axpy_bias_fwd", [&] {
    launch_ls_axpy_bias_fwd<scalar_t>(IN_PTR(scalar_t, x), IN_PTR(scalar_t, res),
                                      IN_PTR(scalar_t, gamma), IN_PTR(scalar_t, bias),
                                      OUT_PTR(scalar_t, out), rows, D, current_stream());
  });
  return out;
}

std::vector<torch::Tensor> ls_axpy_bwd(torch::Tensor dout, torch::Tensor res,
                                       torch::Tensor gamma) {
  const int D = dout.size(-1);
  const long rows = dout.numel() / D;
  auto dres = torch::empty_like(dout);
  auto dgamma = torch::empty({D}, dout.options());
  auto ws = colreduce_workspace(1, D, dout);
  DISPATCH_FLOAT_BF16(dout.scalar_type(), "ls_axpy_bwd", [&] {
    launch_ls_axpy_bwd<scalar_t>(IN_PTR(scalar_t, dout), IN_PTR(scalar_t, res),
                                 IN_PTR(scalar_t, gamma), OUT_PTR(scalar_t, dres),
                                 OUT_PTR(float, ws), OUT_PTR(scalar_t, dgamma), rows, D,
                                 current_stream());
  });
  return {dres, dgamma};
}

std::vector<torch::Tensor> ls_axpy_bias_bwd(torch::Tensor dout, torch::Tensor res,
                                            torch::Tensor gamma, torch::Tensor bias) {
  const int D = dout.size(-1);
  const long rows = dout.numel() / D;
  auto dres = torch::empty_like(dout);
  auto dgamma = torch::empty({D}, dout.options());
  auto dbias = torch::empty({D}, dout.options());
  auto ws = colreduce_workspace(2, D, dout);
  DISPATCH_FLOAT_BF16(dout.scalar_type(), "ls_axpy_bias_bwd", [&] {
    launch_ls_axpy_bias_bwd<scalar_t>(IN_PTR(scalar_t, dout), IN_PTR(scalar_t, res),
                                      IN_PTR(scalar_t, gamma), IN_PTR(scalar_t, bias),
                                      OUT_PTR(scalar_t, dres), OUT_PTR(float, ws),
                                      OUT_PTR(scalar_t, dgamma), OUT_PTR(scalar_t, dbias), rows,
                                      D, current_stream());
  });
  return {dres, dgamma, dbias};
}

torch::Tensor row_gather(torch::Tensor src, torch::Tensor idx) {
  const int D = src.size(-1);
  TORCH_CHECK(D % 8 == 0, "row ops need D % 8 == 0");
  const long M = idx.numel();
  auto out = torch::empty({M, D}, src.options());
  DISPATCH_FLOAT_BF16(src.scalar_type(), "row_gather", [&] {
    launch_row_gather<scalar_t>(IN_PTR(scalar_t, src), IN_PTR(long, idx), OUT_PTR(scalar_t, out),
                                M, D, current_stream());
  });
  return out;
}

void row_scatter_add_(torch::Tensor dst, torch::Tensor idx, torch::Tensor src,
                      torch::Tensor scale) {
  const int D = dst.size(-1);
  const long M = idx.numel();
  DISPATCH_FLOAT_BF16(dst.scalar_type(), "row_scatter_add", [&] {
    launch_row_scatter_add<scalar_t>(OUT_PTR(scalar_t, dst), IN_PTR(long, idx),
                                     IN_PTR(scalar_t, src), OPT_IN_PTR(float, scale), M, D,
                                     current_stream());
  });
}

torch::Tensor row_gather_scaled(torch::Tensor src, torch::Tensor idx, torch::Tensor scale) {
  const int D = src.size(-1);
  const long M = idx.numel();
  auto out = torch::empty({M, D}, src.options());
  DISPATCH_FLOAT_BF16(src.scalar_type(), "row_gather_scaled", [&] {
    launch_row_gather_scaled<scalar_t>(IN_PTR(scalar_t, src), IN_PTR(long, idx),
                                       OPT_IN_PTR(float, scale), OUT_PTR(scalar_t, out), M, D,
                                       current_stream());
  });
  return out;
}

void ls_scatter_add_(torch::Tensor dst, torch::Tensor idx, torch::Tensor src,
                     torch::Tensor gamma, torch::Tensor bias, torch::Tensor scale) {
  const int D = dst.size(-1);
  TORCH_CHECK(D % 8 == 0, "ls_scatter: D must be a multiple of 8");
  const long M = idx.numel();
  DISPATCH_FLOAT_BF16(dst.scalar_type(), "ls_scatter_add_", [&] {
    launch_ls_scatter_add<scalar_t>(OUT_PTR(scalar_t, dst), IN_PTR(long, idx),
                                    IN_PTR(scalar_t, src), OPT_IN_PTR(scalar_t, gamma),
                                    OPT_IN_PTR(scalar_t, bias), OPT_IN_PTR(float, scale), M, D,
                                    current_stream());
  });
}

std::vector<torch::Tensor> ls_scatter_bwd(torch::Tensor dy, torch::Tensor idx,
                                          torch::Tensor src, torch::Tensor gamma,
                                          torch::Tensor bias, torch::Tensor scale) {
  const int D = dy.size(-1);
  const long M = idx.numel();
  auto dres = torch::empty_like(src);
  auto dgamma = gamma.defined() ? torch::empty({D}, dy.options()) : torch::Tensor();
  auto dbias = bias.defined() ? torch::empty({D}, dy.options()) : torch::Tensor();
  auto ws = colreduce_workspace(2, D, dy);
  DISPATCH_FLOAT_BF16(dy.scalar_type(), "ls_scatter_bwd", [&] {
    launch_ls_scatter_bwd<scalar_t>(IN_PTR(scalar_t, dy), IN_PTR(long, idx),
                                    IN_PTR(scalar_t, src), OPT_IN_PTR(scalar_t, gamma),
                                    OPT_IN_PTR(scalar_t, bias), OPT_IN_PTR(float, scale),
                                    OUT_PTR(scalar_t, dres), OUT_PTR(float, ws),
                                    OPT_OUT_PTR(scalar_t, dgamma), OPT_OUT_PTR(scalar_t, dbias),
                                    M, D, current_stream());
  });
  return {dres, dgamma, dbias};
}

torch::Tensor swiglu_fwd(torch::Tensor x12) {
  const int H2 = x12.size(-1);
  const int H = H2 / 2;
  const long rows = x12.numel() / H2;
  auto sizes = x12.sizes().vec();
  sizes.back() = H;
  auto y = torch::empty(sizes, x12.options());
  DISPATCH_FLOAT_BF16(x12.scalar_type(), "swiglu_fwd", [&] {
    launch_swiglu_fwd<scalar_t>(IN_PTR(scalar_t, x12), OUT_PTR(scalar_t, y), rows, H,
                                current_stream());
  });
  return y;
}

torch::Tensor swiglu_bwd(torch::Tensor dy, torch::Tensor x12) {
  const int H2 = x12.size(-1);
  const int H = H2 / 2;
  const long rows = x12.numel() / H2;
  auto dx12 = torch::empty_like(x12);
  DISPATCH_FLOAT_BF16(x12.scalar_type(), "swiglu_bwd", [&] {
    launch_swiglu_bwd<scalar_t>(IN_PTR(scalar_t, dy), IN_PTR(scalar_t, x12),
                                OUT_PTR(scalar_t, dx12), rows, H, current_stream());
  });
  return dx12;
}

torch::Tensor rope_fwd(torch::Tensor x, torch::Tensor sin_t, torch::Tensor cos_t,
                       int64_t prefix) {
  TORCH_CHECK(x.dim() == 4, "rope_fwd expects [B, H, N, hd]");
  TORCH_CHECK(sin_t.scalar_type() == at::ScalarType::Float, "rope tables must be fp32");
  const long BH = x.size(0) * x.size(1);
  const int N = x.size(2);
  const int hd = x.size(3);
  const int P = N - (int)prefix;
  TORCH_CHECK(sin_t.size(0) == P && sin_t.size(1) == hd, "rope table shape mismatch");
  auto y = torch::empty_like(x);
  DISPATCH_FLOAT_BF16(x.scalar_type(), "rope_fwd", [&] {
    launch_rope_fwd<scalar_t>(IN_PTR(scalar_t, x), IN_PTR(float, sin_t), IN_PTR(float, cos_t),
                              OUT_PTR(scalar_t, y), BH, N, P, hd, current_stream());
  });
  return y;
}

}  // namespace

void register_norms_elementwise(pybind11::module_& mod) {
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
}
