// Bindings of the FP8 quantisers and the FP8 GEMM (fp8_gemm.hip), forward and
// backward.

#include "binding_util.h"
#include "fp8_gemm.h"

namespace {

using bf16 = __hip_bfloat16;

#define CHECK_FP8_FMT(fmt, who) \
  TORCH_CHECK((fmt) == FP8_FMT_E4M3 || (fmt) == FP8_FMT_E5M2, who ": format must be 0 (e4m3) or 1 (e5m2)")

// bf16 [M,K] -> (fp8 bytes [M,K] as uint8, fp32 power-of-two scales [M]).
// fmt: FP8_FMT_E4M3 (0, default) or FP8_FMT_E5M2 (1).
std::vector<torch::Tensor> fp8_quant_rows(torch::Tensor x, int64_t fmt) {
  const bf16* x_p = in_ptr<bf16>(x, "fp8_quant_rows: x");
  CHECK_FP8_FMT(fmt, "fp8_quant_rows");
  TORCH_CHECK(x.dim() == 2, "fp8_quant_rows: x must be [M, K]");
  const long M = x.size(0);
  const long K = x.size(1);
  TORCH_CHECK(K > 0 && K % FP8_QUANT_VEC == 0 && K <= INT_MAX,
              "fp8_quant_rows: K must be a positive multiple of ", FP8_QUANT_VEC);
  TORCH_CHECK(is_aligned(x, 16), "fp8_quant_rows: x must be 16-byte aligned");
  auto q = torch::empty({M, K}, x.options().dtype(torch::kUInt8));
  auto scale = torch::empty({M}, x.options().dtype(torch::kFloat));
  launch_fp8_quant_rows(x_p, OUT_PTR(unsigned char, q), OUT_PTR(float, scale), M,
                        (int)K, (int)fmt, current_stream());
  return {q, scale};
}

// bf16 [R,C] -> (fp8 bytes [C,Rp] as uint8 with Rp = ceil(R/128)*128 and zero
// pad, fp32 scales [C], fp32 column sums [C] or an empty tensor).
std::vector<torch::Tensor> fp8_quant_cols_t(torch::Tensor x, int64_t fmt, bool colsum) {
  const bf16* x_p = in_ptr<bf16>(x, "fp8_quant_cols_t: x");
  CHECK_FP8_FMT(fmt, "fp8_quant_cols_t");
  TORCH_CHECK(x.dim() == 2, "fp8_quant_cols_t: x must be [R, C]");
  const long R = x.size(0);
  const long C = x.size(1);
  TORCH_CHECK(R >= 1, "fp8_quant_cols_t: R must be at least 1");
  TORCH_CHECK(C > 0 && C % FP8_QUANT_VEC == 0 && C <= 65535L * FP8_COLS_TC,
              "fp8_quant_cols_t: C must be a positive multiple of ", FP8_QUANT_VEC);
  TORCH_CHECK((R + FP8_COLS_TR - 1) / FP8_COLS_TR <= INT_MAX, "fp8_quant_cols_t: R too large");
  TORCH_CHECK(is_aligned(x, 16), "fp8_quant_cols_t: x must be 16-byte aligned");
  const long Rp = (R + FP8_COLS_TR - 1) / FP8_COLS_TR * FP8_COLS_TR;
  const int np = fp8_cols_partials(R, (int)C);
  auto fopt = x.options().dtype(torch::kFloat);
  auto q = torch::empty({C, Rp}, x.options().dtype(torch::kUInt8));
  auto scale = torch::empty({C}, fopt);
  auto sums = torch::empty({colsum ? C : 0}, fopt);
  auto part = torch::empty({colsum ? 2 : 1, (long)np, C}, fopt);
  float* part_amax = OUT_PTR(float, part);
  launch_fp8_quant_cols_t(x_p, OUT_PTR(unsigned char, q), OUT_PTR(float, scale),
                          OPT_OUT_PTR(float, sums), part_amax,
                          colsum ? part_amax + (long)np * C : nullptr, R, (int)C, (int)fmt,
                          current_stream());
  return {q, scale, sums};
}

// fp32 column sums [C] of bf16 [R,C], by pass 1 of the column quantiser alone
// (the bias gradient when no weight gradient is wanted).
torch::Tensor fp8_colsum(torch::Tensor x) {
  const bf16* x_p = in_ptr<bf16>(x, "fp8_colsum: x");
  TORCH_CHECK(x.dim() == 2, "fp8_colsum: x must be [R, C]");
  const long R = x.size(0);
  const long C = x.size(1);
  TORCH_CHECK(R >= 1, "fp8_colsum: R must be at least 1");
  TORCH_CHECK(C > 0 && C % FP8_QUANT_VEC == 0 && C <= 65535L * FP8_COLS_TC,
              "fp8_colsum: C must be a positive multiple of ", FP8_QUANT_VEC);
  TORCH_CHECK(is_aligned(x, 16), "fp8_colsum: x must be 16-byte aligned");
  const int np = fp8_cols_partials(R, (int)C);
  auto fopt = x.options().dtype(torch::kFloat);
  auto sums = torch::empty({C}, fopt);
  auto part = torch::empty({2, (long)np, C}, fopt);
  float* part_amax = OUT_PTR(float, part);
  launch_fp8_quant_cols_t(x_p, nullptr, nullptr, OUT_PTR(float, sums), part_amax,
                          part_amax + (long)np * C, R, (int)C, FP8_FMT_E4M3, current_stream());
  return sums;
}

// y[M,N] = bf16((xq . wq^T) * sx[m] * sw[n] + bias[n]); xq [M,K] fp8 bytes of format
// fmt_x (e4m3 by default; e5m2 for the backward GEMMs, without bias), wq [N,K] e4m3fn bytes.
torch::Tensor fp8_gemm_nt(torch::Tensor xq, torch::Tensor sx, torch::Tensor wq,
                          torch::Tensor sw, c10::optional<torch::Tensor> bias, int64_t fmt_x) {
  check_hip(xq, "xq");
  CHECK_FP8_FMT(fmt_x, "fp8_gemm_nt");
  TORCH_CHECK(fmt_x == FP8_FMT_E4M3 || !(bias.has_value() && bias->defined()),
              "fp8_gemm_nt: no bias with an e5m2 first operand");
  check_hip(sx, "sx");
  check_hip(wq, "wq");
  check_hip(sw, "sw");
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
  TORCH_CHECK(is_aligned(xq, 16) && is_aligned(wq, 16) && is_aligned(sw, 16),
              "fp8_gemm_nt: operands must be 16-byte aligned");
  const bf16* bias_ptr = nullptr;
  torch::Tensor b;
  if (bias.has_value() && bias->defined()) {
    b = *bias;
    check_hip(b, "b");
    TORCH_CHECK(b.scalar_type() == at::ScalarType::BFloat16 && b.numel() == N,
                "fp8_gemm_nt: bias must be bf16 [N]");
    if (!is_aligned(b, 8)) b = b.clone();
    bias_ptr = IN_PTR(bf16, b);
  }
  auto y = torch::empty({M, N}, xq.options().dtype(torch::kBFloat16));
  launch_fp8_gemm_nt(IN_PTR(unsigned char, xq), IN_PTR(float, sx), IN_PTR(unsigned char, wq),
                     IN_PTR(float, sw), bias_ptr, OUT_PTR(bf16, y), M, (int)N, (int)K,
                     (int)fmt_x, current_stream());
  return y;
}

// One-wave lane-map probe: c[16,16] = a[16,128] . bt[16,128]^T on fp8 bytes of
// formats fmt_a and fmt_b (e4m3 by default).
torch::Tensor probe_mfma_fp8(torch::Tensor a, torch::Tensor bt, int64_t fmt_a, int64_t fmt_b) {
  CHECK_FP8_FMT(fmt_a, "probe_mfma_fp8");
  CHECK_FP8_FMT(fmt_b, "probe_mfma_fp8");
  TORCH_CHECK(a.dim() == 2 && a.size(0) == 16 && a.size(1) == FP8_GEMM_BK &&
                  bt.dim() == 2 && bt.size(0) == 16 && bt.size(1) == FP8_GEMM_BK,
              "probe_mfma_fp8: a and bt must be [16, ", FP8_GEMM_BK, "]");
  auto c = torch::empty({16, 16}, a.options().dtype(torch::kFloat));
  launch_probe_mfma_fp8(IN_PTR(unsigned char, a), IN_PTR(unsigned char, bt), OUT_PTR(float, c),
                        (int)fmt_a, (int)fmt_b, current_stream());
  return c;
}

}  // namespace

void register_fp8(pybind11::module_& mod) {
  mod.def("fp8_quant_rows", &fp8_quant_rows, py::arg("x"), py::arg("fmt") = FP8_FMT_E4M3);
  mod.def("fp8_quant_cols_t", &fp8_quant_cols_t, py::arg("x"), py::arg("fmt") = FP8_FMT_E4M3,
          py::arg("colsum") = false);
  mod.def("fp8_colsum", &fp8_colsum, py::arg("x"));
  mod.def("fp8_gemm_nt", &fp8_gemm_nt, py::arg("xq"), py::arg("sx"), py::arg("wq"), py::arg("sw"),
          py::arg("bias"), py::arg("fmt_x") = FP8_FMT_E4M3);
  mod.def("probe_mfma_fp8", &probe_mfma_fp8, py::arg("a"), py::arg("bt"),
          py::arg("fmt_a") = FP8_FMT_E4M3, py::arg("fmt_b") = FP8_FMT_E4M3);
}
