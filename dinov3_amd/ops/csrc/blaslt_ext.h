// hipBLASLt fused-epilogue entry points (blaslt_ext.hip). All tensors are
// contiguous row-major bf16 unless noted.
#pragma once

#include <torch/extension.h>

#include <vector>

// h = gelu_tanh(x @ w^T + bias), pre-activation saved as aux.
// x [M,K], w [N,K], bias [N]  ->  {h [M,N], pre [M,N]}
std::vector<torch::Tensor> blaslt_gemm_bias_gelu_fwd(torch::Tensor x, torch::Tensor w,
                                                     torch::Tensor bias);
// dpre = dgelu_tanh(dy @ w2, pre); dbias1 = column-sum of dpre (fp32).
// dy [M,N2], w2 [N2,N1], pre [M,N1]  ->  {dpre [M,N1], dbias1 [N1] fp32}
std::vector<torch::Tensor> blaslt_gemm_dgelu_bgrad(torch::Tensor dy, torch::Tensor w2,
                                                   torch::Tensor pre);
// Plain bias GEMM, for validating the layout mapping: y = x @ w^T + bias.
torch::Tensor blaslt_gemm_bias(torch::Tensor x, torch::Tensor w, torch::Tensor bias);
// Probe: how many heuristic algorithms exist for a given epilogue/dtype combo
// on this hardware (no matmul is run). aux_type/bias_type: hipDataType ints,
// -1 = leave unset. Returns n_results (0 = unsupported combo).
int64_t blaslt_probe_epilogue(int64_t epi, int64_t aux_type, int64_t bias_type,
                              int64_t m, int64_t n, int64_t k);
