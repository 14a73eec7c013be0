// The extension module dinov3_amd/ops/_hip_ops: every binding file registers
// its own functions (bind_*.hip); the hipBLASLt entry points come straight from
// blaslt_ext.hip.

#include <torch/extension.h>

#include "blaslt_ext.h"

void register_norms_elementwise(pybind11::module_& mod);
void register_losses(pybind11::module_& mod);
void register_attention(pybind11::module_& mod);
void register_fp8(pybind11::module_& mod);
void register_eval(pybind11::module_& mod);
void register_multi_tensor(pybind11::module_& mod);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("blaslt_gemm_bias_gelu_fwd", &blaslt_gemm_bias_gelu_fwd);
  mod.def("blaslt_gemm_dgelu_bgrad", &blaslt_gemm_dgelu_bgrad);
  mod.def("blaslt_gemm_bias", &blaslt_gemm_bias);
  mod.def("blaslt_probe_epilogue", &blaslt_probe_epilogue);
  register_norms_elementwise(mod);
  register_losses(mod);
  register_attention(mod);
  register_fp8(mod);
  register_eval(mod);
  register_multi_tensor(mod);
}
