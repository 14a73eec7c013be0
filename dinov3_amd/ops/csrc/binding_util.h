// Host helpers shared by the binding files (bind_*.hip): the current stream,
// the float / bf16 dispatch, the column-reduction workspace and the checked
// typed pointers that every launcher argument goes through.
#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <vector>

#include "common.h"  // COLRED_MAX_PARTIALS

inline hipStream_t current_stream() { return at::hip::getCurrentHIPStream().stream(); }

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
inline torch::Tensor colreduce_workspace(int n_acc, int D, const torch::Tensor& like) {
  return torch::empty({(long)n_acc * COLRED_MAX_PARTIALS, D},
                      like.options().dtype(torch::kFloat));
}

// ---- checked typed pointers ----
// The torch dtype an element type T of a launcher stands for, and its name in
// the error messages.
template <typename T> struct DtypeOf;
#define DTYPE_OF(T, SCALAR, NAME)                                \
  template <> struct DtypeOf<T> {                                \
    static constexpr at::ScalarType value = at::ScalarType::SCALAR; \
    static constexpr const char* name = NAME;                    \
  }
DTYPE_OF(float, Float, "fp32");
DTYPE_OF(__hip_bfloat16, BFloat16, "bf16");
DTYPE_OF(long, Long, "int64");
DTYPE_OF(int, Int, "int32");
DTYPE_OF(unsigned char, Byte, "uint8");
#undef DTYPE_OF

// `who` names the tensor in the message, e.g. "layernorm_fwd: w".
inline void check_hip(const torch::Tensor& x, const char* who) {
  TORCH_CHECK(x.defined() && x.is_cuda() && x.is_contiguous(), who,
              " must be a contiguous HIP tensor");
}

// For the alignment checks of the vectorised kernels.
inline bool is_aligned(const torch::Tensor& x, size_t bytes) {
  return (uintptr_t)x.data_ptr() % bytes == 0;
}

// The address of x as elements of T, after checking that x is defined, on a
// HIP device, contiguous and of T's dtype.
template <typename T>
const T* in_ptr(const torch::Tensor& x, const char* who) {
  check_hip(x, who);
  TORCH_CHECK(x.scalar_type() == DtypeOf<T>::value, who, " must be ", DtypeOf<T>::name, ", got ",
              x.scalar_type());
  return static_cast<const T*>(x.data_ptr());
}

template <typename T>
T* out_ptr(const torch::Tensor& x, const char* who) {
  return const_cast<T*>(in_ptr<T>(x, who));
}

// nullptr for an optional tensor that is undefined or empty.
template <typename T>
const T* opt_in_ptr(const torch::Tensor& x, const char* who) {
  return x.defined() && x.numel() > 0 ? in_ptr<T>(x, who) : nullptr;
}

template <typename T>
T* opt_out_ptr(const torch::Tensor& x, const char* who) {
  return x.defined() && x.numel() > 0 ? out_ptr<T>(x, who) : nullptr;
}

// Shorthands that name the tensor by its variable in the message.
#define IN_PTR(T, x) in_ptr<T>(x, #x)
#define OUT_PTR(T, x) out_ptr<T>(x, #x)
#define OPT_IN_PTR(T, x) opt_in_ptr<T>(x, #x)
#define OPT_OUT_PTR(T, x) opt_out_ptr<T>(x, #x)
