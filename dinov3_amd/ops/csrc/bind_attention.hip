// Bindings of the attention kernels (fmha_rope.hip) and of the patch-embedding
// GEMM (patch_embed.hip).

#include "binding_util.h"
#include "fmha_rope.h"  // attention layouts and launchers, launch_probe_mfma
#include "patch_embed.h"

namespace {

using bf16 = __hip_bfloat16;

torch::Tensor probe_mfma(torch::Tensor A, torch::Tensor B) {
  auto C = torch::empty({32, 32}, A.options().dtype(torch::kFloat));
  launch_probe_mfma(IN_PTR(bf16, A), IN_PTR(bf16, B), OUT_PTR(float, C), current_stream());
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

// `who` is "fmha: <argument>"
template <typename T>
const T* attn_in(const torch::Tensor& x, int64_t numel, const char* who) {
  const T* p = in_ptr<T>(x, who);
  TORCH_CHECK(x.numel() == numel, who, " must hold ", numel, " elements, got ", x.numel());
  return p;
}
template <typename T>
T* attn_out(const torch::Tensor& x, int64_t numel, const char* who) {
  return const_cast<T*>(attn_in<T>(x, numel, who));
}

static AttnDims plain_dims(const torch::Tensor& q, const torch::Tensor& k,
                           const torch::Tensor& v) {
  TORCH_CHECK(q.dim() == 4, "fmha expects [B, H, N, hd]");
  const AttnDims d{(int)q.size(0), (int)q.size(1), (int)q.size(2), (int)q.size(3)};
  TORCH_CHECK(d.HD == 64 || d.HD == 128, "fmha: head_dim must be 64 or 128, got ", d.HD);
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(), "fmha: q, k, v differ in shape");
  return d;
}

static AttnDims packed_dims(const torch::Tensor& qkv) {
  TORCH_CHECK(qkv.dim() == 5 && qkv.size(2) == 3, "qkv must be [B, N, 3, H, hd]");
  const AttnDims d{(int)qkv.size(0), (int)qkv.size(3), (int)qkv.size(1), (int)qkv.size(4)};
  TORCH_CHECK(d.HD == 64 || d.HD == 128, "head_dim must be 64 or 128");
  return d;
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
  const float* sin_p = attn_in<float>(sin_t, (int64_t)P * d.HD, "fmha: sin_t");
  TORCH_CHECK(cos_t.defined() && cos_t.sizes() == sin_t.sizes(), "cos_t must match sin_t in shape");
  return {sin_p, attn_in<float>(cos_t, (int64_t)P * d.HD, "fmha: cos_t"), P};
}

// single-pass backward where one workgroup holds the sequence, unless switched off
static bool use_fused_bwd(const AttnDims& d) {
  return fmha_rope::fused_bwd_supported(d.N, d.HD) && fmha_rope::fused_bwd_enabled();
}

std::vector<torch::Tensor> fmha_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v) {
  using L = fmha_rope::PlainLayout;
  const AttnDims d = plain_dims(q, k, v);
  const L::Qkv in{attn_in<bf16>(q, d.numel(), "fmha: q"), attn_in<bf16>(k, d.numel(), "fmha: k"),
                  attn_in<bf16>(v, d.numel(), "fmha: v")};
  auto o = torch::empty_like(q);
  auto lse = torch::empty({d.B, d.H, d.N}, q.options().dtype(torch::kFloat));
  fmha_rope::launch_fwd<L>(in, nullptr, nullptr, OUT_PTR(bf16, o), OUT_PTR(float, lse), d.B, d.H,
                           d.N, d.N, d.HD, d.scale(), current_stream());
  return {o, lse};
}

// dout, o and lse as the backward wrappers receive them, then the launches
// that both layouts share
template <class L>
void run_bwd(const AttnDims& d, typename L::Qkv in, typename L::DQkv grad,
             const torch::Tensor& dout, const torch::Tensor& o, const torch::Tensor& lse,
             const RopeTables& rope) {
  const bf16* dout_p = attn_in<bf16>(dout, d.numel(), "fmha: dout");
  const bf16* o_p = attn_in<bf16>(o, d.numel(), "fmha: o");
  const float* lse_p = attn_in<float>(lse, (int64_t)d.B * d.H * d.N, "fmha: lse");
  auto stream = current_stream();
  if (use_fused_bwd(d)) {
    fmha_rope::launch_bwd_fused<L>(in, dout_p, o_p, rope.sin, rope.cos, lse_p, grad, d.B, d.H,
                                   d.N, rope.P, d.HD, d.scale(), stream);
    return;
  }
  auto D = torch::empty({d.B, d.H, d.N}, lse.options());
  float* D_p = OUT_PTR(float, D);
  fmha_rope::launch_bwd_pre<L>(dout_p, o_p, D_p, d.B, d.H, d.N, d.HD, stream);
  fmha_rope::launch_bwd_dq<L>(in, dout_p, rope.sin, rope.cos, lse_p, D_p, grad, d.B, d.H, d.N,
                              rope.P, d.HD, d.scale(), stream);
  fmha_rope::launch_bwd_dkv<L>(in, dout_p, rope.sin, rope.cos, lse_p, D_p, grad, d.B, d.H, d.N,
                               rope.P, d.HD, d.scale(), stream);
}

std::vector<torch::Tensor> fmha_bwd(torch::Tensor dout, torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o, torch::Tensor lse) {
  using L = fmha_rope::PlainLayout;
  const AttnDims d = plain_dims(q, k, v);
  const L::Qkv in{attn_in<bf16>(q, d.numel(), "fmha: q"), attn_in<bf16>(k, d.numel(), "fmha: k"),
                  attn_in<bf16>(v, d.numel(), "fmha: v")};
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  run_bwd<L>(d, in, L::DQkv{OUT_PTR(bf16, dq), OUT_PTR(bf16, dk), OUT_PTR(bf16, dv)}, dout, o,
             lse, RopeTables{nullptr, nullptr, d.N});
  return {dq, dk, dv};
}

std::vector<torch::Tensor> fmha_rope_fwd_out(torch::Tensor qkv, torch::Tensor sin_t,
                                             torch::Tensor cos_t, int64_t prefix,
                                             torch::Tensor out_o) {
  using L = fmha_rope::PackedLayout;
  const AttnDims d = packed_dims(qkv);
  const L::Qkv in{attn_in<bf16>(qkv, 3 * d.numel(), "fmha: qkv")};
  const RopeTables rope = rope_tables(d, sin_t, cos_t, prefix);
  torch::Tensor o = out_o.defined() && out_o.numel() > 0
                        ? out_o
                        : torch::empty({d.B, d.N, d.H, d.HD}, qkv.options());
  bf16* o_p = attn_out<bf16>(o, d.numel(), "fmha: out_o");
  auto lse = torch::empty({d.B, d.H, d.N}, qkv.options().dtype(torch::kFloat));
  fmha_rope::launch_fwd<L>(in, rope.sin, rope.cos, o_p, OUT_PTR(float, lse), d.B, d.H, d.N,
                           rope.P, d.HD, d.scale(), current_stream());
  return {o, lse};
}

torch::Tensor fmha_rope_bwd_out(torch::Tensor dout, torch::Tensor qkv, torch::Tensor o,
                                torch::Tensor lse, torch::Tensor sin_t,
                                torch::Tensor cos_t, int64_t prefix,
                                torch::Tensor out_dqkv) {
  using L = fmha_rope::PackedLayout;
  const AttnDims d = packed_dims(qkv);
  const L::Qkv in{attn_in<bf16>(qkv, 3 * d.numel(), "fmha: qkv")};
  const RopeTables rope = rope_tables(d, sin_t, cos_t, prefix);
  torch::Tensor dqkv = out_dqkv.defined() && out_dqkv.numel() > 0 ? out_dqkv
                                                                  : torch::empty_like(qkv);
  const L::DQkv grad{attn_out<bf16>(dqkv, 3 * d.numel(), "fmha: out_dqkv")};
  run_bwd<L>(d, in, grad, dout, o, lse, rope);
  return dqkv;
}

// ----------------------------- patch embed ------------------------------

torch::Tensor patch_embed_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor bias,
                              int64_t patch) {
  TORCH_CHECK(x.dim() == 4 && x.scalar_type() == at::ScalarType::BFloat16);
  const int B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int D = w.size(0);
  TORCH_CHECK(C == 3, "patch_embed_fwd kernel supports C=3 (any patch size)");
  TORCH_CHECK(H % patch == 0 && W % patch == 0, "H/W must be multiples of patch");
  const long rows = (long)B * (H / patch) * (W / patch);
  auto out = torch::empty({(long)B, rows / B, (long)D}, x.options());
  launch_patch_embed_fwd(IN_PTR(bf16, x), IN_PTR(bf16, w), IN_PTR(bf16, bias),
                         OUT_PTR(bf16, out), B, C, H, W, (int)patch, D, current_stream());
  return out;
}

}  // namespace

void register_attention(pybind11::module_& mod) {
  mod.def("probe_mfma", &probe_mfma);
  mod.def("fmha_fwd", &fmha_fwd);
  mod.def("fmha_bwd", &fmha_bwd);
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
  mod.def("fmha_fused_bwd_supported", [](int64_t N, int64_t hd) {
    return fmha_rope::fused_bwd_supported((int)N, (int)hd);
  });
  mod.def("patch_embed_fwd", &patch_embed_fwd);
}
