// Bindings of the loss kernels: prototype-score cross-entropy and
// Sinkhorn-Knopp (proto_ce.hip), Gram anchoring (gram_loss.hip).

#include "binding_util.h"
#include "gram_loss.h"
#include "proto_ce.h"

namespace {

using bf16 = __hip_bfloat16;

// ------------------------------ proto CE --------------------------------

// Host checks shared by the prototype ops, before any launch: every tensor is a
// contiguous HIP tensor of the kernel's dtype (IN_PTR / OUT_PTR), on x's device,
// and as long as the kernel's indexing assumes.
void check_len(const torch::Tensor& t, long n, const torch::Tensor& x, const char* who) {
  TORCH_CHECK(t.defined() && t.numel() == n, who, " must have ", n, " elements, got ",
              t.defined() ? t.numel() : -1);
  TORCH_CHECK(t.device() == x.device(), who, " must be on x's device");
}

// x [S, B, K] student logits and the teacher [T, B, K] (probabilities or logits).
void check_dino_pair(const torch::Tensor& x, const torch::Tensor& t, const char* op) {
  TORCH_CHECK(x.dim() == 3 && t.dim() == 3, op, " expects [S,B,K] and [T,B,K]");
  TORCH_CHECK(t.size(1) == x.size(1) && t.size(2) == x.size(2), op,
              ": student and teacher must agree in B and K, got ", x.sizes(), " and ", t.sizes());
  TORCH_CHECK(t.device() == x.device(), op, ": student and teacher must be on one device");
  TORCH_CHECK(x.size(0) * x.size(1) < (1L << 31) && t.size(0) * t.size(1) < (1L << 31), op,
              ": too many rows");
}

// x [M, K] student logits and the row-aligned teacher [M, K].
void check_ibot_pair(const torch::Tensor& x, const torch::Tensor& t, const char* op) {
  TORCH_CHECK(x.dim() == 2 && t.dim() == 2, op, " expects [M,K] and [M,K]");
  TORCH_CHECK(t.sizes() == x.sizes(), op, ": student and teacher must have one shape, got ",
              x.sizes(), " and ", t.sizes());
  TORCH_CHECK(t.device() == x.device(), op, ": student and teacher must be on one device");
  TORCH_CHECK(x.size(0) < (1L << 31), op, ": too many rows");
}

std::vector<torch::Tensor> dino_ce_fwd(torch::Tensor x, torch::Tensor t, double temp,
                                       bool ignore_diag) {
  check_dino_pair(x, t, "dino_ce_fwd");
  const int S = x.size(0), B = x.size(1);
  const int T = t.size(0);
  const long K = x.size(2);
  auto lse = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_dino_ce_fwd(IN_PTR(bf16, x), IN_PTR(float, t), OUT_PTR(float, lse), OUT_PTR(float, st),
                     OUT_PTR(float, loss), S, T, B, K, (float)(1.0 / temp), ignore_diag,
                     current_stream());
  return {loss, lse, st};
}

torch::Tensor dino_ce_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor t,
                          torch::Tensor lse, torch::Tensor st, double temp,
                          bool ignore_diag) {
  check_dino_pair(x, t, "dino_ce_bwd");
  const int S = x.size(0), B = x.size(1);
  const int T = t.size(0);
  const long K = x.size(2);
  check_len(g, 1, x, "dino_ce_bwd: g");
  check_len(lse, (long)S * B, x, "dino_ce_bwd: lse");
  check_len(st, (long)S * B, x, "dino_ce_bwd: st");
  auto dx = torch::empty_like(x);
  launch_dino_ce_bwd(IN_PTR(bf16, x), IN_PTR(float, t), IN_PTR(float, lse), IN_PTR(float, st),
                     IN_PTR(float, g), OUT_PTR(bf16, dx), S, T, B, K, (float)(1.0 / temp),
                     ignore_diag, current_stream());
  return dx;
}

std::vector<torch::Tensor> ibot_ce_fwd(torch::Tensor x, torch::Tensor t, torch::Tensor w,
                                       double temp) {
  check_ibot_pair(x, t, "ibot_ce_fwd");
  const int M = x.size(0);
  const long K = x.size(1);
  check_len(w, M, x, "ibot_ce_fwd: w");
  auto lse = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_ibot_ce_fwd(IN_PTR(bf16, x), IN_PTR(float, t), IN_PTR(float, w), OUT_PTR(float, lse),
                     OUT_PTR(float, st), OUT_PTR(float, loss), M, K, (float)(1.0 / temp),
                     current_stream());
  return {loss, lse, st};
}

torch::Tensor ibot_ce_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor t,
                          torch::Tensor w, torch::Tensor lse, torch::Tensor st,
                          double temp) {
  check_ibot_pair(x, t, "ibot_ce_bwd");
  const int M = x.size(0);
  const long K = x.size(1);
  check_len(g, 1, x, "ibot_ce_bwd: g");
  check_len(w, M, x, "ibot_ce_bwd: w");
  check_len(lse, M, x, "ibot_ce_bwd: lse");
  check_len(st, M, x, "ibot_ce_bwd: st");
  auto dx = torch::empty_like(x);
  launch_ibot_ce_bwd(IN_PTR(bf16, x), IN_PTR(float, t), IN_PTR(float, w), IN_PTR(float, lse),
                     IN_PTR(float, st), IN_PTR(float, g), OUT_PTR(bf16, dx), M, K,
                     (float)(1.0 / temp), current_stream());
  return dx;
}

// A [K] = sum_m exp(x[m, k] / temp) * u[m]; an empty u stands for ones. The
// kernel loads and stores eight columns at a time: K must be a multiple of 8
// and x 16-byte aligned. With no rows A is zero, without a launch.
torch::Tensor sinkhorn_fact_colsum(torch::Tensor x, torch::Tensor u, double temp) {
  TORCH_CHECK(x.dim() == 2, "sinkhorn_fact_colsum expects x [M,K]");
  const long K = x.size(1);
  TORCH_CHECK(x.size(0) < (1L << 31), "sinkhorn_fact_colsum: too many rows");
  const int M = x.size(0);
  TORCH_CHECK(K >= 8 && K % 8 == 0,
              "sinkhorn_fact_colsum: K must be a positive multiple of 8, got ", K);
  const bf16* x_p = IN_PTR(bf16, x);
  TORCH_CHECK(is_aligned(x, 16), "sinkhorn_fact_colsum: x must be 16-byte aligned");
  if (u.defined() && u.numel() > 0) check_len(u, M, x, "sinkhorn_fact_colsum: u");
  auto A = torch::empty({K}, x.options().dtype(torch::kFloat));
  launch_sinkhorn_fact_colsum(x_p, OPT_IN_PTR(float, u), OUT_PTR(float, A), M, K,
                              (float)(1.0 / temp), current_stream());
  return A;
}

torch::Tensor sinkhorn_fact_rowsum(torch::Tensor x, torch::Tensor v, double temp) {
  TORCH_CHECK(x.dim() == 2, "sinkhorn_fact_rowsum expects x [M,K]");
  TORCH_CHECK(x.size(0) < (1L << 31), "sinkhorn_fact_rowsum: too many rows");
  const int M = x.size(0);
  const long K = x.size(1);
  check_len(v, K, x, "sinkhorn_fact_rowsum: v");
  auto u = torch::empty({M}, x.options().dtype(torch::kFloat));
  launch_sinkhorn_fact_rowsum(IN_PTR(bf16, x), IN_PTR(float, v), OUT_PTR(float, u), M, K,
                              (float)(1.0 / temp), current_stream());
  return u;
}

std::vector<torch::Tensor> ibot_ce_fact_fwd(torch::Tensor x, torch::Tensor xt,
                                            torch::Tensor u, torch::Tensor v,
                                            torch::Tensor w, double temp, double tt) {
  check_ibot_pair(x, xt, "ibot_ce_fact_fwd");
  const int M = x.size(0);
  const long K = x.size(1);
  check_len(u, M, x, "ibot_ce_fact_fwd: u");
  check_len(v, K, x, "ibot_ce_fact_fwd: v");
  check_len(w, M, x, "ibot_ce_fact_fwd: w");
  auto lse = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({M}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_ibot_ce_fact_fwd(IN_PTR(bf16, x), IN_PTR(bf16, xt), IN_PTR(float, u), IN_PTR(float, v),
                          IN_PTR(float, w), OUT_PTR(float, lse), OUT_PTR(float, st),
                          OUT_PTR(float, loss), M, K, (float)(1.0 / temp), (float)(1.0 / tt),
                          current_stream());
  return {loss, lse, st};
}

torch::Tensor ibot_ce_fact_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor xt,
                               torch::Tensor u, torch::Tensor v, torch::Tensor w,
                               torch::Tensor lse, torch::Tensor st, double temp,
                               double tt) {
  check_ibot_pair(x, xt, "ibot_ce_fact_bwd");
  const int M = x.size(0);
  const long K = x.size(1);
  check_len(g, 1, x, "ibot_ce_fact_bwd: g");
  check_len(u, M, x, "ibot_ce_fact_bwd: u");
  check_len(v, K, x, "ibot_ce_fact_bwd: v");
  check_len(w, M, x, "ibot_ce_fact_bwd: w");
  check_len(lse, M, x, "ibot_ce_fact_bwd: lse");
  check_len(st, M, x, "ibot_ce_fact_bwd: st");
  auto dx = torch::empty_like(x);
  launch_ibot_ce_fact_bwd(IN_PTR(bf16, x), IN_PTR(bf16, xt), IN_PTR(float, u), IN_PTR(float, v),
                          IN_PTR(float, w), IN_PTR(float, lse), IN_PTR(float, st),
                          IN_PTR(float, g), OUT_PTR(bf16, dx), M, K, (float)(1.0 / temp),
                          (float)(1.0 / tt), current_stream());
  return dx;
}

std::vector<torch::Tensor> dino_ce_fact_fwd(torch::Tensor x, torch::Tensor xt,
                                            torch::Tensor u, torch::Tensor v, double temp,
                                            double tt, bool ignore_diag) {
  check_dino_pair(x, xt, "dino_ce_fact_fwd");
  const int S = x.size(0), B = x.size(1);
  const int T = xt.size(0);
  const long K = x.size(2);
  check_len(u, (long)T * B, x, "dino_ce_fact_fwd: u");
  check_len(v, K, x, "dino_ce_fact_fwd: v");
  auto lse = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto st = torch::empty({S * B}, x.options().dtype(torch::kFloat));
  auto loss = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_dino_ce_fact_fwd(IN_PTR(bf16, x), IN_PTR(bf16, xt), IN_PTR(float, u), IN_PTR(float, v),
                          OUT_PTR(float, lse), OUT_PTR(float, st), OUT_PTR(float, loss), S, T, B,
                          K, (float)(1.0 / temp), (float)(1.0 / tt), ignore_diag,
                          current_stream());
  return {loss, lse, st};
}

torch::Tensor dino_ce_fact_bwd(torch::Tensor g, torch::Tensor x, torch::Tensor xt,
                               torch::Tensor u, torch::Tensor v, torch::Tensor lse,
                               torch::Tensor st, double temp, double tt,
                               bool ignore_diag) {
  check_dino_pair(x, xt, "dino_ce_fact_bwd");
  const int S = x.size(0), B = x.size(1);
  const int T = xt.size(0);
  const long K = x.size(2);
  check_len(g, 1, x, "dino_ce_fact_bwd: g");
  check_len(u, (long)T * B, x, "dino_ce_fact_bwd: u");
  check_len(v, K, x, "dino_ce_fact_bwd: v");
  check_len(lse, (long)S * B, x, "dino_ce_fact_bwd: lse");
  check_len(st, (long)S * B, x, "dino_ce_fact_bwd: st");
  auto dx = torch::empty_like(x);
  launch_dino_ce_fact_bwd(IN_PTR(bf16, x), IN_PTR(bf16, xt), IN_PTR(float, u), IN_PTR(float, v),
                          IN_PTR(float, lse), IN_PTR(float, st), IN_PTR(float, g),
                          OUT_PTR(bf16, dx), S, T, B, K, (float)(1.0 / temp), (float)(1.0 / tt),
                          ignore_diag, current_stream());
  return dx;
}

std::vector<torch::Tensor> sinkhorn_exp(torch::Tensor x, double temp) {
  auto Q = torch::empty(x.sizes(), x.options().dtype(torch::kFloat));
  auto total = torch::zeros({}, x.options().dtype(torch::kFloat));
  launch_sinkhorn_exp(IN_PTR(bf16, x), OUT_PTR(float, Q), OUT_PTR(float, total), x.numel(),
                      (float)(1.0 / temp), current_stream());
  return {Q, total};
}

torch::Tensor sinkhorn_colsum(torch::Tensor Q, torch::Tensor divisor) {
  TORCH_CHECK(Q.dim() == 2 && Q.size(0) < (1L << 31), "sinkhorn_colsum expects Q [M,K]");
  const int M = Q.size(0);
  const long K = Q.size(1);
  check_len(divisor, 1, Q, "sinkhorn_colsum: divisor");
  auto out = torch::empty({K}, Q.options());
  launch_sinkhorn_colsum(IN_PTR(float, Q), OUT_PTR(float, out), M, K, IN_PTR(float, divisor),
                         current_stream());
  return out;
}

void sinkhorn_div_row(torch::Tensor Q, torch::Tensor col, double k_div, torch::Tensor B,
                      bool scale_back) {
  TORCH_CHECK(Q.dim() == 2 && Q.size(0) < (1L << 31), "sinkhorn_div_row expects Q [M,K]");
  const int M = Q.size(0);
  const long K = Q.size(1);
  check_len(col, K, Q, "sinkhorn_div_row: col");
  check_len(B, 1, Q, "sinkhorn_div_row: B");
  launch_sinkhorn_div_row(OUT_PTR(float, Q), IN_PTR(float, col), M, K, (float)k_div,
                          IN_PTR(float, B), scale_back, current_stream());
}

// ------------------------------ Gram loss --------------------------------
// The pieces of ops.gram_loss (gram_loss.hip); the panel loop and the P @ S
// GEMM between them are in ops/gram_loss.py.

constexpr long kGramTile = 128;

void check_gram_inputs(const torch::Tensor& student, const torch::Tensor& teacher) {
  check_hip(student, "student");
  check_hip(teacher, "teacher");
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
  TORCH_CHECK(is_aligned(student, 16) && is_aligned(teacher, 16),
              "gram_loss: student and teacher must be 16-byte aligned");
}

// r [2, G M] fp32: rsqrt of the squared row norms of student (0) and teacher
// (1), or ones without apply_norm.
torch::Tensor gram_rnorm(torch::Tensor student, torch::Tensor teacher, bool apply_norm) {
  check_gram_inputs(student, teacher);
  const long rows = student.size(0) * student.size(1);
  auto r = torch::empty({2, rows}, student.options().dtype(torch::kFloat));
  launch_gram_rnorm(IN_PTR(bf16, student), IN_PTR(bf16, teacher), OUT_PTR(float, r), rows,
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
  check_hip(r, "r");
  check_hip(partials, "partials");
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
  bf16* p_ptr = nullptr;
  if (panel.has_value()) {
    const torch::Tensor& p = panel.value();
    check_hip(p, "p");
    TORCH_CHECK(p.scalar_type() == at::ScalarType::BFloat16 && p.dim() == 2 &&
                    p.size(0) >= ntiles * kGramTile && p.size(1) == nT * kGramTile &&
                    p.device() == student.device(),
                "gram_tiles: panel must be bf16 [>= ntiles * 128, nT * 128] on the inputs' device");
    TORCH_CHECK(is_aligned(p, 16), "gram_tiles: panel must be 16-byte aligned");
    p_ptr = OUT_PTR(bf16, p);
  }
  launch_gram_tiles(IN_PTR(bf16, student), IN_PTR(bf16, teacher), IN_PTR(float, r),
                    IN_PTR(float, r) + G * M, p_ptr, OUT_PTR(float, partials), (int)M, (int)D,
                    (int)mode, tile0, (int)ntiles, current_stream());
}

// loss (0-dim fp32) = sum of the partials in a fixed order / count.
torch::Tensor gram_finish(torch::Tensor partials, double count) {
  const float* partials_p = IN_PTR(float, partials);
  TORCH_CHECK(partials.numel() >= 1, "gram_finish: partials must be fp32 and not empty");
  TORCH_CHECK(count >= 1.0, "gram_finish: count must be at least 1");
  auto loss = torch::empty({}, partials.options());
  launch_gram_finish(partials_p, OUT_PTR(float, loss), partials.numel(), count,
                     current_stream());
  return loss;
}

// dS [G, M, D] bf16 from Draw = P @ S: c r_i (Draw_i - s^_i (s^_i . Draw_i)),
// or c Draw_i without apply_norm.
torch::Tensor gram_norm_bwd(torch::Tensor draw, torch::Tensor student, torch::Tensor r, double c,
                            bool apply_norm) {
  check_gram_inputs(student, draw);
  check_hip(r, "r");
  const long rows = student.size(0) * student.size(1);
  TORCH_CHECK(r.scalar_type() == at::ScalarType::Float && r.dim() == 2 && r.size(0) == 2 &&
                  r.size(1) == rows && r.device() == student.device(),
              "gram_norm_bwd: r must be fp32 [2, G M] on the inputs' device");
  auto ds = torch::empty_like(student);
  launch_gram_norm_bwd(IN_PTR(bf16, draw), IN_PTR(bf16, student), IN_PTR(float, r),
                       OUT_PTR(bf16, ds), rows, (int)student.size(2), (float)c, apply_norm,
                       current_stream());
  return ds;
}

}  // namespace

void register_losses(pybind11::module_& mod) {
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
  mod.def("gram_rnorm", &gram_rnorm, py::arg("student"), py::arg("teacher"),
          py::arg("apply_norm"));
  mod.def("gram_tiles", &gram_tiles, py::arg("student"), py::arg("teacher"), py::arg("r"),
          py::arg("mode"), py::arg("tile0"), py::arg("ntiles"), py::arg("panel"),
          py::arg("partials"));
  mod.def("gram_finish", &gram_finish, py::arg("partials"), py::arg("count"));
  mod.def("gram_norm_bwd", &gram_norm_bwd, py::arg("draw"), py::arg("student"), py::arg("r"),
          py::arg("c"), py::arg("apply_norm"));
}
