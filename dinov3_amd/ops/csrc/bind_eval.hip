// Bindings of the evaluation kernels: k-NN top-k (knn_topk.hip), linear probe
// (linear_probe.hip) and segmentation probe (seg_probe.hip).

#include "binding_util.h"
#include "knn_topk.h"
#include "linear_probe.h"
#include "seg_probe.h"

namespace {

using bf16 = __hip_bfloat16;

// ------------------------------- k-NN -----------------------------------

// (val [Q,k] fp32, idx [Q,k] int32): the k largest dot products of every row of
// q [Q,D] with the rows of bank [N,D], ordered by (value descending, bank row
// ascending). splits: slices of the bank along N; 0 lets the kernel choose.
std::vector<torch::Tensor> knn_topk(torch::Tensor q, torch::Tensor bank, int64_t k,
                                    int64_t splits) {
  check_hip(q, "q");
  check_hip(bank, "bank");
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
  TORCH_CHECK(is_aligned(q, 16) && is_aligned(bank, 16),
              "knn_topk: q and bank must be 16-byte aligned");
  auto val = torch::empty({Q, (long)k}, q.options().dtype(torch::kFloat));
  auto idx = torch::empty({Q, (long)k}, q.options().dtype(torch::kInt));
  if (Q == 0) return {val, idx};
  const int ns = splits > 0 ? (int)splits : knn_topk_auto_splits(Q, N);
  torch::Tensor ws;  // 64-bit keys, held as int64
  if (ns > 1) ws = torch::empty({(long)ns, Q, (long)k}, q.options().dtype(torch::kLong));
  launch_knn_topk(IN_PTR(bf16, q), IN_PTR(bf16, bank),
                  reinterpret_cast<unsigned long long*>(OPT_OUT_PTR(long, ws)),
                  OUT_PTR(float, val), OUT_PTR(int, idx), Q, N, (int)D, (int)k, ns,
                  current_stream());
  return {val, idx};
}

// ----------------------------- linear probe ------------------------------

// Softmax cross-entropy of logits [B, G, Cp] (+ bias [G, Cp]) against labels [B]
// over the first C columns, for G heads at once. Returns (loss_sum [G] fp32,
// correct [G] int64) and, with write_grad, dbias [G, Cp] fp32 after the row
// gradients (softmax - onehot) * grad_scale have replaced the logits in place.
// label -1 marks an ignored row. row_blocks: blocks per head, 0 = chosen.
std::vector<torch::Tensor> probe_ce(torch::Tensor logits, c10::optional<torch::Tensor> bias,
                                    torch::Tensor labels, int64_t C, double grad_scale,
                                    bool write_grad, int64_t row_blocks) {
  check_hip(logits, "logits");
  check_hip(labels, "labels");
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
  TORCH_CHECK(is_aligned(logits, 16), "probe_ce: logits must be 16-byte aligned");
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    const torch::Tensor& b = *bias;
    check_hip(b, "b");
    TORCH_CHECK(b.scalar_type() == at::ScalarType::Float && b.dim() == 2 && b.size(0) == G &&
                    b.size(1) == Cp,
                "probe_ce: bias must be fp32 [G, Cp]");
    TORCH_CHECK(b.device() == logits.device(), "probe_ce: bias and logits must be on one device");
    TORCH_CHECK(is_aligned(b, 16), "probe_ce: bias must be 16-byte aligned");
    bias_ptr = IN_PTR(float, b);
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
  DISPATCH_FLOAT_BF16(logits.scalar_type(), "probe_ce", [&] {
    launch_probe_ce<scalar_t>(OUT_PTR(scalar_t, logits), bias_ptr, IN_PTR(long, labels),
                              OUT_PTR(float, ws), OUT_PTR(float, out), B, (int)G, (int)Cp, (int)C,
                              (float)grad_scale, write_grad, nblk, current_stream());
  });
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
  check_hip(w, "w");
  check_hip(mom, "mom");
  check_hip(grad, "grad");
  check_hip(lr, "lr");
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
  TORCH_CHECK(is_aligned(w, 16) && is_aligned(mom, 16) && is_aligned(grad, 16),
              "probe_sgd_: w, mom and grad must be 16-byte aligned");
  const float* wd_ptr = nullptr;
  if (wd.has_value()) {
    const torch::Tensor& d = *wd;
    check_hip(d, "d");
    TORCH_CHECK(d.scalar_type() == at::ScalarType::Float && d.dim() == 1 && d.size(0) == G &&
                    d.device() == w.device(),
                "probe_sgd_: wd must be fp32 [G] on w's device");
    wd_ptr = IN_PTR(float, d);
  }
  bf16* lp_ptr = nullptr;
  if (w_lp.has_value()) {
    const torch::Tensor& l = *w_lp;
    check_hip(l, "l");
    TORCH_CHECK(l.scalar_type() == at::ScalarType::BFloat16 && l.sizes() == w.sizes() &&
                    l.device() == w.device(),
                "probe_sgd_: w_lp must be bf16, shaped like w, on w's device");
    TORCH_CHECK(is_aligned(l, 16), "probe_sgd_: w_lp must be 16-byte aligned");
    lp_ptr = OUT_PTR(bf16, l);
  }
  if (G == 0 || R == 0) return;
  DISPATCH_FLOAT_BF16(grad.scalar_type(), "probe_sgd_", [&] {
    launch_probe_sgd<scalar_t>(OUT_PTR(float, w), OUT_PTR(float, mom), IN_PTR(scalar_t, grad),
                               IN_PTR(float, lr), wd_ptr, lp_ptr, (int)G, R, (float)lr_scale,
                               (float)momentum, current_stream());
  });
}

// -------------------------- segmentation probe ---------------------------

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
  check_hip(logits, "logits");
  check_hip(labels, "labels");
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
  TORCH_CHECK(is_aligned(logits, 16), "seg_ce: logits must be 16-byte aligned");
  // the labels are read a byte at a time: a slice of images needs no alignment
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    const torch::Tensor& b = *bias;
    check_hip(b, "b");
    TORCH_CHECK(b.scalar_type() == at::ScalarType::Float && b.dim() == 2 && b.size(0) == G &&
                    b.size(1) == Cp,
                "seg_ce: bias must be fp32 [G, Cp]");
    TORCH_CHECK(b.device() == logits.device(), "seg_ce: bias and logits must be on one device");
    TORCH_CHECK(is_aligned(b, 16), "seg_ce: bias must be 16-byte aligned");
    bias_ptr = IN_PTR(float, b);
  }
  const float* scale_ptr = nullptr;
  if (scale.has_value()) {
    const torch::Tensor& sc = *scale;
    check_hip(sc, "sc");
    TORCH_CHECK(sc.scalar_type() == at::ScalarType::Float && sc.numel() == 1 &&
                    sc.device() == logits.device(),
                "seg_ce: scale must be one fp32 value on the logits' device");
    scale_ptr = IN_PTR(float, sc);
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
  torch::Tensor ws, part_db, dbias;  // undefined without write_grad
  if (write_grad) {
    ws = torch::empty({quads, 4, G, Cp}, fopts);
    part_db = torch::empty({(long)seg_ce_fin_rows(quads), G * Cp}, fopts);
    dbias = torch::empty({G, Cp}, fopts);
  }
  DISPATCH_FLOAT_BF16(logits.scalar_type(), "seg_ce", [&] {
    launch_seg_ce<scalar_t>(OUT_PTR(scalar_t, logits), bias_ptr, IN_PTR(unsigned char, labels),
                            OPT_OUT_PTR(float, ws), OUT_PTR(float, part_loss),
                            OUT_PTR(int, part_area), OPT_OUT_PTR(float, part_db),
                            OUT_PTR(float, loss), OUT_PTR(long, areas), OPT_OUT_PTR(float, dbias),
                            scale_ptr, M, (int)h, (int)w, (int)s, (int)G, (int)Cp, (int)C,
                            (float)grad_scale, write_grad, nblk, current_stream());
  });
  std::vector<torch::Tensor> ret = {loss, areas};
  if (write_grad) ret.push_back(dbias);
  return ret;
}

}  // namespace

void register_eval(pybind11::module_& mod) {
  mod.def("knn_topk", &knn_topk, py::arg("q"), py::arg("bank"), py::arg("k"),
          py::arg("splits") = 0);
  mod.def("probe_ce", &probe_ce, py::arg("logits"), py::arg("bias"), py::arg("labels"),
          py::arg("C"), py::arg("grad_scale"), py::arg("write_grad"), py::arg("row_blocks") = 0);
  mod.def("probe_sgd_", &probe_sgd_, py::arg("w"), py::arg("mom"), py::arg("grad"), py::arg("lr"),
          py::arg("wd"), py::arg("lr_scale"), py::arg("momentum"), py::arg("w_lp"));
  mod.def("seg_ce", &seg_ce, py::arg("logits"), py::arg("bias"), py::arg("labels"), py::arg("C"),
          py::arg("grad_scale"), py::arg("write_grad"), py::arg("scale") = py::none());
  mod.attr("SEG_MAX_CLASSES") = SEG_MAX_CLASSES;
}
