"""k-NN evaluation on the device: evaluate_knn with device tensors, feature
extraction that stays on the device, and do_test behind DINOV3_EVAL_ON_DEVICE."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def planted_clusters(seed=0, classes=8, dim=64, bank_per_class=32, query_per_class=8):
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(classes, dim, generator=g), dim=1)

    def replicas(n):
        x = protos.repeat_interleave(n, dim=0)
        return x + 1e-2 * torch.randn(x.shape, generator=g), torch.arange(classes).repeat_interleave(n)

    return replicas(bank_per_class) + replicas(query_per_class)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_evaluate_knn_device_tensors(precision):
    from dinov3_amd.eval import evaluate_knn

    bank, bank_labels, query, query_labels = (t.cuda() for t in planted_clusters())
    # k <= 32 replicas per class: every neighbour is same-class
    assert evaluate_knn(bank, bank_labels, query, query_labels, k=20, precision=precision) == 1.0
    assert evaluate_knn(bank, bank_labels, query, (query_labels + 1) % 8, k=20,
                        precision=precision) == 0.0


def test_evaluate_knn_device_pads_feature_dim():
    """D = 16 is no multiple of the kernel's 32: the evaluation pads with zero
    columns, and the device result equals the CPU form of the same protocol."""
    from dinov3_amd.eval import evaluate_knn, evaluate_knn_sharded

    torch.manual_seed(0)  # two well-separated clusters, as test_eval_knn_and_linear
    c0 = torch.randn(50, 16) + torch.tensor([5.0] + [0.0] * 15)
    c1 = torch.randn(50, 16) - torch.tensor([5.0] + [0.0] * 15)
    feats = torch.cat([c0, c1])
    labels = torch.cat([torch.zeros(50), torch.ones(50)]).long()
    acc = evaluate_knn(feats.cuda(), labels.cuda(), feats.cuda(), labels.cuda(), k=5)
    assert acc > 0.95
    assert acc == evaluate_knn_sharded(feats, labels, feats, labels, ks=(5,))[5]


def test_extract_features_stays_on_device():
    from dinov3_amd.eval import extract_features

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 4 * 4, 32)).cuda()
    loader = [(torch.randn(5, 3, 4, 4), torch.arange(5)), (torch.randn(3, 3, 4, 4), torch.arange(3))]
    dev = torch.device("cuda", 0)
    feats, labels = extract_features(model, loader, device=dev, to_cpu=False)
    ref_feats, ref_labels = extract_features(model, loader, device=dev)
    assert feats.is_cuda and labels.is_cuda and not ref_feats.is_cuda and not ref_labels.is_cuda
    assert feats.shape == (8, 32) and feats.dtype == torch.float32
    assert torch.equal(feats.cpu(), ref_feats) and torch.equal(labels.cpu(), ref_labels)


def test_do_test_eval_on_device(smoke_cfg, monkeypatch):
    from dinov3_amd.train.ssl_meta_arch import SSLMetaArch
    from dinov3_amd.train.train import do_test

    monkeypatch.setenv("DINOV3_EVAL_ON_DEVICE", "1")
    cfg = copy.deepcopy(smoke_cfg)
    cfg.train.dataset_path = "Synthetic:split=TRAIN:length=32"
    model = SSLMetaArch(cfg)
    results = do_test(cfg, model, iteration=0)
    keys = ["knn_top1"] + [f"knn_top1_k{k}" for k in (10, 20, 100, 200)]
    for key in keys:
        assert 0.0 <= results[key] <= 1.0, (key, results[key])
    assert results["knn_top1"] == results["knn_top1_k20"]
    assert "linear_top1" in results
