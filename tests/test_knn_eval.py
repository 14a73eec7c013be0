"""k-NN evaluation on the CPU: the plain-torch top-k oracle, the sharded
evaluation on planted clusters, the unchanged single-process path, and a gloo
world-2 run against the single-process result."""

import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLD = 2


def test_knn_topk_ref_against_brute_force():
    from dinov3_amd.ops import knn_topk_ref

    g = torch.Generator().manual_seed(3)
    q = torch.randint(-2, 3, (7, 4), generator=g).float()
    bank = torch.randint(-2, 3, (19, 4), generator=g).float()
    bank[11] = bank[2]  # a guaranteed tie in every row
    k = 6
    val, idx = knn_topk_ref(q, bank, k)
    assert val.dtype == torch.float32 and idx.dtype == torch.int64
    ties = 0
    for r in range(7):
        sims = [sum(float(q[r, d]) * float(bank[n, d]) for d in range(4)) for n in range(19)]
        order = sorted(range(19), key=lambda n: (-sims[n], n))[:k]
        assert idx[r].tolist() == order
        assert val[r].tolist() == [sims[n] for n in order]
        ties += len(order) - len({sims[n] for n in order})
    assert ties > 0


def planted_clusters(seed=0, classes=8, dim=64, bank_per_class=32, query_per_class=8):
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(classes, dim, generator=g), dim=1)

    def replicas(n):
        x = protos.repeat_interleave(n, dim=0)
        return x + 1e-2 * torch.randn(x.shape, generator=g), torch.arange(classes).repeat_interleave(n)

    return replicas(bank_per_class) + replicas(query_per_class)


def test_evaluate_knn_sharded_planted_clusters():
    from dinov3_amd.eval import evaluate_knn_sharded

    bank, bank_labels, query, query_labels = planted_clusters()
    ks = (1, 10, 20)  # at most the 32 replicas per class: every neighbour is same-class
    for precision in ("bf16", "fp32"):
        accs = evaluate_knn_sharded(bank, bank_labels, query, query_labels, ks=ks,
                                    precision=precision, query_chunk=24)
        assert accs == {1: 1.0, 10: 1.0, 20: 1.0}
        accs = evaluate_knn_sharded(bank, bank_labels, query, (query_labels + 1) % 8, ks=ks,
                                    precision=precision)
        assert accs == {1: 0.0, 10: 0.0, 20: 0.0}


def _evaluate_knn_before(train_features, train_labels, test_features, test_labels, k=20,
                         temperature=0.07, num_classes=None, chunk=1024):
    """evaluate_knn as it was before the sharded evaluation was added."""
    num_classes = num_classes or int(max(train_labels.max(), test_labels.max()).item()) + 1
    train_features = torch.nn.functional.normalize(train_features, dim=1)
    test_features = torch.nn.functional.normalize(test_features, dim=1)
    correct = 0
    total = test_features.shape[0]
    k = min(k, train_features.shape[0])
    for i in range(0, total, chunk):
        tf = test_features[i: i + chunk]
        sim = tf @ train_features.T
        topk_sim, topk_idx = sim.topk(k, dim=1)
        topk_labels = train_labels[topk_idx]
        weights = (topk_sim / temperature).exp()
        votes = torch.zeros(tf.shape[0], num_classes)
        votes.scatter_add_(1, topk_labels, weights)
        pred = votes.argmax(dim=1)
        correct += (pred == test_labels[i: i + chunk]).sum().item()
    return correct / max(total, 1)


def test_evaluate_knn_cpu_path_unchanged():
    from dinov3_amd.eval import evaluate_knn

    torch.manual_seed(0)  # the data of test_eval_knn_and_linear
    c0 = torch.randn(50, 16) + torch.tensor([5.0] + [0.0] * 15)
    c1 = torch.randn(50, 16) - torch.tensor([5.0] + [0.0] * 15)
    feats = torch.cat([c0, c1])
    labels = torch.cat([torch.zeros(50), torch.ones(50)]).long()
    assert evaluate_knn(feats, labels, feats, labels, k=5) == \
        _evaluate_knn_before(feats, labels, feats, labels, k=5)
    # a harder split, so that the value is not simply 1.0
    noisy = feats + 6.0 * torch.randn(100, 16)
    assert evaluate_knn(feats, labels, noisy, labels, k=7, chunk=32) == \
        _evaluate_knn_before(feats, labels, noisy, labels, k=7, chunk=32)


# ------------------------------------------------------------------ gloo
KS = (1, 5, 21)  # the bank shards hold 21 and 20 rows: rank 1 has fewer than max(ks)


def _sign_data():
    """+-1 features in D = 64: every row has norm 8, the normalised entries
    +-1/8 and all dot products are exact in bf16 / fp32, so ties are exact and
    frequent; some bank rows are copies of others across the two shards."""
    g = torch.Generator().manual_seed(11)
    bank = torch.randint(0, 2, (41, 64), generator=g).float() * 2 - 1
    bank[20] = bank[5]
    bank[33] = bank[5]
    bank[8] = bank[40]
    query = torch.randint(0, 2, (13, 64), generator=g).float() * 2 - 1
    query[3] = bank[5]
    bank_labels = torch.randint(0, 4, (41,), generator=g)
    query_labels = torch.randint(0, 4, (13,), generator=g)
    return bank, bank_labels, query, query_labels


def _sharded_worker(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from dinov3_amd.eval import evaluate_knn_sharded

    bank, bank_labels, query, query_labels = _sign_data()
    accs, vals, ids = evaluate_knn_sharded(
        bank[rank::WORLD], bank_labels[rank::WORLD], query[rank::WORLD],
        query_labels[rank::WORLD], ks=KS, query_chunk=6, return_neighbours=True)
    dist.destroy_process_group()
    # single process, full sets
    ref_accs, ref_vals, ref_ids = evaluate_knn_sharded(bank, bank_labels, query, query_labels,
                                                       ks=KS, return_neighbours=True)
    assert accs == ref_accs, (accs, ref_accs)
    assert torch.equal(ids, ref_ids[rank::WORLD]), (ids, ref_ids[rank::WORLD])
    assert torch.equal(vals, ref_vals[rank::WORLD])
    # the tie rule was exercised: equal similarities next to each other, ids ascending
    tied = ref_vals[:, 1:] == ref_vals[:, :-1]
    assert bool(tied.any())
    assert bool((ref_ids[:, 1:][tied] > ref_ids[:, :-1][tied]).all())
    assert ref_ids[3, :3].tolist() == [5, 20, 33]


def test_evaluate_knn_sharded_world2_matches_single_process():
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_sharded_worker, args=(r, 29531)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    for p in procs:
        assert p.exitcode == 0, f"child exited with {p.exitcode}"
