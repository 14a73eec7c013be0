"""Linear-probe grid evaluation on the CPU: one head against torch.optim.SGD,
the grid against one-head runs, planted clusters and the tie rule, the two
plain-torch oracles against literal computations, and a gloo world-2 run
against the single-process result."""

import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLD = 2


def overlapping_classes(seed=0, classes=10, dim=32, n_train=1000, n_val=400):
    """Overlapping Gaussian classes with a common offset of +3, so that
    standardising matters."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(classes, dim, generator=g)

    def draw(n):
        y = torch.randint(0, classes, (n,), generator=g)
        return centres[y] + 1.5 * torch.randn(n, dim, generator=g) + 3.0, y

    return draw(n_train) + draw(n_val)


def planted_clusters(seed=0, classes=8, dim=64, train_per_class=32, val_per_class=8):
    g = torch.Generator().manual_seed(seed)
    protos = torch.nn.functional.normalize(torch.randn(classes, dim, generator=g), dim=1)

    def replicas(n):
        x = protos.repeat_interleave(n, dim=0)
        return x + 1e-2 * torch.randn(x.shape, generator=g), torch.arange(classes).repeat_interleave(n)

    return replicas(train_per_class) + replicas(val_per_class)


def test_one_head_matches_torch_sgd():
    from dinov3_amd.eval.linear import _linear_sharded

    xt, yt, xv, yv = overlapping_classes()
    lr, wd, epochs, batch = 0.1, 1e-3, 3, 128
    out, state = _linear_sharded(xt, yt, xv, yv, (lr,), (wd,), epochs, batch, None, "fp32", True,
                                 0, None, 8192)
    mean = xt.double().mean(dim=0)
    inv_std = (xt.double().var(dim=0, unbiased=False) + 1e-6).rsqrt()
    st, sv = ((xt.double() - mean) * inv_std).float(), ((xv.double() - mean) * inv_std).float()
    got = sv @ state["weight"][0].T + state["bias"][0]

    clf = torch.nn.Linear(32, 10)
    torch.nn.init.zeros_(clf.weight)
    torch.nn.init.zeros_(clf.bias)
    opt = torch.optim.SGD([{"params": [clf.weight], "weight_decay": wd},
                           {"params": [clf.bias], "weight_decay": 0.0}], lr=lr, momentum=0.9)
    total, t = epochs * math.ceil(1000 / batch), 0
    for epoch in range(epochs):
        perm = torch.randperm(1000, generator=torch.Generator().manual_seed(epoch))
        for i in range(0, 1000, batch):
            idx = perm[i: i + batch]
            for group in opt.param_groups:
                group["lr"] = lr * 0.5 * (1.0 + math.cos(math.pi * t / total))
            opt.zero_grad()
            torch.nn.functional.cross_entropy(clf(st[idx]), yt[idx]).backward()
            opt.step()
            t += 1
    with torch.no_grad():
        want = clf(sv)
    assert t == 24
    diff = float((got - want).abs().max())
    print(f"max |val logit difference| = {diff:.3e}, max |weight difference| = "
          f"{float((state['weight'][0] - clf.weight.detach()).abs().max()):.3e}")
    assert diff <= 1e-5
    assert out["top1"][0] == int((want.argmax(dim=1) == yv).sum()) / 400
    assert out["val_loss"][0] == pytest.approx(
        float(torch.nn.functional.cross_entropy(want, yv)), rel=1e-5)


def test_grid_head_equals_one_head_run():
    from dinov3_amd.eval import evaluate_linear_sharded

    xt, yt, xv, yv = overlapping_classes()
    lrs, wds = (1e-3, 1e-2, 1e-1, 1.0), (0.0, 1e-3)
    kwargs = dict(epochs=3, batch_size=128, precision="fp32")
    grid = evaluate_linear_sharded(xt, yt, xv, yv, lrs=lrs, wds=wds, **kwargs)
    assert grid["heads"] == [(lr, wd) for lr in lrs for wd in wds]  # lr-major
    assert len(set(grid["top1"])) > 1  # the heads do differ on this data
    for g, (lr, wd) in enumerate(grid["heads"]):
        one = evaluate_linear_sharded(xt, yt, xv, yv, lrs=(lr,), wds=(wd,), **kwargs)
        assert grid["top1"][g] == one["top1"][0]
        assert torch.allclose(torch.tensor(grid["val_loss"][g]), torch.tensor(one["val_loss"][0]),
                              rtol=1e-5, atol=0.0)
    best = grid["best_head"]
    assert grid["best_top1"] == grid["top1"][best] == max(grid["top1"])
    assert best == grid["top1"].index(max(grid["top1"]))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_planted_clusters_every_head_perfect_and_tie_rule(precision):
    from dinov3_amd.eval import evaluate_linear_sharded

    xt, yt, xv, yv = planted_clusters()
    out = evaluate_linear_sharded(xt, yt, xv, yv, lrs=(1e-3, 1e-2, 1e-1, 1.0), epochs=10,
                                  batch_size=48, precision=precision)
    assert out["top1"] == [1.0] * 4
    assert out["best_head"] == 0 and out["best_top1"] == 1.0  # ties go to the lowest index
    wrong = evaluate_linear_sharded(xt, yt, xv, (yv + 1) % 8, lrs=(1e-1,), epochs=10,
                                    batch_size=48, precision=precision)
    assert wrong["top1"] == [0.0]


def test_probe_ce_ref_against_literal_rows():
    from dinov3_amd.ops import probe_ce_ref

    B, G, C, Cp = 9, 2, 5, 8
    gen = torch.Generator().manual_seed(5)
    logits = torch.randint(-2, 3, (B, G, Cp), generator=gen).float()
    bias = torch.randint(-1, 2, (G, Cp), generator=gen).float()
    logits[:, :, C:] = 9.0  # the pad columns hold the largest values and must not count
    labels = torch.randint(0, C, (B,), generator=gen)
    labels[4] = -1
    scale = 0.25
    work = logits.clone()
    loss_sum, correct, dbias = probe_ce_ref(work, bias, labels, C, scale, True)
    assert loss_sum.dtype == torch.float32 and correct.dtype == torch.int64
    assert dbias.dtype == torch.float32 and dbias.shape == (G, Cp)
    ties = 0
    for g in range(G):
        want_loss, want_correct, want_db = 0.0, 0, [0.0] * C
        for b in range(B):
            z = [float(logits[b, g, c]) + float(bias[g, c]) for c in range(C)]
            top = max(z)
            ties += z.count(top) > 1
            denom = sum(math.exp(v - top) for v in z)
            lab = int(labels[b])
            if lab < 0:
                assert work[b, g].tolist() == [0.0] * Cp
                continue
            want_loss += math.log(denom) + top - z[lab]
            want_correct += z.index(top) == lab  # the lowest index among the maxima
            grad = [(math.exp(v - top) / denom - (c == lab)) * scale for c, v in enumerate(z)]
            want_db = [a + d for a, d in zip(want_db, grad)]
            assert torch.allclose(work[b, g, :C].double(), torch.tensor(grad).double(),
                                  rtol=0, atol=1e-6)
            assert work[b, g, C:].tolist() == [0.0] * (Cp - C)
        assert float(loss_sum[g]) == pytest.approx(want_loss, rel=1e-6)
        assert int(correct[g]) == want_correct
        assert torch.allclose(dbias[g, :C].double(), torch.tensor(want_db).double(), rtol=0,
                              atol=1e-6)
        assert dbias[g, C:].tolist() == [0.0] * (Cp - C)
    assert ties > 0
    # without the gradient the logits stay and the sums are the same
    keep = logits.clone()
    loss2, correct2, none = probe_ce_ref(keep, bias, labels, C, scale, False)
    assert none is None and torch.equal(keep, logits)
    assert torch.equal(loss2, loss_sum) and torch.equal(correct2, correct)


@pytest.mark.parametrize("with_wd", [False, True])
def test_probe_sgd_ref_formula(with_wd):
    from dinov3_amd.ops import probe_sgd_ref_

    G, R = 3, 16
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(G, R, generator=gen)
    mom = torch.randn(G, R, generator=gen)
    lr = torch.tensor([0.1, 0.01, 1.0])
    wd = torch.tensor([0.0, 1e-2, 0.5]) if with_wd else None
    w_lp = torch.zeros(G, R, dtype=torch.bfloat16)
    want_w, want_m = w.double().clone(), mom.double().clone()
    for step, scale in enumerate((1.0, 0.7)):
        grad = torch.randn(G, R, generator=gen)
        if step == 1:
            grad = grad.bfloat16()
        probe_sgd_ref_(w, mom, grad, lr, wd, scale, 0.9, w_lp)
        for g in range(G):
            gp = grad[g].double() + (float(wd[g]) if with_wd else 0.0) * want_w[g]
            want_m[g] = 0.9 * want_m[g] + gp
            want_w[g] = want_w[g] - float(lr[g]) * scale * want_m[g]
        assert torch.allclose(w.double(), want_w, rtol=1e-6, atol=1e-6)
        assert torch.allclose(mom.double(), want_m, rtol=1e-6, atol=1e-6)
        assert torch.equal(w_lp, w.bfloat16())
        want_w, want_m = w.double().clone(), mom.double().clone()  # no drift between the steps


def test_more_than_2048_classes_raises():
    from dinov3_amd.eval import evaluate_linear_sharded

    x = torch.randn(4, 8)
    y = torch.tensor([0, 1, 2, 2048])
    with pytest.raises(ValueError, match="2048"):
        evaluate_linear_sharded(x, y, x, y, epochs=1)
    with pytest.raises(ValueError, match="2048"):
        evaluate_linear_sharded(x, y.clamp(max=3), x, y.clamp(max=3), epochs=1, num_classes=2049)


# ------------------------------------------------------------------ gloo
def _small_set():
    """41 train and 13 val rows: the rank-strided shards are unequal."""
    xt, yt, xv, yv = overlapping_classes(seed=3, classes=4, dim=12, n_train=41, n_val=13)
    return xt, yt, xv, yv


def _sharded_worker(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    from dinov3_amd.eval import evaluate_linear_sharded

    xt, yt, xv, yv = _small_set()
    shards = (xt[rank::WORLD], yt[rank::WORLD], xv[rank::WORLD], yv[rank::WORLD])
    grids = [dict(lrs=(1e-2, 1e-1, 1.0)), dict(lrs=(1e-1,))]  # 3 heads; 1 head: rank 1 is idle
    kwargs = dict(epochs=4, batch_size=16, num_classes=4, precision="fp32")
    got = [evaluate_linear_sharded(*shards, **grid, **kwargs) for grid in grids]
    # explicit ids in another order give the same result
    order = torch.randperm(shards[0].shape[0], generator=torch.Generator().manual_seed(1))
    ids = rank + WORLD * order
    got.append(evaluate_linear_sharded(shards[0][order], shards[1][order], shards[2], shards[3],
                                       sample_ids=ids, **grids[0], **kwargs))
    dist.destroy_process_group()
    # single process, full sets
    for out, grid in zip(got, grids + grids[:1]):
        ref = evaluate_linear_sharded(xt, yt, xv, yv, **grid, **kwargs)
        assert out["top1"] == ref["top1"], (out, ref)
        assert out["best_head"] == ref["best_head"] and out["heads"] == ref["heads"]
        for key in ("val_loss", "train_loss"):
            assert torch.allclose(torch.tensor(out[key]), torch.tensor(ref[key]), rtol=1e-5,
                                  atol=0.0), (key, out[key], ref[key])
        assert all(v > 0 for v in ref["train_loss"])


def test_evaluate_linear_sharded_world2_matches_single_process():
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_sharded_worker, args=(r, 29541)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
    for p in procs:
        assert p.exitcode == 0, f"child exited with {p.exitcode}"
