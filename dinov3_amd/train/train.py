"""Training entrypoint + hot loop.

Parity: dinov3_jax/train/train.py (CLI :51-72, schedulers :127-208, optimizer
:75-122, do_train :319-712) with the reference's defects fixed (SURVEY §8 B1:
optimizer updates APPLY; B2: EMA updates the live teacher).

MI355X process model: torchrun one rank per GPU over RCCL; batches move
host->device with pinned memory + non-blocking copies; gradient reduction
overlaps backward (parallel/ddp.py or the sharding engine in parallel/fsdp.py).
"""

from __future__ import annotations

import math
import argparse
import logging
import os
import sys
from functools import partial
from typing import Dict

import torch

from .. import parallel
from ..checkpointer import find_latest_checkpoint, load_checkpoint, save_checkpoint
from ..configs import setup_config, setup_job
from ..data import (
    DataAugmentationDINO,
    MaskingGenerator,
    SamplerType,
    collate_data_and_cast,
    make_data_loader,
    make_dataset,
)
from ..logging import MetricLogger, setup_logging
from ..parallel.ddp import GradReducer
from .cosine_lr_scheduler import CosineScheduler, linear_warmup_cosine_decay
from .optim import FusedAdamW
from .ssl_meta_arch import SSLMetaArch

logger = logging.getLogger("dinov3")

DTYPE_MAP = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32,
             "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def get_args_parser(add_help: bool = True) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser("DINOv3 MI355X training", add_help=add_help)
    parser.add_argument("--config-file", default="", metavar="FILE", help="path to config file")
    parser.add_argument("--no-resume", action="store_true", help="do not attempt to resume")
    parser.add_argument("--eval-only", action="store_true")
    parser.add_argument("--eval", type=str, default="", help="eval type")
    parser.add_argument("--profiling", action="store_true", help="emit roctx/profiler ranges")
    parser.add_argument("--multi-distillation", action="store_true")
    parser.add_argument("--record-ref-losses", action="store_true",
                        help="dump per-iteration loss terms to ref_losses.json for parity checks")
    parser.add_argument("--ref-losses-path", type=str, default="",
                        help="compare per-iteration losses against a recorded JSON")
    parser.add_argument("--test-ibot", action="store_true", help="run with dino/koleo weights zeroed")
    parser.add_argument("--benchmark-codebase", action="store_true",
                        help="time the train step and print images/sec at exit")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--output-dir", default="", help="output directory")
    parser.add_argument("--max-iterations", type=int, default=-1, help="cap iterations (debug/bench)")
    parser.add_argument("opts", nargs=argparse.REMAINDER,
                        help="config overrides as key=value dotlist")
    return parser


def build_schedulers(cfg) -> Dict[str, object]:
    epoch_len = cfg.train.OFFICIAL_EPOCH_LENGTH
    total = cfg.optim.epochs * epoch_len
    schedules_v2 = cfg.get("schedules")
    if schedules_v2:
        def mk(s, total_iters):
            return linear_warmup_cosine_decay(
                start=s["start"], peak=s["peak"], end=s["end"],
                warmup_iterations=int(s.get("warmup_epochs", 0) * epoch_len),
                total_iterations=total_iters,
                cosine_iterations=int(s["cosine_epochs"] * epoch_len) if "cosine_epochs" in s else None,
            )

        lr = mk(schedules_v2["lr"], total)
        wd = mk(schedules_v2["weight_decay"], total)
        momentum = mk(schedules_v2["momentum"], total)
        teacher_temp = mk(schedules_v2["teacher_temp"], total)
        freeze_iters = int(schedules_v2["lr"].get("freeze_last_layer_epochs", 0) * epoch_len)
    else:
        lr = CosineScheduler(
            base_value=cfg.optim.lr, final_value=cfg.optim.min_lr, total_iters=total,
            warmup_iters=int(cfg.optim.warmup_epochs * epoch_len),
            start_warmup_value=0.0, trunc_extra=cfg.optim.schedule_trunc_extra,
        )
        wd = CosineScheduler(
            base_value=cfg.optim.weight_decay, final_value=cfg.optim.weight_decay_end, total_iters=total,
        )
        momentum = CosineScheduler(
            base_value=cfg.teacher.momentum_teacher, final_value=cfg.teacher.final_momentum_teacher,
            total_iters=total,
        )
        teacher_temp = CosineScheduler(
            base_value=cfg.teacher.teacher_temp, final_value=cfg.teacher.teacher_temp, total_iters=total,
            warmup_iters=int(cfg.teacher.warmup_teacher_temp_epochs * epoch_len),
            start_warmup_value=cfg.teacher.warmup_teacher_temp,
        )
        freeze_iters = int(cfg.optim.freeze_last_layer_epochs * epoch_len)
    return {
        "lr": lr,
        "wd": wd,
        "momentum": momentum,
        "teacher_temp": teacher_temp,
        "freeze_last_layer_iterations": freeze_iters,
        "total_iterations": total,
    }


def build_optimizer(cfg, params_groups) -> FusedAdamW:
    return FusedAdamW(
        params_groups,
        beta1=cfg.optim.adamw_beta1,
        beta2=cfg.optim.adamw_beta2,
        use_master_weights=True,
    )


def build_training_engine(cfg, params_groups):
    """Select the distributed engine per compute_precision.sharding_strategy.

    SHARD_GRAD_OP / FULL_SHARD + world>1 -> ShardedEngine (ZeRO-2 style:
    resident full params, fp32 grad reduce-scatter overlapped with backward,
    sharded optimizer state, bf16 param all-gather after the step).
    Otherwise -> FusedAdamW + bucketed all-reduce GradReducer (NO_SHARD/DDP).

    Returns (optimizer-like, finalize_backward_fn).
    """
    # grads reduce over the training subgroup (the world unless
    # multi-distillation set a per-student subgroup)
    world = parallel.subgroup_size()
    strategy = cfg.compute_precision.sharding_strategy
    if world > 1 and strategy in ("SHARD_GRAD_OP", "FULL_SHARD"):
        from ..parallel.fsdp import ShardedEngine

        engine = ShardedEngine(params_groups, beta1=cfg.optim.adamw_beta1,
                               beta2=cfg.optim.adamw_beta2,
                               process_group=parallel.subgroup())
        return engine, engine.finalize_backward
    optimizer = build_optimizer(cfg, params_groups)
    student_params = [p for g in params_groups for p in g["params"]]
    reducer = GradReducer(student_params, reduce_dtype=torch.float32
                          if cfg.compute_precision.reduce_dtype == "fp32" else None)
    return optimizer, reducer.finalize


def build_multi_resolution_data_loader_from_cfg(cfg, model: SSLMetaArch, start_iter: int = 0):
    """Multi-resolution crop schedules: crops.global_crops_size may be a list
    of sizes (paired with local sizes + ratios) — one loader per resolution,
    combined by sampling ratio (reference train.py:718-769)."""
    g_sizes = cfg.crops.global_crops_size
    if isinstance(g_sizes, int):
        return build_data_loader_from_cfg(cfg, model, start_iter)
    from ..data.loaders import CombinedDataLoader
    import copy

    l_sizes = cfg.crops.local_crops_size
    if isinstance(l_sizes, int):
        l_sizes = [l_sizes] * len(g_sizes)
    ratios = cfg.crops.global_local_crop_pairs_ratios
    if isinstance(ratios, (int, float)):
        ratios = [float(ratios)] * len(g_sizes)
    loaders = []
    for i, (gs, ls) in enumerate(zip(g_sizes, l_sizes)):
        sub = copy.deepcopy(cfg)
        sub.crops.global_crops_size = gs
        sub.crops.local_crops_size = ls
        # decorrelate per-resolution streams (reference train.py:755)
        sub.train.seed = cfg.train.seed + i + 1
        loaders.append(build_data_loader_from_cfg(sub, model, start_iter))
    logger.info("multi-resolution loader: sizes %s ratios %s", list(g_sizes), ratios)
    return CombinedDataLoader(loaders, ratios, seed=cfg.train.seed)


def build_data_loader_from_cfg(cfg, model: SSLMetaArch, start_iter: int = 0):
    img_size = cfg.crops.global_crops_size
    patch_size = cfg.student.patch_size
    n_tokens = (img_size // patch_size) ** 2
    mask_generator = MaskingGenerator(
        input_size=(img_size // patch_size, img_size // patch_size),
        max_num_patches=int(0.5 * n_tokens),
    )
    transform = DataAugmentationDINO(
        cfg.crops.global_crops_scale,
        cfg.crops.local_crops_scale,
        cfg.crops.local_crops_number,
        global_crops_size=cfg.crops.global_crops_size,
        local_crops_size=cfg.crops.local_crops_size,
        gram_teacher_crops_size=cfg.crops.gram_teacher_crops_size,
        gram_teacher_no_distortions=cfg.crops.gram_teacher_no_distortions,
        local_crops_subset_of_global_crops=cfg.crops.localcrops_subset_of_globalcrops,
        patch_size=patch_size,
        share_color_jitter=cfg.crops.share_color_jitter,
        horizontal_flips=cfg.crops.horizontal_flips,
        mean=cfg.crops.rgb_mean,
        std=cfg.crops.rgb_std,
    )
    collate_fn = partial(
        collate_data_and_cast,
        mask_ratio_tuple=tuple(cfg.ibot.mask_ratio_min_max),
        mask_probability=cfg.ibot.mask_sample_probability,
        n_tokens=n_tokens,
        mask_generator=mask_generator,
        random_circular_shift=cfg.ibot.mask_random_circular_shift,
        dtype=DTYPE_MAP.get(cfg.compute_precision.param_dtype, torch.float32),
    )
    dataset = make_dataset(
        dataset_str=cfg.train.dataset_path,
        transform=transform,
        target_transform=lambda _: (),
    )
    # Resume must not replay the sequence from iteration 0: the sampler is
    # advanced by the consumed sample count and the seed offset by start_iter
    # (reference train.py:838-840).
    return make_data_loader(
        dataset=dataset,
        batch_size=cfg.train.batch_size_per_gpu,
        num_workers=cfg.train.num_workers,
        shuffle=True,
        seed=cfg.train.seed + start_iter + 1,
        sampler_type=SamplerType.EPOCH,
        sampler_advance=start_iter * cfg.train.batch_size_per_gpu,
        drop_last=True,
        collate_fn=collate_fn,
    )


def batch_to_device(data: dict, device: torch.device) -> dict:
    return {
        k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v)
        for k, v in data.items()
    }


def do_train(cfg, model: SSLMetaArch, resume: bool = True, max_iterations: int = -1,
             record_losses_to: str = "", compare_losses_to: str = "", profiling: bool = False):
    device = parallel.device()
    param_dtype = DTYPE_MAP.get(cfg.compute_precision.param_dtype, torch.float32)
    if device.type == "cuda":
        model = model.to(device=device, dtype=param_dtype)
    else:
        model = model.to(device)  # fp32 reference path on CPU
    model.train()

    schedulers = build_schedulers(cfg)
    params_groups = model.get_params_groups()
    optimizer, finalize_backward = build_training_engine(cfg, params_groups)

    start_iter = 0
    output_dir = cfg.train.output_dir
    if resume and output_dir:
        latest = find_latest_checkpoint(output_dir)
        if latest is not None:
            # distillation checkpoints omit the frozen teacher (it is rebuilt
            # from distillation.checkpoint_path at construction)
            payload = load_checkpoint(
                latest, model, optimizer,
                strict=not getattr(model, "is_distillation_enabled", False))
            start_iter = payload["iteration"] + 1
            logger.info("resumed at iteration %d", start_iter)

    data_loader = build_multi_resolution_data_loader_from_cfg(cfg, model, start_iter)
    total_iterations = schedulers["total_iterations"]
    if max_iterations > 0:
        total_iterations = min(total_iterations, start_iter + max_iterations)
    ckpt_period = cfg.checkpointing.period

    metrics_file = None
    if output_dir:
        import os

        metrics_file = os.path.join(output_dir, "training_metrics.json")
    metric_logger = MetricLogger(delimiter="  ", output_file=metrics_file)
    header = "Train"

    nan_count = 0
    iteration = start_iter
    # frozen distillation teacher never changes: skip it in checkpoints
    skip_save_prefixes = (
        ("teacher_backbone.", "teacher_dino_head.", "teacher_ibot_head.")
        if getattr(model, "is_distillation_enabled", False) else None)
    # reconstruct how many gram refreshes a resumed run has already done
    # (reference train.py:605-615)
    num_gram_updates = 0
    if (model.gram_use_loss and cfg.gram.rep_update and start_iter > 0
            and start_iter >= cfg.gram.it_first_update):
        num_gram_updates = math.ceil(
            (start_iter + 1 - cfg.gram.it_first_update) / cfg.gram.update_frequency)
        logger.info("gram teacher refreshed %d times before iteration %d",
                    num_gram_updates, start_iter)
    recorded_losses = []
    reference_losses = None
    if compare_losses_to:
        import json

        with open(compare_losses_to) as f:
            reference_losses = json.load(f)

    def infinite_batches():
        epoch = 0
        while True:
            sampler = getattr(data_loader, "sampler", None)
            if sampler is not None and hasattr(sampler, "set_epoch"):
                sampler.set_epoch(epoch)
            elif hasattr(data_loader, "set_epoch"):  # CombinedDataLoader
                data_loader.set_epoch(epoch)
            yield from data_loader
            epoch += 1

    clip = cfg.optim.clip_grad
    batches = infinite_batches()
    prefetched = device.type == "cuda"
    if prefetched:
        # stage the next batch's H2D copies on a side stream, overlapped with
        # the current step's compute (data/prefetch.py)
        from ..data.prefetch import CudaBatchPrefetcher

        batches = CudaBatchPrefetcher(batches, device)
    for data in metric_logger.log_every(
        batches, 10, header, n_iterations=total_iterations, start_iteration=start_iter
    ):
        if iteration >= total_iterations:
            break
        it = iteration
        lr = schedulers["lr"][it]
        wd = schedulers["wd"][it]
        mom = schedulers["momentum"][it]
        teacher_temp = schedulers["teacher_temp"][it]
        last_layer_lr = 0.0 if it < schedulers["freeze_last_layer_iterations"] else lr

        if not prefetched:
            data = batch_to_device(data, device)
        if profiling and device.type == "cuda":
            torch.cuda.nvtx.range_push(f"step_{it}")  # roctx range on ROCm
        try:
            loss, loss_dict = model(data, teacher_temp=teacher_temp, iteration=it)
        except torch.OutOfMemoryError:
            # OOM retry on a shrunken batch (reference helper get_batch_subset,
            # collate.py:97-139, which the reference never wires up)
            from ..data import get_batch_subset

            logger.warning("OOM at iteration %d: retrying with half batch", it)
            if device.type == "cuda":
                torch.cuda.empty_cache()
            data = get_batch_subset(data, divide_by=2)
            loss, loss_dict = model(data, teacher_temp=teacher_temp, iteration=it)

        if not torch.isfinite(loss):
            nan_count += 1
            nan_logger = logging.getLogger("dinov3.nan")
            nan_logger.error("NaN/Inf loss at iteration %d (%d consecutive)", it, nan_count)
            if nan_count > 2:
                raise FloatingPointError(f"aborting: >{nan_count - 1} consecutive non-finite losses")
            optimizer.zero_grad()
            iteration += 1
            continue
        nan_count = 0

        loss.backward()
        finalize_backward()

        clip_scales = None
        if clip is not None and clip > 0:
            sums = optimizer.grad_norm_sums()  # [n_submodels], stays on device
            # Only shard-local sums need the cross-rank reduction; in the DDP
            # path grads are replicated and the sums are already global.
            if parallel.subgroup_size() > 1 and getattr(optimizer, "needs_norm_allreduce", True):
                import torch.distributed as dist

                dist.all_reduce(sums, group=parallel.subgroup())
            clip_scales = optimizer.clip_factors(sums, clip)
            if it % 10 == 0:  # avoid a host sync every step
                for name, s in zip(optimizer.submodels, sums.tolist()):
                    loss_dict[f"grad_norm_{name}"] = s ** 0.5

        optimizer.step(lr=lr, weight_decay=wd, last_layer_lr=last_layer_lr, clip_scales=clip_scales)
        optimizer.zero_grad()
        model.update_ema(mom)
        if profiling and device.type == "cuda":
            torch.cuda.nvtx.range_pop()

        # one-time gram init from the EMA teacher (gram.it_load_ema_teacher,
        # used when no gram checkpoint is configured)
        if (model.gram_use_loss and model.has_gram_teacher
                and model.gram_it_load_ema_teacher >= 0
                and it == model.gram_it_load_ema_teacher):
            logger.info("loading gram teacher from EMA teacher at iteration %d", it)
            model.update_gram_teacher()
        # gram-teacher refresh cadence (reference train.py:668-678): absolute
        # (it+1) phase, capped at gram.max_updates refreshes over the run
        if (model.gram_use_loss and cfg.gram.rep_update
                and (it + 1) >= cfg.gram.it_first_update
                and (it + 1) % cfg.gram.update_frequency == 0
                and (cfg.gram.max_updates is None
                     or num_gram_updates < cfg.gram.max_updates)):
            logger.info("updating gram teacher from EMA teacher after iteration %d", it)
            model.update_gram_teacher()
            num_gram_updates += 1

        metric_logger.update(
            lr=lr, wd=wd, mom=mom, last_layer_lr=last_layer_lr, teacher_temp=teacher_temp,
            total_loss=loss.item(),
            **{k: (v.item() if isinstance(v, torch.Tensor) else v) for k, v in loss_dict.items()
               if k != "total_loss"},
        )

        if record_losses_to or reference_losses is not None:
            entry = {"iteration": it, "total_loss": float(loss.detach())}
            entry.update({k: float(v) for k, v in loss_dict.items()
                          if isinstance(v, (int, float)) or (isinstance(v, torch.Tensor) and v.ndim == 0)})
            if record_losses_to:
                recorded_losses.append(entry)
            if reference_losses is not None and it < len(reference_losses):
                ref = reference_losses[it]
                for k, v in entry.items():
                    if k in ref and abs(v - ref[k]) > 0.05 * max(1.0, abs(ref[k])):
                        logger.warning("loss parity drift at it=%d %s: %g vs ref %g",
                                       it, k, v, ref[k])

        eval_period = cfg.evaluation.eval_period_iterations
        if eval_period and eval_period > 0 and (it + 1) % eval_period == 0:
            try:
                results = do_test(cfg, model, it)
                metric_logger.update(**{f"eval_{k}": v for k, v in results.items()
                                        if isinstance(v, (int, float))})
            except Exception as e:  # eval must never kill training
                logger.warning("periodic eval failed at it=%d: %s", it, e)
            model.train()

        if output_dir and ckpt_period > 0 and (it + 1) % ckpt_period == 0:
            save_checkpoint(
                output_dir, it, model, optimizer,
                max_to_keep=cfg.checkpointing.max_to_keep, keep_every=cfg.checkpointing.keep_every,
                skip_prefixes=skip_save_prefixes,
            )
        iteration += 1

    if record_losses_to and parallel.is_main_process():
        import json

        with open(record_losses_to, "w") as f:
            json.dump(recorded_losses, f)
        logger.info("recorded %d iterations of losses to %s", len(recorded_losses), record_losses_to)
    already_saved = ckpt_period > 0 and iteration % ckpt_period == 0 and iteration > 0
    if output_dir and not already_saved:
        save_checkpoint(
            output_dir, iteration - 1, model, optimizer,
            max_to_keep=cfg.checkpointing.max_to_keep, keep_every=cfg.checkpointing.keep_every,
            skip_prefixes=skip_save_prefixes,
        )
    metric_logger.synchronize_between_processes()
    logger.info("training done at iteration %d", iteration)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def do_test(cfg, model, iteration: int):
    """k-NN + linear-probe eval of the teacher backbone on the configured
    dataset (synthetic decode in this offline environment)."""
    from ..data import SamplerType, make_data_loader, make_dataset
    from ..data.transforms import make_eval_transform
    from ..eval import evaluate_knn, evaluate_linear_probe, extract_features

    device = parallel.device()
    backbone = model.teacher_backbone if hasattr(model, "teacher_backbone") else model
    backbone = backbone.to(device)
    transform = make_eval_transform(crop_size=cfg.crops.global_crops_size,
                                    mean=cfg.crops.rgb_mean, std=cfg.crops.rgb_std)
    base = cfg.train.dataset_path.split(":")[0]
    train_ds = make_dataset(dataset_str=f"{base}:split=TRAIN:length=2048"
                            if base == "Synthetic" else f"{base}:split=TRAIN",
                            transform=transform)
    val_ds = make_dataset(dataset_str=f"{base}:split=VAL:length=512"
                          if base == "Synthetic" else f"{base}:split=VAL",
                          transform=transform)
    kwargs = dict(batch_size=64, num_workers=cfg.train.num_workers, shuffle=False,
                  sampler_type=SamplerType.EPOCH, drop_last=False)
    # DINOV3_EVAL_ON_DEVICE=1: features stay on the device and the k-NN number
    # comes from evaluate_knn_sharded, which is correct for any world size (the
    # sampler gives every rank 1/world of both sets; the default path scores a
    # rank's val slice against its own train slice only). The linear number then
    # is the best head of evaluate_linear_sharded's lr grid, trained on the whole
    # train set whatever the world size; the default path trains one head on the
    # local shard.
    on_device = os.environ.get("DINOV3_EVAL_ON_DEVICE", "0") == "1"
    train_feats, train_labels = extract_features(
        backbone, make_data_loader(dataset=train_ds, **kwargs), to_cpu=not on_device)
    val_feats, val_labels = extract_features(
        backbone, make_data_loader(dataset=val_ds, **kwargs), to_cpu=not on_device)
    results = {"iteration": iteration}
    if on_device:
        from ..eval import evaluate_knn_sharded, evaluate_linear_sharded

        accs = evaluate_knn_sharded(train_feats, train_labels, val_feats, val_labels,
                                    ks=(10, 20, 100, 200))
        results["knn_top1"] = accs[20]
        results.update({f"knn_top1_k{k}": acc for k, acc in accs.items()})
        probe = evaluate_linear_sharded(train_feats, train_labels, val_feats, val_labels)
        results["linear_top1"] = probe["best_top1"]
        results["linear_best_lr"] = probe["heads"][probe["best_head"]][0]
        results.update({f"linear_top1_head{i}": acc for i, acc in enumerate(probe["top1"])})
    else:
        results["knn_top1"] = evaluate_knn(train_feats, train_labels, val_feats, val_labels)
        results["linear_top1"] = evaluate_linear_probe(train_feats, train_labels, val_feats,
                                                       val_labels)
    seg_base = os.environ.get("DINOV3_EVAL_SEG", "")
    if seg_base:
        results.update(_seg_probe_results(cfg, backbone, seg_base, kwargs))
    logger.info("eval results: %s", results)
    return results


def _seg_probe_results(cfg, backbone, base: str, loader_kwargs) -> dict:
    """The dense half of do_test, behind DINOV3_EVAL_SEG=<dataset string base>
    (`SyntheticSeg`, or `ADE20K:root=...`): patch features at
    crops.global_crops_size, then the linear segmentation probe's lr grid."""
    from ..data import make_data_loader, make_dataset
    from ..data.transforms import make_segmentation_transforms
    from ..eval import evaluate_segmentation_linear, extract_dense_features

    name = base.split(":")[0]
    transform, target_transform = make_segmentation_transforms(
        crop_size=cfg.crops.global_crops_size, mean=cfg.crops.rgb_mean, std=cfg.crops.rgb_std,
        reduce_zero_label=name == "ADE20K")
    sizes = {"TRAIN": ":length=256", "VAL": ":length=64"} if name == "SyntheticSeg" else {}
    sets = []
    for split in ("TRAIN", "VAL"):
        dataset = make_dataset(dataset_str=f"{base}:split={split}{sizes.get(split, '')}",
                               transform=transform, target_transform=target_transform)
        sets.append(extract_dense_features(
            backbone, make_data_loader(dataset=dataset, **loader_kwargs), to_cpu=False))
    probe = evaluate_segmentation_linear(*sets[0], *sets[1], num_classes=dataset.NUM_CLASSES)
    best = probe["best_head"]
    results = {"seg_miou": probe["best_miou"], "seg_pixel_acc": probe["pixel_acc"][best],
               "seg_best_lr": probe["heads"][best][0]}
    results.update({f"seg_miou_head{i}": v for i, v in enumerate(probe["miou"])})
    return results


def main(argv=None):
    args = get_args_parser().parse_args(argv)
    setup_job(output_dir=args.output_dir or None, seed=args.seed)
    cfg = setup_config(args)
    if args.test_ibot:
        cfg.dino.loss_weight = 0.0
        cfg.dino.koleo_loss_weight = 0.0
        logger.info("--test-ibot: dino/koleo loss weights zeroed")
    if args.multi_distillation or cfg.multidistillation.enabled:
        cfg.multidistillation.enabled = True
        assert cfg.MODEL.META_ARCHITECTURE == "MultiDistillationMetaArch", \
            "multi-distillation runs need MODEL.META_ARCHITECTURE=MultiDistillationMetaArch"
    # meta-arch dispatch by config (reference train.py:293-299)
    from .multidist_meta_arch import MultiDistillationMetaArch

    meta_arch_cls = {
        "SSLMetaArch": SSLMetaArch,
        "MultiDistillationMetaArch": MultiDistillationMetaArch,
    }.get(cfg.MODEL.META_ARCHITECTURE)
    if meta_arch_cls is None:
        raise ValueError(f"unknown MODEL.META_ARCHITECTURE {cfg.MODEL.META_ARCHITECTURE}")
    if meta_arch_cls is MultiDistillationMetaArch:
        # each rank builds only its own student; collectives are scoped to
        # the student's subgroup inside the wrapper; the per-student merged
        # config drives the optimizer/schedules/data for this rank
        model = MultiDistillationMetaArch(cfg)
        rank_cfg = model.rank_config
        rank_cfg.train.output_dir = cfg.train.output_dir
        cfg = rank_cfg
    else:
        model = meta_arch_cls(cfg)
    if args.eval_only:
        # load weights for evaluation: latest checkpoint unless MODEL.WEIGHTS
        # names one explicitly (reference train.py:302-309)
        weights = cfg.MODEL.get("WEIGHTS", "")
        iteration = 0
        if weights:
            payload = load_checkpoint(weights, model, strict=False)
            iteration = payload.get("iteration", 0)
        elif not args.no_resume and args.output_dir:
            latest = find_latest_checkpoint(args.output_dir)
            if latest is not None:
                payload = load_checkpoint(latest, model, strict=False)
                iteration = payload.get("iteration", 0)
        return do_test(cfg, model, iteration)
    import os
    import time

    record_to = ""
    if args.record_ref_losses:
        record_to = os.path.join(args.output_dir or ".", "ref_losses.json")
    t0 = time.time()
    result = do_train(cfg, model, resume=not args.no_resume, max_iterations=args.max_iterations,
                      record_losses_to=record_to, compare_losses_to=args.ref_losses_path,
                      profiling=args.profiling)
    if args.benchmark_codebase:
        elapsed = time.time() - t0
        logger.info("benchmark: total wall %.1f s (use bench.py for the timed-step metric)", elapsed)
    return result


if __name__ == "__main__":
    main(sys.argv[1:])
