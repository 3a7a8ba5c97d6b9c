"""Per-rank training step and single-node data parallelism for the CALM-ViT path.

Replaces the Spark TorchDistributor launcher + DDP wrapper of
/root/reference/CALM-ViT/distributed_trainer_cls.py (train(): 25-114, __main__: 116-175) with
torch.distributed over RCCL (one process per GPU, env:// rendezvous from RANK/LOCAL_RANK/WORLD_SIZE
as set by torchrun):

  * `init_distributed()`               <- dist.init_process_group(...)                 (cls:46-51)
  * `sync_module_states(model)`        <- DDP ctor broadcast of params+buffers         (cls:55)
  * `BucketedGradReducer`              <- DDP's bucketed gradient all-reduce           (cls:55,87):
        gradients are packed into a few large flat buckets (sized for xGMI: point-to-point links,
        per-link-bound rings -> fewer, larger collectives) as soon as backward has produced them, and
        all-reduced (mean) on a SIDE HIP stream while the rest of backward keeps running.
  * `TrainStep`                        <- one iteration of the step loop               (cls:79-96):
        forward, CE with soft targets, backward, unscale / clip_grad_norm_(1.0), AdamW, zero_grad.
  * `AccumTrainStep` / `FusedClipAdamWindow` / `HeldGradReducer`   (no counterpart: the reference has no accumulation)
        gradient accumulation over k micro-batches per optimizer step: calm_grad_accum behind every micro-backward, one
        gradient exchange and one optimizer-side step per window.
  * `ModelEMA`                         (no counterpart: the reference keeps no weight average)
        exponential moving average of the parameters, one kernel pass behind the optimizer step; exchanged into the
        parameters in place for evaluation.
  * `EvalMetrics` / `validation_shard` / `evaluate(report=True)`   (the reference has the top-1 loop of CALM_ViT_V2.py:228-239 only)
        top-k, cross-entropy, per-class accuracy and confusion matrix of held-out data, tallied on the device
        (calm_eval_metrics) and summed over the ranks; `train(val_dataset=...)` runs it per epoch and keeps the best
        checkpoint.
  * `RegTrainStep` / `ReconMetrics` / `evaluate(recon=True)` / `train(task="reg")`   <- distributed_trainer_reg.py:25-112
        the generative job: Huber + kl_weight * kl on the image or on the device collate's row tokens, and Huber / MAE /
        MSE / PSNR / SSIM of held-out data tallied on the device (calm_recon_metrics); the best checkpoint follows the
        lowest validation Huber.
  * `SharpnessAware` / `SamTrainStep` / `SamRegTrainStep` / `train(sam=)`   (no counterpart: the reference has no SAM)
        sharpness-aware minimisation: calm_sam_perturb behind a first backward (in place, along the true gradient, the
        bits saved), a second pass at the perturbed weights whose gradients calm_grad_accum finishes there,
        calm_sam_restore, then the unchanged optimizer-side step.
  * `FusedClipAdamW(lamb=)` / `lamb_step_torch` / `train(lamb=)`   (no counterpart: the reference has no large-batch optimizer)
        LAMB inside the fused optimizer-side step (calm_optim_step_lamb): AdamW's moments, clip and inf check, every
        tensor's update rescaled by its trust ratio ||w|| / ||update||.
  * `train(drop_path=)`   (no counterpart: the reference has no stochastic depth)
        Vi_Tools_CNN_less_V2.set_drop_path on the model before the step is built: per-sample drops of both residual
        branches of every VMLA_Block (calm_drop_path), the per-block rates recorded in the snapshot header.
  * `soft_target_bce` / `TrainStep(loss=)` / `train(loss="bce")`   (no counterpart: the reference trains with softmax CE)
        binary cross-entropy with logits on the CutMix / MixUp soft targets, the loss of the DeiT III / timm recipe
        (calm_bce_fwd / _bwd with the loss kernels on; the StepMetrics buffer is fed as by the cross-entropy).

  * `MaskedImageModelling` / `RegTrainStep(mim=)` / `train(task="reg", mim=)` / `load_backbone`   (no counterpart)
        masked image modelling, the pre-training form of the generative job: a per-sample patch mask with exactly k set
        patches (calm_mim_draw), the masked tokens as the model's input (calm_mim_apply), the Huber loss over the masked
        elements alone against the clean tokens (calm_mim_huber_fwd / _bwd), and the hand-over of the pre-trained
        `autoencoder.*` tensors to a classifier.
  * `KnnProbe` / `knn_evaluate` / `Predictor(features=True)` / `train(knn=)`   (no counterpart)
        weighted k-NN probe of the frozen backbone features (Wu et al. 2018, DINO's eval_knn): L2-normalised rows
        (calm_knn_normalize), the exact k nearest bank features selected chunk by chunk under a total order (calm_gemm on
        the fp32 pipe + calm_knn_merge), temperature-weighted votes (calm_knn_vote) ranked by `EvalMetrics`; run behind the
        validation report of a pre-training run.

The model also works under stock `torch.nn.parallel.DistributedDataParallel` (that is what the
reference's train() does with it); the reducer here is the MI355X-tuned equivalent.  Under DDP the step
classes leave the gradient tail (ops.grad_tail) off: DDP reads gradients during the backward.
"""
import contextlib
import math
import os
import time
import weakref

import torch
import torch.distributed as dist


def init_distributed(use_gpu=True):
    """Returns (rank, local_rank, world_size).  No-op (0,0,1) when not launched by torchrun."""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return 0, 0, 1
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not dist.is_initialized():
        backend = os.environ.get("CALM_DIST_BACKEND", "nccl" if use_gpu else "gloo")
        if use_gpu and backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        elif use_gpu:
            # rehearsal mode: several ranks may share one GPU (CALM_LOCAL_DEVICE) and exchange through gloo
            torch.cuda.set_device(int(os.environ.get("CALM_LOCAL_DEVICE", local_rank)))
            dist.init_process_group(backend=backend)
        else:
            dist.init_process_group(backend="gloo")
    return rank, local_rank, world


def _flat_groups(tensors, max_bytes):
    groups, cur, size = [], [], 0
    for t in tensors:
        nb = t.numel() * t.element_size()
        if cur and size + nb > max_bytes:
            groups.append(cur)
            cur, size = [], 0
        cur.append(t)
        size += nb
    if cur:
        groups.append(cur)
    return groups


@torch.no_grad()
def sync_module_states(model, src=0, bucket_bytes=256 << 20):
    """Broadcast parameters and buffers from rank `src` (what DDP's constructor does)."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return
    tensors = [p.data for p in model.parameters()] + [b.data for b in model.buffers()]
    by_type = {}
    for t in tensors:
        by_type.setdefault((t.dtype, t.device), []).append(t)
    for group in by_type.values():
        for chunk in _flat_groups(group, bucket_bytes):
            flat = torch.cat([t.reshape(-1) for t in chunk])
            dist.broadcast(flat, src)
            off = 0
            for t in chunk:
                t.copy_(flat[off:off + t.numel()].view_as(t))
                off += t.numel()


def _bucket_groups(params, bucket_bytes, tail_bytes):
    """Parameters in gradient-arrival order -> buckets of ~bucket_bytes; the LAST bucket (the gradients that arrive
    when backward is about to end, whose all-reduce nothing is left to overlap with) holds at most ~tail_bytes."""
    sizes = [p.numel() * p.element_size() for p in params]
    tail, acc = len(params), 0
    while tail > 1 and acc + sizes[tail - 1] <= tail_bytes:
        tail -= 1
        acc += sizes[tail]
    if tail == len(params):                     # the last parameter alone exceeds tail_bytes
        tail = len(params) - 1
    groups = _flat_groups(params[:tail], bucket_bytes) if tail > 0 else []
    groups.append(params[tail:])
    return groups


class BucketedGradReducer:
    """Mean all-reduce of all gradients in large flat buckets, overlapped with backward.

    Parameters are bucketed in reverse registration order (~ the order backward produces their gradients): 64 MiB
    buckets — xGMI rings are per-link bound, so few large collectives — and a small last one, because the tail of
    backward has nothing left to hide a collective behind.  When the last gradient of a bucket has been accumulated,
    the bucket is packed and its all-reduce is launched on a side stream (RCCL over xGMI on the GPU: ReduceOp.AVG, the
    mean inside the collective; gloo on CPU in tests: SUM then a scale).  `finish()` (call after backward) makes the
    compute stream wait for the collectives and re-points every `p.grad` at its slice of the reduced bucket — no copy
    back: the optimizer-side step reads the buckets in place, and since those addresses never change its gradient
    pointer table is uploaded once.  (The gradients are PACKED into the bucket by one `_foreach_copy_` per bucket: the
    optimizer-side step releases `.grad`, so autograd's AccumulateGrad adopts the freshly produced gradient buffers —
    keeping `.grad` pointed at the bucket views across steps would instead make autograd add into them, one extra
    read-modify-write launch per parameter.)"""

    def __init__(self, model, bucket_mb=64, process_group=None, tail_mb=8, force=False):
        """force: run the buckets and collectives in a world of one as well (a single-GPU RCCL rehearsal of exactly the
        code path the 8-GPU job takes; needs an initialised process group)."""
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.enabled = self.world > 1 or (force and dist.is_initialized())
        self.buckets = []
        self._works = []
        if not self.enabled:
            return
        dev = self.params[0].device
        self.on_gpu = dev.type == "cuda"
        self.avg_in_collective = dist.get_backend(process_group) == "nccl"
        self.side = torch.cuda.Stream(device=dev) if self.on_gpu else None
        for group in _bucket_groups(list(reversed(self.params)), bucket_mb << 20, tail_mb << 20):
            n = sum(p.numel() for p in group)
            flat = torch.zeros(n, dtype=group[0].dtype, device=dev)
            views, off = [], 0
            for p in group:
                views.append(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
            self.buckets.append({"params": group, "flat": flat, "views": views, "pending": len(group)})
        from . import ops
        self._where = {}
        for bi, b in enumerate(self.buckets):
            for p in b["params"]:
                self._where[p] = bi
                handle = p.register_post_accumulate_grad_hook(self._hook)
                setattr(p, ops.TAIL_HOOK_ATTR, handle.id)  # _launch flushes the gradient tail before it reads a .grad

    def _hook(self, p):
        b = self.buckets[self._where[p]]
        b["pending"] -= 1
        if b["pending"] == 0:
            self._launch(b)

    def _launch(self, b, pack=True):
        """Launch the all-reduce of bucket `b`; pack=True first copies the `.grad`s into its views, pack=False reduces the
        flat bucket as it stands."""
        if pack:
            from . import ops
            ops.flush_grad_tail()       # gradients the backward deferred to its end are finished before they are packed
            grads = [p.grad for p in b["params"]]
        op = dist.ReduceOp.AVG if self.avg_in_collective else dist.ReduceOp.SUM
        if self.on_gpu:
            # the side stream starts after everything enqueued so far: the gradients exist, and the previous step's
            # optimizer-side kernels (which read this bucket in place) have been issued before them.  The collective is
            # issued SYNCHRONOUSLY (async_op=False) on the side stream: for ProcessGroupNCCL that blocks nobody — it
            # makes RCCL's stream wait for the side stream, enqueues the all-reduce there and makes the side stream wait
            # for its end event — and it is the form that a stream capture supports (fork from the capturing stream by
            # wait_stream, collectives on the fork with async_op=False, join by wait_stream: no Work object outlives
            # the call, nothing is waited on from a non-captured stream; round 3 used async_op=True + work.wait() in
            # finish() and ended in a segfault inside capture_end, gpurun_out/rccl.log)
            self.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.side):
                if pack:
                    torch._foreach_copy_(b["views"], grads)
                dist.all_reduce(b["flat"], op=op, group=self.pg, async_op=False)
                if not self.avg_in_collective:
                    b["flat"].mul_(1.0 / self.world)
            work = None
        else:
            if pack:
                torch._foreach_copy_(b["views"], grads)
            work = dist.all_reduce(b["flat"], op=op, group=self.pg, async_op=True)
        self._works.append((work, b))

    @torch.no_grad()
    def finish(self):
        if not self.enabled:
            return
        for b in self.buckets:                      # bucket not launched by the hooks: some of its
            if b["pending"] > 0:                    # parameters got no gradient this step
                for p in b["params"]:
                    if p.grad is None:
                        p.grad = torch.zeros_like(p)
                self._launch(b)
        self._join()

    def _join(self):
        """Behind the launches: every `p.grad` points at its slice of the reduced bucket and the compute stream waits for
        the collectives."""
        inv = 1.0 / self.world
        for work, b in self._works:
            if work is not None:                    # CPU (gloo) path: asynchronous collectives, waited for here
                work.wait()
                if not self.avg_in_collective:
                    b["flat"].mul_(inv)
            for p, v in zip(b["params"], b["views"]):
                p.grad = v                          # the reduced gradient, in place in its bucket
        if self.on_gpu:
            torch.cuda.current_stream().wait_stream(self.side)
        self._works.clear()
        for b in self.buckets:                      # (under `hold` the hooks never counted down: this changes nothing)
            b["pending"] = len(b["params"])


class HeldGradReducer(BucketedGradReducer):
    """BucketedGradReducer for gradient accumulation: while `hold` is set the per-parameter hooks do nothing, and the
    exchange runs once per window at its boundary.  With FusedClipAdamWindow the window's sums are accumulated IN the
    bucket views (`views_of`) and `reduce_held()` all-reduces the flat buckets as they stand; with a torch optimizer the
    boundary is the ordinary `finish()` — the hooks were held, every bucket still has `pending > 0`, so it packs the
    summed `.grad`s and launches.  One collective per bucket per window either way.  Stock DistributedDataParallel knows
    nothing of a window and all-reduces every micro-batch."""

    def __init__(self, model, bucket_mb=64, process_group=None, tail_mb=8, force=False, hold=True):
        super().__init__(model, bucket_mb=bucket_mb, process_group=process_group, tail_mb=tail_mb, force=force)
        self.hold = hold

    def _hook(self, p):
        if not self.hold:
            super()._hook(p)

    def views_of(self, params):
        """The bucket view of every one of `params`."""
        where = {p: v for b in self.buckets for p, v in zip(b["params"], b["views"])}
        return [where[p] for p in params]

    @torch.no_grad()
    def reduce_held(self):
        """All-reduce every flat bucket as it stands — no pack copy — and point every `p.grad` at its view, as `finish()`
        does.  The collectives start behind the window's last accumulate: overlapping them with the last micro-backward
        is out of scope."""
        if not self.enabled:
            return
        for b in self.buckets:
            self._launch(b, pack=False)
        self._join()


def soft_target_cross_entropy(logits, soft_targets, metrics=None):
    """torch.nn.CrossEntropyLoss() with class-probability targets (cls:63,86; CutMix/MixUp labels).

    With the loss kernels switched on (backend.set_loss_kernels / CALM_LOSS_KERNELS=1) a 2-D fp32 CUDA logits tensor with
    fp32 targets goes through calm_soft_ce_fwd / _bwd (ops.SoftTargetCrossEntropyFn); `metrics` (a StepMetrics) then
    receives the step's loss sum and dominant-class agreement on the device.  Everything else — the switch off, 1-D logits
    (squeeze() at batch 1), CPU tensors, other dtypes — is F.cross_entropy as before."""
    from . import backend
    if (backend.get_loss_kernels() and logits.dim() == 2 and soft_targets.dtype == torch.float32
            and soft_targets.shape == logits.shape and backend.loss_kernels_take(logits)):
        from .ops import SoftTargetCrossEntropyFn
        return SoftTargetCrossEntropyFn.apply(logits, soft_targets, None if metrics is None else metrics.buf)
    return torch.nn.functional.cross_entropy(logits, soft_targets)


def soft_target_bce(logits, soft_targets, metrics=None, target_threshold=None, sum_classes=False):
    """torch.nn.BCEWithLogitsLoss() on the CutMix / MixUp soft targets — the loss of the DeiT III recipe, timm's
    `BinaryCrossEntropy`: every class is its own two-way problem.  The mean over all B * C elements, or with sum_classes
    the sum over the classes and the mean over the batch; target_threshold (None: off) turns the targets into
    (soft_targets > target_threshold) first.

    Under the conditions of soft_target_cross_entropy — the loss kernels switched on, 2-D fp32 logits the installed backend
    can address, fp32 targets of their shape — and with a backend that has bce_fwd, it goes through calm_bce_fwd / _bwd
    (ops.BinaryCrossEntropyFn); `metrics` (a StepMetrics) then receives B * loss and the dominant-class agreement (against
    the targets as they came, not the thresholded ones) on the device.  Everything else — the switch off, 1-D logits
    (squeeze() at batch 1), CPU tensors, other dtypes — is F.binary_cross_entropy_with_logits."""
    from . import backend
    if (backend.get_loss_kernels() and logits.dim() == 2 and soft_targets.dtype == torch.float32
            and soft_targets.shape == logits.shape and backend.loss_kernels_take(logits)
            and hasattr(backend.get_backend(), "bce_fwd")):
        from .ops import BinaryCrossEntropyFn
        return BinaryCrossEntropyFn.apply(logits, soft_targets, None if metrics is None else metrics.buf,
                                          target_threshold, bool(sum_classes))
    if target_threshold is not None:
        soft_targets = (soft_targets > target_threshold).to(soft_targets.dtype)
    if sum_classes:
        rows = logits.shape[0] if logits.dim() > 1 else 1
        return torch.nn.functional.binary_cross_entropy_with_logits(logits, soft_targets, reduction="sum") / rows
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, soft_targets)


def _loss_settings(who, loss):
    """loss= of TrainStep / train() -> {"name": "ce"}, or {"name": "bce", "target_threshold": None | finite float,
    "sum_classes": bool}."""
    if loss is None or loss == "ce":
        return {"name": "ce"}
    if isinstance(loss, str):
        loss = {"name": loss}
    if not isinstance(loss, dict) or "name" not in loss:
        raise ValueError(f'{who}: loss is None, "ce", "bce" or a dict with "name" / "target_threshold" / "sum_classes", '
                         f"got {loss!r}")
    name = loss["name"]
    if name == "ce":
        if set(loss) != {"name"}:
            raise ValueError(f'{who}: loss "ce" takes no options, got {sorted(set(loss) - {"name"})}')
        return {"name": "ce"}
    if name != "bce":
        raise ValueError(f'{who}: loss["name"] is "ce" or "bce", got {name!r}')
    if not set(loss) <= {"name", "target_threshold", "sum_classes"}:
        raise ValueError(f'{who}: loss takes the keys "name", "target_threshold", "sum_classes", got {sorted(loss)}')
    thr, sum_classes = loss.get("target_threshold"), loss.get("sum_classes", False)
    if thr is not None and (isinstance(thr, bool) or not isinstance(thr, (int, float)) or not math.isfinite(thr)):
        raise ValueError(f'{who}: loss["target_threshold"] is None or a finite number, got {thr!r}')
    if not isinstance(sum_classes, bool):
        raise ValueError(f'{who}: loss["sum_classes"] is a bool, got {sum_classes!r}')
    return {"name": "bce", "target_threshold": None if thr is None else float(thr), "sum_classes": sum_classes}


def _cross_entropy_only(who, loss, why):
    """The refusal of the steps whose loss is built on the cross-entropy (or is not a classification loss at all)."""
    if _loss_settings(who, loss)["name"] != "ce":
        raise ValueError(f"{who}: loss={loss!r} is refused: {why}")


class StepMetrics:
    """The device float[4] that calm_soft_ce_fwd / calm_top1_count add to (include/calm_vit.h): loss sum, agreement
    count, rows, steps.  A training loop hands it to its steps and reads it once per epoch — one device-to-host copy
    instead of a `loss.item()` per step (cls:97)."""

    def __init__(self, device):
        self.buf = torch.zeros(4, dtype=torch.float32, device=device)

    def read(self):
        """(loss_sum, agree, rows, steps) as Python numbers: ONE device-to-host copy.  The counts are fp32 on the device,
        exact below 2^24; read and reset() before an accumulation period exceeds that."""
        loss_sum, agree, rows, steps = self.buf.to("cpu").tolist()
        return float(loss_sum), int(agree), int(rows), int(steps)

    def reset(self):
        self.buf.zero_()                    # in place: a captured step keeps adding at this address


def distill_loss_torch(logits, teacher_logits, soft_targets, alpha=0.5, temperature=1.0, mode="soft"):
    """The distillation loss in stock torch: Hinton-style soft distillation — (1 - alpha) * CE(z, y) + alpha * T^2 *
    KL(softmax(t / T) || softmax(z / T)), batch mean — or, in "hard" mode, DeiT-style hard distillation — (1 - alpha) *
    CE(z, y) + alpha * CE(z, argmax t).  No gradient reaches the teacher logits."""
    F = torch.nn.functional
    z, y, t, a, T = logits, soft_targets, teacher_logits.detach().to(logits.dtype), alpha, temperature
    if z.dim() == 1:                                    # (squeeze() at batch 1)
        z, y, t = z[None], y[None], t[None]
    if mode == "hard":
        return (1 - a) * F.cross_entropy(z, y) + a * F.cross_entropy(z, t.argmax(1))
    if mode != "soft":
        raise ValueError(f'distillation mode is "soft" or "hard", got {mode!r}')
    return (1 - a) * F.cross_entropy(z, y) + a * T ** 2 * F.kl_div(F.log_softmax(z / T, 1), F.softmax(t / T, 1),
                                                                   reduction="batchmean")


def distillation_loss(logits, teacher_logits, soft_targets, alpha=0.5, temperature=1.0, mode="soft", metrics=None,
                      distill_metrics=None):
    """The loss of a student trained against a frozen teacher's logits on the CutMix / MixUp labels `soft_targets`.

    Under the conditions of soft_target_cross_entropy — the loss kernels switched on, 2-D fp32 logits the installed backend
    can address, fp32 targets of their shape — and with a backend that has distill_fwd, the two terms are one kernel pass
    per direction (calm_distill_fwd / _bwd, ops.DistillLossFn; the teacher logits fp32 or bf16); `metrics` (a StepMetrics)
    and `distill_metrics` (a DistillMetrics) then accumulate on the device.  Everything else is distill_loss_torch."""
    from . import backend
    if (backend.get_loss_kernels() and logits.dim() == 2 and soft_targets.dtype == torch.float32
            and soft_targets.shape == logits.shape and teacher_logits.shape == logits.shape
            and teacher_logits.dtype in (torch.float32, torch.bfloat16) and teacher_logits.device == logits.device
            and backend.loss_kernels_take(logits) and hasattr(backend.get_backend(), "distill_fwd")):
        from .ops import DistillLossFn
        return DistillLossFn.apply(logits, teacher_logits, soft_targets, float(temperature), float(alpha), mode,
                                   None if metrics is None else metrics.buf,
                                   None if distill_metrics is None else distill_metrics.buf)
    return distill_loss_torch(logits, teacher_logits, soft_targets, alpha, temperature, mode)


class DistillMetrics:
    """The device float[4] that calm_distill_fwd adds to (include/calm_vit.h): sum of the rows' cross-entropy, sum of the
    rows' distillation term (unweighted), rows whose argmax equals the teacher's, rows.  Read once per epoch."""

    def __init__(self, device):
        self.buf = torch.zeros(4, dtype=torch.float32, device=device)

    def read(self):
        """(ce_sum, d_sum, agree, rows) as Python numbers: ONE device-to-host copy.  The counts are fp32 on the device,
        exact below 2^24."""
        ce_sum, d_sum, agree, rows = self.buf.to("cpu").tolist()
        return float(ce_sum), float(d_sum), int(agree), int(rows)

    def reset(self):
        self.buf.zero_()


def eval_metrics_torch(logits, labels, ks, counts, loss_sum, confusion):
    """What calm_eval_metrics adds to its accumulators (include/calm_vit.h), in torch on the tensors' device: class c BEATS
    label l when z_c > z_l, or z_c == z_l and c < l, and the label is in the top k exactly when fewer than k classes beat
    it; a row whose label is outside [0, C) is skipped (counted in `skipped` alone); a row holding a NaN is counted in
    rows, nonfinite and its class's support, is never a hit and adds to neither the loss nor the confusion matrix.  The
    integers equal the kernel's; the loss is the same fp32 formula summed in torch's order."""
    z = logits.float()
    B, C = z.shape
    labels = labels.to(z.device, torch.int64)
    valid = (labels >= 0) & (labels < C)
    l = labels.clamp(0, C - 1)
    zl = z.gather(1, l[:, None])
    cls = torch.arange(C, device=z.device)[None, :]
    beaten = ((z > zl) | ((z == zl) & (cls < l[:, None]))).sum(dim=1)
    nan = torch.isnan(z).any(dim=1)
    finite = valid & ~nan
    zf = torch.where(finite[:, None], z, torch.zeros_like(z))      # (argmax / max of a NaN row are not used)
    m, pred = zf.max(dim=1)                                         # first maximal value: the lowest index wins
    nll = (m - zl[:, 0]) + torch.log(torch.exp(zf - m[:, None]).sum(dim=1))
    head = [valid.sum(), (~valid).sum(), (valid & nan).sum()] + [(finite & (beaten < int(k))).sum() for k in ks]
    counts[:len(head)] += torch.stack(head).to(counts.dtype)
    counts[7:7 + C] += torch.bincount(l[valid], minlength=C)
    counts[7 + C:7 + 2 * C] += torch.bincount(l[finite & (pred == l)], minlength=C)
    loss_sum += torch.where(finite, nll, torch.zeros_like(nll)).sum().double()
    if confusion is not None:
        confusion.view(-1).add_(torch.bincount(l[finite] * C + pred[finite], minlength=C * C))


class EvalMetrics:
    """Validation tallies on the device: rows, top-k hits, the cross-entropy sum, per-class support and top-1 hits and,
    with confusion=True, the [label, prediction] confusion matrix — `counts` (int64 [7 + 2C]: rows, skipped, nonfinite,
    hits@topk[0..3], support[C], hits1[C]), `loss_sum` (float64 [1]) and `confusion` (int64 [C,C] or None), the
    accumulators of calm_eval_metrics (include/calm_vit.h).

    update(logits, labels) adds one batch.  With the loss kernels switched on (backend.set_loss_kernels) and fp32 or bf16
    CUDA logits it is ONE library call — two launches, no host synchronisation, and after the first call at the largest
    batch size no allocation, so it can be captured into a graph; otherwise `eval_metrics_torch`, the same definitions in
    torch, with the same integers.  all_reduce() sums the accumulators over a process group, read() is one device-to-host
    copy, reset() zeroes in place."""

    def __init__(self, num_classes, topk=(1, 5), confusion=False, device="cpu"):
        topk = tuple(topk)
        if not 1 <= len(topk) <= 4 or any(int(k) != k or k < 1 for k in topk) or len(set(topk)) != len(topk):
            raise ValueError(f"EvalMetrics: topk takes one to four distinct integers >= 1, got {topk!r}")
        if int(num_classes) != num_classes or not 1 <= num_classes <= 65536:
            raise ValueError(f"EvalMetrics: num_classes within 1 .. 65536 expected, got {num_classes!r}")
        self.num_classes, self.topk = int(num_classes), tuple(int(k) for k in topk)
        C = self.num_classes
        self.counts = torch.zeros(7 + 2 * C, dtype=torch.int64, device=device)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=device)
        self.confusion = torch.zeros(C, C, dtype=torch.int64, device=device) if confusion else None
        self._records = None                 # the kernel's per-row records: grown to the largest batch seen

    def tensors(self):
        return [t for t in (self.counts, self.loss_sum, self.confusion) if t is not None]

    def update(self, logits, labels):
        from . import backend
        if logits.dim() != 2 or logits.shape[1] != self.num_classes or labels.shape != logits.shape[:1]:
            raise ValueError(f"EvalMetrics.update: logits [B, {self.num_classes}] and labels [B] expected, got "
                             f"{tuple(logits.shape)} and {tuple(labels.shape)}")
        if backend.eval_kernels_take(logits):
            B, C = logits.shape
            logits = logits if logits.stride(1) == 1 else logits.contiguous()
            labels = labels.to(logits.device, torch.int64).contiguous()
            if self._records is None or self._records.numel() < 4 * B:
                self._records = torch.empty(4 * B, dtype=torch.float32, device=logits.device)
            backend.get_backend().eval_metrics(logits, labels, self.topk, self.counts, self.loss_sum, self.confusion, B, C,
                                               self._records)
        else:
            eval_metrics_torch(logits, labels, self.topk, self.counts, self.loss_sum, self.confusion)

    def all_reduce(self, group=None):
        for t in self.tensors():
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

    def reset(self):
        for t in self.tensors():
            t.zero_()                       # in place: a captured update keeps adding at these addresses

    def read(self):
        """The report as a plain dict, from ONE device-to-host copy: n (rows counted), skipped, nonfinite, loss (mean over
        the finite rows), top<k> for every k (hits / n), per_class_accuracy (float64 [C]; NaN where a class has no
        support), mean_per_class_accuracy (over the classes that have support) and confusion (int64 [C,C]) if kept."""
        C = self.num_classes
        flat = torch.cat([self.counts, self.loss_sum.view(torch.int64)]
                         + ([self.confusion.reshape(-1)] if self.confusion is not None else [])).to("cpu")
        n, skipped, nonfinite = (int(v) for v in flat[:3])
        rep = {"n": n, "skipped": skipped, "nonfinite": nonfinite,
               "loss": float(flat[7 + 2 * C:8 + 2 * C].view(torch.float64)) / max(n - nonfinite, 1)}
        for i, k in enumerate(self.topk):
            rep[f"top{k}"] = int(flat[3 + i]) / max(n, 1)
        support, hits1 = flat[7:7 + C].double(), flat[7 + C:7 + 2 * C].double()
        acc = torch.where(support > 0, hits1 / support.clamp(min=1), torch.full_like(support, float("nan")))
        rep["per_class_accuracy"] = acc
        rep["mean_per_class_accuracy"] = float(acc[support > 0].mean()) if bool((support > 0).any()) else 0.0
        if self.confusion is not None:
            rep["confusion"] = flat[8 + 2 * C:].reshape(C, C).clone()
        return rep


RECON_WINDOW, RECON_SIGMA, RECON_C1, RECON_C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2      # SSIM (Wang et al. 2004)


def recon_metrics_torch(tokens, target, mean, std, delta, ssim, sums):
    """What calm_recon_metrics adds to `sums` (float64 [8], include/calm_vit.h), as a plain fp32 torch composition on the
    tensors' device: tokens [B,S,3S] are the channels-last generated image; target is rows [B,S,3S] or the image
    [B,3,S,S].  An image holding a non-finite generated value adds to [0] and [1] only.  Huber / abs / square sums in
    normalised space; pixel space is clamp(v * std_c + mean_c, 0, 1); PSNR_b = 10 log10(1 / max(mse_b, 1e-10)); SSIM_b is
    the mean over the (S - 10)^2 valid positions and the channels of the 11 x 11 Gaussian (sigma 1.5) window form with
    population moments (conv2d per channel).  ssim=False leaves [7] alone."""
    g = tokens.float()
    B, S = g.shape[0], g.shape[1]
    gi = g.reshape(B, S, S, 3).permute(0, 3, 1, 2)
    t = target.to(g.device).float()
    ti = t if t.dim() == 4 else t.reshape(B, S, S, 3).permute(0, 3, 1, 2)
    finite = torch.isfinite(gi).reshape(B, -1).all(dim=1)
    d = gi - ti
    ad = d.abs()
    hub = torch.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta))
    m = torch.tensor(mean, dtype=torch.float32, device=g.device).view(1, 3, 1, 1)
    sd = torch.tensor(std, dtype=torch.float32, device=g.device).view(1, 3, 1, 1)
    px, py = (gi * sd + m).clamp(0.0, 1.0), (ti * sd + m).clamp(0.0, 1.0)
    mse = ((px - py) ** 2).reshape(B, -1).mean(dim=1)
    psnr = 10.0 * torch.log10(1.0 / mse.clamp(min=1e-10))
    zero = torch.zeros(B, dtype=torch.float32, device=g.device)
    kept = lambda v: torch.where(finite, v, zero).sum().double()        # noqa: E731
    vals = [torch.tensor(float(B), dtype=torch.float64, device=g.device), (~finite).sum().double(),
            kept(hub.reshape(B, -1).sum(dim=1)), kept(ad.reshape(B, -1).sum(dim=1)), kept((d * d).reshape(B, -1).sum(dim=1)),
            finite.sum().double() * (3 * S * S), kept(psnr)]
    if ssim:
        k = torch.arange(RECON_WINDOW, dtype=torch.float32, device=g.device) - (RECON_WINDOW - 1) / 2
        w1 = torch.exp(-k * k / (2.0 * RECON_SIGMA ** 2))
        w1 = w1 / w1.sum()
        win = (w1[:, None] * w1[None, :]).expand(3, 1, RECON_WINDOW, RECON_WINDOW).contiguous()
        filt = lambda v: torch.nn.functional.conv2d(v, win, groups=3)       # noqa: E731
        ux, uy = filt(px), filt(py)
        sxx, syy, sxy = filt(px * px) - ux * ux, filt(py * py) - uy * uy, filt(px * py) - ux * uy
        smap = ((2 * ux * uy + RECON_C1) * (2 * sxy + RECON_C2)) / ((ux * ux + uy * uy + RECON_C1) * (sxx + syy + RECON_C2))
        vals.append(kept(smap.reshape(B, -1).mean(dim=1)))
    sums[:len(vals)] += torch.stack(vals)


class ReconMetrics:
    """Reconstruction tallies of a generative model on the device, the counterpart of EvalMetrics: `sums` (float64 [8]) is
    the accumulator of calm_recon_metrics (include/calm_vit.h) — images, non-finite images, Huber / abs / square sums in
    normalised space, elements, and the per-image PSNR and SSIM sums in pixel space (clamp(v * std_c + mean_c, 0, 1)).

    update(tokens, target) adds one batch: tokens [B,S,3S] as the model returns them (fp32 or bf16), target the fp32 input,
    rows [B,S,3S] or image [B,3,S,S].  With the loss kernels switched on and tensors the backend serves it is ONE library
    call — two launches, no host synchronisation, no allocation after the first call at the largest batch, so it can be
    captured into a graph; otherwise `recon_metrics_torch`, the same definitions in fp32 torch.  all_reduce() sums over a
    process group, read() is one device-to-host copy, reset() zeroes in place.  ssim=False skips the windowed pass (and
    serves images with S < 11)."""

    def __init__(self, mean, std, delta=1.0, ssim=True, device="cpu"):
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(mean) != 3 or len(std) != 3 or not float(delta) > 0.0:
            raise ValueError("ReconMetrics: mean and std hold three values each and delta is positive")
        self.mean, self.std, self.delta, self.ssim = mean, std, float(delta), bool(ssim)
        self.sums = torch.zeros(8, dtype=torch.float64, device=device)
        self._records = None                 # the kernel's per-workgroup records: grown to the largest batch seen

    def tensors(self):
        return [self.sums]

    def update(self, tokens, target):
        from . import backend, _lib
        if tokens.dim() != 3 or tokens.shape[2] != 3 * tokens.shape[1]:
            raise ValueError(f"ReconMetrics.update: tokens [B,S,3S] expected, got {tuple(tokens.shape)}")
        B, S = tokens.shape[0], tokens.shape[1]
        if tuple(target.shape) not in ((B, S, 3 * S), (B, 3, S, S)):
            raise ValueError(f"ReconMetrics.update: a target [B,S,3S] or [B,3,S,S] of the tokens' batch expected, got "
                             f"{tuple(target.shape)}")
        if self.ssim and S < RECON_WINDOW:
            raise ValueError(f"ReconMetrics.update: SSIM needs S >= {RECON_WINDOW}, got {S} (build with ssim=False)")
        if backend.recon_kernels_take(tokens, target) and S <= 4096:
            be = backend.get_backend()
            need = be.recon_scratch_floats(B, S)
            if self._records is None or self._records.numel() < need:
                self._records = torch.empty(need, dtype=torch.float32, device=tokens.device)
            be.recon_metrics(tokens.contiguous(), target.contiguous(), _lib.RECON_NCHW if target.dim() == 4 else
                             _lib.RECON_ROWS, self.mean, self.std, self.delta, self.ssim, self.sums, B, S, self._records)
        else:
            recon_metrics_torch(tokens, target, self.mean, self.std, self.delta, self.ssim, self.sums)

    def all_reduce(self, group=None):
        dist.all_reduce(self.sums, op=dist.ReduceOp.SUM, group=group)

    def reset(self):
        self.sums.zero_()                   # in place: a captured update keeps adding at this address

    def read(self):
        """{n, nonfinite, huber, mae, mse, psnr, ssim} from ONE device-to-host copy: huber / mae / mse are means over the
        elements of the finite images, psnr / ssim means over the finite images; ssim is None when built with ssim=False."""
        v = self.sums.to("cpu").tolist()
        n, bad = int(v[0]), int(v[1])
        elems, imgs = max(v[5], 1.0), max(n - bad, 1)
        return {"n": n, "nonfinite": bad, "huber": v[2] / elems, "mae": v[3] / elems, "mse": v[4] / elems,
                "psnr": v[6] / imgs, "ssim": v[7] / imgs if self.ssim else None}


KNN_MAX_K = 256                                     # calm_knn_merge / calm_knn_vote (include/calm_vit.h)
_KNN_LAST = torch.iinfo(torch.int64).max            # where an empty slot sorts by index: behind every bank item


def knn_normalize_torch(x):
    """What calm_knn_normalize computes, in torch: (x / ||x|| as fp32 [N, D], the number of zeroed rows as an int64
    0-dim tensor).  A row with a non-finite element, or whose fp32 norm is 0 or not finite, becomes all +0.0."""
    xf = x.float()
    nrm = (xf * xf).sum(dim=1).sqrt()
    ok = torch.isfinite(xf).all(dim=1) & (nrm > 0) & torch.isfinite(nrm)
    safe = torch.where(ok, nrm, torch.ones_like(nrm))
    out = torch.where(ok[:, None], xf / safe[:, None], torch.zeros_like(xf))
    return out, (~ok).sum()


def knn_merge_torch(sims, base, best_sim, best_idx):
    """What calm_knn_merge does to the running state (best_sim fp32 [Nq, k], best_idx int64 [Nq, k], rewritten in place)
    with the chunk sims [Nq, n] of bank items base .. base + n - 1: the best k of state and chunk under similarity
    descending, then bank index ascending — two stable sorts.  A NaN is -inf; -0.0 equals +0.0 and keeps its bits; an
    empty slot (-inf, -1) sorts behind a real -inf."""
    Nq, n = sims.shape
    k = best_sim.shape[1]
    s = sims.float()
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    idx = (int(base) + torch.arange(n, dtype=torch.int64, device=s.device)).expand(Nq, n)
    S, I = torch.cat([best_sim, s], dim=1), torch.cat([best_idx, idx], dim=1)
    by_idx = torch.where(I < 0, torch.full_like(I, _KNN_LAST), I).sort(dim=1, stable=True).indices
    S, I = S.gather(1, by_idx), I.gather(1, by_idx)
    by_sim = S.sort(dim=1, descending=True, stable=True).indices[:, :k]
    S, I = S.gather(1, by_sim), I.gather(1, by_sim)
    best_sim.copy_(torch.where(I < 0, torch.full_like(S, float("-inf")), S))
    best_idx.copy_(torch.where(I < 0, torch.full_like(I, -1), I))


def knn_vote_torch(best_sim, best_idx, bank_labels, inv_T, num_classes):
    """What calm_knn_vote writes, in torch: scores fp32 [Nq, C], the neighbours' weights exp((sim - the row's largest sim)
    * inv_T) added to their labels' classes slot by slot in ascending order (one fp32 addition per slot, so classes with
    equal votes get equal bits).  Empty slots, indices outside the bank and labels outside [0, C) vote for nothing."""
    Nq, k = best_sim.shape
    C, Nb = int(num_classes), bank_labels.numel()
    scores = torch.zeros(Nq, C, dtype=torch.float32, device=best_sim.device)
    rows = torch.arange(Nq, device=best_sim.device)
    s0 = best_sim[:, 0]
    for j in range(k):
        id_j, s_j = best_idx[:, j], best_sim[:, j]
        inside = (id_j >= 0) & (id_j < Nb)
        lab = bank_labels[id_j.clamp(0, max(Nb - 1, 0))] if Nb else torch.full_like(id_j, -1)
        votes = inside & (lab >= 0) & (lab < C)
        d = torch.where(s_j == s0, torch.zeros_like(s_j), s_j - s0)
        w = torch.exp(d * torch.tensor(float(inv_T), dtype=torch.float32, device=d.device))
        scores[rows[votes], lab[votes]] += w[votes]
    return scores


class KnnProbe:
    """Weighted k-NN probe on frozen features (Wu et al. 2018, DINO's eval_knn): the bank and the queries are L2-normalised,
    every query takes its k nearest bank features by cosine similarity, each neighbour votes for its label with weight
    exp(sim / T), and the votes are ranked by an internal `EvalMetrics`.  No training, deterministic.

    The neighbours are EXACT under a total order — similarity descending, then bank index ascending — selected chunk by
    chunk (`chunk` bank rows at a time: the [Nq, Nb] similarity matrix never exists), so ties are decided and the result
    does not depend on the chunking.  On CUDA fp32 / bf16 features the work is calm_knn_normalize, calm_gemm on the fp32
    pipe, calm_knn_merge and calm_knn_vote (include/calm_vit.h) with no host synchronisation until read(); otherwise the
    torch twins above.

    reset(); add_bank(features [N, D], labels int64 [N]) per bank batch; gather_bank() once when the bank is spread over
    ranks; query(features, labels) per query batch (neighbours(features) -> (sims, idx) [Nq, k] is the retrieval alone);
    all_reduce(); read().  A bank smaller than k is allowed: the empty slots (-inf, -1) do not vote."""

    def __init__(self, num_classes, k=20, temperature=0.07, topk=(1, 5), chunk=16384, confusion=False, device="cpu"):
        if isinstance(k, bool) or int(k) != k or not 1 <= k <= KNN_MAX_K:
            raise ValueError(f"KnnProbe: k is an integer within 1 .. {KNN_MAX_K}, got {k!r}")
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0.0 < temperature < float("inf"):
            raise ValueError(f"KnnProbe: temperature is a positive finite number, got {temperature!r}")
        if isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1:
            raise ValueError(f"KnnProbe: chunk counts bank rows per merge (>= 1), got {chunk!r}")
        self.metrics = EvalMetrics(num_classes, topk=topk, confusion=confusion, device=device)
        self.num_classes, self.topk = self.metrics.num_classes, self.metrics.topk
        self.k, self.temperature, self.chunk = int(k), float(temperature), int(chunk)
        self.device = torch.device(device)
        self.zeroed = torch.zeros(2, dtype=torch.int64, device=device)         # bank rows, query rows
        self.reset()

    def reset(self):
        self.metrics.reset()
        self.zeroed.zero_()
        self.width = None
        self._parts, self._bank, self._labels = [], None, None

    # ---- the three steps, on the kernels or on the twins -----------------------------------------------------------------
    @staticmethod
    def _kernels(t):
        from . import backend
        return backend.knn_kernels_take(t)

    def _check(self, who, features, labels):
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or not features.is_floating_point():
            raise TypeError(f"KnnProbe.{who}: features is a floating-point tensor [N, D]")
        if self.width is not None and features.shape[1] != self.width:
            raise ValueError(f"KnnProbe.{who}: features are {features.shape[1]} wide, the probe has seen {self.width}")
        if features.shape[1] < 1:
            raise ValueError(f"KnnProbe.{who}: features need at least one column")
        if labels is not None and (not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64
                                   or tuple(labels.shape) != (features.shape[0],)):
            raise TypeError(f"KnnProbe.{who}: labels is an int64 tensor [N] = [{features.shape[0]}]")
        self.width = features.shape[1]

    def _normalize(self, features, slot):
        from . import backend
        f = features.detach().to(self.device)
        N, D = f.shape
        if self._kernels(f):
            f = f if f.stride(1) == 1 else f.contiguous()
            out = torch.empty(N, D, dtype=torch.float32, device=f.device)
            backend.get_backend().knn_normalize(f, out, self.zeroed[slot:slot + 1], N, D)
            return out
        out, bad = knn_normalize_torch(f)
        self.zeroed[slot] += bad
        return out

    # ---- the bank -------------------------------------------------------------------------------------------------------
    def add_bank(self, features, labels):
        """Normalise and append: features [N, D], labels int64 [N]; zeroed rows (non-finite, or norm 0) are counted."""
        self._check("add_bank", features, labels)
        self._parts.append((self._normalize(features, 0), labels.detach().to(self.device)))
        self._bank = None

    def bank(self):
        """(features fp32 [Nb, D] normalised, labels int64 [Nb]) as added, or as gather_bank left them."""
        if self._bank is None:
            if not self._parts:
                return None, None
            self._bank = torch.cat([f for f, _ in self._parts]).contiguous()
            self._labels = torch.cat([l for _, l in self._parts]).contiguous()
            self._parts = [(self._bank, self._labels)]
        return self._bank, self._labels

    def gather_bank(self, process_group=None, world_layout="strided"):
        """All-gather every rank's shard and lay the bank out in DATASET order on every rank: rank r's j-th row is item
        r + j * world (world_layout="strided", the layout of `validation_shard`), or the shards one behind the other
        ("concat").  Shards are padded to the longest for the exchange, then trimmed.  Bank indices, and so ties, then do
        not depend on the world size.  Without an initialised process group the bank stays as it is."""
        if world_layout not in ("strided", "concat"):
            raise ValueError(f'KnnProbe.gather_bank: world_layout is "strided" or "concat", got {world_layout!r}')
        if process_group is None and not (dist.is_available() and dist.is_initialized()):
            return
        world, rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        feats, labels = self.bank()
        if feats is None:
            raise ValueError("KnnProbe.gather_bank: every rank adds its shard with add_bank first")
        sizes = torch.zeros(world, dtype=torch.int64, device=self.device)
        sizes[rank] = feats.shape[0]
        dist.all_reduce(sizes, group=process_group)
        sizes = [int(v) for v in sizes.cpu()]
        longest, total, D = max(sizes), sum(sizes), feats.shape[1]
        if world_layout == "strided" and sizes != [len(range(r, total, world)) for r in range(world)]:
            raise ValueError(f"KnnProbe.gather_bank: shards of {sizes} rows are not the strided shards of {total} items")
        pad_f = torch.zeros(longest, D, dtype=torch.float32, device=self.device)
        pad_l = torch.zeros(longest, dtype=torch.int64, device=self.device)
        pad_f[:feats.shape[0]], pad_l[:feats.shape[0]] = feats, labels
        all_f = [torch.empty_like(pad_f) for _ in range(world)]
        all_l = [torch.empty_like(pad_l) for _ in range(world)]
        dist.all_gather(all_f, pad_f, group=process_group)
        dist.all_gather(all_l, pad_l, group=process_group)
        bank = torch.empty(total, D, dtype=torch.float32, device=self.device)
        bank_l = torch.empty(total, dtype=torch.int64, device=self.device)
        at = 0
        for r, n in enumerate(sizes):
            if world_layout == "strided":
                bank[r::world], bank_l[r::world] = all_f[r][:n], all_l[r][:n]
            else:
                bank[at:at + n], bank_l[at:at + n] = all_f[r][:n], all_l[r][:n]
                at += n
        self._bank, self._labels = bank, bank_l
        self._parts = [(bank, bank_l)]
        dist.all_reduce(self.zeroed[0:1], group=process_group)

    # ---- the queries ----------------------------------------------------------------------------------------------------
    def _neighbours(self, q):
        from . import backend
        bank, _ = self.bank()
        if bank is None or bank.shape[0] == 0:
            raise ValueError("KnnProbe: the bank is empty (add_bank first)")
        Nq, D = q.shape
        Nb, k = bank.shape[0], self.k
        best_sim = torch.full((Nq, k), float("-inf"), dtype=torch.float32, device=q.device)
        best_idx = torch.full((Nq, k), -1, dtype=torch.int64, device=q.device)
        if Nq == 0:
            return best_sim, best_idx
        kernels = self._kernels(q)
        scratch = torch.empty(Nq, min(self.chunk, Nb), dtype=torch.float32, device=q.device) if kernels else None
        for base in range(0, Nb, self.chunk):
            rows = bank[base:base + self.chunk]
            n = rows.shape[0]
            if kernels:
                be = backend.get_backend()
                with backend.fp32_matmul():                     # queries [Nq, D] x rows [n, D]^T, both k-contiguous
                    be.gemm(q, rows, scratch, Nq, n, D, (D, 1, 0, 0), (D, 1, 0, 0), (scratch.stride(0), 0, 0))
                be.knn_merge(scratch[:, :n], base, best_sim, best_idx, Nq, n, k)
            else:
                knn_merge_torch(q @ rows.t(), base, best_sim, best_idx)
        return best_sim, best_idx

    def neighbours(self, features):
        """(sims fp32 [Nq, k], idx int64 [Nq, k]): the k nearest bank items of every row by cosine similarity, sorted by
        similarity descending, then bank index ascending; (-inf, -1) where the bank has fewer than k items."""
        self._check("neighbours", features, None)
        return self._neighbours(self._normalize(features, 1))

    def query(self, features, labels):
        """neighbours, the vote, and one `EvalMetrics.update(scores, labels)`; returns the scores fp32 [Nq, C]."""
        from . import backend
        self._check("query", features, labels)
        best_sim, best_idx = self._neighbours(self._normalize(features, 1))
        _, bank_labels = self.bank()
        Nq, C = best_sim.shape[0], self.num_classes
        if self._kernels(best_sim) and Nq > 0:
            scores = torch.empty(Nq, C, dtype=torch.float32, device=best_sim.device)
            backend.get_backend().knn_vote(best_sim, best_idx, bank_labels, 1.0 / self.temperature, scores, Nq, self.k, C)
        else:
            scores = knn_vote_torch(best_sim, best_idx, bank_labels, 1.0 / self.temperature, C)
        self.metrics.update(scores, labels.to(scores.device))
        return scores

    def all_reduce(self, group=None):
        """Sum the tallies over the ranks (the bank's zeroed rows were summed by gather_bank)."""
        self.metrics.all_reduce(group)
        dist.all_reduce(self.zeroed[1:2], op=dist.ReduceOp.SUM, group=group)

    def read(self):
        """The report: n, skipped, bank, bank_zeroed, query_zeroed, k, temperature, top<k>, per_class_accuracy,
        mean_per_class_accuracy and, if kept, confusion — `EvalMetrics.read()` of the votes without its loss (a
        cross-entropy of vote sums means nothing)."""
        rep = self.metrics.read()
        bank, _ = self.bank()
        zeroed = [int(v) for v in self.zeroed.cpu()]
        out = {"n": rep["n"], "skipped": rep["skipped"], "bank": 0 if bank is None else int(bank.shape[0]),
               "bank_zeroed": zeroed[0], "query_zeroed": zeroed[1], "k": self.k, "temperature": self.temperature}
        out.update({key: v for key, v in rep.items() if key not in ("n", "skipped", "nonfinite", "loss")})
        return out


def mim_huber_torch(tokens, target, mask, patch, delta=1.0, masked=None):
    """calm_mim_huber_fwd as a plain torch expression (autograd gives calm_mim_huber_bwd): Huber(delta) between two
    [B,S,3S] tensors, mean over the 3 * patch^2 * masked elements of the masked patches; mask uint8 / bool [B, (S / patch)^2],
    masked: the number of set entries (None: counted here).  The difference is SELECTED before anything is computed on
    it, so unmasked positions contribute exact zeros to the loss and to the gradient, whatever they hold."""
    B, S, _ = target.shape
    G = S // patch
    m = (mask.reshape(B, G, 1, G, 1) != 0).expand(B, G, patch, G, 3 * patch).reshape(B, S, 3 * S)
    d = torch.where(m, tokens.reshape(B, S, 3 * S).float() - target.float(), torch.zeros((), device=target.device))
    n = 3 * patch * patch * (mask.sum() if masked is None else masked)
    return torch.nn.functional.huber_loss(d, torch.zeros_like(d), reduction="sum", delta=delta) / n


class MaskedImageModelling:
    """Masked image modelling for the generative job (SimMIM, Xie et al. 2022; MAE, He et al. 2022): per sample exactly k of
    the P = (S / patch)^2 patches are replaced by `fill` in the model's input, and the loss is the Huber loss between the
    model's tokens and the CLEAN tokens over the masked patches alone — the U-shaped encoder-decoder cannot pass those
    through its skips.

        k = min(P - 1, max(1, floor(ratio * P + 0.5)))          0 < ratio < 1

    patch: the patch side in pixels (S % patch == 0, S / patch <= 32).  fill: a float or three floats (per channel) in
    normalised space; 0 is the dataset mean.  `draw(B, S, device)` -> uint8 mask [B, P] (calm_mim_draw; the 16-byte key comes
    from ops.draw_dropout_key: torch.manual_seed reproduces it, ops.set_dropout_key_override injects it, it is drawn on the
    device); `apply(tokens, mask)` -> the masked copy of row tokens [B,S,3S] (calm_mim_apply); `loss(y_hat, target, mask)`
    -> the scalar (ops.MimHuberFn when the loss kernels take the tensors, `mim_huber_torch` otherwise).  draw and apply
    always go through the backend: there is no torch twin of the mask."""
    delta = 1.0                                   # nn.HuberLoss() of the reference's generative trainer (reg:59)

    def __init__(self, patch=32, ratio=0.6, fill=0.0):
        if isinstance(patch, bool) or not isinstance(patch, int) or patch < 1:
            raise ValueError(f"MaskedImageModelling: patch is a side in pixels (an int >= 1), got {patch!r}")
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < ratio < 1.0:
            raise ValueError(f"MaskedImageModelling: ratio is a share of the patches in (0, 1), got {ratio!r}")
        f3 = list(fill) if isinstance(fill, (tuple, list)) else [fill] * 3
        if len(f3) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in f3):
            raise ValueError(f"MaskedImageModelling: fill is a finite float or three of them, got {fill!r}")
        self.patch, self.ratio, self.fill = patch, float(ratio), [float(v) for v in f3]

    def grid(self, S):
        """(G, P, k) at image side S."""
        G = S // self.patch
        if S % self.patch or G < 1:
            raise ValueError(f"MaskedImageModelling: the image side {S} is not a multiple of the patch side {self.patch}")
        if G > 32:
            raise ValueError(f"MaskedImageModelling: the image side {S} holds {G} patches of side {self.patch} per row, "
                             "more than the 32 the mask kernel ranks")
        P = G * G
        return G, P, min(P - 1, max(1, math.floor(self.ratio * P + 0.5)))

    def draw(self, B, S, device):
        from . import backend, ops
        G, P, k = self.grid(S)
        mask = torch.empty(B, P, dtype=torch.uint8, device=device)
        backend.get_backend().mim_draw(mask, B, G, k, ops.draw_dropout_key(device))
        return mask

    def apply(self, tokens, mask):
        from . import backend
        B, S, _ = tokens.shape
        self.grid(S)
        tokens = tokens if tokens.is_contiguous() else tokens.contiguous()
        out = torch.empty_like(tokens)
        backend.get_backend().mim_apply(tokens, out, mask, self.fill, B, S, self.patch)
        return out

    def loss(self, y_hat, target, mask):
        from . import backend
        B, S, _ = target.shape
        masked = B * self.grid(S)[2]
        y_hat = y_hat.reshape(target.shape)
        if target.dtype == torch.float32 and backend.loss_kernels_take(y_hat):
            from .ops import MimHuberFn
            return MimHuberFn.apply(y_hat, target, mask, self.delta, masked)
        return mim_huber_torch(y_hat, target, mask, self.patch, self.delta, masked)

    def settings(self):
        return {"patch": self.patch, "ratio": self.ratio, "fill": list(self.fill)}


def _mim_settings(who, mim):
    """mim= of RegTrainStep / train() -> None, or the settings() of the MaskedImageModelling it describes."""
    if mim is None or mim is False:
        return None
    if isinstance(mim, MaskedImageModelling):
        return mim.settings()
    if mim is True:
        kw = {}
    elif isinstance(mim, dict):
        if not set(mim) <= {"patch", "ratio", "fill"}:
            raise ValueError(f'{who}: mim takes the keys "patch", "ratio", "fill", got {sorted(mim)}')
        kw = dict(mim)
    elif isinstance(mim, (int, float)):
        kw = {"ratio": mim}
    else:
        raise ValueError(f'{who}: mim is None, True, a ratio or a dict with "patch" / "ratio" / "fill", got {mim!r}')
    return MaskedImageModelling(**kw).settings()          # (refuses a ratio outside (0, 1), a malformed patch or fill)


class TrainStep:
    """One iteration of distributed_trainer_cls.py:79-96 (per rank)."""

    def __init__(self, model, optimizer, reducer=None, max_norm=1.0, scaler=None, autocast_dtype=None, metrics=None,
                 ema=None, loss=None):
        """metrics: a StepMetrics the loss kernel accumulates into (only with the loss kernels switched on).
        ema: a ModelEMA of `model`, updated right behind the optimizer step; a step skipped for inf/NaN gradients leaves
        the average and its update count alone.
        loss: None / "ce" — soft_target_cross_entropy (cls:63,86) — or "bce" / {"name": "bce", "target_threshold": t,
        "sum_classes": bool} — soft_target_bce, the DeiT III / timm recipe's loss on the same soft targets."""
        self.model, self.opt, self.reducer = model, optimizer, reducer
        self.loss_settings = _loss_settings(type(self).__name__, loss)
        self.metrics = metrics
        self.ema = ema
        self.max_norm = max_norm
        self.scaler = scaler
        self.autocast_dtype = autocast_dtype          # torch.bfloat16: the reference's `with autocast(...)` (cls:84)
        self.params = [p for p in model.parameters() if p.requires_grad]
        # the device constants of the optimizer-side sequence, made once for the configurations that read them (None
        # otherwise): the GradScaler growth count of the fused step with the scalar its scale is read through, and the
        # (1,) scalar through which the torch path watches the scale for a skipped step
        self._clean_steps = self._one = self._ema_one = None
        if scaler is not None and scaler.is_enabled():
            dev = self.params[0].device
            if isinstance(optimizer, FusedClipAdamW):
                self._clean_steps = torch.zeros((), dtype=torch.int32, device=dev)
                self._one = torch.ones((), dtype=torch.float32, device=dev)
            elif ema is not None:
                self._ema_one = torch.ones(1, dtype=torch.float32, device=dev)

    def __call__(self, x, y_soft):
        with torch.autocast(device_type="cuda", dtype=self.autocast_dtype or torch.bfloat16,
                            enabled=self.autocast_dtype is not None and x.is_cuda):        # cls:84
            y_hat, _ = self.model(x)                                       # cls:85
            loss = self._loss(y_hat, y_soft)                               # cls:86
        return self._finish(loss, y_hat)

    def _loss(self, y_hat, y_soft):
        if self.loss_settings["name"] == "bce":
            return soft_target_bce(y_hat.squeeze(), y_soft, self.metrics, self.loss_settings["target_threshold"],
                                   self.loss_settings["sum_classes"])
        return soft_target_cross_entropy(y_hat.squeeze(), y_soft, self.metrics)

    def _tail_enabled(self):
        """The gradient tail hands autograd unfinished leaf gradients, so nothing but BucketedGradReducer (which flushes the
        queue first) may read gradients during the backward.  DistributedDataParallel does — C++ hooks on the
        AccumulateGrad nodes copy .grad into its buckets — and so would any other exchange this step does not know of:
        not armed for a model that is, or contains, a DistributedDataParallel, nor in a world of more than one rank
        without the reducer."""
        if any(isinstance(mod, torch.nn.parallel.DistributedDataParallel) for mod in self.model.modules()):
            return False
        return not (self.reducer is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)

    def _finish(self, loss, y_hat):
        """backward, gradient exchange, unscale / clip / optimizer step, zero_grad (cls:87-96)."""
        self._backward(loss)
        self._exchange()
        self._optimizer_step()
        return loss.detach(), y_hat.detach()

    def _backward(self, loss):
        from . import ops
        # the gradient tail (ops.grad_tail): leaf-gradient reductions of this backward run as a few multi-entry launches at
        # its end; armed only while no parameter has a .grad that autograd would add an unfinished tensor to
        with ops.grad_tail(self.params, enabled=self._tail_enabled()):
            if self.scaler is not None:
                self.scaler.scale(loss).backward()                             # cls:87
            else:
                loss.backward()

    def _exchange(self):
        if self.reducer is not None:
            self.reducer.finish()

    def _optimizer_step(self, m=1):
        """unscale / inf check / clip / optimizer step / EMA / scale update / zero_grad on the gradients of m micro-batches
        (their mean; m > 1 only from AccumTrainStep, where the fused optimizer's open window carries the divisor)."""
        if isinstance(self.opt, FusedClipAdamW):                           # cls:88-96 in three launches
            self.opt.max_norm = self.max_norm
            if self._clean_steps is not None:
                # GradScaler semantics on device, no host sync: unscale + inf check + skip-on-inf happen inside
                # calm_optim_step; the scale then backs off (x backoff) on inf/NaN or grows (x growth) after
                # growth_interval clean steps, exactly as scaler.step() / scaler.update() would do it
                sc = self.scaler
                scale = sc.scale(self._one)     # the current scale as a device tensor, no host sync; read once per window
                stats = self.opt.step(grad_scale=scale)
                if self.ema is not None:
                    self.ema.update(skip=stats[1:2])             # found_inf of this step, read on the device
                bad = stats[1] > 0
                # the counter is updated IN PLACE: a captured step (GraphedTrainStep) replays these kernels on the
                # addresses seen at capture, so a rebound tensor would leave every replay reading the pre-capture value
                # (the scale then never grows — or doubles on every replay from recycled memory)
                self._clean_steps.copy_(torch.where(bad, torch.zeros_like(self._clean_steps), self._clean_steps + 1))
                grow = self._clean_steps >= sc.get_growth_interval()
                new_scale = torch.where(bad, scale * sc.get_backoff_factor(),
                                        torch.where(grow, scale * sc.get_growth_factor(), scale))
                self._clean_steps.copy_(torch.where(grow, torch.zeros_like(self._clean_steps), self._clean_steps))
                sc.update(new_scale.detach())          # GradScaler.update(tensor) copies into its scale tensor in place
            else:
                stats = self.opt.step()
                if self.ema is not None:
                    self.ema.update(skip=stats[1:2])
            return
        if self.scaler is not None:
            self.scaler.unscale_(self.opt)                                 # cls:88
        if m > 1:                                                          # the mean of the window, in front of the clip
            torch._foreach_mul_([p.grad for p in self.params if p.grad is not None], 1.0 / m)
        torch.nn.utils.clip_grad_norm_(self.params, max_norm=self.max_norm, error_if_nonfinite=False)   # cls:92
        skip = None
        if self.scaler is not None:
            watch = self._ema_one is not None
            if watch:
                # scaler.step() skips optimizer.step() on inf/NaN and scaler.update() then backs the scale off: the step
                # was skipped exactly when the scale shrank.  Public API only, device arithmetic, no host sync.
                old_scale = self.scaler.scale(self._ema_one)
            self.scaler.step(self.opt)                                     # cls:93-94
            self.scaler.update()
            if watch:
                skip = (self.scaler.scale(self._ema_one) < old_scale).to(torch.float32)
        else:
            self.opt.step()
        if self.ema is not None:
            self.ema.update(skip=skip)
        self.opt.zero_grad()                                               # cls:96


class RegTrainStep(TrainStep):
    """One iteration of the generative trainer (distributed_trainer_reg.py:71-95): the `generate=True` model returns
    tokens [B,S,3S]; they are viewed as the image [B,3,S,S] (:78-79), loss = HuberLoss(img, x) + 0.1 * kl_loss
    (:81,87), then the same scale / clip(1.0) / optimizer step as the classification trainer.

    mim: a `MaskedImageModelling` or its settings dict (None: the job as above).  The step then draws a mask, feeds the
    model the MASKED row tokens and takes `mim.loss(tokens, clean tokens, mask)` + kl_weight * kl: the Huber term looks only
    where the input was replaced.  An image batch [B,3,S,S] is brought to row tokens once (ops.ImageToRowsFn; the first
    Block takes either).  Every forward draws its own mask, so under SamRegTrainStep the two passes see DIFFERENT masks, as
    they see different dropout keys; under AccumRegTrainStep every micro-batch draws one."""

    def __init__(self, model, optimizer, reducer=None, max_norm=1.0, scaler=None, autocast_dtype=None, kl_weight=0.1,
                 ema=None, loss=None, mim=None):
        _cross_entropy_only(type(self).__name__, loss, "the generative job's loss is Huber + kl_weight * kl, it has no "
                            "class targets")
        super().__init__(model, optimizer, reducer, max_norm=max_norm, scaler=scaler, autocast_dtype=autocast_dtype, ema=ema)
        self.kl_weight = kl_weight
        settings = _mim_settings(type(self).__name__, mim)
        self.mim = mim if isinstance(mim, MaskedImageModelling) else \
            None if settings is None else MaskedImageModelling(**settings)

    def __call__(self, x, _y=None):
        """x: the image [B,3,S,S], or the row tokens [B,S,3S] of the device collate — the channels-last image
        (Vi_Tools:389-391), which is then the Huber target in the layout of the model's output."""
        S = x.shape[1] if x.dim() == 3 else x.shape[-1]
        mask, x_in = None, x
        if self.mim is not None:
            if x.dim() == 4:
                from .ops import ImageToRowsFn
                x = ImageToRowsFn.apply(x)                                 # the clean tokens: the target
            mask = self.mim.draw(x.shape[0], S, x.device)
            x_in = self.mim.apply(x, mask)
        with torch.autocast(device_type="cuda", dtype=self.autocast_dtype or torch.bfloat16,
                            enabled=self.autocast_dtype is not None and x.is_cuda):        # reg:76
            y_hat, kl = self.model(x_in)                                   # reg:77
            img = y_hat.reshape(-1, S, S, 3).permute(0, 3, 1, 2)           # reg:78-79 (a view)
            huber = self._huber(y_hat, img, x) if mask is None else self.mim.loss(y_hat, x, mask)
            loss = huber + kl * self.kl_weight                             # reg:81,87
        return self._finish(loss, img)

    @staticmethod
    def _huber(tokens, img, x):
        """nn.HuberLoss() (reg:59, delta = 1): on the token layout through calm_huber_tokens_* when the loss kernels are
        switched on and serve the shape (S % 4 == 0, fp32), stock torch on the permuted view otherwise.  A 3-d x is the
        row-token batch: calm_recon_huber_rows_* (ops.HuberRowsFn) when the loss kernels take the tensors, stock torch on
        the two token tensors otherwise."""
        from . import backend
        if x.dim() == 3:
            y_hat = tokens.reshape(x.shape)
            if backend.get_loss_kernels() and x.dtype == torch.float32 and backend.loss_kernels_take(tokens):
                from .ops import HuberRowsFn
                return HuberRowsFn.apply(y_hat, x, 1.0)
            return torch.nn.functional.huber_loss(y_hat, x)
        if (backend.get_loss_kernels() and tokens.dim() == 3 and x.dim() == 4 and x.dtype == torch.float32
                and x.shape[-1] % 4 == 0 and x.shape[-1] <= 4096 and tokens.shape[0] == x.shape[0]
                and backend.loss_kernels_take(tokens)):
            from .ops import HuberTokensFn
            return HuberTokensFn.apply(tokens, x, 1.0)
        return torch.nn.functional.huber_loss(img, x)


class AccumTrainStep(TrainStep):
    """TrainStep with gradient accumulation over `accumulate` = k micro-batches.

    Every call runs forward, loss and backward of one micro-batch (the gradient tail armed as in TrainStep); the k-th
    call of a window also runs the gradient exchange and TrainStep's unscale / clip / optimizer step / EMA / scale update,
    ONCE, on the mean of the window's k gradients.  `boundary` tells whether the last call stepped; `flush()` steps an
    incomplete window of m < k micro-batches with divisor m.  With FusedClipAdamWindow every micro-batch goes through
    `accumulate()` (the deferred spectral-norm correction with that micro-batch's u, v, sigma, fp32 sums, `.grad`
    released); with a torch optimizer autograd adds into `.grad` and the sum is scaled by 1/m behind `unscale_`, in front
    of `clip_grad_norm_`: the two paths mean the same thing.  A window equals the torch loop "k x (forward, backward),
    then unscale / clip / step" with spectral norm iterating at every forward — not one k-times-larger batch.  The
    GradScaler's scale is read once per window and cannot change inside one; an inf/NaN in any micro-batch skips the
    whole window (EMA and step count untouched, scale backed off) and the next window's first micro-batch overwrites its
    sums.  reducer: a HeldGradReducer; with FusedClipAdamWindow its bucket views become the accumulators."""

    def __init__(self, model, optimizer, reducer=None, accumulate=2, **kw):
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"accumulate counts micro-batches per optimizer step (>= 1), got {accumulate!r}")
        if isinstance(optimizer, FusedClipAdamW) and not isinstance(optimizer, FusedClipAdamWindow):
            raise TypeError("AccumTrainStep needs FusedClipAdamWindow (FusedClipAdamW corrects the spectral-norm gradients "
                            "once per step, with the last forward's u, v, sigma)")
        if reducer is not None and reducer.enabled and not isinstance(reducer, HeldGradReducer):
            raise TypeError("AccumTrainStep needs a HeldGradReducer (BucketedGradReducer all-reduces every backward)")
        super().__init__(model, optimizer, reducer=reducer, **kw)    # (by keyword: DistillTrainStep's third is the teacher)
        self.accumulate = int(accumulate)
        self.window = 0                               # micro-batches in the open window
        self.boundary = True                          # whether the last call stepped the optimizer
        self.fused = isinstance(optimizer, FusedClipAdamWindow)
        if reducer is not None and reducer.enabled:
            reducer.hold = True
            if self.fused:
                optimizer.bind_accumulators(reducer.views_of(optimizer.params))      # the sums ARE the buckets

    def _finish(self, loss, y_hat):
        self._backward(loss)
        if self.fused:
            self.opt.accumulate()
        self.window += 1
        self.boundary = self.window >= self.accumulate
        if self.boundary:
            self._close_window()
        return loss.detach(), y_hat.detach()

    def flush(self):
        """Step an incomplete window (the m < accumulate micro-batches an epoch ends with), dividing by m.  False, and
        nothing done, when no window is open."""
        if self.window == 0:
            return False
        self._close_window()
        self.boundary = True
        return True

    def _close_window(self):
        m = self.window
        if self.reducer is not None and self.reducer.enabled:
            if self.fused:
                self.reducer.reduce_held()
            else:
                self.reducer.finish()
        self._optimizer_step(m)
        self.window = 0


class AccumRegTrainStep(AccumTrainStep, RegTrainStep):
    """RegTrainStep (the generative trainer's forward and loss) with AccumTrainStep's window."""

    def __init__(self, model, optimizer, reducer=None, accumulate=2, kl_weight=0.1, **kw):
        super().__init__(model, optimizer, reducer, accumulate=accumulate, kl_weight=kl_weight, **kw)


class DistillTrainStep(TrainStep):
    """TrainStep against a frozen teacher: the teacher's logits of the same batch first — a lean eval forward under
    torch.no_grad() through a `Predictor`, which stores nothing for a backward and draws no noise, so no RNG stream moves —
    then TrainStep's forward with `distillation_loss` in place of the cross-entropy, then the same backward / exchange /
    optimizer sequence.

    teacher: an nn.Module (wrapped in Predictor(teacher, autocast_dtype=...)) or a ready Predictor.  Its parameters get
    requires_grad_(False); it belongs to no optimizer, reducer, EMA, checkpoint or snapshot.  teacher_graph=True: the
    teacher forward is captured into a hipGraph at the shape of the first batch this step sees and replayed for every
    batch of that shape; other shapes run eagerly (Predictor's rule).  distill_metrics: a DistillMetrics the loss kernel
    accumulates into (only with the loss kernels switched on).  The teacher runs on the step's stream, in front of the
    student forward."""

    def __init__(self, model, optimizer, teacher, reducer=None, alpha=0.5, temperature=1.0, mode="soft", teacher_graph=False,
                 distill_metrics=None, loss=None, **kw):
        _cross_entropy_only(type(self).__name__, loss, "the distillation loss is (1 - alpha) * cross-entropy + the teacher "
                            "term (BCE distillation is not supported)")
        super().__init__(model, optimizer, reducer, **kw)
        _check_distill("DistillTrainStep: %s", mode, alpha, temperature)
        self.alpha, self.temperature, self.mode = float(alpha), float(temperature), mode
        self.distill_metrics = distill_metrics
        self.teacher = teacher if isinstance(teacher, Predictor) else Predictor(teacher, autocast_dtype=self.autocast_dtype)
        self.teacher_graph = bool(teacher_graph) and self.teacher.graph is None
        for p in self.teacher.model.parameters():
            p.requires_grad_(False)
        self._teacher_logits = None

    def _teacher_forward(self, x):
        if self.teacher_graph and x.is_cuda:                # the first batch: capture the teacher forward at its shape
            self.teacher = Predictor(self.teacher.model, example_x=x, autocast_dtype=self.teacher.autocast_dtype, graph=True)
            self.teacher_graph = False
        out = self.teacher(x)
        return (out[0] if isinstance(out, (tuple, list)) else out).detach()

    def __call__(self, x, y_soft):
        self._teacher_logits = self._teacher_forward(x)
        try:
            return super().__call__(x, y_soft)
        finally:
            self._teacher_logits = None

    def _loss(self, y_hat, y_soft):
        return distillation_loss(y_hat.squeeze(), self._teacher_logits.squeeze(), y_soft, self.alpha, self.temperature,
                                 self.mode, self.metrics, self.distill_metrics)


def _check_distill(label, mode, alpha, temperature):
    """The refusals DistillTrainStep and train() share; `label % name` is how the caller names a hyper-parameter."""
    if mode not in ("soft", "hard"):
        raise ValueError(f'{label % "mode"} is "soft" or "hard", got {mode!r}')
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"{label % 'alpha'} lies in [0, 1], got {alpha!r}")
    if not (float(temperature) > 0.0 and math.isfinite(float(temperature))):
        raise ValueError(f"{label % 'temperature'} is a positive finite number, got {temperature!r}")


class AccumDistillTrainStep(AccumTrainStep, DistillTrainStep):
    """DistillTrainStep (the teacher forward and the distillation loss) with AccumTrainStep's window."""

    def __init__(self, model, optimizer, teacher, reducer=None, accumulate=2, **kw):
        super().__init__(model, optimizer, reducer, accumulate=accumulate, teacher=teacher, **kw)


class DeviceCollate:
    """The batch-level part of the reference's input pipeline on the device:
    ToDtype(scale=True) + Normalize + RandomHorizontalFlip + RandomChoice([CutMix(alpha=1.0), MixUp(alpha=0.8)])
    with 1000-way soft labels (distributed_trainer_cls.py:58-61,128-139, torchvision.transforms.v2 semantics), one kernel
    pass over the uint8 batch (calm_collate_mix).  The decode / resize / colour augmentations stay with the loader.
    torchvision is not installed in the build image, so the semantics are restated from its documentation.
    (With an `augment=DeviceAugment(...)` argument the call also runs the colour augmentations on the device, and
    `DeviceResize` in front of the call runs the resize there: the batch it returns is the [B,3,Hs,Ws] uint8 input of
    this call, so the draws made here are the same with and without it.)"""

    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def __init__(self, num_classes=1000, cutmix_alpha=1.0, mixup_alpha=0.8, flip_p=0.5, seed=None):
        import numpy as np
        self.num_classes, self.cutmix_alpha, self.mixup_alpha, self.flip_p = num_classes, cutmix_alpha, mixup_alpha, flip_p
        self.rng = np.random.default_rng(seed)

    def draw(self, B, H, W):
        """(mode, lam, box, flips): the random decisions of one batch (host side, tiny)."""
        rng = self.rng
        mode = 2 if rng.random() < 0.5 else 1                               # RandomChoice([cut_mix, mix_up])
        alpha = self.cutmix_alpha if mode == 2 else self.mixup_alpha
        lam = float(rng.beta(alpha, alpha))
        box = None
        if mode == 2:
            box, lam = SoftMixCollate.cutmix_box(lam, int(rng.integers(0, W)), int(rng.integers(0, H)), H, W)
        flips = torch.from_numpy((rng.random(B) < self.flip_p).astype("uint8"))
        return mode, lam, box, flips

    def draw_corners(self, B, Hs, Ws, H, W):
        """int32 [B, 2] of (y0, x0): the RandomCrop corners of an H x W window inside Hs x Ws, the draws __call__ makes
        for crop=(H, W) after draw() — made here by a caller that needs them before the batch exists (a resize that
        computes only the window) and then passes crop=None and its decisions."""
        import numpy as np
        return np.stack([self.rng.integers(0, Hs - H + 1, B), self.rng.integers(0, Ws - W + 1, B)], axis=1).astype("int32")

    def __call__(self, img_u8, labels, decisions=None, crop=None, tokens=False, augment=None, aug_table=None, erase=None,
                 erase_table=None):
        """crop=(H, W): RandomCrop of every sample to H x W inside the (resized) source, corners drawn uniformly as
        torchvision's RandomCrop.get_params does (cls:130); tokens=True: the batch comes out as the row tokens
        [B, H, 3W] of the first Block (Vi_Tools_CNN_less_V2.py:389-391) — feed it to `model.autoencoder` / a ViT whose
        first Block skips the tokenisation — instead of the image [B,3,H,W].
        augment: a DeviceAugment — ColorJitter / solarize / grayscale / blur of cls:131-135 run in the same pass
        (calm_augment_collate) with parameters from the augment object's own generator, so the draws made here (mode,
        lam, box, flips, corners) are the ones made without it; aug_table: that per-sample table given instead of drawn
        (DeviceAugment.draw's format).  None (the default) is the plain collate.
        erase: a DeviceErase — RandomErasing behind Normalize and in front of the mix, in the same pass
        (calm_augment_collate_erase), with boxes and noise key from the erase object's own generator, drawn after
        everything else, so the draws made here and by `augment` are the ones made without it; erase_table: a
        (table, (seed, offset)) pair in DeviceErase.draw's format given instead of drawn (`erase` then only supplies the
        fill; without it the fill is noise).  Erasing lives in the augmenting kernel: without augment / aug_table the call
        runs it on DeviceAugment.identity(B) with the corners and flips filled in, so the plain-collate user then pays
        the augment kernel's LDS staging of every tile.  Without either argument nothing changes."""
        from .backend import get_backend
        B, _, Hs, Ws = img_u8.shape
        H, W = crop if crop is not None else (Hs, Ws)
        mode, lam, box, flips = decisions if decisions is not None else self.draw(B, H, W)
        corners = corners_host = None
        if crop is not None:
            corners_host = self.draw_corners(B, Hs, Ws, H, W)
            corners = torch.from_numpy(corners_host).to(img_u8.device)
        out = torch.empty((B, H, 3 * W) if tokens else (B, 3, H, W), dtype=torch.float32, device=img_u8.device)
        erasing = erase is not None or erase_table is not None
        if augment is not None or aug_table is not None or erasing:
            table = aug_table if aug_table is not None else augment.draw(B) if augment is not None else DeviceAugment.identity(B)
            DeviceAugment.check_window(table, H, W)
            samples = DeviceAugment.pack(table, corners_host, flips, device=img_u8.device)
            self.last_gray_mean = torch.empty(B, dtype=torch.float32, device=img_u8.device)
            if erasing:
                boxes, key = erase_table if erase_table is not None else erase.draw(B, H, W)
                if len(boxes) != B:
                    raise ValueError(f"DeviceCollate: the erase table holds {len(boxes)} boxes for a batch of {B}")
                DeviceErase.check(boxes, H, W)
                get_backend().augment_collate_erase(img_u8, samples, self.last_gray_mean, out, mode, lam, box, self.MEAN,
                                                    self.STD, DeviceErase.pack(boxes, device=img_u8.device),
                                                    erase.value if erase is not None else None, key, tokens=tokens)
            else:
                get_backend().augment_collate(img_u8, samples, self.last_gray_mean, out, mode, lam, box, self.MEAN,
                                              self.STD, tokens=tokens)
        elif crop is None and not tokens:
            get_backend().collate_mix(img_u8, flips.to(img_u8.device), out, mode, lam, box, self.MEAN, self.STD)
        else:
            get_backend().collate_crop_mix(img_u8, corners, flips.to(img_u8.device), out, mode, lam, box, self.MEAN, self.STD,
                                           tokens=tokens)
        onehot = torch.nn.functional.one_hot(labels, self.num_classes).to(torch.float32)
        y = onehot * lam + onehot.roll(1, 0) * (1.0 - lam)
        self.last_corners = corners
        return out, y


def _records_to_device(t, device):
    """A numpy record array as the uint8 tensor [B, itemsize] of its bytes on `device`: one host-to-device copy."""
    import numpy as np
    return torch.from_numpy(t.view(np.uint8).reshape(len(t), t.dtype.itemsize)).to(device)


def _meta_columns(who, meta, max_side):
    """(offset, h, w), int64 [B] each, of a RaggedU8Collate meta table; the sides are checked against 1 .. max_side."""
    import numpy as np
    m = np.asarray(meta.cpu() if isinstance(meta, torch.Tensor) else meta, dtype=np.int64)
    if m.ndim != 2 or m.shape[1] != 3 or m.shape[0] < 1:
        raise ValueError(f"{who}: meta must be [B, 3] (offset, h, w), got shape {m.shape}")
    off, h, w = m[:, 0], m[:, 1], m[:, 2]
    if (h < 1).any() or (w < 1).any() or (h > max_side).any() or (w > max_side).any():
        raise ValueError(f"{who}: source sides must be within 1 .. {max_side}")
    return off, h, w


class DeviceAugment:
    """The per-sample random parameters of the reference's colour augmentations (distributed_trainer_cls.py:131-135,
    defaults from there) for the device pass calm_augment_collate:
      ColorJitter(brightness, contrast, saturation, hue): a factor drawn uniformly from each range and a random order of
        the four operations per sample, as torchvision's ColorJitter draws them (a range of None leaves the operation out);
      RandomSolarize(solarize_threshold, p=solarize_p); RandomGrayscale(p=grayscale_p);
      GaussianBlur(3, sigma=blur_sigma): sigma uniform in the range (None: no blur).
    Deviation from the reference, stated: it applies these operations to 8-bit PIL images and rounds after each one; the
    device pass keeps fp32 on [0, 1] throughout and quantises nowhere (tests/test_augment_cpu.py bounds the difference
    per operation).  The 8-bit comparison `level >= solarize_threshold` becomes `v >= (solarize_threshold - 0.5) / 255`.
    The object owns its generator: the draws of DeviceCollate do not shift when it is used."""

    def __init__(self, seed=None, brightness=(0.5, 1), contrast=(0.5, 1), saturation=(0.5, 1), hue=(-0.125, 0.125),
                 solarize_p=0.5, solarize_threshold=224, grayscale_p=0.1, blur_sigma=(0.1, 2.0)):
        import numpy as np
        self.ranges = (brightness, contrast, saturation, hue)              # indexed by the operation id
        self.solarize_p, self.solarize_threshold, self.grayscale_p = solarize_p, solarize_threshold, grayscale_p
        self.blur_sigma = blur_sigma
        self.rng = np.random.default_rng(seed)

    @staticmethod
    def dtype():
        """The numpy record of struct calm_aug_sample."""
        import numpy as np
        from . import _lib
        return np.dtype(_lib.AugSample)

    @classmethod
    def identity(cls, B):
        """A table of B samples with no operation and no flag."""
        import numpy as np
        from . import _lib
        t = np.zeros(B, dtype=cls.dtype())
        t["order"] = _lib.AUG_OP_NONE
        t["brightness"] = t["contrast"] = t["saturation"] = 1.0
        return t

    def draw(self, B):
        """The per-sample table of one batch (a numpy record array of calm_aug_sample; corners and the flip bit are
        DeviceCollate's and are filled in by pack)."""
        import numpy as np
        from . import _lib
        rng = self.rng
        t = self.identity(B)
        perm = rng.permuted(np.tile(np.arange(4, dtype=np.uint8), (B, 1)), axis=1)
        names = ("brightness", "contrast", "saturation", "hue")
        for op, (name, rg) in enumerate(zip(names, self.ranges)):
            if rg is None:
                perm[perm == op] = _lib.AUG_OP_NONE
            else:
                t[name] = rng.uniform(rg[0], rg[1], B).astype(np.float32)
        # the operations left out move to the end of the order (they are skipped wherever they stand)
        t["order"] = np.take_along_axis(perm, np.argsort(perm == _lib.AUG_OP_NONE, axis=1, kind="stable"), axis=1)
        flags = np.zeros(B, dtype=np.uint32)
        flags |= np.where(rng.random(B) < self.solarize_p, _lib.AUG_SOLARIZE, 0).astype(np.uint32)
        flags |= np.where(rng.random(B) < self.grayscale_p, _lib.AUG_GRAYSCALE, 0).astype(np.uint32)
        t["solarize_thr"] = np.float32((self.solarize_threshold - 0.5) / 255.0)
        if self.blur_sigma is not None:
            flags |= np.uint32(_lib.AUG_BLUR)
            t["blur_sigma"] = rng.uniform(self.blur_sigma[0], self.blur_sigma[1], B).astype(np.float32)
        t["flags"] = flags
        return t

    @staticmethod
    def check_window(table, H, W):
        from . import _lib
        if (H < 2 or W < 2) and bool((table["flags"] & _lib.AUG_BLUR).any()):
            raise ValueError(f"the 3x3 blur reflects at the window's edge: it needs a window of at least 2 x 2, got {H} x {W}")

    @staticmethod
    def pack(table, corners=None, flips=None, device="cuda"):
        """The device array of calm_aug_sample records, [B,48] uint8, in one host-to-device copy: `table` with the crop
        corners ([B,2] integers, None = (0, 0)) and the flip decisions ([B], None = keep the table's bits) filled in."""
        import numpy as np
        from . import _lib
        t = np.array(table, dtype=DeviceAugment.dtype(), copy=True)
        if corners is not None:
            c = np.asarray(corners)
            t["y0"], t["x0"] = c[:, 0], c[:, 1]
        if flips is not None:
            f = np.asarray(flips).astype(bool)
            t["flags"] = (t["flags"] & ~np.uint32(_lib.AUG_FLIP)) | np.where(f, _lib.AUG_FLIP, 0).astype(np.uint32)
        return _records_to_device(t, device)


class DeviceErase:
    """The per-sample boxes of RandomErasing (Zhong et al.; torchvision.transforms.v2.RandomErasing, timm's "pixel" mode)
    for the device pass calm_augment_collate_erase: with probability p a sample gets one rectangle of the OUTPUT window
    — after crop and flip, behind Normalize, in front of CutMix / MixUp — replaced by `value`:
      "random": per-pixel, per-channel standard normal noise drawn on the device from the batch's (seed, offset) key;
      a float or three floats: that constant per channel, in normalised space (0.0 is the dataset mean).
    The box follows torchvision's RandomErasing.get_params, restated (torchvision is not installed in the build image):
    up to 10 attempts of area = H W U(scale), aspect = exp(U(ln ratio[0], ln ratio[1])), h = round(sqrt(area aspect)),
    w = round(sqrt(area / aspect)), accepted when 0 < h < H and 0 < w < W, then the corner uniform over the positions that
    keep the box inside; a sample for which no attempt fits is not erased.  The draws are numpy's, from this object's own
    generator: bit-parity of the draws with torchvision (torch's generator) is not claimed, and the draws of DeviceCollate
    and DeviceAugment do not shift when the object is used."""

    def __init__(self, p=0.25, scale=(0.02, 1.0 / 3.0), ratio=(0.3, 3.3), value="random", seed=None):
        import numpy as np
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"DeviceErase: p is a probability, got {p!r}")
        if not (len(scale) == 2 and 0.0 < scale[0] <= scale[1] <= 1.0):
            raise ValueError(f"DeviceErase: scale is a range of area shares within (0, 1], got {scale!r}")
        if not (len(ratio) == 2 and 0.0 < ratio[0] <= ratio[1]):
            raise ValueError(f"DeviceErase: ratio is a range of positive aspect ratios, got {ratio!r}")
        if isinstance(value, str):
            if value != "random":
                raise ValueError(f'DeviceErase: value is "random", a float or three floats, got {value!r}')
            self.value = None
        else:
            v = tuple(float(c) for c in np.atleast_1d(np.asarray(value, dtype=np.float64)))
            if len(v) not in (1, 3) or not all(np.isfinite(v)):
                raise ValueError(f'DeviceErase: value is "random", a float or three floats, got {value!r}')
            self.value = v * 3 if len(v) == 1 else v
        self.p, self.scale, self.ratio = float(p), (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.rng = np.random.default_rng(seed)
        self.seed = int(self.rng.integers(0, 2 ** 64, dtype=np.uint64))     # the noise key's seed: fixed for the object

    @staticmethod
    def dtype():
        """The numpy record of struct calm_erase_box."""
        import numpy as np
        from . import _lib
        return np.dtype(_lib.EraseBox)

    @classmethod
    def identity(cls, B):
        """A table of B samples none of which is erased."""
        import numpy as np
        return np.zeros(B, dtype=cls.dtype())

    def draw(self, B, H, W):
        """(table, (seed, offset)): the boxes of one batch (a numpy record array of calm_erase_box) and its noise key —
        the samples in order, then one 64-bit offset for the batch."""
        import math
        import numpy as np
        rng = self.rng
        t = self.identity(B)
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for b in range(B):
            if not rng.random() < self.p:
                continue
            for _ in range(10):
                area = H * W * rng.uniform(self.scale[0], self.scale[1])
                aspect = math.exp(rng.uniform(log_ratio[0], log_ratio[1]))
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if not (0 < h < H and 0 < w < W):
                    continue
                t[b] = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w)
                break
        offset = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        return t, (self.seed, offset)

    @staticmethod
    def check(table, H, W):
        """Refuses a table the kernel must not get: a negative field, or a box that leaves the H x W window."""
        import numpy as np
        t = np.asarray(table)
        y, x, h, w = (t[f].astype(np.int64) for f in ("y", "x", "h", "w"))
        if bool(((y < 0) | (x < 0) | (h < 0) | (w < 0)).any()):
            raise ValueError("DeviceErase: a box has a negative field")
        if bool(((y + h > H) | (x + w > W)).any()):
            raise ValueError(f"DeviceErase: a box leaves the {H} x {W} window")

    @staticmethod
    def pack(table, device="cuda"):
        """The device array of calm_erase_box records, [B,16] uint8, in one host-to-device copy."""
        import numpy as np
        return _records_to_device(np.array(table, dtype=DeviceErase.dtype(), copy=True), device)


class DeviceRandAugment:
    """RandAugment (Cubuk et al.; torchvision.transforms.v2.RandAugment on a PIL image, restated — torchvision is not
    installed in the build image) as a uint8 -> uint8 device stage in front of the collate (calm_randaugment_u8): per
    sample the RandomCrop window and the flip, then `num_ops` operations drawn uniformly from `ops`, every one rounded to
    uint8 as PIL rounds it — the batch equals the PIL chain byte for byte (tests/test_randaug_cpu.py, test_randaug_gpu.py).

    The augmentation space is torchvision's 14 operations, magnitude bin `magnitude` of `num_bins`:
      Identity; ShearX, ShearY linspace(0, 0.3); TranslateX, TranslateY int(linspace(0, 150 / 331 * side)) pixels, side = W
      for X and H for Y; Rotate linspace(0, 30) degrees; Brightness, Color, Contrast, Sharpness factor 1 +- linspace(0, 0.9);
      Posterize 8 - round(i / ((num_bins - 1) / 4)) bits; Solarize threshold linspace(255, 0); AutoContrast; Equalize.
    The signed operations (shears, translations, rotation, the four enhances) flip their sign with probability 1/2.
    `fill`: one integer or three, 0 .. 255, the colour of the pixels a warp brings in from outside the window.
    `trivial_wide(...)` is TrivialAugmentWide on the same kernel: one operation, a uniformly drawn bin, the wide ranges
    (shear 0.99, translation 32 pixels, rotation 135 degrees, enhances 0.99, posterize 8 - round(i / ((num_bins - 1) / 6))).
    The draws are numpy's, from this object's own generator: bit-parity of the draws with torchvision (torch's generator)
    is not claimed, and the draws of DeviceCollate, DeviceAugment, DeviceErase and DeviceResizedCrop do not shift when the
    object is used."""

    OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
           "Posterize", "Solarize", "AutoContrast", "Equalize")
    SIGNED = frozenset(("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness"))

    def __init__(self, num_ops=2, magnitude=9, num_bins=31, fill=0, ops=None, seed=None, _wide=False):
        import numpy as np
        from . import _lib
        if isinstance(num_ops, bool) or int(num_ops) != num_ops or not 0 <= num_ops <= _lib.RA_MAX_OPS:
            raise ValueError(f"DeviceRandAugment: num_ops counts operations per sample, 0 .. {_lib.RA_MAX_OPS}, got {num_ops!r}")
        if isinstance(num_bins, bool) or int(num_bins) != num_bins or num_bins < 2:
            raise ValueError(f"DeviceRandAugment: num_bins counts magnitude bins (>= 2), got {num_bins!r}")
        if isinstance(magnitude, bool) or int(magnitude) != magnitude or not 0 <= magnitude < num_bins:
            raise ValueError(f"DeviceRandAugment: magnitude is a bin, 0 .. num_bins - 1 = {int(num_bins) - 1}, got {magnitude!r}")
        ops = tuple(self.OPS if ops is None else ops)
        if not ops or any(o not in self.OPS for o in ops):
            raise ValueError(f"DeviceRandAugment: ops is a non-empty selection of {self.OPS}, got {ops!r}")
        f = tuple(np.atleast_1d(np.asarray(fill)).tolist())
        f = f * 3 if len(f) == 1 else f
        if len(f) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 255 for v in f):
            raise ValueError(f"DeviceRandAugment: fill is one integer or three in 0 .. 255, got {fill!r}")
        self.num_ops, self.magnitude, self.num_bins, self.fill, self.ops = int(num_ops), int(magnitude), int(num_bins), f, ops
        self.wide = bool(_wide)
        self.rng = np.random.default_rng(seed)
        self._scratch = None

    @classmethod
    def trivial_wide(cls, num_bins=31, fill=0, ops=None, seed=None):
        """TrivialAugmentWide: one operation per sample with a uniformly drawn magnitude bin over the wide ranges."""
        return cls(num_ops=1, magnitude=0, num_bins=num_bins, fill=fill, ops=ops, seed=seed, _wide=True)

    @staticmethod
    def dtype():
        """The numpy record of struct calm_ra_sample."""
        import numpy as np
        from . import _lib
        return np.dtype(_lib.RaSample)

    @classmethod
    def identity(cls, B):
        """A table of B samples with no operation, no flip and the corner (0, 0); the unused slots hold the identity."""
        import numpy as np
        t = np.zeros(B, dtype=cls.dtype())
        t["factor"] = 1.0
        t["coef"] = (65536, 0, 32768, 0, 65536, 32768)
        return t

    def magnitudes(self, name, H, W):
        """The magnitude of every bin for operation `name` on an H x W window, float64 [num_bins] (None: the operation has
        none): the table of torchvision's _augmentation_space, RandAugment's or TrivialAugmentWide's."""
        import numpy as np
        n, wide = self.num_bins, self.wide
        if name in ("Identity", "AutoContrast", "Equalize"):
            return None
        if name in ("ShearX", "ShearY"):
            return np.linspace(0.0, 0.99 if wide else 0.3, n)
        if name in ("TranslateX", "TranslateY"):
            return np.linspace(0.0, 32.0 if wide else 150.0 / 331.0 * (W if name == "TranslateX" else H), n)
        if name == "Rotate":
            return np.linspace(0.0, 135.0 if wide else 30.0, n)
        if name in ("Brightness", "Color", "Contrast", "Sharpness"):
            return np.linspace(0.0, 0.99 if wide else 0.9, n)
        if name == "Posterize":
            return 8.0 - np.round(np.arange(n) / ((n - 1) / (6.0 if wide else 4.0)))
        return np.linspace(255.0, 0.0, n)                                    # Solarize

    @staticmethod
    def fixed_coeffs(a):
        """(A0 .. A5): the six doubles of an inverse affine map in PIL's 16.16 fixed point (the header's FIX)."""
        import math
        fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
        a = [float(v) for v in a]
        return (fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5))

    @classmethod
    def slot(cls, name, value, H, W):
        """(op id, factor, param, coef) of operation `name` with the signed magnitude `value` on an H x W window."""
        import math
        import numpy as np
        from . import _lib
        ident = (65536, 0, 32768, 0, 65536, 32768)
        if name in ("Identity", "AutoContrast", "Equalize"):
            return {"Identity": _lib.RA_OP_IDENTITY, "AutoContrast": _lib.RA_OP_AUTOCONTRAST,
                    "Equalize": _lib.RA_OP_EQUALIZE}[name], 1.0, 0, ident
        if name in ("Brightness", "Color", "Contrast", "Sharpness"):
            op = {"Brightness": _lib.RA_OP_BRIGHTNESS, "Color": _lib.RA_OP_COLOR, "Contrast": _lib.RA_OP_CONTRAST,
                  "Sharpness": _lib.RA_OP_SHARPNESS}[name]
            return op, float(np.float32(1.0 + value)), 0, ident
        if name == "Posterize":
            return _lib.RA_OP_POSTERIZE, 1.0, int(value), ident
        if name == "Solarize":                                               # i < threshold on integers i
            return _lib.RA_OP_SOLARIZE, 1.0, int(math.ceil(value)), ident
        if name == "ShearX":
            a = (1.0, float(value), 0.0, 0.0, 1.0, 0.0)
        elif name == "ShearY":
            a = (1.0, 0.0, 0.0, float(value), 1.0, 0.0)
        elif name == "TranslateX":
            a = (1.0, 0.0, -float(int(value)), 0.0, 1.0, 0.0)
        elif name == "TranslateY":
            a = (1.0, 0.0, 0.0, 0.0, 1.0, -float(int(value)))
        elif name == "Rotate":                                               # Image.rotate's matrix about (W / 2, H / 2)
            r = -math.radians(value % 360.0)
            m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
            cx, cy = W / 2.0, H / 2.0
            m[2] = m[0] * -cx + m[1] * -cy + m[2]
            m[5] = m[3] * -cx + m[4] * -cy + m[5]
            m[2] += cx
            m[5] += cy
            a = m
        else:
            raise ValueError(f"DeviceRandAugment: no operation {name!r}")
        return _lib.RA_OP_AFFINE, 1.0, 0, cls.fixed_coeffs(a)

    def draw(self, B, H, W):
        """The record table of one batch (a numpy record array of calm_ra_sample; corners and flips are DeviceCollate's
        and are filled in by pack).  Per batch, in this order: the operation indices [B, num_ops], the sign decisions
        [B, num_ops] (drawn for every slot, used by the signed operations) and, for trivial_wide, the bins [B, num_ops]."""
        rng, k = self.rng, self.num_ops
        t = self.identity(B)
        which = rng.integers(0, len(self.ops), (B, k))
        negate = rng.random((B, k)) < 0.5
        bins = rng.integers(0, self.num_bins, (B, k)) if self.wide else None
        mags = {name: self.magnitudes(name, H, W) for name in self.ops}
        t["n_ops"] = k
        for b in range(B):
            for j in range(k):
                name = self.ops[which[b, j]]
                m = mags[name]
                value = 0.0 if m is None else float(m[bins[b, j] if self.wide else self.magnitude])
                if name in self.SIGNED and negate[b, j]:
                    value = -value
                t["op"][b, j], t["factor"][b, j], t["param"][b, j], t["coef"][b, j] = self.slot(name, value, H, W)
        return t

    @staticmethod
    def check(table, H, W):
        """Refuses a table the stage must not get: n_ops outside 0 .. 4, an operation id outside the table, posterize bits
        outside 0 .. 8, a non-finite factor, or affine coefficients outside the bounds under which the kernel's 32-bit
        sums cannot overflow (|A0|, |A1|, |A3|, |A4| <= 2^17, |A2|, |A5| <= 2^30; H, W <= 4096)."""
        import numpy as np
        from . import _lib
        t = np.asarray(table)
        if H > _lib.RA_MAX_SIDE or W > _lib.RA_MAX_SIDE or H < 1 or W < 1:
            raise ValueError(f"DeviceRandAugment: the window's sides are 1 .. {_lib.RA_MAX_SIDE}, got {H} x {W}")
        n = t["n_ops"].astype(np.int64)
        if bool(((n < 0) | (n > _lib.RA_MAX_OPS)).any()):
            raise ValueError(f"DeviceRandAugment: n_ops is 0 .. {_lib.RA_MAX_OPS}")
        used = np.arange(_lib.RA_MAX_OPS)[None, :] < n[:, None]
        op = t["op"].astype(np.int64)
        if bool((used & ((op < 0) | (op > _lib.RA_OP_EQUALIZE))).any()):
            raise ValueError("DeviceRandAugment: an operation id outside the table")
        if bool((used & (op == _lib.RA_OP_POSTERIZE) & ((t["param"] < 0) | (t["param"] > 8))).any()):
            raise ValueError("DeviceRandAugment: posterize keeps 0 .. 8 bits")
        if bool((used & ~np.isfinite(t["factor"])).any()):
            raise ValueError("DeviceRandAugment: a factor is not finite")
        c = np.abs(t["coef"].astype(np.int64))
        big = (c[:, :, [0, 1, 3, 4]] > 2 ** 17).any(axis=2) | (c[:, :, [2, 5]] > 2 ** 30).any(axis=2)
        if bool((used & (op == _lib.RA_OP_AFFINE) & big).any()):
            raise ValueError("DeviceRandAugment: affine coefficients outside |A0, A1, A3, A4| <= 2^17, |A2, A5| <= 2^30")

    @staticmethod
    def launch_plan(table):
        """(n_slots, stats_mask) of a table: the slot passes the batch needs and, bit k, whether some sample's slot k needs
        the statistics launch (Contrast, AutoContrast, Equalize)."""
        import numpy as np
        from . import _lib
        t = np.asarray(table)
        n = np.clip(t["n_ops"].astype(np.int64), 0, _lib.RA_MAX_OPS)
        n_slots = int(n.max()) if len(n) else 0
        used = np.arange(_lib.RA_MAX_OPS)[None, :] < n[:, None]
        need = used & np.isin(t["op"], _lib.RA_STATS_OPS)
        return n_slots, sum(1 << k for k in range(_lib.RA_MAX_OPS) if bool(need[:, k].any()))

    @staticmethod
    def pack(table, corners=None, flips=None, device="cuda"):
        """The device array of calm_ra_sample records, [B,160] uint8, in one host-to-device copy: `table` with the crop
        corners ([B,2] integers, None = keep the table's) and the flip decisions ([B], None = keep) filled in."""
        import numpy as np
        t = np.array(table, dtype=DeviceRandAugment.dtype(), copy=True)
        if corners is not None:
            c = np.asarray(corners)
            t["y0"], t["x0"] = c[:, 0], c[:, 1]
        if flips is not None:
            t["flip"] = np.asarray(flips).astype(bool).astype(np.uint32)
        return _records_to_device(t, device)

    def __call__(self, img_u8, corners=None, flips=None, crop=None, table=None):
        """img_u8 [B,3,Hs,Ws] uint8 on the device -> [B,3,H,W] uint8: the window crop=(H, W) at `corners` ([B,2] host
        integers; None: (0, 0), and crop=None: the whole image), the flips ([B], None: none), then the drawn chain —
        or `table`, draw()'s format, given instead of drawn.  The collate behind it takes the batch with crop=None and
        no flips."""
        from .backend import get_backend
        B, _, Hs, Ws = img_u8.shape
        H, W = crop if crop is not None else (Hs, Ws)
        if table is None:
            table = self.draw(B, H, W)
        if len(table) != B:
            raise ValueError(f"DeviceRandAugment: the table holds {len(table)} records for a batch of {B}")
        self.check(table, H, W)
        n_slots, stats_mask = self.launch_plan(table)
        be = get_backend()
        out = torch.empty((B, 3, H, W), dtype=torch.uint8, device=img_u8.device)
        need = be.randaugment_scratch_bytes(B, H, W)
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != img_u8.device:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=img_u8.device)
        be.randaugment_u8(img_u8, self.pack(table, corners, flips, device=img_u8.device), out, n_slots, stats_mask,
                          fill=self.fill, scratch=self._scratch)
        return out


class RaggedU8Collate:
    """DataLoader collate_fn for decoded images of different sizes: samples `(uint8 [h, w, 3], label)` — the array
    np.asarray(pil_image) gives, or a tensor of that shape — become
      packed  uint8 [N]     the images' bytes one after the other, each starting at a multiple of ALIGN = 16 bytes,
      meta    int64 [B, 3]  (byte offset, h, w) per image,
      labels  int64 [B].
    One host-to-device copy per batch then moves every image, whatever its size, and `DeviceResize` turns the packed
    buffer into the [B,3,oh,ow] uint8 batch `DeviceCollate` reads.  The object holds no state: it pickles into worker
    processes, and the three tensors go through the loader's pin_memory like any other batch."""

    ALIGN = 16

    def __call__(self, batch):
        import numpy as np
        imgs = [np.ascontiguousarray(np.asarray(img)) for img, _ in batch]
        meta = np.empty((len(imgs), 3), dtype=np.int64)
        end = 0
        for b, a in enumerate(imgs):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise TypeError(f"RaggedU8Collate expects uint8 images [h, w, 3], got {a.dtype} {a.shape}")
            off = -(-end // self.ALIGN) * self.ALIGN
            meta[b] = off, a.shape[0], a.shape[1]
            end = off + a.size
        packed = np.zeros(end, dtype=np.uint8)
        for (off, _, _), a in zip(meta, imgs):
            packed[off:off + a.size] = a.reshape(-1)
        labels = torch.as_tensor([int(label) for _, label in batch], dtype=torch.int64)
        return torch.from_numpy(packed), torch.from_numpy(meta), labels


class DeviceResize:
    """transforms.Resize(size) of the reference's list (distributed_trainer_cls.py:129) on the device: on a PIL image that
    is Image.resize(size, BILINEAR) — antialiased, two passes, 22-bit fixed point — and calm_resize_u8 computes the same
    bytes.  `size` is (oh, ow).  __call__(packed_dev, meta): the packed uint8 device buffer and the host int64 [B,3] table
    of (offset, h, w) a RaggedU8Collate returns -> uint8 [B,3,oh,ow] on the device.  Source sides 1 .. 16384."""

    MAX_SIDE = 16384

    def __init__(self, size=(256, 256)):
        try:
            oh, ow = (int(v) for v in size)
        except TypeError:
            raise ValueError(f"DeviceResize takes size=(oh, ow), got {size!r}") from None
        if not (1 <= oh <= self.MAX_SIDE and 1 <= ow <= self.MAX_SIDE):
            raise ValueError(f"DeviceResize: output sides must be within 1 .. {self.MAX_SIDE}, got {(oh, ow)}")
        self.size = (oh, ow)

    @staticmethod
    def dtype():
        """The numpy record of struct calm_resize_sample."""
        import numpy as np
        from . import _lib
        return np.dtype(_lib.ResizeSample)

    @classmethod
    def records(cls, meta, nbytes):
        """The host array of calm_resize_sample records for a meta table, checked against a buffer of nbytes bytes (the
        kernel would write zeros for a record it cannot read; here it is an error)."""
        import numpy as np
        off, h, w = _meta_columns("DeviceResize", meta, cls.MAX_SIDE)
        if (off < 0).any() or (off + 3 * h * w > nbytes).any():
            raise ValueError("DeviceResize: an image lies outside the packed buffer")
        t = np.zeros(len(off), dtype=cls.dtype())
        t["offset"], t["h"], t["w"] = off, h, w
        return t

    @classmethod
    def pack(cls, meta, nbytes, device="cuda"):
        """The device array of calm_resize_sample records, [B,16] uint8, in one host-to-device copy."""
        return _records_to_device(cls.records(meta, nbytes), device)

    def __call__(self, packed_dev, meta):
        from .backend import get_backend
        samples = self.pack(meta, packed_dev.numel(), device=packed_dev.device)
        out = torch.empty((samples.shape[0], 3) + self.size, dtype=torch.uint8, device=packed_dev.device)
        get_backend().resize_u8(packed_dev, samples, out)
        return out


class DeviceResizedCrop:
    """Crop a box of every image, resize it with PIL's antialiased bilinear arithmetic and keep a window of the result, in
    one launch over the packed originals of a RaggedU8Collate (calm_resized_crop): per sample a source box, the size
    vh x vw the box is resized to and the top-left corner of the H x W window inside it.  The bytes are those of
    `Image.crop(box).resize((vw, vh), BILINEAR)` — torchvision's resized_crop on a PIL image — sliced to the window.
    torchvision is not installed in the build image, so the semantics of its transforms are restated from its
    documentation; the draws are host-side numpy.  Three constructors:

      .center(resize=256, crop=(224, 224))   Resize(int) + CenterCrop, the standard validation transform: the short side
          goes to `resize`, the long one to int(resize * long / short); the window is the central crop, top =
          int(round((vh - H) / 2.0)).  An image whose resized size does not hold the crop is a ValueError (torchvision
          would pad it).
      .random_resized(size=(224, 224), scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), seed=None)   RandomResizedCrop: per image
          up to ten attempts at a box of area uniform in `scale` times the image's and of log-uniform aspect ratio, the
          corner uniform; after ten failures the central box with the ratio clamped.  The box is resized to `size`.  The
          object owns its generator: the draws of DeviceCollate do not move.
      .window(size=(256, 256), crop=(224, 224))   Resize(size) of which only the crop window is computed; the corners
          ([B, 2] of (y0, x0), DeviceCollate.draw_corners) are given at the call.

    __call__(packed_dev, meta, corners=None, out="u8" | "image" | "tokens") -> uint8 [B,3,H,W] (what DeviceCollate
    reads), fp32 [B,3,H,W] normalised with DeviceCollate's mean / std, or the fp32 row tokens [B,H,3W] of the first
    Block.  The host records of the last call stay in `last_records`."""

    MAX_SIDE = 16384
    MEAN, STD = DeviceCollate.MEAN, DeviceCollate.STD
    OUTPUTS = ("u8", "image", "tokens")

    def __init__(self, kind, size, resize=None, scale=None, ratio=None, seed=None):
        """Use the constructors .center / .random_resized / .window."""
        import numpy as np
        if kind not in ("center", "random_resized", "window"):
            raise ValueError(f"DeviceResizedCrop: unknown kind {kind!r}")
        self.kind, self.size, self.resize, self.scale, self.ratio = kind, size, resize, scale, ratio
        self.rng = np.random.default_rng(seed) if kind == "random_resized" else None
        self.last_records = self.last_fallback = None

    @classmethod
    def _pair(cls, what, v):
        try:
            a, b = (int(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"DeviceResizedCrop: {what} must be a pair of sides, got {v!r}") from None
        if not (1 <= a <= cls.MAX_SIDE and 1 <= b <= cls.MAX_SIDE):
            raise ValueError(f"DeviceResizedCrop: {what} must be within 1 .. {cls.MAX_SIDE}, got {(a, b)}")
        return a, b

    @classmethod
    def center(cls, resize=256, crop=(224, 224)):
        H, W = cls._pair("crop", crop)
        if isinstance(resize, bool) or not isinstance(resize, int) or not 1 <= resize <= cls.MAX_SIDE:
            raise ValueError(f"DeviceResizedCrop.center: resize is the short side, an integer within 1 .. {cls.MAX_SIDE}, "
                             f"got {resize!r}")
        if H > resize and W > resize:
            raise ValueError(f"DeviceResizedCrop.center: a crop of {(H, W)} never fits a short side of {resize}")
        return cls("center", (H, W), resize=resize)

    @classmethod
    def random_resized(cls, size=(224, 224), scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), seed=None):
        size = cls._pair("size", size)
        try:
            (s0, s1), (r0, r1) = (float(v) for v in scale), (float(v) for v in ratio)
        except (TypeError, ValueError):
            raise ValueError("DeviceResizedCrop.random_resized: scale and ratio are (min, max) pairs") from None
        if not (0.0 < s0 <= s1 and 0.0 < r0 <= r1):
            raise ValueError(f"DeviceResizedCrop.random_resized: need 0 < min <= max, got scale {scale!r}, ratio {ratio!r}")
        return cls("random_resized", size, scale=(s0, s1), ratio=(r0, r1), seed=seed)

    @classmethod
    def window(cls, size=(256, 256), crop=(224, 224)):
        vh, vw = cls._pair("size", size)
        H, W = cls._pair("crop", crop)
        if H > vh or W > vw:
            raise ValueError(f"DeviceResizedCrop.window: a crop of {(H, W)} does not fit {(vh, vw)}")
        return cls("window", (H, W), resize=(vh, vw))

    @staticmethod
    def dtype():
        """The numpy record of struct calm_rcrop_sample."""
        import numpy as np
        from . import _lib
        return np.dtype(_lib.RCropSample)

    @classmethod
    def valid(cls, t, nbytes, H, W):
        """bool [B]: calm_resized_crop_check over a record array (the conditions of include/calm_vit.h, in 64-bit)."""
        import numpy as np
        f = {n: t[n].astype(np.int64) for n in t.dtype.names}
        ok = (f["h"] >= 1) & (f["h"] <= cls.MAX_SIDE) & (f["w"] >= 1) & (f["w"] <= cls.MAX_SIDE)
        ok &= (f["offset"] >= 0) & (f["offset"] <= nbytes)
        ok &= np.where(ok, 3 * f["h"] * f["w"] <= nbytes - np.where(ok, f["offset"], 0), False)
        ok &= (f["by0"] >= 0) & (f["bx0"] >= 0) & (f["bh"] >= 1) & (f["bw"] >= 1)
        ok &= (f["by0"] + f["bh"] <= f["h"]) & (f["bx0"] + f["bw"] <= f["w"])
        ok &= (f["vh"] >= 1) & (f["vh"] <= cls.MAX_SIDE) & (f["vw"] >= 1) & (f["vw"] <= cls.MAX_SIDE)
        ok &= (f["wy0"] >= 0) & (f["wx0"] >= 0) & (H >= 1) & (W >= 1) & (f["wy0"] + H <= f["vh"]) & (f["wx0"] + W <= f["vw"])
        return ok

    def _random_box(self, h, w):
        """RandomResizedCrop.get_params for one h x w image -> (top, left, box h, box w), whether the fallback was taken."""
        import math
        rng, area = self.rng, h * w
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target = area * float(rng.uniform(self.scale[0], self.scale[1]))
            aspect = math.exp(float(rng.uniform(log_ratio[0], log_ratio[1])))
            bw, bh = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < bw <= w and 0 < bh <= h:
                return (int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1)), bh, bw), False
        in_ratio = float(w) / float(h)                     # the central box, the ratio clamped to the range
        if in_ratio < self.ratio[0]:
            bw = w
            bh = int(round(bw / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            bh = h
            bw = int(round(bh * self.ratio[1]))
        else:
            bw, bh = w, h
        bh, bw = min(max(bh, 1), h), min(max(bw, 1), w)
        return ((h - bh) // 2, (w - bw) // 2, bh, bw), True

    def records(self, meta, nbytes, corners=None):
        """The host array of calm_rcrop_sample records for a meta table ([B, 3] of (offset, h, w)), checked against a
        buffer of nbytes bytes: what the kernel would answer with zeros is an error here.  .random_resized draws here."""
        import numpy as np
        off, h, w = _meta_columns("DeviceResizedCrop", meta, self.MAX_SIDE)
        B, (H, W) = len(off), self.size
        if (corners is not None) != (self.kind == "window"):
            raise ValueError("DeviceResizedCrop: corners ([B, 2] of (y0, x0)) are given to .window and to nothing else")
        t = np.zeros(B, dtype=self.dtype())
        t["offset"], t["h"], t["w"] = off, h, w
        t["bh"], t["bw"] = h, w                             # the whole image unless a box is drawn
        if self.kind == "center":
            tall = w <= h                                   # the short side goes to `resize`
            long_side = (self.resize * np.where(tall, h, w).astype(np.float64) / np.where(tall, w, h)).astype(np.int64)
            vh, vw = np.where(tall, long_side, self.resize), np.where(tall, self.resize, long_side)
            if (vh < H).any() or (vw < W).any() or (vh > self.MAX_SIDE).any() or (vw > self.MAX_SIDE).any():
                b = int(np.flatnonzero((vh < H) | (vw < W) | (vh > self.MAX_SIDE) | (vw > self.MAX_SIDE))[0])
                raise ValueError(f"DeviceResizedCrop.center: image {b} ({h[b]} x {w[b]}) resizes to {vh[b]} x {vw[b]}, "
                                 f"which does not hold the {H} x {W} crop or exceeds {self.MAX_SIDE}")
            t["vh"], t["vw"] = vh, vw
            t["wy0"] = [int(round((int(v) - H) / 2.0)) for v in vh]
            t["wx0"] = [int(round((int(v) - W) / 2.0)) for v in vw]
        elif self.kind == "random_resized":
            boxes = [self._random_box(int(hh), int(ww)) for hh, ww in zip(h, w)]
            t["by0"], t["bx0"], t["bh"], t["bw"] = (np.asarray(v) for v in zip(*(bx for bx, _ in boxes)))
            t["vh"], t["vw"] = H, W
            self.last_fallback = np.asarray([fb for _, fb in boxes], dtype=bool)
        else:
            c = np.asarray(corners.cpu() if isinstance(corners, torch.Tensor) else corners)
            if c.shape != (B, 2):
                raise ValueError(f"DeviceResizedCrop.window: corners must be [B, 2] (y0, x0), got shape {c.shape}")
            t["vh"], t["vw"] = self.resize
            cc = c.astype(np.int64)
            if (cc < 0).any() or (cc > np.iinfo(np.int32).max).any():
                raise ValueError("DeviceResizedCrop.window: a corner lies outside the resized image")
            t["wy0"], t["wx0"] = cc[:, 0], cc[:, 1]
        bad = ~self.valid(t, int(nbytes), H, W)
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            raise ValueError(f"DeviceResizedCrop: record {b} {t[b]} does not lie in the buffer, its image or its resized size")
        self.last_records = t
        return t

    def pack(self, meta, nbytes, corners=None, device="cuda"):
        """The device array of calm_rcrop_sample records, [B,48] uint8, in one host-to-device copy."""
        return _records_to_device(self.records(meta, nbytes, corners), device)

    def __call__(self, packed_dev, meta, corners=None, out="u8"):
        from .backend import get_backend
        if out not in self.OUTPUTS:
            raise ValueError(f"DeviceResizedCrop: out is one of {self.OUTPUTS}, got {out!r}")
        samples = self.pack(meta, packed_dev.numel(), corners, device=packed_dev.device)
        B, (H, W) = samples.shape[0], self.size
        if out == "u8":
            y = torch.empty((B, 3, H, W), dtype=torch.uint8, device=packed_dev.device)
            get_backend().resized_crop(packed_dev, samples, y)
        else:
            y = torch.empty((B, H, 3 * W) if out == "tokens" else (B, 3, H, W), dtype=torch.float32, device=packed_dev.device)
            get_backend().resized_crop(packed_dev, samples, y, self.MEAN, self.STD, tokens=out == "tokens")
        return y


def _map_tensors(out, fn):
    """fn over the tensors of a model output (a tensor, or a tuple / list of tensors and None)."""
    if isinstance(out, torch.Tensor):
        return fn(out)
    if isinstance(out, (tuple, list)):
        return type(out)(_map_tensors(o, fn) for o in out)
    return out


class Predictor:
    """Inference front of a model: `predictor(x)` returns what `model(x)` returns, computed in eval mode under
    torch.no_grad() with the lean forward (backend.set_lean_inference: the attention keeps nothing for a backward, the
    GELU GEMMs write no pre-activation) whatever the global switch says; the model's training flag and the switch are
    put back before the call returns.  The results equal the training forward's in eval mode bit for bit.

    graph=True (needs example_x) follows GraphedTrainStep: the forward is warmed up on a side stream, captured once into a
    hipGraph at example_x's shape and dtype and replayed, inputs copied into a static buffer — one graph launch instead
    of the host enqueueing every kernel.  The spectral-norm sigma products of eval mode and the bf16 weight copies are part
    of the captured region and read the parameters where they live, so an in-place update of the weights (an optimizer
    step, load_state_dict) is seen by the next replay.  A batch of any other shape or dtype (a ragged last batch) runs
    eagerly, lean.  Outputs of a replay are copies: they stay valid across later calls.  close() releases the graph.

    features=True: `predictor(x)` returns `model.features(x)` (ViT.features: the pooled backbone output [B, D]) instead of
    `model(x)`, lean / graph / autocast as above."""

    def __init__(self, model, example_x=None, autocast_dtype=None, graph=False, warmup=2, features=False):
        self.model = model
        self.autocast_dtype = autocast_dtype
        self.features = bool(features)
        self.graph = None
        self.x = self.out = None
        if graph:
            if example_x is None or not example_x.is_cuda:
                raise ValueError("Predictor(graph=True) needs a CUDA example_x to capture the forward at")
            self.x = example_x.detach().clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                 # warm-up on a side stream (allocator + lazy plans)
                for _ in range(max(int(warmup), 1)):
                    self._eager(self.x)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph_obj = torch.cuda.CUDAGraph()

            def capture(x):
                with torch.cuda.graph(graph_obj):
                    return self._forward(x)
            self.out = self._lean(capture, self.x)
            self.graph = graph_obj

    def _forward(self, x):
        with torch.autocast(device_type="cuda", dtype=self.autocast_dtype or torch.bfloat16,
                            enabled=self.autocast_dtype is not None and x.is_cuda):
            return self.model.features(x) if self.features else self.model(x)

    def _lean(self, fn, x):
        """fn(x) in eval mode, without grad, with the lean switch on; flag and switch restored."""
        from . import backend
        was_training, was_lean = self.model.training, backend.get_lean_inference()
        self.model.eval()
        backend.set_lean_inference(True)
        try:
            with torch.no_grad():
                return fn(x)
        finally:
            backend.set_lean_inference(was_lean)
            self.model.train(was_training)

    def _eager(self, x):
        return self._lean(self._forward, x)

    def __call__(self, x):
        if self.graph is None or x.shape != self.x.shape or x.dtype != self.x.dtype or x.device != self.x.device:
            return self._eager(x)
        self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        return _map_tensors(self.out, torch.clone)

    def close(self):
        """Release the captured graph and its static tensors; later calls run eagerly."""
        if self.graph is not None:
            self.graph.reset()
        self.graph = self.x = self.out = None


def evaluate(model, batches, lean=False, graph=False, autocast_dtype=None, transform=None, transform_out="tokens", ema=None,
             report=False, topk=(1, 5), confusion=False, process_group=None, recon=False):
    """Top-1 accuracy over (x, labels) batches in eval mode (CALM_ViT_V2.py:228-239).  With the loss kernels switched on
    the hits are counted on the device (calm_top1_count into a StepMetrics) and read once after the last batch instead of
    once per batch.  lean / graph: the forward goes through a Predictor (lean kernels; graph=True captures it at the first
    batch's shape and replays it, other shapes run eagerly) under autocast_dtype if one is given; without either flag the
    model is called as before.
    transform: a DeviceResizedCrop.center (DeviceResizedCrop.center(256, (224, 224)) is Resize(256) + CenterCrop(224) +
    Normalize).  `batches` then yield what a RaggedU8Collate returns, (packed, meta, labels) with the decoded images as
    they are, and x is the output of one launch on the model's device: the first Block's row tokens [B,H,3W]
    (transform_out="tokens", the form train(device_collate=True) feeds the model) or the image [B,3,H,W] ("image": for a
    model whose first layer is not this ViT's first Block, which alone takes row tokens — the kernel has both outputs and
    the caller has to be able to choose).
    ema: a ModelEMA of `model`.  The whole loop runs inside `ema.applied()`: the averages are exchanged into the parameters
    in place (every cached address and captured graph stays valid) and exchanged back when the loop ends or raises.
    report=True: instead of the top-1 float the call returns the dict of `EvalMetrics.read()` — n, skipped, nonfinite,
    loss (mean cross-entropy), top<k> for every k of `topk`, per_class_accuracy, mean_per_class_accuracy and, with
    confusion=True, the confusion matrix — over integer labels [B].  Every batch is one `EvalMetrics.update` (one library
    call without a host synchronisation where the loss kernels serve the logits), and the tallies are summed over
    `process_group`, or over the default group when torch.distributed is initialised, before the one read: every rank
    evaluates its own `validation_shard` and every rank returns the report of the whole set.  At least one batch is
    needed (the class count comes from the logits).  report=False (the default) is the loop as it was.
    recon=True (a `generate=True` model; excludes report=True): `batches` yield x or (x, _), x the image [B,3,S,S] or the row
    tokens [B,S,3S]; the model's tokens are measured against x by a `ReconMetrics` (DeviceCollate's mean / std, delta 1,
    SSIM where S >= 11) — one library call per batch where the loss kernels serve the tensors — with the same lean /
    graph / ema / transform / process_group handling, and the call returns `ReconMetrics.read()` of the whole set."""
    if recon and report:
        raise ValueError("evaluate: recon=True and report=True exclude each other (one model is not both kinds)")
    if ema is not None:
        if ema.model is not model:
            raise ValueError("evaluate: ema= must be the ModelEMA of the model being evaluated")
        with ema.applied():
            return evaluate(model, batches, lean=lean, graph=graph, autocast_dtype=autocast_dtype, transform=transform,
                            transform_out=transform_out, report=report, topk=topk, confusion=confusion,
                            process_group=process_group, recon=recon)
    from . import backend
    if transform is not None:
        if not isinstance(transform, DeviceResizedCrop):
            raise TypeError(f"evaluate: transform must be a DeviceResizedCrop, got {type(transform).__name__}")
        if transform.kind != "center":                      # no random crops in an evaluation; .window needs corners per call
            raise ValueError("evaluate: transform takes a DeviceResizedCrop.center(...), the deterministic validation transform")
        if transform_out not in ("tokens", "image"):
            raise ValueError(f'evaluate: transform_out is "tokens" or "image", got {transform_out!r}')
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise ValueError("evaluate: transform= runs a HIP kernel, the model must be on a GPU")

        def _transformed(src):
            for packed, meta, labels in src:
                yield transform(packed.to(device, non_blocking=True), meta, out=transform_out), labels.to(device)
        batches = _transformed(batches)
    was_training = model.training
    model.eval()
    correct = total = 0
    metrics = None
    predictor = None
    tallies = None
    with torch.no_grad():
        for batch in batches:
            x, labels = batch if isinstance(batch, (tuple, list)) else (batch, None)
            if lean or graph:
                if predictor is None:
                    predictor = Predictor(model, example_x=x if graph else None, autocast_dtype=autocast_dtype, graph=graph)
                y_hat, _ = predictor(x)
            else:
                y_hat, _ = model(x)
            if recon:
                S = x.shape[1] if x.dim() == 3 else x.shape[-1]
                if tallies is None:
                    tallies = ReconMetrics(DeviceCollate.MEAN, DeviceCollate.STD, ssim=S >= RECON_WINDOW, device=y_hat.device)
                tallies.update(y_hat.reshape(x.shape[0], S, 3 * S), x)
                continue
            logits = y_hat.reshape(x.shape[0], -1)
            if report:
                if tallies is None:
                    tallies = EvalMetrics(logits.shape[1], topk=topk, confusion=confusion, device=logits.device)
                tallies.update(logits, labels.to(logits.device))
                continue
            if backend.get_loss_kernels() and labels.dim() == 1 and backend.loss_kernels_take(logits):
                if metrics is None:
                    metrics = StepMetrics(logits.device)
                logits = logits if logits.stride(-1) == 1 else logits.contiguous()
                backend.get_backend().top1_count(logits, labels.to(logits.device, torch.int64).contiguous(), metrics.buf,
                                                 logits.shape[0], logits.shape[1])
                continue
            correct += int((logits.argmax(dim=1) == labels).sum())
            total += int(labels.numel())
    if metrics is not None:
        _, hits, rows, _ = metrics.read()
        correct, total = correct + hits, total + rows
    if predictor is not None:
        predictor.close()
    model.train(was_training)
    if report or recon:
        if tallies is None:
            raise ValueError(f"evaluate: {'report' if report else 'recon'}=True needs at least one batch")
        if process_group is not None or (dist.is_available() and dist.is_initialized()):
            tallies.all_reduce(process_group)
        return tallies.read()
    return correct / max(total, 1)


def knn_evaluate(model, bank_batches, query_batches, num_classes, k=20, temperature=0.07, topk=(1, 5), lean=True, graph=False,
                 autocast_dtype=None, transform=None, transform_out="tokens", ema=None, process_group=None, features=None,
                 confusion=False):
    """Weighted k-NN accuracy of the model's frozen features (`KnnProbe`): every rank embeds its bank shard (batches of
    (x, int64 labels)), the shards are gathered into dataset order (`KnnProbe.gather_bank`: rank r holds items r, r + world,
    ..., what `validation_shard` hands out), every rank embeds and queries its query shard, the tallies are summed over
    `process_group` — or the default group when torch.distributed is initialised — and every rank returns
    `KnnProbe.read()` of the whole set.  The feature is `model.features(x)` (ViT.features: the pooled backbone output)
    through a `Predictor(features=True)` — lean kernels; graph=True captures the forward at the first batch's shape and
    replays it, other shapes run eagerly — or, with lean=False and graph=False, the plain call in eval mode.
    features: a callable x -> [B, D] that replaces the model forward (a head of the caller's own).  transform,
    transform_out and ema are `evaluate`'s.  The training flag and the lean switch are as before when the call returns
    or raises."""
    if ema is not None:
        if ema.model is not model:
            raise ValueError("knn_evaluate: ema= must be the ModelEMA of the model being evaluated")
        with ema.applied():
            return knn_evaluate(model, bank_batches, query_batches, num_classes, k=k, temperature=temperature, topk=topk,
                                lean=lean, graph=graph, autocast_dtype=autocast_dtype, transform=transform,
                                transform_out=transform_out, process_group=process_group, features=features,
                                confusion=confusion)
    if features is not None and not callable(features):
        raise TypeError(f"knn_evaluate: features is a callable x -> [B, D], got {type(features).__name__}")
    KnnProbe(num_classes, k=k, temperature=temperature, topk=topk)     # (a bad setting is refused before any forward)
    if transform is not None:
        if not isinstance(transform, DeviceResizedCrop):
            raise TypeError(f"knn_evaluate: transform must be a DeviceResizedCrop, got {type(transform).__name__}")
        if transform.kind != "center":
            raise ValueError("knn_evaluate: transform takes a DeviceResizedCrop.center(...), the deterministic validation transform")
        if transform_out not in ("tokens", "image"):
            raise ValueError(f'knn_evaluate: transform_out is "tokens" or "image", got {transform_out!r}')
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise ValueError("knn_evaluate: transform= runs a HIP kernel, the model must be on a GPU")

        def _transformed(src):
            for packed, meta, labels in src:
                yield transform(packed.to(device, non_blocking=True), meta, out=transform_out), labels.to(device)
        bank_batches, query_batches = _transformed(bank_batches), _transformed(query_batches)
    was_training = model.training
    model.eval()
    predictor = probe = None
    try:
        with torch.no_grad():
            def embed(x):
                nonlocal predictor
                if features is not None:
                    return features(x)
                if lean or graph:
                    if predictor is None:
                        predictor = Predictor(model, example_x=x if graph else None, autocast_dtype=autocast_dtype, graph=graph,
                                              features=True)
                    return predictor(x)
                with torch.autocast(device_type="cuda", dtype=autocast_dtype or torch.bfloat16,
                                    enabled=autocast_dtype is not None and x.is_cuda):
                    return model.features(x)

            for x, labels in bank_batches:
                f = embed(x)
                if probe is None:
                    probe = KnnProbe(num_classes, k=k, temperature=temperature, topk=topk, confusion=confusion, device=f.device)
                probe.add_bank(f, labels.to(f.device, torch.int64))
            if probe is None:
                raise ValueError("knn_evaluate: the bank needs at least one batch on every rank")
            distributed = process_group is not None or (dist.is_available() and dist.is_initialized())
            if distributed:
                probe.gather_bank(process_group)
            for x, labels in query_batches:
                f = embed(x)
                probe.query(f, labels.to(f.device, torch.int64))
            if distributed:
                probe.all_reduce(process_group)
            return probe.read()
    finally:
        if predictor is not None:
            predictor.close()
        model.train(was_training)


def validation_shard(dataset, rank, world):
    """The samples rank, rank + world, ... of `dataset`, WITHOUT padding: DistributedSampler fills the shards up with
    repeated samples, which a validation pass would count twice.  The shards of all ranks cover every index exactly once,
    so the `n` of an all-reduced report equals len(dataset)."""
    if not 0 <= rank < world:
        raise ValueError(f"validation_shard: rank {rank} is outside a world of {world}")
    return torch.utils.data.Subset(dataset, range(rank, len(dataset), world))


def save_samples(imgs, out_dir, prefix="sample_"):
    """CALM_ViT_V2.py:113-118: sigmoid of the generated images [B,3,H,W], one 8-bit RGB PNG per image
    (`<out_dir>/sample_<i>.png`).  Returns the paths.  The PNG is written with zlib only (no plotting dependency)."""
    import struct
    import zlib
    os.makedirs(out_dir, exist_ok=True)
    x = torch.sigmoid(imgs.detach().float()).permute(0, 2, 3, 1)            # HWC, as the reference hands to imsave
    u8 = (x * 255.0).round().clamp_(0, 255).to(torch.uint8).cpu().numpy()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    paths = []
    for i, img in enumerate(u8):
        h, w, _ = img.shape
        raw = b"".join(b"\x00" + img[r].tobytes() for r in range(h))         # filter type 0 per scanline
        png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
               + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
        path = os.path.join(out_dir, f"{prefix}{i}.png")
        with open(path, "wb") as f:
            f.write(png)
        paths.append(path)
    return paths


def make_optimizer(model, lr=3.1e-3, weight_decay=0.02, betas=(0.9, 0.98), capturable=False, groups=None):
    """optim.AdamW(model.parameters(), lr=3.1e-3, weight_decay=0.02, betas=(0.9, 0.98)) (cls:146,158).
    groups: the parameter groups FusedClipAdamW(groups=) takes (e.g. from `param_groups`), laid out the same way — the
    base group first — so that a torch run and a fused run share them."""
    params = [p for p in model.parameters() if p.requires_grad]
    fused = params[0].is_cuda
    if groups is not None:
        params = _optimizer_groups(model, params, groups, lr, weight_decay)[0]
    return torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay, betas=betas, fused=fused,
                             capturable=capturable and fused)


def _optimizer_groups(model, params, groups, lr, weight_decay):
    """torch-style `groups` ({"params": [...], "lr": ..., "weight_decay": ...}, optionally "names") over `params` (the
    trainable parameters of `model`, in model order) -> (param groups, group index per parameter of `params`).  Group 0
    is the base group — every parameter no group names, with `lr` / `weight_decay`; it may be empty."""
    index = {id(p): i for i, p in enumerate(params)}
    owned = {id(p) for p in model.parameters()}
    group_of = [0] * len(params)
    taken = set()
    out = [{"params": [], "lr": lr, "weight_decay": weight_decay}]
    for k, g in enumerate(groups, start=1):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError(f'parameter group {k}: a dict with "params" (and "lr" / "weight_decay") is expected')
        extra = set(g) - {"params", "lr", "weight_decay", "names"}
        if extra & {"betas", "eps"}:
            raise ValueError(f"parameter group {k} sets {sorted(extra & {'betas', 'eps'})}: betas and eps are shared by all "
                             "groups (one hyper-parameter block per optimizer step)")
        if extra:
            raise ValueError(f"parameter group {k}: unknown keys {sorted(extra)}")
        glr, gwd = float(g.get("lr", lr)), float(g.get("weight_decay", weight_decay))
        if not glr >= 0.0:
            raise ValueError(f"parameter group {k}: negative learning rate {glr!r}")
        members = [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])
        for p in members:
            if id(p) not in owned:
                raise ValueError(f"parameter group {k} holds a tensor that is not a parameter of the model")
            if not p.requires_grad:
                raise ValueError(f"parameter group {k} holds a parameter with requires_grad=False (leave frozen "
                                 "parameters out of every group)")
            if id(p) in taken:
                raise ValueError(f"parameter group {k} holds a parameter that is in another group (or twice in this one)")
            taken.add(id(p))
            group_of[index[id(p)]] = k
        d = {"params": members, "lr": glr, "weight_decay": gwd}
        if "names" in g:
            d["names"] = list(g["names"])
        out.append(d)
    out[0]["params"] = [p for p in params if id(p) not in taken]
    return out, group_of


def param_groups(model, rules, lr=3.1e-3, weight_decay=0.02):
    """Parameter groups from name rules -> (groups, frozen_params), for FusedClipAdamW(groups=) / make_optimizer(groups=).

    rules: an ordered list of (pattern, options).  pattern: an `fnmatch` pattern on the `named_parameters()` name, or a
    callable (name, param) -> bool; the FIRST rule that matches a parameter decides, a parameter no rule matches goes to
    the base group (the optimizer's own lr / weight_decay; it is not listed here).  options: a subset of "lr",
    "lr_scale" (times the base `lr`; not together with "lr"), "weight_decay", "frozen" (True: the parameter is returned in
    frozen_params and is in no group — the caller sets requires_grad_(False) before building the optimizer).  Rules that
    end at the same (lr, weight_decay) share one group, so there are as many groups as distinct pairs (a pair equal to
    the base one stays in the base group); every group lists its "names" beside its "params".  A rule that matches no
    parameter is an error.  The preset rules="no_decay": weight_decay = 0 for every parameter with ndim <= 1 — biases,
    LayerNorm weight / bias, ls_att / ls_mlp, the RoPE inv_freq; a spectral-normed `weight_orig` is 2-d and keeps its
    decay."""
    import fnmatch
    if isinstance(rules, str):
        if rules != "no_decay":
            raise ValueError(f'param_groups: the only preset is "no_decay", got {rules!r}')
        rules = [(lambda name, p: p.ndim <= 1, {"weight_decay": 0.0})]
    rules = list(rules)
    for k, (pattern, options) in enumerate(rules):
        if not (callable(pattern) or isinstance(pattern, str)):
            raise ValueError(f"param_groups: rule {k}: the pattern is an fnmatch string or a callable (name, param) -> bool")
        if not set(options) <= {"lr", "lr_scale", "weight_decay", "frozen"}:
            raise ValueError(f'param_groups: rule {k} takes "lr", "lr_scale", "weight_decay", "frozen", got {sorted(options)}')
        if "lr" in options and "lr_scale" in options:
            raise ValueError(f'param_groups: rule {k} sets both "lr" and "lr_scale"')
    hits = [0] * len(rules)
    by_pair, frozen = {}, []
    for name, p in model.named_parameters():
        for k, (pattern, options) in enumerate(rules):
            if pattern(name, p) if callable(pattern) else fnmatch.fnmatchcase(name, pattern):
                break
        else:
            continue
        hits[k] += 1
        if options.get("frozen"):
            frozen.append(p)
            continue
        if not p.requires_grad:
            continue
        glr = float(options["lr"]) if "lr" in options else lr * float(options.get("lr_scale", 1.0))
        pair = (glr, float(options.get("weight_decay", weight_decay)))
        if pair == (lr, weight_decay):
            continue
        g = by_pair.setdefault(pair, {"params": [], "names": [], "lr": pair[0], "weight_decay": pair[1]})
        g["params"].append(p)
        g["names"].append(name)
    for k, n in enumerate(hits):
        if n == 0:
            raise ValueError(f"param_groups: rule {k} ({rules[k][0]!r}) matches no parameter of the model")
    return list(by_pair.values()), frozen


_build_param_groups = param_groups              # (train() has an argument of that name)


def _clear_deferred(refs, attr, token):
    """Remove the deferral mark from the parameters that still carry THIS optimizer's token: a mark re-set by a newer
    optimizer on the same model is not the dropped one's to clear (its finalizer may run long after the new one exists)."""
    for r in refs:
        p = r()
        if p is not None and getattr(p, attr, None) == token:
            delattr(p, attr)


def _stale_ptrs(tensors, ptrs):
    """A plan caches raw addresses: has any of `tensors` left the address recorded for it in `ptrs` (uint64 array)?"""
    import numpy as np
    now = np.fromiter((t.data_ptr() for t in tensors), dtype=np.uint64, count=len(tensors))
    return not np.array_equal(now, ptrs)


class FusedClipAdamW(torch.optim.Optimizer):
    """unscale + inf/NaN check + clip_grad_norm_(max_norm) + AdamW + zero_grad of distributed_trainer_cls.py:88-96 as
    THREE kernel launches over all parameters (calm_optim_step), with the spectral-norm weight-gradient correction
    folded in: while an instance is live, the backward of every spectral-normed layer that is not combined with a
    LayerScale leaves the gradient w.r.t. the normalised weight in `weight_orig.grad` (≈600 tiny launches per step
    less) and this step applies dW_orig = (G - <G, W/sigma> u v^T)/sigma on the fly — so between backward and step()
    those `.grad`s are NOT the reference's gradients; mean all-reduce commutes with the correction (it is linear and
    u, v, sigma, W are replicated), so the BucketedGradReducer / DDP run unchanged in between.  close() restores the
    in-backward correction.  Same update rule, hyper-parameters and state names as torch.optim.AdamW.

    It IS a torch.optim.Optimizer: `CosineAnnealingLR(optimizer, T_max=epochs, eta_min=1e-6)` of the reference's
    train() (cls:52,108-109) wraps it, and the learning rate a step uses is `param_groups[0]["lr"]`.

    groups=None (the reference's own call): one param group, calm_optim_step.  groups=[{"params": [...], "lr": ...,
    "weight_decay": ...}, ...] (torch's form; `param_groups()` builds them from name rules): the parameters no group
    names form the base group with the constructor's lr / weight_decay — group 0, first in `param_groups`, possibly
    empty; betas and eps are shared.  With more than one group the step is calm_optim_step_groups: the same three
    launches, the norm / clip / inf check / step count over ALL parameters, and pass 3 reading every tensor's
    `param_groups[g]["lr"]` / `["weight_decay"]` from a device table that is rewritten only when a value changed — so a
    torch scheduler drives every group, also through a captured step.  `params`, `exp_avg`, `exp_avg_sq` keep the order of
    model.parameters() whatever the grouping.  Refused: a group that sets betas or eps, a parameter in two groups, one
    that is not the model's or has requires_grad=False, a negative lr.

    `monitor`: None, or the attached `GradMonitor` (`GradMonitor.attach()`), whose `observe()` every step — eager,
    windowed or captured — calls on the step's gradients in front of the update.

    `perturbed_by`: None, or the `SharpnessAware` whose perturbation the parameters carry right now: until its restore()
    it stands in front of step() and refuses it (an attribute of the INSTANCE that perturb() sets and restore() removes,
    so step() itself has no branch for it).

    lamb=None | True | {"trust_clip": None, "always_adapt": False}: the step is LAMB (calm_optim_step_lamb, four launches):
    the same unscale / inf check / clip / moments, and every tensor's update u = Adam direction + weight_decay * w applied
    as w -= lr * trust * u with trust = ||w|| / ||u|| per tensor — 1 for a tensor without weight decay unless always_adapt
    (timm's rule), 1 where either norm is 0, at most trust_clip.  One entry point serves one and several param groups.  The
    state is AdamW's (`exp_avg`, `exp_avg_sq`, the step count), so snapshots and the accumulation window are unchanged;
    `trust_ratios()` reads what the last applied step used.  `lamb` holds the normalised settings, or None."""

    monitor = None
    perturbed_by = None

    def __init__(self, model, lr=3.1e-3, weight_decay=0.02, betas=(0.9, 0.98), eps=1e-8, max_norm=1.0, defer_sn=True,
                 groups=None, lamb=None):
        from . import ops
        from .backend import get_backend
        from .spectral_norm import SpectralWeight
        self.be = get_backend()
        self.max_norm = max_norm
        self.lamb = _lamb_settings("FusedClipAdamW", lamb)
        params = [p for p in model.parameters() if p.requires_grad]
        names = {id(p): n for n, p in model.named_parameters()}
        self.param_names = [names[id(p)] for p in params]
        group_of = [0] * len(params)
        if groups is None:
            super().__init__(params, dict(lr=lr, weight_decay=weight_decay, betas=tuple(betas), eps=eps))
        else:
            pg, group_of = _optimizer_groups(model, params, groups, lr, weight_decay)
            super().__init__(pg, dict(lr=lr, weight_decay=weight_decay, betas=tuple(betas), eps=eps))
        self.params = params
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        sn = {}
        if defer_sn:
            for m in model.modules():
                if isinstance(m, SpectralWeight) and not getattr(m, "layer_scaled", False):
                    sn[id(m.weight_orig)] = m
        self._records, self._deferred, self._sn_tensors = [], [], []
        for p, ea, eas, grp in zip(self.params, self.exp_avg, self.exp_avg_sq, group_of):
            m = sn.get(id(p))
            info = None
            if m is not None:
                info = (m.weight_u, m.weight_v, m._sigma, m.rows, m.cols)
                self._deferred.append(p)
                self._sn_tensors.append((m, m.weight_u.data_ptr(), m.weight_v.data_ptr(), m._sigma.data_ptr()))
            self._records.append({"param": p.data, "exp_avg": ea, "exp_avg_sq": eas, "sn": info})
            if self.grouped:
                self._records[-1]["group"] = grp
        self._plan = self._make_plan(self._records)
        # the deferral is a mark on the PARAMETER OBJECT (ops reads it in forward), not a set of raw addresses: it
        # survives a re-materialised buffer and cannot be inherited by an unrelated tensor at a recycled address
        # The mark carries its owner: a second optimizer built over the same model takes the marks over, and the first
        # one's finalizer (or close()) then leaves them alone — clearing them would make backward correct the gradient
        # AND this step correct it again.
        self._token = id(self)
        self._defer_attr = ops.DEFER_ATTR
        for p in self._deferred:
            setattr(p, ops.DEFER_ATTR, self._token)
        # an optimizer that is dropped without close() must not leave its layers deferred (their backward would hand
        # out un-corrected gradients with nobody left to correct them)
        self._finalizer = weakref.finalize(self, _clear_deferred, [weakref.ref(p) for p in self._deferred], ops.DEFER_ATTR,
                                           self._token)
        self.stats = torch.zeros(2, dtype=torch.float32, device=self.params[0].device)   # [grad norm, found_inf]
        # (with parameter groups the rates always live on the device, in the plan's group table)
        # learning rate as a device scalar for captured steps (GraphedTrainStep sets lr_on_device and refreshes it from
        # param_groups[0]["lr"] before a replay whenever a scheduler has changed it); eager steps pass the host value
        self.lr_on_device = False
        self._lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=self.params[0].device)
        self._lr_dev_value = float(lr)
        # LAMB without the entry point (CPU parameters): the (wn, un, trust) table lamb_step_torch writes
        self._trust_host = None
        if self.lamb is not None and not hasattr(self.be, "optim_step_lamb"):
            self._trust_host = torch.zeros(len(self.params), 3, dtype=torch.float32)
            self._trust_host[:, 2] = 1.0
        if self.lamb is not None:
            # (through a weak reference: a bound method stored on its own instance would be a cycle, and the finalizer
            # above is to run when the last outside reference goes)
            me = weakref.ref(self)
            self._launch = lambda *a, **kw: FusedClipAdamW._launch_lamb(me(), *a, **kw)

    @property
    def grouped(self):
        """More than one param group: the step goes through calm_optim_step_groups."""
        return len(self.param_groups) > 1

    def _make_plan(self, records):
        if self.grouped and hasattr(self.be, "optim_step_groups"):
            return self.be.optim_plan(records, n_groups=len(self.param_groups))
        return self.be.optim_plan(records)

    def group_hparams(self):
        """[(lr, weight_decay)] of every param group as they are now (what the next step uses)."""
        return [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups]

    def sync_lr_to_device(self):
        """Write param_groups[0]["lr"] to the device scalar a captured step reads (no-op when unchanged); with parameter
        groups, the whole (lr, weight_decay) table when any value changed."""
        if self.grouped:
            if hasattr(self.be, "optim_step_groups"):
                self._plan.groups.set(self.group_hparams())
            return
        lr = float(self.lr)
        if lr != self._lr_dev_value:
            self._lr_dev.fill_(lr)
            self._lr_dev_value = lr

    @property
    def step_count(self):
        """Completed (un-skipped) optimizer steps: the counter lives on the device and does not advance when an
        inf/NaN gradient skips the update — torch.optim.AdamW under a GradScaler.  Reading it synchronises."""
        return int(self._plan.step_dev.item())

    # the hyper-parameters live in the param groups, where LR schedulers read and write them (these: group 0's)
    lr = property(lambda self: self.param_groups[0]["lr"], lambda self, v: self.param_groups[0].__setitem__("lr", v))
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"])
    betas = property(lambda self: self.param_groups[0]["betas"])
    eps = property(lambda self: self.param_groups[0]["eps"])

    def close(self):
        self._finalizer()
        self._deferred = []

    def _check_plan(self):
        """The plan caches raw addresses: refuse to update orphaned storage after the model was moved / re-materialised
        (model.to(...), .float(), a replaced buffer) once the optimizer exists."""
        ok = not _stale_ptrs(self.params, self._plan.param_ptrs)
        for m, pu, pv, ps in self._sn_tensors:
            ok = ok and m.weight_u.data_ptr() == pu and m.weight_v.data_ptr() == pv and m._sigma.data_ptr() == ps
        if not ok:
            raise RuntimeError("FusedClipAdamW: parameters or spectral-norm buffers were moved or replaced after the "
                               "optimizer was built (model.to / .float / load with assign=True); build the optimizer "
                               "after the model is on its final device")

    def _check_owner(self):
        self._check_plan()
        for p in self._deferred:
            if getattr(p, self._defer_attr, None) != self._token:
                raise RuntimeError("FusedClipAdamW: another optimizer took over (or cleared) the deferred spectral-norm "
                                   "correction of this model; only the newest optimizer of a model may step")

    def _contiguous_grads(self, keep):
        """The `.grad` of every parameter, contiguous, zeros where there is none; keep: a gradient made here becomes the
        parameter's `.grad`."""
        grads = []
        for p in self.params:
            g = p.grad
            if g is None or not g.is_contiguous():
                g = torch.zeros_like(p) if g is None else g.contiguous()
                if keep:
                    p.grad = g
            grads.append(g)
        return grads

    def _hparams(self):
        """(lr, beta1, beta2, eps, weight_decay, max_norm, step) as the backend's optimizer-side entry points take them."""
        return (float(self.lr), self.betas[0], self.betas[1], self.eps, self.weight_decay, self.max_norm or 0.0, 0)

    def _launch(self, plan, grads, divisor, records=None):
        """calm_optim_step (calm_optim_step_groups with more than one param group) over `plan` — whose records are
        `records`, default the deferred plan's — with `grads` divided by `divisor` (a device scalar, or None); every
        `.grad` is released afterwards.  Returns the stats tensor."""
        hp = self._hparams()
        if self.monitor is not None:            # a GradMonitor: this step's gradients, in front of the step
            self.monitor.observe(plan, grads, divisor, self._records if records is None else records)
        if self.grouped:
            if hasattr(self.be, "optim_step_groups"):
                self.be.optim_step_groups(plan, grads, hp, self.group_hparams(), divisor, self.stats)
            else:                               # a backend without the entry point (CPU parameters)
                optim_step_groups_torch(self._records if records is None else records, plan.step_dev, grads, hp,
                                        self.group_hparams(), divisor, self.stats)
            for p in self.params:
                p.grad = None
            return self.stats
        if self.lr_on_device and not torch.cuda.is_current_stream_capturing():
            self.sync_lr_to_device()
        self.be.optim_step(plan, grads, hp, divisor, self.stats, lr_dev=self._lr_dev if self.lr_on_device else None)
        for p in self.params:
            p.grad = None
        return self.stats

    def _launch_lamb(self, plan, grads, divisor, records=None):
        """_launch of an optimizer built with lamb=: calm_optim_step_lamb, one entry point for one and for several param
        groups.  __init__ puts it in front of `_launch` as an attribute of the INSTANCE, so `_launch` has no branch for it
        and FusedClipAdamWindow, whose window steps through `self._launch`, steps with LAMB too."""
        hp = self._hparams()
        if self.monitor is not None:            # a GradMonitor: this step's gradients, in front of the step
            self.monitor.observe(plan, grads, divisor, self._records if records is None else records)
        group_hp = self.group_hparams() if self.grouped else None
        lamb_hp = (self.lamb["trust_clip"], self.lamb["always_adapt"])
        if self._trust_host is None:
            on_dev = self.lr_on_device and not self.grouped
            if on_dev and not torch.cuda.is_current_stream_capturing():
                self.sync_lr_to_device()
            self.be.optim_step_lamb(plan, grads, hp, lamb_hp, divisor, self.stats, group_hp=group_hp,
                                    lr_dev=self._lr_dev if on_dev else None)
        else:                                   # a backend without the entry point (CPU parameters)
            lamb_step_torch(self._records if records is None else records, plan.step_dev, grads, hp, lamb_hp, group_hp,
                            divisor, self.stats, self._trust_host)
        for p in self.params:
            p.grad = None
        return self.stats

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """One optimizer-side step on the current `.grad`s; grads are released (set to None) afterwards.
        grad_scale: device scalar the loss was multiplied by (GradScaler), or None.  Returns the stats tensor."""
        if closure is not None:
            raise NotImplementedError("FusedClipAdamW.step takes no closure")
        self._check_owner()
        return self._launch(self._plan, self._contiguous_grads(keep=True), grad_scale)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def state_dict(self):
        hparams = dict(lr=self.lr, weight_decay=self.weight_decay, betas=self.betas, eps=self.eps, max_norm=self.max_norm)
        if self.grouped:
            hparams["groups"] = [list(pair) for pair in self.group_hparams()]
        if self.lamb is not None:
            hparams["lamb"] = dict(self.lamb)
        return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "hparams": hparams}

    def load_state_dict(self, sd):
        if "hparams" in sd:
            if (sd["hparams"].get("lamb") is not None) != (self.lamb is not None):
                raise ValueError(f"FusedClipAdamW.load_state_dict: the state was written with{'' if sd['hparams'].get('lamb') else 'out'} "
                                 f"LAMB, this optimizer steps with{'' if self.lamb else 'out'} it")
            saved = sd["hparams"].get("groups")
            if (len(saved) if saved is not None else 1) != len(self.param_groups):
                raise ValueError(f"FusedClipAdamW.load_state_dict: the state holds {len(saved) if saved is not None else 1} "
                                 f"parameter group(s), this optimizer has {len(self.param_groups)}")
            self.lr = sd["hparams"]["lr"]
            if saved is not None:
                for g, (glr, gwd) in zip(self.param_groups, saved):
                    g["lr"], g["weight_decay"] = glr, gwd
        self._plan.step_dev.fill_(int(sd["step"]))
        for dst, src in zip(self.exp_avg, sd["exp_avg"]):
            dst.copy_(src)
        for dst, src in zip(self.exp_avg_sq, sd["exp_avg_sq"]):
            dst.copy_(src)

    def trust_ratios(self):
        """{parameter name: (w_norm, update_norm, trust)} of the last applied LAMB step, from one read of the table (it
        synchronises); (0, 0, 1) for every tensor before the first one.  A skipped step leaves the table as it was."""
        if self.lamb is None:
            raise RuntimeError("FusedClipAdamW.trust_ratios: the optimizer was built without lamb=")
        table = self._trust_host if self._trust_host is not None else self._plan.lamb_buffers(self.be)[1]
        rows = table.detach().cpu().tolist()
        return {n: (r[0], r[1], r[2]) for n, r in zip(self.param_names, rows)}


def _lamb_settings(who, lamb):
    """lamb= of FusedClipAdamW / train() -> None, or {"trust_clip": None | float > 0, "always_adapt": bool}."""
    if lamb is None or lamb is False:
        return None
    if lamb is True:
        lamb = {}
    if not isinstance(lamb, dict):
        raise ValueError(f'{who}: lamb is None, True or a dict with "trust_clip" / "always_adapt", got {lamb!r}')
    if not set(lamb) <= {"trust_clip", "always_adapt"}:
        raise ValueError(f'{who}: lamb takes the keys "trust_clip", "always_adapt", got {sorted(lamb)}')
    clip, always = lamb.get("trust_clip"), lamb.get("always_adapt", False)
    if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, float)) or not (clip > 0.0 and math.isfinite(clip))):
        raise ValueError(f'{who}: lamb["trust_clip"] is None or a positive finite limit, got {clip!r}')
    if not isinstance(always, (bool, int)) or always not in (0, 1):
        raise ValueError(f'{who}: lamb["always_adapt"] is a flag, got {always!r}')
    return {"trust_clip": None if clip is None else float(clip), "always_adapt": bool(always)}


def lamb_step_torch(records, step_dev, grads, hp, lamb_hp, group_hp, grad_scale, stats_out, trust_out=None):
    """calm_optim_step_lamb in torch, for a backend without `optim_step_lamb` (CPU parameters), in the header's fp32 order:
    the correction, the norm / clip / inf check and the step count of optim_step_groups_torch; then per record, with
    (lr_t, wd_t) = group_hp[record["group"]] (group_hp None: hp's), m = m + (g' - m)(1 - b1), v = v b2 + g'^2 (1 - b2),
    r = (m / (sqrt(v) / sqrt(bc2) + eps)) / bc1, u = r + wd_t w, trust = ||w|| / ||u|| where the tensor adapts and both norms
    are positive, else 1, at most trust_clip, and w -= (lr_t trust) u unless lr_t == 0.  lamb_hp = (trust_clip or None,
    always_adapt); trust_out: None or float32 [n, 3] <- (wn, un, trust).  A skipped step writes nothing."""
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))        # the ABI's hyper-parameters are fp32  # noqa: E731
    lr0, b1, b2, eps, wd0, max_norm, _ = (f32(x) for x in hp)
    clip, always = f32(lamb_hp[0] or 0.0), bool(lamb_hp[1])
    group_hp = None if group_hp is None else [(f32(lr), f32(wd)) for lr, wd in group_hp]
    fixed = []
    for r, g in zip(records, grads):
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            G = g.reshape(rows, cols)
            c = (G * r["param"].reshape(rows, cols)).sum() / sigma
            g = ((G - (c * u)[:, None] * v[None, :]) * (1.0 / sigma)).reshape(g.shape)
        fixed.append(g)
    inv = 1.0 / float(grad_scale) if grad_scale is not None else 1.0
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in fixed)).float() * inv
    bad = not bool(torch.isfinite(norm))
    stats_out[0], stats_out[1] = norm, float(bad)
    if bad:
        return
    step_dev += 1
    step = int(step_dev)
    mul = (min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0) * inv
    bc1, isb2 = 1 - b1 ** step, 1.0 / math.sqrt(1 - b2 ** step)
    for k, (r, g) in enumerate(zip(records, fixed)):
        lr, wd = (lr0, wd0) if group_hp is None else group_hp[r.get("group", 0)]
        g = g * mul
        p, m, v = r["param"], r["exp_avg"], r["exp_avg_sq"]
        m.copy_(m + (g - m) * (1 - b1))
        v.copy_(v * b2 + g * g * (1 - b2))
        u = (m / (v.sqrt() * isb2 + eps)) / bc1 + wd * p
        wn, un = (p * p).sum().sqrt(), (u * u).sum().sqrt()
        trust = wn / un if (always or wd != 0.0) and bool(wn > 0) and bool(un > 0) else torch.ones(())
        if clip > 0:
            trust = trust.clamp(max=clip)
        if trust_out is not None:
            trust_out[k, 0], trust_out[k, 1], trust_out[k, 2] = wn, un, trust
        if lr != 0.0:
            p.sub_((torch.tensor(lr, dtype=torch.float32) * trust) * u)


def optim_step_groups_torch(records, step_dev, grads, hp, group_hp, grad_scale, stats_out):
    """calm_optim_step_groups in torch, for a backend without `optim_step_groups` (CPU parameters): the deferred
    spectral-norm correction of a record with `sn`, the norm / clip / inf check over ALL records, then torch.optim.AdamW's
    update of every record with the (lr, weight_decay) of `group_hp[record["group"]]`.  hp as for optim_step (its lr and
    weight_decay are ignored); step_dev: the int32 step count, advanced unless the step is skipped for inf/NaN."""
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))        # the ABI's hyper-parameters are fp32  # noqa: E731
    _, b1, b2, eps, _, max_norm, _ = (f32(x) for x in hp)
    group_hp = [(f32(lr), f32(wd)) for lr, wd in group_hp]
    fixed = []
    for r, g in zip(records, grads):
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            G = g.reshape(rows, cols)
            c = (G * r["param"].reshape(rows, cols)).sum() / sigma
            g = ((G - (c * u)[:, None] * v[None, :]) * (1.0 / sigma)).reshape(g.shape)
        fixed.append(g)
    inv = 1.0 / float(grad_scale) if grad_scale is not None else 1.0
    norm = torch.sqrt(sum((g.double() ** 2).sum() for g in fixed)).float() * inv
    bad = not bool(torch.isfinite(norm))
    stats_out[0], stats_out[1] = norm, float(bad)
    if bad:
        return
    step_dev += 1
    step = int(step_dev)
    mul = (min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0) * inv
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    for r, g in zip(records, fixed):
        lr, wd = group_hp[r.get("group", 0)]
        g = g * mul
        p, m, v = r["param"], r["exp_avg"], r["exp_avg_sq"]
        p.mul_(1 - lr * wd)
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        p.addcdiv_(m, (v.sqrt() / (bc2 ** 0.5)).add_(eps), value=-lr / bc1)


def grad_accum_torch(records, grads, accs, first):
    """calm_grad_accum in torch, for a backend without `grad_accum` (CPU parameters): acc = (first ? 0 : acc) + g', with
    g' = (G - <G, W_orig>/sigma u v^T) * (1/sigma) for a record with `sn`, g' = G otherwise.  With first, `accs` are
    written without being read."""
    for r, g, a in zip(records, grads, accs):
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            G = g.reshape(rows, cols)
            c = (G * r["param"].reshape(rows, cols)).sum() / sigma
            g = (G - (c * u)[:, None] * v[None, :]) * (1.0 / sigma)
        if first:
            a.copy_(g.reshape(a.shape))
        else:
            a.add_(g.reshape(a.shape))


class FusedClipAdamWindow(FusedClipAdamW):
    """FusedClipAdamW with a gradient-accumulation window.

    `accumulate()` takes the current `.grad`s into the window: calm_grad_accum walks the optimizer's own (deferred) table
    with this micro-batch's gradient pointers, applies the spectral-norm correction with the u, v, sigma of the forward
    that produced them — the power iteration advances them in place at every training forward, so raw gradients summed
    over several forwards could not be corrected once at the end — and adds the finished gradients to fp32 accumulators
    (`first = 1` at the start of a window: written without being read, they may hold NaN from a skipped window).  Every
    `.grad` is then released: the next backward finds the gradient tail armable and autograd adopts fresh buffers.
    `step()` with `window > 0` runs calm_optim_step (calm_optim_step_groups with parameter groups: the plain plan carries
    the same group indices and shares the group table) over a second, "plain" plan — the same parameters, moments and device
    step counter, no correction, gradients = the accumulators, whose addresses are fixed, so its table is uploaded once
    — with `grad_scale * window` (or `window`) as the divisor: the mean over the micro-batches costs no pass.  `step()`
    with `window == 0` is FusedClipAdamW.step()."""

    def __init__(self, model, *args, **kw):
        super().__init__(model, *args, **kw)
        self.window = 0                         # micro-batches accumulated since the last step
        self._acc = self._acc_plan = self._acc_records = self._acc_ptrs = self._acc_ptrs_dev = None
        self._window_divisors = {}

    def bind_accumulators(self, accs=None):
        """Build the window: the fp32 accumulators (`accs`: tensors shaped like the parameters to accumulate in, e.g. the
        HeldGradReducer's bucket views; None: allocated here) and the plain plan that steps from them.  Refused inside
        an open window."""
        import numpy as np
        if self.window > 0:
            raise RuntimeError("FusedClipAdamWindow.bind_accumulators: a window is open; step() or zero_grad() first")
        if accs is None:
            accs = [torch.zeros_like(p, dtype=torch.float32) for p in self.params]
        accs = list(accs)
        if len(accs) != len(self.params) or any(a.shape != p.shape or a.dtype != torch.float32 or a.device != p.device
                                                or not a.is_contiguous() for a, p in zip(accs, self.params)):
            raise ValueError("FusedClipAdamWindow.bind_accumulators: one contiguous fp32 tensor per parameter, of its shape "
                             "and on its device")
        self._acc_records = [dict(r, sn=None) for r in self._records]        # (the group indices travel with them)
        plan = self._make_plan(self._acc_records)
        plan.step_dev = self._plan.step_dev     # one counter: snapshots and step_count see every step
        if self.grouped and hasattr(self.be, "optim_step_groups"):
            plan.groups = self._plan.groups     # one (lr, weight_decay) table: both plans step the same groups
        if self.lamb is not None and self._trust_host is None:
            plan._lamb = self._plan.lamb_buffers(self.be)       # one scratch, one trust table: trust_ratios() reads either
        self._acc, self._acc_plan = accs, plan
        self._acc_ptrs = np.asarray([a.data_ptr() for a in accs], dtype=np.uint64)
        self._acc_ptrs_dev = torch.from_numpy(self._acc_ptrs.view(np.int64).copy()).to(self.params[0].device)

    def _check_plan(self):
        super()._check_plan()
        if self._acc is not None and _stale_ptrs(self._acc, self._acc_ptrs):
            raise RuntimeError("FusedClipAdamWindow: an accumulator was moved or replaced after the window was built")

    @torch.no_grad()
    def accumulate(self):
        """Take the current `.grad`s into the window (a parameter without one contributes zeros) and release them."""
        if self._acc is None:
            self.bind_accumulators()
        self._check_owner()
        grads = self._contiguous_grads(keep=False)
        first = self.window == 0                # the old sums (NaN after a skipped window) are overwritten, not read
        if hasattr(self.be, "grad_accum"):
            self.be.grad_accum(self._plan, grads, self._acc_ptrs_dev, first)
        else:
            grad_accum_torch(self._records, grads, self._acc, first)
        for p in self.params:
            p.grad = None
        self.window += 1

    def _window_divisor(self, grad_scale):
        """grad_scale * window (or window alone) as the device scalar calm_optim_step divides by."""
        if grad_scale is not None:
            return grad_scale * float(self.window)
        d = self._window_divisors.get(self.window)
        if d is None:
            d = self._window_divisors[self.window] = torch.full((1,), float(self.window), dtype=torch.float32,
                                                                device=self.params[0].device)
        return d

    @torch.no_grad()
    def step(self, closure=None, grad_scale=None):
        """With `window > 0`: one optimizer-side step on the mean of the window's accumulated gradients, then
        `window = 0`.  With `window == 0`: FusedClipAdamW.step()."""
        if self.window == 0 or closure is not None:
            return super().step(closure=closure, grad_scale=grad_scale)      # (which refuses a closure)
        self._check_owner()
        for p, a in zip(self.params, self._acc):
            if p.grad is not None and p.grad.data_ptr() != a.data_ptr():
                raise RuntimeError("FusedClipAdamWindow.step: a window is open and a parameter has a gradient outside it; "
                                   "accumulate() takes gradients into the window")
        stats = self._launch(self._acc_plan, self._acc, self._window_divisor(grad_scale), self._acc_records)
        self.window = 0
        return stats

    def zero_grad(self, set_to_none=True):
        """Release every `.grad` and discard an open window."""
        super().zero_grad(set_to_none)
        self.window = 0


def grad_stats_torch(records, step_dev, grads, hp, grad_scale, out, summary):
    """calm_grad_stats in torch, for a backend without `grad_stats` (CPU parameters), with the header's semantics in fp32:
    g' = G / grad_scale, for a record with `sn` g' = ((G - <G, W_orig>/sigma u v^T) * (1/sigma)) / grad_scale; grad_sq and
    grad_absmax over the elements whose g' is finite, param_sq / param_absmax, dir_sq of the Adam direction
    (1/bc1) m / (sqrt(v) / sqrt(bc2) + eps) at t = step_dev (0 while t < 1), nonfinite = the inf / NaN elements of the RAW
    gradient, and the sticky fields.  out: numpy record array of `_lib.GradStat` (one per record), summary: numpy
    int32[4] = calls, bad_calls, first_bad_call, first_bad_tensor; both initialised by the caller (counts 0, firsts -1)."""
    f32 = lambda x: torch.tensor(float(x), dtype=torch.float32)               # noqa: E731
    b1, b2, eps = f32(hp[1]), f32(hp[2]), f32(hp[3])
    inv = 1.0 / f32(float(grad_scale)) if grad_scale is not None else f32(1.0)
    t = int(step_dev)
    if t >= 1:
        inv_bc1 = 1.0 / (1.0 - torch.pow(b1, float(t)))
        inv_sqrt_bc2 = 1.0 / torch.sqrt(1.0 - torch.pow(b2, float(t)))
    call, first = int(summary[0]), -1
    for k, (r, g) in enumerate(zip(records, grads)):
        g = g.detach().float().reshape(-1)
        p = r["param"].detach().reshape(-1)
        bad = int((~torch.isfinite(g)).sum())
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            G = g.reshape(rows, cols)
            c = (G * p.reshape(rows, cols)).sum() / sigma
            g = ((G - (c * u)[:, None] * v[None, :]) * (1.0 / sigma)).reshape(-1)
        g = g * inv
        g = g[torch.isfinite(g)]
        e = out[k]
        e["grad_sq"], e["grad_absmax"] = float((g * g).sum()), float(g.abs().max()) if g.numel() else 0.0
        e["param_sq"], e["param_absmax"] = float((p * p).sum()), float(p.abs().max())
        e["dir_sq"] = 0.0
        if t >= 1:
            d = inv_bc1 * (r["exp_avg"].reshape(-1) / (r["exp_avg_sq"].reshape(-1).sqrt() * inv_sqrt_bc2 + eps))
            e["dir_sq"] = float((d * d).sum())
        e["nonfinite"] = bad
        if bad:
            e["bad_calls"] += 1
            if e["first_bad_call"] < 0:
                e["first_bad_call"] = call
            if first < 0:
                first = k
    summary[0] = call + 1
    if first >= 0:
        summary[1] += 1
        if summary[2] < 0:
            summary[2], summary[3] = call, first


class GradMonitor:
    """Per-tensor statistics of the gradients a FusedClipAdamW / FusedClipAdamWindow steps on, kept on the device.

    `GradMonitor(model, optimizer).attach()` arms it: every optimizer step — the eager one, the step that closes an
    accumulation window (then on the window's mean gradient) and a captured one — runs calm_grad_stats over the
    optimizer's own table in front of the update: three launches, no host synchronisation.  The statistics are of the TRUE
    gradient: corrected for the deferred spectral-norm layers, whose `.grad` between backward and step is not the
    gradient, and divided by the GradScaler's scale; clipping is not applied.  A step that the optimizer skips for an
    inf / NaN gradient is counted, with the tensors that held the values.  The trained parameters are those of the run
    without a monitor, bit for bit: the call writes only its own buffers.

    `read()` is the one host synchronisation (one device-to-host copy) and returns
      norm       the gradient norm of the last observed step over the finite elements (root of the float64 sum of grad_sq)
      calls      steps observed since the last reset();  skipped: those with a non-finite gradient
      first_bad  None, or {"call": 0-based index of the first such step, "tensor": the lowest tensor's name}
      groups     per param group: lr (the group's current rate), tensors, grad_norm, weight_norm, update_ratio =
                 lr * sqrt(sum dir_sq / sum param_sq), nonfinite (names of the tensors with a non-finite gradient in the
                 last observed step)
      tensors    name -> the calm_grad_stat fields, group, and grad_norm, weight_norm, update_ratio derived likewise
    dir_sq is the squared norm of the Adam direction of the moments as they were in front of the step — the update of the
    last applied step divided by its rate, without weight decay; it is 0 until a step has been applied.
    `reset()` clears the counters.  Under GraphedTrainStep attach before the capture: the kernels are captured with the
    step, and the counters then count replays (and the warm-up steps, until reset()).  With CPU parameters, or a backend
    without the entry point, `grad_stats_torch` computes the same report.  Names come from model.named_parameters().
    The monitor's state is not part of TrainState: a resumed run counts anew."""

    def __init__(self, model, optimizer):
        import numpy as np
        from . import _lib
        if not isinstance(optimizer, FusedClipAdamW):
            raise ValueError("GradMonitor reads the table of the fused optimizer: it needs a FusedClipAdamW or a "
                             f"FusedClipAdamWindow, got {type(optimizer).__name__}")
        names = {id(p): n for n, p in model.named_parameters()}
        missing = [k for k, p in enumerate(optimizer.params) if id(p) not in names]
        if missing:
            raise ValueError(f"GradMonitor: {len(missing)} parameters of the optimizer are not parameters of this model")
        self.optimizer = optimizer
        self.names = [names[id(p)] for p in optimizer.params]
        self.group_of = [int(r.get("group", 0)) for r in optimizer._records]
        self.n = len(self.names)
        self.dtype = np.dtype(_lib.GradStat)
        dev = optimizer.params[0].device
        self.native = dev.type == "cuda" and hasattr(optimizer.be, "grad_stats")
        init = np.zeros(self.n, dtype=self.dtype)
        init["first_bad_call"] = -1
        self._init = np.concatenate([init.view(np.uint8), np.asarray([0, 0, -1, -1], dtype=np.int32).view(np.uint8)])
        if self.native:
            # one buffer, so that read() is one copy: the records, then the summary
            self._buf = torch.empty(self._init.size, dtype=torch.uint8, device=dev)
            self._init_dev = torch.from_numpy(self._init.copy()).to(dev)
            self._out, self._summary = self._buf[:self.n * self.dtype.itemsize], self._buf[self.n * self.dtype.itemsize:].view(torch.int32)
            self._scratch = torch.empty(optimizer.be.grad_stats_scratch_floats(optimizer._plan), dtype=torch.float32, device=dev)
        else:
            self._host = self._init.copy()
        self.reset()

    def attach(self):
        """Arm the monitor: the optimizer's steps call observe() from now on.  Returns self."""
        self.optimizer.monitor = self
        return self

    def detach(self):
        if self.optimizer.monitor is self:
            self.optimizer.monitor = None

    def reset(self):
        """Clear the statistics and the sticky state: counts 0, firsts -1."""
        if self.native:
            self._buf.copy_(self._init_dev)
        else:
            self._host[:] = self._init

    def _views(self, host):
        import numpy as np
        nb = self.n * self.dtype.itemsize
        return host[:nb].view(self.dtype), host[nb:].view(np.int32)

    @torch.no_grad()
    def observe(self, plan, grads, divisor, records):
        """Called by FusedClipAdamW._launch in front of the step over `plan` (records `records`) with `grads` / `divisor`."""
        opt = self.optimizer
        hp = opt._hparams()
        if self.native:
            opt.be.grad_stats(plan, grads, hp, divisor, self._out, self._summary, self._scratch)
        else:
            out, summary = self._views(self._host)
            grad_stats_torch(records, plan.step_dev, grads, hp, divisor, out, summary)

    def read(self):
        import math
        rec, summary = self._views(self._buf.cpu().numpy() if self.native else self._host.copy())
        root = lambda x: math.sqrt(x) if x >= 0 else math.nan                 # noqa: E731  (inf stays inf, NaN stays NaN)
        ratio = lambda lr, d2, p2: lr * root(d2 / p2) if p2 > 0 else 0.0      # noqa: E731
        rates = [lr for lr, _ in self.optimizer.group_hparams()]
        tensors = {}
        groups = [dict(group=g, lr=lr, tensors=0, grad_sq=0.0, param_sq=0.0, dir_sq=0.0, nonfinite=[]) for g, lr in enumerate(rates)]
        for name, g, r in zip(self.names, self.group_of, rec):
            t = {k: (int(r[k]) if k in ("nonfinite", "bad_calls", "first_bad_call") else float(r[k])) for k in self.dtype.names}
            t.update(group=g, grad_norm=root(t["grad_sq"]), weight_norm=root(t["param_sq"]),
                     update_ratio=ratio(rates[g], t["dir_sq"], t["param_sq"]))
            tensors[name] = t
            G = groups[g]
            G["tensors"] += 1
            for k in ("grad_sq", "param_sq", "dir_sq"):
                G[k] += t[k]                                # (float64 sums of the fp32 per-tensor values)
            if t["nonfinite"] > 0:
                G["nonfinite"].append(name)
        for G in groups:
            g2, p2, d2 = G.pop("grad_sq"), G.pop("param_sq"), G.pop("dir_sq")
            G.update(grad_norm=root(g2), weight_norm=root(p2), update_ratio=ratio(G["lr"], d2, p2))
        calls, skipped, first_call, first_tensor = (int(x) for x in summary)
        return dict(norm=root(sum(t["grad_sq"] for t in tensors.values())), calls=calls, skipped=skipped,
                    first_bad=None if first_call < 0 else {"call": first_call, "tensor": self.names[first_tensor]},
                    groups=groups, tensors=tensors)


def sam_perturb_torch(records, grads, hp, grad_scale, backups, stats_out):
    """calm_sam_perturb in torch, for a backend without `sam_perturb` (CPU parameters), with the header's fp32 formula:
    g' = G / grad_scale, for a record with `sn` g' = ((G - <G, W_orig>/sigma u v^T) * (1/sigma)) / grad_scale; s = g', or
    with adaptive t = |w| + eta and s = t g'; norm = sqrt(sum s^2) over ALL records; found_inf when a RAW gradient element
    is inf / NaN or the norm is not finite; scale = found_inf ? 0 : rho / (norm + eps).  Every backup receives its
    parameter's bits; unless found_inf, w += (scale t) s.  hp = (rho, eps, eta, adaptive); stats_out[3] <- norm,
    found_inf, scale."""
    f32 = lambda x: torch.tensor(float(x), dtype=torch.float32)               # the ABI's hyper-parameters are fp32  # noqa: E731
    rho, eps, eta = f32(hp[0]), f32(hp[1]), f32(hp[2])
    adaptive = bool(hp[3])
    inv = 1.0 / f32(float(grad_scale)) if grad_scale is not None else f32(1.0)
    bad, total, dirs = False, torch.zeros((), dtype=torch.float32), []
    for r, g in zip(records, grads):
        g = g.detach().float().reshape(-1)
        p = r["param"].detach().reshape(-1)
        bad = bad or not bool(torch.isfinite(g).all())
        if r["sn"] is not None:
            u, v, sigma, rows, cols = r["sn"]
            G = g.reshape(rows, cols)
            c = (G * p.reshape(rows, cols)).sum() / sigma
            g = ((G - (c * u)[:, None] * v[None, :]) * (1.0 / sigma)).reshape(-1)
        g = g * inv
        t = p.abs() + eta if adaptive else None
        s = t * g if adaptive else g
        total = total + (s * s).sum()
        dirs.append((s, t))
    norm = torch.sqrt(total)
    bad = bad or not bool(torch.isfinite(norm))
    scale = torch.zeros((), dtype=torch.float32) if bad else rho / (norm + eps)
    stats_out[0], stats_out[1], stats_out[2] = norm, float(bad), scale
    for r, b, (s, t) in zip(records, backups, dirs):
        b.copy_(r["param"])
        if not bad:
            r["param"].add_(((scale * t) * s if adaptive else scale * s).reshape(r["param"].shape))


def sam_restore_torch(records, backups):
    """calm_sam_restore in torch: every parameter receives the bits of its backup."""
    for r, b in zip(records, backups):
        r["param"].copy_(b)


class SharpnessAware:
    """Sharpness-aware minimisation (SAM; adaptive=True: ASAM) on the table of a FusedClipAdamW / FusedClipAdamWindow.

    `perturb()` behind the first backward moves every parameter IN PLACE by rho along the normalised TRUE gradient —
    calm_sam_perturb corrects the `.grad` of the deferred spectral-norm layers, which between backward and step is not the
    gradient, and divides by the GradScaler's scale — after saving its bits; `restore()` behind the second backward puts
    the saved bits back (calm_sam_restore), so the addresses the optimizer plan, the EMA plan and the bf16 weight copies
    cache stay valid and the weights return exactly, on every rank alike.  Four launches and one, no host synchronisation.
    With adaptive=True the step of an element is rho t^2 g' / ||t g'||, t = |w| + eta.

    `perturb()` reads the current `.grad`s (a parameter without one contributes zeros) and then sets EVERY `.grad` to None.
    The second backward must start with no `.grad` left: then the gradient tail arms, the reducer's pack sees fresh
    buffers, and autograd adopts the new gradients instead of adding them into the first pass's.  A non-finite gradient in
    the first pass makes the perturbation zero (found_inf = 1, scale = 0, no parameter written); nothing else follows from
    it here.  While the weights are perturbed the optimizer refuses to step.  The second pass's `.grad`s of the deferred
    layers are gradients w.r.t. the weight normalised at w + e(w): finish them BEFORE restore() —
    `FusedClipAdamWindow.accumulate()`, as SamTrainStep does — because the correction reads the weights through the table.

    `read()` is the one host synchronisation: {"norm", "found_inf", "scale"} of the last perturb().  With CPU parameters,
    or a backend without the entry points, `sam_perturb_torch` / `sam_restore_torch` do the same.  SAM keeps no state
    between steps: nothing of it belongs to a TrainState."""

    def __init__(self, model, optimizer, rho=0.05, adaptive=False, eta=0.01, eps=1e-12):
        import numpy as np
        if not isinstance(optimizer, FusedClipAdamW):
            raise ValueError("SharpnessAware walks the table of the fused optimizer: it needs a FusedClipAdamW or a "
                             f"FusedClipAdamWindow, got {type(optimizer).__name__}")
        own = {id(p) for p in model.parameters()}
        missing = [k for k, p in enumerate(optimizer.params) if id(p) not in own]
        if missing:
            raise ValueError(f"SharpnessAware: {len(missing)} parameters of the optimizer are not parameters of this model")
        rho, eta, eps = float(rho), float(eta), float(eps)
        if not (rho > 0.0 and math.isfinite(rho)):
            raise ValueError(f"SharpnessAware: rho is a positive finite radius, got {rho!r}")
        if not (eps > 0.0 and math.isfinite(eps)) or float(torch.tensor(eps, dtype=torch.float32)) <= 0.0:
            raise ValueError(f"SharpnessAware: eps is a positive fp32 number, got {eps!r}")
        if not (eta >= 0.0 and math.isfinite(eta)):
            raise ValueError(f"SharpnessAware: eta is a non-negative finite number, got {eta!r}")
        self.optimizer = optimizer
        self.rho, self.adaptive, self.eta, self.eps = rho, bool(adaptive), eta, eps
        dev = optimizer.params[0].device
        self.native = dev.type == "cuda" and hasattr(optimizer.be, "sam_perturb")
        self.backups = [torch.empty_like(p, memory_format=torch.contiguous_format) for p in optimizer.params]
        self.stats = torch.zeros(3, dtype=torch.float32, device=dev)         # [norm, found_inf, scale]
        self._step_attr = None
        if self.native:
            ptrs = np.asarray([b.data_ptr() for b in self.backups], dtype=np.uint64)
            self._backup_ptrs_dev = torch.from_numpy(ptrs.view(np.int64).copy()).to(dev)
            self._scratch = torch.empty(optimizer.be.sam_scratch_floats(optimizer._plan), dtype=torch.float32, device=dev)

    @property
    def perturbed(self):
        return self.optimizer.perturbed_by is self

    def _hparams(self):
        return (self.rho, self.eps, self.eta, int(self.adaptive))

    @torch.no_grad()
    def perturb(self, grad_scale=None):
        """w -> w + e(w) from the current `.grad`s; grad_scale: the device scalar the loss was multiplied by, or None.
        Every `.grad` is None afterwards."""
        opt = self.optimizer
        if opt.perturbed_by is not None:
            raise RuntimeError("SharpnessAware.perturb: the parameters are already perturbed; restore() first")
        opt._check_owner()                      # (with _check_plan: parameters / spectral-norm buffers moved since construction)
        grads = opt._contiguous_grads(keep=False)
        if self.native:
            opt.be.sam_perturb(opt._plan, grads, self._hparams(), grad_scale, self._backup_ptrs_dev, self._scratch, self.stats)
        else:
            sam_perturb_torch(opt._records, grads, self._hparams(), grad_scale, self.backups, self.stats)
        for p in opt.params:
            p.grad = None
        opt.perturbed_by = self
        # the guard of optimizer.step(): an instance attribute in front of the method (and of a scheduler's counting
        # wrapper, which is one too and is put back by restore())
        self._step_attr = opt.__dict__.get("step")
        opt.step = self._refuse_step

    def _refuse_step(self, *args, **kw):
        raise RuntimeError("FusedClipAdamW.step: the parameters carry a SharpnessAware perturbation; restore() comes "
                           "before the step (the update belongs to the unperturbed weights)")

    @torch.no_grad()
    def restore(self):
        """The bits perturb() saved, back into the parameters."""
        opt = self.optimizer
        if opt.perturbed_by is not self:
            raise RuntimeError("SharpnessAware.restore: the parameters are not perturbed (perturb() comes first)")
        opt._check_plan()
        if self.native:
            opt.be.sam_restore(opt._plan, self._backup_ptrs_dev)
        else:
            sam_restore_torch(opt._records, self.backups)
        opt.perturbed_by = None
        if self._step_attr is not None:
            opt.step = self._step_attr
        else:
            del opt.step
        self._step_attr = None

    def read(self):
        norm, found_inf, scale = (float(v) for v in self.stats.cpu())
        return {"norm": norm, "found_inf": found_inf, "scale": scale}


class SamTrainStep(TrainStep):
    """TrainStep with sharpness-aware minimisation: two passes over the same batch per optimizer step.

      1. forward, loss, backward at w (same autocast, same GradScaler scale), the gradient exchange held;
      2. `sam.perturb(grad_scale=the current scale, read on the device as _optimizer_step reads it)`: w -> w + e(w),
         every `.grad` released;
      3. forward, loss, backward at w + e(w), then `optimizer.accumulate()`: the second pass's gradients are FINISHED here
         (calm_grad_accum, a window of one), while the parameters still hold w + e(w) — the deferred spectral-norm
         correction <G, W_orig / sigma> u v^T needs the W_orig, u, v, sigma of the forward that produced G, and behind the
         restore the table would point at w instead;
      4. `sam.restore()`: the saved bits of w; then the exchange of the finished gradients (`reduce_held()`);
      5. TrainStep's unchanged optimizer-side sequence, which steps the window of one.

    optimizer: a FusedClipAdamWindow (for step 3).  The step returns the loss and the output of the FIRST pass, and a
    metrics object is fed by the first pass only.  EMA, the GradScaler bookkeeping and a GradMonitor (it observes the second
    pass's gradients, those the step applies) are untouched.  A non-finite gradient in the first pass makes the
    perturbation zero, so the second pass is an ordinary pass at w; nothing is skipped on its account: only the
    optimizer's own found_inf, of the second pass's gradients, skips the update and backs the scale off.

    In a world of more than one rank (reducer: a HeldGradReducer, whose bucket views become the window's accumulators) the
    default (sync=False) is the per-rank perturbation of the SAM paper's m-sharpness: the first pass's gradients are NOT
    exchanged, so the perturbed weights differ between the ranks and half the communication is saved; every rank finishes
    its second-pass gradient with its own perturbed weights before the exchange, and restore() brings every rank back to
    identical bits (saved bits, not a subtraction), so the parameters never drift.  The spectral-norm buffers u, v, sigma
    do become rank-local then: the second forward iterates them on the rank's own perturbed weights (as BatchNorm
    statistics are rank-local under data parallelism; a checkpoint holds rank 0's).  sync=True exchanges the first pass
    through the reducer as well: one perturbation for all ranks, and the buffers stay replicated.  With sync=False a
    model that is, or contains, a stock DistributedDataParallel is refused: it would all-reduce both backwards.

    Two consequences of running the model twice: spectral norm's power iteration advances at both training forwards (as
    torch's would under a two-pass closure), so the second pass's u, v, sigma are one iteration further; and dropout and
    latent-noise keys are drawn in both passes, so the two passes see different masks / noise."""

    def __init__(self, model, optimizer, reducer=None, sam=None, sync=False, **kw):
        if not isinstance(sam, SharpnessAware) or sam.optimizer is not optimizer:
            raise ValueError("SamTrainStep needs sam=SharpnessAware(model, optimizer) over this step's optimizer")
        if not isinstance(optimizer, FusedClipAdamWindow):
            raise TypeError("SamTrainStep needs a FusedClipAdamWindow: the second pass's gradients are finished by "
                            "accumulate() while the weights are still perturbed (FusedClipAdamW.step would correct the "
                            "spectral-norm gradients against the restored weights)")
        if optimizer.window > 0:
            raise RuntimeError("SamTrainStep: the optimizer has an open accumulation window")
        self.sync = bool(sync)
        if not self.sync and any(isinstance(mod, torch.nn.parallel.DistributedDataParallel) for mod in model.modules()):
            raise TypeError("SamTrainStep(sync=False): DistributedDataParallel all-reduces every backward, the first "
                            "pass's too; use the bare model with a HeldGradReducer, or sync=True")
        if reducer is not None and reducer.enabled and not isinstance(reducer, HeldGradReducer):
            raise TypeError("SamTrainStep needs a HeldGradReducer (BucketedGradReducer all-reduces every backward)")
        super().__init__(model, optimizer, reducer=reducer, **kw)
        self.sam = sam
        self._second = False
        self._batch = None
        self._held = reducer is not None and reducer.enabled
        if self._held:
            reducer.hold = True
            optimizer.bind_accumulators(reducer.views_of(optimizer.params))      # the finished gradients ARE the buckets

    def __call__(self, x, y=None):
        self._batch = (x, y)
        try:
            return super().__call__(x, y)
        finally:
            self._batch, self._second = None, False

    def _finish(self, loss, y_hat):
        if self._second:                        # the second pass: its backward, and its gradients finished at w + e(w)
            self._backward(loss)
            self.opt.accumulate()
            return None
        if self._held:
            self.reducer.hold = not self.sync   # sync: the hooks launch the first pass's buckets
        try:
            self._backward(loss)
            if self._held and self.sync:
                self.reducer.finish()
        finally:
            if self._held:
                self.reducer.hold = True
        scale = self.scaler.scale(self._one) if self._clean_steps is not None else None
        self.sam.perturb(grad_scale=scale)
        metrics, self.metrics, self._second = self.metrics, None, True
        try:
            super().__call__(*self._batch)      # forward and loss of the task's step at w + e(w); re-enters _finish above
        except BaseException:
            self.opt.zero_grad()                # (discards the window, if the failure left one open)
            raise
        finally:
            self.metrics, self._second = metrics, False
            if self.sam.perturbed:
                self.sam.restore()
        if self._held:
            self.reducer.reduce_held()
        self._optimizer_step()
        return loss.detach(), y_hat.detach()


class SamRegTrainStep(SamTrainStep, RegTrainStep):
    """RegTrainStep (the generative trainer's forward and loss) with SamTrainStep's two passes."""

    def __init__(self, model, optimizer, reducer=None, sam=None, sync=False, kl_weight=0.1, **kw):
        super().__init__(model, optimizer, reducer, sam=sam, sync=sync, kl_weight=kl_weight, **kw)


def ema_weight(decay, schedule, n):
    """The weight w = 1 - d of weight-EMA update number n + 1 as calm_ema_update's first launch evaluates it, in fp32:
    d = decay (EMA_CONSTANT) or min(decay, (1 + n) / (10 + n)) (EMA_WARMUP).  numpy's float32 division is correctly
    rounded, as the kernel's is."""
    import numpy as np
    from . import _lib
    f = np.float32
    d = f(decay)
    if schedule == _lib.EMA_WARMUP:
        d = min(d, (f(1.0) + f(n)) / (f(10.0) + f(n)))
    return float(f(1.0) - d)


class ModelEMA:
    """Exponential moving average of a model's parameters (timm's ModelEmaV2 / torch's AveragedModel):
    after every optimizer step  ema += (1 - d) * (p - ema),  d = decay, or min(decay, (1 + n) / (10 + n)) with warmup=True
    (n = updates applied so far), so a short run is not dominated by the initial weights.

    Every entry of `model.named_parameters()` gets an fp32 clone (the "shadow"), initialised to the current value.
    CUDA parameters are updated by calm_ema_update — one pass over all of them, a launch of its own behind
    calm_optim_step — and there is no torch fallback for them; CPU parameters (the gloo path of train(use_gpu=False)) take
    the same arithmetic through Tensor.lerp_ with the host-computed fp32 weight (`ema_weight`) and a host counter.

    Buffers are NOT shadowed.  The only ones this model has are the spectral-norm `weight_u` / `weight_v`: unit direction
    vectors of the power iteration on the LIVE weight, not quantities a mean of which means anything (the average of unit
    vectors is not a unit vector, and sigma = u^T W v is taken with them).  They stay shared: evaluating with the average
    uses the live u / v, as a copy of the model loaded with `model_state_dict()` does.

    Evaluation exchanges the averages INTO the parameters (calm_ema_swap) instead of exchanging tensor objects: the
    optimizer plan, the spectral-norm plan, the bf16 weight-copy plan and captured graphs (Predictor, GraphedTrainStep)
    cache raw parameter addresses, and all of them stay valid; a captured eval graph sees the averages on its next
    replay.  `with ema.applied(): ...` swaps in and, in a finally, back."""

    def __init__(self, model, decay=0.9999, warmup=True):
        from . import _lib
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"ModelEMA: decay must be in [0, 1), got {decay}")
        self.model = model
        self.decay = decay
        self.schedule = _lib.EMA_WARMUP if warmup else _lib.EMA_CONSTANT
        named = list(model.named_parameters())
        if not named:
            raise ValueError("ModelEMA: the model has no parameters")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        for n, p in named:
            if p.dtype != torch.float32:
                raise TypeError(f"ModelEMA: fp32 parameters expected, {n} is {p.dtype}")
        self.shadows = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self._swapped = False
        self._bind(0)

    def _bind(self, count):
        """Record the parameter addresses and, on a GPU, build the device plan; `count` = updates applied so far."""
        import numpy as np
        devices = {p.device for p in self.params}
        if len(devices) != 1:
            raise ValueError(f"ModelEMA: parameters on one device expected, got {sorted(map(str, devices))}")
        self.device = devices.pop()
        self._plan = None
        self._count = int(count)
        if self.device.type == "cuda":
            from .backend import get_backend
            self._be = get_backend()
            self._plan = self._be.ema_plan([(p.data, s) for p, s in zip(self.params, self.shadows)])
            self._plan.count_dev.fill_(int(count))
        self._ptrs = np.fromiter((p.data_ptr() for p in self.params), dtype=np.uint64, count=len(self.params))

    def rebind(self):
        """After the model was moved on purpose (model.to(device)): move the averages to the parameters' device and
        record the new addresses; the update count is kept."""
        if self._swapped:
            raise RuntimeError("ModelEMA.rebind: the averages are swapped into the model; swap() back first")
        count = self.num_updates
        self.shadows = [s.to(p.device) for s, p in zip(self.shadows, self.params)]
        self._bind(count)

    def _check(self):
        """The plan caches raw addresses (as FusedClipAdamW._check_plan): refuse to read orphaned storage."""
        if _stale_ptrs(self.params, self._ptrs):
            raise RuntimeError("ModelEMA: parameters were moved or replaced after the average was built (model.to / .float "
                               "/ load with assign=True); build it after the model is on its final device, or rebind()")

    @property
    def is_swapped(self):
        """True while the parameters hold the averages (and the shadows the live weights)."""
        return self._swapped

    @property
    def num_updates(self):
        """Updates applied (skipped ones not counted).  On a GPU the counter lives on the device: reading it synchronises."""
        return int(self._plan.count_dev.item()) if self._plan is not None else self._count

    def state_tensors(self):
        """The tensors that are this object's state, for an in-place snapshot / restore (GraphedTrainStep)."""
        return list(self.shadows) + ([self._plan.count_dev] if self._plan is not None else [])

    @torch.no_grad()
    def update(self, skip=None):
        """One update from the current parameters.  skip: a one-element fp32 tensor on the parameters' device; non-zero
        leaves the averages and the update count untouched (a step the optimizer skipped for inf/NaN gradients)."""
        if self._swapped:
            raise RuntimeError("ModelEMA.update: the averages are swapped into the model; swap() back before training on")
        self._check()
        if self._plan is not None:
            self._be.ema_update(self._plan, self.decay, self.schedule, skip)
            return
        if skip is not None and float(skip.reshape(-1)[0]) != 0.0:
            return
        w = ema_weight(self.decay, self.schedule, self._count)
        for p, s in zip(self.params, self.shadows):
            s.lerp_(p.detach(), w)
        self._count += 1

    @torch.no_grad()
    def swap(self):
        """Exchange parameters and averages in place, element for element."""
        self._check()
        if self._plan is not None:
            self._be.ema_swap(self._plan)
        else:
            for p, s in zip(self.params, self.shadows):
                t = p.detach().clone()
                p.detach().copy_(s)
                s.copy_(t)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def applied(self):
        """The model holds the averages inside the block; the live weights come back when it ends or raises."""
        if self._swapped:
            raise RuntimeError("ModelEMA.applied: the averages are swapped in already")
        self.swap()
        try:
            yield self.model
        finally:
            self.swap()

    def _live_shadows(self, what):
        if self._swapped:
            raise RuntimeError(f"ModelEMA.{what}: the averages are swapped into the model; swap() back first")
        return self.shadows

    def state_dict(self):
        from . import _lib
        return {"decay": self.decay, "warmup": self.schedule == _lib.EMA_WARMUP, "num_updates": self.num_updates,
                "shadow": {n: s.detach().clone() for n, s in zip(self.names, self._live_shadows("state_dict"))}}

    @torch.no_grad()
    def load_state_dict(self, sd):
        from . import _lib
        shadows = self._live_shadows("load_state_dict")
        got = sd["shadow"]
        if set(got) != set(self.names):
            missing, extra = sorted(set(self.names) - set(got)), sorted(set(got) - set(self.names))
            raise KeyError(f"ModelEMA.load_state_dict: parameter names differ (missing {missing[:3]}, unexpected {extra[:3]})")
        for n, s in zip(self.names, shadows):
            if tuple(got[n].shape) != tuple(s.shape):
                raise ValueError(f"ModelEMA.load_state_dict: {n} has shape {tuple(got[n].shape)}, expected {tuple(s.shape)}")
        decay = float(sd["decay"])
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"ModelEMA.load_state_dict: decay must be in [0, 1), got {decay}")
        for n, s in zip(self.names, shadows):
            s.copy_(got[n])                                       # in place: the plan holds these addresses
        self.decay = decay
        self.schedule = _lib.EMA_WARMUP if sd["warmup"] else _lib.EMA_CONSTANT
        self._count = int(sd["num_updates"])
        if self._plan is not None:
            self._plan.count_dev.fill_(self._count)

    def model_state_dict(self):
        """The model's state_dict() with every parameter replaced by a clone of its average (buffers as they are): loads
        into a ViT — and into the reference's — under the same keys."""
        sd = self.model.state_dict()
        for n, s in zip(self.names, self._live_shadows("model_state_dict")):
            sd[n] = s.detach().clone()
        return sd


class _TailSampler(torch.utils.data.Sampler):
    """The indices of `sampler` without its first `skip` ones: the rest of an epoch whose first batches a run that is
    being resumed has already trained on.  The indices are dropped here — nothing is loaded and thrown away."""

    def __init__(self, sampler, skip):
        self.sampler, self.skip = sampler, max(int(skip), 0)

    def __iter__(self):
        return iter(list(self.sampler)[self.skip:])

    def __len__(self):
        return max(len(self.sampler) - self.skip, 0)


def resume_tail(sampler, skip_batches, batch_size):
    """Sampler over what is left of the current epoch of `sampler` (set_epoch already called) behind its first
    `skip_batches` batches of `batch_size` samples."""
    return _TailSampler(sampler, int(skip_batches) * int(batch_size))


def _b64(t):
    import base64
    return base64.b64encode(t.cpu().numpy().tobytes()).decode("ascii")


def _unb64(text):
    import base64
    import numpy as np
    return torch.from_numpy(np.frombuffer(base64.b64decode(text), dtype=np.uint8).copy())


class TrainState:
    """The whole state of a training run as ONE file, written without stalling the training thread, and resumed from
    exactly: parameters and buffers, the optimizer's moments and step count, the weight EMA and its update count, the
    step metrics, the GradScaler's scale and the growth count of the fused step, the scheduler, the learning rate (a
    FusedClipAdamW with more than one param group: every group's, as "lrs"; a file of another group count is refused), the
    torch CPU / CUDA RNG states, the numpy generators of the device collate / augmentation and the position in the run.
    The tensor set is the one GraphedTrainStep(restore_after_warmup=True) puts back, which
    tests/test_determinism_gpu.py shows to be sufficient bit for bit.

        st = TrainState(model, optimizer, scaler, scheduler, ema, step, metrics, generators={"collate": dcoll.rng})
        st.save_async(path, {"epoch": e, "batch": b, "step": n})    # one kernel launch on the training stream
        st.poll()                                                   # once per step: hands a finished copy to the writer
        st.wait()                                                   # the file is in place (or the writer's error raises)
        progress = st.load(path)                                    # in place: every plan and captured graph stays valid
        st.close()

    On a GPU the tensors are gathered into one device buffer by calm_snapshot_pack (one launch on the current stream); a
    side stream that waits for it copies the buffer into one pinned host buffer; poll() sees that copy's event complete
    and starts a plain Python thread that computes the CRC32, writes `path + ".tmp"`, fsyncs and renames — that thread
    makes no torch or HIP call, every GPU API call stays on the calling thread.  load() reads the payload into the pinned
    buffer, copies it to the device once and scatters it with calm_snapshot_unpack.  A CPU model packs with plain tensor
    copies into the same layout (backend.snapshot_layout), so a file written on either kind of device loads on the other.

    Entries are named, so a file is checked against the live objects before a byte is scattered: `model.<state_dict key>`,
    `optim.exp_avg.<i>` / `optim.exp_avg_sq.<i>` / `optim.step` (FusedClipAdamW; loaded strictly in place), `ema.shadow.<name>`
    / `ema.count`, `metrics`, `step.clean_steps`, `scaler.scale`.  For a torch optimizer the tensors of
    `state_dict()["state"]` that live on the model's device are packed in order as `optim.state.<i>.<key>`, every other
    value goes into the header, and the load goes through `optimizer.load_state_dict`.

    File: 8 bytes magic, uint64 little-endian header length, the JSON header, zero padding to a multiple of 4 096 bytes,
    the payload.  The header holds the format version, the entry list (name, dtype, shape, offset, nbytes), packed_bytes,
    the payload's CRC32 and the host state — JSON throughout, no pickle.  With `sidecar_rank=r` the per-rank host state (RNG
    states, generators) is written to and read from the small JSON file `<path>.rank<r>.json` instead: in a world of
    more than one rank every rank keeps its own, and only rank 0 writes the payload (`payload=False` elsewhere)."""

    MAGIC = b"CALMSNAP"
    VERSION = 1
    PAGE = 4096
    _PER_RANK = ("rng", "generators", "rank")

    def __init__(self, model, optimizer, scaler=None, scheduler=None, ema=None, step=None, metrics=None, generators=None,
                 payload=True, sidecar_rank=None):
        self.model, self.opt, self.scheduler, self.ema, self.metrics = model, optimizer, scheduler, ema, metrics
        self.scaler = scaler if scaler is not None and scaler.is_enabled() else None
        self.generators = dict(generators) if isinstance(generators, dict) else \
            {str(i): g for i, g in enumerate(generators or [])}
        self.payload, self.sidecar_rank = bool(payload), sidecar_rank
        self._optim_desc = None
        self.fused = isinstance(optimizer, FusedClipAdamW)
        self.device = next(model.parameters()).device
        self.on_gpu = self.device.type == "cuda"
        if self.scaler is not None and self.on_gpu:
            self.scaler.scale(torch.ones((), dtype=torch.float32, device=self.device))   # creates the scale tensor
        self._ema_count = torch.zeros(1, dtype=torch.int32) if ema is not None and ema._plan is None else None
        self._plan = self._plan_key = None
        self._host = self._host_np = None
        self._side = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        self._copied = None                       # event behind the device-to-host copy of the save in flight
        self._job = None                          # (path, header fields) of a save whose copy has not been handed over
        self._thread = None
        self._error = None
        self.step = None
        self.bind_step(step)

    # ---- the tensor set ---------------------------------------------------------------------------------------
    def bind_step(self, step):
        """The TrainStep whose GradScaler growth count (fused optimizer: `_clean_steps`) belongs to the state; a
        GraphedTrainStep stands for its captured inner step.  Rebinding waits for a save in flight."""
        self.wait()
        step = getattr(step, "inner", step)
        if step is not None and self.fused and self.scaler is not None and step._clean_steps is None:
            raise ValueError(f"TrainState.bind_step: {type(step).__name__} keeps no GradScaler growth count (it was built "
                             "without this state's scaler or without its fused optimizer), so the state would lack "
                             "step.clean_steps; give the step and the state the same optimizer and scaler")
        self.step = step
        self._plan_key = None

    def _fixed_entries(self):
        """[(name, tensor)] of everything that is loaded in place, in file order except for a torch optimizer's state."""
        head = [("model." + k, v) for k, v in self.model.state_dict().items()]
        optim, tail = [], []
        if self.fused:
            optim += [(f"optim.exp_avg.{i}", t) for i, t in enumerate(self.opt.exp_avg)]
            optim += [(f"optim.exp_avg_sq.{i}", t) for i, t in enumerate(self.opt.exp_avg_sq)]
            optim.append(("optim.step", self.opt._plan.step_dev))
        if self.ema is not None:
            tail += [("ema.shadow." + n, s) for n, s in zip(self.ema.names, self.ema.shadows)]
            tail.append(("ema.count", self.ema._plan.count_dev if self.ema._plan is not None else self._ema_count))
        if self.metrics is not None:
            tail.append(("metrics", self.metrics.buf))
        if self.step is not None and self.step._clean_steps is not None and self.fused and self.scaler is not None:
            tail.append(("step.clean_steps", self.step._clean_steps))
        if self.scaler is not None and self.on_gpu:
            tail.append(("scaler.scale", self.scaler._scale))
        return head, optim, tail

    def _torch_optim_state(self):
        """A torch optimizer's state_dict() split into packed tensors and a JSON description."""
        sd = self.opt.state_dict()
        entries, desc = [], {}
        for idx, st in sd["state"].items():
            d = desc[str(idx)] = {}
            for key, v in st.items():
                if isinstance(v, torch.Tensor) and v.device == self.device:
                    name = f"optim.state.{idx}.{key}"
                    entries.append((name, v))
                    d[key] = {"entry": name}
                elif isinstance(v, torch.Tensor):
                    d[key] = {"tensor": v.cpu().reshape(-1).tolist(), "dtype": str(v.dtype).replace("torch.", ""),
                              "shape": list(v.shape)}
                else:
                    d[key] = {"value": v}
        return entries, {"state": desc, "param_groups": sd["param_groups"]}

    def _check_ready(self, what):
        if self.ema is not None and self.ema.is_swapped:
            raise RuntimeError(f"TrainState.{what}: the weight averages are swapped into the model; swap() back first")

    @staticmethod
    def _spec(entries):
        return [(n, t.dtype, tuple(t.shape)) for n, t in entries]

    def _bind(self, entries):
        """The plan (GPU) and the host buffer for this entry list; rebuilt only when the list changes."""
        from . import backend
        key = tuple((n, t.data_ptr(), t.dtype, tuple(t.shape)) for n, t in entries)
        if key == self._plan_key:
            return
        offsets, sizes, total = backend.snapshot_layout(self._spec(entries))
        if self.on_gpu:
            self._plan = backend.get_backend().snapshot_plan([t for _, t in entries], [n for n, _ in entries])
            assert self._plan.offsets == offsets and self._plan.packed_bytes == total
        self._layout = (offsets, sizes, total)
        if self._host is None or self._host.numel() != total:
            self._host = torch.zeros(max(total, 1), dtype=torch.uint8)
            if self.on_gpu:
                self._host = self._host.pin_memory()
            self._host_np = self._host.numpy()[:total]
        self._plan_key = key
        self._entries = entries
        self._entry_list = [{"name": n, "dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape),
                             "offset": off, "nbytes": nb} for (n, t), off, nb in zip(entries, offsets, sizes)]

    def _current_entries(self):
        if self.fused and self._plan_key is not None:
            return self._entries                  # a fixed set of tensors (the optimizer and the EMA refuse moved ones)
        head, optim, tail = self._fixed_entries()
        self._optim_desc = None
        if not self.fused:
            optim, self._optim_desc = self._torch_optim_state()
        return head + optim + tail

    # ---- host state -------------------------------------------------------------------------------------------
    def host_state(self, progress):
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        h = {"progress": {k: int(progress[k]) for k in ("epoch", "batch", "step")}, "world": world, "rank": rank,
             "lr": self.opt.param_groups[0]["lr"],
             "scheduler": None if self.scheduler is None else self.scheduler.state_dict(),
             "rng": {"torch_cpu": _b64(torch.get_rng_state()),
                     "cuda": _b64(torch.cuda.get_rng_state(self.device)) if self.on_gpu else None},
             "generators": {n: g.bit_generator.state for n, g in self.generators.items()}}
        if self.fused and len(self.opt.param_groups) > 1:     # (a torch optimizer's groups travel in its own state dict)
            h["lrs"] = [g["lr"] for g in self.opt.param_groups]
        if self.fused and self.opt.lamb is not None:          # the state is AdamW's; the key alone tells the two rules apart
            h["lamb"] = dict(self.opt.lamb)
        rates = self._drop_path_rates()
        if rates is not None:                                 # stochastic depth changes what a step computes, not its state
            h["drop_path"] = rates
        if self._mim_settings() is not None:                  # so does masked image modelling
            h["mim"] = self._mim_settings()
        if not self.fused and self.payload:
            h["optimizer"] = self._optim_desc
            if self.scaler is not None:            # torch's own GradScaler policy: its growth count (reading it synchronises)
                h["scaler"] = {"growth_tracker": int(self.scaler.state_dict()["_growth_tracker"])}
        return h

    def _drop_path_rates(self):
        """The per-block stochastic-depth rates of the model in forward order, or None when every rate is 0."""
        from .Vi_Tools_CNN_less_V2 import drop_path_rates
        rates = [r for _, r in drop_path_rates(self.model)]
        return rates if any(r > 0 for r in rates) else None

    def _mim_settings(self):
        """settings() of the bound step's MaskedImageModelling, or None."""
        mim = getattr(self.step, "mim", None)
        return None if mim is None else mim.settings()

    def _set_rng(self, h):
        torch.set_rng_state(_unb64(h["rng"]["torch_cpu"]))
        if self.on_gpu and h["rng"].get("cuda") is not None:
            torch.cuda.set_rng_state(_unb64(h["rng"]["cuda"]), self.device)

    def reapply_rng(self):
        """Set the torch RNG states of the last load() again: a DataLoader iterator draws its base seed from the CPU
        generator when it is made, and a run resumed inside an epoch makes that iterator after the state was loaded —
        the uninterrupted run made it before the state was saved."""
        if self._loaded_host is not None:
            self._set_rng(self._loaded_host)

    # ---- save ------------------------------------------------------------------------------------------------
    def save_async(self, path, progress):
        """Snapshot the state as it is now on the current stream; returns once the pack is enqueued."""
        import json
        self.wait()
        self._check_ready("save_async")
        if getattr(self.opt, "window", 0) > 0 or getattr(self.step, "window", 0) > 0:
            raise RuntimeError("TrainState.save_async: a gradient-accumulation window is open; snapshots are taken behind "
                               "an optimizer step (AccumTrainStep.boundary / flush())")
        if not self.payload:                      # a rank that only keeps its own host state
            side = self.host_state(progress)
            self._write_atomic(self.sidecar(path), json.dumps({k: side[k] for k in self._PER_RANK + ("progress", "world")}).encode())
            return
        entries = self._current_entries()
        self._bind(entries)
        offsets, sizes, total = self._layout
        if self._ema_count is not None:
            self._ema_count.fill_(self.ema._count)
        host = self.host_state(progress)
        header = {"version": self.VERSION, "packed_bytes": total, "entries": self._entry_list}
        if self.sidecar_rank is not None:
            side = {k: host.pop(k) for k in self._PER_RANK}
            side["progress"], side["world"] = host["progress"], host["world"]
            self._write_atomic(self.sidecar(path), json.dumps(side).encode())
        header["host"] = host
        json.dumps(host)                          # what cannot be written raises here, on the caller's thread
        if self.on_gpu:
            from .backend import get_backend
            get_backend().snapshot_pack(self._plan)
            packed = torch.cuda.Event()
            packed.record()
            with torch.cuda.stream(self._side):
                self._side.wait_event(packed)
                self._host[:total].copy_(self._plan.packed, non_blocking=True)
                self._copied = torch.cuda.Event()
                self._copied.record(self._side)
            self._job = (path, header)
        else:
            with torch.no_grad():
                for (n, t), off, nb in zip(entries, offsets, sizes):
                    if nb:
                        self._host[off:off + nb] = t.detach().contiguous().reshape(-1).view(torch.uint8)
            self._job = (path, header)
            self.poll()

    def sidecar(self, path):
        return f"{path}.rank{int(self.sidecar_rank)}.json"

    def poll(self):
        """Hand a finished device-to-host copy to the writer thread (never blocks)."""
        if self._job is None or (self._copied is not None and not self._copied.query()):
            return
        import threading
        (path, header), self._job, self._copied = self._job, None, None
        self._thread = threading.Thread(target=self._write, args=(path, header, self._host_np), daemon=True)
        self._thread.start()

    def _write(self, path, header, payload):
        """Writer thread: plain Python, no torch or HIP call."""
        try:
            import json
            import struct
            import zlib
            header["crc32"] = zlib.crc32(payload) & 0xFFFFFFFF
            text = json.dumps(header).encode()
            pad = -(16 + len(text)) % self.PAGE
            self._write_atomic(path, self.MAGIC + struct.pack("<Q", len(text)) + text + b"\0" * pad, payload)
        except BaseException as e:              # re-raised by wait()
            self._error = e

    @staticmethod
    def _write_atomic(path, *parts):
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            for part in parts:
                f.write(part)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)

    def wait(self):
        """Block until the save in flight is in place; re-raise what its writer raised."""
        if getattr(self, "_job", None) is not None:
            if self._copied is not None:
                self._copied.synchronize()
            self.poll()
        if getattr(self, "_thread", None) is not None:
            self._thread.join()
            self._thread = None
        if getattr(self, "_error", None) is not None:
            e, self._error = self._error, None
            raise e

    def close(self):
        self.wait()

    # ---- load ------------------------------------------------------------------------------------------------
    @classmethod
    def read_header(cls, path):
        """(header dict, payload offset) of a snapshot file; refuses a wrong magic or version and a short file."""
        import json
        import struct
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(16)
            if len(head) < 16 or head[:8] != cls.MAGIC:
                raise ValueError(f"{path}: not a training snapshot (magic {head[:8]!r}, expected {cls.MAGIC!r})")
            n = struct.unpack("<Q", head[8:])[0]
            if 16 + n > size:
                raise ValueError(f"{path}: short file: the header is {n} bytes, the file holds {size}")
            header = json.loads(f.read(n).decode())
        if header.get("version") != cls.VERSION:
            raise ValueError(f"{path}: snapshot format version {header.get('version')!r}, this build reads {cls.VERSION}")
        start = -(-(16 + n) // cls.PAGE) * cls.PAGE
        if start + int(header["packed_bytes"]) > size:
            raise ValueError(f"{path}: short file: {size} bytes, header and payload need {start + int(header['packed_bytes'])}")
        return header, start

    def load(self, path):
        """Put the state of the file back, in place; returns its progress.  Refuses, naming the first difference, a wrong
        magic or version, a short file, a CRC mismatch, an entry whose name, dtype or shape differs from the live set and
        another world size."""
        import json
        import zlib
        from . import backend
        self.wait()
        self._check_ready("load")
        header, start = self.read_header(path)
        host = dict(header["host"])
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if int(host["world"]) != world:
            raise ValueError(f"{path}: written by a world of {host['world']} ranks, this one has {world}")
        if self.sidecar_rank is not None:
            with open(self.sidecar(path)) as f:
                side = json.load(f)
            if side["progress"] != host["progress"] or int(side["world"]) != world:
                raise ValueError(f"{self.sidecar(path)}: written at {side['progress']} in a world of {side['world']}, "
                                 f"{path} at {host['progress']} in a world of {host['world']}")
            host.update({k: side[k] for k in self._PER_RANK})
        if set(host["generators"]) != set(self.generators):
            raise ValueError(f"{path}: generators {sorted(host['generators'])} in the file, {sorted(self.generators)} given")
        n_groups = len(host["lrs"]) if "lrs" in host else 1
        if self.fused and n_groups != len(self.opt.param_groups):
            raise ValueError(f"{path}: written with {n_groups} parameter group(s), this optimizer has "
                             f"{len(self.opt.param_groups)}")
        if self.fused and ("lamb" in host) != (self.opt.lamb is not None):
            raise ValueError(f"{path}: written with{'' if 'lamb' in host else 'out'} LAMB, this optimizer steps "
                             f"with{'' if self.opt.lamb is not None else 'out'} it")
        rates = self._drop_path_rates()
        if host.get("drop_path") != rates:
            said = lambda r: "without drop_path" if r is None else f"with drop_path rates {min(r):.4g} .. {max(r):.4g}"  # noqa: E731
            raise ValueError(f"{path}: written {said(host.get('drop_path'))}, this model runs {said(rates)}")
        if host.get("mim") != self._mim_settings():
            said = lambda m: "without mim" if m is None else f"with mim patch {m['patch']}, ratio {m['ratio']:.4g}, fill {m['fill']}"  # noqa: E731
            raise ValueError(f"{path}: written {said(host.get('mim'))}, this step trains {said(self._mim_settings())}")
        # the entries: everything but a torch optimizer's state must be the live set, name by name
        head, optim, tail = self._fixed_entries()
        live = head + optim + tail
        entries, k = [], 0
        dt = lambda e: getattr(torch, e["dtype"])  # noqa: E731
        for i, e in enumerate(header["entries"]):
            if not self.fused and e["name"].startswith("optim.state."):
                entries.append((e["name"], torch.zeros(e["shape"], dtype=dt(e), device=self.device)))
                continue
            if k >= len(live):
                raise ValueError(f"{path}: entry {i} ({e['name']}) has no counterpart in the live state")
            n, t = live[k]
            if e["name"] != n:
                raise ValueError(f"{path}: entry {i} is {e['name']} in the file and {n} in the live state")
            if dt(e) != t.dtype or tuple(e["shape"]) != tuple(t.shape):
                raise ValueError(f"{path}: entry {n} is {e['dtype']} {tuple(e['shape'])} in the file and "
                                 f"{str(t.dtype).replace('torch.', '')} {tuple(t.shape)} in the live state")
            entries.append((n, t))
            k += 1
        if k < len(live):
            raise ValueError(f"{path}: the live state has {live[k][0]}, the file does not")
        offsets, sizes, total = backend.snapshot_layout(self._spec(entries))
        if total != int(header["packed_bytes"]) or offsets != [e["offset"] for e in header["entries"]] \
                or sizes != [e["nbytes"] for e in header["entries"]]:
            raise ValueError(f"{path}: the offsets in the header are not the layout of its entries")
        self._plan_key = None
        self._bind(entries)
        with open(path, "rb") as f:
            f.seek(start)
            got = f.readinto(memoryview(self._host_np)) if total else 0
        if got != total:
            raise ValueError(f"{path}: short file: {got} of {total} payload bytes")
        crc = zlib.crc32(self._host_np) & 0xFFFFFFFF
        if crc != int(header["crc32"]):
            raise ValueError(f"{path}: payload CRC32 {crc:#010x}, the header says {int(header['crc32']):#010x}")
        with torch.no_grad():
            if self.on_gpu:
                self._plan.packed.copy_(self._host[:total], non_blocking=True)
                backend.get_backend().snapshot_unpack(self._plan)
                torch.cuda.current_stream().synchronize()          # the pinned buffer and fresh tensors are free again
            else:
                for (n, t), off, nb in zip(entries, offsets, sizes):
                    if nb:
                        t.copy_(self._host[off:off + nb].view(t.dtype).reshape(t.shape))
        # host state
        if self._ema_count is not None:
            self.ema._count = int(self._ema_count[0])
        if not self.fused:
            by_name = dict(entries)
            state = {}
            for idx, d in host["optimizer"]["state"].items():
                st = state[int(idx)] = {}
                for key, v in d.items():
                    if "entry" in v:
                        st[key] = by_name[v["entry"]]
                    elif "tensor" in v:
                        st[key] = torch.tensor(v["tensor"], dtype=getattr(torch, v["dtype"])).reshape(v["shape"])
                    else:
                        st[key] = v["value"]
            groups = host["optimizer"]["param_groups"]
            for g in groups:
                if "betas" in g:
                    g["betas"] = tuple(g["betas"])
            self.opt.load_state_dict({"state": state, "param_groups": groups})
            if self.scaler is not None and "scaler" in host:
                sd = self.scaler.state_dict()
                sd["_growth_tracker"] = int(host["scaler"]["growth_tracker"])
                self.scaler.load_state_dict(sd)
            self._plan_key = None                 # the tensors made above are now the optimizer's (or copies of them)
        self.opt.param_groups[0]["lr"] = host["lr"]
        if self.fused:
            for g, glr in zip(self.opt.param_groups, host.get("lrs", ())):
                g["lr"] = glr
        if self.scheduler is not None:
            if host["scheduler"] is None:
                raise ValueError(f"{path}: written without a scheduler, this run has one")
            self.scheduler.load_state_dict(host["scheduler"])
        for n, g in self.generators.items():
            g.bit_generator.state = host["generators"][n]
        self._loaded_host = host
        self._set_rng(host)
        return dict(host["progress"])

    _loaded_host = None


class GraphedTrainStep:
    """The same step captured once into a hipGraph and replayed: every kernel of the library only enqueues on the
    current stream (no allocation, no host sync), so forward + loss + backward + gradient exchange + unscale / clip /
    AdamW is one graph launch — with the library's fused optimizer-side step (FusedClipAdamW: its step counter, plan
    and learning rate live on the device) or a capturable torch optimizer, with or without the reference trainer's
    autocast(bfloat16) + GradScaler (the scale update is device arithmetic: TrainStep._optimizer_step).  Removes the ~3000
    host-side launches per step: the host's share of a step drops from tens of milliseconds to one graph launch, which
    is what keeps 8 ranks on one host from becoming host-bound.  N > 1: pass the BucketedGradReducer — its bucket
    copies and RCCL all-reduces are captured with the step (round 4; the collectives are issued in the
    capture-compatible form, see BucketedGradReducer._launch); without one the constructor refuses a world of more than
    one rank.  Inputs are copied into static buffers.  A learning-rate scheduler acts on replays: FusedClipAdamW reads
    the rate from a device scalar (calm_optim_step's lr_dev, ABI v7) that __call__ refreshes from
    param_groups[0]["lr"] before the replay — with parameter groups, the (lr, weight_decay) table of
    calm_optim_step_groups, rewritten when any group's value changed; capturable torch optimizers keep theirs on the
    device already.

    The warm-up steps in front of the capture (allocator, lazy plans) are real training steps on the example batch.
    restore_after_warmup=True (FusedClipAdamW only) undoes them: parameters, buffers (spectral-norm u / v), optimizer
    moments, the device step counter, the GradScaler state and the CUDA RNG state are put back IN PLACE after the
    capture, so that the first replay is step 1 of the run — the replayed trajectory then equals the eager one."""

    def __init__(self, model, optimizer, example_x, example_y, max_norm=1.0, warmup=3, scaler=None, autocast_dtype=None,
                 reducer=None, restore_after_warmup=False, metrics=None, ema=None, loss=None):
        """loss: TrainStep's loss= (None / "ce" / "bce" / a dict), handed to the inner step.
        ema: a ModelEMA of `model`; calm_ema_update is captured behind the optimizer step, and restore_after_warmup puts
        the averages and their device update count back with the rest, so the first replay is update 1.
        reducer: a BucketedGradReducer whose bucket copies and RCCL all-reduces are captured with the step (round 4:
        the collectives are issued in the capture-compatible form, see BucketedGradReducer._launch; exercised in a world
        of one in a child process by scripts/rccl_capture_check.py — DESIGN.md section 6 records the outcome)."""
        if reducer is None and dist.is_initialized() and dist.get_world_size() > 1:
            # the captured step would contain no gradient exchange: replicas would silently train apart
            raise RuntimeError("GraphedTrainStep captures a single-GPU step unless it is given the BucketedGradReducer "
                               "to capture with it; with world_size > 1 pass reducer=... or use TrainStep")
        # metrics: the StepMetrics buffer's address is baked into the graph, so replays keep accumulating into it
        self.inner = TrainStep(model, optimizer, reducer, max_norm=max_norm, scaler=scaler, autocast_dtype=autocast_dtype,
                               metrics=metrics, ema=ema, loss=loss)
        self.opt = optimizer
        if isinstance(optimizer, FusedClipAdamW):
            optimizer.lr_on_device = True          # replays read the learning rate from a device scalar
        self.x = example_x.clone()
        self.y = example_y.clone()
        snap = None
        if restore_after_warmup:
            if not isinstance(optimizer, FusedClipAdamW):
                raise ValueError("restore_after_warmup needs FusedClipAdamW (its whole state is a known set of tensors)")
            live = list(model.parameters()) + list(model.buffers()) + optimizer.exp_avg + optimizer.exp_avg_sq + \
                [optimizer._plan.step_dev] + ([metrics.buf] if metrics is not None else []) + \
                ([] if ema is None else ema.state_tensors())
            snap = ([(t, t.detach().clone()) for t in live], torch.cuda.get_rng_state(example_x.device),
                    None if scaler is None or not scaler.is_enabled() else scaler.get_scale())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                     # warm-up on a side stream (allocator + lazy plans)
            for _ in range(max(warmup, 1 if scaler is not None else 0)):
                self.inner(self.x, self.y)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if reducer is not None and getattr(reducer, "enabled", False) and getattr(reducer, "on_gpu", False):
            # The warm-up's all-reduces left Work objects with ProcessGroupNCCL's watchdog thread, which drops a finished
            # one only at its next sweep (every 100 ms) and finds out by hipEventQuery — a call the runtime refuses from
            # any thread while a stream captures in global mode: the watchdog then throws and the process aborts.  All of
            # them are finished here, so three sweep periods later its list is empty and it queries nothing during the
            # capture (collectives issued while capturing are not handed to it).
            time.sleep(0.3)
        if isinstance(optimizer, FusedClipAdamW):
            optimizer.sync_lr_to_device()          # nothing is written to the rates during the capture
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.y_hat = self.inner(self.x, self.y)
        if snap is not None:                               # in place: the graph replays on these addresses
            with torch.no_grad():
                for t, c in snap[0]:
                    t.copy_(c)
            torch.cuda.set_rng_state(snap[1], example_x.device)
            if snap[2] is not None:
                scaler.update(new_scale=float(snap[2]))                # fill_ on the scale tensor the graph reads
                if self.inner._clean_steps is not None:
                    self.inner._clean_steps.zero_()                    # (the fused step keeps the growth count itself)
            torch.cuda.synchronize()

    def __call__(self, x, y_soft):
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y_soft, non_blocking=True)
        if isinstance(self.opt, FusedClipAdamW):
            self.opt.sync_lr_to_device()           # a scheduler's new rate reaches the replay without re-capture
        self.graph.replay()
        return self.loss, self.y_hat


class SoftMixCollate:
    """collate_fn of the reference's DataLoader (distributed_trainer_cls.py:58-62): default_collate, then
    RandomChoice([CutMix(num_classes, alpha=1.0), MixUp(num_classes, alpha=0.8)]) on the batch — torchvision.transforms.v2
    semantics restated (torchvision is not installed here; tests/golden/mix_vectors.json pins them): the partner of
    sample i is sample i-1 (`roll(1, 0)`), lam ~ Beta(alpha, alpha);
      MixUp : x = lam x + (1 - lam) x_rolled,                      y = lam onehot + (1 - lam) onehot_rolled
      CutMix: a box of area ratio (1 - lam) centred at a uniform point, clipped to the image, is pasted from the
              partner; lam is then corrected to 1 - box_area / image_area.
    Host side, float images [B,3,H,W]; `DeviceCollate` is the uint8-on-device form of the same decisions."""

    def __init__(self, num_classes=1000, cutmix_alpha=1.0, mixup_alpha=0.8, seed=None):
        self.num_classes, self.cutmix_alpha, self.mixup_alpha = num_classes, cutmix_alpha, mixup_alpha
        self.seed = seed
        self._rng = None
        self._rng_worker = None

    @property
    def rng(self):
        """The generator of THIS process: DataLoader workers each receive a pickled copy of the collate object, so a
        generator built in __init__ would hand every worker the same (mode, lam, box) sequence.  It is
        created on first use from (seed, worker id) — torchvision's transforms draw from the per-worker-seeded torch RNG
        in the reference (num_workers=5, cls:62)."""
        import numpy as np
        info = torch.utils.data.get_worker_info()
        wid = info.id if info is not None else -1
        if self._rng is None or self._rng_worker != wid:
            self._rng = np.random.default_rng(None if self.seed is None else [int(self.seed), wid + 1])
            self._rng_worker = wid
        return self._rng

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_rng"], st["_rng_worker"] = None, None        # never ship generator state to a worker
        return st

    @staticmethod
    def cutmix_box(lam, cx, cy, H, W):
        """torchvision v2 CutMix._get_params: r = 0.5 sqrt(1 - lam); box = centre -+ (r W, r H) truncated to ints and
        clipped; returns (y1, y2, x1, x2) and the corrected lam."""
        r = 0.5 * (1.0 - lam) ** 0.5
        rw, rh = int(r * W), int(r * H)
        x1, y1, x2, y2 = max(cx - rw, 0), max(cy - rh, 0), min(cx + rw, W), min(cy + rh, H)
        return (y1, y2, x1, x2), 1.0 - (x2 - x1) * (y2 - y1) / float(W * H)

    def mix(self, x, labels, mode, lam, box=None):
        onehot = torch.nn.functional.one_hot(labels, self.num_classes).to(torch.float32)
        xr = x.roll(1, 0)
        if mode == 1:
            out = x * lam + xr * (1.0 - lam)
        else:
            y1, y2, x1, x2 = box
            out = x.clone()
            out[..., y1:y2, x1:x2] = xr[..., y1:y2, x1:x2]
        return out, onehot * lam + onehot.roll(1, 0) * (1.0 - lam)

    def __call__(self, batch):
        x = torch.stack([b[0] for b in batch])
        labels = torch.as_tensor([int(b[1]) for b in batch])
        H, W = x.shape[-2:]
        mode = 2 if self.rng.random() < 0.5 else 1
        alpha = self.cutmix_alpha if mode == 2 else self.mixup_alpha
        lam = float(self.rng.beta(alpha, alpha))
        box = None
        if mode == 2:
            box, lam = self.cutmix_box(lam, int(self.rng.integers(0, W)), int(self.rng.integers(0, H)), H, W)
        return self.mix(x, labels, mode, lam, box)


def load_backbone(model, source, prefix="autoencoder."):
    """Copy every tensor of `source` whose key starts with `prefix` into `model`, in place: the hand-over from a
    `generate=True` model pre-trained with train(task="reg", mim=) to a classifier, which share the backbone
    `ViT.autoencoder` key for key (parameters, spectral-norm `weight_orig` / `weight_u` / `weight_v` and every other buffer).
    source: a state dict, or the path of a checkpoint train() wrote (the `_ema` / `_best` files as well).  The key sets
    under the prefix and all shapes must agree; otherwise ValueError names the first three offenders and nothing is
    copied.  Everything else in `model` (head, pool, proj) is left alone.  Returns {"loaded": keys copied, "ignored": keys
    of the source outside the prefix}."""
    sd = torch.load(source, map_location="cpu") if isinstance(source, (str, os.PathLike)) else source
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError("load_backbone: source is a state dict or the path of one")
    own = model.state_dict()
    mine, theirs = [k for k in own if k.startswith(prefix)], [k for k in sd if k.startswith(prefix)]
    bad = [f"{k} (missing in the source)" for k in mine if k not in sd]
    bad += [f"{k} (not in the model)" for k in theirs if k not in own]
    bad += [f"{k} ({tuple(sd[k].shape)} in the source, {tuple(own[k].shape)} in the model)"
            for k in mine if k in sd and sd[k].shape != own[k].shape]
    if not mine or bad:
        bad = bad or [f"no key of the model starts with {prefix!r}"]
        raise ValueError(f"load_backbone: {len(bad)} mismatch(es) under {prefix!r}: " + "; ".join(bad[:3]))
    with torch.no_grad():
        for k in mine:
            own[k].copy_(sd[k])
    return {"loaded": mine, "ignored": [k for k in sd if not k.startswith(prefix)]}


def _improves(best, name, value, lower):
    """The selection rule of the best checkpoints: True, and best[name] = value, when value strictly beats best[name] —
    lies below it with lower=True, above it otherwise."""
    if (value < best.get(name, float("inf"))) if lower else (value > best.get(name, -1.0)):
        best[name] = value
        return True
    return False


def _val_best_so_far(val_log, key="top1", lower=False):
    """{"top1": best live top-1, "ema_top1": best averaged top-1} from the lines of an existing validation log; with
    key="huber", lower=True the lowest validation Huber of a generative run under "huber" / "ema_huber"."""
    import json
    best = {}
    if os.path.exists(val_log):
        with open(val_log) as f:
            for rec in (json.loads(line) for line in f if line.strip()):
                for name, r in ((key, rec), ("ema_" + key, rec.get("ema"))):
                    if r is not None and key in r:
                        _improves(best, name, r[key], lower)
    return best


class _ClsTask:
    """What train() asks of its job, for the classification job (distillation included: it is this task with another
    step): the step's own keywords, the text of a log_every line behind "Device: [r, l], ", the keywords of the validation
    `evaluate`, its printed report and `best` = (report key, lower is better), the rule of the best checkpoints."""
    name, reg, best = "cls", False, ("top1", False)

    def __init__(self, metrics, topk, loss=None):
        self.step_kw, self.topk = {"metrics": metrics, "loss": loss}, topk
        self.eval_kw = dict(report=True, topk=topk)

    def log_text(self, loss, y_hat, y):                    # (one host read of the accuracy: only on log_every batches)
        correct = (y_hat.reshape(y.shape[0], -1).argmax(1) == y.argmax(1)).sum().item()
        return f"Loss: {float(loss)}, Accuracy: {100.0 * correct / y.size(0):.4f}%"

    def val_text(self, r):
        tops = ", ".join(f"top-{k}: {100.0 * r[f'top{k}']:.4f}%" for k in self.topk)
        return (f"{tops}, Loss: {r['loss']}, Mean per-class accuracy: {100.0 * r['mean_per_class_accuracy']:.4f}%, "
                f"Samples: {r['n']}")


class _RegTask:
    """_ClsTask's counterpart for task="reg": no step metrics, the loss alone in a log line (reg:100), `ReconMetrics` for a
    report and the strictly lower validation Huber for the best checkpoints."""
    name, reg, best = "reg", True, ("huber", True)
    eval_kw = dict(recon=True)

    def __init__(self, kl_weight, mim=None):
        self.step_kw = {"kl_weight": kl_weight, "mim": mim}

    def log_text(self, loss, y_hat, y):
        return f"Loss: {float(loss)}"

    def val_text(self, r):
        return (f"Huber: {r['huber']}, MAE: {r['mae']}, MSE: {r['mse']}, PSNR: {r['psnr']:.4f} dB, SSIM: {r['ssim']}, "
                f"Samples: {r['n']}, Non-finite: {r['nonfinite']}")


_STEP_CLASSES = {("cls", False): TrainStep, ("cls", True): AccumTrainStep, ("reg", False): RegTrainStep,
                 ("reg", True): AccumRegTrainStep, ("distill", False): DistillTrainStep, ("distill", True): AccumDistillTrainStep,
                 ("cls", "sam"): SamTrainStep, ("reg", "sam"): SamRegTrainStep}


def _make_step(task, model, optimizer, reducer, accumulate, teacher, distill_kw, sam_kw=None, **kw):
    """The step of train(): (the task, or "distill" with a teacher) x (accumulate > 1) picks the class; kw are the
    keywords every class takes, the task adds its own, a teacher adds distill_kw, a window adds accumulate=.  sam_kw (the
    normalised sam= of train(), which excludes a teacher and a window): the SharpnessAware is built here and the class is
    the task's two-pass step."""
    kw.update(task.step_kw)
    if sam_kw is not None:
        sam_kw = dict(sam_kw)
        sync = sam_kw.pop("sync")
        return _STEP_CLASSES[task.name, "sam"](model, optimizer, reducer, sam=SharpnessAware(model, optimizer, **sam_kw),
                                               sync=sync, **kw)
    args = (model, optimizer, reducer)
    if teacher is not None:
        args = (model, optimizer, teacher, reducer)
        kw.update(distill_kw)
    if accumulate > 1:
        kw["accumulate"] = accumulate
    return _STEP_CLASSES["distill" if teacher is not None else task.name, accumulate > 1](*args, **kw)


def _validate_epoch(task, model, ema, val_dataset, rank, world, device, batch_size, transform, epoch, n_steps,
                    checkpoint_path, val_log, best, verbose, transform_out="tokens", knn=None):
    """One validation pass of train(): every rank evaluates its shard (live weights, then the averaged ones), the reports
    are all-reduced inside evaluate; the caller's rank 0 passes checkpoint_path / val_log / verbose and does the writing.
    The RNG states and the training flag are as before when it returns.  The task decides what is measured (for "reg" the
    samples' labels are ignored and the report is ReconMetrics.read()), how it is printed and, with task.best, which
    report value the best checkpoint follows."""
    import json
    from torch.utils.data import DataLoader
    use_gpu = device.type == "cuda"
    cpu_rng = torch.get_rng_state()
    dev_rng = torch.cuda.get_rng_state(device) if use_gpu else None
    was_training = model.training
    shard = validation_shard(val_dataset, rank, world)
    collate = RaggedU8Collate() if transform is not None else None

    def batches():
        for batch in DataLoader(shard, batch_size=int(batch_size), shuffle=False, collate_fn=collate, num_workers=0):
            if transform is not None:
                yield batch                                   # (packed, meta, labels): evaluate moves and transforms it
            else:
                x, labels = batch if isinstance(batch, (tuple, list)) else (batch, None)
                yield x.to(device, non_blocking=True), None if labels is None or task.reg else labels.to(device, non_blocking=True)
    try:
        kw = dict(lean=True, autocast_dtype=torch.bfloat16 if use_gpu else None, transform=transform,
                  transform_out=transform_out, **task.eval_kw)
        rep = evaluate(model, batches(), **kw)
        rep_ema = evaluate(model, batches(), ema=ema, **kw) if ema is not None else None
        knn_rep = knn_ema = None
        if knn is not None:
            knn["seen"] += 1
            if knn["seen"] % int(knn["every"]) == 0:
                def labelled(data):                            # (the probe needs the labels a generative validation drops)
                    for batch in DataLoader(data, batch_size=int(knn["batch_size"] or batch_size), shuffle=False,
                                            collate_fn=collate, num_workers=0):
                        yield batch if transform is not None else (batch[0].to(device, non_blocking=True), batch[1].to(device))
                bank = validation_shard(knn["bank"], rank, world)
                knn_kw = dict(k=knn["k"], temperature=knn["temperature"], lean=True, autocast_dtype=kw["autocast_dtype"],
                              transform=transform, transform_out=transform_out)
                knn_rep = knn_evaluate(model, labelled(bank), labelled(shard), knn["num_classes"], **knn_kw)
                if ema is not None:
                    knn_ema = knn_evaluate(model, labelled(bank), labelled(shard), knn["num_classes"], ema=ema, **knn_kw)
    finally:
        torch.set_rng_state(cpu_rng)
        if dev_rng is not None:
            torch.cuda.set_rng_state(dev_rng, device)
        model.train(was_training)
    scalars = lambda r: {k: v for k, v in r.items() if not isinstance(v, torch.Tensor)}
    line = {"epoch": epoch + 1, "step": n_steps, **scalars(rep)}
    if rep_ema is not None:
        line["ema"] = scalars(rep_ema)
    if knn_rep is not None:
        line["knn"] = scalars(knn_rep)
    if knn_ema is not None:
        line["ema"]["knn"] = scalars(knn_ema)
    if verbose:
        for tag, r in (("", rep), (" (EMA)", rep_ema)):
            if r is not None:
                print(f"Epoch: {epoch + 1}, Validation{tag}: {task.val_text(r)}")
        for tag, r in (("", knn_rep), (" (EMA)", knn_ema)):
            if r is not None:
                tops = ", ".join(f"top-{t}: {100.0 * r[f'top{t}']:.4f}%" for t in (1, 5))
                print(f"Epoch: {epoch + 1}, k-NN{tag} (k={r['k']}, T={r['temperature']}): {tops}, Bank: {r['bank']}, "
                      f"Samples: {r['n']}")
    if val_log is not None:
        os.makedirs(os.path.dirname(os.path.abspath(val_log)), exist_ok=True)
        with open(val_log, "a") as f:
            f.write(json.dumps(line) + "\n")
    if checkpoint_path:
        stem, ext = os.path.splitext(checkpoint_path)
        key, lower = task.best
        if _improves(best, key, rep[key], lower):
            torch.save(model.state_dict(), stem + "_best" + ext)
        if rep_ema is not None and _improves(best, "ema_" + key, rep_ema[key], lower):
            torch.save(ema.model_state_dict(), stem + "_ema_best" + ext)
    return line


def _check_train_args(initializer, optimizer, use_gpu, num_classes, device_collate, crop, graph, device_metrics,
                      device_augment, device_resize, resize_window, random_resized_crop, ema, snapshot_path, snapshot_every,
                      accumulate, val_dataset, val_every, val_batch_size, val_transform, val_topk, task, teacher, distill,
                      param_groups, scheduler_step, monitor=None, random_erasing=None, label_smoothing=0.0, rand_augment=None,
                      sam=None, lamb=None, drop_path=None, loss=None, mim=None, knn=None):
    """Every refusal train() makes from its arguments alone: it touches no device and no process group, so a bad call
    fails before either exists.  Returns the normalised values the job is assembled from: accumulate (int), ema_kw
    (None without ema), distill_kw (DistillTrainStep's keywords, {} without a teacher), teacher_mod, resize (the
    DeviceResize or None), window (the DeviceResizedCrop.window or None), reg, per_step, monitor_kw (None without
    monitor=; "every" None: log_every), erase (None, a DeviceErase, or the dict of arguments one is built from),
    label_smoothing (float), rand_augment (None, a DeviceRandAugment, or the dict of arguments one is built from), sam_kw
    (None without sam=; SharpnessAware's keywords and "sync"), lamb (None, or the normalised settings of
    FusedClipAdamW(lamb=) — the argument's, or those of the optimizer object handed in), drop_path (None, or
    {"rate", "schedule"} for set_drop_path), loss (the normalised loss= of TrainStep), mim (None, or the settings of the
    MaskedImageModelling the step is built with)."""
    from . import backend as _backend
    from types import SimpleNamespace
    drop_kw = _drop_path_settings(drop_path)
    loss_kw = _loss_settings("train", loss)
    mim_kw = _mim_settings("train", mim)
    knn_kw = _knn_settings(knn, val_dataset, num_classes)
    if scheduler_step not in ("epoch", "step"):
        raise ValueError(f'train: scheduler_step is "epoch" or "step", got {scheduler_step!r}')
    if param_groups is not None and not (isinstance(optimizer, str) and optimizer == "fused"):
        raise ValueError('train: param_groups= needs optimizer="fused"; build the groups into the optimizer you hand in '
                         "(FusedClipAdamW(groups=) / make_optimizer(groups=))")
    monitor_kw = None
    if monitor is not None and monitor is not False:
        if not ((isinstance(optimizer, str) and optimizer == "fused") or isinstance(optimizer, FusedClipAdamW)):
            raise ValueError('train: monitor= needs optimizer="fused" or a FusedClipAdamW (the monitor reads the fused '
                             "optimizer's table)")
        if monitor is not True and not isinstance(monitor, dict):
            raise ValueError(f'train: monitor is None, True or a dict with "every" / "top" / "per_tensor", got {monitor!r}')
        monitor_kw = {"every": None, "top": 8, "per_tensor": False, **({} if monitor is True else monitor)}
        if set(monitor_kw) != {"every", "top", "per_tensor"}:
            raise ValueError(f'train: monitor takes the keys "every", "top", "per_tensor", got {sorted(monitor)}')
        for key in ("every", "top"):
            v = monitor_kw[key]
            if v is not None and (isinstance(v, bool) or int(v) != v or v < (1 if key == "every" else 0)):
                raise ValueError(f'train: monitor["{key}"] counts {"optimizer steps (>= 1)" if key == "every" else "tensors (>= 0)"}, got {v!r}')
        if monitor_kw["top"] is None:
            raise ValueError('train: monitor["top"] counts tensors (>= 0), got None')
        monitor_kw["per_tensor"] = bool(monitor_kw["per_tensor"])
    sam_kw = None
    if sam is not None and sam is not False:
        if isinstance(sam, dict):
            sam_kw = dict(sam)
        elif not isinstance(sam, bool) and isinstance(sam, (int, float)):
            sam_kw = {"rho": sam}
        else:
            raise ValueError(f'train: sam is None, a radius rho or a dict with "rho" / "adaptive" / "eta" / "eps" / "sync", got {sam!r}')
        if not set(sam_kw) <= {"rho", "adaptive", "eta", "eps", "sync"}:
            raise ValueError(f'train: sam takes the keys "rho", "adaptive", "eta", "eps", "sync", got {sorted(sam_kw)}')
        sam_kw = {"rho": 0.05, "adaptive": False, "eta": 0.01, "eps": 1e-12, "sync": False, **sam_kw}
        rho = sam_kw["rho"]
        if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not (rho > 0.0 and math.isfinite(rho)):
            raise ValueError(f'train: sam["rho"] is a positive finite radius, got {rho!r}')
        if not (isinstance(optimizer, FusedClipAdamW) or (isinstance(optimizer, str) and optimizer == "fused")):
            raise ValueError('train: sam= needs optimizer="fused" or a FusedClipAdamWindow (the perturbation walks the fused '
                             "optimizer's table; a torch optimizer's `.grad`s are not corrected for it)")
        if isinstance(optimizer, FusedClipAdamW) and not isinstance(optimizer, FusedClipAdamWindow):
            raise ValueError('train: sam= needs optimizer="fused" or a FusedClipAdamWindow, not a FusedClipAdamW (the second '
                             "pass's gradients are finished in a window of one while the weights are still perturbed)")
        if graph:
            raise ValueError("train: sam= excludes graph=True (a captured two-pass step is not supported)")
        if int(accumulate) == accumulate and accumulate > 1:
            raise ValueError("train: sam= excludes accumulate > 1 (SAM under an accumulation window is not supported)")
        if teacher is not None:
            raise ValueError("train: sam= excludes teacher= (SAM under distillation is not supported)")
    lamb_kw = _lamb_settings("train", lamb)
    if lamb_kw is not None:
        if not (isinstance(optimizer, FusedClipAdamW) or (isinstance(optimizer, str) and optimizer == "fused")):
            raise ValueError('train: lamb= needs optimizer="fused" or a FusedClipAdamW built with lamb= (the trust ratios are '
                             "taken inside the fused optimizer-side step; a torch optimizer is not given them)")
        if isinstance(optimizer, FusedClipAdamW) and optimizer.lamb != lamb_kw:
            raise ValueError(f"train: lamb={lamb_kw} contradicts the optimizer handed in, which was built with "
                             f"lamb={optimizer.lamb}")
    elif isinstance(optimizer, FusedClipAdamW):
        lamb_kw = optimizer.lamb
    if task not in ("cls", "reg"):
        raise ValueError(f'train: task is "cls" or "reg", got {task!r}')
    reg = task == "reg"
    if reg and loss is not None:
        raise ValueError('train: loss= excludes task="reg" (the generative job\'s loss is Huber + kl_weight * kl)')
    if teacher is not None and loss_kw["name"] != "ce":
        raise ValueError(f"train: teacher= excludes loss={loss!r} (the distillation loss is built on the cross-entropy; BCE "
                         "distillation is not supported)")
    if mim_kw is not None and not reg:
        raise ValueError('train: mim= needs task="reg" (masked image modelling is the generative job\'s pre-training; the '
                         "classifier has no reconstruction target)")
    if reg and graph:
        raise ValueError('train: task="reg" excludes graph=True (GraphedTrainStep captures the classification step)')
    if reg and device_metrics:
        raise ValueError('train: task="reg" excludes device_metrics=True (StepMetrics belongs to the classification loss)')
    generates = getattr(initializer, "generate", None)
    if generates is not None and bool(generates) != reg:
        raise ValueError(f'train: task="{task}" needs a model built with generate={reg}, got generate={bool(generates)}')
    distill_kw = {}
    if distill is not None:
        if teacher is None:
            raise ValueError("train: distill= sets the loss against a teacher; it needs teacher=")
        distill_kw = dict(distill)
        if not set(distill_kw) <= {"alpha", "temperature", "mode", "graph"}:
            raise ValueError(f'train: distill takes the keys "alpha", "temperature", "mode", "graph", got {sorted(distill_kw)}')
    teacher_mod = None
    if teacher is not None:
        teacher_mod = teacher.model if isinstance(teacher, Predictor) else teacher
        if reg:
            raise ValueError('train: teacher= excludes task="reg" (distillation is the classification job\'s loss)')
        if graph:
            raise ValueError("train: teacher= excludes graph=True (the captured step builds its own TrainStep)")
        if getattr(teacher_mod, "generate", False):
            raise ValueError("train: teacher= needs a classifier, got a model built with generate=True")
        distill_kw = {"alpha": float(distill_kw.get("alpha", 0.5)), "temperature": float(distill_kw.get("temperature", 1.0)),
                      "mode": distill_kw.get("mode", "soft"), "teacher_graph": bool(distill_kw.get("graph", False))}
        _check_distill('train: distill["%s"]', distill_kw["mode"], distill_kw["alpha"], distill_kw["temperature"])
    if device_metrics and not (use_gpu and _backend.get_loss_kernels()):
        raise ValueError("device_metrics=True needs use_gpu=True and the loss kernels switched on "
                         "(backend.set_loss_kernels(True) or CALM_LOSS_KERNELS=1)")
    if device_collate and not use_gpu:
        raise ValueError("device_collate=True needs use_gpu=True (the collate is a HIP kernel)")
    if device_augment and not device_collate:
        raise ValueError("device_augment=True needs device_collate=True (the augmentation is part of the collate kernel)")
    resize = window = None
    if device_resize is not None:
        if not device_collate:
            raise ValueError("device_resize=(oh, ow) needs device_collate=True (the resized uint8 batch feeds the collate kernel)")
        resize = DeviceResize(device_resize)               # (refuses a size that is not a pair of sides within 1 .. 16384)
    if resize_window:
        if device_resize is None or crop is None:
            raise ValueError("resize_window=True needs device_resize=(oh, ow) and crop=(H, W): it resizes only the crop window")
        window = DeviceResizedCrop.window(resize.size, crop)    # (refuses a crop that does not fit the resized size)
    if random_resized_crop is not None:
        if not isinstance(random_resized_crop, DeviceResizedCrop) or random_resized_crop.kind != "random_resized":
            raise ValueError("random_resized_crop takes a DeviceResizedCrop.random_resized(...)")
        if not device_collate:
            raise ValueError("random_resized_crop needs device_collate=True (the cropped uint8 batch feeds the collate kernel)")
        if device_resize is not None or crop is not None:
            raise ValueError("random_resized_crop excludes device_resize and crop: it is the crop and the resize")
    erase = None
    if random_erasing is not None and random_erasing is not False:
        if not device_collate:
            raise ValueError("random_erasing needs device_collate=True (the erasing is part of the collate kernel)")
        if reg:
            raise ValueError('train: random_erasing excludes task="reg" (the row tokens are also the Huber target)')
        if isinstance(random_erasing, DeviceErase):
            erase = random_erasing
        elif isinstance(random_erasing, dict):
            erase = dict(random_erasing)
            if not set(erase) <= {"p", "scale", "ratio", "value", "seed"}:
                raise ValueError(f'train: random_erasing takes the keys "p", "scale", "ratio", "value", "seed", got {sorted(erase)}')
            DeviceErase(**erase)                            # (refuses malformed ranges here, not at the first batch)
        elif not isinstance(random_erasing, bool) and isinstance(random_erasing, (int, float)):
            erase = {"p": float(random_erasing)}
            DeviceErase(**erase)
        else:
            raise ValueError("train: random_erasing is a probability, a dict of DeviceErase's arguments or a DeviceErase, "
                             f"got {random_erasing!r}")
    randaug = None
    if rand_augment is not None and rand_augment is not False:
        if not device_collate:
            raise ValueError("rand_augment needs device_collate=True (the stage feeds the collate kernel its uint8 batch)")
        if isinstance(rand_augment, DeviceRandAugment):
            randaug = rand_augment
        elif rand_augment is True or isinstance(rand_augment, dict):
            randaug = {} if rand_augment is True else dict(rand_augment)
            if not set(randaug) <= {"num_ops", "magnitude", "num_bins", "fill", "ops", "seed"}:
                raise ValueError('train: rand_augment takes the keys "num_ops", "magnitude", "num_bins", "fill", "ops", "seed", '
                                 f"got {sorted(randaug)}")
            DeviceRandAugment(**randaug)                    # (refuses malformed arguments here, not at the first batch)
        else:
            raise ValueError("train: rand_augment is None, True, a dict of DeviceRandAugment's arguments or a DeviceRandAugment, "
                             f"got {rand_augment!r}")
        side = crop if crop is not None else device_resize if device_resize is not None else \
            random_resized_crop.size if random_resized_crop is not None else None
        if side is not None and max(side) > 4096:
            raise ValueError(f"train: rand_augment works on windows of at most 4096 x 4096, got {tuple(side)}")
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)) or not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"train: label_smoothing is an epsilon in [0, 1), got {label_smoothing!r}")
    if label_smoothing > 0.0 and reg:
        raise ValueError('train: label_smoothing excludes task="reg" (the generative job has no class targets)')
    if graph and not (use_gpu and (optimizer == "fused" or isinstance(optimizer, FusedClipAdamW))):
        raise ValueError('graph=True needs use_gpu=True and optimizer="fused" (FusedClipAdamW)')
    if int(accumulate) != accumulate or accumulate < 1:
        raise ValueError(f"train: accumulate counts micro-batches per optimizer step (>= 1), got {accumulate!r}")
    accumulate = int(accumulate)
    if accumulate > 1 and graph:
        raise ValueError("train: accumulate > 1 excludes graph=True (capturing an accumulation window is not supported)")
    if accumulate > 1 and isinstance(optimizer, FusedClipAdamW) and not isinstance(optimizer, FusedClipAdamWindow):
        raise ValueError('train: accumulate > 1 needs optimizer="fused" or a FusedClipAdamWindow, not a FusedClipAdamW')
    if snapshot_every is not None and (snapshot_path is None or int(snapshot_every) < 1):
        raise ValueError("snapshot_every counts steps (>= 1) between the snapshots written to snapshot_path")
    ema_kw = None
    if ema is not None:
        ema_kw = dict(ema) if isinstance(ema, dict) else {"decay": float(ema)}
        if not set(ema_kw) <= {"decay", "warmup"} or not 0.0 <= float(ema_kw.get("decay", 0.9999)) < 1.0:
            raise ValueError(f'train: ema takes a decay in [0, 1) or a dict with "decay" / "warmup", got {ema!r}')
    if int(val_every) != val_every or val_every < 1:
        raise ValueError(f"train: val_every counts epochs between validation passes (>= 1), got {val_every!r}")
    if val_transform is not None and not use_gpu:
        raise ValueError("train: val_transform needs use_gpu=True (the validation transform is a HIP kernel)")
    if val_dataset is not None:
        if val_batch_size is not None and (int(val_batch_size) != val_batch_size or val_batch_size < 1):
            raise ValueError(f"train: val_batch_size counts samples (>= 1), got {val_batch_size!r}")
        if not reg and 1 not in tuple(val_topk):
            raise ValueError(f"train: val_topk must contain 1 (the best checkpoint follows top-1), got {val_topk!r}")
        if not reg:
            EvalMetrics(num_classes, topk=val_topk)         # (refuses a malformed val_topk here, not after the first epoch)
    return SimpleNamespace(accumulate=accumulate, ema_kw=ema_kw, distill_kw=distill_kw, teacher_mod=teacher_mod, resize=resize,
                           window=window, reg=reg, per_step=scheduler_step == "step", monitor_kw=monitor_kw, erase=erase,
                           label_smoothing=float(label_smoothing), rand_augment=randaug, sam_kw=sam_kw, lamb=lamb_kw,
                           drop_path=drop_kw, loss=loss_kw, mim=mim_kw, knn=knn_kw)


def _knn_settings(knn, val_dataset, num_classes):
    """knn= of train() -> None, or {"bank", "k", "temperature", "every", "batch_size", "num_classes", "seen"}."""
    if knn is None or knn is False:
        return None
    kw = dict(knn) if isinstance(knn, dict) else {"bank": knn}
    if not set(kw) <= {"bank", "k", "temperature", "every", "batch_size"} or kw.get("bank") is None:
        raise ValueError(f'train: knn takes a bank dataset, or a dict with "bank" (needed), "k", "temperature", "every", '
                         f'"batch_size", got {sorted(kw) if isinstance(knn, dict) else knn!r}')
    if val_dataset is None:
        raise ValueError("train: knn= needs val_dataset (its samples are the queries of the probe)")
    kw = {"k": 20, "temperature": 0.07, "every": 1, "batch_size": None, **kw}
    if not hasattr(kw["bank"], "__len__") or not hasattr(kw["bank"], "__getitem__") or len(kw["bank"]) < 1:
        raise ValueError('train: knn["bank"] is a map-style dataset of (x, integer label) with at least one sample')
    if isinstance(kw["every"], bool) or int(kw["every"]) != kw["every"] or kw["every"] < 1:
        raise ValueError(f'train: knn["every"] counts validation passes between probes (>= 1), got {kw["every"]!r}')
    if kw["batch_size"] is not None and (int(kw["batch_size"]) != kw["batch_size"] or kw["batch_size"] < 1):
        raise ValueError(f'train: knn["batch_size"] counts samples (>= 1), got {kw["batch_size"]!r}')
    KnnProbe(num_classes, k=kw["k"], temperature=kw["temperature"])     # (refuses a bad k / temperature / class count here)
    return {**kw, "num_classes": int(num_classes), "seen": 0}


def _drop_path_settings(drop_path):
    """drop_path= of train() -> None, or {"rate": in [0, 1), "schedule": "linear" | "uniform"}."""
    if drop_path is None or drop_path is False:
        return None
    if isinstance(drop_path, dict):
        if not set(drop_path) <= {"rate", "schedule"} or "rate" not in drop_path:
            raise ValueError(f'train: drop_path takes the keys "rate" (needed) and "schedule", got {sorted(drop_path)}')
        kw = {"schedule": "linear", **drop_path}
    elif not isinstance(drop_path, bool) and isinstance(drop_path, (int, float)):
        kw = {"rate": drop_path, "schedule": "linear"}
    else:
        raise ValueError(f'train: drop_path is None, a rate or a dict with "rate" / "schedule", got {drop_path!r}')
    rate = kw["rate"]
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 <= rate < 1.0:
        raise ValueError(f'train: drop_path["rate"] is a probability in [0, 1), got {rate!r}')
    if kw["schedule"] not in ("linear", "uniform"):
        raise ValueError(f'train: drop_path["schedule"] is "linear" or "uniform", got {kw["schedule"]!r}')
    return {"rate": float(rate), "schedule": kw["schedule"]}


class _TrainInput:
    """The input side of train(): owns the DeviceCollate, the DeviceAugment and the DeviceErase (seeded 2006 + rank) and
    turns a batch of the DataLoader into (x, y) on the device; y is None for reg, and under cls it is smoothed here
    (label_smoothing) behind whichever collate made it.  `collate_fn` is what the DataLoader gets: the caller's
    own, SoftMixCollate for "mix" under cls, None (default_collate) for "mix" under reg and for a stacked uint8 batch,
    RaggedU8Collate in front of a resize stage.

    The draw order is the contract (resume= and the bit-for-bit runs rest on it): the decisions come from
    `DeviceCollate.draw` first and the crop corners second — with a window from `draw_corners` here, otherwise inside
    the collate call.  Under reg the draw is made all the same and then mapped to decisions that mix nothing (MixUp with
    lam = 1), so the generators advance as under cls; the collate gets zero labels and its soft labels are dropped."""

    def __init__(self, device_collate, device_augment, resize, window, random_resized_crop, crop, collate_fn, num_classes,
                 rank, reg, device, random_erasing=None, label_smoothing=0.0, rand_augment=None):
        self.resize, self.window, self.resized_crop, self.crop = resize, window, random_resized_crop, crop
        self.reg, self.device = reg, device
        self.num_classes, self.label_smoothing = num_classes, float(label_smoothing)
        # eps / K as a 0-dim host tensor (it broadcasts against a batch on any device); None: no smoothing, no extra op
        self._smooth = torch.tensor(self.label_smoothing / num_classes, dtype=torch.float32) if self.label_smoothing > 0.0 else None
        self.collate = self.augment = self.erase = self.randaug = None
        if device_collate:
            self.collate = DeviceCollate(num_classes=num_classes, seed=2006 + rank)
            self.augment = DeviceAugment(seed=2006 + rank) if device_augment else None
            if isinstance(random_erasing, DeviceErase):
                self.erase = random_erasing
            elif random_erasing is not None:               # a dict of DeviceErase's arguments (_check_train_args made it)
                self.erase = DeviceErase(**{"seed": 2006 + rank, **random_erasing})
            if isinstance(rand_augment, DeviceRandAugment):
                self.randaug = rand_augment
            elif rand_augment is not None:                  # a dict of DeviceRandAugment's arguments (_check_train_args made it)
                self.randaug = DeviceRandAugment(**{"seed": 2006 + rank, **rand_augment})
            collate_fn = None                               # default_collate: stack uint8 images and labels
            if resize is not None or random_resized_crop is not None:
                collate_fn = RaggedU8Collate()              # images of any size: one packed buffer and its table
        elif collate_fn == "mix":
            collate_fn = None if reg else SoftMixCollate(num_classes=num_classes, seed=2006 + rank)      # reg:58
        self.collate_fn = collate_fn

    def generators(self, num_workers):
        """The numpy generators a snapshot has to hold (TrainState's `generators`)."""
        gens = {}
        if self.collate is not None:
            gens["collate"] = self.collate.rng
            if self.augment is not None:
                gens["augment"] = self.augment.rng
            if self.resized_crop is not None:
                gens["resized_crop"] = self.resized_crop.rng
            if self.erase is not None:
                gens["erase"] = self.erase.rng
            if self.randaug is not None:
                gens["rand_augment"] = self.randaug.rng
        elif isinstance(self.collate_fn, SoftMixCollate) and num_workers == 0:
            gens["mix"] = self.collate_fn.rng
        return gens

    def __call__(self, batch):
        dcoll, device, decisions, crop = self.collate, self.device, None, self.crop
        if self.window is not None:
            packed, meta, y = batch
            decisions = dcoll.draw(len(meta), *self.window.size)       # the order of DeviceCollate.__call__: decisions,
            corners = dcoll.draw_corners(len(meta), *self.resize.size, *self.window.size)      # then corners
            x = self.window(packed.to(device, non_blocking=True), meta, corners=corners)    # only the crop window, uint8
            crop = None                                                # the batch is at the crop size already
        elif self.resized_crop is not None:
            packed, meta, y = batch
            x = self.resized_crop(packed.to(device, non_blocking=True), meta)               # box -> [B,3,H,W] uint8
        elif self.resize is not None:
            packed, meta, y = batch
            x = self.resize(packed.to(device, non_blocking=True), meta)    # packed originals -> [B,3,oh,ow] uint8
        else:
            x, y = batch if isinstance(batch, (tuple, list)) else (batch, None)
            x = x.to(device, non_blocking=True)
        if self.randaug is not None:
            # the decisions and the corners in the collate's own order, then the stage's draws: it crops and flips, and the
            # collate takes its uint8 batch with crop=None and no flips
            B, (Hs, Ws) = x.shape[0], x.shape[-2:]
            H, W = crop if crop is not None else (Hs, Ws)
            if decisions is None:
                decisions = dcoll.draw(B, H, W)
            corners = dcoll.draw_corners(B, Hs, Ws, H, W) if crop is not None else None
            x = self.randaug(x, corners, decisions[3], crop)
            decisions, crop = (*decisions[:3], torch.zeros_like(decisions[3])), None
        if self.reg:                                                   # the labels are ignored (reg:74-77)
            if dcoll is not None:                                      # uint8 batch -> row tokens; the draws as for "cls"
                if decisions is None:
                    decisions = dcoll.draw(x.shape[0], *(crop if crop is not None else x.shape[-2:]))
                x, _ = dcoll(x, torch.zeros(x.shape[0], dtype=torch.int64, device=device),
                             decisions=(1, 1.0, None, decisions[3]), crop=crop, tokens=True, augment=self.augment)
            return x, None
        y = y.to(device, non_blocking=True)
        if dcoll is not None:                                          # uint8 batch -> row tokens + soft labels
            x, y = dcoll(x, y.long(), decisions=decisions, crop=crop, tokens=True, augment=self.augment, erase=self.erase)
        if self._smooth is not None:                                   # y (1 - eps) + eps / K on the soft targets: one op
            if not (y.is_floating_point() and y.dim() == 2 and y.shape[1] == self.num_classes):
                raise ValueError(f"train: label_smoothing acts on soft targets [B, {self.num_classes}], the collate gave "
                                 f"{y.dtype} {tuple(y.shape)}")
            y = torch.add(self._smooth, y, alpha=1.0 - self.label_smoothing)
        return x, y


def _fused_optimizer(model, param_groups, accumulate, verbose, window=False, lamb=None):
    """train(optimizer="fused"): FusedClipAdamW (FusedClipAdamWindow for an accumulation window, or with `window`: sam=
    finishes its second pass's gradients in a window of one) over the model on its
    device, with the groups of param_groups=; the frozen parameters lose requires_grad here, before the reducer and the EMA
    are built.  lamb: FusedClipAdamW's.  verbose: print one line per group."""
    group_kw = {} if lamb is None else {"lamb": lamb}
    if param_groups is not None:
        groups, frozen = _build_param_groups(model, param_groups)
        for p in frozen:                    # before the reducer, the optimizer and the EMA: all three filter on it
            p.requires_grad_(False)
        group_kw["groups"] = groups
    optimizer = FusedClipAdamWindow(model, **group_kw) if accumulate > 1 or window else FusedClipAdamW(model, **group_kw)
    if param_groups is not None and verbose:
        for k, g in enumerate(optimizer.param_groups):
            print(f"Parameter group {k}: {len(g['params'])} tensors, {sum(p.numel() for p in g['params'])} elements, "
                  f"lr {g['lr']}, weight decay {g['weight_decay']}")
    return optimizer


def _capture_step(step, st, model, optimizer, x, y, **kw):
    """The first batch of train(graph=True): the step captured at its shape (the capture's warm-up steps are undone).
    With snapshots, the eager step's growth count moves into the captured one, which keeps its own, and the TrainState
    follows the captured step from here on."""
    gstep = GraphedTrainStep(model, optimizer, x, y, max_norm=1.0, autocast_dtype=torch.bfloat16, restore_after_warmup=True,
                             **kw)
    if st is not None:
        if step._clean_steps is not None:                   # (then the captured step, built alike, has one too)
            gstep.inner._clean_steps.copy_(step._clean_steps)
        st.bind_step(gstep)
    return gstep


def _end_epoch(epoch, i, n_batches, n_steps, y_hat, *, task, model, step, accumulate, scheduler, per_step, ema, metrics,
               dmetrics, who, checkpoint_path, samples_dir, validate, st, snapshot_path):
    """What train() does between the last batch of an epoch and the next epoch, in this order: the incomplete
    accumulation window stepped, the StepMetrics and DistillMetrics lines, the checkpoint (and the EMA's), the samples,
    validation, the per-epoch scheduler step, the epoch-end snapshot.  i: the index of the last batch run (skip - 1 when
    there was none), who: (rank, local_rank, main), validate: (epoch, n_steps) -> None when this epoch is validated.
    Returns n_steps."""
    rank, local_rank, main = who
    if accumulate > 1 and step.flush():     # the epoch's last, incomplete window: stepped before the checkpoint
        n_steps += 1
        if per_step and scheduler is not None:
            scheduler.step()
    if metrics is not None:
        loss_sum, agree, rows, _ = metrics.read()          # the epoch's one device-to-host copy
        metrics.reset()
        if main:
            print(f"Epoch: {epoch + 1}, Device: [{rank}, {local_rank}], Mean loss: {loss_sum / max(rows, 1)}, "
                  f"Dominant-class accuracy: {100.0 * agree / max(rows, 1):.4f}%")
    if dmetrics is not None:
        ce_sum, d_sum, t_agree, t_rows = dmetrics.read()   # one device-to-host copy per epoch
        dmetrics.reset()
        if main and t_rows > 0:
            print(f"Epoch: {epoch + 1}, Device: [{rank}, {local_rank}], Mean CE: {ce_sum / t_rows}, "
                  f"Mean distillation term: {d_sum / t_rows}, Teacher agreement: {100.0 * t_agree / t_rows:.4f}%")
    if main and checkpoint_path:
        os.makedirs(os.path.dirname(os.path.abspath(checkpoint_path)), exist_ok=True)
        torch.save(model.state_dict(), checkpoint_path)                                            # cls:105-107
        if ema is not None:
            stem, ext = os.path.splitext(checkpoint_path)
            torch.save(ema.model_state_dict(), stem + "_ema" + ext)
    if task.reg and samples_dir and main and i >= 0:
        save_samples(y_hat, samples_dir)                                                           # reg:103
    if validate is not None:
        validate(epoch, n_steps)
    if scheduler is not None and not per_step:
        scheduler.step()                                                                           # cls:108-109
    if st is not None and snapshot_path is not None and i + 1 >= n_batches:     # the epoch ran to its end
        st.save_async(snapshot_path, {"epoch": epoch + 1, "batch": 0, "step": n_steps})
    return n_steps


class _MonitorLog:
    """Rank 0's side of train(monitor=): one read of the GradMonitor per line, printed and appended to `path` (None:
    printed only).  A run without resume= starts the file anew."""

    def __init__(self, monitor, path, top, who, fresh=True):
        self.monitor, self.path, self.top, self.who = monitor, path, int(top), who
        self.skipped, self.bad = 0, {}
        if path and fresh and os.path.exists(path):
            os.remove(path)

    @staticmethod
    def _json(v):
        """Strict JSON: a non-finite float becomes null."""
        if isinstance(v, float):
            return v if v == v and abs(v) != float("inf") else None
        if isinstance(v, dict):
            return {k: _MonitorLog._json(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [_MonitorLog._json(x) for x in v]
        return v

    def line(self, epoch, n_steps, per_tensor=False):
        import json
        rep = self.monitor.read()
        tensors = rep["tensors"]
        key = lambda k: lambda n: tensors[n][k] if tensors[n][k] == tensors[n][k] else float("inf")       # noqa: E731
        top = lambda k: [{"name": n, k: tensors[n][k]} for n in sorted(tensors, key=key(k), reverse=True)[:self.top]]  # noqa: E731
        grew = [n for n, t in tensors.items() if t["bad_calls"] > self.bad.get(n, 0)]
        out = dict(epoch=epoch + 1, step=n_steps, norm=rep["norm"], calls=rep["calls"], skipped=rep["skipped"],
                   first_bad=rep["first_bad"], groups=rep["groups"], top_grad_norm=top("grad_norm"),
                   top_update_ratio=top("update_ratio"),
                   nonfinite=[{"name": n, "bad_calls": tensors[n]["bad_calls"], "first_bad_call": tensors[n]["first_bad_call"]}
                              for n in grew])
        trust = None
        if getattr(self.monitor.optimizer, "lamb", None) is not None:      # one read of the optimizer's trust table
            ratios = self.monitor.optimizer.trust_ratios()
            by_trust = sorted(ratios, key=lambda n: ratios[n][2])
            vals = [ratios[n][2] for n in by_trust]
            trust = dict(min=vals[0], median=vals[len(vals) // 2], max=vals[-1])
            out["trust"] = trust
            out["top_small_trust"] = [{"name": n, "trust": ratios[n][2], "weight_norm": ratios[n][0], "update_norm": ratios[n][1]}
                                      for n in by_trust[:self.top]]
        if per_tensor:
            out["tensors"] = tensors
        if self.path:
            os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
            with open(self.path, "a") as f:
                f.write(json.dumps(self._json(out), allow_nan=False) + "\n")
        text = f"Epoch: {epoch + 1}, Step: {n_steps}, Device: [{self.who[0]}, {self.who[1]}], Gradient norm: {rep['norm']:.6g}, " \
               f"Skipped steps: {rep['skipped']}"
        worst = out["top_update_ratio"][:1]
        if worst:
            text += f", Largest update ratio: {worst[0]['update_ratio']:.3g} ({worst[0]['name']})"
        if trust is not None:
            text += f", Trust ratio min / median / max: {trust['min']:.3g} / {trust['median']:.3g} / {trust['max']:.3g}"
        if rep["skipped"] > self.skipped:
            text += f", Non-finite gradient in: {', '.join(grew)}"
        print(text)
        self.skipped = rep["skipped"]
        self.bad = {n: t["bad_calls"] for n, t in tensors.items()}
        return out


def train(initializer, optimizer, scheduler=None, use_gpu=True, dataset=None, epochs=15, batch_size=128,
          checkpoint_path=None, num_classes=1000, num_workers=0, collate_fn="mix", log_every=100, max_steps=None,
          destroy_process_group=True, device_collate=False, crop=None, graph=False, selfcheck="raise",
          device_metrics=False, device_augment=False, device_resize=None, resize_window=False, random_resized_crop=None,
          ema=None, snapshot_path=None, snapshot_every=None, resume=None, accumulate=1, val_dataset=None, val_every=1,
          val_batch_size=None, val_transform=None, val_topk=(1, 5), task="cls", kl_weight=0.1, samples_dir=None,
          teacher=None, distill=None, param_groups=None, scheduler_step="epoch", monitor=None, random_erasing=None,
          label_smoothing=0.0, rand_augment=None, sam=None, lamb=None, drop_path=None, loss=None, mim=None,
          knn=None):
    """Per-rank training job: the reference's `train(initializer, optimizer, scheduler, use_gpu, dataset, epochs,
    batch_size)` (distributed_trainer_cls.py:25-114) on torch.distributed + RCCL instead of Spark's TorchDistributor —
    start one process per GPU with `python -m torch.distributed.run --nproc-per-node N ...` (RANK / LOCAL_RANK /
    WORLD_SIZE from the environment, cls:48-50).

      * init_process_group (nccl on GPUs, gloo on CPU)                                   cls:46
      * CosineAnnealingLR(optimizer, T_max=epochs, eta_min=1e-6), stepped once per epoch  cls:52,108-109
        (scheduler=None / True: built here as the reference does — it builds this schedule whatever it is handed;
        a scheduler OBJECT passed in is kept and stepped instead; scheduler=False: constant rate)
      * model.to(device); parameters + buffers broadcast from rank 0; gradients mean-all-reduced in buckets on a side
        stream (sync_module_states + BucketedGradReducer = what DDP(model) does)          cls:54-55
      * DistributedSampler(dataset, shuffle=True, seed=2006), set_epoch(epoch)           cls:56-57,73
      * DataLoader with the CutMix / MixUp soft-label collate                            cls:58-62
      * per step: autocast(bf16) forward, CE, GradScaler, clip_grad_norm_(1.0), optimizer step, zero_grad   cls:79-96
      * rank 0: loss / dominant-class accuracy print every 100 steps, state_dict checkpoint per epoch      cls:97-107
      * returns the model on the CPU after destroy_process_group()                       cls:112-114

    optimizer: a torch optimizer over `initializer.parameters()` (the reference hands in AdamW(lr=3.1e-3,
    weight_decay=0.02, betas=(0.9, 0.98))), or the string "fused" for FusedClipAdamW with those hyper-parameters (built
    here, after the model is on its device).  checkpoint_path: the reference writes /config/Codebase/models/model_cls.pth.

    device_collate=True: the dataset yields uint8 images [3,Hs,Ws] and integer labels; the DataLoader only
    stacks them (default collate), the uint8 batch goes host-to-device as it is (a quarter of the fp32 bytes) and
    `DeviceCollate` does ToDtype + Normalize + RandomCrop(crop) + flip + CutMix / MixUp in one kernel pass, writing the
    first Block's row tokens [B,S,3S] directly — the model's first Block takes them without the image_to_rows pass
    (cls:58-62,128-139; Vi_Tools:389-391).

    device_augment=True (needs device_collate=True): the colour augmentations of cls:131-135 — ColorJitter, RandomSolarize,
    RandomGrayscale, GaussianBlur — run in that same pass (`DeviceAugment`, seeded 2006 + rank, with the reference's
    ranges) instead of in DataLoader workers; the dataset then yields the resized uint8 images unaugmented.

    device_resize=(oh, ow) (needs device_collate=True): the Resize of cls:129 runs on the device as well.  The dataset
    yields the decoded images as they are, `(uint8 [h, w, 3], label)` of any size; the loader packs a batch into one
    byte buffer (`RaggedU8Collate`), and `DeviceResize` resamples it to [B,3,oh,ow] uint8 with PIL's antialiased
    bilinear arithmetic, bit for bit, in front of the unchanged `DeviceCollate` call.  The run equals the one without
    device_resize on the same images resized by PIL.  None (the default): the dataset yields the resized images.

    resize_window=True (needs device_resize and crop): the decisions and the crop corners of a batch are drawn first, in
    the order `DeviceCollate` draws them, and only the crop window of every resized image is computed
    (`DeviceResizedCrop.window`) — 23 % fewer pixels at 224 of 256 — before the collate takes the batch at the crop size.
    The run equals the one without the flag bit for bit.

    random_resized_crop=DeviceResizedCrop.random_resized(...) (needs device_collate=True; excludes device_resize and
    crop): RandomResizedCrop on the device.  The dataset yields the decoded images as for device_resize; the transform
    draws a box per image from its own generator and hands the collate a batch already at its size.

    selfcheck ("raise" | "fallback" | None; GPU only, once per process): before the first step the box is asked whether
    the two bf16 GEMM families agree on it (HipBackend.selfcheck_bf16_gemm — round 3 saw one box of the pool on which the
    default pipelined family returned a deterministic wrong gradient); "raise" stops the job with the pattern of the
    differing elements, "fallback" warns and trains on the 256x128 family.

    graph=True (GPU, optimizer "fused" / FusedClipAdamW): the step — forward, loss, backward, the bucketed RCCL
    all-reduces of a world > 1, unscale / clip / AdamW — is captured into a hipGraph on the first batch
    (GraphedTrainStep with restore_after_warmup: the capture's warm-up steps are undone) and replayed per batch: one
    graph launch of host work per step instead of ~3000 kernel launches.  The DataLoader then drops the last partial
    batch of an epoch (a graph has one batch shape); a batch of any other shape would run the eager step.

    device_metrics=True (GPU, loss kernels switched on — backend.set_loss_kernels / CALM_LOSS_KERNELS=1): the per-step
    `epoch_loss += loss.item()` of cls:97 — a host sync per step whose sum nothing reads — is dropped; the loss kernel
    accumulates loss and dominant-class agreement in a StepMetrics buffer on the device and rank 0 prints one line per
    epoch from a single read of it.  The log_every lines are unchanged (they synchronise as before).

    ema: a decay (float) or {"decay": ..., "warmup": ...}: a ModelEMA of the model, built after the broadcast of rank 0's
    parameters — every rank then holds the same average without any communication — and updated behind every optimizer
    step (not behind one skipped for inf/NaN gradients).  With checkpoint_path, rank 0 also writes
    `ema.model_state_dict()` beside it as `<stem>_ema<ext>` once per epoch.  The live model is what is returned; the
    ModelEMA is `model._calm_ema` afterwards (on the CPU with the model).

    snapshot_path / snapshot_every / resume (training snapshots, `TrainState`): with snapshot_path, rank 0 writes the
    whole state of the run — model, optimizer, EMA, scaler, scheduler, RNG states, collate / augmentation generators,
    position — to that one file right behind every snapshot_every-th step, at every epoch end and behind the last step
    of a run that max_steps cuts short; the training thread pays one kernel launch per snapshot, the copy and the write
    run beside the following steps.  In a world of more than one rank every rank also writes its own host state (its RNG
    states and generators differ) to `<snapshot_path>.rank<r>.json`; no collective is added.  The per-epoch
    checkpoint_path files are written as before.  resume=path: every rank loads that file (and its sidecar) in place
    before the first step, the loop continues at the saved epoch and batch — the indices of the batches already trained
    on are dropped from the sampler, nothing is loaded and thrown away — and max_steps counts from the restored step.
    The resumed trajectory equals the uninterrupted one bit for bit where the augmentation generators live in the main
    process (device_collate=True, or num_workers=0); the `SoftMixCollate` generators inside persistent DataLoader
    workers are not captured, and a resumed run then draws a fresh stream from them.

    accumulate=k > 1 (gradient accumulation: `AccumTrainStep`, `"fused"` builds a `FusedClipAdamWindow`, the reducer is a
    `HeldGradReducer`; excludes graph=True): every batch of the loader is a micro-batch and every k-th one steps the
    optimizer on the mean of the window's gradients — the effective batch is k * batch_size per rank with the memory of
    one.  max_steps and snapshot_every count OPTIMIZER steps, log_every keeps counting batches.  The incomplete window
    an epoch ends with is stepped (divisor: its own length) before the checkpoint and scheduler.step(), so windows start
    at batch indices that are multiples of k in every epoch.  Snapshots are written only right behind an optimizer step,
    and resume= continues at such a boundary.  The gradients are exchanged once per window.  A window equals the torch
    loop "k x (forward, backward), then unscale / clip / step" with spectral norm iterating at every forward; it does
    not equal one k-times-larger batch.

    val_dataset (validation; yields (x, integer label), or (uint8 [h, w, 3], label) with val_transform): behind every
    val_every-th epoch's checkpoint and in front of scheduler.step() every rank evaluates its `validation_shard` in
    batches of val_batch_size (default: batch_size) through a lean `Predictor` — `evaluate(report=True, lean=True,
    topk=val_topk, transform=val_transform)`, under autocast(bf16) on a GPU as the training forward — and the tallies are
    summed over the ranks.  Rank 0 prints one line (top-k, loss, mean per-class accuracy) and appends one JSON line
    {"epoch", "step", report without the per-class arrays} to `<checkpoint stem>_val.jsonl`; when top-1 strictly
    improves on the best so far it also writes `<stem>_best<ext>`.  With ema, the pass is repeated on the averaged weights
    (`ema.applied()`), logged under "ema", and `<stem>_ema_best<ext>` is kept the same way.  resume= takes the best
    values so far from the existing `_val.jsonl` and appends to it; a run without resume= starts the log anew.  Validation does not move the run: the CPU and device RNG states are
    saved around it and put back and the model is left in training mode, so the returned parameters equal those of the
    same run without val_dataset bit for bit.  val_topk must contain 1; checkpoint_path may be None (nothing is written,
    rank 0 still prints).

    task="reg": the reference's SECOND job, the generative trainer (distributed_trainer_reg.py:25-112), for a
    `generate=True` model: `RegTrainStep` (`AccumRegTrainStep` with accumulate > 1) — HuberLoss(generated image, input) +
    kl_weight * kl (reg:59,78-87) — the default collate without CutMix / MixUp (reg:58; labels, if the dataset yields any,
    are ignored), a log line with the loss alone (reg:100), the checkpoint per epoch (reg:102) and, with samples_dir, rank
    0's `save_samples` of the last batch's generated images behind it (reg:103).  device_collate and everything that
    needs it work as for "cls": the collate is called with decisions that mix nothing — the draws are made as before, so
    the generators advance as they do under "cls", and MixUp with lam = 1 is the identity on a uint8 batch — the soft labels
    are dropped and the row tokens are both the model's input and the Huber target.  ema, snapshots, resume and accumulate
    work as for "cls".  val_dataset runs `evaluate(recon=True, lean=True)` per rank shard, logs the `ReconMetrics`
    scalars and keeps `<stem>_best<ext>` / `<stem>_ema_best<ext>` by strictly LOWER validation Huber (val_topk is not
    used).  graph=True and device_metrics=True are refused (the captured step and the device metrics are the
    classification job's).

    teacher (knowledge distillation; an nn.Module or a `Predictor`, a classifier over the same classes): the step is a
    `DistillTrainStep` (`AccumDistillTrainStep` with accumulate > 1) — the frozen teacher's logits of every batch, image or
    row tokens alike, then `distillation_loss`.  distill: a dict with any of "alpha" (0.5), "temperature" (1.0), "mode"
    ("soft": (1 - alpha) CE + alpha T^2 KL, or "hard": (1 - alpha) CE + alpha CE against the teacher's argmax) and "graph"
    (False; True captures the teacher forward into a hipGraph at the first batch's shape).  The teacher is moved to the
    device and put in eval mode for the run, its parameters and buffers are broadcast from rank 0, and it is handed back
    on the device and in the mode it came in; it is never part of the optimizer, the gradient exchange, the EMA, a
    checkpoint or a snapshot, so resume= needs the same teacher handed in again and then continues bit for bit.  With the
    loss kernels switched on, rank 0 prints one extra line per epoch from a single read of a `DistillMetrics`: mean
    cross-entropy, mean distillation term, agreement with the teacher (of the batches since the epoch began or the run was
    resumed).  The log_every line is unchanged; its loss is the total.  accumulate, ema, device_collate and its
    companions, val_dataset and snapshots work as before.  task="reg", graph=True (the captured step builds its own
    TrainStep), a `generate=True` teacher and distill without teacher are refused.

    param_groups (needs optimizer="fused"): the rules of `param_groups()` — an ordered list of (fnmatch pattern or
    callable, {"lr" | "lr_scale", "weight_decay", "frozen"}) — or the preset "no_decay" (no weight decay on biases, norms,
    scales and inv_freq).  The frozen parameters get requires_grad_(False) before the reducer, the optimizer and the EMA
    are built, so none of the three sees them; FusedClipAdamW / FusedClipAdamWindow is built with the groups and steps
    through calm_optim_step_groups, the scheduler drives every group's rate, and rank 0 prints one line per group
    (tensors, elements, lr, weight decay).  Works with accumulate, ema, graph=True, snapshots / resume= (a snapshot of
    another group count is refused), teacher= and task="reg".  With an optimizer OBJECT it is refused: build the groups
    into the optimizer you hand in (`FusedClipAdamW(groups=)`, `make_optimizer(groups=)`).  Freezing saves no backward
    work: the weight-gradient GEMMs of frozen layers are still computed and autograd drops the result, and the
    spectral-norm power iteration of a frozen layer still advances at every training forward (as torch's does), so its
    u / v / sigma buffers move although `weight_orig` does not.

    scheduler_step="epoch" (the reference: scheduler.step() once per epoch) | "step": scheduler.step() right behind every
    optimizer step — where the step count advances, the end-of-epoch flush of an accumulation window included — and in
    front of that step's snapshot, so a snapshot holds the schedule's position and resume= stays exact; it is then not
    called at the epoch end.  A scheduler built here is CosineAnnealingLR(T_max = epochs * optimizer steps per epoch,
    eta_min=1e-6).  A step skipped for inf/NaN gradients still advances the schedule (torch under a GradScaler: the
    host does not know).

    monitor=True | {"every": n, "top": k, "per_tensor": bool} (needs optimizer="fused" or a FusedClipAdamW; unknown keys
    and every < 1 are refused): a `GradMonitor` is attached to the optimizer, so every optimizer step — eager, windowed
    (then on the window's mean gradient) or captured — runs calm_grad_stats in front of the update on EVERY rank (the
    gradients are equal behind the all-reduce, so the ranks stay in step), without a host synchronisation.  Rank 0 reads it
    every `every` optimizer steps (default: log_every) and at every epoch end, prints one line (gradient norm, skipped
    steps, the largest update-to-weight ratio; when the skipped count grew, the tensors responsible) and appends one JSON
    line to `<checkpoint stem>_grad.jsonl` (checkpoint_path=None: printed only): epoch, step, norm, calls, skipped,
    first_bad, the per-group table, the `top` (default 8) tensors by gradient norm and by update ratio, every tensor with a
    non-finite gradient since the last line, and at the epoch end, with per_tensor, the whole per-tensor table.  A run
    without resume= starts the file anew; the counters are not part of a snapshot, so a resumed run counts anew.  With
    graph=True the counters are cleared behind the capture (its warm-up steps are undone).  The returned model carries the
    monitor as `model._calm_monitor`.  The run's parameters equal those of the same run without monitor=, bit for bit.
    Works with accumulate, param_groups, ema, teacher=, task="reg", graph=True and snapshots / resume=.

    random_erasing (needs device_collate=True; refused under task="reg", whose tokens are also the Huber target) and
    label_smoothing, the regularisers DeiT-style recipes pair with CutMix / MixUp; both default to off.  random_erasing:
    a probability p, a dict of `DeviceErase`'s arguments (p, scale, ratio, value, seed) or a `DeviceErase`; built here it is
    seeded 2006 + rank and owns its generator, so no other draw shifts.  The erasing runs inside the collate kernel
    (calm_augment_collate_erase) behind Normalize and in front of CutMix / MixUp, each partner erased with its own box and
    its own noise, on boxes in the coordinates of the batch the model sees — so it is the same with device_augment,
    device_resize, resize_window and random_resized_crop; without device_augment the collate then runs the augmenting
    kernel on an identity table.  A teacher sees the erased batch the student sees.  The generator is part of a snapshot
    ("erase"), so resume= continues bit for bit, and a snapshot written without random_erasing is refused by a run with it
    (and the other way round).  label_smoothing=eps in [0, 1) (task="cls" only): the soft targets of either collate become
    y (1 - eps) + eps / num_classes — what torch.nn.CrossEntropyLoss(label_smoothing=eps) does to probability targets —
    in one op in front of the step; the loss kernels and the distillation CE take them as they take any soft target, the
    log line's dominant-class accuracy does not move (the argmax is the same), the validation loss is not smoothed, and
    eps = 0 adds no op.

    rand_augment=True | a dict of `DeviceRandAugment`'s arguments (num_ops, magnitude, num_bins, fill, ops, seed) | a
    `DeviceRandAugment` (`DeviceRandAugment.trivial_wide(...)` for TrivialAugmentWide); needs device_collate=True.  The
    RandAugment of the DeiT / timm recipe as a uint8 -> uint8 device stage (calm_randaugment_u8, PIL-exact bytes) between
    the uint8 batch — the dataset's, or the output of device_resize / resize_window / random_resized_crop — and the
    collate.  Built here it is seeded 2006 + rank and owns its generator.  Per batch the collate's decisions and the crop
    corners are drawn first, in the order they are drawn without the stage, then the stage's own draws; the stage crops
    and flips (the reference's order: crop, flip, then the operations) and the collate — with device_augment and
    random_erasing as before — takes its batch with crop=None and no flips.  The generator is part of a snapshot
    ("rand_augment"), so resume= continues bit for bit.  Works with both tasks, accumulate and graph= (the stage runs in
    front of the captured step).  With num_ops=0 the run equals the one without the argument bit for bit; without the
    argument nothing changes.

    sam=rho | {"rho": 0.05, "adaptive": False, "eta": 0.01, "eps": 1e-12, "sync": False} (sharpness-aware minimisation; needs
    optimizer="fused", which then builds a FusedClipAdamWindow, or such an object): the step is a `SamTrainStep`
    (`SamRegTrainStep` under task="reg") over a `SharpnessAware` — per batch a first forward / backward at w,
    calm_sam_perturb (w += rho s / ||s|| along the TRUE gradient, in place, the bits saved; adaptive: ASAM's
    s = (|w| + eta) g), a second forward / backward at the perturbed weights whose gradients calm_grad_accum finishes
    there (a window of one), calm_sam_restore, and the unchanged optimizer-side sequence on those gradients: about two
    plain steps of time.  The loss and output of the log lines, and the device metrics, are the first pass's; EMA, monitor= (it
    sees the second pass's gradients, those applied), val_dataset, param_groups, device_collate and its companions work as
    before.  In a world of more than one rank the reducer is a `HeldGradReducer`: with sync=False (default) the first
    pass's gradients stay on their rank, so each rank perturbs along its own gradient and only the second pass is
    exchanged (the spectral-norm buffers u, v, sigma are then rank-local); sync=True exchanges both.  Either way the
    restored weights are the saved bits, identical on all ranks.
    Spectral norm's power iteration advances at both forwards, and dropout / latent-noise keys are drawn in both.  SAM
    holds no state between steps, so snapshots / resume= stay bit for bit.  The returned model carries the SharpnessAware
    as `model._calm_sam`.  Refused: graph=True, accumulate > 1, teacher=, unknown keys, rho <= 0, a torch optimizer or a
    FusedClipAdamW without the window.

    lamb=True | {"trust_clip": None, "always_adapt": False} (the large-batch optimizer of DeiT III / timm's `lamb`; needs
    optimizer="fused", which is then built with it, or a FusedClipAdamW / FusedClipAdamWindow built with the same lamb=): the
    optimizer-side step is calm_optim_step_lamb — AdamW's moments, clip and inf check, and per tensor
    w -= lr trust (Adam direction + weight_decay w) with trust = ||w|| / ||update||, 1 for tensors without weight decay
    unless always_adapt, at most trust_clip.  It is the optimizer's step, so graph=True, accumulate, sam=, ema,
    param_groups / scheduler_step, teacher=, task="reg", monitor= and snapshots / resume= work as before; the optimizer
    state is AdamW's, and a snapshot written with lamb= is refused by a run without it (and the other way round).  With
    monitor= each line also carries the minimum, median and maximum trust ratio and the `top` tensors by smallest trust; the
    update-ratio fields keep their meaning (the AdamW direction at the group's rate) — under LAMB the APPLIED ratio
    ||dw|| / ||w|| of an adapted, unclipped tensor is its lr by construction.  Rank 0 prints one line with the settings, and
    the returned model carries the optimizer as `model._calm_lamb` (`trust_ratios()`).  Refused: unknown keys,
    trust_clip <= 0, a torch optimizer, an optimizer object whose lamb setting differs from the argument.

    drop_path=rate | {"rate": r, "schedule": "linear" | "uniform"} (stochastic depth: timm's `drop_path_rate`, the
    regulariser of the DeiT / DeiT III recipes; no counterpart in the reference): `set_drop_path(model, rate, schedule)`
    before the step is built, so VMLA_Block i of n drops each of its two residual branches per sample with probability
    rate i / (n - 1) ("linear") or rate ("uniform") — skip + drop_path(dropout(ls branch)) through calm_drop_path, the mask
    regenerated in the backward from a 16-byte key drawn on the device.  It needs no particular optimizer and works with
    graph=True (every replay draws new masks), accumulate, sam= (the two passes draw DIFFERENT masks, as they do for
    dropout: the perturbation is taken on one sub-network and the step on another), lamb=, ema, teacher= (the teacher runs
    in eval mode and is not dropped), task="reg", monitor=, device_collate and its companions.  Validation and eval run the
    full network.  The keys come from torch's device generator, whose state a snapshot holds: resume= continues bit for
    bit; the snapshot's header records the per-block rates, and a snapshot written with rates is refused by a run with
    other rates or none (and the other way round).  Rank 0 prints one line with the schedule and the lowest / highest
    rate, and the returned model keeps its rates.  Refused: unknown keys, a rate outside [0, 1), an unknown schedule.

    loss=None | "ce" | "bce" | {"name": "bce", "target_threshold": None, "sum_classes": False} (the training loss of the
    classification job; None / "ce": the reference's soft-target cross-entropy): "bce" is the binary cross-entropy with
    logits that DeiT III / timm's `BinaryCrossEntropy` train with on the same CutMix / MixUp soft targets —
    `soft_target_bce`, the mean over all B * C elements (torch.nn.BCEWithLogitsLoss()), or with sum_classes the sum over
    the classes and the mean over the batch; target_threshold=t trains against (y > t).  With the loss kernels switched on
    the step runs calm_bce_fwd / _bwd, and device_metrics=True reads the same buffer: the epoch line's mean loss is the
    mean of the printed BCE, its dominant-class accuracy is taken against the targets as they came.  label_smoothing stays
    the one op in front of the step — y (1 - eps) + eps / num_classes is exactly what timm's BinaryCrossEntropy(smoothing=
    eps) does to its targets.  The log_every line and its dominant-class accuracy are unchanged.  Validation
    (evaluate(report=True)) keeps reporting the softmax cross-entropy of the logits, whatever the training loss.  It is the
    step's loss, so graph=True, accumulate, sam=, lamb=, ema, param_groups, monitor=, drop_path=, device_collate and its
    companions and snapshots work as before; the setting has no state and is not part of a snapshot: resume= needs the
    same loss= handed in again, as it needs the same teacher=.  Rank 0 prints one line naming the loss and its options
    when it is not the cross-entropy.  Refused: an unknown name or key, a threshold that is not finite, a sum_classes that
    is not a bool, task="reg" (any loss=), teacher= with "bce" (the distillation loss is built on the cross-entropy).

    mim=True | ratio | {"patch": 32, "ratio": 0.6, "fill": 0.0} | a `MaskedImageModelling` (masked image modelling, SimMIM /
    MAE style; needs task="reg"; no counterpart in the reference): the step is built with `RegTrainStep(mim=)` — per batch a
    mask with exactly k = round(ratio * P) of the P = (S / patch)^2 patches of every sample (calm_mim_draw, from a 16-byte
    key drawn on the device), the masked row tokens as the model's input (calm_mim_apply; `fill` in normalised space, a
    float or one per channel), and Huber(tokens, CLEAN tokens) over the masked patches alone + kl_weight * kl
    (calm_mim_huber_fwd / _bwd with the loss kernels on).  Reconstructing what the skips of the encoder-decoder hand
    through teaches the backbone little; predicting what was removed does.  An image batch is brought to row tokens once;
    device_collate and its companions, accumulate (a mask per micro-batch), sam= (a mask per pass), lamb=, ema,
    param_groups, monitor=, drop_path= and snapshots work as before.  The key comes from torch's device generator, whose
    state a snapshot holds, so resume= continues bit for bit; the snapshot's header records the settings only when mim is
    on, and a snapshot written with settings is refused by a run with others or none (and the other way round).
    Validation keeps reporting `ReconMetrics` on the UNMASKED input.  The log line is unchanged (its loss is the masked
    one); rank 0 prints one line with the settings.  `load_backbone(classifier, checkpoint)` then hands the pre-trained
    `autoencoder.*` tensors to a classifier for fine-tuning.  Refused: task="cls", unknown keys, a ratio outside (0, 1), a
    patch that is not a positive int; an image side that is no multiple of the patch, or more than 32 patches per row, at
    the first batch.

    knn=bank_dataset or {"bank": dataset, "k": 20, "temperature": 0.07, "every": 1, "batch_size": None} (needs val_dataset):
    a weighted k-NN probe of the frozen backbone features (`knn_evaluate`, `KnnProbe`) behind the validation report, on every
    `every`-th validation pass, for the live weights and for the averaged ones — what a pre-training run (task="reg",
    mim=) otherwise only learns from a fine-tuning.  The bank yields what val_dataset yields ((x, integer label);
    val_transform applies to both), each rank embeds its `validation_shard` of the bank and of the queries, the bank is
    gathered into dataset order, so the result does not depend on the world size.  Rank 0 prints `Epoch: e, k-NN (k=20,
    T=0.07): top-1: ...%, top-5: ...%, Bank: N, Samples: n`; the validation log line gains "knn": {...} and "ema": {...,
    "knn": {...}}.  The best-checkpoint rule does not change and training is untouched: the parameters equal those of
    the same run without knn= bit for bit."""
    from functools import partial
    from torch.utils.data import DataLoader, DistributedSampler
    from . import backend as _backend
    args = _check_train_args(initializer, optimizer, use_gpu, num_classes, device_collate, crop, graph, device_metrics,
                          device_augment, device_resize, resize_window, random_resized_crop, ema, snapshot_path,
                          snapshot_every, accumulate, val_dataset, val_every, val_batch_size, val_transform, val_topk, task,
                          teacher, distill, param_groups, scheduler_step, monitor, random_erasing, label_smoothing, rand_augment,
                          sam, lamb, drop_path, loss, mim, knn)
    accumulate, per_step, teacher_mod = args.accumulate, args.per_step, args.teacher_mod
    rank, local_rank, world = init_distributed(use_gpu)
    main = rank == 0 and local_rank == 0                    # the one process that prints and writes
    if val_dataset is not None and len(val_dataset) < world:
        raise ValueError(f"train: val_dataset holds {len(val_dataset)} samples, fewer than the {world} ranks")
    device = torch.device(f"cuda:{local_rank}" if use_gpu else "cpu")
    if use_gpu:
        torch.cuda.set_device(device)
    if use_gpu and selfcheck:
        be = _backend.get_backend()
        if not getattr(be, "_selfcheck_done", False):
            be.selfcheck_bf16_gemm(on_mismatch=selfcheck)
            be._selfcheck_done = True
            torch.cuda.empty_cache()
    model = initializer.to(device)
    if args.drop_path is not None:
        from .Vi_Tools_CNN_less_V2 import set_drop_path
        rates = [r for _, r in set_drop_path(model, args.drop_path["rate"], args.drop_path["schedule"])]
        if main:
            print(f"drop_path: {args.drop_path['schedule']} over {len(rates)} blocks, rates {min(rates, default=0.0):.4f} .. "
                  f"{max(rates, default=0.0):.4f}")
    if args.mim is not None and main:
        print(f"mim: patch {args.mim['patch']}, ratio {args.mim['ratio']:.4f}, fill {args.mim['fill']}")
    if isinstance(optimizer, str) and optimizer == "fused":
        optimizer = _fused_optimizer(model, param_groups, accumulate, verbose=main, window=args.sam_kw is not None,
                                     lamb=args.lamb)
    if args.lamb is not None and main:
        print(f"LAMB: per-tensor trust ratios on, trust_clip {args.lamb['trust_clip']}, always_adapt {args.lamb['always_adapt']}")
    if (scheduler is None or scheduler is True) and not per_step:
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=epochs, eta_min=1e-6)      # cls:52
    elif scheduler is False:
        scheduler = None
    sync_module_states(model)
    mon = mon_log = None
    if args.monitor_kw is not None:
        mon = GradMonitor(model, optimizer).attach()        # every rank runs the kernels; rank 0 alone reads
        mon_every = int(args.monitor_kw["every"] or log_every)
        mon_log = _MonitorLog(mon, os.path.splitext(checkpoint_path)[0] + "_grad.jsonl" if checkpoint_path else None,
                              args.monitor_kw["top"], (rank, local_rank), fresh=resume is None) if main else None
    dmetrics = None
    if teacher_mod is not None:
        teacher_home = (next(iter(teacher_mod.parameters())).device, teacher_mod.training)
        teacher_mod.to(device).eval()
        sync_module_states(teacher_mod)
        dmetrics = DistillMetrics(device) if _backend.get_loss_kernels() else None
    ema_obj = ModelEMA(model, **args.ema_kw) if ema is not None else None
    held = accumulate > 1 or args.sam_kw is not None        # (SamTrainStep exchanges a window of one: reduce_held)
    reducer = (HeldGradReducer(model) if held else BucketedGradReducer(model)) if world > 1 else None
    if world > 1:
        sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True, seed=2006)       # cls:56
    else:
        sampler = DistributedSampler(dataset, num_replicas=1, rank=0, shuffle=True, seed=2006)
    sampler.set_epoch(0)
    inp = _TrainInput(device_collate, device_augment, args.resize, args.window, random_resized_crop, crop, collate_fn, num_classes,
                      rank, args.reg, device, random_erasing=args.erase, label_smoothing=args.label_smoothing,
                      rand_augment=args.rand_augment)
    loader_kw = dict(batch_size=batch_size, collate_fn=inp.collate_fn, num_workers=num_workers, pin_memory=use_gpu,
                     drop_last=bool(graph))
    loader = DataLoader(dataset, sampler=sampler, persistent_workers=num_workers > 0, **loader_kw)
    if per_step and (scheduler is None or scheduler is True):       # one schedule position per optimizer step
        steps_per_epoch = -(-len(loader) // accumulate)
        scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=max(epochs * steps_per_epoch, 1), eta_min=1e-6)
    scaler = torch.amp.GradScaler("cuda", enabled=use_gpu)                                                 # cls:64
    metrics = StepMetrics(device) if device_metrics else None
    job = _RegTask(kl_weight, args.mim) if args.reg else _ClsTask(metrics, val_topk, args.loss)
    if args.loss["name"] != "ce" and main:
        print(f"loss: binary cross-entropy with logits, target_threshold {args.loss['target_threshold']}, "
              f"sum_classes {args.loss['sum_classes']}")
    step = _make_step(job, model, optimizer, reducer, accumulate, teacher, {**args.distill_kw, "distill_metrics": dmetrics},
                      max_norm=1.0, scaler=scaler if use_gpu else None, autocast_dtype=torch.bfloat16 if use_gpu else None,
                      ema=ema_obj, sam_kw=args.sam_kw)
    model.train()
    n_steps = 0
    gstep = None
    st = None
    start_epoch = start_batch = 0
    if snapshot_path is not None or resume is not None:
        st = TrainState(model, optimizer, scaler=scaler if use_gpu else None, scheduler=scheduler, ema=ema_obj, step=step,
                        metrics=metrics, generators=inp.generators(num_workers), payload=main,
                        sidecar_rank=rank if world > 1 else None)
    validate = None
    if val_dataset is not None:
        val_log = os.path.splitext(checkpoint_path)[0] + "_val.jsonl" if checkpoint_path else None
        val_best = _val_best_so_far(val_log, *job.best) if resume is not None and val_log else {}
        if resume is None and val_log and main and os.path.exists(val_log):
            os.remove(val_log)                              # a new run starts its own log; a resumed one appends
        validate = partial(_validate_epoch, job, model, ema_obj, val_dataset, rank, world, device,
                           val_batch_size or batch_size, val_transform, checkpoint_path=checkpoint_path if main else None,
                           val_log=val_log if main else None, best=val_best, verbose=main,
                           transform_out="tokens" if device_collate or not args.reg else "image", knn=args.knn)
    try:
        if resume is not None:
            progress = st.load(resume)
            start_epoch, start_batch, n_steps = progress["epoch"], progress["batch"], progress["step"]
        for epoch in range(start_epoch, epochs):
            sampler.set_epoch(epoch)
            model.train()
            epoch_loss = 0.0
            skip = start_batch if epoch == start_epoch else 0
            epoch_loader = loader
            if skip:                                # the rest of the epoch the saved run was in: indices dropped, not data
                epoch_loader = DataLoader(dataset, sampler=resume_tail(sampler, skip, batch_size), **loader_kw)
            batches = iter(epoch_loader)
            if skip:
                st.reapply_rng()                    # (the iterator drew its base seed; the saved run had drawn it before)
            n_batches = skip + len(epoch_loader)
            i, y_hat = skip - 1, None
            for i, batch in enumerate(batches, start=skip):
                x, y = inp(batch)
                if graph and gstep is None:
                    gstep = _capture_step(step, st, model, optimizer, x, y, scaler=scaler, reducer=reducer, metrics=metrics,
                                          ema=ema_obj, loss=args.loss)
                    if mon is not None:
                        mon.reset()                 # the capture's warm-up steps were undone: they are not counted
                if gstep is not None and x.shape == gstep.x.shape and y.shape == gstep.y.shape:
                    loss, y_hat = gstep(x, y)
                else:
                    loss, y_hat = step(x, y)
                stepped = accumulate == 1 or step.boundary          # accumulate > 1: a window's last micro-batch steps
                n_steps += int(stepped)
                if stepped and per_step and scheduler is not None:
                    scheduler.step()                # in front of this step's snapshot: it holds the schedule's position
                if mon_log is not None and stepped and n_steps % mon_every == 0:
                    mon_log.line(epoch, n_steps)
                done = stepped and max_steps is not None and n_steps >= max_steps
                if st is not None:                  # right behind the step, before anything else touches state
                    if stepped and snapshot_path is not None and ((snapshot_every and n_steps % int(snapshot_every) == 0)
                                                                  or (done and i + 1 < n_batches)):
                        st.save_async(snapshot_path, {"epoch": epoch, "batch": i + 1, "step": n_steps})
                    st.poll()
                if metrics is None:
                    epoch_loss += loss.item()                                                              # cls:97
                if main and i % log_every == 0:                                                    # cls:98-104, reg:100
                    print(f"Epoch: {epoch + 1}, Batch: {i + 1}, Device: [{rank}, {local_rank}], "
                          f"{job.log_text(loss, y_hat, y)}")
                if done:
                    break
            validating = validate is not None and (epoch + 1) % int(val_every) == 0
            n_steps = _end_epoch(epoch, i, n_batches, n_steps, y_hat, task=job, model=model, step=step,
                                 accumulate=accumulate, scheduler=scheduler, per_step=per_step, ema=ema_obj, metrics=metrics,
                                 dmetrics=dmetrics, who=(rank, local_rank, main), checkpoint_path=checkpoint_path,
                                 samples_dir=samples_dir, validate=validate if validating else None, st=st,
                                 snapshot_path=snapshot_path)
            if mon_log is not None:                 # behind the flushed window: the epoch's last step is in the report
                mon_log.line(epoch, n_steps, per_tensor=args.monitor_kw["per_tensor"])
            if max_steps is not None and n_steps >= max_steps:
                break
    finally:
        if st is not None:                 # the last snapshot is in place before the graph and the process group go
            st.close()
        if gstep is not None:              # the captured graph holds RCCL kernels: released before the process group
            gstep = None
            import gc
            gc.collect()
            torch.cuda.synchronize()
        if isinstance(optimizer, FusedClipAdamW):
            optimizer.close()
        if teacher_mod is not None:        # handed back where and as it came in
            if isinstance(step.teacher, Predictor) and step.teacher is not teacher:
                step.teacher.close()
            teacher_mod.to(teacher_home[0]).train(teacher_home[1])
    model = model.to("cpu")                                                                                # cls:112
    if ema_obj is not None:
        ema_obj.rebind()                   # the averages follow the parameters to the CPU
        model._calm_ema = ema_obj
    if mon is not None:
        mon.detach()
        model._calm_monitor = mon
    if args.sam_kw is not None:
        model._calm_sam = step.sam
    if args.lamb is not None:
        model._calm_lamb = optimizer
    if destroy_process_group and dist.is_initialized():
        dist.destroy_process_group()
    return model
