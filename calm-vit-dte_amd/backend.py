"""Tensor-level front of the C-ABI: turns torch tensors into raw device pointers and enqueues the
HIP kernels of libcalmvit_hip.so on torch's current HIP stream.  PyTorch is only the allocator
and stream provider here.

`get_backend()` returns the one product backend (HipBackend) and raises if the library cannot be
loaded; HipBackend rejects non-CUDA tensors.  `use_backend()` exists so that tests/ can check the
host-side autograd plumbing against a torch emulation of the C-ABI kept under tests/ — nothing
in the package ever installs another backend.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import ACT_GELU, ACT_GELU_BWD, ACT_NONE  # noqa: F401  (re-exported)

SN_EPS = 1e-12

# calm_gemm_args.dtype (include/calm_vit.h): which matrix pipe the GEMMs use.  Tensors are fp32 in every mode.
GEMM_WORKSPACE = os.environ.get("CALM_GEMM_WORKSPACE", "1") != "0"      # A/B switch: 0 = split launches always use atomics
BF16_STORAGE = os.environ.get("CALM_BF16_STORAGE", "1") != "0"          # A/B switch: 0 = fp32 tensors in bf16 mode too
PRECISIONS = {"fp32": 0, "bf16": 1, "bf16x3": 2, "fp8": 1}     # calm_gemm_args.dtype; "fp8" = the bf16 pipeline with the
                                                                # forward / input-gradient Linear GEMMs on fp8 operands
FP8_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)
_precision = "fp32"


def set_matmul_precision(name):
    """'fp32'   exact fp32 MFMA (default; BASELINE config #2, parity 1e-3 rel fp32 with margin 1e3)
    'bf16'   bf16 operands, fp32 accumulate (autocast(bfloat16) arithmetic; BASELINE configs #3-#5)
    'bf16x3' bf16 hi/lo split, 3 MFMA passes: fp32-level results (~1e-5) on the bf16 matrix pipe
    'fp8'    the bf16 pipeline with the forward and input-gradient products of the large Linear layers on per-tensor
             scaled OCP fp8 operands (e4m3 activations / weights, e5m2 gradients; BASELINE config #5); weight gradients,
             attention and everything else as in 'bf16'"""
    global _precision
    if name not in PRECISIONS:
        raise ValueError(f"unknown matmul precision {name!r}; choose from {sorted(PRECISIONS)}")
    _precision = name


def get_matmul_precision():
    return _precision


# What the fp32 attention keeps for its backward: "probs" = the probabilities P [B,H,Sq,Skv] (default), "lse" = the row
# log-sum-exp [B,H,Sq]; the backward then rebuilds P in a transient scratch (ops.LatentMaskAttentionLseFn).
ATTENTION_STORAGES = ("probs", "lse")


def _check_attention_storage(name):
    if name not in ATTENTION_STORAGES:
        raise ValueError(f"unknown attention storage {name!r}; choose from {sorted(ATTENTION_STORAGES)}")
    return name


_attention_storage = _check_attention_storage(os.environ.get("CALM_ATTN_STORAGE") or "probs")   # read once, at import


def set_attention_storage(name):
    """'probs' the fp32 attention saves its probabilities for the backward (default)
    'lse'   it saves the row log-sum-exp instead and the backward recomputes the probabilities: less memory held
            between forward and backward, one more Q K^T per head in the backward.  Shapes without a fused kernel
            (HipBackend.attn_fwd_supported) and the bf16 attention are unaffected."""
    global _attention_storage
    _attention_storage = _check_attention_storage(name)


def get_attention_storage():
    return _attention_storage


# Lean inference forward: under torch.no_grad() the attention stores nothing for a backward that will not run
# (calm_attention_infer / calm_attention16_infer) and the GELU GEMMs request no pre-activation.  Off by default.
_lean_inference = os.environ.get("CALM_LEAN_INFERENCE", "0") not in ("", "0")    # read once, at import


def set_lean_inference(on):
    """True: forwards that run with grad disabled take the lean kernels (ops.latent_mask_attention_infer; MlpFn and
    SNLinearFn without C_pre): same outputs bit for bit, none of the tensors only a backward reads.  With grad enabled
    nothing changes, whatever the switch says.  False (default): every forward is the training forward."""
    global _lean_inference
    _lean_inference = bool(on)


def get_lean_inference():
    return _lean_inference


def lean_forward():
    """Whether a forward issued now is a lean one: the switch is on and autograd records nothing."""
    return _lean_inference and not torch.is_grad_enabled()


# The loss end of the step on the library's own kernels (csrc/loss.hip) instead of stock torch: off by default.
_loss_kernels = os.environ.get("CALM_LOSS_KERNELS", "0") not in ("", "0")        # read once, at import


def set_loss_kernels(on):
    """True: trainer.soft_target_cross_entropy / RegTrainStep / evaluate run calm_soft_ce_* / calm_huber_tokens_* /
    calm_top1_count, and EvalMetrics runs calm_eval_metrics, where their conditions hold (fp32 CUDA tensors, for
    calm_eval_metrics bf16 as well; see trainer.py).  False (default): stock torch,
    bit for bit what the step computed before the kernels existed."""
    global _loss_kernels
    _loss_kernels = bool(on)


def get_loss_kernels():
    return _loss_kernels


# Weight-gradient GEMMs of a backward on the library's side lane (calm_gemm_lane; ops._lin_wgrad): on by default (Small-224
# fp32: -1.8 ms of a 128.8 ms step, DESIGN.md section 7, "Weight-gradient lane").  CALM_WGRAD_LANE=0 is the A/B switch,
# read once, at import.
_wgrad_lane = os.environ.get("CALM_WGRAD_LANE", "1") != "0"


def set_wgrad_lane(on):
    """True: while the gradient tail is armed (the trainer's step classes), the weight-gradient GEMMs whose first reader
    is the optimizer-side step are issued on a second, lowest-priority stream the library owns and joined before the
    backward ends.  Same plans, same kernels: with CALM_GEMM_OPT_DETERMINISTIC the step is bit for bit the step without
    the lane.  Inside a graph capture the lane is off whatever the switch says.  False: one stream."""
    global _wgrad_lane
    _wgrad_lane = bool(on)
    if isinstance(_backend, HipBackend):
        _backend.gemm_set_option(HipBackend.GEMM_OPT_LANE, int(_wgrad_lane))


def get_wgrad_lane():
    return _wgrad_lane


def wgrad_lane():
    """Whether ops._lin_wgrad may use the side lane now."""
    return _wgrad_lane


def loss_kernels_take(t):
    """Whether the loss kernels serve tensor `t` now: the switch is on and `t` is an fp32 tensor the installed backend
    can address (HipBackend: CUDA tensors only)."""
    return _loss_kernels and t.dtype == torch.float32 and (t.is_cuda or not isinstance(get_backend(), HipBackend))


def eval_kernels_take(t):
    """Whether calm_eval_metrics serves logits `t` now (trainer.EvalMetrics): as loss_kernels_take, and bf16 as well."""
    return (_loss_kernels and t.dtype in (torch.float32, torch.bfloat16)
            and (t.is_cuda or not isinstance(get_backend(), HipBackend)))


def knn_kernels_take(t):
    """Whether the calm_knn kernels serve features `t` (trainer.KnnProbe): fp32 or bf16, on a device the installed backend
    can address (HipBackend: CUDA tensors only).  Anything else goes to the torch twins."""
    return t.dtype in (torch.float32, torch.bfloat16) and (t.is_cuda or not isinstance(get_backend(), HipBackend))


@contextlib.contextmanager
def fp32_matmul():
    """GEMMs issued inside run on the exact fp32 pipe whatever set_matmul_precision / an enclosing autocast say (the k-NN
    probe's similarities: ties are decided on their bits)."""
    global _precision
    old, _precision = _precision, "fp32"
    try:
        with torch.autocast("cuda", enabled=False):
            yield
    finally:
        _precision = old


def recon_kernels_take(tokens, target):
    """Whether calm_recon_metrics serves this pair now (trainer.ReconMetrics): the switch is on, the generated tokens are
    fp32 or bf16, the target is fp32, and the installed backend can address both."""
    return eval_kernels_take(tokens) and target.dtype == torch.float32 and target.device == tokens.device


def effective_precision():
    """The pipe a GEMM issued now runs on.  Inside `torch.autocast("cuda", dtype=torch.bfloat16)` — how the reference
    trainer calls the model (distributed_trainer_cls.py:84-85) — Linear/matmul operands are rounded to bf16 with fp32
    accumulation, i.e. the 'bf16' mode; activations and parameters stay fp32 tensors.  Outside autocast: the mode
    chosen with set_matmul_precision."""
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if dt != torch.bfloat16:
            raise NotImplementedError(f"autocast dtype {dt} is not supported on this path (the reference uses bfloat16)")
        return "bf16"
    return "bf16" if _precision == "fp8" else _precision


def fp8_linears():
    """True when the Linear layers' forward / input-gradient GEMMs are to run on fp8 operands (set_matmul_precision('fp8');
    also inside autocast(bfloat16), which then selects the bf16 pipeline around them)."""
    return _precision == "fp8" and BF16_STORAGE


def _ptr(t, allow_none=False, bf16_ok=False, fp8_ok=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError("required tensor is None")
    if not t.is_cuda:
        raise RuntimeError("CALM-ViT ops run only on the MI355X HIP path: got a CPU tensor "
                           "(there is no CPU fallback; move the model and inputs to 'cuda')")
    if t.dtype != torch.float32 and not (bf16_ok and t.dtype == torch.bfloat16) and not (fp8_ok and t.dtype in FP8_DTYPES):
        raise TypeError(f"fp32 tensor expected, got {t.dtype}")
    return t.data_ptr()


def _ptr16(t):
    if t is None or not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous():
        raise TypeError("contiguous bf16 CUDA tensor expected")
    return t.data_ptr()


_ST_OF = {torch.bfloat16: _lib.ST_BF16, torch.float8_e4m3fn: _lib.ST_FP8_E4M3, torch.float8_e5m2: _lib.ST_FP8_E5M2}


def _st(t):
    """CALM_ST_* storage type of a tensor argument (None -> fp32)."""
    if t is None:
        return _lib.ST_F32
    return _ST_OF.get(t.dtype, _lib.ST_F32)


def bf16_pipeline():
    """True when activations that only GEMMs consume are to be kept as bf16 tensors: the bf16 matrix pipe is selected
    (autocast(bfloat16) or set_matmul_precision('bf16')) and the pipeline is not switched off (CALM_BF16_STORAGE=0:
    fp32 tensors, operands rounded while staged — the A/B switch)."""
    return BF16_STORAGE and effective_precision() == "bf16"


def act_dtype(last_dim):
    """Storage type for a GEMM-only activation whose contiguous extent is `last_dim` (bf16 rows are staged as 16-byte
    vectors of 8 elements)."""
    return torch.bfloat16 if bf16_pipeline() and last_dim % 8 == 0 else torch.float32


# ---- argument checks the device input entry points share (collate, augment, resize, resized crop, RandAugment) ----
_RECORD_NAMES = {_lib.AugSample: "calm_aug_sample", _lib.EraseBox: "calm_erase_box", _lib.ResizeSample: "calm_resize_sample",
                 _lib.RCropSample: "calm_rcrop_sample", _lib.RaSample: "calm_ra_sample"}


def _u8_image_batch(who, img_u8, planar=False):
    """img_u8 is a contiguous uint8 CUDA image batch (planar=True: of shape [B,3,Hs,Ws]); returns its shape."""
    ok = img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous()
    if not ok or (planar and (img_u8.dim() != 4 or img_u8.shape[1] != 3)):
        raise TypeError(f"{who} expects a contiguous uint8 CUDA image batch" + (" [B,3,Hs,Ws]" if planar else ""))
    return img_u8.shape


def _records(who, t, B, struct, what="samples"):
    """t is the device array of B `struct` records as a contiguous uint8 CUDA tensor [B, sizeof(struct)]; its pointer."""
    size = C.sizeof(struct)
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (B, size):
        raise TypeError(f"{who}: {what} must be a contiguous uint8 CUDA tensor [B,{size}] ({_RECORD_NAMES[struct]} records)")
    return t.data_ptr()


def _out_hw(out, tokens):
    """(H, W) of an output [B,3,H,W] or, tokens=True, [B,H,3W]."""
    return (out.shape[1], out.shape[2] // 3) if tokens else (out.shape[2], out.shape[3])


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  The raw accessor (what torch's own generated code
    uses) costs 0.3 us; `torch.cuda.current_stream().cuda_stream` builds a Stream object per call — 9 us x 1 500 launches
    per step = 3.5 ms of the 58 ms a Base-224 step takes the host to issue (scripts/host_profile.py)."""
    if _raw_stream is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def chunk_table(lengths, chunk):
    """The host half of the chunk walk of csrc/chunk_table.h: entries of `lengths` units each are cut into chunks of
    `chunk` units -> (chunk0 per entry, the entry of every chunk).  An entry of length 0 has no chunk.  Host only."""
    chunk0, chunk_entry = [], []
    for i, n in enumerate(lengths):
        chunk0.append(len(chunk_entry))
        chunk_entry += [i] * ((n + chunk - 1) // chunk)
    return chunk0, chunk_entry


def _disjoint(spans):
    """No two of the [begin, end) address ranges share a byte (an exchange of, or a scatter into, ranges that do is a race)."""
    spans = sorted(spans)
    return not any(b[0] < a[1] for a, b in zip(spans, spans[1:]))


class ChunkPlan:
    """What every chunk-table launch is given: `n` records in `table_dev` (device bytes) and the record of each of the
    `n_chunks` chunks in `chunk_dev` (int32)."""

    def _tables(self, rec, lengths, chunk, dev):
        """rec: numpy array of the records (its chunk0 field is filled in here), `lengths[i]` units in record i."""
        chunk0, chunk_entry = chunk_table(lengths, chunk)
        rec["chunk0"] = chunk0
        self.n = len(rec)
        self.n_chunks = len(chunk_entry)
        self.table_dev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
        self.chunk_dev = torch.tensor(chunk_entry, dtype=torch.int32, device=dev)


class GroupTable:
    """The (lr, weight_decay) of every parameter group in device memory (`dev`: float32 [n_groups, 2], the
    calm_optim_group records calm_optim_step_groups reads) and the host values last uploaded (`host`).  Plans that step
    the same parameters share one table (FusedClipAdamWindow's two plans).

    `set()` uploads only when a value differs from `host`, and never while the stream is capturing: a captured step
    reads whatever the table holds when it is replayed.  The values travel through a ring of pinned buffers, each
    guarded by an event behind its copy, for the reason OptimPlan's docstring gives."""
    RING = 4

    def __init__(self, n_groups, dev):
        self.n = int(n_groups)
        self.dev = torch.zeros(self.n, 2, dtype=torch.float32, device=dev)
        self.host = np.zeros((self.n, 2), dtype=np.float32)
        self.stage = [torch.empty(self.n, 2, dtype=torch.float32).pin_memory() for _ in range(self.RING)]
        self.events = [None] * self.RING
        self.slot = 0

    def set(self, group_hp):
        """group_hp: one (lr, weight_decay) per group.  True when the device table was rewritten."""
        vals = np.asarray(group_hp, dtype=np.float32).reshape(-1, 2)
        if vals.shape[0] != self.n:
            raise ValueError(f"the plan has {self.n} parameter groups, {vals.shape[0]} (lr, weight_decay) pairs given")
        if not np.all(vals[:, 0] >= 0):                     # (also refuses NaN)
            raise ValueError("a parameter group's learning rate is negative")
        if np.array_equal(vals, self.host) or torch.cuda.is_current_stream_capturing():
            return False
        k = self.slot
        if self.events[k] is not None:
            self.events[k].synchronize()
        self.stage[k].numpy()[:] = vals
        self.dev.copy_(self.stage[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        self.slot = (k + 1) % self.RING
        self.host = vals.copy()
        return True


class OptimPlan(ChunkPlan):
    """Device table of calm_optim_tensor records for calm_optim_step; only the gradient pointers change per step.
    A record's optional "group" (default 0) is the tensor's parameter group for calm_optim_step_groups, below `n_groups`;
    `groups` is the plan's GroupTable.

    The pointers travel through a RING of pinned staging buffers, each guarded by an event recorded behind its
    host-to-device copy: an asynchronous copy from pinned memory reads the host bytes when the DMA runs, not when it is
    enqueued, and the host runs steps ahead of the GPU — a single buffer would be overwritten with the next step's
    pointers before the copy of this step's has executed.  A step whose gradients sit at the addresses of the previous
    upload (gradients kept in the all-reduce buckets, `BucketedGradReducer`) uploads nothing."""
    RING = 4

    def __init__(self, be, records, n_groups=1):
        rec = np.zeros(len(records), dtype=np.dtype(_lib.OptimTensor))
        for i, r in enumerate(records):
            p = r["param"]
            if not p.is_contiguous():
                raise TypeError("optimizer-side step expects contiguous parameters")
            e = rec[i]
            g = r.get("group", 0)
            if int(g) != g or not 0 <= g < n_groups:
                raise ValueError(f"record {i}: parameter group {g!r} outside 0 .. {n_groups - 1}")
            e["group"] = int(g)
            e["param"], e["exp_avg"], e["exp_avg_sq"] = _ptr(p), _ptr(r["exp_avg"]), _ptr(r["exp_avg_sq"])
            if r["exp_avg"].shape != p.shape or r["exp_avg_sq"].shape != p.shape:
                raise ValueError("optimizer state shape mismatch")
            e["numel"] = p.numel()
            if r["sn"] is not None:
                u, v, sigma, rows, cols = r["sn"]
                if rows * cols != p.numel() or p.numel() >= 2 ** 31:      # the kernels index (row, col) in 32 bits
                    raise ValueError("spectral-norm layer too large for the optimizer-side step")
                e["sn_u"], e["sn_v"], e["sn_sigma"], e["rows"], e["cols"] = _ptr(u), _ptr(v), _ptr(sigma), rows, cols
        dev = records[0]["param"].device
        # (table_dev as uploaded here has no gradient pointers: upload() rewrites it in front of every step)
        self._tables(rec, [r["param"].numel() for r in records], int(be.lib.calm_optim_chunk_elems()), dev)
        self.rec = rec
        self.hosts = [torch.empty(rec.nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.RING)]
        self.graph_host = torch.empty(rec.nbytes, dtype=torch.uint8).pin_memory()   # the table a captured step copies from
        self.events = [None] * self.RING
        self.slot = 0
        self.uploaded = None                    # gradient pointers of the table now (being) copied to table_dev
        self.scratch = torch.empty(6 * self.n + 4 + 3 * self.n_chunks, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)      # advanced by the device, not on skipped steps
        self.param_ptrs = rec["param"].copy()
        self.n_groups, self._groups = int(n_groups), None
        self._lamb = None                       # (scratch, trust table) of calm_optim_step_lamb, made at its first use

    @property
    def groups(self):
        """The plan's GroupTable, made at its first use (a plan stepped through calm_optim_step alone never has one)."""
        if self._groups is None:
            self._groups = GroupTable(self.n_groups, self.table_dev.device)
        return self._groups

    @groups.setter
    def groups(self, table):
        if table.n != self.n_groups:
            raise ValueError(f"the plan has {self.n_groups} parameter groups, the table {table.n}")
        self._groups = table

    def lamb_buffers(self, be):
        """(scratch, trust table) of calm_optim_step_lamb, made once — outside a capture they would be ordinary
        allocations, inside one they live in the graph's pool, and either way every later call finds the same addresses.
        The trust table starts at (0, 0, 1): what a tensor shows until an applied step writes it."""
        if self._lamb is None:
            dev = self.table_dev.device
            trust = torch.zeros(self.n, 3, dtype=torch.float32, device=dev)
            trust[:, 2] = 1.0
            self._lamb = (torch.empty(be.lamb_scratch_floats(self), dtype=torch.float32, device=dev), trust)
        return self._lamb

    @property
    def lamb_trust(self):
        return None if self._lamb is None else self._lamb[1]

    def upload(self, grad_ptrs):
        """Stage this step's gradient pointers (numpy uint64 array) and enqueue their copy on the current stream."""
        if self.uploaded is not None and np.array_equal(self.uploaded, grad_ptrs):
            return
        if torch.cuda.is_current_stream_capturing():
            # hipGraph capture (GraphedTrainStep): the gradients live in the graph's private pool, so these addresses are
            # the ones every replay sees; the copy becomes a memcpy node out of a pinned buffer of its own that is never
            # rewritten (no event bookkeeping: a captured event cannot be synchronised on)
            self.rec["grad"] = grad_ptrs
            self.graph_host.numpy()[:] = self.rec.view(np.uint8).reshape(-1)       # (pinned at construction: no allocation here)
            self.table_dev.copy_(self.graph_host, non_blocking=True)
            self.uploaded = grad_ptrs.copy()
            return
        k = self.slot
        if self.events[k] is not None:
            self.events[k].synchronize()        # the copy out of this staging buffer (RING steps ago) has executed
        self.rec["grad"] = grad_ptrs
        self.hosts[k].numpy()[:] = self.rec.view(np.uint8).reshape(-1)
        self.table_dev.copy_(self.hosts[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        self.slot = (k + 1) % self.RING
        self.uploaded = grad_ptrs.copy()


class EmaPlan(ChunkPlan):
    """Device tables of calm_ema_entry records for calm_ema_update / calm_ema_swap, fixed at construction: the entry
    table, the chunk table, the update counter `count_dev` (int32[1], advanced by the device, not on skipped updates) and
    `weight_out` (float32[2]: the weight 1 - d of the last update, and whether it was skipped).  `src_ptrs` / `ema_ptrs`
    record the addresses the table holds (ModelEMA checks them against the parameters before every update).  Tensors with
    no elements have no entry."""

    def __init__(self, be, pairs):
        for src, ema in pairs:
            if not (src.is_contiguous() and ema.is_contiguous()):
                raise TypeError("weight EMA expects contiguous parameters and averages")
            if src.shape != ema.shape:
                raise ValueError("weight EMA shape mismatch")
            _ptr(src), _ptr(ema)                                   # fp32 tensors on the device, or it raises
        pairs = [(src, ema) for src, ema in pairs if src.numel() > 0]
        if not pairs:
            raise ValueError("weight EMA needs at least one tensor with elements")
        ent = np.zeros(len(pairs), dtype=np.dtype(_lib.EmaEntry))
        for i, (src, ema) in enumerate(pairs):
            e = ent[i]
            e["src"], e["ema"], e["numel"] = src.data_ptr(), ema.data_ptr(), src.numel()
        if not _disjoint((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for pr in pairs for t in pr):
            raise ValueError("weight EMA expects parameters and averages that do not overlap in memory")
        dev = pairs[0][0].device
        self._tables(ent, [src.numel() for src, _ in pairs], int(be.lib.calm_ema_chunk_elems()), dev)
        self.count_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.weight_out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.src_ptrs = ent["src"].copy()
        self.ema_ptrs = ent["ema"].copy()


SNAPSHOT_ALIGN = 16


def snapshot_layout(specs):
    """The packed layout of a training snapshot, a pure host function (GPU and CPU models alike, and the reader of a
    file): specs = [(name, dtype, shape)] in the order they are packed -> (offsets, sizes, packed_bytes).  Every offset is
    the running end rounded up to SNAPSHOT_ALIGN = 16 bytes, the order is the given one, a tensor without elements takes
    no room (size 0 at the running offset).  Sizes are whole 4-byte words — calm_snapshot_pack moves words — and anything
    else is refused by name."""
    offsets, sizes, end = [], [], 0
    for name, dtype, shape in specs:
        numel = 1
        for d in shape:
            if int(d) < 0:
                raise ValueError(f"snapshot layout: {name} has a negative extent {tuple(shape)}")
            numel *= int(d)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        if nbytes % 4:
            raise ValueError(f"snapshot layout: {name} ({dtype}, {tuple(shape)}) is {nbytes} bytes, not whole 4-byte words")
        off = -(-end // SNAPSHOT_ALIGN) * SNAPSHOT_ALIGN
        offsets.append(off)
        sizes.append(nbytes)
        if nbytes:
            end = off + nbytes
    return offsets, sizes, -(-end // SNAPSHOT_ALIGN) * SNAPSHOT_ALIGN


def snapshot_chunks(sizes, chunk_bytes):
    """The chunk table of calm_snapshot_pack / _unpack over entries of `sizes` bytes (all > 0): (chunk0 per entry, the
    entry of every chunk).  Host only."""
    if any(nb <= 0 for nb in sizes):
        raise ValueError("snapshot chunk table: entries have at least one word")
    return chunk_table(sizes, chunk_bytes)


class SnapshotPlan(ChunkPlan):
    """Device tables of calm_snapshot_entry records for calm_snapshot_pack / _unpack over a fixed list of live tensors, and
    the packed device buffer they gather into (zeroed once: the padding between entries is never written again, so equal
    states give equal buffers).  `offsets` / `sizes` are per given tensor (snapshot_layout over them; a tensor without
    elements has size 0 and no entry), `ptrs` the addresses the table holds.  What the host can check is checked here:
    device, contiguity, 4-byte alignment, whole words, tensors that overlap one another."""

    def __init__(self, be, tensors, names=None):
        tensors = list(tensors)
        names = list(names) if names is not None else [f"tensor {i}" for i in range(len(tensors))]
        if len(names) != len(tensors):
            raise ValueError("snapshot plan: one name per tensor")
        for n, t in zip(names, tensors):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise TypeError(f"snapshot plan: {n} is not a CUDA tensor")
            if not t.is_contiguous():
                raise TypeError(f"snapshot plan: {n} is not contiguous")
            if t.data_ptr() % 4 and t.numel():
                raise ValueError(f"snapshot plan: {n} is not 4-byte aligned")
        self.offsets, self.sizes, self.packed_bytes = snapshot_layout([(n, t.dtype, tuple(t.shape))
                                                                       for n, t in zip(names, tensors)])
        live = [(t, off, nb) for t, off, nb in zip(tensors, self.offsets, self.sizes) if nb > 0]
        if not live:
            raise ValueError("snapshot plan needs at least one tensor with elements")
        devices = {t.device for t, _, _ in live}
        if len(devices) != 1:
            raise ValueError(f"snapshot plan: tensors on one device expected, got {sorted(map(str, devices))}")
        for (_, off, nb) in live:                                  # (what snapshot_layout guarantees, kept as a check)
            if off % SNAPSHOT_ALIGN or nb % 4 or off + nb > self.packed_bytes:
                raise ValueError("snapshot plan: an entry leaves the packed buffer")
        if not _disjoint((t.data_ptr(), t.data_ptr() + nb) for t, _, nb in live):
            raise ValueError("snapshot plan expects tensors that do not overlap in memory")
        self.chunk_bytes = int(be.lib.calm_snapshot_chunk_bytes())
        ent = np.zeros(len(live), dtype=np.dtype(_lib.SnapshotEntry))
        for i, (t, off, nb) in enumerate(live):
            e = ent[i]
            e["tensor"], e["offset"], e["nbytes"] = t.data_ptr(), off, nb
        dev = live[0][0].device
        self._tables(ent, [nb for _, _, nb in live], self.chunk_bytes, dev)          # (live entries: every nb > 0)
        self.entries = ent
        self.packed = torch.zeros(self.packed_bytes, dtype=torch.uint8, device=dev)
        if self.packed.data_ptr() % SNAPSHOT_ALIGN:
            raise RuntimeError("snapshot plan: the packed buffer is not 16-byte aligned")
        self.ptrs = ent["tensor"].copy()
        self.tensors = [t for t, _, _ in live]                        # keeps the addresses in the table alive


class CastPlan(ChunkPlan):
    """Device tables of calm_cast_entry records for calm_cast_bf16 over fixed (fp32 source, bf16 destination) pairs."""

    def __init__(self, be, pairs):
        ent = np.zeros(len(pairs), dtype=np.dtype(_lib.CastEntry))
        for i, (src, dst) in enumerate(pairs):
            if dst.dtype != torch.bfloat16 or dst.numel() != src.numel() or not (src.is_contiguous() and dst.is_contiguous()):
                raise TypeError("cast_plan: contiguous fp32 source / bf16 destination of equal size expected")
            ent[i]["src"], ent[i]["dst"], ent[i]["numel"] = _ptr(src), _ptr(dst, bf16_ok=True), src.numel()
        self._tables(ent, [src.numel() for src, _ in pairs], int(be.lib.calm_cast_chunk_elems()), pairs[0][0].device)


class SnPlan:
    """Device-resident plan for the batched spectral-norm power iteration."""

    def __init__(self, info, blob_dev, scratch, key):
        self.info = info
        self.blob_dev = blob_dev
        self.scratch = scratch
        self.key = key


class HipBackend:
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self._scratch_bufs = {}
        self._scratch_retired = []      # buffers a larger one replaced: a captured graph may hold their addresses
        self._scratch_need = {}
        self.plan_epoch = 0
        self.upcast_launches = 0        # calm_gemm launches re-run on fp32 copies (CALM_E_LAYOUT with bf16 tensors)
        self._lane_ws = []              # workspaces of launches on the side lane, kept until gemm_lane_join
        if _wgrad_lane:
            self.gemm_set_option(self.GEMM_OPT_LANE, 1)

    def _partials(self, op, rows, cols, device):
        """Device scratch for the fixed-order cross-workgroup reduction of one call (calm_reduce_scratch_floats).  One
        buffer per (device, stream), reused by every call on that stream: the launches of one stream run in order, so a
        call's rows of partials have been consumed by its own reduction pass before the next call writes any.  A buffer
        that a larger one replaces stays referenced: its address may be baked into a captured graph, whose replays would
        otherwise write partial sums into memory the allocator has handed to another tensor."""
        need = self._scratch_need.get((op, rows, cols))
        if need is None:                                         # (a step has ~170 such calls over ~20 distinct shapes)
            need = self._scratch_need[(op, rows, cols)] = int(self.lib.calm_reduce_scratch_floats(op, rows, cols))
        key = (device.index, _stream())
        buf = self._scratch_bufs.get(key)
        if buf is None or buf.numel() < need:
            if buf is not None:
                self._scratch_retired.append(buf)
            buf = torch.empty(max(need, 1 << 20), dtype=torch.float32, device=device)
            self._scratch_bufs[key] = buf
        return buf.data_ptr()

    def _own_partials(self, op, rows, cols, device):
        """Scratch of one DEFERRED reduction (the *_part methods): a buffer of the call's own, because its rows of partials
        stay unread until reduce_partials_batch runs at the end of the backward — the shared buffer of _partials would be
        overwritten by the next call."""
        need = self._scratch_need.get((op, rows, cols))
        if need is None:
            need = self._scratch_need[(op, rows, cols)] = int(self.lib.calm_reduce_scratch_floats(op, rows, cols))
        return torch.empty(need, dtype=torch.float32, device=device)

    def reduce_partials_batch(self, items):
        """items: [(partials, ReduceShape, [output tensors, one per segment])] as the *_part methods return them — every
        reduction of the list in ceil(len / calm_reduce_batch_max()) launches, each bit-identical with the single form."""
        ent = (_lib.ReduceEntry * len(items))()
        for e, (part, shape, outs) in zip(ent, items):
            if len(outs) != shape.nseg:
                raise ValueError("reduce_partials_batch: one output per segment expected")
            e.partials, e.G, e.n, e.stride, e.nseg = _ptr(part), shape.G, shape.n, shape.stride, shape.nseg
            for k, o in enumerate(outs):
                if o.numel() != shape.begin[k + 1] - shape.begin[k] or not o.is_contiguous():
                    raise ValueError("reduce_partials_batch: output size does not match its segment")
                e.out[k] = _ptr(o)
            for k in range(shape.nseg + 1):
                e.begin[k] = shape.begin[k]
        _lib.check(self.lib.calm_reduce_partials_batch(ent, len(items), _stream()), "calm_reduce_partials_batch")

    # ---- GEMM -------------------------------------------------------------------------
    GEMM_OPT_PIPE, GEMM_OPT_PIPE32, GEMM_OPT_DETERMINISTIC, GEMM_OPT_LANE = 0, 1, 2, 3

    def gemm_set_option(self, option, value):
        """calm_gemm_set_option (ABI v6; v7: GEMM_OPT_DETERMINISTIC = k-split launches through the workspace and a
        fixed-order reduction instead of fp32 atomics; GEMM_OPT_LANE = gemm(lane=True) launches go to the side lane,
        see set_wgrad_lane); returns the previous value."""
        prev = self.lib.calm_gemm_set_option(int(option), int(value))
        if prev < 0:
            raise ValueError(f"calm_gemm_set_option({option}, {value}) -> {prev}")
        self.plan_epoch += 1            # answers of gemm_describe cached before this call are stale
        return prev

    def selfcheck_bf16_gemm(self, rows=57344, on_mismatch="raise"):
        """Canary for the default bf16 GEMM family: round 3 saw ONE box of the pool on which the
        pipelined persistent family (gemm_bf16p_kernel: 128 KiB of LDS, 256 VGPRs, LDS-DMA) returned a deterministic
        wrong GELU' input gradient at 57344 x 1344 x 1344 while the 256x128 family was right; the audit found no code
        defect.  Until the cause is pinned, a training job can ask the box itself: this runs the three
        operand-layout instantiations of the family at the bench's sizes — forward with fused bias + GELU (k-contiguous
        pair), the GELU' input gradient (k-contiguous x row-contiguous) and a per-image product (row-contiguous pair) —
        on both families and compares them (healthy boxes: identical up to a handful of results that sit on a bf16
        rounding boundary — one ulp; a fault: more than one ulp AND more than 2^-9 of the largest element).  on_mismatch: "raise" (RuntimeError with the pattern of the differing elements), or "fallback"
        (warn and switch this process to the 256x128 family — still the HIP path, 10-20 % slower GEMMs).
        Returns {"ok", "cases": [{name, n_diff, n_bad, max_diff, plan, first}]}.  ~0.8 GB of scratch tensors, a few ms."""
        import warnings
        dev = torch.device("cuda", torch.cuda.current_device())
        gen = torch.Generator(device=dev).manual_seed(20061)           # (on the device: 250 M normals take seconds on the host)
        mk = lambda *shape, scale=1.0: (torch.randn(*shape, generator=gen, device=dev) * scale).bfloat16()
        M, K, N = int(rows), 672, 1344
        x, w1, dy, w2 = mk(M, K), mk(N, K, scale=K ** -0.5), mk(M, N), mk(N, N, scale=N ** -0.5)
        bias = torch.randn(N, generator=gen, device=dev) * 0.1
        sigma = torch.tensor([1.3], device=dev)
        S, nb = 224, 64
        pa, pb = mk(nb, S, S), mk(nb, S, 3 * S, scale=S ** -0.5)
        hp = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        e16 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.bfloat16)
        cases = [
            ("forward bias+GELU (kk)", lambda out: ((x, w1, out, M, N, K, (K, 1, 0, 0), (K, 1, 0, 0), (N, 0, 0)),
                                                    dict(inv_scale=sigma, bias=bias, act=ACT_GELU, C_pre=hp, split_k=1)), (M, N)),
            ("GELU' input gradient (km)", lambda out: ((dy, w2, out, M, N, N, (N, 1, 0, 0), (1, N, 0, 0), (N, 0, 0)),
                                                       dict(inv_scale=sigma, act=ACT_GELU_BWD, aux=hp, split_k=1)), (M, N)),
            ("per-image product (mm)", lambda out: ((pa, pb, out, S, 3 * S, S, (1, S, S * S, 0), (1, 3 * S, S * 3 * S, 0),
                                                     (3 * S, S * 3 * S, 0)), dict(batch=(nb, 1), split_k=1)), (nb, S, 3 * S)),
        ]
        prev_prec = get_matmul_precision()
        set_matmul_precision("bf16")
        report, ok = [], True
        try:
            for name, build, shape in cases:
                got, alt = e16(*shape), e16(*shape)
                args, kw = build(got)
                plan = self.gemm_describe(*args, **kw)
                self.gemm(*args, **kw)
                prev = self.gemm_set_option(self.GEMM_OPT_PIPE, 0)
                try:
                    args2, kw2 = build(alt)
                    self.gemm(*args2, **kw2)
                finally:
                    self.gemm_set_option(self.GEMM_OPT_PIPE, prev)
                # the families accumulate k in different groupings, so a result that sits on a bf16 rounding boundary may
                # land on either neighbour (measured: ~700 of 77 M elements of the GELU case, one ulp each); a fault is
                # an element MORE than one bf16 ulp away AND off by more than 2^-9 of the largest element (the round-3
                # box: 1.2e-2 of it; one stale 16-byte operand chunk: ~2e-2)
                key = lambda t: torch.where(t.view(torch.int16) < 0, -(t.view(torch.int16).int() & 0x7FFF), t.view(torch.int16).int())
                ulps = (key(got) - key(alt)).abs()
                scale = float(alt.float().abs().max())
                err = (got.float() - alt.float()).abs()
                bad = (ulps > 1) & (err > 2.0 ** -9 * scale)
                n_diff, n_bad = int((ulps > 0).sum()), int(bad.sum())
                rec = {"name": name, "n_diff": n_diff, "n_bad": n_bad, "max_diff": float(err.max()) / max(scale, 1e-30),
                       "plan": plan, "first": []}
                if n_bad:
                    idx = bad.reshape(-1, shape[-1]).nonzero()[:8].tolist()
                    g2, a2 = got.reshape(-1, shape[-1]), alt.reshape(-1, shape[-1])
                    rec["first"] = [(r, c, float(g2[r, c]), float(a2[r, c])) for r, c in idx]
                    rec["rows"] = [int(bad.reshape(-1, shape[-1]).nonzero()[:, 0].min()), int(bad.reshape(-1, shape[-1]).nonzero()[:, 0].max())]
                    if plan["family"] == 3:
                        ok = False
                report.append(rec)
        finally:
            set_matmul_precision(prev_prec)
        res = {"ok": ok, "cases": report}
        if not ok:
            msg = ("the pipelined bf16 GEMM family disagrees with the 256x128 family on this box (see DESIGN.md section 2): " +
                   "; ".join(f"{r['name']}: {r['n_bad']} elements beyond one ulp (rows {r.get('rows')}), max {r['max_diff']:.2e} "
                             f"of the largest element, first (row, col, pipelined, 256x128) {r['first'][:3]}"
                             for r in report if r["n_bad"]))
            if on_mismatch == "fallback":
                self.gemm_set_option(self.GEMM_OPT_PIPE, 0)
                warnings.warn(msg + " -- continuing on the 256x128 family (calm_gemm_set_option(PIPE, 0))")
            else:
                raise RuntimeError(msg)
        return res

    def gemm_describe(self, *args, **kw):
        """calm_gemm_describe (ABI v7) for the launch `gemm(*args, **kw)` would make: a dict of the plan's fields
        (family, tile, tiles, k-slices, items, grid ...).  Nothing is enqueued."""
        g, _keep = self._gemm_args(*args, **kw)
        plan = _lib.GemmPlan()
        _lib.check(self.lib.calm_gemm_describe(C.byref(g), C.byref(plan)), "calm_gemm_describe")
        return {name: getattr(plan, name) for name, _ in _lib.GemmPlan._fields_}

    def gemm(self, A, B, Cout, M, N, K, a, b, c, batch=(1, 1), alpha=1.0, inv_scale=None, bias=None,
             col_scale=None, residual=None, r=(0, 0, 0), C_pre=None, aux=None, act=ACT_NONE,
             accumulate=False, reduce_batch=False, split_k=0, a_dq=None, b_dq=None, lane=False):
        """a_dq / b_dq: device dequantisation factors of fp8 operands (quantize_fp8's state[1:2]).
        lane=True: calm_gemm_lane_fork on the current stream, then the launch through calm_gemm_lane — on the library's
        side lane while GEMM_OPT_LANE is on and the stream is not capturing, else on the current stream.  The caller
        keeps A, B and Cout referenced until gemm_lane_join(); the backend keeps the launch's workspace until then."""
        g, (A, B, Cout) = self._gemm_args(A, B, Cout, M, N, K, a, b, c, batch, alpha, inv_scale, bias, col_scale, residual,
                                          r, C_pre, aux, act, accumulate, reduce_batch, split_k, a_dq, b_dq)
        ws = None
        if split_k != 1 and GEMM_WORKSPACE:
            # split launches with many k-slices per output combine them through a workspace instead of atomics; the
            # buffer comes from torch's caching allocator and is stream-ordered like every other tensor of the step
            need = self.lib.calm_gemm_workspace_bytes(C.byref(g))
            if need > 0:
                ws = torch.empty(need // 4, dtype=torch.float32, device=Cout.device)
                g.workspace, g.workspace_bytes = ws.data_ptr(), need
        if lane:
            # (the fork follows the workspace allocation: whatever the allocator did to hand it out is ordered before it)
            _lib.check(self.lib.calm_gemm_lane_fork(_stream()), "calm_gemm_lane_fork")
            rc = self.lib.calm_gemm_lane(C.byref(g), _stream())
        else:
            rc = self.lib.calm_gemm(C.byref(g), _stream())
        fp8_operand = g.a_type >= _lib.ST_FP8_E4M3 or g.b_type >= _lib.ST_FP8_E4M3     # fp8 tensors have no fp32 re-run: report
        if rc == _lib.E_LAYOUT and not fp8_operand and (g.a_type or g.b_type or g.c_type or g.aux_type or g.r_type):
            # a bf16 tensor in a launch whose sizes / strides rule out 16-byte staging (the 10-class head of the fixture
            # models, a 36-token stage): rare and tiny — run it on fp32 copies through the generic kernels
            return self._gemm_upcast(A, B, Cout, M, N, K, a, b, c, batch, alpha, inv_scale, bias, col_scale, residual,
                                     r, C_pre, aux, act, accumulate, reduce_batch, split_k, g)
        _lib.check(rc, "calm_gemm")
        if lane and ws is not None:
            self._lane_ws.append(ws)    # (the caching allocator knows the block as the current stream's, not the lane's)

    def gemm_lane_join(self):
        """calm_gemm_lane_join on the current stream: what it is given next follows every lane launch so far."""
        _lib.check(self.lib.calm_gemm_lane_join(_stream()), "calm_gemm_lane_join")
        self._lane_ws.clear()

    def gemm_lane_stats(self):
        """calm_gemm_lane_stats: {"forks", "launches", "joins", "events"} since the library was loaded."""
        out = (C.c_int64 * 4)()
        _lib.check(self.lib.calm_gemm_lane_stats(C.byref(out)), "calm_gemm_lane_stats")
        return dict(zip(("forks", "launches", "joins", "events"), out))

    def _gemm_args(self, A, B, Cout, M, N, K, a, b, c, batch=(1, 1), alpha=1.0, inv_scale=None, bias=None,
                   col_scale=None, residual=None, r=(0, 0, 0), C_pre=None, aux=None, act=ACT_NONE,
                   accumulate=False, reduce_batch=False, split_k=0, a_dq=None, b_dq=None):
        """(calm_gemm_args, (A, B, C) base tensors) for a launch."""
        g = _lib.GemmArgs()
        # grouped form: A / B / Cout / inv_scale given as lists of separately allocated tensors, one per b0 entry
        groups = [len(t) for t in (A, B, Cout, inv_scale) if isinstance(t, (list, tuple))]
        if groups:
            n = groups[0]
            if any(k != n for k in groups) or batch != (n, 1):
                raise ValueError("grouped gemm: every list needs batch[0] entries and batch[1] must be 1")
            g.n_group = n
            for name, t in (("A_group", A), ("B_group", B), ("C_group", Cout), ("inv_scale_group", inv_scale)):
                if isinstance(t, (list, tuple)):
                    tab = getattr(g, name)
                    if name != "inv_scale_group" and len({ti.dtype for ti in t}) != 1:
                        raise TypeError("grouped gemm: the tensors of one operand must share a storage type")
                    for i, ti in enumerate(t):
                        tab[i] = _ptr(ti, True, bf16_ok=name != "inv_scale_group")
            A, B, Cout = (t[0] if isinstance(t, (list, tuple)) else t for t in (A, B, Cout))
            inv_scale = None
        g.A, g.B, g.C = _ptr(A, bf16_ok=True, fp8_ok=True), _ptr(B, bf16_ok=True, fp8_ok=True), _ptr(Cout, bf16_ok=True)
        g.a_dq, g.b_dq = _ptr(a_dq, True), _ptr(b_dq, True)
        g.a_type, g.b_type, g.c_type, g.aux_type, g.r_type = _st(A), _st(B), _st(Cout), _st(aux), _st(residual)
        if C_pre is not None and C_pre.dtype != Cout.dtype:
            raise TypeError("gemm: C_pre must have C's storage type")
        g.M, g.N, g.K = M, N, K
        g.batch0, g.batch1 = batch
        g.a_rs, g.a_cs, g.a_b0, g.a_b1 = a
        g.b_rs, g.b_cs, g.b_b0, g.b_b1 = b
        g.c_rs, g.c_b0, g.c_b1 = c
        g.alpha = alpha
        g.inv_scale = _ptr(inv_scale, True)
        g.bias = _ptr(bias, True)
        g.col_scale = _ptr(col_scale, True)
        g.residual = _ptr(residual, True, bf16_ok=True)
        g.r_rs, g.r_b0, g.r_b1 = r
        g.C_pre = _ptr(C_pre, True, bf16_ok=True)
        g.aux = _ptr(aux, True, bf16_ok=True)
        g.act = act
        g.accumulate = int(accumulate)
        g.reduce_batch = int(reduce_batch)
        g.split_k = split_k
        g.dtype = PRECISIONS[effective_precision()]
        return g, (A, B, Cout)

    def _gemm_upcast(self, A, B, Cout, M, N, K, a, b, c, batch, alpha, inv_scale, bias, col_scale, residual, r, C_pre,
                     aux, act, accumulate, reduce_batch, split_k, g):
        if g.n_group:
            raise RuntimeError("calm_gemm: grouped launch with bf16 tensors that cannot be staged (CALM_E_LAYOUT)")

        self.upcast_launches += 1

        def up(t):
            if t is None or t.dtype != torch.bfloat16:
                return t
            if not t.is_contiguous():
                raise RuntimeError("calm_gemm: non-contiguous bf16 tensor in a launch that cannot be vectorised")
            t32 = torch.empty(t.shape, dtype=torch.float32, device=t.device)
            _lib.check(self.lib.calm_cast_f32_one(t.data_ptr(), t32.data_ptr(), t.numel(), _stream()), "calm_cast_f32_one")
            return t32
        C32, P32 = up(Cout), up(C_pre)
        self.gemm(up(A), up(B), C32, M, N, K, a, b, c, batch=batch, alpha=alpha, inv_scale=inv_scale, bias=bias,
                  col_scale=col_scale, residual=up(residual), r=r, C_pre=P32, aux=up(aux), act=act, accumulate=accumulate,
                  reduce_batch=reduce_batch, split_k=split_k)
        if C32 is not Cout:
            self.cast_bf16(C32, Cout)
        if P32 is not C_pre:
            self.cast_bf16(P32, C_pre)

    # ---- device-side collate -------------------------------------------------------------
    def collate_mix(self, img_u8, flip, out, mode, lam, box, mean, std):
        """img_u8 [B,3,H,W] uint8, flip [B] uint8 or None, out [B,3,H,W] fp32; mode 0/1/2 = none/MixUp/CutMix."""
        B, _, H, W = _u8_image_batch("collate_mix", img_u8)
        cbox = (C.c_int32 * 4)(*box) if box is not None else None
        cm, cs = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        fp = flip.data_ptr() if flip is not None else None
        _lib.check(self.lib.calm_collate_mix(img_u8.data_ptr(), fp, _ptr(out), B, H, W, mode, float(lam), cbox, cm, cs,
                                             _stream()), "calm_collate_mix")

    def collate_crop_mix(self, img_u8, crop_yx, flip, out, mode, lam, box, mean, std, tokens=False):
        """img_u8 [B,3,Hs,Ws] uint8; crop_yx [B,2] int32 on the device (or None); out [B,3,H,W] or, tokens=True,
        [B,H,3W] fp32 (the row tokens of the first Block)."""
        B, _, Hs, Ws = _u8_image_batch("collate_crop_mix", img_u8)
        H, W = _out_hw(out, tokens)
        if crop_yx is not None and (crop_yx.dtype != torch.int32 or not crop_yx.is_cuda or not crop_yx.is_contiguous()):
            raise TypeError("collate_crop_mix: crop_yx must be a contiguous int32 CUDA tensor [B,2]")
        cbox = (C.c_int32 * 4)(*box) if box is not None else None
        cm, cs = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        _lib.check(self.lib.calm_collate_crop_mix(img_u8.data_ptr(), Hs, Ws, crop_yx.data_ptr() if crop_yx is not None else None,
                                                  flip.data_ptr() if flip is not None else None, _ptr(out), B, H, W,
                                                  int(tokens), mode, float(lam), cbox, cm, cs, _stream()),
                   "calm_collate_crop_mix")

    def augment_collate(self, img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens=False):
        """collate_crop_mix with ColorJitter / solarize / flip / grayscale / 3x3 Gaussian blur per sample in front of
        Normalize (calm_augment_collate).  img_u8 [B,3,Hs,Ws] uint8; samples: the device array of B calm_aug_sample
        records as a contiguous uint8 CUDA tensor [B,48] (trainer.DeviceAugment.pack: crop corners and flips are in it);
        gray_mean [B] fp32 CUDA, written (the contrast means); out [B,3,H,W] or, tokens=True, [B,H,3W] fp32."""
        args = self._augment_args("augment_collate", img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens)
        _lib.check(self.lib.calm_augment_collate(*args, _stream()), "calm_augment_collate")

    @staticmethod
    def _augment_args(who, img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens):
        """The tensor checks and the C arguments, up to std, that calm_augment_collate and calm_augment_collate_erase share."""
        B, _, Hs, Ws = _u8_image_batch(who, img_u8)
        H, W = _out_hw(out, tokens)
        if out.shape[0] != B or out.numel() != B * 3 * H * W or not out.is_contiguous():
            raise TypeError(f"{who}: out must be contiguous [B,3,H,W] or, tokens=True, [B,H,3W]")
        samples_ptr = _records(who, samples, B, _lib.AugSample)
        if (gray_mean.dtype != torch.float32 or not gray_mean.is_cuda or not gray_mean.is_contiguous()
                or gray_mean.numel() != B):
            raise TypeError(f"{who}: gray_mean must be a contiguous fp32 CUDA tensor [B]")
        cbox = (C.c_int32 * 4)(*box) if box is not None else None
        cm, cs = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        return (img_u8.data_ptr(), Hs, Ws, samples_ptr, gray_mean.data_ptr(), _ptr(out), B, H, W, int(tokens), mode,
                float(lam), cbox, cm, cs)

    def augment_collate_erase(self, img_u8, samples, gray_mean, out, mode, lam, box, mean, std, boxes, value, key,
                              tokens=False):
        """augment_collate with RandomErasing between Normalize and the mix (calm_augment_collate_erase).  boxes: the
        device array of B calm_erase_box records as a contiguous uint8 CUDA tensor [B,16] (trainer.DeviceErase.pack;
        output coordinates, h == 0 or w == 0: not erased — the caller has checked them, DeviceErase.check); value: None
        for per-pixel standard normal noise, or three floats in normalised space; key: (seed, offset), the noise key,
        integers below 2^64.  The other arguments as augment_collate."""
        args = self._augment_args("augment_collate_erase", img_u8, samples, gray_mean, out, mode, lam, box, mean, std, tokens)
        boxes_ptr = _records("augment_collate_erase", boxes, img_u8.shape[0], _lib.EraseBox, "boxes")
        seed, offset = (int(k) for k in key)
        if not (0 <= seed < 2 ** 64 and 0 <= offset < 2 ** 64):
            raise ValueError("augment_collate_erase: key is (seed, offset), two integers in [0, 2^64)")
        cv = (C.c_float * 3)(*value) if value is not None else None
        _lib.check(self.lib.calm_augment_collate_erase(*args, boxes_ptr, 0 if value is not None else 1, cv, seed,
                                                       offset, _stream()),
                   "calm_augment_collate_erase")

    def resize_u8(self, packed, samples, out):
        """PIL's antialiased bilinear Image.resize over a ragged batch, bit for bit (calm_resize_u8).  packed: 1-D uint8
        CUDA tensor holding B images as h x w x 3 interleaved bytes; samples: the device array of B calm_resize_sample
        records (offset, h, w) as a contiguous uint8 CUDA tensor [B,16] (trainer.DeviceResize.pack); out [B,3,oh,ow]
        uint8 CUDA, written."""
        if not packed.is_cuda or packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
            raise TypeError("resize_u8 expects a contiguous 1-D uint8 CUDA buffer")
        if not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 4 or out.shape[1] != 3 or not out.is_contiguous():
            raise TypeError("resize_u8: out must be a contiguous uint8 CUDA tensor [B,3,oh,ow]")
        B, _, oh, ow = out.shape
        samples_ptr = _records("resize_u8", samples, B, _lib.ResizeSample)
        _lib.check(self.lib.calm_resize_u8(packed.data_ptr(), packed.numel(), samples_ptr, out.data_ptr(), B, oh, ow,
                                           _stream()), "calm_resize_u8")

    def resized_crop(self, packed, samples, out, mean=None, std=None, tokens=False):
        """PIL's crop(box).resize(size, BILINEAR) over a ragged batch, of which only a window is computed
        (calm_resized_crop).  packed: 1-D uint8 CUDA tensor holding B images as h x w x 3 interleaved bytes; samples: the
        device array of B calm_rcrop_sample records as a contiguous uint8 CUDA tensor [B,48]
        (trainer.DeviceResizedCrop.pack); out, written: uint8 [B,3,H,W] (the resized bytes), fp32 [B,3,H,W] (normalised
        with mean / std, three floats each) or, tokens=True, fp32 [B,H,3W] (the first Block's row tokens)."""
        if not packed.is_cuda or packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
            raise TypeError("resized_crop expects a contiguous 1-D uint8 CUDA buffer")
        if not out.is_cuda or not out.is_contiguous() or out.dtype not in (torch.uint8, torch.float32):
            raise TypeError("resized_crop: out must be a contiguous uint8 or fp32 CUDA tensor")
        if tokens:
            if out.dtype != torch.float32 or out.dim() != 3 or out.shape[2] % 3 != 0:
                raise TypeError("resized_crop: tokens=True writes a contiguous fp32 CUDA tensor [B,H,3W]")
            kind = _lib.RCROP_TOKENS
        else:
            if out.dim() != 4 or out.shape[1] != 3:
                raise TypeError("resized_crop: out must be a contiguous uint8 or fp32 CUDA tensor [B,3,H,W]")
            kind = _lib.RCROP_U8 if out.dtype == torch.uint8 else _lib.RCROP_IMAGE
        B, (H, W) = out.shape[0], _out_hw(out, tokens)
        samples_ptr = _records("resized_crop", samples, B, _lib.RCropSample)
        cm = cs = None
        if kind != _lib.RCROP_U8:
            if mean is None or std is None or len(mean) != 3 or len(std) != 3:
                raise TypeError("resized_crop: an fp32 output needs mean and std, three floats each")
            cm, cs = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        _lib.check(self.lib.calm_resized_crop(packed.data_ptr(), packed.numel(), samples_ptr, out.data_ptr(), B, H, W,
                                              kind, cm, cs, _stream()), "calm_resized_crop")

    def randaugment_scratch_bytes(self, B, H, W):
        """Bytes of scratch randaugment_u8 needs for a [B,3,H,W] output (calm_randaugment_scratch_bytes)."""
        n = self.lib.calm_randaugment_scratch_bytes(B, H, W)
        if n < 0:
            _lib.check(int(n), "calm_randaugment_scratch_bytes")
        return int(n)

    def randaugment_u8(self, img_u8, samples, out, n_slots, stats_mask, fill=None, scratch=None):
        """The uint8 RandAugment stage (calm_randaugment_u8): per sample the crop window and the flip, then up to four
        PIL-exact uint8 operations.  img_u8 [B,3,Hs,Ws] uint8; samples: the device array of B calm_ra_sample records as a
        contiguous uint8 CUDA tensor [B,160] (trainer.DeviceRandAugment.pack: corners and flips are in it); out
        [B,3,H,W] uint8, written; n_slots: the slot passes to run (the batch's largest n_ops); stats_mask: bit k set when
        some sample's slot k is Contrast, AutoContrast or Equalize; fill: three integers 0 .. 255 (None: black);
        scratch: a uint8 CUDA tensor of at least randaugment_scratch_bytes(B, H, W) bytes (None: allocated here)."""
        B, _, Hs, Ws = _u8_image_batch("randaugment_u8", img_u8, planar=True)
        if (not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 4 or out.shape[0] != B or out.shape[1] != 3
                or not out.is_contiguous()):
            raise TypeError("randaugment_u8: out must be a contiguous uint8 CUDA tensor [B,3,H,W]")
        H, W = out.shape[2], out.shape[3]
        samples_ptr = _records("randaugment_u8", samples, B, _lib.RaSample)
        need = self.randaugment_scratch_bytes(B, H, W)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.uint8, device=img_u8.device)
        if not scratch.is_cuda or scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need:
            raise TypeError(f"randaugment_u8: scratch must be a contiguous uint8 CUDA tensor of at least {need} bytes")
        cf = None
        if fill is not None:
            if len(fill) != 3 or not all(int(v) == v and 0 <= v <= 255 for v in fill):
                raise ValueError(f"randaugment_u8: fill is three integers in 0 .. 255, got {fill!r}")
            cf = (C.c_uint8 * 3)(*(int(v) for v in fill))
        _lib.check(self.lib.calm_randaugment_u8(img_u8.data_ptr(), Hs, Ws, samples_ptr, out.data_ptr(), B, H, W,
                                                int(n_slots), int(stats_mask), cf, scratch.data_ptr(), scratch.numel(),
                                                _stream()), "calm_randaugment_u8")

    # ---- optimizer-side step ------------------------------------------------------------
    def optim_plan(self, records, n_groups=1):
        """records: one dict per parameter — param, exp_avg, exp_avg_sq, sn (None or (u, v, sigma, rows, cols)) and,
        optionally, group (the parameter group of optim_step_groups, below n_groups; default 0)."""
        return OptimPlan(self, records, n_groups)

    def optim_step(self, plan, grads, hp, grad_scale, stats_out, lr_dev=None):
        """hp = (lr, beta1, beta2, eps, weight_decay, max_norm, step); stats_out[2] <- grad norm, found_inf.
        The step count used for the bias correction is plan.step_dev (device; not advanced on skipped steps).
        lr_dev: device scalar that overrides hp's lr (a captured step reads its learning rate from it)."""
        plan.upload(np.asarray([_ptr(g) for g in grads], dtype=np.uint64))
        h = _lib.OptimHparams(*hp)
        _lib.check(self.lib.calm_optim_step(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                            _ptr(plan.scratch), C.byref(h), _ptr(grad_scale, True), _ptr(stats_out),
                                            plan.step_dev.data_ptr(), _ptr(lr_dev, True), _stream()), "calm_optim_step")

    def optim_step_groups(self, plan, grads, hp, group_hp, grad_scale, stats_out):
        """calm_optim_step_groups: optim_step with the (lr, weight_decay) of every tensor taken from its parameter
        group.  hp as for optim_step (its lr and weight_decay are ignored); group_hp: one (lr, weight_decay) per group
        of the plan, written to the plan's device table when a value changed since the last upload — never while the
        stream is capturing: a captured step reads the table as it is at replay (GroupTable.set between replays).
        CAUTION: a call inside a capture whose group_hp differs from the values last uploaded therefore steps with the
        uploaded ones, silently; upload the rates in front of the capture (plan.groups.set / sync_lr_to_device), as
        GraphedTrainStep does."""
        plan.upload(np.asarray([_ptr(g) for g in grads], dtype=np.uint64))
        plan.groups.set(group_hp)
        h = _lib.OptimHparams(*hp)
        _lib.check(self.lib.calm_optim_step_groups(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(),
                                                   plan.n_chunks, _ptr(plan.scratch), C.byref(h),
                                                   plan.groups.dev.data_ptr(), plan.groups.n, _ptr(grad_scale, True),
                                                   _ptr(stats_out), plan.step_dev.data_ptr(), _stream()),
                   "calm_optim_step_groups")

    def lamb_scratch_floats(self, plan):
        """calm_optim_lamb_scratch_floats for the table of `plan` (host only)."""
        return int(self.lib.calm_optim_lamb_scratch_floats(plan.n, plan.n_chunks))

    def optim_step_lamb(self, plan, grads, hp, lamb_hp, grad_scale, stats_out, group_hp=None, lr_dev=None, scratch=None,
                        trust_out=None):
        """calm_optim_step_lamb: optim_step (group_hp None) or optim_step_groups (group_hp: one (lr, weight_decay) per
        group of the plan, uploaded as optim_step_groups uploads them — the same CAUTION about captures holds) with the
        update of every tensor scaled by its trust ratio.  lamb_hp = (trust_clip or None / 0 for no limit, always_adapt).
        The scratch and the table (wn, un, trust) per tensor, `plan.lamb_trust` (float32 [n, 3]), are allocated at the
        plan's first LAMB step and kept for its lifetime: a captured step bakes their addresses in.  scratch / trust_out:
        the caller's own buffers instead (lamb_scratch_floats(plan) floats; float32 [n, 3])."""
        plan.upload(np.asarray([_ptr(g) for g in grads], dtype=np.uint64))
        if group_hp is not None:
            plan.groups.set(group_hp)
        if scratch is None or trust_out is None:
            own = plan.lamb_buffers(self)
            scratch, trust_out = own[0] if scratch is None else scratch, own[1] if trust_out is None else trust_out
        if scratch.dtype != torch.float32 or scratch.numel() < self.lamb_scratch_floats(plan):
            raise ValueError("optim_step_lamb: scratch smaller than calm_optim_lamb_scratch_floats answers")
        if trust_out.dtype != torch.float32 or trust_out.numel() != 3 * plan.n or not trust_out.is_contiguous():
            raise ValueError("optim_step_lamb expects three contiguous float32 per tensor of the plan as trust_out")
        clip, always = lamb_hp
        h, lh = _lib.OptimHparams(*hp), _lib.LambHparams(float(clip or 0.0), int(bool(always)))
        grouped = group_hp is not None
        _lib.check(self.lib.calm_optim_step_lamb(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                                 _ptr(scratch), C.byref(h), C.byref(lh),
                                                 plan.groups.dev.data_ptr() if grouped else None,
                                                 plan.groups.n if grouped else 0, _ptr(grad_scale, True), _ptr(stats_out),
                                                 _ptr(trust_out), plan.step_dev.data_ptr(),
                                                 None if grouped else _ptr(lr_dev, True), _stream()), "calm_optim_step_lamb")

    def grad_accum(self, plan, grads, acc_ptrs_dev, first):
        """calm_grad_accum over the table of `plan` (the optimizer's deferred plan, this micro-batch's gradient pointers
        uploaded as for optim_step): acc = (first ? 0 : acc) + corrected gradient.  acc_ptrs_dev: int64 device tensor of
        plan.n accumulator addresses.  Uses the first plan.n_chunks floats of plan.scratch."""
        if acc_ptrs_dev.numel() != plan.n or acc_ptrs_dev.dtype != torch.int64 or not acc_ptrs_dev.is_cuda:
            raise ValueError("grad_accum expects one int64 accumulator address per tensor of the plan, on the device")
        plan.upload(np.asarray([_ptr(g) for g in grads], dtype=np.uint64))
        _lib.check(self.lib.calm_grad_accum(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                            acc_ptrs_dev.data_ptr(), _ptr(plan.scratch), int(bool(first)), _stream()),
                   "calm_grad_accum")

    def grad_stats_scratch_floats(self, plan):
        """calm_grad_stats_scratch_floats for the table of `plan` (host only)."""
        return int(self.lib.calm_grad_stats_scratch_floats(plan.n, plan.n_chunks))

    def grad_stats(self, plan, grads, hp, grad_scale, out, summary, scratch):
        """calm_grad_stats over the table of `plan` with this step's gradient pointers, uploaded as for optim_step (the
        optim_step that follows with the same gradients then uploads nothing).  hp as for optim_step (beta1, beta2, eps
        are read; the step count is plan.step_dev).  out: uint8 device tensor of plan.n calm_grad_stat records, summary:
        int32[4], both initialised by the caller (counts 0, firsts -1); scratch: the caller's OWN float32 buffer of
        grad_stats_scratch_floats(plan) elements — never plan.scratch, which belongs to the step."""
        if out.numel() != plan.n * C.sizeof(_lib.GradStat) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError("grad_stats expects one 32-byte calm_grad_stat record per tensor of the plan (uint8)")
        if summary.numel() != 4 or summary.dtype != torch.int32:
            raise ValueError("grad_stats expects an int32[4] summary")
        if scratch.dtype != torch.float32 or scratch.numel() < self.grad_stats_scratch_floats(plan):
            raise ValueError("grad_stats: scratch smaller than calm_grad_stats_scratch_floats answers")
        plan.upload(np.asarray([_ptr(g) for g in grads], dtype=np.uint64))
        h = _lib.OptimHparams(*hp)
        _lib.check(self.lib.calm_grad_stats(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                            C.byref(h), plan.step_dev.data_ptr(), _ptr(grad_scale, True), out.data_ptr(),
                                            summary.data_ptr(), _ptr(scratch), _stream()), "calm_grad_stats")

    def sam_scratch_floats(self, plan):
        """calm_sam_scratch_floats for the table of `plan` (host only)."""
        return int(self.lib.calm_sam_scratch_floats(plan.n, plan.n_chunks))

    def sam_perturb(self, plan, grads, hp, grad_scale, backup_ptrs_dev, scratch, stats_out):
        """calm_sam_perturb over the table of `plan` with the gradient pointers of the first pass, uploaded as for
        optim_step.  hp = (rho, eps, eta, adaptive); grad_scale: device scalar or None; backup_ptrs_dev: int64 device
        tensor of plan.n addresses of fp32 storage shaped like the parameters; scratch: the caller's OWN float32 buffer of
        sam_scratch_floats(plan) elements — never plan.scratch, which belongs to the step; stats_out[3] <- norm,
        found_inf, scale."""
        if backup_ptrs_dev.numel() != plan.n or backup_ptrs_dev.dtype != torch.int64 or not backup_ptrs_dev.is_cuda:
            raise ValueError("sam_perturb expects one int64 backup address per tensor of the plan, on the device")
        if scratch.dtype != torch.float32 or scratch.numel() < self.sam_scratch_floats(plan):
            raise ValueError("sam_perturb: scratch smaller than calm_sam_scratch_floats answers")
        if stats_out.dtype != torch.float32 or stats_out.numel() != 3:
            raise ValueError("sam_perturb expects a float32[3] stats_out")
        plan.upload(np.asarray([_ptr(g) for g in grads], dtype=np.uint64))
        rho, eps, eta, adaptive = hp
        h = _lib.SamHparams(rho, eps, eta, int(adaptive))
        _lib.check(self.lib.calm_sam_perturb(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                             C.byref(h), _ptr(grad_scale, True), backup_ptrs_dev.data_ptr(), _ptr(scratch),
                                             _ptr(stats_out), _stream()), "calm_sam_perturb")

    def sam_restore(self, plan, backup_ptrs_dev):
        """calm_sam_restore: the bits calm_sam_perturb saved, back into the parameters of `plan`."""
        if backup_ptrs_dev.numel() != plan.n or backup_ptrs_dev.dtype != torch.int64 or not backup_ptrs_dev.is_cuda:
            raise ValueError("sam_restore expects one int64 backup address per tensor of the plan, on the device")
        _lib.check(self.lib.calm_sam_restore(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                             backup_ptrs_dev.data_ptr(), _stream()), "calm_sam_restore")

    # ---- weight EMA ---------------------------------------------------------------------
    def ema_plan(self, pairs):
        """pairs: [(fp32 parameter, its fp32 average of the same shape)] -> plan for ema_update / ema_swap."""
        return EmaPlan(self, pairs)

    def ema_update(self, plan, decay, schedule, skip=None):
        """ema += (1 - d) * (src - ema) over the plan; d = decay (EMA_CONSTANT) or min(decay, (1 + n) / (10 + n))
        (EMA_WARMUP) with n = plan.count_dev.  skip: device scalar; non-zero leaves averages and counter untouched."""
        _lib.check(self.lib.calm_ema_update(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                            decay, schedule, plan.count_dev.data_ptr(), _ptr(skip, True),
                                            _ptr(plan.weight_out), _stream()), "calm_ema_update")

    def ema_swap(self, plan):
        """Exchange every parameter with its average, in place."""
        _lib.check(self.lib.calm_ema_swap(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                          _stream()), "calm_ema_swap")

    # ---- training snapshots --------------------------------------------------------------
    def snapshot_plan(self, tensors, names=None):
        """tensors: the live CUDA tensors of a training state, in pack order -> SnapshotPlan (tables + packed buffer)."""
        return SnapshotPlan(self, tensors, names)

    def snapshot_pack(self, plan):
        """Gather every tensor of the plan into plan.packed: one launch on the current stream."""
        _lib.check(self.lib.calm_snapshot_pack(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                               plan.packed.data_ptr(), plan.packed_bytes, _stream()), "calm_snapshot_pack")

    def snapshot_unpack(self, plan):
        """Scatter plan.packed back into the tensors of the plan, in place: one launch on the current stream."""
        _lib.check(self.lib.calm_snapshot_unpack(plan.table_dev.data_ptr(), plan.n, plan.chunk_dev.data_ptr(), plan.n_chunks,
                                                 plan.packed.data_ptr(), plan.packed_bytes, _stream()), "calm_snapshot_unpack")

    # ---- LayerNorm --------------------------------------------------------------------
    def layernorm_fwd(self, x, w, y, mean, rstd, rows, D, eps):
        """y may be a bf16 tensor (bf16 pipeline: the output only feeds GEMMs)."""
        _lib.check(self.lib.calm_layernorm_fwd(_ptr(x), _ptr(w), _ptr(y, bf16_ok=True), _ptr(mean), _ptr(rstd), rows, D,
                                               eps, _st(y), _stream()), "calm_layernorm_fwd")

    def layernorm_bwd(self, dy, x, w, mean, rstd, dx, dw, rows, D, dx_add=None):
        _lib.check(self.lib.calm_layernorm_bwd(_ptr(dy, bf16_ok=True), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx),
                                               _ptr(dw), _ptr(dx_add, True), rows, D, _st(dy),
                                               self._partials(_lib.RED_LAYERNORM_BWD, rows, D, x.device), _stream()),
                   "calm_layernorm_bwd")

    def layernorm_bwd_part(self, dy, x, w, mean, rstd, dx, rows, D, dx_add=None):
        """layernorm_bwd without the sum over workgroups: -> (partials, shape) for reduce_partials_batch."""
        part, shape = self._own_partials(_lib.RED_LAYERNORM_BWD, rows, D, x.device), _lib.ReduceShape()
        _lib.check(self.lib.calm_part_layernorm_bwd(_ptr(dy, bf16_ok=True), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd),
                                                    _ptr(dx), _ptr(dx_add, True), rows, D, _st(dy), _ptr(part),
                                                    C.byref(shape), _stream()), "calm_part_layernorm_bwd")
        return part, shape

    # ---- bf16 weight copies --------------------------------------------------------------
    def cast_plan(self, pairs):
        """pairs: [(fp32 source tensor, bf16 destination tensor of the same numel)] -> plan for cast_run."""
        return CastPlan(self, pairs)

    # ---- fp8 (BASELINE config #5) ------------------------------------------------------
    def quantize_fp8(self, x, q_dtype):
        """Per-tensor scaled fp8 copy of a contiguous fp32 / bf16 tensor: returns (q, dq) with dq a device scalar
        (amax / FP8_MAX) for calm_gemm's a_dq / b_dq."""
        if not x.is_contiguous():
            raise TypeError("quantize_fp8 expects a contiguous tensor")
        q = torch.empty(x.shape, dtype=q_dtype, device=x.device)
        state = torch.empty(2, dtype=torch.float32, device=x.device)
        _lib.check(self.lib.calm_quantize_fp8(_ptr(x, bf16_ok=True), _st(x), x.numel(), q.data_ptr(), _st(q), _ptr(state),
                                              _stream()), "calm_quantize_fp8")
        return q, state[1:2]

    def transpose_u8(self, x):
        """[rows, cols] one-byte tensor -> its transpose [cols, rows] (contiguous)."""
        rows, cols = x.shape
        out = torch.empty(cols, rows, dtype=x.dtype, device=x.device)
        _lib.check(self.lib.calm_transpose_u8(x.data_ptr(), out.data_ptr(), rows, cols, _stream()), "calm_transpose_u8")
        return out

    def cast_bf16(self, src, dst):
        _lib.check(self.lib.calm_cast_bf16_one(_ptr(src), _ptr(dst, bf16_ok=True), src.numel(), _stream()),
                   "calm_cast_bf16_one")

    def cast_run(self, plan):
        _lib.check(self.lib.calm_cast_bf16(plan.table_dev.data_ptr(), plan.chunk_dev.data_ptr(), plan.n_chunks, _stream()),
                   "calm_cast_bf16")

    # ---- RoPE -------------------------------------------------------------------------
    def rope_fwd(self, content, xr, inv_freq, table, out, B, S, H, dc, dr):
        """content / xr / out: fp32 or bf16 tensors, independently."""
        _lib.check(self.lib.calm_rope_fwd(_ptr(content, True, bf16_ok=True), _ptr(xr, bf16_ok=True), _ptr(inv_freq),
                                          _ptr(table), _ptr(out, bf16_ok=True), B, S, H, dc, dr, _st(content), _st(xr),
                                          _st(out), _stream()), "calm_rope_fwd")

    def rope_bwd(self, d_out, xr, table, d_content, d_xr, d_inv_freq, B, S, H, dc, dr):
        _lib.check(self.lib.calm_rope_bwd(_ptr(d_out, bf16_ok=True), _ptr(xr, bf16_ok=True), _ptr(table),
                                          _ptr(d_content, True, bf16_ok=True), _ptr(d_xr, bf16_ok=True), _ptr(d_inv_freq),
                                          B, S, H, dc, dr, _st(d_out), _st(xr), _st(d_content), _st(d_xr),
                                          self._partials(_lib.RED_ROPE_BWD, B * S * H, dr, xr.device), _stream()),
                   "calm_rope_bwd")

    def rope_bwd_part(self, d_out, xr, table, d_content, d_xr, B, S, H, dc, dr):
        """rope_bwd without the sum over workgroups: -> (partials, shape) for reduce_partials_batch."""
        part, shape = self._own_partials(_lib.RED_ROPE_BWD, B * S * H, dr, xr.device), _lib.ReduceShape()
        _lib.check(self.lib.calm_part_rope_bwd(_ptr(d_out, bf16_ok=True), _ptr(xr, bf16_ok=True), _ptr(table),
                                               _ptr(d_content, True, bf16_ok=True), _ptr(d_xr, bf16_ok=True),
                                               B, S, H, dc, dr, _st(d_out), _st(xr), _st(d_content), _st(d_xr),
                                               _ptr(part), C.byref(shape), _stream()), "calm_part_rope_bwd")
        return part, shape

    # ---- softmax ----------------------------------------------------------------------
    def softmax_fwd(self, x, rows, cols):
        _lib.check(self.lib.calm_softmax_fwd(_ptr(x), rows, cols, _stream()), "calm_softmax_fwd")

    def softmax_bwd(self, p, dp, rows, cols):
        _lib.check(self.lib.calm_softmax_bwd(_ptr(p), _ptr(dp), rows, cols, _stream()), "calm_softmax_bwd")

    def softmax_bwd_heads(self, p, dp, dm, B, H, Sq, cols):
        _lib.check(self.lib.calm_softmax_bwd_heads(_ptr(p), _ptr(dp), _ptr(dm), B, H, Sq, cols, _stream()),
                   "calm_softmax_bwd_heads")

    def sum_heads(self, dl, dm, B, H, per_head):
        _lib.check(self.lib.calm_sum_heads(_ptr(dl), _ptr(dm), B, H, per_head, _stream()), "calm_sum_heads")

    # ---- fused latent-mask attention ---------------------------------------------------
    def attn_fwd_supported(self, Sq, Skv, H, hd):
        return bool(self.lib.calm_attention_fwd_supported(Sq, Skv, H, hd))

    def attn_fwd(self, q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, P, B, Sq, Skv, H, hd):
        _lib.check(self.lib.calm_attention_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(w1), _ptr(b1), _ptr(s1), _ptr(w2),
                                               _ptr(b2), _ptr(s2), _ptr(out), _ptr(R), _ptr(hp), _ptr(hg),
                                               _ptr(Mk), _ptr(P, True), B, Sq, Skv, H, hd, _stream()), "calm_attention_fwd")

    def attn_bwd_preferred(self, Sq, Skv, H, hd):
        return bool(self.lib.calm_attention_bwd_preferred(Sq, Skv, H, hd))

    def attn_bwd(self, q, k, v, dout, P, dS, dq, dk, dv, dM, B, Sq, Skv, H, hd):
        _lib.check(self.lib.calm_attention_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(dout), _ptr(P), _ptr(dS), _ptr(dq),
                                               _ptr(dk), _ptr(dv), _ptr(dM), B, Sq, Skv, H, hd, _stream()),
                   "calm_attention_bwd")

    # the same backward split around the mask-MLP backward (ops.LatentMaskAttentionFn): front writes dS and dM, back
    # takes dR and writes the complete dq, dk, dv — the two dR products ride on its contractions
    def attn_bwd_fold_preferred(self, Sq, Skv, H, hd):
        return bool(self.lib.calm_attention_bwd_fold_preferred(Sq, Skv, H, hd))

    def attn_bwd_front(self, v, dout, P, dS, dM, B, Sq, Skv, H, hd):
        _lib.check(self.lib.calm_attention_bwd_front(_ptr(v), _ptr(dout), _ptr(P), _ptr(dS), _ptr(dM), B, Sq, Skv, H, hd,
                                                     _stream()), "calm_attention_bwd_front")

    def attn_bwd_back(self, q, k, dout, P, dS, dR, dq, dk, dv, B, Sq, Skv, H, hd):
        _lib.check(self.lib.calm_attention_bwd_back(_ptr(q), _ptr(k), _ptr(dout), _ptr(P), _ptr(dS), _ptr(dR), _ptr(dq),
                                                    _ptr(dk), _ptr(dv), B, Sq, Skv, H, hd, _stream()),
                   "calm_attention_bwd_back")

    ATTN_OPT_BACK = 0
    ATTN_BACK_TABLE, ATTN_BACK_STRIPE, ATTN_BACK_RING = 0, 1, 2

    def attn_set_option(self, option, value):
        """calm_attention_set_option: ATTN_OPT_BACK = how the kernels of attn_bwd_back stage a head's stripe — the
        per-geometry table (default), the whole stripe, or the slab ring.  Returns the previous value."""
        prev = self.lib.calm_attention_set_option(int(option), int(value))
        if prev < 0:
            raise ValueError(f"calm_attention_set_option({option}, {value}) -> {prev}")
        return prev

    def attn_fwd_lse(self, q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, lse, B, Sq, Skv, H, hd):
        _lib.check(self.lib.calm_attention_fwd_lse(_ptr(q), _ptr(k), _ptr(v), _ptr(w1), _ptr(b1), _ptr(s1), _ptr(w2),
                                                   _ptr(b2), _ptr(s2), _ptr(out), _ptr(R), _ptr(hp), _ptr(hg),
                                                   _ptr(Mk), _ptr(lse), B, Sq, Skv, H, hd, _stream()),
                   "calm_attention_fwd_lse")

    def attn_bwd_lse_scratch_bytes(self, B, Sq, Skv, H, hd):
        """Bytes of scratch attn_bwd_lse needs; 0 = no fused instantiation for the shape."""
        return int(self.lib.calm_attention_bwd_lse_scratch_bytes(B, Sq, Skv, H, hd))

    def attn_bwd_lse(self, q, k, v, dout, Mk, lse, scratch, dq, dk, dv, dM, B, Sq, Skv, H, hd):
        """scratch: contiguous CUDA tensor of at least attn_bwd_lse_scratch_bytes(...) bytes (any dtype)."""
        if scratch is None or not scratch.is_cuda or not scratch.is_contiguous():
            raise TypeError("attn_bwd_lse: contiguous CUDA scratch tensor expected")
        _lib.check(self.lib.calm_attention_bwd_lse(_ptr(q), _ptr(k), _ptr(v), _ptr(dout), _ptr(Mk), _ptr(lse),
                                                   scratch.data_ptr(), scratch.numel() * scratch.element_size(),
                                                   _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dM), B, Sq, Skv, H, hd, _stream()),
                   "calm_attention_bwd_lse")

    def attn_infer(self, q, k, v, w1, b1, s1, w2, b2, s2, out, Mk, B, Sq, Skv, H, hd):
        _lib.check(self.lib.calm_attention_infer(_ptr(q), _ptr(k), _ptr(v), _ptr(w1), _ptr(b1), _ptr(s1), _ptr(w2),
                                                 _ptr(b2), _ptr(s2), _ptr(out), _ptr(Mk), B, Sq, Skv, H, hd, _stream()),
                   "calm_attention_infer")

    # ---- the same attention on the bf16 matrix pipe (bf16 pipeline) ----------------------
    def attn16_supported(self, S, H, hd):
        return bool(self.lib.calm_attention16_supported(S, H, hd))

    def attn16_fwd(self, q, k, v, w1, b1, s1, w2, b2, s2, out, R, hp, hg, Mk, MkT, lse, B, S, H, hd):
        h = lambda t: _ptr16(t)
        _lib.check(self.lib.calm_attention16_fwd(h(q), h(k), h(v), h(w1), _ptr(b1), _ptr(s1), h(w2), _ptr(b2), _ptr(s2),
                                                 h(out), h(R), h(hp), h(hg), h(Mk), h(MkT), _ptr(lse), B, S, H, hd,
                                                 _stream()), "calm_attention16_fwd")

    def attn16_infer(self, q, k, v, w1, b1, s1, w2, b2, s2, out, Mk, B, S, H, hd):
        h = lambda t: _ptr16(t)
        _lib.check(self.lib.calm_attention16_infer(h(q), h(k), h(v), h(w1), _ptr(b1), _ptr(s1), h(w2), _ptr(b2), _ptr(s2),
                                                   h(out), h(Mk), B, S, H, hd, _stream()), "calm_attention16_infer")

    def attn16_bwd(self, q, k, v, out, dout, Mk, MkT, lse, delta, dq, dk, dv, dM, B, S, H, hd):
        h = lambda t: _ptr16(t)
        _lib.check(self.lib.calm_attention16_bwd(h(q), h(k), h(v), h(out), h(dout), h(Mk), h(MkT), _ptr(lse), _ptr(delta),
                                                 h(dq), h(dk), h(dv), h(dM), B, S, H, hd, _stream()),
                   "calm_attention16_bwd")

    # ---- latent -----------------------------------------------------------------------
    def latent_fwd(self, mv, noise, z, std, kl_sum, rows, mvh):
        _lib.check(self.lib.calm_latent_fwd(_ptr(mv), _ptr(noise, True), _ptr(z), _ptr(std), _ptr(kl_sum), rows,
                                            mvh, self._partials(_lib.RED_LATENT_FWD, rows, mvh, mv.device), _stream()),
                   "calm_latent_fwd")

    def latent_bwd(self, dz, d_kl_sum, mv, noise, std, dmv, rows, mvh):
        _lib.check(self.lib.calm_latent_bwd(_ptr(dz, True), _ptr(d_kl_sum, True), _ptr(mv), _ptr(noise, True),
                                            _ptr(std), _ptr(dmv), rows, mvh, _stream()), "calm_latent_bwd")

    # ---- spectral norm ----------------------------------------------------------------
    def sn_plan(self, layers):
        """layers: list of (w2d, u, v, sigma) tensors.  Returns an SnPlan bound to their addresses."""
        n = len(layers)
        arr = (_lib.SnLayer * n)()
        for i, (w, u, v, sg) in enumerate(layers):
            rows = w.shape[0]
            cols = w.numel() // rows
            arr[i].w, arr[i].u, arr[i].v, arr[i].sigma = _ptr(w), _ptr(u), _ptr(v), _ptr(sg)
            arr[i].rows, arr[i].cols = rows, cols
        info = _lib.SnPlanInfo()
        _lib.check(self.lib.calm_sn_plan(arr, n, None, C.byref(info)), "calm_sn_plan")
        blob = np.zeros(info.blob_bytes, dtype=np.uint8)
        _lib.check(self.lib.calm_sn_plan(arr, n, blob.ctypes.data, C.byref(info)), "calm_sn_plan")
        dev = layers[0][0].device
        blob_dev = torch.from_numpy(blob).to(dev)
        scratch = torch.empty(int(info.scratch_floats), dtype=torch.float32, device=dev)
        key = tuple(t.data_ptr() for layer in layers for t in layer)
        return SnPlan(info, blob_dev, scratch, key)

    def sn_power_iter(self, plan, training):
        _lib.check(self.lib.calm_sn_power_iter(plan.blob_dev.data_ptr(), C.byref(plan.info), int(training), SN_EPS,
                                               _ptr(plan.scratch), _stream()), "calm_sn_power_iter")

    def sn_weight_bwd(self, G, w, u, v, sigma, ls, dW, d_ls, rows, cols):
        scratch = torch.empty(rows + 2, dtype=torch.float32, device=G.device)
        _lib.check(self.lib.calm_sn_weight_bwd(_ptr(G), _ptr(w), _ptr(u), _ptr(v), _ptr(sigma), _ptr(ls, True),
                                               _ptr(dW), _ptr(d_ls, True), rows, cols, _ptr(scratch), _stream()),
                   "calm_sn_weight_bwd")

    def sn_weight_bwd_batch(self, items):
        """items: [(G, w, u, v, sigma, ls, dW, d_ls, rows, cols)], the arguments of sn_weight_bwd — all of them in two
        launches per calm_sn_bwd_batch_max() layers, each layer bit-identical with the single form."""
        rowdot = torch.empty(sum(it[8] for it in items), dtype=torch.float32, device=items[0][0].device)
        ent = (_lib.SnBwdEntry * len(items))()
        off = 0
        for e, (G, w, u, v, sigma, ls, dW, d_ls, rows, cols) in zip(ent, items):
            e.G, e.w_orig, e.u, e.v, e.sigma, e.ls = _ptr(G), _ptr(w), _ptr(u), _ptr(v), _ptr(sigma), _ptr(ls, True)
            e.d_w_orig, e.d_ls, e.rowdot = _ptr(dW), _ptr(d_ls, True), rowdot.data_ptr() + 4 * off
            e.rows, e.cols = rows, cols
            off += rows
        _lib.check(self.lib.calm_sn_weight_bwd_batch(ent, len(items), _stream()), "calm_sn_weight_bwd_batch")

    # ---- tokenisation / conv ----------------------------------------------------------
    def image_to_rows(self, img, rows, B, S):
        _lib.check(self.lib.calm_image_to_rows(_ptr(img), _ptr(rows), B, S, _stream()), "calm_image_to_rows")

    def rows_to_image(self, rows, img, B, S):
        _lib.check(self.lib.calm_rows_to_image(_ptr(rows), _ptr(img), B, S, _stream()), "calm_rows_to_image")

    def grid_transpose(self, x, out, B, S):
        _lib.check(self.lib.calm_grid_transpose(_ptr(x), _ptr(out), B, S, _stream()), "calm_grid_transpose")

    def dwconv_fwd(self, x, w, inv_scale, bias, y, y_pre, act, B, S, Cch):
        _lib.check(self.lib.calm_dwconv3x3_fwd(_ptr(x), _ptr(w), _ptr(inv_scale, True), _ptr(bias, True), _ptr(y),
                                               _ptr(y_pre, True), act, B, S, Cch, _stream()), "calm_dwconv3x3_fwd")

    def dwconv_bwd(self, dz, x, w, inv_scale, dx, dw, db, B, S, Cch):
        _lib.check(self.lib.calm_dwconv3x3_bwd(_ptr(dz), _ptr(x), _ptr(w), _ptr(inv_scale, True), _ptr(dx),
                                               _ptr(dw), _ptr(db), B, S, Cch, _stream()), "calm_dwconv3x3_bwd")

    def cnn_fwd(self, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, out, B, S, hidden, residual=True):
        """residual=False: the bare proj(x) (a caller of the reference invoking `block.proj` on its own)."""
        _lib.check(self.lib.calm_cnn_residual_fwd(_ptr(x), _ptr(w0), _ptr(s0), _ptr(b0), _ptr(w2), _ptr(s2),
                                                  _ptr(b2), _ptr(w4), _ptr(s4), _ptr(b4), _ptr(out), B, S, hidden,
                                                  int(residual), _stream()), "calm_cnn_residual_fwd")

    def cnn_bwd(self, dy, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, dx, g0, gb0, g2, gb2, g4, gb4, B, S, hidden,
                residual=True):
        _lib.check(self.lib.calm_cnn_residual_bwd(_ptr(dy), _ptr(x), _ptr(w0), _ptr(s0), _ptr(b0), _ptr(w2),
                                                  _ptr(s2), _ptr(b2), _ptr(w4), _ptr(s4), _ptr(b4), _ptr(dx),
                                                  _ptr(g0), _ptr(gb0), _ptr(g2), _ptr(gb2), _ptr(g4), _ptr(gb4),
                                                  B, S, hidden, int(residual),
                                                  self._partials(_lib.RED_CNN_BWD, B, S, dy.device), _stream()),
                   "calm_cnn_residual_bwd")

    def cnn_bwd_part(self, dy, x, w0, s0, b0, w2, s2, b2, w4, s4, b4, dx, B, S, hidden, residual=True):
        """cnn_bwd without the sum over workgroups: -> (partials, shape), six segments g0 | gb0 | g2 | gb2 | g4 | gb4."""
        part, shape = self._own_partials(_lib.RED_CNN_BWD, B, S, dy.device), _lib.ReduceShape()
        _lib.check(self.lib.calm_part_cnn_residual_bwd(_ptr(dy), _ptr(x), _ptr(w0), _ptr(s0), _ptr(b0), _ptr(w2),
                                                       _ptr(s2), _ptr(b2), _ptr(w4), _ptr(s4), _ptr(b4), _ptr(dx),
                                                       B, S, hidden, int(residual), _ptr(part), C.byref(shape),
                                                       _stream()), "calm_part_cnn_residual_bwd")
        return part, shape

    # ---- loss end of the step (csrc/loss.hip) -------------------------------------------
    def soft_ce_fwd(self, logits, targets, row_stats, loss, metrics, B, C):
        """logits / targets [B,C] with unit column stride (any row stride); row_stats [B,2], loss 0-dim, metrics [4] or None."""
        _lib.check(self.lib.calm_soft_ce_fwd(_ptr(logits), logits.stride(0), _ptr(targets), targets.stride(0),
                                             _ptr(row_stats), _ptr(loss), _ptr(metrics, True), B, C,
                                             self._partials(_lib.RED_SOFT_CE, B, C, logits.device), _stream()),
                   "calm_soft_ce_fwd")

    def soft_ce_bwd(self, logits, targets, row_stats, dloss, dlogits, B, C):
        _lib.check(self.lib.calm_soft_ce_bwd(_ptr(logits), logits.stride(0), _ptr(targets), targets.stride(0),
                                             _ptr(row_stats), _ptr(dloss), _ptr(dlogits), B, C, _stream()),
                   "calm_soft_ce_bwd")

    # binary cross-entropy with logits: logits / targets fp32 [B,C] with unit column stride (any row stride); flags: a sum
    # of _lib.BCE_SUM_CLASSES / BCE_THRESHOLD; loss 0-dim, metrics [4] or None; dlogits contiguous [B,C]
    def bce_fwd(self, logits, targets, flags, threshold, loss, metrics, B, C):
        _lib.check(self.lib.calm_bce_fwd(_ptr(logits), logits.stride(0), _ptr(targets), targets.stride(0), int(flags),
                                         float(threshold), _ptr(loss), _ptr(metrics, True), B, C,
                                         self._partials(_lib.RED_BCE, B, C, logits.device), _stream()), "calm_bce_fwd")

    def bce_bwd(self, logits, targets, flags, threshold, dloss, dlogits, B, C):
        _lib.check(self.lib.calm_bce_bwd(_ptr(logits), logits.stride(0), _ptr(targets), targets.stride(0), int(flags),
                                         float(threshold), _ptr(dloss), _ptr(dlogits), B, C, _stream()), "calm_bce_bwd")

    # knowledge distillation: logits / targets fp32 and teacher fp32 or bf16, all [B,C] with unit column stride (any row
    # stride); row_stats [B, DISTILL_ROW_STATS]; mode "soft" | "hard"; metrics / dmetrics [4] or None
    _DISTILL_MODES = {"soft": _lib.DISTILL_SOFT, "hard": _lib.DISTILL_HARD}

    def _distill_inputs(self, what, logits, teacher, targets, row_stats, mode, B, C):
        if mode not in self._DISTILL_MODES:
            raise ValueError(f'{what}: mode is "soft" or "hard", got {mode!r}')
        for name, t in (("logits", logits), ("teacher", teacher), ("targets", targets)):
            if t.dim() != 2 or tuple(t.shape) != (B, C) or t.stride(1) != 1:
                raise ValueError(f"{what}: {name} is [B,C] with unit column stride")
        if row_stats.numel() < B * _lib.DISTILL_ROW_STATS or not row_stats.is_contiguous():
            raise ValueError(f"{what}: row_stats is contiguous [B, {_lib.DISTILL_ROW_STATS}]")
        return (_ptr(logits), logits.stride(0), _ptr(teacher, bf16_ok=True), teacher.stride(0), _st(teacher), _ptr(targets),
                targets.stride(0))

    def distill_fwd(self, logits, teacher, targets, temperature, alpha, mode, row_stats, loss, metrics, dmetrics, B, C):
        head = self._distill_inputs("distill_fwd", logits, teacher, targets, row_stats, mode, B, C)
        for name, t in (("metrics", metrics), ("dmetrics", dmetrics)):
            if t is not None and (t.numel() < 4 or not t.is_contiguous()):
                raise ValueError(f"distill_fwd: {name} holds four contiguous floats")
        _lib.check(self.lib.calm_distill_fwd(*head, float(temperature), float(alpha), self._DISTILL_MODES[mode],
                                             _ptr(row_stats), _ptr(loss), _ptr(metrics, True), _ptr(dmetrics, True), B, C,
                                             self._partials(_lib.RED_DISTILL, B, C, logits.device), _stream()),
                   "calm_distill_fwd")

    def distill_bwd(self, logits, teacher, targets, temperature, alpha, mode, row_stats, dloss, dlogits, B, C):
        head = self._distill_inputs("distill_bwd", logits, teacher, targets, row_stats, mode, B, C)
        if tuple(dlogits.shape) != (B, C) or not dlogits.is_contiguous():
            raise ValueError("distill_bwd: dlogits is contiguous [B,C]")
        _lib.check(self.lib.calm_distill_bwd(*head, float(temperature), float(alpha), self._DISTILL_MODES[mode],
                                             _ptr(row_stats), _ptr(dloss), _ptr(dlogits), B, C, _stream()),
                   "calm_distill_bwd")

    def distill_scratch_floats(self, B, C):
        """Floats of `partials` one distill_fwd call at (B, C) writes (calm_reduce_scratch_floats, cached)."""
        need = self._scratch_need.get((_lib.RED_DISTILL, B, C))
        if need is None:
            need = self._scratch_need[(_lib.RED_DISTILL, B, C)] = int(self.lib.calm_reduce_scratch_floats(_lib.RED_DISTILL, B, C))
        return need

    def huber_tokens_fwd(self, tokens, x, delta, loss, B, S):
        _lib.check(self.lib.calm_huber_tokens_fwd(_ptr(tokens), _ptr(x), float(delta), _ptr(loss), B, S,
                                                  self._partials(_lib.RED_HUBER, B * S, 3 * S, tokens.device), _stream()),
                   "calm_huber_tokens_fwd")

    def huber_tokens_bwd(self, tokens, x, delta, dloss, dtokens, B, S):
        _lib.check(self.lib.calm_huber_tokens_bwd(_ptr(tokens), _ptr(x), float(delta), _ptr(dloss), _ptr(dtokens), B, S,
                                                  _stream()), "calm_huber_tokens_bwd")

    def top1_count(self, logits, labels, metrics, B, C):
        if not labels.is_cuda or labels.dtype != torch.int64 or not labels.is_contiguous():
            raise TypeError("top1_count expects contiguous int64 CUDA labels")
        _lib.check(self.lib.calm_top1_count(_ptr(logits), logits.stride(0), labels.data_ptr(), _ptr(metrics), B, C,
                                            _stream()), "calm_top1_count")

    def eval_metrics(self, logits, labels, ks, counts, loss_sum, confusion, B, C, partials=None):
        """calm_eval_metrics: logits [B,C] fp32 or bf16 with unit column stride (any row stride), labels [B] int64; the
        batch's tallies are ADDED to counts (int64 [7 + 2C]: rows, skipped, nonfinite, hits@ks[0..3], support[C],
        hits1[C]), loss_sum (float64 [1]) and confusion (int64 [C,C] or None).  ks: 1 to 4 integers >= 1.  partials: the
        caller's own record scratch (fp32, >= 4 * B elements) — the shared reduction scratch when None."""
        if not labels.is_cuda or labels.dtype != torch.int64 or not labels.is_contiguous():
            raise TypeError("eval_metrics expects contiguous int64 CUDA labels")
        for name, t, dt in (("counts", counts, torch.int64), ("loss_sum", loss_sum, torch.float64),
                            ("confusion", confusion, torch.int64)):
            if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous()):
                raise TypeError(f"eval_metrics expects a contiguous {dt} CUDA tensor for {name}")
        if counts.numel() < _lib.EVAL_COUNTS_HEAD + 2 * C or (confusion is not None and confusion.numel() < C * C):
            raise ValueError("eval_metrics: counts holds 7 + 2 C values, confusion C * C")
        if partials is None:
            part = self._partials(_lib.RED_EVAL, B, C, logits.device)
        else:
            if partials.numel() < 4 * B:
                raise ValueError("eval_metrics: partials holds one 16-byte record per row")
            part = _ptr(partials)
        karr = (_lib.C.c_int32 * len(ks))(*[int(k) for k in ks])
        _lib.check(self.lib.calm_eval_metrics(_ptr(logits, bf16_ok=True), logits.stride(0), _st(logits), labels.data_ptr(),
                                              karr, len(ks), counts.data_ptr(), loss_sum.data_ptr(),
                                              None if confusion is None else confusion.data_ptr(), B, C, part, _stream()),
                   "calm_eval_metrics")

    # ---- the generative job on row tokens (csrc/recon.hip) -------------------------------
    def huber_rows_fwd(self, tokens, target, delta, loss, n):
        """nn.HuberLoss(delta) between two contiguous fp32 tensors of one flat layout, n elements; loss 0-dim."""
        _lib.check(self.lib.calm_recon_huber_rows_fwd(_ptr(tokens), _ptr(target), float(delta), _ptr(loss), n,
                                                      self._partials(_lib.RED_HUBER, n, 1, tokens.device), _stream()),
                   "calm_recon_huber_rows_fwd")

    def huber_rows_bwd(self, tokens, target, delta, dloss, dtokens, n):
        _lib.check(self.lib.calm_recon_huber_rows_bwd(_ptr(tokens), _ptr(target), float(delta), _ptr(dloss), _ptr(dtokens),
                                                      n, _stream()), "calm_recon_huber_rows_bwd")

    def recon_metrics(self, tokens, target, layout, mean, std, delta, want_ssim, sums, B, S, partials=None):
        """calm_recon_metrics: generated tokens [B,S,3S] fp32 or bf16 against the fp32 target, rows [B,S,3S]
        (layout = RECON_ROWS) or image [B,3,S,S] (RECON_NCHW), both contiguous; the batch's tallies are ADDED to sums
        (float64 [8]: images, non-finite images, Huber / abs / square sums, elements, PSNR sum, SSIM sum).  partials: the
        caller's own record scratch (fp32) — the shared reduction scratch when None."""
        if not sums.is_cuda or sums.dtype != torch.float64 or sums.numel() < 8 or not sums.is_contiguous():
            raise TypeError("recon_metrics expects a contiguous float64 CUDA tensor of 8 values for sums")
        if not (tokens.is_contiguous() and target.is_contiguous()) or tokens.numel() != 3 * B * S * S \
                or target.numel() != tokens.numel():
            raise ValueError("recon_metrics: contiguous tokens [B,S,3S] and a target of as many elements expected")
        if partials is None:
            part = self._partials(_lib.RED_RECON, B, S, tokens.device)
        else:
            if partials.numel() < self.recon_scratch_floats(B, S):
                raise ValueError("recon_metrics: partials is smaller than calm_reduce_scratch_floats(CALM_RED_RECON, B, S)")
            part = _ptr(partials)
        m3, s3 = (_lib.C.c_float * 3)(*[float(v) for v in mean]), (_lib.C.c_float * 3)(*[float(v) for v in std])
        _lib.check(self.lib.calm_recon_metrics(_ptr(tokens, bf16_ok=True), _st(tokens), _ptr(target), int(layout), m3, s3,
                                               float(delta), int(bool(want_ssim)), sums.data_ptr(), B, S, part, _stream()),
                   "calm_recon_metrics")

    def recon_scratch_floats(self, B, S):
        """Floats of record scratch one recon_metrics call at (B, S) writes (calm_reduce_scratch_floats, cached)."""
        need = self._scratch_need.get((_lib.RED_RECON, B, S))
        if need is None:
            need = self._scratch_need[(_lib.RED_RECON, B, S)] = int(self.lib.calm_reduce_scratch_floats(_lib.RED_RECON, B, S))
        return need

    # ---- dropout (csrc/dropout.hip) -----------------------------------------------------
    def dropout(self, x, residual, y, n, p, key, e0=0):
        """y[j] = x[j] * mask(e0 + j) / (1 - p) + residual[j] with the Philox mask of `key` (device int64 [2] = seed, offset,
        read by the kernel); x / residual / y fp32 or bf16 independently, residual may be None, y may be x."""
        if key is None or not key.is_cuda or key.dtype != torch.int64 or key.numel() != 2 or not key.is_contiguous():
            raise TypeError("dropout expects its key as a contiguous int64 CUDA tensor of two elements (seed, offset)")
        _lib.check(self.lib.calm_dropout(_ptr(x, bf16_ok=True), _ptr(residual, True, bf16_ok=True), _ptr(y, bf16_ok=True),
                                         n, e0, float(p), key.data_ptr(), _st(x), _st(residual), _st(y), _stream()),
                   "calm_dropout")

    def drop_path(self, x, residual, y, B, L, p, key, sample0=0):
        """y[b, j] = x[b, j] * mask(sample0 + b) / (1 - p) + residual[b, j] over B rows of L elements: stochastic depth with
        ONE decision per row, the dropout mask's decision for element index sample0 + b under `key` (device int64 [2] = seed,
        offset, read by the kernel); x / residual / y fp32 or bf16 independently, residual may be None, y may be x."""
        if key is None or not key.is_cuda or key.dtype != torch.int64 or key.numel() != 2 or not key.is_contiguous():
            raise TypeError("drop_path expects its key as a contiguous int64 CUDA tensor of two elements (seed, offset)")
        _lib.check(self.lib.calm_drop_path(_ptr(x, bf16_ok=True), _ptr(residual, True, bf16_ok=True), _ptr(y, bf16_ok=True),
                                           B, L, sample0, float(p), key.data_ptr(), _st(x), _st(residual), _st(y),
                                           _stream()),
                   "calm_drop_path")

    # ---- masked image modelling (csrc/mim.hip) ------------------------------------------
    @staticmethod
    def _mim_mask(who, mask, B, P):
        if mask is None or not mask.is_cuda or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != B * P:
            raise TypeError(f"{who} expects its mask as a contiguous uint8 CUDA tensor [B, P] = [{B}, {P}]")
        return mask.data_ptr()

    def mim_draw(self, mask, B, G, k, key, sample0=0):
        """mask [B, G * G] uint8: exactly k patches of every sample set, the k lowest-ranked words of the dropout generator
        at element indices (sample0 + b) * 1024 + i under `key` (device int64 [2] = seed, offset, read by the kernel)."""
        if key is None or not key.is_cuda or key.dtype != torch.int64 or key.numel() != 2 or not key.is_contiguous():
            raise TypeError("mim_draw expects its key as a contiguous int64 CUDA tensor of two elements (seed, offset)")
        _lib.check(self.lib.calm_mim_draw(self._mim_mask("mim_draw", mask, B, G * G), B, G, k, sample0, key.data_ptr(),
                                          _stream()), "calm_mim_draw")

    def mim_apply(self, x, y, mask, fill, B, S, p):
        """y = mask ? fill[channel] : x over row tokens [B,S,3S] (contiguous fp32; y may be x); fill: three floats."""
        f3 = (_lib.C.c_float * 3)(*[float(v) for v in fill])
        _lib.check(self.lib.calm_mim_apply(_ptr(x), _ptr(y), self._mim_mask("mim_apply", mask, B, (S // p) ** 2), f3, B, S, p,
                                           _stream()), "calm_mim_apply")

    def mim_huber_fwd(self, tokens, target, mask, delta, loss, B, S, p, masked):
        """Huber(delta) between two contiguous fp32 [B,S,3S] tensors, mean over the 3 p^2 `masked` masked elements; loss 0-dim."""
        _lib.check(self.lib.calm_mim_huber_fwd(_ptr(tokens), _ptr(target), self._mim_mask("mim_huber_fwd", mask, B, (S // p) ** 2),
                                               float(delta), _ptr(loss), B, S, p, int(masked),
                                               self._partials(_lib.RED_MIM, B, S, tokens.device), _stream()),
                   "calm_mim_huber_fwd")

    def mim_huber_bwd(self, tokens, target, mask, delta, dloss, dtokens, B, S, p, masked):
        _lib.check(self.lib.calm_mim_huber_bwd(_ptr(tokens), _ptr(target), self._mim_mask("mim_huber_bwd", mask, B, (S // p) ** 2),
                                               float(delta), _ptr(dloss), _ptr(dtokens), B, S, p, int(masked), _stream()),
                   "calm_mim_huber_bwd")

    # ---- k-NN probe (csrc/knn.hip) --------------------------------------------------------
    @staticmethod
    def _knn_state(who, best_sim, best_idx, Nq, k):
        for name, t, dt in (("best_sim", best_sim, torch.float32), ("best_idx", best_idx, torch.int64)):
            if t is None or not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != (Nq, k):
                raise TypeError(f"{who} expects {name} as a contiguous {dt} CUDA tensor [Nq, k] = [{Nq}, {k}]")

    def knn_normalize(self, x, out, bad, N, D):
        """out[i] = x[i] / ||x[i]|| for x [N, D] fp32 or bf16 with unit column stride (any row stride), out fp32 [N, D]
        contiguous; a row with a non-finite element or a zero norm becomes +0.0 and bad (int64 CUDA [1]) gains 1."""
        if x.dim() != 2 or tuple(x.shape) != (N, D) or x.stride(1) != 1 or tuple(out.shape) != (N, D) or not out.is_contiguous():
            raise ValueError(f"knn_normalize: x [N, D] = [{N}, {D}] with unit column stride and a contiguous out [N, D] expected")
        if not bad.is_cuda or bad.dtype != torch.int64 or bad.numel() < 1:
            raise TypeError("knn_normalize expects bad as an int64 CUDA tensor of one element")
        _lib.check(self.lib.calm_knn_normalize(_ptr(x, bf16_ok=True), x.stride(0) if N > 1 else max(x.stride(0), D), _st(x),
                                               _ptr(out), bad.data_ptr(), N, D, _stream()), "calm_knn_normalize")

    def knn_merge(self, sims, base, best_sim, best_idx, Nq, n, k):
        """The running top-k state (best_sim fp32 [Nq, k], best_idx int64 [Nq, k]; empty slot = (-inf, -1)) merged with the
        similarities sims [Nq, n] (fp32, unit column stride, any row stride) of the bank items base .. base + n - 1, under
        the order similarity descending, then bank index ascending."""
        if sims.dim() != 2 or tuple(sims.shape) != (Nq, n) or sims.stride(1) != 1:
            raise ValueError(f"knn_merge: sims [Nq, n] = [{Nq}, {n}] with unit column stride expected")
        self._knn_state("knn_merge", best_sim, best_idx, Nq, k)
        _lib.check(self.lib.calm_knn_merge(_ptr(sims), sims.stride(0) if Nq > 1 else max(sims.stride(0), n), int(base),
                                           best_sim.data_ptr(), best_idx.data_ptr(), Nq, n, k, _stream()), "calm_knn_merge")

    def knn_vote(self, best_sim, best_idx, bank_labels, inv_T, scores, Nq, k, C):
        """scores [Nq, C] (fp32, unit column stride) = the votes of the state's neighbours for their labels (bank_labels
        int64 CUDA [Nb]) with weight exp((sim - the row's largest sim) * inv_T); every element is overwritten."""
        self._knn_state("knn_vote", best_sim, best_idx, Nq, k)
        if not bank_labels.is_cuda or bank_labels.dtype != torch.int64 or bank_labels.dim() != 1 or not bank_labels.is_contiguous():
            raise TypeError("knn_vote expects bank_labels as a contiguous int64 CUDA tensor [Nb]")
        if scores.dim() != 2 or tuple(scores.shape) != (Nq, C) or scores.stride(1) != 1:
            raise ValueError(f"knn_vote: scores [Nq, C] = [{Nq}, {C}] with unit column stride expected")
        _lib.check(self.lib.calm_knn_vote(best_sim.data_ptr(), best_idx.data_ptr(), bank_labels.data_ptr(), bank_labels.numel(),
                                          float(inv_T), _ptr(scores), scores.stride(0) if Nq > 1 else max(scores.stride(0), C),
                                          Nq, k, C, _stream()), "calm_knn_vote")

    # ---- helpers ----------------------------------------------------------------------
    def add(self, a, b, out, n):
        _lib.check(self.lib.calm_add(_ptr(a), _ptr(b), _ptr(out), n, _stream()), "calm_add")

    def gelu_fwd(self, x, y, n):
        _lib.check(self.lib.calm_gelu_fwd(_ptr(x), _ptr(y), n, _stream()), "calm_gelu_fwd")

    def gelu_bwd(self, dy, z, dz, n):
        _lib.check(self.lib.calm_gelu_bwd(_ptr(dy), _ptr(z), _ptr(dz), n, _stream()), "calm_gelu_bwd")

    def colsum(self, x, out, rows, cols):
        _lib.check(self.lib.calm_colsum(_ptr(x, bf16_ok=True), _ptr(out), rows, cols, _st(x),
                                        self._partials(_lib.RED_COLSUM, rows, cols, x.device), _stream()), "calm_colsum")

    def colsum_part(self, x, rows, cols):
        """colsum without the sum over workgroups: -> (partials, shape) for reduce_partials_batch."""
        part, shape = self._own_partials(_lib.RED_COLSUM, rows, cols, x.device), _lib.ReduceShape()
        _lib.check(self.lib.calm_part_colsum(_ptr(x, bf16_ok=True), rows, cols, _st(x), _ptr(part), C.byref(shape),
                                             _stream()), "calm_part_colsum")
        return part, shape

    def row_scale(self, x, s, out, rows, cols):
        _lib.check(self.lib.calm_row_scale(_ptr(x), _ptr(s), _ptr(out, bf16_ok=True), rows, cols, _st(out), _stream()),
                   "calm_row_scale")

    def mean_seq_fwd(self, x, y, B, S, D):
        _lib.check(self.lib.calm_mean_seq_fwd(_ptr(x), _ptr(y), B, S, D, _stream()), "calm_mean_seq_fwd")

    def mean_seq_bwd(self, dy, dx, B, S, D):
        _lib.check(self.lib.calm_mean_seq_bwd(_ptr(dy), _ptr(dx), B, S, D, _stream()), "calm_mean_seq_bwd")


_backend = None


def get_backend():
    """The product backend.  Raises RuntimeError when libcalmvit_hip.so is not built/loadable."""
    global _backend
    if _backend is None:
        _backend = HipBackend()
    return _backend


@contextlib.contextmanager
def use_backend(b):
    """TEST HOOK ONLY (tests/): run the host logic against another implementation of the C-ABI."""
    global _backend
    old = _backend
    _backend = b
    try:
        yield b
    finally:
        _backend = old
