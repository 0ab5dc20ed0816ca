"""The training loop around the hot path (hp:297-351): micro-steps with gradient accumulation,
the learning-rate schedule, and one HD-PiSSA optimizer step (hp:352-398 -> HDPissaStep) every
``accumulation_steps`` micro-batches.

Kept from the reference: loss / accumulation_steps per micro-batch (hp:326), the schedule
evaluated at the step counter BEFORE its increment (hp:338-350), one step per accumulation
boundary ((i + 1) % accumulation_steps == 0, hp:335), the per-step loss log = the sum over the
micro-batches of the rank-averaged loss (hp:328-336).

Changed: the reference all-reduces the loss and reads it back to the host
(``.item()``) on EVERY micro-batch -- a collective and a device synchronisation per micro-step,
for logging only (the gradients do not depend on it).  Here, by default (``loss_sync="step"``),
the micro-batch losses are summed on the device in float64 and reduced / read back once per
optimizer step; ``loss_sync="micro"`` reproduces the reference's per-micro-step cadence.

Added (opt-in, ``max_grad_norm=``; the reference does not clip): the step clips the global gradient norm
and skips a non-finite step on the device (HDPissaStep).  ``grad_norm_list`` then holds the norm of every
optimizer step and ``skipped_steps`` the running count of skipped ones.  With ``loss_sync="step"`` the
loss read-back moves behind the step and fetches the step's clip record in the same transfer: still one
synchronisation per optimizer step.

Added (opt-in, ``merge_rounding="stochastic"``, ``sr_seed=``; the reference rounds to nearest): bf16 weights
take the step's update by stochastic rounding from the float32 sum (HDPissaStep).  Nothing is added to the
checkpoint: the rounding stream is a function of ``t`` and ``sr_seed``.

Added (opt-in, ``compute_dtype=torch.bfloat16``; the reference computes in the precision it stores): the model
forward of every micro-batch runs under ``torch.autocast(dtype=compute_dtype)``.  The adapter layers are
configured by ``replace_with_custom_layer(compute_dtype=)``: float32 master weights, a bf16 copy for the base
GEMMs, kept current by the step.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from .schedule import lr_at
from .step import HDPissaStep


class HDPissaTrainer:
    def __init__(self, model: nn.Module, world_size: int, rank: int, lr: float, total_steps: int,
                 accumulation_steps: int = 1, warmup_steps: int = 0, warmup_ratio: float = 0.0,
                 schedule: str = "cosine", exchange: str = "gather", loss_sync: str = "step", comm=None, ops=None,
                 beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 max_grad_norm: Optional[float] = None, merge_rounding: str = "nearest",
                 sr_seed: Optional[int] = None, compute_dtype: Optional[torch.dtype] = None):
        if compute_dtype not in (None, torch.bfloat16):
            raise ValueError(f"compute_dtype must be None or torch.bfloat16, got {compute_dtype!r}")
        self.compute_dtype = compute_dtype
        if loss_sync not in ("step", "micro"):
            raise ValueError("loss_sync must be 'step' or 'micro'")
        if accumulation_steps < 1:
            raise ValueError("accumulation_steps must be >= 1 (the reference divides the global "
                             "accumulation by world_size, hp:266)")
        self.model = model
        self.world_size, self.rank = world_size, rank
        self.initial_lr = lr
        self.total_steps = total_steps
        if warmup_steps == 0 and warmup_ratio > 0:          # hp:306-307
            warmup_steps = int(warmup_ratio * total_steps)
        self.warmup_steps = warmup_steps
        self.schedule = schedule
        self.accumulation_steps = accumulation_steps
        self.loss_sync = loss_sync
        self.stepper = HDPissaStep(model, world_size, rank, comm=comm, ops=ops, exchange=exchange, beta1=beta1,
                                   beta2=beta2, eps=eps, max_grad_norm=max_grad_norm, merge_rounding=merge_rounding,
                                   sr_seed=sr_seed)
        self.max_grad_norm = self.stepper.max_grad_norm
        self.grad_norm_list: List[float] = []   # per optimizer step (max_grad_norm set)
        self.skipped_steps = 0                  # optimizer steps skipped for a non-finite gradient norm
        self.t = 0                 # optimizer steps taken (hp:300, 350)
        self.micro = 0             # micro-batches seen in the current epoch (the reference's i)
        self.loss_list: List[float] = []
        self.lr_list: List[float] = []
        self._acc_host = 0.0       # loss_sync == "micro"
        self._acc_dev: Optional[torch.Tensor] = None  # loss_sync == "step"

    def _reduce(self, x: torch.Tensor) -> torch.Tensor:
        if self.world_size > 1 and dist.is_available() and dist.is_initialized():
            dist.all_reduce(x, op=dist.ReduceOp.SUM)
        return x

    def micro_step(self, batch: Dict[str, torch.Tensor]) -> bool:
        """One micro-batch (hp:321-333); runs the optimizer step at an accumulation boundary
        (hp:335-398).  Returns True when a step ran."""
        dev = next(self.model.parameters()).device
        input_ids = batch["input_ids"].to(dev, non_blocking=True)
        attention_mask = batch["attention_mask"].to(dev, non_blocking=True)
        labels = batch["labels"].to(dev, non_blocking=True)
        if self.compute_dtype is not None:
            with torch.autocast(dev.type, dtype=self.compute_dtype):
                outputs = self.model(input_ids=input_ids, attention_mask=attention_mask, labels=labels)
        else:
            outputs = self.model(input_ids=input_ids, attention_mask=attention_mask, labels=labels)
        loss = outputs.loss / float(self.accumulation_steps)
        if self.loss_sync == "micro":
            avg = self._reduce(loss.detach().clone()) / self.world_size
            self._acc_host += avg.item()
        else:
            v = loss.detach().double()
            self._acc_dev = v if self._acc_dev is None else self._acc_dev + v
        loss.backward()
        self.micro += 1
        if self.micro % self.accumulation_steps != 0:
            return False
        self.optimizer_step()
        return True

    def optimizer_step(self) -> None:
        if self.max_grad_norm is not None:
            return self._optimizer_step_clipped()
        if self.loss_sync == "micro":
            acc = self._acc_host
        else:
            acc = float(self._reduce(self._acc_dev).item()) / self.world_size if self._acc_dev is not None else 0.0
        self.loss_list.append(acc)                            # hp:336
        lr = lr_at(self.t, self.initial_lr, self.warmup_steps, self.total_steps, self.schedule)  # hp:338-344
        self.lr_list.append(lr)
        self.t += 1                                           # hp:350
        self.stepper.step(lr, self.t)                         # hp:352-398
        self._acc_host, self._acc_dev = 0.0, None             # hp:400

    def _optimizer_step_clipped(self) -> None:
        """optimizer_step with the clip record: the step first, then ONE read-back that brings the window's
        loss (loss_sync="step") and the record of the step that just ran."""
        from ._lib import clip_record
        acc_dev = None
        if self.loss_sync == "step" and self._acc_dev is not None:
            acc_dev = self._reduce(self._acc_dev).reshape(1)   # (enqueued before the step, read after it)
        lr = lr_at(self.t, self.initial_lr, self.warmup_steps, self.total_steps, self.schedule)  # hp:338-344
        self.t += 1                                           # hp:350
        self.stepper.step(lr, self.t)                         # hp:352-398
        rec = self.stepper.clip_state
        if acc_dev is not None:
            raw = torch.cat([rec, acc_dev.to(rec.device).view(torch.uint8)]).cpu()
            acc = float(raw[rec.numel():].view(torch.float64).item()) / self.world_size
        else:
            raw = rec.cpu()
            acc = self._acc_host if self.loss_sync == "micro" else 0.0
        info = clip_record(raw[:rec.numel()].numpy().tobytes())
        self.loss_list.append(acc)                            # hp:336
        self.lr_list.append(lr)
        self.grad_norm_list.append(info["norm"])
        self.skipped_steps = info["skipped_total"]
        self._acc_host, self._acc_dev = 0.0, None             # hp:400

    def train_epoch(self, dataloader, epoch: int = 0) -> List[float]:
        """hp:316-335 for one epoch: every micro-batch of this rank's shard.  As the reference does at
        each epoch start (hp:317), the accumulated loss restarts at 0: micro-batches of a previous
        epoch that did not complete an accumulation window are not carried into this epoch's log
        (their gradients are, as in the reference: nothing clears .grad between epochs)."""
        sampler = getattr(dataloader, "sampler", None)
        if hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        self.micro = 0
        self._acc_host, self._acc_dev = 0.0, None             # hp:317
        for batch in dataloader:
            self.micro_step(batch)
        return self.loss_list
