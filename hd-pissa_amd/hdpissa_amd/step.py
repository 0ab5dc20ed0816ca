"""The HD-PiSSA optimizer step: hp:352-398 on MI355X.

Reference, per module per step: ~20 elementwise launches of Adam, 4 all_gathers (dA, dB and
the *constant* A, B), 4*Wn zeros_like, Wn x (3 GEMMs + 3 elementwise over out x in) and a
merge -- ~48 N Wn bytes of HBM traffic per rank.  Here, per arena (all modules):

  1. K3  one Adam launch over the flat arena: grad (x1e16) -> m, v -> delta; clears grad.
         (Wn = 1 with single-segment H2 plans -- bf16 W, r >= 32: Adam runs inside the plan's operand
         preparation instead, writing the delta halves of the fp16 panels as it goes)
  2. exchange -- three interchangeable strategies (``exchange=``):
     "gather"    (default) RCCL all-gather of the deltas only (A_i, B_i were shared at
                 init), bucketed on a side stream; per module ONE fused K4 launch with
                 K = 2 r Wn that recomputes sum_i (B'_i A'_i - B_i A_i) in the reference's
                 rank order and merges it into W_res in the epilogue (dW never hits HBM).
     "allreduce" (north-star contract) per module K4 with K = 2r writes this rank's dW_i into
                 a bucketed float32 buffer; RCCL all-reduce of each bucket on a side stream,
                 overlapped with the next bucket's K4; then the K5 merge kernel W += sum dW.
                 bf16 models: the same buckets exchanged rank-ordered (all-to-all of the float32
                 terms, bf16 fold in rank order, all-gather of the bf16 shards, K5), which is the
                 reference's per-rank bf16 rounding (hp:389-392) that a summing all-reduce loses.
     "shard"     the gather exchange's delta all-gather, then rank k runs the K = 2 r Wn merge only on
                 its own 1/Wn row block of every W (``shard_rows``: blocks in units of 8 rows, so row
                 pointers stay 16-byte aligned) -- 1/Wn of gather's MFMA and panel work per rank -- and
                 one all-gather per W bucket of the merged rows restores the replicated weight: the own
                 rows packed into a send buffer and the other ranks' rows scattered into W_res by the
                 grouped copy kernel (hdp_copy_group), the all-gather and scatter on the side stream under
                 the next bucket's K4.  Every element of W is computed by one rank and copied to the
                 others: the replicas are bitwise equal in both dtypes.  World size 1: the gather path.
  3. A.grad = B.grad = None  (hp:397-398).

Opt-in, off by default (``max_grad_norm=``; the reference has neither): global gradient-norm clipping and
the non-finite-step skip, decided on the device.  In front of step 1, over the collected gradients of ALL
arenas: one sum-of-squares launch per arena (float64 accumulation of (grad x 1e16)^2), at Wn > 1 one
all-gather of those few bytes (the ranks own disjoint singular components: the global norm is the norm of
the whole adapter gradient, and every rank sums the same values in the same rank-major order), one finish
launch that writes the clip record {sumsq, norm, coef = min(1, c / (norm + 1e-6)), skip} -- and K3 / the
fused Adam-pack read that record in stream order, as they read the probe's error word: Adam runs on
(grad x 1e16) x coef; a non-finite sum leaves m and v alone and writes delta = 0, so the merge adds exactly
0 to W_res.  No host synchronisation.  ``t`` still advances on a skipped step: the bias corrections of the
following steps run one step ahead of the moments.

Opt-in, off by default (``merge_rounding="stochastic"``, ``sr_seed=``; the reference rounds to nearest): a
bf16 W takes its update as sr(float32(W) + dW) -- 16 random bits per element added below the bf16 cut of the
float32 sum (hdpissa_amd.rounding has the contract and its numpy replica) -- because at fine-tuning learning
rates dW is far below half a bf16 ulp of W and round-to-nearest returns the old weight.  bf16 modules then
skip the fused Adam-pack and K4's MERGE epilogue: after K3, K4 runs as a STORE plan (float32 dW, the plain
float32 sum over the ranks' segments -- no per-rank bf16 rounding) into two bucketed float32 buffers, and one
hdp_merge_group_sr per bucket merges on the same stream; under "allreduce" the bf16 buckets take the plain
float32 all-reduce instead of the rank-ordered fold.  The random bits depend on (sr_seed, module, t, element)
only, so every rank -- and under "shard" whichever rank merges a row -- writes the same W.  float32 modules
take exactly the launches they always took.

Opt-in, off by default (``merge_rounding="compensated"``; the reference rounds to nearest): a bf16 W carries a
bf16 compensation term ``layer.W_c`` of its shape (Kahan summation) and takes its update as s = (W_c + dW) + W,
W = bf16(s), W_c = bf16(s - W) (hdpissa_amd.rounding has the contract and its numpy replica): 4 B per element,
the base GEMMs read W_res as it is, and the update is kept to about 16 mantissa bits instead of 8.  The step is
the stochastic mode's with one hdp_merge_group_comp per bucket in place of hdp_merge_group_sr: K3, STORE plans
into the float32 buckets, the merge on the same stream; under "allreduce" the plain float32 all-reduce; under
"shard" the rank merges its row blocks of W with the same rows of W_c, and the bucket's pack, all-gather and
scatter carry the W_c rows beside the W rows -- so W_res and W_c are bitwise equal on all ranks under every
exchange.  A W_c whose W_res was written since the last merge (its version counter moved) is zeroed in front
of its merge.  ``sr_seed`` is ignored.  float32 modules take exactly the launches they always took.

Opt-in, off by default (``compute_dtype=torch.bfloat16`` on the layers; the reference computes in the precision
it stores): float32 master weights with a bf16 compute copy.  When ``step()`` returns, every layer that keeps a
copy has W_lp == bf16(W_res) element for element, in stream order on the current stream, on every rank, under
every exchange, with and without ``max_grad_norm`` and after a skipped step: one grouped cast launch
(hdp_shadow_group) per K4 / K5 launch site and bucket over that bucket's shadowed float32 modules -- gather:
after the bucket's MERGE on the main stream; allreduce: after the bucket's K5 on the stream that ran it; shard:
after the bucket's scatter on the side stream (the own rows are ordered by the hand-over event, the end by the
drain).  Buckets without such modules, and steppers without any, launch nothing.

Semantics kept from the reference: Adam without weight decay, bias correction with the
post-increment t (hp:350), A and B never updated (hp:375-376; the deltas are recomputed
against the *initial* factors every step), grads scaled x1e16 (hp:356-357), bf16 models
accumulate dW in bf16 rank by rank (zeros_like(W_res), hp:389).
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from ._lib import HDP_DW_MERGE, HDP_DW_STORE
from .layer import CustomLinearLayer, FactorArena, custom_layers


def _buckets(sizes: List[int], cap: int) -> List[Tuple[int, int]]:
    """Greedy contiguous buckets of module indices with sum(size) <= cap (>= 1 module each)."""
    out, start, acc = [], 0, 0
    for i, s in enumerate(sizes):
        if acc and acc + s > cap:
            out.append((start, i))
            start, acc = i, 0
        acc += s
    if start < len(sizes):
        out.append((start, len(sizes)))
    return out


def shard_rows(out: int, Wn: int, k: int) -> Tuple[int, int]:
    """Rows [r0, r1) of an ``out``-row W that rank ``k`` of ``Wn`` merges under exchange="shard": equal
    blocks of ``8 * ceil(out / (8 Wn))`` rows, so every block starts on a multiple of 8 rows (the W row and
    the B / dB row then stay 16-byte aligned for any in and r); trailing ranks get a short block or none."""
    block = 8 * -(-out // (8 * Wn))
    return min(out, k * block), min(out, (k + 1) * block)


def shard_item(item, Wn: int, k: int):
    """Rank k's row block of one gathered K4 item ``(out, in, r, nseg, dA, dB, delta_stride, A, B,
    factor_stride, dst)`` (dst the out x in W), or None if the rank owns no row of it.  A row block is an
    item in its own right: out' = r1 - r0, dst = W[r0:r1], dB and B advanced by r0 * r floats (inside
    every segment: the strides stay), dA and A as they are."""
    out, inn, r, nseg, dA, dB, dstr, A, B, fstr, dst = item
    r0, r1 = shard_rows(out, Wn, k)
    if r1 <= r0:
        return None
    return (r1 - r0, inn, r, nseg, dA, dB[r0 * r:], dstr, A, B[r0 * r:], fstr, dst[r0:r1])


class _ShardBucket:
    """One W bucket of the shard exchange: modules [a, b) of one dtype; per module the byte offset of
    its slot in a rank's shard (16-byte aligned, ``block * in`` elements long on every rank, whatever
    rows the rank really owns) and the shard's length ``nbytes`` (equal on all ranks).  ``comp``
    (merge_rounding="compensated"): a bf16 module has a second slot of the same length, ``cslots``, for the
    same rows of its compensation term W_c (None for the other modules)."""

    def __init__(self, layers, a: int, b: int, Wn: int, comp: bool = False):
        self.a, self.b = a, b
        self.slots, self.cslots, off = [], [], 0
        for L in layers[a:b]:
            self.slots.append(off)
            block = shard_rows(L.out_features, Wn, 0)[1]
            size = -(-block * L.in_features * L.W_res.element_size() // 16) * 16
            off += size
            self.cslots.append(off if comp and L.W_res.dtype == torch.bfloat16 else None)
            if self.cslots[-1] is not None:
                off += size
        self.nbytes = off
        self.views = None  # (W_res pointers, dsts, owners, pack, scatter), built on first use (_shard_views)


class _ArenaPlan:
    def __init__(self, arena: FactorArena, exchange: str, bucket_bytes: int, sr: bool = False,
                 sr_bytes: int = 1 << 30, comp: bool = False):
        self.arena = arena
        # merge_rounding="stochastic": the bf16 modules' float32 dW goes through HBM -- gather / shard: two
        # buffers of at most ``sr_bytes`` of dense float32 dW (the all-reduce leg's layout; a module above
        # the bound has a bucket of its own); allreduce: its own dw_bufs, summed by the plain all-reduce
        # (merge_rounding="compensated" runs the same plans and buffers: ``sr`` is set for it too, ``comp``
        # says which merge follows the STORE)
        self.sr = sr and any(L.W_res.dtype == torch.bfloat16 for L in arena.layers)
        self.comp = comp and self.sr
        self.sr_cap = max(1, sr_bytes // 4)
        self.sr_bufs: List[torch.Tensor] = []
        self.sr_turn = 0
        self.sr_progs: Dict[object, tuple] = {}   # launch programs of _sr_merge, per launch site
        Wn = arena.world_size
        if self.sr and exchange != "allreduce":
            self._build_sr()
        # (shard: bucket_bytes bounds the W buckets; the delta buckets keep gather's default bound)
        self._build_gather(min(bucket_bytes, 256 << 20) if exchange == "shard" else bucket_bytes,
                           exchange in ("gather", "shard") and Wn > 1)
        self.s_buckets: List[_ShardBucket] = []
        self.s_send: List[torch.Tensor] = []
        self.s_gath: List[torch.Tensor] = []
        if exchange == "shard" and Wn > 1:
            self._build_shard(bucket_bytes)
        self.a_buckets = []
        self.dw_bufs: List[torch.Tensor] = []
        self.a_ordered: List[bool] = []
        self.a_shard: List[int] = []
        self.o_recv: List[torch.Tensor] = []
        self.o_shard: List[torch.Tensor] = []
        self.o_gath: List[torch.Tensor] = []
        if exchange == "allreduce":
            self._build_allreduce(bucket_bytes)
        self.plans: Dict[tuple, list] = {}   # grouped K4 launches, built on first use
        # compute_dtype=: layers of this arena keep a bf16 copy of a float32 W_res; per launch site the
        # (pointers, (W_lp, W_res) pairs, layers) of its shadowed modules, cached while no buffer moved
        self.shadowed = any(L._buffers.get("W_lp") is not None for L in arena.layers)
        self.shadow_pairs: Dict[object, tuple] = {}

    def _build_sr(self) -> None:
        arena = self.arena
        sizes = [-(-L.out_features * L.in_features // 4) * 4 for L in arena.layers
                 if L.W_res.dtype == torch.bfloat16]  # (slots stay 16-byte aligned)
        n = min(sum(sizes), max(self.sr_cap, max(sizes)))
        self.sr_bufs = [torch.empty(n, dtype=torch.float32, device=arena.fac.device) for _ in range(2)]

    def _build_gather(self, bucket_bytes: int, gathered: bool) -> None:
        """Buckets over the delta arena (module-aligned ranges): (a, b, start, end) for modules [a, b);
        ``g_of[i]``: the bucket of module i; ``delta_all``: every rank's deltas, bucket by bucket."""
        arena, Wn, F = self.arena, self.arena.world_size, self.arena.F
        n = len(arena.layers)
        ends = [arena.offsets[i + 1][0] if i + 1 < n else F for i in range(n)]
        starts = [arena.offsets[i][0] for i in range(n)]
        self.g_buckets = [(a, b, starts[a], ends[b - 1]) for a, b in
                          _buckets([ends[i] - starts[i] for i in range(n)], max(1, bucket_bytes // 4 // max(Wn, 1)))]
        self.g_of = [gi for gi, (a, b, _, _) in enumerate(self.g_buckets) for _ in range(a, b)]
        self.delta_all = torch.empty(Wn * F, dtype=torch.float32, device=arena.fac.device) if gathered else None

    def _build_shard(self, bucket_bytes: int) -> None:
        """W buckets over dense W bytes, split where the dtype changes; two send and two gather buffers
        (bytes) sized for the longest shard."""
        layers, Wn, dev = self.arena.layers, self.arena.world_size, self.arena.fac.device
        run, n = 0, len(layers)
        for i in range(1, n + 1):
            if i == n or layers[i].W_res.dtype != layers[run].W_res.dtype:
                sizes = [L.W_res.numel() * L.W_res.element_size() for L in layers[run:i]]
                self.s_buckets += [_ShardBucket(layers, run + a, run + b, Wn, self.comp)
                                   for a, b in _buckets(sizes, max(1, bucket_bytes))]
                run = i
        cap = max(sb.nbytes for sb in self.s_buckets)
        self.s_send = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.s_gath = [torch.empty(Wn * cap, dtype=torch.uint8, device=dev) for _ in range(2)]

    def _build_allreduce(self, bucket_bytes: int) -> None:
        """Buckets over dense dW sizes and the two float32 dW buffers.  Rank-ordered bf16 exchange (bf16
        buckets at Wn > 1): per bucket the 1/Wn shard length (a multiple of 8 elements), the all-to-all
        receive buffers, the folded bf16 shards and the all-gathered bf16 dW (double-buffered like dw_bufs)."""
        layers, Wn, dev = self.arena.layers, self.arena.world_size, self.arena.fac.device
        sizes = [L.out_features * L.in_features for L in layers]
        self.a_buckets = _buckets(sizes, max(1, bucket_bytes // 4))
        cap = max(sum(sizes[a:b]) for a, b in self.a_buckets)
        for a, b in self.a_buckets:
            self.a_ordered.append(Wn > 1 and not self.sr and all(L.W_res.dtype == torch.bfloat16 for L in layers[a:b]))
            self.a_shard.append(-(-sum(sizes[a:b]) // (8 * Wn)) * 8)
        if any(self.a_ordered):
            sh = max(s for s, o in zip(self.a_shard, self.a_ordered) if o)
            cap = max(cap, Wn * sh)
            self.o_recv = [torch.empty(Wn * sh, dtype=torch.float32, device=dev) for _ in range(2)]
            self.o_shard = [torch.empty(sh, dtype=torch.bfloat16, device=dev) for _ in range(2)]
            self.o_gath = [torch.empty(Wn * sh, dtype=torch.bfloat16, device=dev) for _ in range(2)]
        self.dw_bufs = [torch.zeros(cap, dtype=torch.float32, device=dev) for _ in range(2)]

    @staticmethod
    def local_item(arena: FactorArena, i: int, dst: torch.Tensor):
        """The K4 item of module i on this rank's own deltas and factors (one segment), writing ``dst``."""
        L = arena.layers[i]
        oa, ob = arena.offsets[i]
        return (L.out_features, L.in_features, L.r, 1, arena.delta[oa:], arena.delta[ob:], 0,
                arena.fac[oa:], arena.fac[ob:], 0, dst)

    def gathered_item(self, i: int):
        """The K4 item of module i on every rank's deltas and factors (Wn segments: the deltas relative to
        the module's delta bucket in ``delta_all``, the factors in ``fac_all``), merging into W_res."""
        arena, Wn = self.arena, self.arena.world_size
        _, _, s, e = self.g_buckets[self.g_of[i]]
        base, fac = self.delta_all[Wn * s:], arena.fac_all.view(-1)
        L = arena.layers[i]
        oa, ob = arena.offsets[i]
        return (L.out_features, L.in_features, L.r, Wn, base[oa - s:], base[ob - s:], e - s,
                fac[oa:], fac[ob:], arena.F, L.W_res)

    def delta_plans(self, key, ops, make_items, mode, dsts) -> list:
        """Grouped K4 plans for one launch site (cached; rebuilt if a destination moved).
        Items are split where the destination dtype changes (one plan per dtype run)."""
        plans = self.plans.get(key)
        if plans is not None:
            ok, k = True, 0
            for p, _ in plans:
                ok = ok and p.valid(dsts[k:k + p.n])
                k += p.n
            if ok and k == len(dsts):
                return plans
        items = make_items()
        plans, run = [], []
        for it, d in zip(items, dsts):
            if run and run[-1][1].dtype != d.dtype:
                plans.append(self._make_plan(ops, run, mode))
                run = []
            run.append((it, d))
        if run:
            plans.append(self._make_plan(ops, run, mode))
        self.plans[key] = plans
        return plans

    @staticmethod
    def _make_plan(ops, run, mode):
        rnd = run[0][1].dtype == torch.bfloat16
        return ops.delta_plan([it for it, _ in run], mode, rnd), [d for _, d in run]


class _Pipeline:
    """The side-stream pipeline of one exchange: work for the side stream is ordered after what the main
    stream has enqueued, and the main stream waits for an event of the side stream before it reuses a buffer
    pair (two pairs, ``q`` = bucket % 2) and, at the end, for the last one.  On the CPU (``side`` None:
    synchronous collectives) the work runs in place and every wait is a no-op."""

    def __init__(self, device, side):
        self.side = side
        self.cur = torch.cuda.current_stream(device) if side is not None else None
        self.freed = [None, None]
        self.last = None

    def wait(self, ev) -> None:
        """The main stream waits for ``ev`` (None: nothing to wait for)."""
        if ev is not None:
            self.cur.wait_event(ev)

    def acquire(self, q: int) -> None:
        """Before the main stream writes buffer pair q: the side-stream work that read it is done."""
        self.wait(self.freed[q])

    def mark(self):
        """An event at the side stream's current position (None on the CPU)."""
        if self.side is None:
            return None
        ev = torch.cuda.Event()
        ev.record(self.side)
        return ev

    @contextmanager
    def on_side(self, q: Optional[int] = None):
        """The body runs on the side stream, after everything the main stream has enqueued so far; with
        ``q`` its end is marked as the release of buffer pair q."""
        if self.side is None:
            yield
            return
        ready = torch.cuda.Event()
        ready.record(self.cur)
        with torch.cuda.stream(self.side):
            self.side.wait_event(ready)
            yield
            if q is not None:
                self.freed[q] = self.last = self.mark()

    def drain(self) -> None:
        self.wait(self.last)


def _copy_pairs(pairs) -> None:
    for dst, src in pairs:
        dst.copy_(src)


def _sr_seed(merge_rounding: str, sr_seed: Optional[int]) -> Optional[int]:
    """The seed a stepper runs with: None under "nearest" and "compensated" (no random bits), else ``sr_seed`` as an unsigned 64-bit value
    (default: derived from torch's initial seed)."""
    if merge_rounding != "stochastic":
        return None
    from .rounding import default_sr_seed
    return default_sr_seed(torch.initial_seed()) if sr_seed is None else int(sr_seed) & (2 ** 64 - 1)


class HDPissaStep:
    """Stateful step object: holds the exchange plan, bucket buffers, side stream and events."""

    def __init__(self, model: nn.Module, world_size: int, rank: int = 0, comm=None, ops=None,
                 exchange: str = "gather", bucket_bytes: Optional[int] = None, beta1: float = 0.9,
                 beta2: float = 0.999, eps: float = 1e-8, max_grad_norm: Optional[float] = None,
                 merge_rounding: str = "nearest", sr_seed: Optional[int] = None):
        if exchange not in ("gather", "allreduce", "shard"):
            raise ValueError("exchange must be 'gather', 'allreduce' or 'shard'")
        if merge_rounding not in ("nearest", "stochastic", "compensated"):
            raise ValueError("merge_rounding must be 'nearest', 'stochastic' or 'compensated'")
        self.layers = [m for _, m in custom_layers(model)]
        if not self.layers:
            raise ValueError("model has no CustomLinearLayer")
        self.world_size, self.rank = world_size, rank
        self.exchange = exchange
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        # stochastic-rounding merge of the bf16 modules (off by default: nothing below is built or launched
        # then).  The rounding stream is a function of (sr_seed, module index, t, element): the same on every
        # rank, and continued by a resume with the same sr_seed
        self.merge_rounding = merge_rounding
        self.sr_seed = _sr_seed(merge_rounding, sr_seed)
        if merge_rounding == "stochastic":
            self._layer_index = {id(L): i for i, L in enumerate(self.layers)}
        sr_bytes = (1 << 30) if bucket_bytes is None else min(1 << 30, bucket_bytes)
        if bucket_bytes is None:
            # gather: ~256 MB of per-rank deltas per all-gather bucket; allreduce: 1 GB of dense
            # float32 dW per bucket (two buffers): bigger K4-store / K5 launches, fewer collectives;
            # shard: 1 GB of W per bucket (the delta all-gather keeps gather's 256 MB)
            bucket_bytes = (256 << 20) if exchange == "gather" else (1 << 30)
        arenas: Dict[int, FactorArena] = {}
        for L in self.layers:
            if L._arena is None:
                raise RuntimeError(f"{L.name} has no factor arena")
            if L._arena.world_size != world_size:
                raise ValueError("layer world_size differs from the step's world_size")
            arenas.setdefault(id(L._arena), L._arena)
        self.device = self.layers[0].W_res.device
        if ops is None:
            from .ops import default_ops
            ops = default_ops()
        self.ops = ops
        if merge_rounding == "stochastic" and not hasattr(ops, "merge_group_sr"):
            raise NotImplementedError(f"the op set {getattr(ops, 'name', ops)!r} has no merge_group_sr: "
                                      "merge_rounding='stochastic' needs the stochastic-rounding merge kernel")
        if merge_rounding == "compensated" and not hasattr(ops, "merge_group_comp"):
            raise NotImplementedError(f"the op set {getattr(ops, 'name', ops)!r} has no merge_group_comp: "
                                      "merge_rounding='compensated' needs the compensated merge kernel")
        # the merge that follows a bf16 bucket's STORE under "stochastic" / "compensated" (never called under
        # "nearest"); compensated: every bf16 layer carries W_c from here on (an existing one is kept)
        self._merge_bf16 = self._merge_comp if merge_rounding == "compensated" else self._merge_sr
        if merge_rounding == "compensated":
            for L in self.layers:
                if L.W_res.dtype == torch.bfloat16:
                    L.enable_compensation()
        self.plans = [_ArenaPlan(a, exchange, bucket_bytes, merge_rounding != "nearest", sr_bytes,
                                 merge_rounding == "compensated") for a in arenas.values()]
        if comm is None:  # the arena's init communicator (module-sharded SVD) if it has one
            comm = next((p.arena.comm for p in self.plans if getattr(p.arena, "comm", None) is not None), None)
        if comm is None:
            from .comm import make_comm
            comm = make_comm(rank, world_size, self.device)
        self.comm = comm
        self.on_gpu = self.device.type == "cuda"
        self.side = torch.cuda.Stream(device=self.device) if self.on_gpu else None
        # grouped persistent K4 (one launch per bucket); HDP_DELTA_GROUPED=0 -> one launch per module
        # (K = 2 r Wn > 32, gathered segments: the grouped plan runs the packed bf16x3 kernel --
        # tools/delta_bench.py, 56 LLaMA-7B modules: Wn 2 / 4 / 8 = 2.8 / 3.8 / 6.3 ms vs
        # 3.7 / 5.3 / 8.5 ms for per-module f32 launches)
        self.grouped = hasattr(ops, "delta_plan") and os.environ.get("HDP_DELTA_GROUPED", "1") != "0"
        self._fuse_adam = os.environ.get("HDP_FUSED_ADAM", "1") != "0"
        # the bucket's K5 and the shard exchange's pack / scatter as one launch where the op set has them
        self._merge_group = getattr(ops, "merge_group", None) or (lambda pairs: [ops.merge(W, dW) for W, dW in pairs])
        self._copy = getattr(ops, "copy_group", None) or _copy_pairs
        # the bf16 copies of a bucket's float32 modules as one launch (compute_dtype=; never called without one)
        self._shadow_group = getattr(ops, "shadow_group", None) or _copy_pairs
        # global gradient-norm clipping + non-finite-step skip (off by default: nothing below is built or
        # launched then).  c > 0; math.inf = measure and guard only
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.clip_state: Optional[torch.Tensor] = None   # the device record (hdp_clip_state, 32 bytes)
        if self.max_grad_norm is not None:
            if not self.max_grad_norm > 0.0:  # (NaN fails too)
                raise ValueError("max_grad_norm must be > 0 (math.inf: measure the norm and guard only)")
            if not (hasattr(ops, "grad_sumsq") and hasattr(ops, "clip_finish")):
                raise NotImplementedError(f"the op set {getattr(ops, 'name', ops)!r} has no grad_sumsq / clip_finish: "
                                          "max_grad_norm needs the fused device-side norm")
            make = getattr(ops, "clip_state", None)
            self.clip_state = make(self.device) if make is not None else \
                torch.zeros(32, dtype=torch.uint8, device=self.device)
            # per-arena sums, padded to 16 bytes (the all-gather's unit; the pad stays 0.0, which the
            # finish's in-order sum passes over), and at Wn > 1 every rank's copy of them, rank-major
            n = -(-len(self.plans) // 2) * 2
            self._sums = torch.zeros(n, dtype=torch.float64, device=self.device)
            self._sums_all = torch.zeros(world_size * n, dtype=torch.float64, device=self.device) \
                if world_size > 1 else self._sums

    def clip_info(self) -> dict:
        """The clip record of the last step, read back (this synchronises): {"norm", "coef", "skipped",
        "skipped_total"} (and "sumsq")."""
        if self.clip_state is None:
            raise RuntimeError("clip_info: the stepper was built without max_grad_norm")
        from ._lib import clip_record
        return clip_record(self.clip_state.cpu().numpy().tobytes())

    def _clip_record(self) -> torch.Tensor:
        """Gradient norm of every arena (every rank's) -> the clip record, all on the current stream."""
        ops = self.ops
        for plan in self.plans:
            self._collect_grads(plan.arena)
        for i, plan in enumerate(self.plans):
            ops.grad_sumsq(plan.arena.grad, self._sums[i:i + 1])
        if self.world_size > 1:
            self.comm.allgather_any(self._sums.view(torch.uint8), self._sums_all.view(torch.uint8))
        ops.clip_finish(self._sums_all, self.max_grad_norm, self.clip_state)
        return self.clip_state

    def invalidate_factors(self) -> None:
        """The factors A / B were rewritten in place in a way the arena's version counter does not see
        (``.data`` writes, raw-pointer copies): every cached K4 plan re-packs its constant operand halves
        and factor maxima on its next fused Adam run.  Writes through the tensors themselves (``copy_``,
        ``load_state_dict``, ``load_hdpissa_state``) are detected without this call."""
        for plan in self.plans:
            plan.arena.probe_queue.flush()  # pending probe groups read the old operands
            for plans in plan.plans.values():
                for p, _ in plans:
                    inv = getattr(p, "invalidate", None)
                    if inv is not None:
                        inv()
        for L in self.layers:  # the probe's cached B^T and the native one-call slot captured the old B
            L._Bt = None
            L._fslot = None

    # -----------------------------------------------------------------------------------
    def _collect_grads(self, arena: FactorArena) -> None:
        """Make sure the arena's grad buffer holds every layer's A.grad / B.grad."""
        for L in arena.layers:
            prm = L._parameters  # (not nn.Module.__getattr__: 2 lookups per layer per step)
            for p, view in ((prm["A"], L._gA), (prm["B"], L._gB)):
                g = p.grad
                if g is None:
                    view.zero_()  # no backward reached this layer: zero gradient
                elif g is not view and g.data_ptr() != view.data_ptr():
                    view.copy_(g)

    def step(self, lr: float, t: int) -> None:
        """One optimizer step (hp:352-398); ``t`` is the counter after hp:350's increment."""
        with torch.no_grad():
            for plan in self.plans:
                plan.arena.probe_queue.flush()  # grads of deferred probe launches first
                plan.arena.cast_cache = None
            chk = getattr(self.ops, "probe_errors", None)
            if chk is not None and chk():
                # a probe launch that has completed reported a failed hand-off: its gradients are
                # wrong, so no update is applied (host-mapped word: no synchronisation here).  Launches
                # still running when this check passes are covered on the device: K3 reads the same
                # word in stream order and, while it is set, leaves m / v as they were and writes
                # delta = 0, so the merge adds exactly 0 to W_res (the next flush / step raises)
                from ._lib import HdpError
                raise HdpError("probe kernels reported a failed hand-off (hdp_probe_errors); the "
                               "accumulated gradients are not trustworthy -- step refused")
            clip = self._clip_record() if self.max_grad_norm is not None else None
            for plan in self.plans:
                self._step_arena(plan, lr, t, clip)
        for L in self.layers:  # hp:397-398
            prm = L._parameters
            prm["A"].grad = None
            prm["B"].grad = None

    def _step_arena(self, plan: _ArenaPlan, lr: float, t: int, clip: Optional[torch.Tensor] = None) -> None:
        arena, ops, Wn = plan.arena, self.ops, self.world_size
        kw = {}
        if clip is not None:
            kw["clip"] = clip  # (the gradients of every arena were collected for the norm)
        else:
            self._collect_grads(arena)
        self._t = t
        plan.sr_turn = 0
        # (stochastic rounding and the compensated merge work from the float32 dW: no MERGE epilogue, so no
        # fused Adam-pack either)
        fused = None if plan.sr else self._fused_plans(plan, lr, t)
        if fused is not None:
            # K3 folded into K4's operand preparation -- per plan one Adam pass that also
            # writes the delta halves of the H2 panels, then the merge (no standalone Adam / pack)
            for p, _ in fused:
                p.run_adam(arena.grad, arena.m, arena.v, arena.delta, t, lr, self.beta1, self.beta2, self.eps,
                           zero_grad=True, **kw)
            self._shadow(plan, "g1", arena.layers)  # (fused plans merge bf16 W only: nothing to cast)
            return
        ops.adam(arena.grad, arena.m, arena.v, arena.delta, t, lr, self.beta1, self.beta2, self.eps, zero_grad=True,
                 **kw)
        if self.exchange == "gather" or (self.exchange == "shard" and Wn == 1):
            self._gather(plan)
        elif self.exchange == "shard":
            self._shard(plan)
        else:
            self._allreduce(plan)
        if plan.comp:  # W_c is consistent with the W_res this step wrote (whatever counted the writes)
            for L in arena.layers:
                if L._buffers.get("W_c") is not None:
                    L._comp_version = L._buffers["W_res"]._version

    def _fused_plans(self, plan: _ArenaPlan, lr: float, t: int):
        """The Wn = 1 gather plans when every one of them folds Adam in (single-segment H2 merges:
        bf16 W at r >= 32), else None (HDP_FUSED_ADAM=0 turns the fold off)."""
        if not (self.exchange in ("gather", "shard") and self.world_size == 1 and self.grouped) or not self._fuse_adam:
            return None
        from .ops import adam_delta_bound
        if adam_delta_bound(t, lr, self.beta1, self.beta2) is None:
            return None
        plans = self._k4_w1(plan, run=False)
        if all(getattr(p, "fused_adam", None) is not None and p.fused_adam() for p, _ in plans):
            return plans
        return None

    @staticmethod
    def _items_w1(arena: FactorArena):
        return [_ArenaPlan.local_item(arena, i, L.W_res) for i, L in enumerate(arena.layers)]

    def _k4(self, plan: _ArenaPlan, key, make_items, mode: int, dsts, run: bool = True):
        """K4 over the items ``make_items()`` returns, item j writing ``dsts[j]`` -- the one place K4 is
        launched from.  Grouped (the default): the plans cached under ``key``, one per run of one destination
        dtype, rebuilt if a destination moved; returns them (``run=False``: without launching).
        HDP_DELTA_GROUPED=0: one launch per module.  bf16 destinations round per rank (hp:389-392)."""
        if self.grouped:
            plans = plan.delta_plans(key, self.ops, make_items, mode, dsts)
            if run:
                for p, _ in plans:
                    p.run()
            return plans
        for it, d in zip(make_items(), dsts):
            self.ops.delta_gemm(*it, mode, d.dtype == torch.bfloat16)
        return None

    def _k4_w1(self, plan: _ArenaPlan, run: bool = True):
        """World size 1: every module's merge on this rank's own deltas."""
        arena = plan.arena
        return self._k4(plan, "g1", lambda: self._items_w1(arena), HDP_DW_MERGE, [L.W_res for L in arena.layers], run)

    # -- compute_dtype: the bf16 copies of float32 W_res ---------------------------------
    def _shadow(self, plan: _ArenaPlan, key, layers) -> None:
        """W_lp <- bf16(W_res) for the shadowed float32 modules among ``layers`` (one launch site's bucket):
        one shadow_group on the current stream, after the writes to their W_res enqueued on it; nothing
        where the bucket has no such module.  The pair list is cached under ``key`` while no buffer moved."""
        if not plan.shadowed:
            return
        ptrs = tuple((L._buffers["W_res"].data_ptr(), 0 if L._buffers.get("W_lp") is None else L._buffers["W_lp"].data_ptr())
                     for L in layers)
        cache = plan.shadow_pairs.get(key)
        if cache is None or cache[0] != ptrs:
            sh = [L for L in layers if L._buffers.get("W_lp") is not None and L._buffers["W_res"].dtype == torch.float32
                  and L._buffers["W_lp"].dtype == torch.bfloat16]
            cache = plan.shadow_pairs[key] = (ptrs, [(L._buffers["W_lp"], L._buffers["W_res"]) for L in sh], sh)
        _, pairs, sh = cache
        if not pairs:
            return
        self._shadow_group(pairs)
        for L, (_, W) in zip(sh, pairs):
            L._shadow_version = W._version

    # -- merge_rounding = "stochastic" / "compensated" -----------------------------------
    def _sr_offset(self, L) -> int:
        from .rounding import sr_offset
        return sr_offset(self._layer_index[id(L)], self._t)

    def _merge_sr(self, entries) -> None:
        """One merge_group_sr on the current stream over ``(W rows, float32 dW, element index of the first
        element in its W, layer)`` entries: the layer gives the module's Philox offset of this step."""
        self.ops.merge_group_sr([(W, dW, e0, self._sr_offset(L)) for W, dW, e0, L in entries], self.sr_seed)

    def _merge_comp(self, entries) -> None:
        """merge_rounding="compensated": one merge_group_comp on the current stream over the same entries --
        the rows of the layer's W_c that lie where the W rows lie in W_res ride along; a W_c whose W_res was
        written since it was last made consistent is zeroed first, on this stream."""
        triples = []
        for W, dW, e0, L in entries:
            C = L._compensation()
            if C is None:  # (the buffer was taken away since the constructor made it)
                C = L.enable_compensation()
            triples.append((W, C.view(-1)[e0:e0 + W.numel()].view(W.shape), dW))
        self.ops.merge_group_comp(triples)

    def _sr_slots(self, src: torch.Tensor, slots) -> list:
        """The all-reduce leg's merge of one bucket under stochastic rounding: the bf16 modules of ``slots``
        ((layer, offset into src, n)) merged by one merge_group_sr on the current stream; returns the other
        (float32) slots for the caller's K5."""
        sr = [(L.W_res, src[o:o + n], 0, L) for L, o, n in slots if L.W_res.dtype == torch.bfloat16]
        if sr:
            self._merge_bf16(sr)
        return [s for s in slots if s[0].W_res.dtype != torch.bfloat16]

    def _sr_merge(self, plan: _ArenaPlan, key, make_items, dsts, owners) -> None:
        """One launch site of the gather / shard exchanges under stochastic rounding.  ``make_items``: the K4
        items that would MERGE into ``dsts`` (whole W_res, or the rank's row blocks), ``owners`` their layers.
        Runs of float32 destinations take the MERGE plans they always took.  Runs of bf16 destinations: the
        same items as STORE plans (no per-rank bf16 rounding: dW is the float32 sum over the segments) into
        dense float32 buckets of the two sr buffers, each followed by its merge_group_sr on this stream.
        The launch program (_sr_program) is cached while no destination moved."""
        ptrs = tuple(d.data_ptr() for d in dsts)
        cache = plan.sr_progs.get(key)
        if cache is None or cache[0] != ptrs:
            cache = plan.sr_progs[key] = (ptrs, self._sr_program(key, make_items(), dsts, owners, plan.sr_cap))
        for bf16, pkey, its, ds, slots in cache[1]:
            if not bf16:
                self._k4(plan, pkey, lambda: its, HDP_DW_MERGE, ds)
                continue
            buf = plan.sr_bufs[plan.sr_turn % 2]
            plan.sr_turn += 1  # (before the key's parity is taken)
            stores = [buf[off:off + n] for off, n, _, _ in slots]
            self._k4(plan, pkey + (plan.sr_turn % 2,), lambda: [it + (s,) for it, s in zip(its, stores)], HDP_DW_STORE,
                     stores)
            self._merge_bf16([(d, s, e0, L) for d, s, (_, _, e0, L) in zip(ds, stores, slots)])

    @staticmethod
    def _sr_program(key, items, dsts, owners, cap: int) -> list:
        """The launch program of one _sr_merge site: per run of one destination dtype, in order, float32:
        ``(False, plan key, items, dsts, None)``, a MERGE; bf16, per bucket of at most ``cap`` floats:
        ``(True, plan key, items without dst, dsts, slots)`` -- a STORE into the slots ``(offset, n, elem0,
        layer)`` of an sr buffer, then the merge of every slot into its dst.  elem0: the element index of the
        dst's first element in its W -- for a row block r0 * in (a multiple of 8: blocks start on multiples of
        8 rows); with the module's offset, the bits any rank would give these rows."""
        prog, k = [], 0
        while k < len(items):
            e = k
            while e < len(items) and dsts[e].dtype == dsts[k].dtype:
                e += 1
            if dsts[k].dtype != torch.bfloat16:
                prog.append((False, (key, "f", k), items[k:e], dsts[k:e], None))
            else:
                sizes = [-(-it[0] * it[1] // 4) * 4 for it in items[k:e]]  # slots stay 16-byte aligned
                for a, b in _buckets(sizes, cap):
                    slots, off = [], 0
                    for j in range(k + a, k + b):
                        elem0 = dsts[j].storage_offset() - owners[j].W_res.storage_offset()
                        slots.append((off, items[j][0] * items[j][1], elem0, owners[j]))
                        off += sizes[j - k]
                    prog.append((True, (key, "sr", k + a), [it[:-1] for it in items[k + a:k + b]], dsts[k + a:k + b], slots))
            k = e
        return prog

    # -- exchange = "gather" -------------------------------------------------------------
    def _gather(self, plan: _ArenaPlan) -> None:
        layers = plan.arena.layers
        if self.world_size == 1:
            if plan.sr:
                self._sr_merge(plan, "g1", lambda: self._items_w1(plan.arena), [L.W_res for L in layers], layers)
            else:
                self._k4_w1(plan)
            self._shadow(plan, "g1", layers)
            return
        pipe = _Pipeline(self.device, self.side)
        events = self._gather_deltas(plan, pipe)
        for bi, (a, b, _, _) in enumerate(plan.g_buckets):
            pipe.wait(events[bi])
            items = lambda a=a, b=b: [plan.gathered_item(i) for i in range(a, b)]  # noqa: E731
            dsts = [L.W_res for L in layers[a:b]]
            if plan.sr:
                self._sr_merge(plan, ("g", bi), items, dsts, layers[a:b])
            else:
                self._k4(plan, ("g", bi), items, HDP_DW_MERGE, dsts)
            self._shadow(plan, ("g", bi), layers[a:b])

    def _gather_deltas(self, plan: _ArenaPlan, pipe: _Pipeline) -> list:
        """The bucketed all-gather of the deltas into ``delta_all`` (on the side stream on the GPU);
        returns one event per delta bucket (None on the CPU, where the collectives are synchronous)."""
        arena, Wn = plan.arena, self.world_size
        events = []
        with pipe.on_side():
            for (a, b, s, e) in plan.g_buckets:
                self.comm.allgather(arena.delta[s:e], plan.delta_all[Wn * s:Wn * e])
                events.append(pipe.mark())
        return events

    # -- exchange = "shard" --------------------------------------------------------------
    def _shard_items(self, plan: _ArenaPlan, sb: _ShardBucket, k: int) -> list:
        """Rank k's K4 items of one W bucket: its row block (``shard_item``) of every module that gives
        it rows, on the gathered deltas and factors as the gather exchange lays them out."""
        items = (shard_item(plan.gathered_item(i), self.world_size, k) for i in range(sb.a, sb.b))
        return [it for it in items if it is not None]

    def _shard_views(self, plan: _ArenaPlan, sb: _ShardBucket):
        """(dsts, owners, pack, scatter) of one W bucket, cached while no W_res moved: this rank's row blocks
        (the K4 destinations) and their layers, and per buffer pair the (dst, src) byte ranges that move them
        into the send buffer and every other rank's rows from the gather buffer into W_res."""
        layers, Wn = plan.arena.layers[sb.a:sb.b], self.world_size
        comps = [L._buffers.get("W_c") if coff is not None else None for L, coff in zip(layers, sb.cslots)]
        ptrs = tuple(L.W_res.data_ptr() for L in layers) + tuple(0 if c is None else c.data_ptr() for c in comps)
        if sb.views is not None and sb.views[0] == ptrs:
            return sb.views[1:]
        dsts, owners, pack, scat = [], [], ([], []), ([], [])
        for L, off, coff, comp in zip(layers, sb.slots, sb.cslots, comps):
            row = L.in_features * L.W_res.element_size()
            for j in range(Wn):
                r0, r1 = shard_rows(L.out_features, Wn, j)
                if r1 <= r0:
                    continue
                if j == self.rank:
                    dsts.append(L.W_res[r0:r1])
                    owners.append(L)
                # (compensated: the same rows of W_c travel in the module's second slot)
                for T, at in ((L.W_res, off),) + (((comp, coff),) if comp is not None else ()):
                    rows = T[r0:r1].reshape(-1).view(torch.uint8)
                    for q in range(2):
                        if j == self.rank:
                            pack[q].append((plan.s_send[q][at:at + (r1 - r0) * row], rows))
                        else:
                            o = j * sb.nbytes + at
                            scat[q].append((rows, plan.s_gath[q][o:o + (r1 - r0) * row]))
        sb.views = (ptrs, dsts, owners, pack, scat)
        return sb.views[1:]

    def _shard(self, plan: _ArenaPlan) -> None:
        Wn = self.world_size
        pipe = _Pipeline(self.device, self.side)
        events = self._gather_deltas(plan, pipe)
        for bi, sb in enumerate(plan.s_buckets):
            q = bi % 2
            pipe.wait(events[plan.g_of[sb.b - 1]])  # the delta buckets that cover modules [a, b) (in stream order)
            if plan.comp:  # (a stale W_c is zeroed here, whether or not this rank merges rows of it)
                for L in plan.arena.layers[sb.a:sb.b]:
                    L._compensation()
            dsts, owners, pack, scat = self._shard_views(plan, sb)
            items = lambda sb=sb: self._shard_items(plan, sb, self.rank)  # noqa: E731
            if dsts and plan.sr:
                self._sr_merge(plan, ("s", bi), items, dsts, owners)
            elif dsts:  # (no rows in the whole bucket: no plan)
                self._k4(plan, ("s", bi), items, HDP_DW_MERGE, dsts)
            pipe.acquire(q)  # the all-gather and scatter that read this buffer pair are done
            self._copy(pack[q])
            with pipe.on_side(q):
                self.comm.allgather_any(plan.s_send[q][:sb.nbytes], plan.s_gath[q][:Wn * sb.nbytes])
                self._copy(scat[q])  # (the own block is already in place)
                self._shadow(plan, ("s", bi), plan.arena.layers[sb.a:sb.b])  # (own rows: on_side's ready event)
        pipe.drain()

    # -- exchange = "allreduce" ----------------------------------------------------------
    def _allreduce(self, plan: _ArenaPlan) -> None:
        arena = plan.arena
        pipe = _Pipeline(self.device, self.side)
        for bi, (a, b) in enumerate(plan.a_buckets):
            q = bi % 2
            buf = plan.dw_bufs[q]
            pipe.acquire(q)  # the merges that read this buffer are done
            off, slots = 0, []
            for i in range(a, b):
                L = arena.layers[i]
                n = L.out_features * L.in_features
                slots.append((L, off, n))
                off += n
            dsts = [buf[o:o + n] for _, o, n in slots]
            self._k4(plan, ("a", bi), lambda: [plan.local_item(arena, a + j, d) for j, d in enumerate(dsts)],
                     HDP_DW_STORE, dsts)
            if self.on_gpu and self.world_size == 1:
                # the all-reduce of one rank is the identity: the bucket's K5 follows its K4 on the
                # same stream (a side-stream merge would only contend with the next K4 for HBM)
                if plan.sr:
                    slots = self._sr_slots(buf, slots)
                if slots:
                    self._merge_group([(L.W_res, buf[o:o + n].view_as(L.W_res)) for L, o, n in slots])
                self._shadow(plan, ("a", bi), arena.layers[a:b])
            else:
                with pipe.on_side(q):
                    self._exchange_merge(plan, bi, buf, off, slots)
                    self._shadow(plan, ("a", bi), arena.layers[a:b])
        pipe.drain()

    def _exchange_merge(self, plan: _ArenaPlan, bi: int, buf: torch.Tensor, off: int, slots) -> None:
        """One bucket's exchange + merge on the current stream.

        float32 W: RCCL all-reduce of the per-rank float32 dW_i, then K5 (W += sum_i dW_i).
        bfloat16 W (rank-ordered): the reference rounds its running dW to bf16 after EVERY rank's
        term, in rank order (hp:389-392: zeros_like(W_res) is bf16), which a summing all-reduce
        cannot reproduce.  Instead an all-to-all hands every rank all Wn float32 terms of its 1/Wn
        shard of the bucket, the fold kernel applies them in rank order with the bf16 rounding
        (hdp_fold_bf16), the folded bf16 shards are all-gathered, and K5 merges bf16(W + dW) --
        the reference's arithmetic, on 6 N (Wn - 1) / Wn bytes per rank instead of the ring
        all-reduce's 8 N (Wn - 1) / Wn."""
        ops, Wn = self.ops, self.world_size
        if plan.a_ordered and plan.a_ordered[bi]:
            sh = plan.a_shard[bi]
            k = bi % 2
            recv, shard, gath = plan.o_recv[k][:Wn * sh], plan.o_shard[k][:sh], plan.o_gath[k][:Wn * sh]
            self.comm.alltoall(buf[:Wn * sh], recv)
            ops.fold_bf16(recv.view(Wn, sh), shard)
            self.comm.allgather_any(shard, gath)
            src = gath
        else:
            self.comm.allreduce_sum(buf[:off])
            src = buf
            if plan.sr:  # bf16 W: the plain float32 sum over ranks, rounded once (no rank-ordered fold)
                slots = self._sr_slots(src, slots)
                if not slots:
                    return
        self._merge_group([(L.W_res, src[o:o + n].view_as(L.W_res)) for L, o, n in slots])


_STEPPERS: Dict[int, HDPissaStep] = {}


def hd_pissa_step(model: nn.Module, lr: float, t: int, world_size: int, rank: int = 0, beta1: float = 0.9,
                  beta2: float = 0.999, epsilon: float = 1e-8, exchange: str = "gather", comm=None,
                  ops=None, max_grad_norm: Optional[float] = None, merge_rounding: str = "nearest",
                  sr_seed: Optional[int] = None) -> HDPissaStep:
    """Functional form of the reference block hp:352-398 (one call per optimizer step).
    The step object (plan, buffers, streams) is cached per model.  ``max_grad_norm``: clip the global
    gradient norm and skip non-finite steps on the device (HDPissaStep; None, the default: the reference's
    step).  ``merge_rounding="stochastic"`` (with ``sr_seed``): bf16 weights take the update by stochastic
    rounding from the float32 sum; ``merge_rounding="compensated"``: bf16 weights carry a bf16 compensation term
    ``layer.W_c`` (``sr_seed`` is ignored; HDPissaStep; "nearest", the default: the reference's merge)."""
    st = _STEPPERS.get(id(model))
    mgn = None if max_grad_norm is None else float(max_grad_norm)
    seed = _sr_seed(merge_rounding, sr_seed)
    if st is None or st.exchange != exchange or st.max_grad_norm != mgn or st.merge_rounding != merge_rounding \
            or st.sr_seed != seed:
        st = HDPissaStep(model, world_size, rank, comm=comm, ops=ops, exchange=exchange, beta1=beta1, beta2=beta2,
                         eps=epsilon, max_grad_norm=max_grad_norm, merge_rounding=merge_rounding, sr_seed=sr_seed)
        _STEPPERS[id(model)] = st
    st.step(lr, t)
    return st
