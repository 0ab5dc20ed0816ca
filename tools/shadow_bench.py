"""Cost of the bf16 compute copy of float32 master weights (compute_dtype=torch.bfloat16) on one GPU
(measurement tool).

One JSON line per measurement, appended to profiles/shadow_bench.jsonl (--out); HIP events around ``--inner``
repetitions, ``--runs`` alternating runs, medians and spreads reported:

  kernel  hdp_shadow_group on one W bucket of the workload's decoder layers (the step's buckets: at most 2^28
          float32 W elements = 1 GB; 4 B read + 2 B written per element) beside hdp_copy_group moving the same
          bytes (3 B per element read and written) in the same process; each as a fraction of the 8 TB/s HBM peak.
  model   the whole model's copies (--layers decoder layers): one shadow_group call over every module (one launch
          per 170) against one ``copy_`` per module -- device time (events) and host time (the calls, unsynchronised).
  step    HDPissaStep.step on ``--layers`` decoder layers (random factors: the traffic does not depend on their
          values), with the copy against without on two copies of the model.
  ab      the default step (compute_dtype=None) of this tree against another build of the library (``--parent
          DIR``: a built checkout of the parent commit), each in ``--runs`` fresh processes, alternating.  The new
          median should lie inside the parent's own spread.

  python tools/shadow_bench.py --mode kernel|model|step|ab [--workload llama2-7b] [--layers N] [--parent DIR]
Reads nothing outside the repository (and --parent).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hidden, intermediate, kv_dim, r (bench.py's WORKLOADS: the one that keeps W_res in float32)
CONFIGS = {
    "llama2-7b": dict(hidden=4096, inter=11008, kv=4096, r=16),
}
HBM_TBPS = 8.0
NAMES = ["q_proj", "o_proj", "k_proj", "v_proj", "gate_proj", "up_proj", "down_proj"]
BUCKET_ELEMS = (1 << 30) // 4


def layer_shapes(c):
    h, i, kv = c["hidden"], c["inter"], c["kv"]
    return [(h, h), (h, h), (kv, h), (kv, h), (i, h), (i, h), (h, i)]  # (out, in) in NAMES' order


def med(t):
    return round(statistics.median(t), 4)


def spread(t):
    return round(max(t) - min(t), 4)


def timed(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def weights(torch, shapes, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    Ws = [torch.empty(o, i, device=dev, dtype=torch.float32).normal_(0.0, 0.05, generator=g) for o, i in shapes]
    return Ws, [torch.empty_like(W, dtype=torch.bfloat16) for W in Ws]


def run_kernel(args, torch, ops):
    c = CONFIGS[args.workload]
    dev = torch.device("cuda:0")
    shapes, acc = [], 0
    for o, i in layer_shapes(c) * args.layers:  # the step's greedy bucket: modules while they fit
        if acc and acc + o * i > BUCKET_ELEMS:
            break
        shapes.append((o, i))
        acc += o * i
    Ws, lps = weights(torch, shapes, dev)
    pairs = list(zip(lps, Ws))
    scratch = torch.empty(3 * acc, dtype=torch.uint8, device=dev)
    copies, off = [], 0
    for W in Ws:  # the same bytes through the copy kernel: 3 B per element in, 3 B out
        nb = 3 * W.numel()
        copies.append((scratch[off:off + nb], W.view(-1).view(torch.uint8)[:nb]))
        off += nb

    def sh():
        ops.shadow_group(pairs)

    def cp():
        ops.copy_group(copies)

    for fn in (sh, cp):
        fn()
    torch.cuda.synchronize()
    for lp, W in pairs:
        assert torch.equal(lp, W.to(torch.bfloat16))
    ts, tc = [], []
    for _ in range(args.runs):
        ts.append(timed(torch, sh, args.inner))
        tc.append(timed(torch, cp, args.inner))
    s_tbps, c_tbps = 6.0 * acc / med(ts) / 1e9, 6.0 * acc / med(tc) / 1e9
    return dict(mode="kernel", workload=args.workload, modules=len(shapes), elements=acc, bytes=6 * acc,
                inner=args.inner, shadow_ms=med(ts), shadow_spread_ms=spread(ts), shadow_runs=[round(x, 4) for x in ts],
                shadow_TBps=round(s_tbps, 3), shadow_frac_hbm=round(s_tbps / HBM_TBPS, 3), copy_ms=med(tc),
                copy_spread_ms=spread(tc), copy_runs=[round(x, 4) for x in tc], copy_TBps=round(c_tbps, 3),
                copy_frac_hbm=round(c_tbps / HBM_TBPS, 3), ratio_of_copy_fraction=round(s_tbps / c_tbps, 4),
                target_met=bool(s_tbps >= 0.9 * c_tbps),
                note="hdp_shadow_group (4 B read + 2 B written per element) against hdp_copy_group on the same byte "
                     "count, one W bucket; medians of alternating runs in one process; target: shadow's fraction of "
                     "HBM peak >= 0.9 of the copy's")


def run_model(args, torch, ops):
    c = CONFIGS[args.workload]
    dev = torch.device("cuda:0")
    shapes = layer_shapes(c) * args.layers
    Ws, lps = weights(torch, shapes, dev)
    pairs = list(zip(lps, Ws))
    n = sum(W.numel() for W in Ws)

    def grouped():
        ops.shadow_group(pairs)

    def per_module():
        for lp, W in pairs:
            lp.copy_(W)

    def host(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        return 1e3 * dt

    for fn in (grouped, per_module):
        fn()
    torch.cuda.synchronize()
    tg, tp, hg, hp = [], [], [], []
    for _ in range(args.runs):
        tg.append(timed(torch, grouped, args.inner))
        tp.append(timed(torch, per_module, args.inner))
        hg.append(host(grouped))
        hp.append(host(per_module))
    return dict(mode="model", workload=args.workload, layers=args.layers, modules=len(pairs), elements=n,
                inner=args.inner, grouped_ms=med(tg), grouped_spread_ms=spread(tg), grouped_TBps=round(6.0 * n / med(tg) / 1e9, 3),
                copy_ms=med(tp), copy_spread_ms=spread(tp), copy_TBps=round(6.0 * n / med(tp) / 1e9, 3),
                grouped_host_ms=med(hg), copy_host_ms=med(hp),
                note="every module's bf16 copy: one shadow_group call (a launch per 170 modules) against one torch "
                     "copy_ per module; device time by events, host time of the unsynchronised calls")


class _RandomFactors:
    """The op set with the SVD-slice init replaced by random factors (measurement only)."""

    def __init__(self, ops, torch):
        self._ops, self._torch = ops, torch

    def __getattr__(self, k):
        return getattr(self._ops, k)

    def svd_topk_batch(self, Ws, r, nranks):
        torch, out = self._torch, []
        for W in Ws:
            o, i = W.shape
            g = torch.Generator(device=W.device).manual_seed(o * 7 + i)
            out.append((torch.randn(r * nranks, i, device=W.device, generator=g) * 0.05,
                        torch.randn(nranks, o, r, device=W.device, generator=g) * 0.05,
                        torch.ones(r * nranks, dtype=torch.float64, device=W.device)))
        return out


def build(args, torch, ops, modes):
    """Per entry of ``modes`` (a compute dtype or None) a float32 model of --layers decoder layers with its
    stepper, and the function that refills the gradients and steps it."""
    import torch.nn as nn
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    c = CONFIGS[args.workload]
    dev = torch.device("cuda:0")
    fns, info = [], {}
    for mode in modes:
        model = nn.Module()
        model.layers = nn.ModuleList()
        g = torch.Generator(device=dev).manual_seed(1)
        for _ in range(args.layers):
            blk = nn.Module()
            for name, (out, inn) in zip(NAMES, layer_shapes(c)):
                lin = nn.Linear(inn, out, bias=False, device="meta")
                w = torch.empty(out, inn, device=dev, dtype=torch.float32).normal_(0.0, 0.02, generator=g)
                lin.weight = nn.Parameter(w, requires_grad=False)
                setattr(blk, name, lin)
            model.layers.append(blk)
        kw = {} if mode is None else {"compute_dtype": mode}  # (None: no new argument, the parent's call)
        layers = replace_with_custom_layer(model, NAMES, 0, 1, c["r"], float(c["r"]), ops=_RandomFactors(ops, torch), **kw)
        for L in layers:
            L._ops = ops
        arena = layers[0]._arena
        arena.probe_queue.ops = ops
        st = HDPissaStep(model, 1, 0, ops=ops)
        src = torch.randn(arena.F, device=dev, generator=g) * 1e-14
        t = [0]

        def fn(st=st, arena=arena, layers=layers, src=src, t=t):
            arena.grad.copy_(src)  # what the probe launches leave behind (the step clears it)
            for L in layers:       # the probe's gradients are views of the arena
                L.A.grad, L.B.grad = L._gA, L._gB
            t[0] += 1
            st.step(2e-5, t[0])
        fns.append(fn)
        info = dict(F=arena.F, w_elements=sum(L.W_res.numel() for L in layers))
    return fns, info


def run_step(args, torch, ops):
    (f_off, f_on), info = build(args, torch, ops, [None, torch.bfloat16])
    for fn in (f_off, f_on, f_off, f_on):
        fn()
    torch.cuda.synchronize()
    t0, t1 = [], []
    for _ in range(args.runs):
        t0.append(timed(torch, f_off, args.inner))
        t1.append(timed(torch, f_on, args.inner))
    added = med(t1) - med(t0)
    return dict(mode="step", workload=args.workload, layers=args.layers, **info, inner=args.inner,
                without_ms=med(t0), without_spread_ms=spread(t0), without_runs=[round(x, 4) for x in t0],
                with_ms=med(t1), with_spread_ms=spread(t1), with_runs=[round(x, 4) for x in t1],
                added_ms=round(added, 4), ratio=round(med(t1) / med(t0), 4),
                added_TBps=round(6.0 * info["w_elements"] / added / 1e9, 3) if added > 0 else None,
                note="HDPissaStep.step (gather, Wn = 1) incl. a 4 B/entry refill of the gradient arena; float32 r16 "
                     "with the bf16 copy against without on two copies of the model, medians of alternating runs; "
                     "as counted: +6 B on K4's 8 B per W element")


def run_none(args, torch, ops):
    """One process of the A/B: the default step alone (this tree's library, or --tree's).  No new argument is
    passed: the parent's code does not know them."""
    (f_off,), info = build(args, torch, ops, [None])
    f_off()
    f_off()
    torch.cuda.synchronize()
    t = [timed(torch, f_off, args.inner) for _ in range(3)]
    return dict(mode="none", step_ms=med(t), **info)


def run_ab(args):
    if not args.parent or not os.path.isdir(os.path.join(args.parent, "hd-pissa_amd", "hdpissa_amd")):
        raise SystemExit("--mode ab needs --parent DIR: a built checkout of the parent commit")
    new, old = [], []
    for _ in range(args.runs):  # alternating, a fresh process each
        for tree, acc in ((ROOT, new), (os.path.abspath(args.parent), old)):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", "none", "--tree", tree, "--workload", args.workload,
                   "--layers", str(args.layers), "--inner", str(args.inner), "--out", os.devnull]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"{tree}: exit {p.returncode}\n{p.stderr[-2000:]}")
            acc.append(json.loads(p.stdout.strip().splitlines()[-1])["step_ms"])
    inside = min(old) <= med(new) <= max(old)
    return dict(mode="ab", workload=args.workload, layers=args.layers, inner=args.inner, new_step_ms=med(new),
                new_runs=new, new_spread_ms=spread(new), parent_step_ms=med(old), parent_runs=old,
                parent_spread_ms=spread(old), new_median_inside_parent_spread=inside, ratio=round(med(new) / med(old), 4),
                note="the default step (compute_dtype=None) of this tree against the parent commit's build, one fresh "
                     "process per run, alternating")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="kernel", choices=["kernel", "model", "step", "ab", "none"])
    ap.add_argument("--workload", default="llama2-7b", choices=sorted(CONFIGS))
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=None, help="default: 50 (kernel), 10 otherwise")
    ap.add_argument("--parent", default=None, help="ab: a built checkout of the parent commit")
    ap.add_argument("--tree", default=ROOT, help="none: the tree whose hdpissa_amd is measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shadow_bench.jsonl"))
    args = ap.parse_args()
    if args.inner is None:
        args.inner = 50 if args.mode == "kernel" else 10
    if args.mode == "ab":
        res = run_ab(args)
    else:
        sys.path[:0] = [args.tree, os.path.join(args.tree, "hd-pissa_amd")]
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("shadow_bench needs a HIP device (there is no CPU path)")
        from hdpissa_amd.ops import default_ops
        res = {"kernel": run_kernel, "model": run_model, "step": run_step, "none": run_none}[args.mode](
            args, torch, default_ops())
    line = json.dumps(res)
    print(line, flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
