"""Cost of gradient-norm clipping (max_grad_norm) on one GPU (measurement tool).

Three measurements, one JSON line each, appended to profiles/clip_bench.jsonl (--out); HIP events around
``--inner`` repetitions, ``--runs`` alternating runs, medians and spreads reported:

  kernel  the flat factor arena of a workload (llama2-7b: F = 40 M float32; mistral-7b bf16 r64: F = 168 M):
          grad_sumsq + clip_finish (4 B per entry) beside K3 (hdp_adam_factors, 28 B per entry with
          zero_grad) in the same call -- K3 has the same access form and is the yardstick for the
          float64-accumulating read; each as a fraction of the 8 TB/s HBM peak.
  step    HDPissaStep.step on ``--layers`` decoder layers of the workload (random factors: the traffic does
          not depend on their values) with max_grad_norm = inf against None.  mistral-7b takes the fused
          Adam-pack path (bf16 W, r = 64, Wn = 1).
  ab      the None step of this tree against another build of the library (``--parent DIR``: a checkout of
          the parent commit, built), each in ``--runs`` fresh processes, alternating -- the protocol of
          profiles/r08_sweep_plan_ab.jsonl.  The new median should lie inside the parent's own spread.

  python tools/clip_bench.py --mode kernel|step|ab --workload llama2-7b|mistral-7b [--layers 8] [--parent DIR]
Reads nothing outside the repository (and --parent).
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hidden, intermediate, kv_dim, layers, dtype, r (bench.py's WORKLOADS)
CONFIGS = {
    "llama2-7b": dict(hidden=4096, inter=11008, kv=4096, layers=32, dtype="float32", r=16),
    "mistral-7b": dict(hidden=4096, inter=14336, kv=1024, layers=32, dtype="bfloat16", r=64),
}
HBM_TBPS = 8.0
NAMES = ["q_proj", "o_proj", "k_proj", "v_proj", "gate_proj", "up_proj", "down_proj"]


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


def run_kernel(args, torch, ops):
    c = CONFIGS[args.workload]
    dev = torch.device("cuda:0")
    F = c["layers"] * c["r"] * sum(o + i for o, i in layer_shapes(c))
    g = torch.Generator(device=dev).manual_seed(0)
    grad = torch.randn(F, device=dev, generator=g) * 1e-14
    m, v, d = (torch.zeros(F, device=dev) for _ in range(3))
    sums = torch.zeros(2, dtype=torch.float64, device=dev)
    state = ops.clip_state(dev)
    t = [0]

    def sumsq():
        ops.grad_sumsq(grad, sums[0:1])
        ops.clip_finish(sums, math.inf, state)

    def k3():  # zero_grad off: the same gradient every time (the kernel's loads and arithmetic are the same;
        t[0] += 1  # its 4 B store per entry is missing: 24 B per entry here)
        ops.adam(grad, m, v, d, t[0], 2e-5, 0.9, 0.999, 1e-8, False)

    for fn in (sumsq, k3):
        fn()
    torch.cuda.synchronize()
    ts, tk = [], []
    for _ in range(args.runs):
        ts.append(timed(torch, sumsq, args.inner))
        tk.append(timed(torch, k3, args.inner))
    s_tbps, k_tbps = 4.0 * F / med(ts) / 1e9, 24.0 * F / med(tk) / 1e9
    return dict(mode="kernel", workload=args.workload, F=F, sumsq_bytes=4 * F, sumsq_finish_ms=med(ts),
                sumsq_spread_ms=spread(ts), sumsq_runs=[round(x, 4) for x in ts], sumsq_TBps=round(s_tbps, 3),
                sumsq_frac_hbm=round(s_tbps / HBM_TBPS, 3), k3_bytes=24 * F, k3_ms=med(tk), k3_spread_ms=spread(tk),
                k3_runs=[round(x, 4) for x in tk], k3_TBps=round(k_tbps, 3), k3_frac_hbm=round(k_tbps / HBM_TBPS, 3),
                note="grad_sumsq (3 launches: vector kernel, in-order sum of the partials) + clip_finish against K3 "
                     "(zero_grad off, 24 B per entry) on the same arena; medians of alternating runs")


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


def build(args, torch, ops, clips):
    """One model of --layers decoder layers, and a stepper per entry of ``clips`` on it."""
    import torch.nn as nn
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    c = CONFIGS[args.workload]
    dev, dt = torch.device("cuda:0"), getattr(torch, c["dtype"])
    model = nn.Module()
    model.layers = nn.ModuleList()
    g = torch.Generator(device=dev).manual_seed(1)
    for _ in range(args.layers):
        blk = nn.Module()
        for name, (out, inn) in zip(NAMES, layer_shapes(c)):
            lin = nn.Linear(inn, out, bias=False, device="meta")
            w = torch.empty(out, inn, device=dev, dtype=torch.float32).normal_(0.0, 0.02, generator=g)
            lin.weight = nn.Parameter(w.to(dt), requires_grad=False)
            setattr(blk, name, lin)
        model.layers.append(blk)
    layers = replace_with_custom_layer(model, NAMES, 0, 1, c["r"], float(c["r"]), ops=_RandomFactors(ops, torch))
    for L in layers:
        L._ops = ops
    arena = layers[0]._arena
    arena.probe_queue.ops = ops
    steppers = [HDPissaStep(model, 1, 0, ops=ops, **({} if clip is None else {"max_grad_norm": clip})) for clip in clips]
    src = torch.randn(arena.F, device=dev, generator=g) * 1e-14
    t = [0]

    def step_fn(st):
        def fn():
            arena.grad.copy_(src)  # what the probe launches leave behind (the step clears it)
            for L in layers:       # the probe's gradients are views of the arena
                L.A.grad, L.B.grad = L._gA, L._gB
            t[0] += 1
            st.step(2e-5, t[0])
        return fn
    fused = [st._fused_plans(st.plans[0], 2e-5, 1) is not None for st in steppers]
    return arena, [step_fn(st) for st in steppers], fused


def run_step(args, torch, ops):
    arena, (f_none, f_inf), fused = build(args, torch, ops, [None, math.inf])
    for fn in (f_none, f_inf, f_none, f_inf):
        fn()
    torch.cuda.synchronize()
    tn, ti = [], []
    for _ in range(args.runs):
        tn.append(timed(torch, f_none, args.inner))
        ti.append(timed(torch, f_inf, args.inner))
    return dict(mode="step", workload=args.workload, layers=args.layers, F=arena.F, fused_adam=fused[0],
                none_ms=med(tn), none_spread_ms=spread(tn), none_runs=[round(x, 4) for x in tn],
                inf_ms=med(ti), inf_spread_ms=spread(ti), inf_runs=[round(x, 4) for x in ti],
                added_ms=round(med(ti) - med(tn), 4), ratio=round(med(ti) / med(tn), 4),
                note="HDPissaStep.step (Wn = 1) incl. a 4 B/entry refill of the gradient arena; max_grad_norm = inf "
                     "against None on the same model, medians of alternating runs")


def run_none(args, torch, ops):
    """One process of the A/B: the None step alone (this tree's library, or --tree's)."""
    arena, (f_none,), fused = build(args, torch, ops, [None])
    f_none()
    f_none()
    torch.cuda.synchronize()
    t = [timed(torch, f_none, args.inner) for _ in range(3)]
    return dict(mode="none", none_ms=med(t), F=arena.F, fused_adam=fused[0])


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
            acc.append(json.loads(p.stdout.strip().splitlines()[-1])["none_ms"])
    inside = min(old) <= med(new) <= max(old)
    return dict(mode="ab", workload=args.workload, layers=args.layers, new_none_ms=med(new), new_runs=new,
                new_spread_ms=spread(new), parent_none_ms=med(old), parent_runs=old, parent_spread_ms=spread(old),
                new_median_inside_parent_spread=inside, ratio=round(med(new) / med(old), 4),
                note="max_grad_norm = None step of this tree against the parent commit's build, one fresh process "
                     "per run, alternating")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="kernel", choices=["kernel", "step", "ab", "none"])
    ap.add_argument("--workload", default="llama2-7b", choices=sorted(CONFIGS))
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent", default=None, help="ab: a built checkout of the parent commit")
    ap.add_argument("--tree", default=ROOT, help="none: the tree whose hdpissa_amd is measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.jsonl"))
    args = ap.parse_args()
    if args.mode == "ab":
        res = run_ab(args)
    else:
        sys.path[:0] = [args.tree, os.path.join(args.tree, "hd-pissa_amd")]
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("clip_bench needs a HIP device (there is no CPU path)")
        from hdpissa_amd.ops import default_ops
        res = {"kernel": run_kernel, "step": run_step, "none": run_none}[args.mode](args, torch, default_ops())
    line = json.dumps(res)
    print(line, flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
