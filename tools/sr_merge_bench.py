"""Cost of the stochastic-rounding merge (merge_rounding="stochastic") on one GPU (measurement tool).

Three measurements, one JSON line each, appended to profiles/sr_merge_bench.jsonl (--out); HIP events around
``--inner`` repetitions, ``--runs`` alternating runs, medians and spreads reported:

  kernel  hdp_merge_group_sr on the first dW bucket of a workload's decoder layers (the step's buckets: at most
          2^28 float32 dW elements) beside K5's bf16-W / float32-dW merge (hdp_merge_group) on the same buffers
          in the same process -- both move 8 B per element; each as a fraction of the 8 TB/s HBM peak.  Random
          W ~ 0.05 N(0, 1), |dW| ~ 0.1 bf16 ulp of W.
  step    HDPissaStep.step on ``--layers`` decoder layers of the workload (random factors: the traffic does not
          depend on their values), "stochastic" against "nearest" on two copies of the model, at --wn 1 or at an
          emulated --wn 8 (exchange="gather" with a communicator that copies this rank's deltas into every
          rank's slot: the K = 2 r Wn plans of a real run, the exchange itself a device copy).
  ab      the "nearest" step of this tree against another build of the library (``--parent DIR``: a built
          checkout of the parent commit), each in ``--runs`` fresh processes, alternating.  The new median should
          lie inside the parent's own spread.

  python tools/sr_merge_bench.py --mode kernel|step|ab --workload mistral-7b|llama2-13b [--wn 8] [--parent DIR]
Reads nothing outside the repository (and --parent).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hidden, intermediate, kv_dim, dtype, r (bench.py's WORKLOADS: the two that keep W_res in bfloat16)
CONFIGS = {
    "mistral-7b": dict(hidden=4096, inter=14336, kv=1024, dtype="bfloat16", r=64),
    "llama2-13b": dict(hidden=5120, inter=13824, kv=5120, dtype="bfloat16", r=128),
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


def run_kernel(args, torch, ops):
    c = CONFIGS[args.workload]
    dev = torch.device("cuda:0")
    shapes, acc = [], 0
    for o, i in layer_shapes(c) * args.layers:  # the step's greedy bucket: modules while they fit
        if acc and acc + o * i > BUCKET_ELEMS:
            break
        shapes.append((o, i))
        acc += o * i
    g = torch.Generator(device=dev).manual_seed(0)
    dW = torch.empty(acc, device=dev, dtype=torch.float32)
    Ws, items, pairs, off = [], [], [], 0
    for j, (o, i) in enumerate(shapes):
        w = torch.empty(o, i, device=dev, dtype=torch.float32).normal_(0.0, 0.05, generator=g)
        d = dW[off:off + o * i].view(o, i)
        d.normal_(0.0, 1.0, generator=g).mul_(w.abs() * (0.1 * 2.0 ** -8))
        W = w.bfloat16()
        Ws.append(W)
        items.append((W, dW[off:off + o * i], 0, (j << 32) | 1))
        pairs.append((W, d))
        off += o * i
    del w

    def sr():
        ops.merge_group_sr(items, 12345)

    def k5():
        ops.merge_group(pairs)

    for fn in (sr, k5):
        fn()
    torch.cuda.synchronize()
    ts, tk = [], []
    for _ in range(args.runs):
        ts.append(timed(torch, sr, args.inner))
        tk.append(timed(torch, k5, args.inner))
    s_tbps, k_tbps = 8.0 * acc / med(ts) / 1e9, 8.0 * acc / med(tk) / 1e9
    return dict(mode="kernel", workload=args.workload, modules=len(shapes), elements=acc, bytes=8 * acc,
                sr_ms=med(ts), sr_spread_ms=spread(ts), sr_runs=[round(x, 4) for x in ts], sr_TBps=round(s_tbps, 3),
                sr_frac_hbm=round(s_tbps / HBM_TBPS, 3), k5_ms=med(tk), k5_spread_ms=spread(tk),
                k5_runs=[round(x, 4) for x in tk], k5_TBps=round(k_tbps, 3), k5_frac_hbm=round(k_tbps / HBM_TBPS, 3),
                gap_ms=round(med(ts) - med(tk), 4), ratio=round(med(ts) / med(tk), 4),
                note="hdp_merge_group_sr against hdp_merge_group (bf16 W, float32 dW) on one dW bucket, 8 B per "
                     "element each; medians of alternating runs in one process")


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


class _EmulatedComm:
    """Wn ranks on one GPU for timing: every rank's contribution is a copy of this rank's (measurement only)."""
    name = "emulated"

    def __init__(self, wn):
        self.rank, self.world_size = 0, wn

    def allgather(self, send, recv):
        recv.view(self.world_size, -1).copy_(send.reshape(1, -1).expand(self.world_size, -1))

    allgather_any = allgather

    def broadcast(self, t, root):
        pass


def build(args, torch, ops, modes):
    """Per entry of ``modes`` a model of --layers decoder layers with its stepper, and the function that refills
    the gradients and steps it."""
    import torch.nn as nn
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    c = CONFIGS[args.workload]
    dev, dt, wn = torch.device("cuda:0"), getattr(torch, c["dtype"]), args.wn
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
                lin.weight = nn.Parameter(w.to(dt), requires_grad=False)
                setattr(blk, name, lin)
            model.layers.append(blk)
        layers = replace_with_custom_layer(model, NAMES, 0, wn, c["r"], float(c["r"]), ops=_RandomFactors(ops, torch))
        for L in layers:
            L._ops = ops
        arena = layers[0]._arena
        arena.probe_queue.ops = ops
        kw = dict(merge_rounding=mode, sr_seed=7) if mode == "stochastic" else {}
        if wn > 1:
            kw["comm"] = _EmulatedComm(wn)
        st = HDPissaStep(model, wn, 0, ops=ops, **kw)
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
        info["fused_adam_" + mode] = wn == 1 and st._fused_plans(st.plans[0], 2e-5, 1) is not None \
            if mode == "nearest" else False
    return fns, info


def run_step(args, torch, ops):
    (f_near, f_sr), info = build(args, torch, ops, ["nearest", "stochastic"])
    for fn in (f_near, f_sr, f_near, f_sr):
        fn()
    torch.cuda.synchronize()
    tn, ts = [], []
    for _ in range(args.runs):
        tn.append(timed(torch, f_near, args.inner))
        ts.append(timed(torch, f_sr, args.inner))
    return dict(mode="step", workload=args.workload, layers=args.layers, wn=args.wn, **info,
                nearest_ms=med(tn), nearest_spread_ms=spread(tn), nearest_runs=[round(x, 4) for x in tn],
                stochastic_ms=med(ts), stochastic_spread_ms=spread(ts), stochastic_runs=[round(x, 4) for x in ts],
                added_ms=round(med(ts) - med(tn), 4), ratio=round(med(ts) / med(tn), 4),
                note="HDPissaStep.step incl. a 4 B/entry refill of the gradient arena; stochastic against nearest on "
                     "two copies of the model, medians of alternating runs"
                     + ("" if args.wn == 1 else "; Wn emulated on one GPU (every rank's deltas = this rank's)"))


def run_none(args, torch, ops):
    """One process of the A/B: the default step alone (this tree's library, or --tree's).  No new argument is
    passed: the parent's HDPissaStep does not know them."""
    (f_near,), info = build(args, torch, ops, ["nearest"])
    f_near()
    f_near()
    torch.cuda.synchronize()
    t = [timed(torch, f_near, args.inner) for _ in range(3)]
    return dict(mode="none", nearest_ms=med(t), **info)


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
            acc.append(json.loads(p.stdout.strip().splitlines()[-1])["nearest_ms"])
    inside = min(old) <= med(new) <= max(old)
    return dict(mode="ab", workload=args.workload, layers=args.layers, new_nearest_ms=med(new), new_runs=new,
                new_spread_ms=spread(new), parent_nearest_ms=med(old), parent_runs=old, parent_spread_ms=spread(old),
                new_median_inside_parent_spread=inside, ratio=round(med(new) / med(old), 4),
                note="the default (nearest) step of this tree against the parent commit's build, one fresh process "
                     "per run, alternating")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="kernel", choices=["kernel", "step", "ab", "none"])
    ap.add_argument("--workload", default="mistral-7b", choices=sorted(CONFIGS))
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--wn", type=int, default=1, help="step: world size (> 1: emulated on one GPU)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--parent", default=None, help="ab: a built checkout of the parent commit")
    ap.add_argument("--tree", default=ROOT, help="none: the tree whose hdpissa_amd is measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_merge_bench.jsonl"))
    args = ap.parse_args()
    if args.mode == "ab":
        res = run_ab(args)
    else:
        sys.path[:0] = [args.tree, os.path.join(args.tree, "hd-pissa_amd")]
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("sr_merge_bench needs a HIP device (there is no CPU path)")
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
