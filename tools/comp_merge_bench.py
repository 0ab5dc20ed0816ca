"""Cost of the compensated merge (merge_rounding="compensated") on one GPU (measurement tool).

One JSON line, appended to profiles/comp_merge_bench.jsonl (--out); HIP events around ``--inner`` repetitions,
``--runs`` alternating runs, medians and spreads reported:

  hdp_merge_group_comp on the first dW bucket of a workload's decoder layers (the step's buckets: at most 2^28
  float32 dW elements) beside the stochastic-rounding merge (hdp_merge_group_sr) and K5's bf16-W / float32-dW
  merge (hdp_merge_group) on the same bucket in the same process: time, GB/s and the fraction of the 8 TB/s HBM
  peak at 12, 8 and 8 B per element.  Random W ~ 0.05 N(0, 1), |dW| ~ 0.1 bf16 ulp of W, the compensation term
  starting at 0 (it fills up during the warm-up calls).

  python tools/comp_merge_bench.py --workload mistral-7b|llama2-13b [--layers 8] [--runs 5] [--inner 10]
Reads nothing outside the repository.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# hidden, intermediate, kv_dim (bench.py's WORKLOADS: the two that keep W_res in bfloat16)
CONFIGS = {
    "mistral-7b": dict(hidden=4096, inter=14336, kv=1024),
    "llama2-13b": dict(hidden=5120, inter=13824, kv=5120),
}
HBM_TBPS = 8.0
BUCKET_ELEMS = (1 << 30) // 4
KERNELS = (("comp", 12.0), ("sr", 8.0), ("k5", 8.0))  # name, algorithmic bytes per element


def layer_shapes(c):
    h, i, kv = c["hidden"], c["inter"], c["kv"]
    return [(h, h), (h, h), (kv, h), (kv, h), (i, h), (i, h), (h, i)]  # (out, in): q, o, k, v, gate, up, down


def med(t):
    return round(statistics.median(t), 4)


def timed(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def run(args, torch, ops):
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
    comp, sr, k5, off = [], [], [], 0
    for j, (o, i) in enumerate(shapes):
        w = torch.empty(o, i, device=dev, dtype=torch.float32).normal_(0.0, 0.05, generator=g)
        d = dW[off:off + o * i].view(o, i)
        d.normal_(0.0, 1.0, generator=g).mul_(w.abs() * (0.1 * 2.0 ** -8))
        W = w.bfloat16()
        comp.append((W, torch.zeros_like(W), d))
        sr.append((W, dW[off:off + o * i], 0, (j << 32) | 1))
        k5.append((W, d))
        off += o * i
    del w
    fns = {"comp": lambda: ops.merge_group_comp(comp), "sr": lambda: ops.merge_group_sr(sr, 12345),
           "k5": lambda: ops.merge_group(k5)}
    for name, _ in KERNELS:
        fns[name]()
        fns[name]()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in KERNELS}
    for _ in range(args.runs):
        for name, _ in KERNELS:
            times[name].append(timed(torch, fns[name], args.inner))
    res = dict(mode="kernel", workload=args.workload, modules=len(shapes), elements=acc)
    for name, per in KERNELS:
        t = times[name]
        tbps = per * acc / med(t) / 1e9
        res.update({f"{name}_bytes_per_element": per, f"{name}_ms": med(t), f"{name}_spread_ms": round(max(t) - min(t), 4),
                    f"{name}_runs": [round(x, 4) for x in t], f"{name}_GBps": round(1e3 * tbps, 1),
                    f"{name}_frac_hbm": round(tbps / HBM_TBPS, 3)})
    res["comp_over_sr"] = round(res["comp_ms"] / res["sr_ms"], 4)
    res["comp_frac_over_sr_frac"] = round(res["comp_frac_hbm"] / res["sr_frac_hbm"], 4)
    res["note"] = ("hdp_merge_group_comp (12 B per element) against hdp_merge_group_sr and hdp_merge_group (bf16 W, "
                   "float32 dW; 8 B per element each) on one dW bucket; medians of alternating runs in one process")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mistral-7b", choices=sorted(CONFIGS))
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "comp_merge_bench.jsonl"))
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-pissa_amd")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("comp_merge_bench needs a HIP device (there is no CPU path)")
    from hdpissa_amd.ops import default_ops
    res = run(args, torch, default_ops())
    line = json.dumps(res)
    print(line, flush=True)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
