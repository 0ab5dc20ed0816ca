"""Masked probe backward (adapter dropout) at the headline module shape of bench.py's llama2-7b workload:
out = in = 4096, r = 16, T = batch 2 x 512 tokens, float32 and bf16 activations.

Times, interleaved on the same GPU with device events, medians over --reps rounds:
  (a) HipOps.probe_grads_dropout (the fused kernel + its finish kernel);
  (b) the reference's formulation in torch, float32 as the reference runs it (hp:139 under autograd):
      D = G.float().T @ X.float(); M = rand >= p; gA = s/(1-p) B^T (M D); gB = s/(1-p) (M D) A^T.
Prints one JSON line per dtype and appends it to profiles/probe_dropout_bench.jsonl:
times, the ratio (b) / (a), the fused kernel's own time from the library's kernel timing, and its achieved
share of the MFMA peak of its math (f32: 157.3 TF, bf16: 2500 TF dense).

  python tools/probe_dropout_bench.py [--T 1024 --out 4096 --in 4096 --r 16 --p 0.1 --reps 30 --inner 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-pissa_amd")]
import torch  # noqa: E402

PEAK_TF = {"float32": 157.3, "bfloat16": 2500.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--out", type=int, default=4096)
    ap.add_argument("--in", dest="inn", type=int, default=4096)
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "probe_dropout_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_dropout_bench needs a HIP device (no CPU timing)")
    from hdpissa_amd._lib import kernel_timing
    from hdpissa_amd.ops import default_ops
    ops, dev = default_ops(), "cuda:0"
    T, out, inn, r, p = args.T, args.out, args.inn, args.r, args.p
    scale = 1e-16
    torch.manual_seed(0)
    A = torch.randn(r, inn, device=dev)
    B = torch.randn(out, r, device=dev)
    Bt = B.t().contiguous()
    flops = 2.0 * T * inn * out + 4.0 * r * inn * out
    for dt in (torch.float32, torch.bfloat16):
        X = torch.randn(T, inn, device=dev).to(dt)
        G = (torch.randn(T, out, device=dev) * 1e-3).to(dt)
        gA, gB = torch.zeros(r, inn, device=dev), torch.zeros(out, r, device=dev)
        calls = [0]

        def fused():
            calls[0] += 1
            ops.probe_grads_dropout(X, G, A, B, gA, gB, scale, True, p, 1234, calls[0], Bt=Bt)

        def torch_ref():
            D = G.float().t() @ X.float()
            MD = (torch.rand(out, inn, device=dev) >= p) * D
            return (scale / (1 - p)) * (B.t() @ MD), (scale / (1 - p)) * (MD @ A.t())

        def timed(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.inner):
                fn()
            e.record()
            e.synchronize()
            return s.elapsed_time(e) / args.inner

        for _ in range(3):
            fused()
            torch_ref()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):  # interleaved: both see the same machine state
            ta.append(timed(fused))
            tb.append(timed(torch_ref))
        kernel_timing(enable=True, reset=True)
        for _ in range(args.inner):
            fused()
        torch.cuda.synchronize()
        kt = kernel_timing(enable=False)
        k_us = kt.get("probe_dropout", {}).get("avg_us")
        f_us = kt.get("probe_dropout_finish", {}).get("avg_us")
        name = str(dt).replace("torch.", "")
        ma, mb = statistics.median(ta), statistics.median(tb)
        rec = {
            "tool": "probe_dropout_bench", "dtype": name, "T": T, "out": out, "in": inn, "r": r, "p": p,
            "fused_ms_median": round(ma, 4), "fused_ms_min": round(min(ta), 4), "fused_ms_max": round(max(ta), 4),
            "torch_f32_ms_median": round(mb, 4), "torch_f32_ms_min": round(min(tb), 4),
            "torch_f32_ms_max": round(max(tb), 4), "torch_over_fused": round(mb / ma, 3),
            "kernel_us": None if k_us is None else round(k_us, 1),
            "finish_kernel_us": None if f_us is None else round(f_us, 1),
            "kernel_tflops": None if k_us is None else round(flops / k_us / 1e6, 1),
            "mfma_peak_tflops": PEAK_TF[name],
            "kernel_share_of_mfma_peak": None if k_us is None else round(flops / k_us / 1e6 / PEAK_TF[name], 4),
            "reps": args.reps, "inner": args.inner,
        }
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.jsonl), exist_ok=True)
        with open(args.jsonl, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
