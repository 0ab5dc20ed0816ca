"""Per-step cost of the K2 sweep's shared-X (FUSE) phases A and C by r-blocks per side, at the LLaMA-2-7B
float32 r = 16 shapes -- the weights of the range planner (kSwWeightA / kSwWeightC in csrc/hdp_probe.hip).

Each configuration is a HOMOGENEOUS group of 45,056 phase-A / phase-C steps (what the 7B group has), so every
workgroup's range holds one kind of step and the phase time / steps is that kind's cost:
  nb = 3: q/k/v sets only           nb = 2: gate/up sets only          nb = 4: four 4096-wide modules per X
  nb = 1: o_proj + down_proj, plus ONE q/k set of 16 rows (8 steps) so that the group runs the FUSE instances
Run with HDP_PROBE_BALANCE=0 (the equal split).  Measurement tool.
  python tools/probe_weights.py [--T 692] [--reps 10]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-pissa_amd")]
import torch  # noqa: E402

from hdpissa_amd._lib import kernel_timing  # noqa: E402
from hdpissa_amd.ops import default_ops  # noqa: E402

H, I, R, DEV = 4096, 11008, 16, "cuda:0"


def module(X, out):
    T, inn = X.shape
    G = torch.randn(T, out, device=DEV) * 1e-3
    return (X, G, torch.randn(R, inn, device=DEV) * 0.05, torch.randn(R, out, device=DEV) * 0.05,
            torch.zeros(R, inn, device=DEV), torch.zeros(out, R, device=DEV), 1e-16, True)


def group(nb, T):
    items = []
    x = lambda inn, t=T: torch.randn(t, inn, device=DEV)
    if nb == 1:
        for _ in range(64):
            items.append(module(x(H), H))  # o_proj
            items.append(module(x(I), H))  # down_proj (its S1 side is G, 4096 wide)
        xs = x(H, 16)
        items += [module(xs, H), module(xs, H)]
    else:
        outs = {2: [I, I], 3: [H, H, H], 4: [H, H, H, H]}[nb]
        for _ in range(128):
            xs = x(H)
            items += [module(xs, o) for o in outs]
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=692)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ops = default_ops()
    S = (args.T + 15) // 16
    for nb in (1, 2, 3, 4, 1, 3):  # (1 and 3 twice: the run-to-run spread of the ratio that matters)
        items = group(nb, args.T)
        steps = 128 * 8 * S  # stripes of 512 columns of the 4096-wide S1 sides
        for _ in range(2):
            ops.probe_grads_group(items)
        torch.cuda.synchronize()
        kernel_timing(enable=True, reset=True)
        for _ in range(args.reps):
            ops.probe_grads_group(items)
        torch.cuda.synchronize()
        kt = kernel_timing(enable=False)
        us = {k: v["total_ms"] * 1e3 / args.reps for k, v in kt.items()}
        print(json.dumps(dict(nb=nb, T=args.T, steps=steps, balance=os.environ.get("HDP_PROBE_BALANCE", "1"),
                              lib=os.environ.get("HDPISSA_LIB", "default"),
                              us_per_step_A=round(us["probe_sweep_a"] / steps, 4),
                              us_per_step_C=round(us["probe_sweep_c"] / steps, 4),
                              phases_us={k: round(v, 1) for k, v in us.items()})), flush=True)
        del items
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
