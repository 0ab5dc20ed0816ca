"""Device work of exchange="shard" against exchange="gather" on one GPU (measurement tool).

Emulates rank 0 of a Wn = 8 run on a few decoder layers at a config's shapes, r and dtype, with locally
filled delta / factor segments laid out like the gathered arena (as bench.py's dw_emulated_wn does), and
times, alternating on the one box, HIP events around each run:
  (a) gather: the full K = 2 r Wn MERGE plan over every module;
  (b) shard:  rank 0's row-block plan, the pack of its rows into the send buffer, and the scatter of the 7
              other ranks' rows from a gather buffer into W (hdp_copy_group); no collective -- the all-gather
              itself needs a multi-GPU node and stays a parameter of DESIGN section 6's cost model.
It also times the scatter of the first W bucket alone (the modules within the step's default 1 GB of W): the
copy kernel's bytes/s, algorithmic bytes = 2 x bytes copied.
One JSON line per run, appended to profiles/shard_bench.jsonl (--out); reads nothing outside the repository.
  python tools/shard_bench.py --workload llama2-7b|mistral-7b|llama2-13b [--layers 2] [--runs 5] [--inner 10]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-pissa_amd")]
import torch  # noqa: E402

from hdpissa_amd._lib import HDP_DW_MERGE  # noqa: E402
from hdpissa_amd.ops import default_ops  # noqa: E402
from hdpissa_amd.step import _buckets, shard_item, shard_rows  # noqa: E402

# hidden, intermediate, kv_dim, dtype, r (bench.py's WORKLOADS)
CONFIGS = {
    "llama2-7b": dict(hidden=4096, inter=11008, kv=4096, dtype="float32", r=16),
    "mistral-7b": dict(hidden=4096, inter=14336, kv=1024, dtype="bfloat16", r=64),
    "llama2-13b": dict(hidden=5120, inter=13824, kv=5120, dtype="bfloat16", r=128),
}
HBM_TBPS = 8.0


def layer_shapes(c):
    h, i, kv = c["hidden"], c["inter"], c["kv"]
    return [(h, h), (h, h), (kv, h), (kv, h), (i, h), (i, h), (h, i)]  # q o k v gate up down: (out, in)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mistral-7b", choices=sorted(CONFIGS))
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--wn", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shard_bench needs a HIP device (there is no CPU path)")
    c, wn, dev = CONFIGS[args.workload], args.wn, torch.device("cuda:0")
    dt = torch.bfloat16 if c["dtype"] == "bfloat16" else torch.float32
    r, esz = c["r"], 2 if dt == torch.bfloat16 else 4
    ops = default_ops()
    shapes = layer_shapes(c) * args.layers
    offs, F = [], 0
    for out, inn in shapes:  # the arena's layout: A (r x in) then B (out x r) per module
        offs.append((F, F + r * inn))
        F += r * (inn + out)
    g = torch.Generator(device=dev).manual_seed(0)
    fac = torch.randn(wn * F, device=dev, generator=g) * 0.05
    dlt = torch.randn(wn * F, device=dev, generator=g) * 1e-5
    Ws = [torch.zeros(out, inn, device=dev, dtype=dt) for out, inn in shapes]
    full = [(out, inn, r, wn, dlt[oa:], dlt[ob:], F, fac[oa:], fac[ob:], F, W)
            for (out, inn), (oa, ob), W in zip(shapes, offs, Ws)]
    rnd = dt == torch.bfloat16
    plan_a = ops.delta_plan(full, HDP_DW_MERGE, rnd)
    plan_b = ops.delta_plan([shard_item(it, wn, 0) for it in full], HDP_DW_MERGE, rnd)
    # one shard per rank: a 16-byte aligned slot of block x in elements per module
    slots, nb = [], 0
    for out, inn in shapes:
        slots.append(nb)
        nb += -(-shard_rows(out, wn, 0)[1] * inn * esz // 16) * 16
    send = torch.empty(nb, dtype=torch.uint8, device=dev)
    gath = torch.zeros(wn * nb, dtype=torch.uint8, device=dev)
    a0, b0 = _buckets([W.numel() * esz for W in Ws], 1 << 30)[0]  # the step's first W bucket
    pack, scat, scat0 = [], [], []
    for m, ((out, inn), W, off) in enumerate(zip(shapes, Ws, slots)):
        for j in range(wn):
            r0, r1 = shard_rows(out, wn, j)
            if r1 <= r0:
                continue
            rows, n = W[r0:r1].reshape(-1).view(torch.uint8), (r1 - r0) * inn * esz
            if j == 0:
                pack.append((send[off:off + n], rows))
            else:
                scat.append((rows, gath[j * nb + off:j * nb + off + n]))
                if a0 <= m < b0:
                    scat0.append(scat[-1])
    scat_bytes = sum(d.numel() for d, _ in scat0)

    def run_a():
        plan_a.run()

    def run_b():
        plan_b.run()
        ops.copy_group(pack)
        ops.copy_group(scat)

    def run_scatter():
        ops.copy_group(scat0)

    for fn in (run_a, run_b, run_scatter):  # warm every shape the timed windows use
        fn()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(args.runs):  # alternating
        ta.append(timed(run_a, args.inner))
        tb.append(timed(run_b, args.inner))
        tc.append(timed(run_scatter, args.inner))
    med = statistics.median
    spread = lambda t: round(max(t) - min(t), 3)  # noqa: E731
    copy_tbps = 2 * scat_bytes / med(tc) / 1e9
    res = dict(workload=args.workload, layers=args.layers, wn=wn, dtype=c["dtype"], r=r, k4_math=plan_a.math(),
               k4_math_shard=plan_b.math(), w_bytes=sum(W.numel() for W in Ws) * esz,
               gather_ms=round(med(ta), 3), gather_spread_ms=spread(ta), gather_runs=[round(x, 3) for x in ta],
               shard_ms=round(med(tb), 3), shard_spread_ms=spread(tb), shard_runs=[round(x, 3) for x in tb],
               scatter_ms=round(med(tc), 3), scatter_spread_ms=spread(tc), scatter_bytes=scat_bytes,
               scatter_ranges=len(scat0), copy_TBps=round(copy_tbps, 3), copy_frac_hbm=round(copy_tbps / HBM_TBPS, 3),
               ratio=round(med(tb) / med(ta), 3),
               note="(a) gather = full K = 2 r Wn MERGE plan; (b) shard = rank 0's row-block plan + pack + scatter of "
                    "7 foreign blocks; medians of alternating runs, collectives excluded from both")
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
