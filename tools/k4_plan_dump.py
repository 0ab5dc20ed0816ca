"""What K4 plan creation decides (comparison tool, not part of the library).

  python tools/k4_plan_dump.py > plans.txt

Creates the plans of the K4 test matrix that fit in a few hundred MB -- the ragged shapes of the GPU tests as
one plan, and one module of every BASELINE shape as a plan of its own, at nseg 1 and 8, float32 and bf16 W,
MERGE and STORE with and without per-rank rounding, under every math, x3 staging and HDP_K4_DEFER value
the GPU tests use -- and prints hdp_delta_plan_math, hdp_delta_plan_tiles (total and grid) and
hdp_delta_plan_fused_adam for each.  One line per (shapes, nseg, dtype, mode, round): its 26 plans grouped
by what was decided, each group followed by the settings math/stage/defer values that gave it ("-": HDP_K4_DEFER
unset).  Nothing is launched but plan creation.  Two builds that make the same decisions print the same
lines (profiles/k4_plan_dump_*.txt).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hd-pissa_amd")]

import torch  # noqa: E402

RAGGED = [(200, 320), (384, 250), (75, 130), (128, 192)]
PLANS = [("ragged-r%d" % r, [(o, i, r) for o, i in RAGGED]) for r in (1, 4, 20, 100, 128)]
PLANS += [("llama2-7b-%dx%d" % s, [s + (16,)]) for s in ((4096, 4096), (11008, 4096), (4096, 11008))]
PLANS += [("mistral-7b-%dx%d" % s, [s + (64,)]) for s in ((4096, 4096), (1024, 4096), (14336, 4096), (4096, 14336))]
PLANS += [("llama2-13b-%dx%d" % s, [s + (128,)]) for s in ((5120, 5120), (13824, 5120), (5120, 13824))]
MODES = [("f32", "merge", False), ("bf16", "merge", False), ("bf16", "merge", True), ("f32", "store", False),
         ("f32", "store", True)]
DEFERS = [None, "0", "1", "2", "4"]
SETTINGS = ([("auto", "wide", d) for d in DEFERS] + [("f32", "wide", None)] +
            [("x3", st, d) for st in ("regs", "glds", "wide") for d in DEFERS] + [("h2", "wide", d) for d in DEFERS])


def main():
    from hdpissa_amd._lib import HDP_DW_MERGE, HDP_DW_STORE, lib
    from hdpissa_amd.ops import default_ops
    ops = default_ops()
    dev = torch.device("cuda:0")
    nmax = max(sum(o * i for o, i, _ in mods) for _, mods in PLANS)
    fmax = 8 * max(sum(r * (o + i) for o, i, r in mods) for _, mods in PLANS)
    W = {"f32": torch.empty(nmax, device=dev), "bf16": torch.empty(nmax, device=dev, dtype=torch.bfloat16)}
    fac, dlt = torch.empty(fmax, device=dev), torch.empty(fmax, device=dev)
    for name, mods in PLANS:
        F = sum(r * (o + i) for o, i, r in mods)
        for nseg in (1, 8):
            for dtype, mode, rnd in MODES:
                items, off, woff = [], 0, 0
                for o, i, r in mods:
                    items.append((o, i, r, nseg, dlt[off:], dlt[off + r * i:], F, fac[off:], fac[off + r * i:], F,
                                  W[dtype][woff:woff + o * i]))
                    off += r * (o + i)
                    woff += o * i
                got = {}  # decision -> {math/stage: [defer values]}
                for math, stage, defer in SETTINGS:
                    lib().hdp_delta_set_math({"auto": 0, "f32": 1, "x3": 2, "h2": 3}[math])
                    lib().hdp_delta_set_x3_stage({"regs": 0, "glds": 1, "wide": 2}[stage])
                    if defer is None:
                        os.environ.pop("HDP_K4_DEFER", None)
                    else:
                        os.environ["HDP_K4_DEFER"] = defer
                    plan = ops.delta_plan(items, HDP_DW_MERGE if mode == "merge" else HDP_DW_STORE, rnd)
                    tiles, grid = plan.tiles()
                    what = "%s tiles=%d grid=%d fused_adam=%d" % (plan.math(), tiles, grid, plan.fused_adam())
                    got.setdefault(what, {}).setdefault(math + "/" + stage, []).append(defer or "-")
                    plan.close()
                print("%s nseg=%d %s %s round=%d | %s" % (name, nseg, dtype, mode, rnd, " ; ".join(
                    what + " : " + " ".join(k + "/" + ".".join(d) for k, d in by.items()) for what, by in got.items())),
                      flush=True)


if __name__ == "__main__":
    main()
