"""exchange="shard" without a communicator: the eight row-block K4 plans of ranks 0-7 (hdpissa_amd.step.shard_item,
what HDPissaStep builds) against ONE full-module plan of the same build, on gathered operands (r = 16, nseg = 8).

Under the exact maths (X3, F32) the operand splits are per element and the K order of an output element
does not depend on the item or tile that holds it: the row blocks reproduce the full plan bit for bit.  Under the
default math (H2 above K = 32, whose per-k scales come from column maxima over the ITEM's rows) they need not,
and each side is held to the oracle's bars instead: float32 merged W 1e-5 and update 1e-4 against
O.delta_w_exact; bf16 update 2e-2 with < 2 % of elements differing from O.merge(O.delta_w(...)).

Measured (MI355X), worst over the shapes, default math -- see DESIGN section 3.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R, NSEG, WN = 16, 8, 8
SHAPES = {
    "200x320-f32": (200, 320, "float32"),        # a short block (rank 6: 8 rows) and a rank with no rows
    "384x250-bf16": (384, 250, "bfloat16"),      # rows not 16-byte aligned: the element-wise epilogue
    "11008x256-bf16": (1376 * 8, 256, "bfloat16"),   # the real gate/up block: 1376 = 5 * 256 + 96 rows per rank
    "11008x256-f32": (1376 * 8, 256, "float32"),
    "128x192-bf16": (128, 192, "bfloat16"),      # blocks of 16 rows, far below one tile
}


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host operands, their segment-strided device copies and the oracle's results (computed once)."""
    out, inn, dt = SHAPES[name]
    g = np.random.default_rng(out * 3 + inn)
    f = lambda s, *shape: (g.standard_normal(shape) * s).astype(np.float32)  # noqa: E731
    A, B = [f(0.3, R, inn) for _ in range(NSEG)], [f(0.3, out, R) for _ in range(NSEG)]
    dA, dB = [f(3e-2, R, inn) for _ in range(NSEG)], [f(3e-2, out, R) for _ in range(NSEG)]
    W = f(0.05, out, inn)
    if dt == "bfloat16":
        W = O.round_bf16(W)
    fstr = R * inn + out * R + 16  # A_i then B_i per segment (arena-like), padded
    dstr = fstr + 32
    fac, dl = np.zeros(fstr * NSEG + 64, np.float32), np.zeros(dstr * NSEG + 64, np.float32)
    for i in range(NSEG):
        fac[i * fstr:i * fstr + R * inn] = A[i].reshape(-1)
        fac[i * fstr + R * inn:i * fstr + R * inn + out * R] = B[i].reshape(-1)
        dl[i * dstr:i * dstr + R * inn] = dA[i].reshape(-1)
        dl[i * dstr + R * inn:i * dstr + R * inn + out * R] = dB[i].reshape(-1)
    tf, td = torch.from_numpy(fac).to(DEV), torch.from_numpy(dl).to(DEV)
    if dt == "float32":
        ref = O.delta_w_exact(dA, dB, A, B)
    else:
        ref = O.merge(W, O.delta_w(dA, dB, A, B, dt), dt)
    return W, ref, (out, inn, R, NSEG, td, td[R * inn:], dstr, tf, tf[R * inn:], fstr)


def _merge_both(ops, name):
    """(W_a merged by one full plan, W_b merged by the eight row-block plans), as host float arrays."""
    from hdpissa_amd._lib import HDP_DW_MERGE
    from hdpissa_amd.step import shard_item, shard_rows
    out, inn, dt = SHAPES[name]
    W, _, args = _case(name)
    tdt = torch.bfloat16 if dt == "bfloat16" else torch.float32
    rnd = dt == "bfloat16"
    Wa = torch.from_numpy(W).to(DEV).to(tdt)
    Wb = Wa.clone()
    full = ops.delta_plan([args + (Wa,)], HDP_DW_MERGE, rnd)
    full.run()
    blocks = 0
    for k in range(WN):
        it = shard_item(args + (Wb,), WN, k)
        r0, r1 = shard_rows(out, WN, k)
        assert (it is None) == (r1 <= r0)
        if it is None:
            continue
        assert it[0] == r1 - r0 and it[-1].data_ptr() == Wb[r0:].data_ptr()
        p = ops.delta_plan([it], HDP_DW_MERGE, rnd)
        p.run()
        p.close()
        blocks += 1
    torch.cuda.synchronize()
    full.close()
    assert blocks == (7 if out == 200 else 8)
    return Wa, Wb


@pytest.mark.parametrize("math", ["x3", "f32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_row_blocks_equal_full_plan_bitwise(ops, name, math):
    from hdpissa_amd._lib import HDP_MATH_F32, HDP_MATH_X3, lib
    prev = lib().hdp_delta_set_math(HDP_MATH_X3 if math == "x3" else HDP_MATH_F32)
    try:  # (plans keep the math of their creation)
        Wa, Wb = _merge_both(ops, name)
    finally:
        lib().hdp_delta_set_math(prev)
    assert not torch.equal(Wa, torch.from_numpy(_case(name)[0]).to(Wa))  # the merge did run
    assert torch.equal(Wa, Wb), float((Wa != Wb).float().mean())


@pytest.mark.parametrize("name", list(SHAPES))
def test_row_blocks_hold_oracle_bars_default_math(ops, name):
    from hdpissa_amd._lib import HDP_MATH_AUTO, lib
    prev = lib().hdp_delta_set_math(HDP_MATH_AUTO)
    try:
        Wa, Wb = _merge_both(ops, name)
    finally:
        lib().hdp_delta_set_math(prev)
    W, ref, _ = _case(name)
    for side, Wt in (("full", Wa), ("blocks", Wb)):
        got = Wt.float().cpu().numpy()
        if SHAPES[name][2] == "float32":
            ew = O.rel_err(got, W.astype(np.float64) + ref)
            eu = O.rel_err(got.astype(np.float64) - W, ref)
            print(f"{name} {side}: W {ew:.3e} update {eu:.3e}")
            assert ew < 1e-5 and eu < 1e-4, (side, ew, eu)
        else:
            eu = O.rel_err(got - W, ref - W)
            diff = float(np.mean(got != ref))
            print(f"{name} {side}: update {eu:.3e} differing {diff:.4f}")
            assert eu < 2e-2 and diff < 0.02, (side, eu, diff)
    print(f"{name}: blocks != full on {float((Wa != Wb).float().mean()):.4f} of elements")
