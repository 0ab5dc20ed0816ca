"""merge_rounding="compensated" on the GPU: hdp_merge_group_comp against the numpy replica bit for bit in W and in C
(sizes around the 8192-element chunk, each of W, C and dW off 16 bytes in turn, 1 / 127 / 128 vector items per
call beside empty and element-wise ones, canaries either side of every W and every C, the values of the host
contract table tiled), its refusals, the step's plumbing at Wn = 1 ((W_res, W_c) = replica(the pre-step pair, the
float32 dW of a separately built K4 STORE plan), with and without max_grad_norm; allreduce == gather; a mixed
model under compute_dtype) and the reason for the mode: 128 constant-gradient steps at lr 5e-5.

Measured (MI355X) -- see DESIGN section 3.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from comp_cases import comp_cases
from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = 256 * 4 * 8    # elements of one chunk of the vector kernel: 256 lanes x kU = 4 vectors x 8 bf16
CAP = 127              # vector items of one launch
CANARY = 0x5A5B        # bf16 bits either side of every W and every C
PAD = 64               # canary elements either side (a multiple of 8: the shift is the item's own)


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd import _lib
    from hdpissa_amd.ops import HipOps
    assert _lib.MERGE_COMP_CHUNK == CHUNK and _lib.MERGE_COMP_MAX == CAP
    return HipOps()


@pytest.fixture(scope="module")
def table():
    """The host contract table (997 random triples + the special ones = 1024), computed once."""
    return comp_cases(7, 1024 - 27)


# ------------------------------------------------------------------------------------------ the kernel
def _inputs(table, n, turn):
    """The table tiled to n elements, rotated by ``turn`` so that its rows meet different lanes and residues."""
    return tuple(np.resize(np.roll(x, turn), n) for x in table)


def _padded(bits, shift):
    buf = np.full(PAD + shift + bits.size + PAD, CANARY, dtype=np.uint16)
    buf[PAD + shift:PAD + shift + bits.size] = bits
    t = torch.from_numpy(buf.view(np.int16)).to(DEV)
    assert t.data_ptr() % 16 == 0
    return buf, t, t[PAD + shift:PAD + shift + bits.size].view(torch.bfloat16)


def _check_call(ops, table, items):
    """items: (n, W shift, C shift in elements, dW shift in floats).  One merge_group_comp call over all of them;
    every W and C against the replica (bits where finite, NaN positions) and their canaries."""
    from hdpissa_amd.rounding import comp_merge_bits
    host, dev = [], []
    for k, (n, ws, cs, ds) in enumerate(items):
        wb, cb, dw = _inputs(table, n, 5 * k + n)
        _, tw, W = _padded(wb, ws)
        _, tc, C = _padded(cb, cs)
        td = torch.zeros(ds + n + 8, dtype=torch.float32, device=DEV)
        td[ds:ds + n] = torch.from_numpy(dw).to(DEV)
        assert td.data_ptr() % 16 == 0
        host.append((wb, cb, dw))
        dev.append((tw, tc, W, C, td[ds:ds + n]))
    ops.merge_group_comp([(W, C, d) for _, _, W, C, d in dev])
    torch.cuda.synchronize()
    for k, ((n, ws, cs, ds), (wb, cb, dw), (tw, tc, _, _, _)) in enumerate(zip(items, host, dev)):
        want_w, want_c = comp_merge_bits(wb, cb, dw)
        for name, t, sh, want in (("W", tw, ws, want_w), ("C", tc, cs, want_c)):
            got = t.cpu().numpy().view(np.uint16)
            assert np.all(got[:PAD + sh] == CANARY), (k, n, f"canary before {name}")
            assert np.all(got[PAD + sh + n:] == CANARY), (k, n, f"canary after {name}")
            out = got[PAD + sh:PAD + sh + n]
            nan = (want & 0x7FFF) > 0x7F80
            assert np.array_equal(nan, (out & 0x7FFF) > 0x7F80), (k, n, name, "NaN positions")
            bad = np.nonzero((out != want) & ~nan)[0]
            assert bad.size == 0, (k, n, name, ws, cs, ds, bad[:8], out[bad[:8]], want[bad[:8]])
        if n >= 64:
            assert np.any(want_w != wb) and np.any(want_c != cb), (k, n, "nothing to merge")


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 43])
def test_kernel_sizes(ops, table, n):
    _check_call(ops, table, [(n, 0, 0, 0)])


@pytest.mark.parametrize("ws,cs,ds", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (4, 0, 0), (0, 4, 0), (0, 0, 2), (3, 5, 2), (8, 16, 4)],
                         ids=lambda x: str(x))
def test_kernel_misaligned(ops, table, ws, cs, ds):
    """Each of W, C and dW off 16 bytes in turn (the element-wise form); (8, 16, 4) is aligned again (the vector
    form at shifted bases)."""
    _check_call(ops, table, [(CHUNK + 1, ws, cs, ds), (77, ws, cs, ds), (3 * CHUNK + 43, ws, cs, ds)])


@pytest.mark.parametrize("count", [1, CAP, CAP + 1])
def test_kernel_item_counts(ops, table, count):
    """1, 127 and 128 vector items in one call (127 per launch), empty and element-wise items beside them."""
    items = []
    for i in range(count):  # all on the vector path (with and without tails): 128 of them take two launches
        n = [8 * (i % 7) + i % 3 + 1, 16, 2048 + i, CHUNK + 8 * i][i % 4] if count > 1 else 3 * CHUNK + 43
        items.append((n, 0, 0, 0))
    items[1:1] = [(0, 0, 0, 0)]
    items += [(CHUNK + 3, 1, 0, 0), (333, 0, 3, 0), (0, 0, 0, 0), (41, 0, 0, 1)]
    _check_call(ops, table, items)


def test_refusals_raise_before_any_launch(ops):
    from hdpissa_amd._lib import kernel_timing
    bf = lambda n: torch.zeros(n, device=DEV, dtype=torch.bfloat16)  # noqa: E731
    f32 = lambda n: torch.zeros(n, device=DEV)  # noqa: E731
    good = (bf(64), bf(64), f32(64))
    kernel_timing(enable=True, reset=True)
    try:
        with pytest.raises(TypeError):
            ops.merge_group_comp([good, (f32(8), bf(8), f32(8))])          # a float32 W
        with pytest.raises(TypeError):
            ops.merge_group_comp([good, (bf(8), f32(8), f32(8))])          # a non-bf16 C
        with pytest.raises(TypeError):
            ops.merge_group_comp([good, (bf(8), bf(8).half(), f32(8))])
        with pytest.raises(ValueError):
            ops.merge_group_comp([good, (bf(8), bf(8), f32(9))])           # mismatched numel
        with pytest.raises(ValueError):
            ops.merge_group_comp([good, (bf(8), bf(9), f32(8))])
        with pytest.raises(ValueError):
            ops.merge_group_comp([good, (bf(16)[::2], bf(8), f32(8))])     # not contiguous
        torch.cuda.synchronize()
        assert "merge_comp" not in kernel_timing(enable=False, reset=True)
    finally:
        kernel_timing(enable=False)
    ops.merge_group_comp([])  # nothing to do


# ------------------------------------------------------------------------------------------ the step, Wn = 1
SHAPES = [("q_proj", 75, 130), ("o_proj", 128, 192)]
LR = 2e-3


def _model(shapes, dts, seed=5):
    model = nn.Module()
    g = torch.Generator().manual_seed(seed)
    for (name, out, inn), dt in zip(shapes, dts):
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_((torch.randn(out, inn, generator=g) * 0.05).bfloat16().float())
        setattr(model, name, lin.to(DEV).to(dt).requires_grad_(False))
    return model


def _grads(L, j, step):
    g = torch.Generator().manual_seed(1000 * step + 10 * j)
    return torch.randn(L.A.shape, generator=g) * 1e-14, torch.randn(L.B.shape, generator=g) * 1e-14


def _set_grads(layers, step):
    for j, L in enumerate(layers):
        gA, gB = _grads(L, j, step)
        L.A.grad, L.B.grad = gA.to(DEV), gB.to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _build(r, dts=(torch.bfloat16, torch.bfloat16), layer_kw=None, **kw):
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    model = _model(SHAPES, dts)
    layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, r, float(r), **(layer_kw or {}))
    return model, layers, HDPissaStep(model, 1, 0, **kw)


@pytest.mark.parametrize("clip", [None, math.inf], ids=["noclip", "clip-inf"])
@pytest.mark.parametrize("r", [16, 32])
def test_step_equals_replica_on_store_dw(ops, r, clip):
    from helpers import rel_err
    from hdpissa_amd._lib import HDP_DW_STORE, kernel_timing
    from hdpissa_amd.rounding import comp_merge_reference
    kw = {} if clip is None else {"max_grad_norm": clip}
    if r == 32:  # the premise: "nearest" takes the fused Adam-pack at these shapes
        _, _, near = _build(r, **kw)
        assert near._fused_plans(near.plans[0], LR, 1) is not None
    _, layers, st = _build(r, merge_rounding="compensated", **kw)
    assert st.sr_seed is None and st.plans[0].sr and st.plans[0].comp and len(st.plans[0].sr_bufs) == 2
    assert all(L.W_c is not None and L.W_c.dtype == torch.bfloat16 and not L.W_c.any() for L in layers)
    arena = layers[0]._arena
    for step in (1, 2):
        _set_grads(layers, step)
        before = [(L.W_res.clone(), L.W_c.clone()) for L in layers]
        kernel_timing(enable=True, reset=True)
        try:
            st.step(LR, step)
            torch.cuda.synchronize()
            timing = kernel_timing(enable=False, reset=True)
        finally:
            kernel_timing(enable=False)
        # K3 on its own (not the fused Adam-pack), K4 as a STORE plan, one merge_comp launch for the bucket
        assert timing["adam"]["launches"] == 1 and timing["merge_comp"]["launches"] == 1, timing
        assert "merge" not in timing and "merge_sr" not in timing
        assert timing["merge_comp"]["bytes_per_launch"] == 12.0 * sum(L.W_res.numel() for L in layers)
        # the same items as a STORE plan of this test's own, on the deltas K3 left in the arena
        items, bufs = [], []
        for it in st._items_w1(arena):
            bufs.append(torch.zeros(it[0] * it[1], dtype=torch.float32, device=DEV))
            items.append(it[:-1] + (bufs[-1],))
        ops.delta_plan(items, HDP_DW_STORE, False).run()
        torch.cuda.synchronize()
        for j, L in enumerate(layers):
            dA, dB = (x.cpu().numpy() for x in arena.views(arena.delta, j))
            A, B = L.A.detach().cpu().numpy(), L.B.detach().cpu().numpy()
            exact = O.delta_w_exact([dA], [dB], [A], [B])
            err = rel_err(bufs[j].cpu().numpy().reshape(exact.shape), exact)
            print(f"r={r} clip={clip} step {step} module {j}: STORE dW rel err {err:.3e}")
            assert err < 1e-5, (step, j, err)
            want_w, want_c = comp_merge_reference(*before[j], bufs[j].view_as(L.W_res))
            assert np.array_equal(_bits(L.W_res), _bits(want_w)), (step, j, float(np.mean(_bits(L.W_res) != _bits(want_w))))
            assert np.array_equal(_bits(L.W_c), _bits(want_c)), (step, j, float(np.mean(_bits(L.W_c) != _bits(want_c))))
            assert not torch.equal(L.W_res, before[j][0]) and L.W_c.any()
    if clip is not None:
        assert st.clip_info()["coef"] == 1.0


def test_allreduce_equals_gather_at_wn1():
    """r 16 with the K4 math pinned to x3 (what HDP_K4_MATH=x3 pins), so that the STORE dW cannot depend on the
    plan's grouping: the two exchanges give the same bits in W_res and in W_c."""
    from hdpissa_amd._lib import HDP_MATH_X3, lib
    prev = lib().hdp_delta_set_math(HDP_MATH_X3)
    try:
        res = {}
        for exchange in ("gather", "allreduce"):
            _, layers, st = _build(16, merge_rounding="compensated", exchange=exchange)
            for step in (1, 2):
                _set_grads(layers, step)
                st.step(LR, step)
            torch.cuda.synchronize()
            res[exchange] = [(L.W_res.clone(), L.W_c.clone()) for L in layers]
        for (gw, gc), (aw, ac) in zip(res["gather"], res["allreduce"]):
            assert np.array_equal(_bits(gw), _bits(aw)) and np.array_equal(_bits(gc), _bits(ac))
            assert gc.any()
    finally:
        lib().hdp_delta_set_math(prev)


def test_mixed_model_under_compute_dtype():
    """A float32 module with a bf16 compute copy beside a bf16 module: after a step the copy is bf16(W_res), the
    float32 module carries no compensation term, and the bf16 module took merge_comp."""
    from hdpissa_amd._lib import kernel_timing
    _, layers, st = _build(16, dts=(torch.float32, torch.bfloat16), layer_kw=dict(compute_dtype=torch.bfloat16),
                           merge_rounding="compensated")
    f32, b16 = layers
    assert f32.W_lp is not None and f32.W_c is None and b16.W_lp is None and b16.W_c is not None
    _set_grads(layers, 1)
    before = [L.W_res.clone() for L in layers]
    kernel_timing(enable=True, reset=True)
    try:
        st.step(LR, 1)
        torch.cuda.synchronize()
        timing = kernel_timing(enable=False, reset=True)
    finally:
        kernel_timing(enable=False)
    assert timing["merge_comp"]["launches"] == 1, timing
    assert timing["merge_comp"]["bytes_per_launch"] == 12.0 * b16.W_res.numel()
    assert not torch.equal(f32.W_res, before[0]) and not torch.equal(b16.W_res, before[1]) and b16.W_c.any()
    assert torch.equal(f32.W_lp, f32.W_res.to(torch.bfloat16))
    assert f32._shadow_version == f32.W_res._version


# ------------------------------------------------------------------------------------------ the reason for it
def test_compensation_keeps_the_update():
    """One bf16 layer 128 x 192, r 16, lr 5e-5, the same gradients before each of 128 steps (the inputs of
    tests/test_comp_host.py's drift test).  err(x) = ||x - (W0 + sum dW)|| / ||sum dW||, sum dW from a float32-W
    copy of the layer on the same factors.  Required: err(nearest) >= 0.8, err(W_res, compensated) <= 0.5
    err(stochastic), err(float32(W_res) + float32(W_c)) <= 0.5 err(W_res, compensated).  The CPU op sets gave
    0.8996, 0.2289, 0.0269 and 0.0029; measured on the MI355X: 0.8966, 0.2243,
    0.0270 (0.12 of stochastic) and 0.0029 (0.11 of W_res alone)."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    lr, steps, shapes = 5e-5, 128, [("q_proj", 128, 192)]

    def build(dt, **kw):
        model = _model(shapes, [dt])
        (L,) = replace_with_custom_layer(model, ["q_proj"], 0, 1, 16, 16.0)
        return L, (lambda: HDPissaStep(model, 1, 0, **kw))

    def run(L, st):
        g = torch.Generator().manual_seed(77)
        gA, gB = (torch.randn(s, generator=g) * 1e-14 for s in (L.A.shape, L.B.shape))
        for t in range(1, steps + 1):
            L.A.grad, L.B.grad = gA.to(DEV), gB.to(DEV)
            st.step(lr, t)
        torch.cuda.synchronize()
        return L.W_res.float().cpu().numpy().astype(np.float64)

    Lf, mk = build(torch.float32)
    W0 = Lf.W_res.float().cpu().numpy().astype(np.float64)
    Wf = run(Lf, mk())
    total = np.linalg.norm(Wf - W0)
    err = {}
    for mode, kw in (("nearest", {}), ("stochastic", dict(merge_rounding="stochastic", sr_seed=20240607)),
                     ("compensated", dict(merge_rounding="compensated"))):
        L, mk = build(torch.bfloat16, **kw)
        with torch.no_grad():
            L._arena.fac_all.copy_(Lf._arena.fac_all)  # the very same factors
        assert np.array_equal(L.W_res.float().cpu().numpy().astype(np.float64), W0)
        err[mode] = float(np.linalg.norm(run(L, mk()) - Wf) / total)
        if mode == "compensated":
            both = L.W_res.float().cpu().numpy().astype(np.float64) + L.W_c.float().cpu().numpy().astype(np.float64)
            err["compensated W+C"] = float(np.linalg.norm(both - Wf) / total)
    print("128 steps at lr 5e-5: " + ", ".join(f"{k} {v:.4f}" for k, v in err.items()))
    assert err["nearest"] >= 0.8, err
    assert err["compensated"] <= 0.5 * err["stochastic"], err
    assert err["compensated W+C"] <= 0.5 * err["compensated"], err
