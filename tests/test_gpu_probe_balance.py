"""K2 sweep with planned (cost-weighted) workgroup ranges.

A reduced decoder stack in ONE group call: 24 layers of hidden 1024, intermediate 1536, kv 512, r = 16,
float32, X shared by pointer within a projection group as autograd saves it (q/k/v one X, gate/up one X) --
168 modules.  Phases A and C then have 24 x 8 stripes x 25 steps = 4,800 steps for at most 256 workgroups:
ranges of ~19 steps, well above the minimum of 8, over sides of 3 (q/k/v), 2 (gate/up) and 1 (o_proj,
down_proj) r-blocks -- so phase A's weighted boundaries fall mid-stripe in heavy and light sides alike, and
in phases B and C the 25-step stripes are split into pieces summed by the finish pass (ranges, first / piece
index and the finish's job list all come from the planned boundary table).  T = 400, and T = 397 with a
ragged last step.

* parity of every module's A.grad / B.grad with the float64 oracle (O.probe_grads) at 1e-5 relative, the bar
  of every K2 test, members mixing accumulate and overwrite -- with the weighted ranges and with
  HDP_PROBE_BALANCE=0 (the equal split; the knob is read per launch);
* the same call twice gives bitwise equal gradients; and the weighted ranges give the bits of the equal split
  (only phase A is weighted: a PROJ step's sums do not depend on which workgroup runs it);
* the hand-off error word stays clear;
* r = 32 (r-block 2), hidden 1024, T = 131, one layer: parity at the other r-block that forms shared-X sets.
"""
import numpy as np
import pytest
import torch

from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
LAYERS, H, I, KV = 24, 1024, 1536, 512
SCALE = 3e-16


def _mods(h, i, kv):
    return [("q_proj", "attn", h, h), ("k_proj", "attn", kv, h), ("v_proj", "attn", kv, h), ("o_proj", "o", h, h),
            ("gate_proj", "mlp", i, h), ("up_proj", "mlp", i, h), ("down_proj", "down", h, i)]


def _np(t):
    return t.detach().double().cpu().numpy()


def _stack(T, r, layers, seed):
    """Inputs of `layers` decoder layers and the oracle's expectation of every gradient (computed once)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    mods = []
    for layer in range(layers):
        xs = {}
        for j, (name, grp, out, inn) in enumerate(_mods(H, I, KV)):
            if grp not in xs:
                xs[grp] = torch.empty(T, inn, device=DEV).normal_(generator=g)
            X = xs[grp]
            G = torch.empty(T, out, device=DEV).normal_(0, 1e-3, generator=g)
            A = torch.randn(r, inn, device=DEV, generator=g) * 0.05
            B = torch.randn(out, r, device=DEV, generator=g) * 0.05
            acc = (j + layer) % 2 == 0  # members mix accumulate / overwrite
            gA0 = torch.randn(r, inn, device=DEV, generator=g) * 1e-16
            gB0 = torch.randn(out, r, device=DEV, generator=g) * 1e-16
            eA, eB = O.probe_grads(_np(X), _np(G), _np(A), _np(B), 1.0)
            mods.append(dict(name=f"{layer}.{name}", X=X, G=G, A=A, Bt=B.t().contiguous(), gA0=gA0, gB0=gB0, acc=acc,
                             refA=(_np(gA0) if acc else 0.0) + 3.0 * eA,  # the oracle's scale is 1e-16 alpha
                             refB=(_np(gB0) if acc else 0.0) + 3.0 * eB))
    return mods


def _run(ops, mods):
    """One group call on fresh copies of the initial gradients; returns [(gA, gB)]."""
    from hdpissa_amd._lib import lib
    assert lib().hdp_probe_errors(1) == 0
    items = [(m["X"], m["G"], m["A"], m["Bt"], m["gA0"].clone(), m["gB0"].clone(), SCALE, m["acc"]) for m in mods]
    ops.probe_grads_group(items)
    torch.cuda.synchronize()
    assert lib().hdp_probe_errors(1) == 0, "hand-off error word set"
    return [(it[4], it[5]) for it in items]


def _check(mods, grads, what):
    worst = (0.0, None)
    for m, (gA, gB) in zip(mods, grads):
        errA, errB = O.rel_err(_np(gA), m["refA"]), O.rel_err(_np(gB), m["refB"])
        worst = max(worst, (errA, m["name"] + ".A"), (errB, m["name"] + ".B"))
    print(f"{what}: worst relative error {worst[0]:.3e} at {worst[1]}")
    assert worst[0] < TOL, (what, worst)


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


@pytest.fixture(scope="module", params=[400, 397])
def stack(request):
    return request.param, _stack(request.param, 16, LAYERS, 100 + request.param)


@pytest.mark.parametrize("balance", ["1", "0"])
def test_probe_balance_parity(ops, stack, balance, monkeypatch):
    T, mods = stack
    monkeypatch.setenv("HDP_PROBE_BALANCE", balance)
    _check(mods, _run(ops, mods), f"T={T} balance={balance}")


def test_probe_balance_deterministic(ops, stack, monkeypatch):
    T, mods = stack
    monkeypatch.delenv("HDP_PROBE_BALANCE", raising=False)
    a, b = _run(ops, mods), _run(ops, mods)
    for m, (a1, b1), (a2, b2) in zip(mods, a, b):
        assert torch.equal(a1, a2) and torch.equal(b1, b2), (T, m["name"])
    monkeypatch.setenv("HDP_PROBE_BALANCE", "0")
    for m, (a1, b1), (a2, b2) in zip(mods, a, _run(ops, mods)):
        assert torch.equal(a1, a2) and torch.equal(b1, b2), (T, m["name"], "equal split")


def test_probe_balance_r32(ops, monkeypatch):
    monkeypatch.delenv("HDP_PROBE_BALANCE", raising=False)
    mods = _stack(131, 32, 1, 7)
    _check(mods, _run(ops, mods), "r=32 T=131")
