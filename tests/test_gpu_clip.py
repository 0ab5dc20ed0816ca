"""Gradient-norm clipping and the non-finite-step skip on the device: grad_sumsq_kernel, clip_finish_kernel,
the clipped K3 and the clipped fused Adam-pack, and the whole step / trainer at Wn = 1.

Expected values: numpy float64 for the sum (any order of summing n non-negative float64 terms is within
n 2^-52 of any other: clip_ref.sumsq_bound), numpy float32 for the record's norm and coefficient (bit for
bit), and clip_ref.adam_factors_clip -- the oracle's Adam on (raw x 1e16) x coef, pinned to the oracle at
coef = 1 by tests/test_clip_host.py -- for m, v and delta (bit for bit).  W is held to the oracle bars of
DESIGN section 3.
"""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import clip_ref as R
from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# 2 * 256 * 4 floats = one full chunk of the kernel (256 lanes x kSumsqU = 2 vectors of 4 floats); 1,300,003 is
# 635 workgroups with a ragged last chunk plus a scalar tail.  The persistent grid is capped at 2048 workgroups
# (4,194,304 floats per round): test_sumsq_more_than_one_grid_round goes past it
SIZES = [1, 3, 4, 5, 1023, 2 * 256 * 4, 2 * 256 * 4 + 5, 1_300_003]


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


def _place(a, off):
    """``a`` on the device at a 16-byte aligned base (off = 0) or one float past it (the scalar path)."""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    v = buf[off:off + a.size]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * off
    return v


def _sumsq(ops, g, scale=1e16):
    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.grad_sumsq(g, out, scale)
    return out


def _record(ops, sums, c, state=None):
    from hdpissa_amd._lib import clip_record
    state = ops.clip_state(DEV) if state is None else state
    ops.clip_finish(sums, c, state)
    return state, clip_record(state.cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def normal_data():
    g = np.random.default_rng(0)
    return {n: (g.standard_normal(n) * 1e-14).astype(np.float32) for n in SIZES}


# ------------------------------------------------------------------------------------- grad_sumsq
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_against_float64(ops, normal_data, n, off):
    raw = normal_data[n]
    g = _place(raw, off)
    got = _sumsq(ops, g)
    again = _sumsq(ops, g)
    ref = R.sumsq(raw)
    val = float(got.item())
    print(f"n={n} off={off}: rel err {abs(val - ref) / ref:.3e} (bound {R.sumsq_bound(n):.3e})")
    assert abs(val - ref) <= ref * R.sumsq_bound(n)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))  # the same bits on every run


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_integers_exact(ops, n, off):
    ints = np.random.default_rng(n).integers(-1000, 1001, n)
    got = float(_sumsq(ops, _place(ints.astype(np.float32), off), 1.0).item())
    assert got == float(sum(int(x) * int(x) for x in ints))


def test_sumsq_more_than_one_grid_round(ops):
    """Two full rounds of the 2048-workgroup grid, a third, ragged one, and a scalar tail."""
    n = 2 * 2048 * 2048 + 5 * 2048 + 7
    g = np.random.default_rng(7)
    ints = g.integers(-1000, 1001, n)
    got = float(_sumsq(ops, _place(ints.astype(np.float32), 0), 1.0).item())
    assert got == float(np.sum(ints.astype(np.int64) ** 2))
    raw = (g.standard_normal(n) * 1e-14).astype(np.float32)
    val, ref = float(_sumsq(ops, _place(raw, 0)).item()), R.sumsq(raw)
    assert abs(val - ref) <= ref * R.sumsq_bound(n)


@pytest.mark.parametrize("off", [0, 1])
def test_sumsq_range_and_huge_norm(ops, off):
    n = 2 * 256 * 4 + 5
    tiny = np.full(n, 1e-30, np.float32)   # gs = 1e-14, and the raw square (1e-60) is below float32
    val = float(_sumsq(ops, _place(tiny, off)).item())
    ref = R.sumsq(tiny)
    assert ref > 0 and abs(val - ref) <= ref * R.sumsq_bound(n)
    huge = np.full(n, 1e9, np.float32)     # gs = 1e25: its float32 square overflows
    huge[::3] *= -1
    s = _sumsq(ops, _place(huge, off))
    ref = R.sumsq(huge)
    assert np.isfinite(ref) and ref > 1e50 and abs(float(s.item()) - ref) <= ref * R.sumsq_bound(n)
    for c in (1.0, 1e20):  # (both below the norm of ~4.5e26)
        _, rec = _record(ops, s, c)
        assert not rec["skipped"] and np.isfinite(rec["norm"]) and rec["norm"] > 1e25
        assert np.float32(rec["norm"]) == R.norm_of(rec["sumsq"])
        assert np.float32(rec["coef"]) == R.coef_of(rec["norm"], c) and 0 < rec["coef"] < 1


def test_clip_finish_bits(ops, normal_data):
    raw = normal_data[1023]
    s = _sumsq(ops, _place(raw, 0))
    norm = float(R.norm_of(float(s.item())))
    for c, clipped in ((0.25 * norm, True), (norm * (1 + 1e-3), False), (4.0 * norm, False), (math.inf, False)):
        _, rec = _record(ops, s, c)
        assert rec["sumsq"] == float(s.item())
        assert np.float32(rec["norm"]).view(np.uint32) == R.norm_of(rec["sumsq"]).view(np.uint32)
        assert np.float32(rec["coef"]).view(np.uint32) == R.coef_of(rec["norm"], c).view(np.uint32)
        assert (rec["coef"] < 1.0) == clipped and not rec["skipped"] and rec["skipped_total"] == 0
    # several sums are added in index order
    parts = torch.tensor([3.0, 1e-20, 1e20, -1e20, 4.0], dtype=torch.float64, device=DEV)
    _, rec = _record(ops, parts, 1.0)
    assert rec["sumsq"] == ((((3.0 + 1e-20) + 1e20) - 1e20) + 4.0)


def test_validation_and_empty(ops):
    from hdpissa_amd._lib import lib
    L = lib()
    empty = torch.zeros(0, dtype=torch.float32, device=DEV)
    s = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    ops.grad_sumsq(empty, s)
    assert float(s.item()) == 0.0
    _, rec = _record(ops, torch.zeros(0, dtype=torch.float64, device=DEV), 1.0)
    assert rec == {"sumsq": 0.0, "norm": 0.0, "coef": 1.0, "skipped": False, "skipped_total": 0}
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    assert L.hdp_grad_sumsq(None, 4, 1.0, s.data_ptr(), ws.data_ptr(), 512, None) == 1
    assert b"null" in L.hdp_last_error()
    assert L.hdp_grad_sumsq(ws.data_ptr(), -1, 1.0, s.data_ptr(), ws.data_ptr(), 512, None) == 1
    assert b"n < 0" in L.hdp_last_error()
    assert L.hdp_grad_sumsq(ws.data_ptr(), 4, 1.0, None, ws.data_ptr(), 512, None) == 1
    assert L.hdp_grad_sumsq(ws.data_ptr(), 4, 1.0, s.data_ptr(), ws.data_ptr(), 8, None) == 1
    assert b"workspace" in L.hdp_last_error()
    assert L.hdp_clip_finish(s.data_ptr(), 1, 1.0, None, None) == 1
    assert L.hdp_clip_finish(None, 1, 1.0, ws.data_ptr(), None) == 1
    assert L.hdp_clip_finish(s.data_ptr(), -1, 1.0, ws.data_ptr(), None) == 1
    assert L.hdp_clip_finish(s.data_ptr(), 1, 0.0, ws.data_ptr(), None) == 1
    assert b"max_norm" in L.hdp_last_error()
    torch.cuda.synchronize()
    assert float(s.item()) == 0.0 and not torch.any(ws)  # nothing was launched


# ------------------------------------------------------------------------------------- clipped K3
def _adam_inputs(n, t):
    g = np.random.default_rng(100 * n + t)
    raw = (g.standard_normal(n) * 1e-14).astype(np.float32)
    if t == 1:
        return raw, np.zeros(n, np.float32), np.zeros(n, np.float32)
    return raw, (g.standard_normal(n) * 0.3).astype(np.float32), (g.random(n) * 0.2).astype(np.float32)


@pytest.mark.parametrize("zero_grad", [True, False])
@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("n", [5, 1024 + 3, 70_000])
def test_adam_clip(ops, n, t, zero_grad):
    raw, m0, v0 = _adam_inputs(n, t)
    lr = 2e-3

    def run(c):
        g, m, v = (torch.from_numpy(x.copy()).to(DEV) for x in (raw, m0, v0))
        d = torch.full((n,), 9.0, device=DEV)
        rec = None
        if c is None:
            ops.adam(g, m, v, d, t, lr, 0.9, 0.999, 1e-8, zero_grad)
        else:
            state, rec = _record(ops, _sumsq(ops, g), c)
            ops.adam(g, m, v, d, t, lr, 0.9, 0.999, 1e-8, zero_grad, clip=state)
        assert torch.equal(g, torch.zeros_like(g) if zero_grad else torch.from_numpy(raw).to(DEV))
        return m.cpu().numpy(), v.cpu().numpy(), d.cpu().numpy(), rec

    norm = float(R.norm_of(R.sumsq(raw)))
    m, v, d, rec = run(0.3 * norm)
    assert rec["coef"] < 1.0 and np.float32(rec["coef"]) == R.coef_of(rec["norm"], 0.3 * norm)
    mr, vr, dr = R.adam_factors_clip(raw, m0, v0, t, lr, rec["coef"])
    assert np.array_equal(m.view(np.uint32), mr.view(np.uint32))  # (delta alone hardly sees the clip at t = 1)
    assert np.array_equal(v.view(np.uint32), vr.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), dr.view(np.uint32))
    plain = run(None)
    assert not np.array_equal(plain[0], m) and not np.array_equal(plain[1], v)
    for c in (math.inf, norm * (1 + 1e-3)):  # coef = 1: the unclipped bits
        mc, vc, dc, rec = run(c)
        assert rec["coef"] == 1.0
        for a, b in zip((mc, vc, dc), plain[:3]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_adam_skip(ops, bad):
    n, lr = 1024 + 3, 2e-3
    raw, m0, v0 = _adam_inputs(n, 2)
    poisoned = raw.copy()
    poisoned[517] = bad
    g, m, v = (torch.from_numpy(x.copy()).to(DEV) for x in (poisoned, m0, v0))
    d = torch.full((n,), 9.0, device=DEV)
    state, rec = _record(ops, _sumsq(ops, g), 1.0)
    assert rec["skipped"] and rec["skipped_total"] == 1 and rec["coef"] == 1.0
    ops.adam(g, m, v, d, 2, lr, 0.9, 0.999, 1e-8, True, clip=state)
    assert np.array_equal(m.cpu().numpy().view(np.uint32), m0.view(np.uint32))
    assert np.array_equal(v.cpu().numpy().view(np.uint32), v0.view(np.uint32))
    assert not torch.any(d) and not torch.any(g)
    # the next, finite step updates normally (and the counter stays)
    g.copy_(torch.from_numpy(raw))
    _, rec = _record(ops, _sumsq(ops, g), 1.0, state)
    assert not rec["skipped"] and rec["skipped_total"] == 1 and rec["coef"] < 1.0
    ops.adam(g, m, v, d, 3, lr, 0.9, 0.999, 1e-8, True, clip=state)
    mr, vr, dr = R.adam_factors_clip(raw, m0, v0, 3, lr, rec["coef"])
    assert np.array_equal(m.cpu().numpy(), mr) and np.array_equal(v.cpu().numpy(), vr)
    assert np.array_equal(d.cpu().numpy(), dr) and not torch.any(g)
    _, rec = _record(ops, _sumsq(ops, torch.from_numpy(poisoned).to(DEV)), 1.0, state)
    assert rec["skipped"] and rec["skipped_total"] == 2


# ------------------------------------------------------------------------------------- the whole step
def _model(shapes, dt, seed=5):
    model = nn.Module()
    g = torch.Generator().manual_seed(seed)
    for name, out, inn in shapes:
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
        setattr(model, name, lin.to(DEV).to(dt).requires_grad_(False))
    return model


def _grads(L, j, step, scale):
    g = torch.Generator().manual_seed(1000 * step + 10 * j)
    return torch.randn(L.A.shape, generator=g) * scale, torch.randn(L.B.shape, generator=g) * scale


def _set_grads(layers, step, scale):
    for j, L in enumerate(layers):
        gA, gB = _grads(L, j, step, scale)
        L.A.grad, L.B.grad = gA.to(DEV), gB.to(DEV)


SCALES = {1: 1e-14, 2: 1e-15}


@pytest.mark.parametrize("dtname", ["float32", "bfloat16"])
@pytest.mark.parametrize("arenas", [1, 2])
def test_step_wn1(dtname, arenas):
    from helpers import rel_err
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from test_gpu_ranks_one_gpu import SHAPES
    dt, r, lr = getattr(torch, dtname), 16, 2e-3
    names = [s[0] for s in SHAPES]

    def build(c):
        model = _model(SHAPES, dt)
        if arenas == 1:
            layers = replace_with_custom_layer(model, names, 0, 1, r, 16.0)
        else:
            layers = replace_with_custom_layer(model, names[:2], 0, 1, r, 16.0) + \
                replace_with_custom_layer(model, names[2:], 0, 1, r, 16.0)
        return layers, HDPissaStep(model, 1, 0, max_grad_norm=c)

    probe = build(None)[0]
    n1 = math.sqrt(sum(R.sumsq(x.numpy()) for j, L in enumerate(probe) for x in _grads(L, j, 1, SCALES[1])))
    c = 0.3 * n1  # step 1 (norm n1) clips, step 2 (gradients 10 x smaller) does not
    layers, st = build(c)
    assert len(st.plans) == arenas
    F = sum(p.arena.F for p in st.plans)
    mv = [[np.zeros(L.A.shape, np.float32), np.zeros(L.A.shape, np.float32), np.zeros(L.B.shape, np.float32),
           np.zeros(L.B.shape, np.float32)] for L in layers]
    for step in (1, 2):
        W0 = [L.W_res.float().cpu().numpy() for L in layers]
        _set_grads(layers, step, SCALES[step])
        st.step(lr, step)
        info = st.clip_info()
        ss = sum(R.sumsq(x.numpy()) for j, L in enumerate(layers) for x in _grads(L, j, step, SCALES[step]))
        assert abs(info["sumsq"] - ss) <= ss * R.sumsq_bound(F)  # the norm over every arena
        assert np.float32(info["norm"]) == R.norm_of(info["sumsq"])
        assert np.float32(info["coef"]) == R.coef_of(info["norm"], c)
        assert (info["coef"] < 1.0) == (step == 1) and not info["skipped"]
        for j, L in enumerate(layers):
            gA, gB = (x.numpy() for x in _grads(L, j, step, SCALES[step]))
            mA, vA, dA = R.adam_factors_clip(gA, mv[j][0], mv[j][1], step, lr, info["coef"])
            mB, vB, dB = R.adam_factors_clip(gB, mv[j][2], mv[j][3], step, lr, info["coef"])
            mv[j] = [mA, vA, mB, vB]
            for got, ref in ((L.m_A, mA), (L.v_A, vA), (L.m_B, mB), (L.v_B, vB)):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
            da, db = L._arena.views(L._arena.delta, L._arena.layers.index(L))
            assert np.array_equal(da.cpu().numpy(), dA) and np.array_equal(db.cpu().numpy(), dB)
            A, B = L.A.detach().cpu().numpy(), L.B.detach().cpu().numpy()
            ref = O.merge(W0[j], O.delta_w([dA], [dB], [A], [B], dtname), dtname)
            got = L.W_res.float().cpu().numpy()
            if dt == torch.float32:
                assert rel_err(got, ref) < 1e-5, (step, j, rel_err(got, ref))
            else:
                upd = rel_err(got - W0[j], ref - W0[j])
                assert upd < 2e-2, (step, j, upd)


@pytest.mark.parametrize("dtname", ["float32", "bfloat16"])
def test_step_inf_norm_equals_unclipped_step(dtname):
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from test_gpu_ranks_one_gpu import SHAPES
    dt = getattr(torch, dtname)
    res = []
    for c in (None, math.inf):
        model = _model(SHAPES, dt)
        layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, 16, 16.0)
        st = HDPissaStep(model, 1, 0, max_grad_norm=c)
        for step in (1, 2):
            _set_grads(layers, step, SCALES[step])
            st.step(2e-3, step)
        torch.cuda.synchronize()
        ar = layers[0]._arena
        res.append((ar.m.clone(), ar.v.clone(), [L.W_res.clone() for L in layers]))
        if c is not None:
            assert st.clip_info()["coef"] == 1.0 and st.clip_info()["norm"] > 0
    (m1, v1, W1), (m2, v2, W2) = res
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and all(torch.equal(a, b) for a, b in zip(W1, W2))


# ------------------------------------------------------------------------------------- the fused path
def test_fused_adam_pack_clip_and_skip():
    """bf16 W, r = 32, Wn = 1: Adam runs inside the plan's operand preparation.  Step 1 clips, step 2 is
    skipped (one inf), step 3 clips again: m, v, delta equal the K3 path's (HDP_FUSED_ADAM=0) bit for bit, W
    relates to it as in test_fused_adam_step_matches_two_pass, and the skipped step leaves W alone."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    shapes = [("q_proj", 384, 512), ("o_proj", 512, 256)]
    lr = 1e-3
    res = []
    for fused in ("1", "0"):
        os.environ["HDP_FUSED_ADAM"] = fused
        try:
            model = _model(shapes, torch.bfloat16)
            layers = replace_with_custom_layer(model, ["q_proj", "o_proj"], 0, 1, 32, 32.0)
            probe = math.sqrt(sum(R.sumsq(x.numpy()) for j, L in enumerate(layers) for x in _grads(L, j, 1, 1e-14)))
            st = HDPissaStep(model, 1, 0, max_grad_norm=0.3 * probe)
        finally:
            os.environ.pop("HDP_FUSED_ADAM", None)
        plans = st._fused_plans(st.plans[0], lr, 1)
        if fused == "1":
            assert plans is not None and all(p.fused_adam() for p, _ in plans)
        else:
            assert plans is None
        ar = layers[0]._arena
        snaps = []
        for step in (1, 2, 3):
            _set_grads(layers, step, 1e-14)
            if step == 2:
                layers[1].A.grad[5, 7] = math.inf
            m0, v0, W0 = ar.m.clone(), ar.v.clone(), [L.W_res.clone() for L in layers]
            st.step(lr, step)
            info = st.clip_info()
            assert info["skipped"] == (step == 2) and (step == 2 or info["coef"] < 1.0)
            if step == 2:
                assert torch.equal(ar.m, m0) and torch.equal(ar.v, v0) and not torch.any(ar.delta)
                assert all(torch.equal(L.W_res, w) for L, w in zip(layers, W0))
                assert not torch.any(ar.grad)
                if fused == "1":
                    assert not any(p.fused_fallback() for p, _ in plans)
            snaps.append((ar.m.clone(), ar.v.clone(), ar.delta.clone(), [L.W_res.float().clone() for L in layers]))
        res.append(snaps)
    for (m1, v1, d1, W1), (m2, v2, d2, W2) in zip(*res):
        assert torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(d1, d2)
        for a, b in zip(W1, W2):
            assert float((a != b).float().mean()) < 0.02
            ulp = torch.clamp(torch.maximum(a.abs(), b.abs()), min=2.0 ** -126) * 2.0 ** -7
            assert bool(torch.all((a - b).abs() <= ulp * 1.0001)), float(((a - b).abs() / ulp).max())
    assert torch.any(res[0][0][0]) and not torch.equal(res[0][0][0], res[0][2][0])


# ------------------------------------------------------------------------------------- the trainer
class _Toy(nn.Module):
    """Two adapter layers behind an embedding; an HF-style output (.loss)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.emb = nn.Embedding(32, 128)
        self.q_proj = nn.Linear(128, 192, bias=False)
        self.o_proj = nn.Linear(192, 64, bias=False)
        with torch.no_grad():
            self.emb.weight.copy_(torch.randn(32, 128, generator=g))
            self.q_proj.weight.copy_(torch.randn(192, 128, generator=g) * 0.1)
            self.o_proj.weight.copy_(torch.randn(64, 192, generator=g) * 0.1)
        for p in self.parameters():
            p.requires_grad = False

    def forward(self, input_ids, attention_mask=None, labels=None):
        h = self.o_proj(torch.tanh(self.q_proj(self.emb(input_ids))))
        return types.SimpleNamespace(loss=((h.sum(-1) - labels.float()) ** 2).mean())


def test_trainer_logs_the_norm():
    from hdpissa_amd import replace_with_custom_layer
    from hdpissa_amd.train import HDPissaTrainer
    model = _Toy().to(DEV)
    replace_with_custom_layer(model, ["q_proj", "o_proj"], 0, 1, 16, 16.0)
    tr = HDPissaTrainer(model, 1, 0, 1e-3, 3, accumulation_steps=2, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(11)
    norms = []
    for _ in range(6):
        b = dict(input_ids=torch.randint(0, 32, (2, 8), generator=g), attention_mask=torch.ones(2, 8, dtype=torch.long),
                 labels=torch.randint(0, 4, (2, 8), generator=g))
        if tr.micro_step(b):
            norms.append(tr.stepper.clip_info()["norm"])
    assert len(tr.grad_norm_list) == 3 and tr.grad_norm_list == norms and all(n > 0 and math.isfinite(n) for n in norms)
    assert tr.skipped_steps == 0 and len(tr.loss_list) == 3 and all(math.isfinite(x) for x in tr.loss_list)
