"""Adapter dropout on the GPU: the kernel's mask against the host replica bit for bit, the fused masked probe
backward against the float64 formula

    D = G^T X,   gA = s/(1-p) B^T (M . D),   gB = s/(1-p) (M . D) A^T

with the replica's mask M (the bar the unmasked probe is held to: norm-wise 1e-5), its bitwise
reproducibility, and the autograd path of a CustomLinearLayer with dropout > 0."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = (5 << 32) | 0x9E3779B9   # above 2^32
OFF0 = (3 << 32) | 7            # above 2^32
OFF1 = (3 << 32) | 8
SCALE = float(np.float32(1e-16) * np.float32(2.0))

# T, out, in, r: several tiles both ways, ragged by 8, T not a multiple of the k chunk / one r-block of 64 /
# exact tiles at the largest r
SHAPES = [(136, 392, 520, 16), (72, 264, 136, 64), (64, 256, 256, 128)]


def _ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


# the last four: out * in no multiple of 4 (the last thread writes 1 - 3 elements); 3 x 1025 ends one element
# into a second block of 256 threads
@pytest.mark.parametrize("out,inn", [(392, 520), (264, 136), (1, 1), (7, 13), (75, 130), (3, 1025)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_equals_host_replica(out, inn, p):
    from hdpissa_amd._lib import check, lib
    from hdpissa_amd.dropout import dropout_mask_reference
    ref = dropout_mask_reference(out, inn, p, SEED, OFF0)
    m = _ops().dropout_mask(out, inn, p, SEED, OFF0)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (out, inn)
    assert np.array_equal(m.cpu().numpy(), ref)
    # the same call into a buffer with a guard behind the mask: nothing is written past out * in
    n, guard = out * inn, 1024
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    check(lib().hdp_dropout_mask(out, inn, p, SEED, OFF0, buf.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "hdp_dropout_mask")
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n], ref.reshape(-1))
    assert np.all(got[n:] == 0xA5)


@functools.lru_cache(maxsize=None)
def _case(T, out, inn, r, bf16, p):
    """Inputs (on the device) and the float64 references of the two offsets, computed once per case."""
    from hdpissa_amd.dropout import dropout_mask_reference
    g = np.random.default_rng(1000 * r + T)
    dt = torch.bfloat16 if bf16 else torch.float32
    X = torch.from_numpy(g.standard_normal((T, inn)).astype(np.float32)).to(DEV).to(dt)
    G = torch.from_numpy(g.standard_normal((T, out)).astype(np.float32)).to(DEV).to(dt)
    A = torch.from_numpy(g.standard_normal((r, inn)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(g.standard_normal((out, r)).astype(np.float32)).to(DEV)
    X64, G64 = X.float().cpu().numpy().astype(np.float64), G.float().cpu().numpy().astype(np.float64)
    A64, B64 = A.cpu().numpy().astype(np.float64), B.cpu().numpy().astype(np.float64)
    D = G64.T @ X64
    refs = []
    for off in (OFF0, OFF1):
        MD = dropout_mask_reference(out, inn, p, SEED, off) * D
        s = SCALE / (1.0 - p)
        refs.append((s * (B64.T @ MD), s * (MD @ A64.T)))
    return X, G, A, B, refs


@pytest.mark.parametrize("with_bt", [False, True], ids=["B", "Bt"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,out,inn,r", SHAPES)
def test_masked_probe_against_float64(T, out, inn, r, bf16, with_bt):
    p = 0.3
    X, G, A, B, refs = _case(T, out, inn, r, bf16, p)
    ops = _ops()
    Bt = B.t().contiguous() if with_bt else None
    gA = torch.full_like(A, float("nan"))  # accumulate = 0 must overwrite
    gB = torch.full_like(B, float("nan"))
    ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, False, p, SEED, OFF0, Bt=Bt)
    eA, eB = O.rel_err(gA.cpu().numpy(), refs[0][0]), O.rel_err(gB.cpu().numpy(), refs[0][1])
    print(f"overwrite: rel_err gA {eA:.3e} gB {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5
    ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, True, p, SEED, OFF1, Bt=Bt)
    eA = O.rel_err(gA.cpu().numpy(), refs[0][0] + refs[1][0])
    eB = O.rel_err(gB.cpu().numpy(), refs[0][1] + refs[1][1])
    print(f"accumulate: rel_err gA {eA:.3e} gB {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_masked_probe_is_bitwise_reproducible(bf16):
    T, out, inn, r = SHAPES[0]
    X, G, A, B, _ = _case(T, out, inn, r, bf16, 0.3)
    ops = _ops()
    res = []
    for _ in range(2):
        gA, gB = torch.empty_like(A), torch.empty_like(B)
        ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, False, 0.3, SEED, OFF0)
        res.append((gA, gB))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    gA, gB = torch.empty_like(A), torch.empty_like(B)
    ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, False, 0.3, SEED, OFF1)
    assert not torch.equal(gA, res[0][0])  # another offset is another mask


def test_empty_batch():
    _, out, inn, r = SHAPES[1]
    _, _, A, B, _ = _case(*SHAPES[1], False, 0.3)
    X, G = torch.empty(0, inn, device=DEV), torch.empty(0, out, device=DEV)
    gA, gB = torch.ones_like(A), torch.ones_like(B)
    _ops().probe_grads_dropout(X, G, A, B, gA, gB, SCALE, True, 0.3, SEED, OFF0)
    assert torch.all(gA == 1) and torch.all(gB == 1)
    _ops().probe_grads_dropout(X, G, A, B, gA, gB, SCALE, False, 0.3, SEED, OFF0)
    assert not torch.any(gA) and not torch.any(gB)


def _model(W, dropout, factors=None):
    from hdpissa_amd import CustomLinearLayer, replace_with_custom_layer
    out, inn = W.shape
    model = nn.Module()
    model.q_proj = nn.Linear(inn, out, bias=False).to(DEV)
    with torch.no_grad():
        model.q_proj.weight.copy_(torch.from_numpy(W))
    model.q_proj.weight.requires_grad = False
    if factors is None:
        (layer,) = replace_with_custom_layer(model, ["q_proj"], 0, 1, 16, 32.0, dropout)
    else:
        layer = CustomLinearLayer(model.q_proj, "q_proj", 0, 1, 16, 32.0, dropout, _factors=factors)
        model.q_proj = layer
    return model, layer


def test_layer_autograd_path():
    from hdpissa_amd import hd_pissa_step
    from hdpissa_amd.dropout import dropout_mask_reference
    out, inn, p = 200, 136, 0.25
    g = np.random.default_rng(7)
    q1, _ = np.linalg.qr(g.standard_normal((out, inn)))
    q2, _ = np.linalg.qr(g.standard_normal((inn, inn)))
    W = ((q1 * 0.95 ** np.arange(inn)) @ q2.T).astype(np.float32)
    model, layer = _model(W, p)
    _, plain = _model(W, 0.0, (layer.A.detach().clone(), layer.B.detach().clone()[None]))
    assert layer.training and layer.dropout_rate == p and layer.dropout_calls == 0
    s = layer.probe_scale / (1.0 - p)
    A64, B64 = layer.A.detach().cpu().numpy().astype(np.float64), layer.B.detach().cpu().numpy().astype(np.float64)
    refA, refB, states = 0.0, 0.0, []
    for mb in range(2):
        x = torch.from_numpy(g.standard_normal((3, 8, inn)).astype(np.float32)).to(DEV)
        G = torch.from_numpy(g.standard_normal((3, 8, out)).astype(np.float32)).to(DEV)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = layer(xa), plain(xb)
        ya.backward(G)
        yb.backward(G)
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)
        seed, off = layer.last_dropout_state
        assert seed == torch.cuda.initial_seed() and off == mb and layer.dropout_calls == mb + 1
        states.append(off)
        D = G.reshape(-1, out).cpu().numpy().astype(np.float64).T @ x.reshape(-1, inn).cpu().numpy().astype(np.float64)
        MD = dropout_mask_reference(out, inn, p, seed, off) * D
        refA = refA + s * (B64.T @ MD)
        refB = refB + s * (MD @ A64.T)
    assert states[0] != states[1]
    eA, eB = O.rel_err(layer.A.grad.cpu().numpy(), refA), O.rel_err(layer.B.grad.cpu().numpy(), refB)
    print(f"layer: rel_err A.grad {eA:.3e} B.grad {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5
    assert O.rel_err(layer.A.grad.cpu().numpy(), plain.A.grad.cpu().numpy()) > 1e-2  # the mask did act

    # eval: today's unmasked path, bit for bit; no RNG state is drawn
    layer.eval()
    for L in (layer, plain):
        L.A.grad, L.B.grad = None, None
    x = torch.from_numpy(g.standard_normal((5, inn)).astype(np.float32)).to(DEV)
    G = torch.from_numpy(g.standard_normal((5, out)).astype(np.float32)).to(DEV)
    layer(x).backward(G)
    plain(x).backward(G)
    torch.cuda.synchronize()
    assert layer.dropout_calls == 2
    assert torch.equal(layer.A.grad, plain.A.grad) and torch.equal(layer.B.grad, plain.B.grad)

    # a masked micro-batch on top of the queued path, then the optimizer step consumes the gradients
    layer.train()
    layer(x).backward(G)
    assert layer.last_dropout_state[1] == 2
    W0 = layer.W_res.clone()
    hd_pissa_step(model, 1e-2, 1, 1)
    torch.cuda.synchronize()
    assert not torch.equal(layer.W_res, W0) and bool(torch.isfinite(layer.W_res).all())


def test_layer_full_dropout_contributes_nothing():
    g = np.random.default_rng(3)
    W = g.standard_normal((64, 48)).astype(np.float32)
    A = torch.from_numpy(g.standard_normal((16, 48)).astype(np.float32)).to(DEV)
    B = torch.from_numpy(g.standard_normal((64, 16)).astype(np.float32)).to(DEV)
    _, layer = _model(W, 1.0, (A, B[None]))
    x = torch.from_numpy(g.standard_normal((4, 48)).astype(np.float32)).to(DEV)
    G = torch.from_numpy(g.standard_normal((4, 64)).astype(np.float32)).to(DEV)
    layer(x).backward(G)
    assert not torch.any(layer.A.grad) and not torch.any(layer.B.grad)
    layer.eval()
    layer(x).backward(G)
    torch.cuda.synchronize()
    kept = layer.A.grad.clone()
    assert torch.any(kept)
    layer.train()
    layer(x).backward(G)  # accumulating call with everything dropped leaves the gradients
    assert torch.equal(layer.A.grad, kept)
