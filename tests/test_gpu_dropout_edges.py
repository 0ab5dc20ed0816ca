"""The masked probe backward at the shapes where its branches lie: the scalar load path of ragged rows (alone and
mixed with the vector path), Philox blocks that straddle a lane's four elements (`in` no multiple of 4), r
tails, more than one band of in-tiles with a partial last band, T = 1 / one past a chunk / below one bf16 MFMA
step, p next to 0 and next to 1, and the layer around it (bf16, two masked layers, ragged 3-D input at an odd
storage offset, masked calls next to queued unmasked ones).

Two kinds of check: integer inputs, where every partial sum is an integer below 2^24 and the float64 result
must come out bit for bit, and Gaussian inputs against the float64 formula with the host replica's mask at the
bar of tests/test_gpu_dropout.py (norm-wise 1e-5)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import hdpissa_oracle as O
from test_gpu_dropout import OFF0, OFF1, SCALE, SEED, _case, _ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# T, out, in, r
EDGE_SHAPES = [
    (1, 75, 130, 20),     # one token; scalar loads of X and G in both dtypes; in % 4 == 2; r tail
    (33, 136, 1160, 16),  # 10 in-tiles: a full band of 8 and a band of 2; 2 out-tiles; 20 tiles (xcd_remap's
                          # remainder arm); one token past a 32-token chunk
    (17, 1160, 68, 100),  # 10 out-tiles, 1 in-tile; r = 100: 7 blocks, the last of 4; X vector loads in float32
                          # but scalar in bf16, G vector loads in both
    (40, 129, 257, 1),    # one element past a tile both ways; r = 1; odd in: all four residues of e0
    (9, 130, 131, 128),   # the largest r on ragged tiles; in % 4 == 3; T < 16
]
_IDS = ["x".join(map(str, s)) for s in EDGE_SHAPES]


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _masked_ref(D, A64, B64, mask, s):
    MD = mask * D
    return s * (B64.T @ MD), s * (MD @ A64.T)


# ---- exact integer layout ---------------------------------------------------------------------------------
INT_SCALE = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def _int_case(T, out, inn, r, p):
    """Integer X, G in [-3, 3] and A, B in [-2, 2] (exact in bf16 and float32) and the float64 results of the
    two offsets.  |D| <= 9 T, so a partial sum of either contraction is an integer of magnitude at most
    2 * 9 * T * max(out, in), and so is the sum of the two calls' halves; INT_SCALE / (1 - p) is a power of
    two.  Everything the kernel adds is therefore exact in float32 in any order."""
    from hdpissa_amd.dropout import dropout_mask_reference
    assert 2 * (2 * 9 * T * max(out, inn)) < 2 ** 24
    assert float(np.log2(1.0 - p)).is_integer()
    g = np.random.default_rng(77 * T + r)
    X = g.integers(-3, 4, (T, inn)).astype(np.float32)
    G = g.integers(-3, 4, (T, out)).astype(np.float32)
    A = g.integers(-2, 3, (r, inn)).astype(np.float32)
    B = g.integers(-2, 3, (out, r)).astype(np.float32)
    D = G.astype(np.float64).T @ X.astype(np.float64)
    refs = [_masked_ref(D, A.astype(np.float64), B.astype(np.float64), dropout_mask_reference(out, inn, p, SEED, off),
                        INT_SCALE / (1.0 - p)) for off in (OFF0, OFF1)]
    dev = [torch.from_numpy(a).to(DEV) for a in (X, G, A, B)]
    return dev, refs


@pytest.mark.parametrize("with_bt", [False, True], ids=["B", "Bt"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", [0.5, 0.75])
@pytest.mark.parametrize("T,out,inn,r", EDGE_SHAPES, ids=_IDS)
def test_masked_probe_integer_layout(T, out, inn, r, p, bf16, with_bt):
    (X, G, A, B), refs = _int_case(T, out, inn, r, p)
    if bf16:
        X, G = X.to(torch.bfloat16), G.to(torch.bfloat16)
    Bt = B.t().contiguous() if with_bt else None
    ops = _ops()
    gA = torch.full_like(A, float("nan"))  # accumulate = 0 must overwrite
    gB = torch.full_like(B, float("nan"))
    ops.probe_grads_dropout(X, G, A, B, gA, gB, INT_SCALE, False, p, SEED, OFF0, Bt=Bt)
    wantA, wantB = (torch.from_numpy(a.astype(np.float32)) for a in refs[0])
    assert torch.equal(gA.cpu(), wantA), f"gA: {int((gA.cpu() != wantA).sum())} of {wantA.numel()} entries differ"
    assert torch.equal(gB.cpu(), wantB), f"gB: {int((gB.cpu() != wantB).sum())} of {wantB.numel()} entries differ"
    ops.probe_grads_dropout(X, G, A, B, gA, gB, INT_SCALE, True, p, SEED, OFF1, Bt=Bt)
    wantA, wantB = (torch.from_numpy((a + b).astype(np.float32)) for a, b in zip(refs[0], refs[1]))
    assert torch.equal(gA.cpu(), wantA), f"gA += : {int((gA.cpu() != wantA).sum())} of {wantA.numel()} entries differ"
    assert torch.equal(gB.cpu(), wantB), f"gB += : {int((gB.cpu() != wantB).sum())} of {wantB.numel()} entries differ"


# ---- float64 parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bt", [False, True], ids=["B", "Bt"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("T,out,inn,r", EDGE_SHAPES, ids=_IDS)
def test_masked_probe_against_float64_at_the_edges(T, out, inn, r, bf16, with_bt):
    p = 0.3
    X, G, A, B, refs = _case(T, out, inn, r, bf16, p)
    ops = _ops()
    Bt = B.t().contiguous() if with_bt else None
    gA = torch.full_like(A, float("nan"))
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


P_SHAPE = (72, 264, 136, 64)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_tiny_p_keeps_everything_and_equals_the_unmasked_probe(bf16):
    """p = 1e-9: the threshold is 4, so (for this seed and offset) no element is dropped and 1 - p is 1 in float32:
    the masked kernel and the unmasked probe are both held to the unmasked float64 formula."""
    from hdpissa_amd.dropout import dropout_mask_reference, dropout_threshold
    T, out, inn, r = P_SHAPE
    p = 1e-9
    assert dropout_threshold(p) == 4
    assert dropout_mask_reference(out, inn, p, SEED, OFF0).all()
    X, G, A, B, _ = _case(T, out, inn, r, bf16, 0.3)
    D = _np64(G).T @ _np64(X)
    refA, refB = SCALE * (_np64(B).T @ D), SCALE * (D @ _np64(A).T)
    ops = _ops()
    gA, gB = torch.full_like(A, float("nan")), torch.full_like(B, float("nan"))
    ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, False, p, SEED, OFF0)
    eA, eB = O.rel_err(gA.cpu().numpy(), refA), O.rel_err(gB.cpu().numpy(), refB)
    print(f"p = 1e-9 masked: rel_err gA {eA:.3e} gB {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5
    uA, uB = torch.full_like(A, float("nan")), torch.full_like(B, float("nan"))
    ops.probe_grads(X, G, A, B, uA, uB, SCALE, False)
    eA, eB = O.rel_err(uA.cpu().numpy(), refA), O.rel_err(uB.cpu().numpy(), refB)
    print(f"unmasked probe: rel_err gA {eA:.3e} gB {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_p_next_to_one(bf16):
    """p = 0.999: a few dozen elements survive and carry a factor of about 1000.  The kernel sees float32(p) and
    its 1.0f - p is exact for p >= 0.5, so the reference uses float32(p) throughout (1 - 0.999 and
    1 - float32(0.999) differ by 2e-5 relative, more than the bar)."""
    from hdpissa_amd.dropout import dropout_mask_reference
    T, out, inn, r = P_SHAPE
    p = 0.999
    p32 = float(np.float32(p))
    masks = [dropout_mask_reference(out, inn, p32, SEED, off) for off in (OFF0, OFF1)]
    for m in masks:
        assert 1 <= int(m.sum()) < 0.01 * m.size
    print(f"kept {int(masks[0].sum())} and {int(masks[1].sum())} of {masks[0].size}")
    X, G, A, B, _ = _case(T, out, inn, r, bf16, 0.3)
    D = _np64(G).T @ _np64(X)
    refs = [_masked_ref(D, _np64(A), _np64(B), m, SCALE / (1.0 - p32)) for m in masks]
    ops = _ops()
    gA, gB = torch.full_like(A, float("nan")), torch.full_like(B, float("nan"))
    ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, False, p, SEED, OFF0)
    eA, eB = O.rel_err(gA.cpu().numpy(), refs[0][0]), O.rel_err(gB.cpu().numpy(), refs[0][1])
    print(f"overwrite: rel_err gA {eA:.3e} gB {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5
    ops.probe_grads_dropout(X, G, A, B, gA, gB, SCALE, True, p, SEED, OFF1)
    eA = O.rel_err(gA.cpu().numpy(), refs[0][0] + refs[1][0])
    eB = O.rel_err(gB.cpu().numpy(), refs[0][1] + refs[1][1])
    print(f"accumulate: rel_err gA {eA:.3e} gB {eB:.3e}")
    assert eA < 1e-5 and eB < 1e-5


# ---- the layer --------------------------------------------------------------------------------------------
def _layers(specs, r, alpha, dropout, dtype=torch.float32):
    """A model of len(specs) adapter layers in ONE arena, from given (W, A, B) (numpy): no SVD runs."""
    from hdpissa_amd import CustomLinearLayer
    from hdpissa_amd.layer import FactorArena
    model, layers, factors = nn.Module(), [], []
    for j, (W, A, B) in enumerate(specs):
        out, inn = W.shape
        lin = nn.Linear(inn, out, bias=False).to(DEV).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W))
        lin.weight.requires_grad = False
        fac = (torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)[None])
        layer = CustomLinearLayer(lin, f"p{j}_proj", 0, 1, r, alpha, dropout, _factors=fac, _defer_arena=True)
        setattr(model, f"p{j}_proj", layer)
        layers.append(layer)
        factors.append(fac)
    FactorArena(layers, factors, 1, 0, torch.device(DEV))
    return model, layers


def _spec(g, out, inn, r):
    return (g.standard_normal((out, inn)).astype(np.float32) / np.sqrt(inn),
            g.standard_normal((r, inn)).astype(np.float32), g.standard_normal((out, r)).astype(np.float32))


def _xg(g, lead, inn, out, dtype=torch.float32):
    x = torch.from_numpy(g.standard_normal((*lead, inn)).astype(np.float32)).to(DEV).to(dtype)
    G = torch.from_numpy(g.standard_normal((*lead, out)).astype(np.float32)).to(DEV).to(dtype)
    return x, G


def _layer_terms(layer, x, G, state=None):
    """float64 (gA, gB) of one call: unmasked (state None) or with the replica mask of state = (p, seed, offset)."""
    from hdpissa_amd.dropout import dropout_mask_reference
    out, inn = layer.out_features, layer.in_features
    D = _np64(G).reshape(-1, out).T @ _np64(x).reshape(-1, inn)
    if state is None:
        mask, s = 1.0, layer.probe_scale
    else:
        p, seed, off = state
        mask, s = dropout_mask_reference(out, inn, p, seed, off), layer.probe_scale / (1.0 - p)
    return _masked_ref(D, _np64(layer.A), _np64(layer.B), mask, s)


def _grad_err(layer, refA, refB, what):
    eA, eB = O.rel_err(layer.A.grad.cpu().numpy(), refA), O.rel_err(layer.B.grad.cpu().numpy(), refB)
    print(f"{what}: rel_err A.grad {eA:.3e} B.grad {eB:.3e}")
    return eA, eB


def test_bf16_layer():
    out, inn, r, p = 264, 136, 16, 0.25
    g = np.random.default_rng(11)
    spec = _spec(g, out, inn, r)
    _, (layer,) = _layers([spec], r, 32.0, p, torch.bfloat16)
    _, (plain,) = _layers([spec], r, 32.0, 0.0, torch.bfloat16)
    assert layer.W_res.dtype == torch.bfloat16 and layer.A.dtype == torch.float32
    refA, refB = 0.0, 0.0
    for mb in range(2):
        x, G = _xg(g, (3, 8), inn, out, torch.bfloat16)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, yb = layer(xa), plain(xb)
        ya.backward(G)
        yb.backward(G)
        assert ya.dtype == torch.bfloat16
        assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad)  # the mask touches neither
        seed, off = layer.last_dropout_state
        assert off == mb
        a, b = _layer_terms(layer, x, G, (p, seed, off))
        refA, refB = refA + a, refB + b
    assert layer.A.grad.dtype == torch.float32
    eA, eB = _grad_err(layer, refA, refB, "bf16 layer")
    assert eA < 1e-5 and eB < 1e-5
    assert O.rel_err(layer.A.grad.cpu().numpy(), plain.A.grad.cpu().numpy()) > 1e-2  # the mask did act


def test_two_masked_layers_have_their_own_masks():
    """Same shape, same factors, same x and G: the two layers differ in the arena index alone, which is the high
    half of the RNG offset."""
    out, inn, r, p = 200, 136, 16, 0.25
    g = np.random.default_rng(12)
    spec = _spec(g, out, inn, r)
    _, layers = _layers([spec, spec], r, 32.0, p)
    x, G = _xg(g, (24,), inn, out)
    refs = []
    for L in layers:
        L(x).backward(G)
        seed, off = L.last_dropout_state
        assert off & 0xFFFFFFFF == 0
        refs.append(_layer_terms(L, x, G, (p, seed, off)))
    hi = [L.last_dropout_state[1] >> 32 for L in layers]
    assert hi == [0, 1]
    for j, L in enumerate(layers):
        eA, eB = _grad_err(L, *refs[j], f"layer {j}, own mask")
        assert eA < 1e-5 and eB < 1e-5
        eA, eB = _grad_err(L, *refs[1 - j], f"layer {j}, the other's mask")
        assert eA > 1e-2 and eB > 1e-2


def test_ragged_layer_with_3d_and_offset_input():
    """out x in = 75 x 130 (scalar loads, in % 4 == 2), r = 20; a 3-D x, then x[1:] / G[1:] whose storage offsets
    are no multiple of 16 bytes (the layer re-bases them)."""
    out, inn, r, p = 75, 130, 20, 0.25
    g = np.random.default_rng(13)
    _, (layer,) = _layers([_spec(g, out, inn, r)], r, 40.0, p)
    assert layer.alpha == 2.0 and layer.probe_scale > 0
    x, G = _xg(g, (3, 5), inn, out)
    layer(x).backward(G)
    refA, refB = _layer_terms(layer, x, G, (p, *layer.last_dropout_state))
    xb, Gb = _xg(g, (4, 5), inn, out)
    xs, Gs = xb[1:], Gb[1:]
    assert xs.is_contiguous() and xs.data_ptr() & 15 and Gs.data_ptr() & 15
    layer(xs).backward(Gs)
    assert layer.last_dropout_state[1] == 1
    a, b = _layer_terms(layer, xs, Gs, (p, *layer.last_dropout_state))
    eA, eB = _grad_err(layer, refA + a, refB + b, "ragged layer")
    assert eA < 1e-5 and eB < 1e-5


@pytest.mark.parametrize("direct", [False, True], ids=["autograd", "pending-queue"])
@pytest.mark.parametrize("masked_first", [False, True], ids=["unmasked-then-masked", "masked-then-unmasked"])
def test_masked_and_queued_calls_keep_their_order(masked_first, direct):
    """An unmasked call of the layer goes through the probe queue, a masked one runs at once: no synchronise lies
    between them, and the sum is the unmasked float64 term plus the masked one.  `pending-queue` calls
    _probe_backward outside autograd, where the unmasked item is still queued when the masked call arrives."""
    from hdpissa_amd import flush_probes
    out, inn, r, p = 264, 136, 16, 0.25
    g = np.random.default_rng(14)
    model, (layer,) = _layers([_spec(g, out, inn, r)], r, 32.0, p)
    x1, G1 = _xg(g, (3, 8), inn, out)
    x2, G2 = _xg(g, (40,), inn, out)
    state = [None]

    def unmasked():
        if direct:
            layer._probe_backward(x1, G1)
            assert layer._arena.probe_queue.pending(layer)
        else:
            layer.eval()
            layer(x1).backward(G1)

    def masked():
        if direct:
            state[0] = (p, SEED, OFF0)
            layer._probe_backward(x2, G2, state[0])
        else:
            layer.train()
            layer(x2).backward(G2)
            state[0] = (p, *layer.last_dropout_state)

    for call in ((masked, unmasked) if masked_first else (unmasked, masked)):
        call()  # nothing here reads the device back
    flush_probes(model)
    u, m = _layer_terms(layer, x1, G1), _layer_terms(layer, x2, G2, state[0])
    eA, eB = _grad_err(layer, u[0] + m[0], u[1] + m[1], "ordering")
    assert eA < 1e-5 and eB < 1e-5
    assert O.rel_err(layer.A.grad.cpu().numpy(), u[0]) > 1e-2  # both calls are in the sum
    assert O.rel_err(layer.A.grad.cpu().numpy(), m[0]) > 1e-2
