"""The round-to-nearest grouped merges (hdp_merge_group with float32 and bf16 W, hdp_merge_group_bf16dw): the
bits of oracle.hdpissa_oracle.merge, nothing outside W, the timing table's bytes.

Every W sits inside a larger buffer pre-filled with a canary that must survive on both sides; every dW sits
inside random data that must not change.  The sizes go around one vector and one chunk of each op (what one
workgroup merges at a time: 4,096 elements for float32 W, 16,384 for bf16 W, 8,192 with a bf16 dW) and the
shifts move W and dW off 16 bytes separately and together, so the vector kernel, the scalar tail and the
element-wise path of a misaligned item are all taken.  All values are finite (the vector path rounds with the
packed conversion, single elements with the scalar one: the same bits for finite values).
"""
import numpy as np
import pytest
import torch

from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64  # elements either side of a range (a multiple of 16 bytes in every dtype)
OPS = {
    # W dtype, dW dtype, elements per vector, elements per chunk, algorithmic bytes per element, oracle dtype
    "f32": (torch.float32, torch.float32, 4, 4096, 12, "float32"),
    "bf16": (torch.bfloat16, torch.float32, 8, 16384, 8, "bfloat16"),
    "bf16dw": (torch.bfloat16, torch.bfloat16, 8, 8192, 6, "bfloat16"),
}


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


def _ints(dt):
    return (torch.int32, np.uint32, 0x5A5A5A5A) if dt == torch.float32 else (torch.int16, np.uint16, 0x5A5A)


def _case(op, n, w_off, d_off, seed):
    """One item: W and dW start ``*_off`` elements past a 64-byte boundary of their buffers.  Returns
    (W, dW, W buffer (integer view), dW buffer copy, expected W bits)."""
    wdt, ddt, _, _, _, model = OPS[op]
    g = np.random.default_rng(1000003 * seed + 17 * n + 3 * w_off + 5 * d_off)
    w = (g.standard_normal(n) * 0.05).astype(np.float32)
    # updates from far below half an ulp of their weight to larger than it
    d = (g.standard_normal(n) * np.exp2(g.integers(-22, 1, n))).astype(np.float32)
    if wdt == torch.bfloat16:
        w = O.round_bf16(w)
    if ddt == torch.bfloat16:
        d = O.round_bf16(d)
    ref = O.merge(w, d, model)
    wi, wnp, canary = _ints(wdt)
    if wdt == torch.bfloat16:
        assert not (ref.view(np.uint32) & 0xFFFF).any()
        ref_bits = (ref.view(np.uint32) >> 16).astype(np.uint16)
    else:
        ref_bits = ref.view(np.uint32)
    wbuf = torch.full((n + 2 * PAD + 16,), canary, dtype=wi, device=DEV)
    dbuf = torch.from_numpy(g.standard_normal(n + 2 * PAD + 16).astype(np.float32)).to(DEV).to(ddt)
    assert wbuf.data_ptr() % 64 == 0 and dbuf.data_ptr() % 64 == 0
    W = wbuf.view(wdt)[PAD + w_off:PAD + w_off + n]
    dW = dbuf[PAD + d_off:PAD + d_off + n]
    W.copy_(torch.from_numpy(w).to(DEV).to(wdt))    # (exact: w holds bf16 values where W is bf16)
    dW.copy_(torch.from_numpy(d).to(DEV).to(ddt))
    return W, dW, wbuf, dbuf.clone(), ref_bits


def _check(op, cases, specs):
    wdt, ddt, *_ = OPS[op]
    wi, wnp, canary = _ints(wdt)
    di = _ints(ddt)[0]
    torch.cuda.synchronize()
    for (W, dW, wbuf, dbuf0, ref_bits), (n, w_off, d_off) in zip(cases, specs):
        got = W.view(wi).cpu().numpy().view(wnp)
        bad = np.flatnonzero(got != ref_bits)
        assert bad.size == 0, (op, n, w_off, d_off, int(bad.size), "first at", int(bad[0]))
        assert bool((wbuf[:PAD + w_off].cpu().numpy().view(wnp) == canary).all()), (op, n, w_off, "canary before W")
        assert bool((wbuf[PAD + w_off + n:].cpu().numpy().view(wnp) == canary).all()), (op, n, w_off, "canary after W")
        assert torch.equal(dW.view(di), dbuf0.view(di)[PAD + d_off:PAD + d_off + n]), (op, n, "dW changed")


def _sizes(op):
    vec, chunk = OPS[op][2], OPS[op][3]
    return [0, 1, vec - 1, vec, vec + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 43]


def _shifts(op):
    vec = OPS[op][2]
    return [(0, 0), (1, 0), (0, 1), (3, 2), (vec, vec), (vec // 2, 0)]


@pytest.mark.parametrize("k", range(9))
@pytest.mark.parametrize("op", list(OPS))
def test_sizes_and_shifts(ops, op, k):
    """Size k of {0, 1, vec-1, vec, vec+1, chunk-1, chunk, chunk+1, 3 chunk + 43} at every W / dW shift, one
    item per call.  ((vec, vec) keeps both 16-byte aligned for a float32 dW; a bf16 dW moved by 8 elements
    too.)"""
    n = _sizes(op)[k]
    for i, (w_off, d_off) in enumerate(_shifts(op)):
        case = _case(op, n, w_off, d_off, seed=i)
        ops.merge_group([(case[0], case[1])])
        _check(op, [case], [(n, w_off, d_off)])


@pytest.mark.parametrize("count", [1, 64, 65])
@pytest.mark.parametrize("op", list(OPS))
def test_item_counts(ops, op, count):
    """1, 64 and 65 non-empty items in one call -- aligned, ragged and misaligned ones mixed, empty items
    among them.  (The launch count is not asserted: these merges keep their per-item path for ragged and
    misaligned items; one launch per 64 items is deferred with their move onto the shared chunk walk.)"""
    from hdpissa_amd._lib import kernel_timing
    vec, chunk, bpe = OPS[op][2], OPS[op][3], OPS[op][4]
    sizes = (3 * vec, 1250, vec + 1, chunk + vec, 1, 2 * chunk + 5)
    shifts = ((0, 0), (1, 0), (vec, vec), (0, 1), (0, 0), (3, 2))
    specs = [(sizes[i % 6], *shifts[(i // 2) % 6]) for i in range(count)]
    specs[0] = (2 * chunk + 40, 0, 0)
    specs = specs[:1] + [(0, 0, 0)] + specs[1:] + [(0, 1, 1)]
    cases = [_case(op, n, w, d, seed=i) for i, (n, w, d) in enumerate(specs)]
    kernel_timing(enable=True, reset=True)
    try:
        ops.merge_group([(c[0], c[1]) for c in cases])
        torch.cuda.synchronize()
        kt = kernel_timing(reset=True)
    finally:
        kernel_timing(enable=False)
    _check(op, cases, specs)
    total = sum(n for n, _, _ in specs)
    assert kt["merge"]["bytes_per_launch"] * kt["merge"]["launches"] == pytest.approx(bpe * total)


@pytest.mark.parametrize("op", list(OPS))
def test_only_empty_items_launch_nothing(ops, op):
    from hdpissa_amd._lib import kernel_timing
    cases = [_case(op, 0, 0, 0, seed=0), _case(op, 0, 1, 1, seed=1)]
    kernel_timing(enable=True, reset=True)
    try:
        ops.merge_group([(c[0], c[1]) for c in cases])
        torch.cuda.synchronize()
        kt = kernel_timing(reset=True)
    finally:
        kernel_timing(enable=False)
    _check(op, cases, [(0, 0, 0), (0, 1, 1)])
    assert "merge" not in kt
