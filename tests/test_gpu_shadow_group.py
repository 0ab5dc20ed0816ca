"""hdp_shadow_group (the grouped float32 -> bf16 cast behind compute_dtype=): the bits of the host replica
rounding.rne_bf16_bits, and nothing outside its ranges.

Finite outputs must match the replica bit for bit and NaN must sit where the replica has NaN.  Every
destination range sits inside a larger buffer pre-filled with a canary that must survive on both sides; every
source range sits inside random data that must not change.  A chunk is what one workgroup casts at a time:
256 lanes x 8 vectors x 8 elements.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0x5A5A  # (int16 view of the bf16 destination buffers)
PAD = 64         # elements either side of a range


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


def _chunk():
    from hdpissa_amd._lib import SHADOW_CHUNK
    return SHADOW_CHUNK


def _values(n, seed):
    """n float32 bit patterns: N(0,1) values with every special class spliced in where it fits."""
    g = np.random.default_rng(seed)
    u = g.standard_normal(n).astype(np.float32).view(np.uint32).copy()
    hi = (g.integers(0, 1 << 16, n).astype(np.uint32) & np.uint32(0x7FFF)) | (g.integers(0, 2, n).astype(np.uint32) << 15)
    hi = np.where((hi & 0x7F80) == 0x7F80, hi & np.uint32(0xBFFF), hi).astype(np.uint32)  # (finite upper halves)
    special = [
        hi << 16,                                    # exact bf16 values
        ((hi & ~np.uint32(1)) << 16) | 0x8000,       # exact ties, even upper half (round down)
        ((hi | np.uint32(1)) << 16) | 0x8000,        # exact ties, odd upper half (round up; may carry)
        ((hi & ~np.uint32(1)) << 16) | 0x8001,       # tie + 1 ulp
        ((hi | np.uint32(1)) << 16) | 0x7FFF,        # tie - 1 ulp
        (hi << 16) | 0x8001, (hi << 16) | 0x7FFF,
    ]
    k = 0
    for sp in special:
        idx = np.arange(k, n, 16)
        u[idx] = sp[idx].astype(np.uint32)
        k += 1
    consts = [0x7F7FFFFF, 0xFF7FFFFF,                # largest finite float32, both signs (-> +-inf)
              0x7F7F8000, 0x7F7F7FFF,                # tie at the top (-> inf) and just below (-> largest bf16)
              0x7F800000, 0xFF800000,                # +-inf
              0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FBFFFFF, 0xFF80FFFF,  # quiet and signalling NaN
              0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x00008000, 0x00007FFF, 0x00018000, 0x807F8000,  # subnormals
              0x00000000, 0x80000000]                # +-0
    for j, c in enumerate(consts):
        if 7 + 16 * j < n:
            u[7 + 16 * j] = c
        elif j < n:
            u[j] = c
    return u


def _case(n, dst_off=0, src_off=0, seed=0):
    """(dst view, src view, dst buffer (int16 view), src buffer copy, source bits): the views start ``*_off``
    elements past a 64-byte boundary of their buffers."""
    bits = _values(n, 7919 * seed + n + 3 * dst_off + 5 * src_off)
    g = np.random.default_rng(seed + 1)
    sb = g.standard_normal(n + 2 * PAD + 8).astype(np.float32).view(np.uint32)
    sb[PAD + src_off:PAD + src_off + n] = bits
    sbuf = torch.from_numpy(sb.view(np.float32).copy()).to(DEV)
    dbuf = torch.full((n + 2 * PAD + 8,), CANARY, dtype=torch.int16, device=DEV)
    assert sbuf.data_ptr() % 64 == 0 and dbuf.data_ptr() % 64 == 0
    dst = dbuf.view(torch.bfloat16)[PAD + dst_off:PAD + dst_off + n]
    src = sbuf[PAD + src_off:PAD + src_off + n]
    return dst, src, dbuf, sbuf.clone(), bits


def _check(cases, specs):
    from hdpissa_amd.rounding import rne_bf16_bits
    torch.cuda.synchronize()
    for (dst, src, dbuf, sbuf0, bits), (n, d_off, s_off) in zip(cases, specs):
        got = dst.view(torch.int16).cpu().numpy().view(np.uint16)
        ref = rne_bf16_bits(bits).astype(np.uint16)
        nan = (ref & 0x7FFF) > 0x7F80
        assert np.array_equal((got & 0x7FFF) > 0x7F80, nan), (n, "NaN positions")
        assert np.array_equal(got[~nan], ref[~nan]), (n, d_off, s_off, int(np.sum(got[~nan] != ref[~nan])))
        assert torch.equal(src.view(torch.int32), sbuf0.view(torch.int32)[PAD + s_off:PAD + s_off + n]), n  # source untouched
        assert bool((dbuf[:PAD + d_off] == CANARY).all()), (n, "canary before the range")
        assert bool((dbuf[PAD + d_off + n:] == CANARY).all()), (n, "canary after the range")


def _run(ops, specs):
    cases = [_case(n, d, s, seed=i) for i, (n, d, s) in enumerate(specs)]
    ops.shadow_group([(c[0], c[1]) for c in cases])
    _check(cases, specs)
    return cases


def test_chunk_is_what_the_sizes_assume():
    assert _chunk() == 16384


# dst element offsets are 2 bytes, src element offsets 4 bytes: (dst_off, src_off) = both aligned, src off by
# 4 bytes, dst off by 2 bytes, both off
ALIGN = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.mark.parametrize("dst_off,src_off", ALIGN)
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 16383, 16384, 16385, 3 * 16384 + 43])
def test_sizes_and_alignments(ops, n, dst_off, src_off):
    """Around one vector (8), around one chunk, several chunks with a vector and an element tail; at each
    alignment pairing (only both-aligned items run as vectors)."""
    _run(ops, [(n, dst_off, src_off)])


def test_aligned_to_16_bytes_but_not_more(ops):
    """Offsets that keep both pointers 16-byte aligned (8 bf16 / 4 float32 elements) take the vector path."""
    cases = _run(ops, [(16384 + 13, 8, 4), (100, 8, 0)])
    assert cases[0][0].data_ptr() % 16 == 0 and cases[0][1].data_ptr() % 16 == 0


@pytest.mark.parametrize("count", ["one", "cap", "cap+1"])
def test_item_counts(ops, count):
    """1, cap and cap + 1 non-empty items in one call, empty items among them: the last needs a second launch
    (and only the last)."""
    from hdpissa_amd._lib import SHADOW_GROUP_MAX, kernel_timing
    n = {"one": 1, "cap": SHADOW_GROUP_MAX, "cap+1": SHADOW_GROUP_MAX + 1}[count]
    specs = [((24, 1250, 9, 16384 + 8, 1)[i % 5], (0, 1, 0, 8)[i % 4], (0, 0, 1, 4)[i % 4]) for i in range(n)]
    specs[0] = (2 * 16384 + 40, 0, 0)
    specs = specs[:1] + [(0, 0, 0)] + specs[1:] + [(0, 1, 1)]
    cases = [_case(k, d, s, seed=i) for i, (k, d, s) in enumerate(specs)]
    kernel_timing(enable=True, reset=True)
    try:
        ops.shadow_group([(c[0], c[1]) for c in cases])
        torch.cuda.synchronize()
        kt = kernel_timing(reset=True)
    finally:
        kernel_timing(enable=False)
    _check(cases, specs)
    assert kt["shadow_group"]["launches"] == (2 if count == "cap+1" else 1)
    total = sum(k for k, _, _ in specs)
    # the timing table's algorithmic bytes: 4 read + 2 written per element
    assert kt["shadow_group"]["bytes_per_launch"] * kt["shadow_group"]["launches"] == pytest.approx(6 * total)


def test_only_empty_items_launch_nothing(ops):
    from hdpissa_amd._lib import kernel_timing
    kernel_timing(enable=True, reset=True)
    try:
        _run(ops, [(0, 0, 0), (0, 1, 1)])
        kt = kernel_timing(reset=True)
    finally:
        kernel_timing(enable=False)
    assert "shadow_group" not in kt


def test_weight_matrices(ops):
    """Whole matrices through HipOps.shadow_group: ragged (in % 8 != 0) and tile-sized, against torch's own
    round-to-nearest-even cast; and the wrapper's checks."""
    g = torch.Generator().manual_seed(3)
    Ws = [torch.randn(75, 130, generator=g).to(DEV) * 0.05, torch.randn(128, 192, generator=g).to(DEV)]
    lps = [torch.empty_like(W, dtype=torch.bfloat16) for W in Ws]
    ops.shadow_group(list(zip(lps, Ws)))
    torch.cuda.synchronize()
    for lp, W in zip(lps, Ws):
        assert torch.equal(lp.view(torch.int16), W.to(torch.bfloat16).view(torch.int16))
    with pytest.raises(TypeError):
        ops.shadow_group([(lps[0].float(), Ws[0])])
    with pytest.raises(TypeError):
        ops.shadow_group([(lps[0], Ws[0].to(torch.bfloat16))])
    with pytest.raises(ValueError):
        ops.shadow_group([(lps[0][:2], Ws[0][:3])])
    with pytest.raises(ValueError):
        ops.shadow_group([(lps[1][:, :8], Ws[1][:, :8])])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shadow_group([(lps[0].cpu(), Ws[0].cpu())])
