"""hdp_copy_group (the shard exchange's pack / scatter kernel): byte-exact, and nothing outside its ranges.

Every destination range sits inside a larger buffer pre-filled with a canary byte that must survive on both
sides; every source range sits inside random bytes that must not change.  A chunk is what one workgroup
copies at a time: 256 lanes x 8 vectors x 16 bytes.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 256 * 8 * 16
CANARY = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import default_ops
    return default_ops()


def _case(nbytes, dst_off=0, src_off=0, seed=0):
    """(dst view, src view, dst buffer, src buffer copy): the views start ``*_off`` bytes past a 64-byte
    boundary of their (512-byte aligned) buffers."""
    g = torch.Generator().manual_seed(1000 * seed + nbytes + 16 * dst_off + src_off)
    sbuf = torch.randint(0, 256, (nbytes + 2 * PAD + 16,), dtype=torch.uint8, generator=g).to(DEV)
    dbuf = torch.full((nbytes + 2 * PAD + 16,), CANARY, dtype=torch.uint8, device=DEV)
    assert sbuf.data_ptr() % 64 == 0 and dbuf.data_ptr() % 64 == 0
    return (dbuf[PAD + dst_off:PAD + dst_off + nbytes], sbuf[PAD + src_off:PAD + src_off + nbytes], dbuf,
            sbuf.clone())


def _check(cases, dst_offs):
    torch.cuda.synchronize()
    for (dst, src, dbuf, sbuf0), off in zip(cases, dst_offs):
        n = dst.numel()
        assert torch.equal(dst, src), n
        assert torch.equal(src, sbuf0[src.storage_offset():src.storage_offset() + n]), n  # source untouched
        assert bool((dbuf[:PAD + off] == CANARY).all()), (n, "canary before the range")
        assert bool((dbuf[PAD + off + n:] == CANARY).all()), (n, "canary after the range")


def _run(ops, specs):
    cases = [_case(n, d, s, seed=i) for i, (n, d, s) in enumerate(specs)]
    ops.copy_group([(c[0], c[1]) for c in cases])
    _check(cases, [d for _, d, _ in specs])


@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, CHUNK, CHUNK + 16, 2500, 1 << 20])
def test_sizes(ops, nbytes):
    """0 B .. 17 B, exactly one chunk, one chunk + one vector, 5 rows x 250 bf16 (no multiple of 16), 1 MB."""
    _run(ops, [(nbytes, 0, 0)])


@pytest.mark.parametrize("dst_off,src_off", [(0, 2), (2, 0), (8, 8), (5, 5), (3, 11)])
@pytest.mark.parametrize("nbytes", [1, 15, 17, 2500, 2 * CHUNK + 100])
def test_alignments(ops, nbytes, dst_off, src_off):
    """dst aligned with src at offset 2, the reverse (both byte by byte), and both at offset 8 (a head up to
    dst's next 16-byte boundary, vectors, a tail); odd equal and unequal offsets as well."""
    _run(ops, [(nbytes, dst_off, src_off)])


@pytest.mark.parametrize("count", ["one", "cap", "cap+1"])
def test_item_counts(ops, count):
    """1, cap and cap + 1 non-empty items in one call: the last needs a second launch (and only the last)."""
    from hdpissa_amd._lib import COPY_GROUP_MAX, kernel_timing
    n = {"one": 1, "cap": COPY_GROUP_MAX, "cap+1": COPY_GROUP_MAX + 1}[count]
    # sizes around the vector and chunk edges, a few alignments; one item of several chunks
    specs = [((48, 2500, 17, CHUNK + 16, 1)[i % 5], (0, 8, 0, 3)[i % 4], (0, 8, 2, 3)[i % 4]) for i in range(n)]
    specs[0] = (3 * CHUNK + 40, 0, 0)
    cases = [_case(nb, d, s, seed=i) for i, (nb, d, s) in enumerate(specs)]
    kernel_timing(enable=True, reset=True)
    try:
        ops.copy_group([(c[0], c[1]) for c in cases])
        torch.cuda.synchronize()
        kt = kernel_timing(reset=True)
    finally:
        kernel_timing(enable=False)
    _check(cases, [d for _, d, _ in specs])
    assert kt["copy_group"]["launches"] == (2 if count == "cap+1" else 1)
    total = sum(nb for nb, _, _ in specs)
    # the timing table's algorithmic bytes: 2 x the bytes copied
    assert kt["copy_group"]["bytes_per_launch"] * kt["copy_group"]["launches"] == pytest.approx(2 * total)


def test_zero_length_items_in_the_middle(ops):
    _run(ops, [(100, 0, 0), (0, 0, 0), (0, 4, 2), (CHUNK + 5, 8, 8), (0, 0, 0), (33, 1, 0)])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_tensor_row_blocks(ops, dt):
    """Row blocks of bf16 / float32 matrices through HipOps.copy_group, packed into a byte buffer and
    scattered back into another matrix (what the shard exchange does)."""
    g = torch.Generator().manual_seed(3)
    W = torch.randn(40, 250, generator=g).to(DEV).to(dt)
    esz = W.element_size()
    blocks = [(8, 13), (16, 40), (0, 8)]
    buf = torch.full((40 * 250 * esz + 64,), CANARY, dtype=torch.uint8, device=DEV)
    offs, off = [], 0
    for r0, r1 in blocks:
        offs.append(off)
        off += -(-(r1 - r0) * 250 * esz // 16) * 16
    ops.copy_group([(buf[o:o + (r1 - r0) * 250 * esz], W[r0:r1]) for o, (r0, r1) in zip(offs, blocks)])
    V = torch.full_like(W, 7.0)
    ops.copy_group([(V[r0:r1], buf[o:o + (r1 - r0) * 250 * esz]) for o, (r0, r1) in zip(offs, blocks)])
    torch.cuda.synchronize()
    for r0, r1 in blocks:
        assert torch.equal(V[r0:r1], W[r0:r1])
    assert bool((V[13:16] == 7.0).all())  # rows of no block stay
    for o, (r0, r1) in zip(offs, blocks):  # the slot padding stays
        end = o + (r1 - r0) * 250 * esz
        assert bool((buf[end:-(-end // 16) * 16] == CANARY).all())
    with pytest.raises(ValueError):
        ops.copy_group([(V[0:2], W[0:3])])
    with pytest.raises(ValueError):
        ops.copy_group([(V[:, :8], W[:, :8])])
