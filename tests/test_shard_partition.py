"""shard_rows: the row partition of exchange="shard" (host, pure function)."""
import pytest

from hdpissa_amd.step import shard_rows

OUTS = [1, 7, 8, 20, 128, 200, 1376 * 8, 4096]
WNS = [1, 2, 4, 8]


@pytest.mark.parametrize("wn", WNS)
@pytest.mark.parametrize("out", OUTS)
def test_partition(out, wn):
    blocks = [shard_rows(out, wn, k) for k in range(wn)]
    # disjoint, ordered, covering [0, out)
    assert blocks[0][0] == 0 and blocks[-1][1] == out
    for (a0, a1), (b0, b1) in zip(blocks, blocks[1:]):
        assert a1 == b0
    for r0, r1 in blocks:
        assert 0 <= r0 <= r1 <= out
        # every block that holds rows starts on a multiple of 8 (an empty trailing block is
        # (out, out) by the min() of the definition: it has no row pointer to align)
        assert r0 % 8 == 0 if r1 > r0 else r0 == out
    # equal lengths except the trailing ones: full blocks, then at most one short block, then empty ones
    block = 8 * -(-out // (8 * wn))
    lens = [r1 - r0 for r0, r1 in blocks]
    full = [n for n in lens if n == block]
    assert lens[:len(full)] == full
    rest = lens[len(full):]
    assert all(n < block for n in rest)
    assert all(n == 0 for n in rest[1:])
    assert sum(lens) == out


@pytest.mark.parametrize("out", OUTS)
def test_world_size_one_is_the_whole_matrix(out):
    assert shard_rows(out, 1, 0) == (0, out)


def test_short_and_empty_trailing_blocks():
    # out = 200 at Wn = 8: blocks of 32 rows, rank 6 gets 8 rows and rank 7 none
    assert [shard_rows(200, 8, k) for k in range(8)] == \
        [(0, 32), (32, 64), (64, 96), (96, 128), (128, 160), (160, 192), (192, 200), (200, 200)]
    assert shard_rows(7, 4, 0) == (0, 7) and shard_rows(7, 4, 3) == (7, 7)
