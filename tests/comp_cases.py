"""The input table of the compensated-merge contract tests (tests/test_comp_contract.py on the host,
tests/test_gpu_merge_comp.py on the GPU, tiled): (bf16 bits of W, bf16 bits of C, float32 dW) triples.

* random finite weights W ~ 0.05 N(0, 1) with |dW| from 1e-3 to 4 bf16 ulp of W, both signs, and C in turn
  zero, +- small (up to 0.4 ulp), exactly +- half an ulp, and +- 1.5 ulp;
* SPECIAL: sums that are exactly a bf16 value (c' = 0), ties, the largest finite value with a carry
  (w' = inf, c' = +0), +-inf and NaN in W and in dW (c' = +0), subnormal sums, and +-0.
"""
import math

import numpy as np

INF, NAN = float("inf"), float("nan")
_TOP = float(np.uint32(0x7F7FFFFF).view(np.float32) - np.uint32(0x7F7F0000).view(np.float32))  # exact: 16 set bits


def bf16_bits(x) -> int:
    """The bf16 bits of a float that is exactly a bf16 value."""
    u = int(np.float32(x).view(np.uint32))
    assert u & 0xFFFF == 0, x
    return u >> 16


H = bf16_bits(2.0 ** -8)   # half an ulp of 1.0
SPECIAL = [
    # (w, c, dW)                                  what the contract gives
    (0x3F80, 0x0000, 2.0 ** -7),                  # 0: s = 1 + ulp exactly: w' = 0x3F81, c' = 0
    (0x3F80, H, 2.0 ** -8),                       # 1: c + dW = one ulp exactly: w' = 0x3F81, c' = 0
    (0x3F80, 0x0000, 0.0),                        # 2: nothing to add: (0x3F80, 0)
    (0x3F80, H, 0.0),                             # 3: a tie, to even: w' = 0x3F80, c' = +half an ulp
    (0x3F81, H, 0.0),                             # 4: a tie, to even: w' = 0x3F82, c' = -half an ulp
    (0x3F80, bf16_bits(1.5 * 2.0 ** -7), 1e-4),   # 5: c above an ulp: w' moves by two ulp
    (0xBF80, bf16_bits(-(2.0 ** -9)), -(2.0 ** -9)),  # 6: two quarter-ulps make the half: the tie stays, c' = -half
    (0x7F7F, 0x0000, _TOP),                       # 7: the largest finite float32 sum: carry, w' = inf, c' = +0
    (0xFF7F, 0x0000, -_TOP),                      # 8: w' = -inf, c' = +0
    (0x7F7F, 0x0000, 1e37),                       # 9: the float32 add itself overflows
    (0xFF7F, 0x3C00, -1e37),                      # 10
    (0x7F80, 0x0000, 1.0),                        # 11: +inf in W
    (0xFF80, 0x3C00, 1.0),                        # 12: -inf in W
    (0x3F80, 0x0000, INF),                        # 13: +inf in dW
    (0x3F80, 0x3C00, -INF),                       # 14: -inf in dW
    (0x7F80, 0x0000, -INF),                       # 15: inf - inf: NaN
    (0x7FC0, 0x0000, 0.0),                        # 16: NaN in W
    (0x3F80, 0x0000, NAN),                        # 17: NaN in dW
    (0xFFC1, 0x3C00, 1.0),                        # 18: NaN in W with a payload
    (0x0001, 0x0000, 0.0),                        # 19: subnormal W stays: (0x0001, 0)
    (0x0001, 0x0000, 1e-42),                      # 20: subnormal sums
    (0x0080, 0x0000, -1e-40),                     # 21
    (0x0001, 0x0001, 1e-41),                      # 22
    (0x0000, 0x0000, 0.0),                        # 23: +0
    (0x8000, 0x0000, 0.0),                        # 24: -0 + 0 = +0
    (0x8000, 0x8000, -0.0),                       # 25: all -0: w' = -0
    (0x0000, 0x8000, 0.0),                        # 26
]
NSPECIAL = len(SPECIAL)


def comp_cases(seed: int, n: int):
    """``n`` random triples followed by SPECIAL: (w bits uint16, c bits uint16, dW float32) arrays."""
    from hdpissa_amd.rounding import rne_bf16_bits
    g = np.random.default_rng(seed)
    w = (g.standard_normal(n) * 0.05).astype(np.float32)
    wb = (w.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    wf = (wb.astype(np.uint32) << np.uint32(16)).view(np.float32)
    ulp = np.exp2(np.frexp(np.abs(wf))[1].astype(np.float64) - 8.0)  # |w| = m 2^e, m in [0.5, 1): ulp = 2^(e - 8)
    dw = (ulp * np.exp(g.uniform(math.log(1e-3), math.log(4.0), n)) * g.choice([-1.0, 1.0], n)).astype(np.float32)
    kind = np.arange(n) % 7
    scale = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                      [0.0 * ulp, g.uniform(0.0, 0.4, n), -g.uniform(0.0, 0.4, n), 0.5 + 0 * ulp, -0.5 + 0 * ulp,
                       1.5 + 0 * ulp], -1.5 + 0 * ulp)
    cb = rne_bf16_bits((scale * ulp).astype(np.float32).view(np.uint32)).astype(np.uint16)
    sw = np.array([s[0] for s in SPECIAL], dtype=np.uint16)
    sc = np.array([s[1] for s in SPECIAL], dtype=np.uint16)
    sd = np.array([s[2] for s in SPECIAL], dtype=np.float32)
    return np.concatenate([wb, sw]), np.concatenate([cb, sc]), np.concatenate([dw, sd])
