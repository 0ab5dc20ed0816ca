"""Stochastic-rounding merge on the host (CPU): the header the kernel shares (csrc/hdp_sr.h), compiled with the
host compiler -- plain and with -fsanitize=address,undefined -- behind tests/sr_check.cpp, against the numpy
replica (hdpissa_amd/rounding.py): r16 and the rounding function at every residue of e mod 8, from e = 0 and
around e = 2^35 (the block index crosses 2^32), for finite, exactly representable, largest-finite, +-inf and
NaN sums; the replica's own properties (unbiased up-rounding per bin of the low half, dW = 0 a no-op); and the
step's host logic through a test-only op set (CpuOps + merge_group_sr from the replica): every rank bitwise
equal under gloo, the constructor's gates, float32 modules of a mixed model untouched."""
import math
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from cpu_ops import CpuOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SR_SRC = os.path.join(ROOT, "tests", "sr_check.cpp")
SR_INC = os.path.join(ROOT, "hd-pissa_amd", "csrc")
H_SEED = (0x1234 << 32) | 0x9E3779B9   # above 2^32
H_OFF = (5 << 32) | 0xFFFFFFFE         # module 5, t = 2^32 - 2
HI = 1 << 35  # element index whose block index (e >> 3) is 2^32: the counter's low word wraps, the high word is 1


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if c and shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module", params=[("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                ids=["plain", "asan-ubsan"])
def sr_exe(request, tmp_path_factory):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("sr") / "sr_check")
    # g++ does not know the headers' `#pragma unroll`
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", *request.param, "-I", SR_INC, SR_SRC,
                    "-o", exe], check=True)

    def run(*args):
        p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        return [int(x, 16) for x in p.stdout.split()]
    return run


def _r16_by_hand(e, seed, offset):
    """The contract with the counter written out, one element at a time: no use of rounding.sr_r16."""
    from hdpissa_amd.dropout import philox4x32_10
    blk = e >> 3
    words = philox4x32_10((blk & 0xFFFFFFFF, blk >> 32, offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    w = int(np.asarray(words[(e & 7) >> 1]).reshape(-1)[0])
    return (w >> (16 * (e & 1))) & 0xFFFF


@pytest.mark.parametrize("start", [0, HI - 2048], ids=["from-0", "around-2^35"])
def test_header_r16(sr_exe, start):
    """4096 consecutive elements: every residue of e mod 8; around 2^35 the block counter's high word changes."""
    from hdpissa_amd.rounding import sr_r16
    n = 4096
    e = np.uint64(start) + np.arange(n, dtype=np.uint64)
    want = sr_r16(e, H_SEED, H_OFF)
    for j in list(range(16)) + [2040, 2047, 2048, 2049, 2055, 4095]:
        assert int(want[j]) == _r16_by_hand(start + j, H_SEED, H_OFF), j
    got = sr_exe("r16", H_SEED, H_OFF, start, n)
    assert len(got) == n
    bad = [start + j for j in range(n) if got[j] != int(want[j])]
    assert not bad, f"r16 differs from the replica at e = {bad[:8]} ({len(bad)} of {n})"
    assert max(got) <= 0xFFFF and len(set(got)) > n // 2


def test_r16_sees_every_argument():
    from hdpissa_amd.rounding import sr_r16
    e = np.arange(4096, dtype=np.uint64)
    a = sr_r16(e, H_SEED, H_OFF)
    assert np.any(a != sr_r16(e + np.uint64(HI), H_SEED, H_OFF))               # the counter's high word
    assert np.any(a != sr_r16(e, H_SEED & 0xFFFFFFFF, H_OFF))                   # the seed's high word
    assert np.any(a != sr_r16(e, H_SEED, H_OFF & 0xFFFFFFFF))                   # the module index
    assert np.any(a != sr_r16(e, H_SEED, H_OFF + 1))                            # the step counter
    assert np.any(a.reshape(-1, 8)[:, 0] != a.reshape(-1, 8)[:, 1])             # the halves of one word


def _cases(g, n):
    """(bf16 bits of W, float32 dW) pairs: random finite ones with |dW| from ~1e-3 to 4 bf16 ulp of W, then the
    special sums, repeated so that every one meets every residue of e mod 8."""
    w = (g.standard_normal(n) * 0.05).astype(np.float32)
    wb = (w.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    wf = (wb.astype(np.uint32) << np.uint32(16)).view(np.float32)
    ulp = np.abs(wf) * np.float32(2.0 ** -7)
    dw = (ulp * np.exp(g.uniform(math.log(1e-3), math.log(4.0), n)) * g.choice([-1.0, 1.0], n)).astype(np.float32)
    top = np.uint32(0x7F7FFFFF).view(np.float32) - np.uint32(0x7F7F0000).view(np.float32)  # exact: 16 set bits
    special = [
        (0x3F80, 0.0), (0x3F80, 2.0 ** -7), (0xBF80, -2.0 ** -7), (0x3F80, -0.0), (0x0000, 0.0), (0x8000, 0.0),  # exact
        (0x7F7F, float(top)), (0xFF7F, -float(top)),      # the largest finite float32 sum: any r16 > 0 carries to inf
        (0x7F7F, 1e37), (0xFF7F, -1e37),                  # the float32 add itself overflows: an infinite sum
        (0x7F80, 1.0), (0xFF80, 1.0), (0x3F80, float("inf")), (0x3F80, float("-inf")),          # +-inf
        (0x7F80, float("-inf")), (0x7FC0, 0.0), (0x3F80, float("nan")), (0xFFC1, 1.0),          # NaN sums
        (0x0001, 0.0), (0x0001, 1e-42), (0x0080, -1e-40),                                        # subnormal sums
    ]
    sw = np.array([s[0] for s in special] * 9, dtype=np.uint16)   # 21 cases x 9: 21 is odd, so the residues turn
    sd = np.array([s[1] for s in special] * 9, dtype=np.float32)
    return np.concatenate([wb, sw]), np.concatenate([dw, sd])


@pytest.mark.parametrize("e0", [0, 3, HI - 24, HI - 21], ids=["0", "3", "2^35-24", "2^35-21"])
def test_header_merge(sr_exe, e0):
    from hdpissa_amd.rounding import sr_merge_bits
    wb, dw = _cases(np.random.default_rng(7 + e0 % 1000), 1024)
    want = sr_merge_bits(wb, dw, e0, H_SEED, H_OFF)
    args = []
    for a, b in zip(wb, dw.view(np.uint32)):
        args += [hex(int(a)), hex(int(b))]
    got = np.array(sr_exe("merge", H_SEED, H_OFF, e0, *args), dtype=np.uint16)
    assert got.shape == want.shape
    nan = (want & 0x7FFF) > 0x7F80
    assert np.array_equal(nan, (got & 0x7FFF) > 0x7F80), "NaN positions differ"
    bad = np.nonzero((got != want) & ~nan)[0]
    assert bad.size == 0, f"e0 = {e0}: bits differ at {bad[:8]}: got {got[bad[:8]]} want {want[bad[:8]]}"
    # the special values did what the contract says (replica side; the header equals it bit for bit)
    sp = want[1024:].reshape(9, -1)
    assert np.all(sp[:, 0] == 0x3F80) and np.all(sp[:, 1] == 0x3F81) and np.all(sp[:, 2] == 0xBF81)
    assert np.all(sp[:, 3] == 0x3F80) and np.all(sp[:, 4] == 0x0000)
    assert np.all(np.isin(sp[:, 6], [0x7F7F, 0x7F80])) and np.any(sp[:, 6] == 0x7F80)
    assert np.all(np.isin(sp[:, 7], [0xFF7F, 0xFF80])) and np.any(sp[:, 7] == 0xFF80)
    assert np.all(sp[:, 8] == 0x7F80) and np.all(sp[:, 9] == 0xFF80)
    assert np.all(sp[:, 10] == 0x7F80) and np.all(sp[:, 11] == 0xFF80) and np.all(sp[:, 12] == 0x7F80)
    assert np.all(sp[:, 13] == 0xFF80)
    assert np.all((sp[:, 14:18] & 0x7FFF) > 0x7F80)
    # the random part really rounds both ways
    dn = (wb[:1024].astype(np.uint32) << 16).view(np.float32) + dw[:1024]
    assert 0.05 < np.mean(want[:1024] != (dn.view(np.uint32) >> 16)) < 0.95


def test_replica_up_rounding_is_unbiased():
    """2^16 elements whose float32 sums have the low halves 0 .. 65535 (each once), 256 offsets: in each of 16
    equal-width bins of the low half the share rounded up lies within 5 binomial standard deviations of
    bin centre / 65536 (an element with low half l rounds up iff l + r16 >= 65536: probability l / 65536)."""
    from hdpissa_amd.rounding import sr_offset, sr_r16, sr_round_bits
    n, noff = 1 << 16, 256
    low = np.random.default_rng(3).permutation(n).astype(np.uint32)  # (not aligned with e mod 8)
    u = np.uint32(0x3F800000) | low
    e = np.arange(n, dtype=np.uint64)
    up = np.zeros(n, dtype=np.int64)
    for t in range(1, noff + 1):
        out = sr_round_bits(u, sr_r16(e, 20240607, sr_offset(3, t)))
        assert np.all((out == 0x3F80) | (out == 0x3F81))
        up += out == 0x3F81
    for b in range(16):
        sel = (low >> 12) == b
        trials = int(sel.sum()) * noff
        p = (4096 * b + 2047.5) / 65536.0
        freq = up[sel].sum() / trials
        sd = math.sqrt(p * (1 - p) / trials)
        assert abs(freq - p) <= 5 * sd, (b, freq, p, sd)


def test_replica_zero_dw_changes_nothing():
    from hdpissa_amd.rounding import sr_merge_bits
    g = np.random.default_rng(11)
    wb = g.integers(0, 1 << 16, 1 << 14).astype(np.uint16)
    wb = wb[(wb & 0x7FFF) <= 0x7F80]  # (no NaN: a NaN never compares equal)
    out = sr_merge_bits(wb, np.zeros(wb.size, np.float32), 5, 99, 1)
    f = lambda b: (b.astype(np.uint32) << 16).view(np.float32)  # noqa: E731
    assert np.array_equal(f(out), f(wb))
    assert np.array_equal(out[wb != 0x8000], wb[wb != 0x8000])  # only -0 + 0 = +0 changes bits


def test_seed_and_offset_helpers():
    from hdpissa_amd.rounding import SR_SEED_OFFSET, default_sr_seed, sr_offset
    assert SR_SEED_OFFSET % 2 == 1 and SR_SEED_OFFSET < 1 << 64
    assert default_sr_seed(0) == SR_SEED_OFFSET and default_sr_seed((1 << 64) - 1) == SR_SEED_OFFSET - 1
    assert sr_offset(3, 7) == (3 << 32) | 7 and sr_offset(1, (1 << 32) + 2) == (1 << 32) | 2


# ---- the step's host logic through a test-only op set ------------------------------------------------------
class SrCpuOps(CpuOps):
    """CpuOps + merge_group_sr from the numpy replica -- TEST ONLY."""
    name = "cpu-test-sr"

    def __init__(self, factors=None):
        super().__init__(factors)
        self.sr_calls = []

    def merge_group_sr(self, triples, seed):
        from hdpissa_amd.rounding import sr_merge_reference
        for W, dW, elem0, offset in triples:
            assert W.dtype == torch.bfloat16 and dW.dtype == torch.float32 and W.numel() == dW.numel()
            self.sr_calls.append((W.numel(), int(elem0), int(offset)))
            W.copy_(sr_merge_reference(W, dW.reshape(W.shape), elem0, seed, offset))


def _model(shapes, dts, seed=5):
    model = nn.Module()
    g = torch.Generator().manual_seed(seed)
    for (name, out, inn), dt in zip(shapes, dts):
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
        setattr(model, name, lin.to(dt).requires_grad_(False))
    return model


SHAPES = [("q_proj", 48, 40), ("k_proj", 20, 40), ("o_proj", 64, 24), ("up_proj", 40, 56)]


def _grads(L, j, rank, step):
    g = torch.Generator().manual_seed(1000 * step + 10 * j + rank)
    return torch.randn(L.A.shape, generator=g) * 1e-14, torch.randn(L.B.shape, generator=g) * 1e-14


def test_op_set_without_the_kernel_is_refused():
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    model = _model(SHAPES[:1], [torch.bfloat16])
    ops = CpuOps()
    assert not hasattr(ops, "merge_group_sr")
    replace_with_custom_layer(model, ["q_proj"], 0, 1, 4, 16.0, ops=ops)
    with pytest.raises(NotImplementedError):
        HDPissaStep(model, 1, 0, ops=ops, merge_rounding="stochastic")
    HDPissaStep(model, 1, 0, ops=ops)  # "nearest" needs nothing new


def test_bad_merge_rounding_is_a_value_error():
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    model = _model(SHAPES[:1], [torch.bfloat16])
    ops = SrCpuOps()
    replace_with_custom_layer(model, ["q_proj"], 0, 1, 4, 16.0, ops=ops)
    for bad in ("stochastic-ish", "", None, "NEAREST"):
        with pytest.raises(ValueError):
            HDPissaStep(model, 1, 0, ops=ops, merge_rounding=bad)


@pytest.mark.parametrize("exchange", ["gather", "allreduce"])
def test_mixed_model_float32_modules_untouched(exchange):
    """bf16 and float32 modules in one arena: after two steps the float32 W are bit-identical to a "nearest"
    run, the bf16 W equal the replica applied to the float32 dW (recomputed with the op set's own K4 STORE),
    and the stream is keyed by (module index, t)."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from hdpissa_amd.rounding import sr_merge_reference, sr_offset
    dts = [torch.bfloat16, torch.float32, torch.bfloat16, torch.float32]
    names = [s[0] for s in SHAPES]
    runs = {}
    for mode in ("nearest", "stochastic"):
        model = _model(SHAPES, dts)
        ops = SrCpuOps()
        layers = replace_with_custom_layer(model, names, 0, 1, 4, 16.0, ops=ops)
        st = HDPissaStep(model, 1, 0, ops=ops, exchange=exchange, bucket_bytes=4096, merge_rounding=mode, sr_seed=77)
        for step in (1, 2):
            for j, L in enumerate(layers):
                L.A.grad, L.B.grad = _grads(L, j, 0, step)
            before = [L.W_res.clone() for L in layers]
            st.step(2e-3, step)
            if mode == "stochastic":
                arena = layers[0]._arena
                for j, L in enumerate(layers):
                    if L.W_res.dtype != torch.bfloat16:
                        continue
                    oa, ob = arena.offsets[j]
                    dW = torch.zeros(L.out_features, L.in_features)
                    ops.delta_gemm(L.out_features, L.in_features, L.r, 1, arena.delta[oa:], arena.delta[ob:], 0,
                                   arena.fac[oa:], arena.fac[ob:], 0, dW, 0, False)
                    want = sr_merge_reference(before[j], dW, 0, 77, sr_offset(j, step))
                    assert torch.equal(L.W_res.view(torch.int16), want.view(torch.int16)), (step, j)
                    assert not torch.equal(L.W_res, before[j])
        runs[mode] = ([L.W_res.clone() for L in layers], ops.sr_calls)
    (wn, calls_n), (ws, calls_s) = runs["nearest"], runs["stochastic"]
    assert calls_n == []
    assert sorted(calls_s) == sorted((SHAPES[j][1] * SHAPES[j][2], 0, sr_offset(j, t)) for j in (0, 2) for t in (1, 2))
    for j, dt in enumerate(dts):
        if dt == torch.float32:
            assert torch.equal(wn[j], ws[j]), j
        else:
            assert not torch.equal(wn[j], ws[j]), j


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, wn, port, exchange, errfile):
    import sys
    for p in (HERE, ROOT, os.path.join(ROOT, "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from hdpissa_amd.comm import TorchComm
        from hdpissa_amd.rounding import sr_merge_reference, sr_offset
        from test_sr_host import SHAPES, SrCpuOps, _grads, _model
        model = _model(SHAPES, [torch.bfloat16] * 4)
        comm, ops = TorchComm(rank, wn), SrCpuOps()
        layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], rank, wn, 4, 16.0, comm=comm, ops=ops)
        st = HDPissaStep(model, wn, rank, comm=comm, ops=ops, exchange=exchange, bucket_bytes=4096,
                         merge_rounding="stochastic", sr_seed=123)
        arena = layers[0]._arena
        for step in (1, 2):
            for j, L in enumerate(layers):
                L.A.grad, L.B.grad = _grads(L, j, rank, step)
            before = [L.W_res.clone() for L in layers]
            st.step(2e-3, step)
            for j, L in enumerate(layers):
                w = L.W_res.float().clone()
                ws = [torch.zeros_like(w) for _ in range(wn)]
                dist.all_gather(ws, w)
                assert all(torch.equal(ws[0], x) for x in ws), f"step {step} module {j}: ranks differ"
                assert not torch.equal(L.W_res, before[j])
            if exchange == "gather":
                # W = the replica on the float32 sum over ranks of the K4 terms (no per-rank bf16 rounding),
                # recomputed by the same whole-module call the step made
                F, fac = arena.F, arena.fac_all.view(-1)
                deltas = [torch.zeros(F) for _ in range(wn)]
                dist.all_gather(deltas, arena.delta.clone())
                dall = torch.cat(deltas)
                for j, L in enumerate(layers):
                    oa, ob = arena.offsets[j]
                    dW = torch.zeros(L.out_features, L.in_features)
                    ops.delta_gemm(L.out_features, L.in_features, L.r, wn, dall[oa:], dall[ob:], F, fac[oa:], fac[ob:], F,
                                   dW, 0, False)
                    want = sr_merge_reference(before[j], dW, 0, 123, sr_offset(j, step))
                    assert torch.equal(L.W_res.view(torch.int16), want.view(torch.int16)), (step, j)
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange", ["allreduce", "gather", "shard"])
def test_gloo_ranks_bitwise_equal(exchange, tmp_path):
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(_worker, args=(2, _port(), exchange, errfile), nprocs=2, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")
