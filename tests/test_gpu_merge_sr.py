"""merge_rounding="stochastic" on the GPU: hdp_merge_group_sr against the numpy replica bit for bit (sizes around
the 16384-element chunk, misaligned items, element indices around 2^35, 1 / 64 / 65 items per call, canaries),
the step's plumbing at Wn = 1 (W = replica(W before, the float32 dW of a separately built K4 STORE plan), with
and without max_grad_norm, seeds), ranks as processes on the one GPU (gather and shard, Wn = 2 and 8), the reason
for the feature (128 constant-gradient steps at lr 5e-5: round-to-nearest drops the update, stochastic rounding
keeps it) and resume.

Measured (MI355X) -- see DESIGN section 3.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from oracle import hdpissa_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda:0")
CHUNK = 16384          # elements of one chunk of the vector kernel: 256 lanes x 8 vectors x 8 bf16
CANARY = 0x5A5B        # bf16 bits either side of every W
PAD = 64               # canary elements either side (a multiple of 8: W's alignment is the item's own shift)
SEED = (0xABCD << 32) | 0x1234567
HI = 1 << 35


@pytest.fixture(scope="module")
def ops():
    from hdpissa_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------ the kernel
SPECIAL = [
    (0x3F80, 0.0), (0x3F80, 2.0 ** -7), (0xBF80, -2.0 ** -7), (0x3F80, -0.0), (0x0000, 0.0), (0x8000, 0.0),
    (0x7F7F, None), (0xFF7F, None),                   # the largest finite float32 sum (dW filled in below)
    (0x7F7F, 1e37), (0xFF7F, -1e37),                  # the add overflows
    (0x7F80, 1.0), (0xFF80, 1.0), (0x3F80, float("inf")), (0x3F80, float("-inf")),
    (0x7F80, float("-inf")), (0x7FC0, 0.0), (0x3F80, float("nan")), (0xFFC1, 1.0),
]
_TOP = float(np.uint32(0x7F7FFFFF).view(np.float32) - np.uint32(0x7F7F0000).view(np.float32))


def _inputs(g, n):
    """bf16 bits of a random W ~ 0.05 N(0, 1) and a float32 dW of 1e-3 .. 4 bf16 ulp of it, either sign; the
    special sums overwrite a stretch in the middle (rotated by n, so that they meet different residues)."""
    w = (g.standard_normal(n) * 0.05).astype(np.float32)
    wb = (w.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    wf = (wb.astype(np.uint32) << np.uint32(16)).view(np.float32)
    dw = (np.abs(wf) * np.float32(2.0 ** -7) * np.exp(g.uniform(math.log(1e-3), math.log(4.0), n))
          * g.choice([-1.0, 1.0], n)).astype(np.float32)
    if n >= len(SPECIAL):
        at = (n // 2 + n) % (n - len(SPECIAL) + 1)
        for k, (b, d) in enumerate(SPECIAL):
            wb[at + k] = b
            dw[at + k] = (_TOP if b == 0x7F7F else -_TOP) if d is None else d
    return wb, dw


def _check_call(ops, items, seed=SEED):
    """items: (n, W shift in elements, dW shift in floats, elem0, offset).  One merge_group_sr call over all of
    them; every W against the replica (bits where finite, NaN positions) and its canaries."""
    from hdpissa_amd.rounding import sr_merge_bits
    g = np.random.default_rng(len(items) * 1000003 + sum(it[0] for it in items))
    host, dev = [], []
    for n, ws, ds, elem0, offset in items:
        wb, dw = _inputs(g, n)
        buf = np.full(PAD + ws + n + PAD, CANARY, dtype=np.uint16)
        buf[PAD + ws:PAD + ws + n] = wb
        tb = torch.from_numpy(buf.view(np.int16)).to(DEV)
        td = torch.zeros(ds + n + 8, dtype=torch.float32, device=DEV)
        td[ds:ds + n] = torch.from_numpy(dw).to(DEV)
        assert tb.data_ptr() % 16 == 0 and td.data_ptr() % 16 == 0
        W = tb[PAD + ws:PAD + ws + n].view(torch.bfloat16)
        host.append((wb, dw, buf))
        dev.append((tb, W, td[ds:ds + n]))
    ops.merge_group_sr([(W, d, it[3], it[4]) for (_, W, d), it in zip(dev, items)], seed)
    torch.cuda.synchronize()
    for k, ((n, ws, ds, elem0, offset), (wb, dw, buf), (tb, _, _)) in enumerate(zip(items, host, dev)):
        got = tb.cpu().numpy().view(np.uint16)
        assert np.all(got[:PAD + ws] == CANARY), (k, n, "canary before W")
        assert np.all(got[PAD + ws + n:] == CANARY), (k, n, "canary after W")
        want = sr_merge_bits(wb, dw, elem0, seed, offset)
        out = got[PAD + ws:PAD + ws + n]
        nan = (want & 0x7FFF) > 0x7F80
        assert np.array_equal(nan, (out & 0x7FFF) > 0x7F80), (k, n, "NaN positions")
        bad = np.nonzero((out != want) & ~nan)[0]
        assert bad.size == 0, (k, n, ws, ds, elem0, bad[:8], out[bad[:8]], want[bad[:8]])
        if n >= 64:
            assert np.any(out != wb), (k, n, "nothing was merged")


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 43])
def test_kernel_sizes(ops, n):
    _check_call(ops, [(n, 0, 0, 0, (2 << 32) | 9)])


@pytest.mark.parametrize("ws,ds", [(1, 0), (0, 1), (3, 2), (8, 4), (4, 0)], ids=lambda x: str(x))
def test_kernel_misaligned(ops, ws, ds):
    """W or dW off 16 bytes (the element-wise form); (8, 4) is aligned again (the vector form at a shifted base)."""
    _check_call(ops, [(CHUNK + 1, ws, ds, 0, 7), (77, ws, ds, 8, (1 << 32) | 7)])


@pytest.mark.parametrize("elem0", [0, 3, 8, HI - 24, HI - 21], ids=["0", "3", "8", "2^35-24", "2^35-21"])
def test_kernel_elem0(ops, elem0):
    """64 elements from elem0: across 2^35 the block index crosses 2^32; elem0 % 8 != 0 runs element-wise."""
    _check_call(ops, [(64, 0, 0, elem0, (9 << 32) | 0xFFFFFFFF)])
    _check_call(ops, [(CHUNK + 9, 0, 0, elem0, 3)])


@pytest.mark.parametrize("count", [1, 64, 65])
def test_kernel_item_counts(ops, count):
    """1, 64 and 65 items in one call (64 per launch), vector and element-wise items mixed, empty ones between."""
    items = []
    for i in range(count):  # all on the vector path (with and without tails): 65 of them take two launches
        n = [8 * (i % 7) + i % 3 + 1, 16, 2048 + i, CHUNK + 8 * i][i % 4] if count > 1 else 3 * CHUNK + 43
        items.append((n, 0, 0, [0, 8, 4096, HI - 8][(i // 4) % 4], (i << 32) | 5))
    if count > 1:  # and beside them an empty item and two element-wise ones
        items[1:1] = [(0, 0, 0, 0, 1)]
        items += [(CHUNK + 3, 1, 0, 0, (99 << 32) | 5), (333, 0, 0, 3, (98 << 32) | 5)]
    _check_call(ops, items)


def test_kernel_seed_offset_and_type_checks(ops):
    from hdpissa_amd.rounding import sr_merge_bits
    g = np.random.default_rng(1)
    wb, dw = _inputs(g, 4096)
    outs = []
    for seed, offset in ((1, 1), (2, 1), (1, 2), (1, 1)):
        W = torch.from_numpy(wb.view(np.int16).copy()).to(DEV).view(torch.bfloat16)
        ops.merge_group_sr([(W, torch.from_numpy(dw).to(DEV), 0, offset)], seed)
        outs.append(W.view(torch.int16).cpu().numpy().view(np.uint16))
        want = sr_merge_bits(wb, dw, 0, seed, offset)
        fin = (want & 0x7FFF) <= 0x7F80
        assert np.array_equal(outs[-1][fin], want[fin])
    assert np.array_equal(outs[0], outs[3]) and np.any(outs[0] != outs[1]) and np.any(outs[0] != outs[2])
    with pytest.raises(TypeError):
        ops.merge_group_sr([(torch.zeros(8, device=DEV), torch.zeros(8, device=DEV), 0, 0)], 1)
    with pytest.raises(ValueError):
        ops.merge_group_sr([(torch.zeros(8, device=DEV, dtype=torch.bfloat16), torch.zeros(9, device=DEV), 0, 0)], 1)


# ------------------------------------------------------------------------------------------ the step, Wn = 1
SHAPES = [("q_proj", 75, 130), ("o_proj", 128, 192)]
LR = 2e-3


def _model(shapes, dt, seed=5):
    model = nn.Module()
    g = torch.Generator().manual_seed(seed)
    for name, out, inn in shapes:
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_((torch.randn(out, inn, generator=g) * 0.05).bfloat16().float())
        setattr(model, name, lin.to(DEV).to(dt).requires_grad_(False))
    return model


def _grads(L, j, step):
    g = torch.Generator().manual_seed(1000 * step + 10 * j)
    return torch.randn(L.A.shape, generator=g) * 1e-14, torch.randn(L.B.shape, generator=g) * 1e-14


def _set_grads(layers, step):
    for j, L in enumerate(layers):
        gA, gB = _grads(L, j, step)
        L.A.grad, L.B.grad = gA.to(DEV), gB.to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _build(r, **kw):
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    model = _model(SHAPES, torch.bfloat16)
    layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, r, float(r))
    return model, layers, HDPissaStep(model, 1, 0, **kw)


@pytest.mark.parametrize("clip", [None, math.inf], ids=["noclip", "clip-inf"])
@pytest.mark.parametrize("r", [16, 32])
def test_step_equals_replica_on_store_dw(ops, r, clip):
    from helpers import rel_err
    from hdpissa_amd._lib import HDP_DW_STORE, kernel_timing
    from hdpissa_amd.rounding import sr_merge_reference, sr_offset
    kw = {} if clip is None else {"max_grad_norm": clip}
    if r == 32:  # the premise: "nearest" takes the fused Adam-pack at these shapes
        _, _, near = _build(r, **kw)
        assert near._fused_plans(near.plans[0], LR, 1) is not None
    _, layers, st = _build(r, merge_rounding="stochastic", sr_seed=SEED, **kw)
    assert st.sr_seed == SEED and st.plans[0].sr and len(st.plans[0].sr_bufs) == 2
    arena = layers[0]._arena
    for step in (1, 2):
        _set_grads(layers, step)
        before = [L.W_res.clone() for L in layers]
        kernel_timing(enable=True, reset=True)
        try:
            st.step(LR, step)
            torch.cuda.synchronize()
            timing = kernel_timing(enable=False, reset=True)
        finally:
            kernel_timing(enable=False)
        # K3 on its own (not the fused Adam-pack), K4 as a STORE plan, one merge_sr launch for the bucket
        assert timing["adam"]["launches"] == 1 and timing["merge_sr"]["launches"] == 1, timing
        assert "merge" not in timing
        # the same items as a STORE plan of this test's own, on the deltas K3 left in the arena
        items, bufs = [], []
        for it in st._items_w1(arena):
            bufs.append(torch.zeros(it[0] * it[1], dtype=torch.float32, device=DEV))
            items.append(it[:-1] + (bufs[-1],))
        ops.delta_plan(items, HDP_DW_STORE, False).run()
        torch.cuda.synchronize()
        for j, L in enumerate(layers):
            dA, dB = (x.cpu().numpy() for x in arena.views(arena.delta, j))
            A, B = L.A.detach().cpu().numpy(), L.B.detach().cpu().numpy()
            exact = O.delta_w_exact([dA], [dB], [A], [B])
            err = rel_err(bufs[j].cpu().numpy().reshape(exact.shape), exact)
            print(f"r={r} clip={clip} step {step} module {j}: STORE dW rel err {err:.3e}")
            assert err < 1e-5, (step, j, err)
            want = sr_merge_reference(before[j], bufs[j].view_as(L.W_res), 0, SEED, sr_offset(j, step))
            assert np.array_equal(_bits(L.W_res), _bits(want)), (step, j, float(np.mean(_bits(L.W_res) != _bits(want))))
            assert not torch.equal(L.W_res, before[j])
    if clip is not None:
        assert st.clip_info()["coef"] == 1.0


def test_step_seeds():
    res = []
    for seed in (11, 12, 11):
        _, layers, st = _build(16, merge_rounding="stochastic", sr_seed=seed)
        for step in (1, 2):
            _set_grads(layers, step)
            st.step(LR, step)
        torch.cuda.synchronize()
        res.append([L.W_res.clone() for L in layers])
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[2]))
    assert all(not torch.equal(a, b) for a, b in zip(res[0], res[1]))


def test_default_seed_and_functional_cache():
    """sr_seed=None derives the seed from torch.initial_seed(); hd_pissa_step's stepper cache keys on both arguments."""
    from hdpissa_amd import hd_pissa_step, replace_with_custom_layer
    from hdpissa_amd.rounding import SR_SEED_OFFSET
    model = _model(SHAPES, torch.bfloat16)
    layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, 16, 16.0)
    _set_grads(layers, 1)
    a = hd_pissa_step(model, LR, 1, 1)
    assert a.merge_rounding == "nearest" and a.sr_seed is None
    _set_grads(layers, 2)
    b = hd_pissa_step(model, LR, 2, 1, merge_rounding="stochastic")
    assert b is not a and b.sr_seed == (torch.initial_seed() + SR_SEED_OFFSET) % 2 ** 64
    _set_grads(layers, 3)
    assert hd_pissa_step(model, LR, 3, 1, merge_rounding="stochastic") is b
    _set_grads(layers, 4)
    c = hd_pissa_step(model, LR, 4, 1, merge_rounding="stochastic", sr_seed=5)
    assert c is not b and c.sr_seed == 5
    with pytest.raises(ValueError):
        hd_pissa_step(model, LR, 5, 1, merge_rounding="up")


# ------------------------------------------------------------------------------------------ the reason for it
def test_stochastic_rounding_keeps_the_update():
    """One bf16 layer 128 x 192, r 16, lr 5e-5, the same gradients before each of 128 steps.  error = ||W - (W0 +
    sum dW)|| / ||sum dW||, sum dW from a float32-W copy of the layer on the same factors.  Required:
    error(nearest) >= 0.8 and error(stochastic) <= 0.5 error(nearest).  The CPU simulation of these inputs
    (replica + oracle op set, seed 20240607) gave 0.900 and 0.229 (ratio 0.254); measured on the MI355X: 0.8966 and
    0.2243 (ratio 0.250)."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    lr, steps, shapes = 5e-5, 128, [("q_proj", 128, 192)]

    def build(dt, **kw):
        model = _model(shapes, dt)
        (L,) = replace_with_custom_layer(model, ["q_proj"], 0, 1, 16, 16.0)
        return L, (lambda: HDPissaStep(model, 1, 0, **kw))

    def run(L, st):
        g = torch.Generator().manual_seed(77)
        gA, gB = (torch.randn(s, generator=g) * 1e-14 for s in (L.A.shape, L.B.shape))
        for t in range(1, steps + 1):
            L.A.grad, L.B.grad = gA.to(DEV), gB.to(DEV)
            st.step(lr, t)
        torch.cuda.synchronize()
        return L.W_res.float().cpu().numpy().astype(np.float64)

    Lf, mk = build(torch.float32)
    W0 = Lf.W_res.float().cpu().numpy().astype(np.float64)
    Wf = run(Lf, mk())
    total = np.linalg.norm(Wf - W0)
    err = {}
    for mode, kw in (("nearest", {}), ("stochastic", dict(merge_rounding="stochastic", sr_seed=20240607))):
        L, mk = build(torch.bfloat16, **kw)
        with torch.no_grad():
            L._arena.fac_all.copy_(Lf._arena.fac_all)  # the very same factors
        assert np.array_equal(L.W_res.float().cpu().numpy().astype(np.float64), W0)
        err[mode] = float(np.linalg.norm(run(L, mk()) - Wf) / total)
    print(f"128 steps at lr 5e-5: error nearest {err['nearest']:.4f} stochastic {err['stochastic']:.4f} "
          f"ratio {err['stochastic'] / err['nearest']:.4f}")
    assert err["nearest"] >= 0.8, err
    assert err["stochastic"] <= 0.5 * err["nearest"], err


# ------------------------------------------------------------------------------------------ resume
def test_resume_continues_the_rounding_stream(tmp_path):
    from hdpissa_amd import load_hdpissa_state, save_hdpissa_state
    kw = dict(merge_rounding="stochastic", sr_seed=SEED)
    _, la, sa = _build(16, **kw)
    for step in (1, 2, 3):
        _set_grads(la, step)
        sa.step(LR, step)
    mb, lb, sb = _build(16, **kw)
    for step in (1, 2):
        _set_grads(lb, step)
        sb.step(LR, step)
    path = str(tmp_path / "state.safetensors")
    save_hdpissa_state(mb, path, t=2)
    mc, lc, sc = _build(16, **kw)
    t = load_hdpissa_state(mc, path)
    assert t == 2
    _set_grads(lc, t + 1)
    sc.step(LR, t + 1)
    torch.cuda.synchronize()
    for a, c in zip(la, lc):
        assert torch.equal(a.W_res, c.W_res)
    assert torch.equal(la[0]._arena.m, lc[0]._arena.m) and torch.equal(la[0]._arena.v, lc[0]._arena.v)
    _, ld, sd = _build(16, merge_rounding="stochastic", sr_seed=SEED + 1)  # (another seed would not)
    for step in (1, 2, 3):
        _set_grads(ld, step)
        sd.step(LR, step)
    assert not torch.equal(la[0].W_res, ld[0].W_res)


# ------------------------------------------------------------------------------------------ ranks on one GPU
# the shapes and bucket bounds of tests/test_gpu_ranks_shard.py: a short block and a rank with no rows at Wn = 8,
# rows of 250 elements, four W buckets
RSHAPES = [("q_proj", 256, 192), ("k_proj", 128, 192), ("o_proj", 200, 320), ("up_proj", 384, 250)]
W_BUCKET_BYTES = 100_000
MAX_DIFF_SHARE = 1e-3     # share of elements off the replica on the exact dW (each by at most one bf16 ulp)


class HostComm:
    """torch.distributed (gloo) on host copies of the device buffers -- TEST ONLY (the ranks share the GPU)."""
    name = "host-gloo"

    def __init__(self, rank, world_size):
        self.rank, self.world_size = rank, world_size

    def allgather(self, send, recv):
        self.allgather_any(send, recv)

    def broadcast(self, t, root):
        h = t.cpu()
        dist.broadcast(h, src=root)
        t.copy_(h.to(t.device))

    def allgather_any(self, send, recv):
        s8 = send.reshape(-1).view(torch.uint8).cpu()  # (gloo has no bf16 gather: move the bytes)
        outs = [torch.empty_like(s8) for _ in range(self.world_size)]
        dist.all_gather(outs, s8)
        recv.view(torch.uint8).copy_(torch.cat(outs).to(recv.device))


def _ordered(bits):
    """bf16 bit patterns -> integers ordered like the values (adjacent values differ by 1)."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def _worker(rank, wn, port, math_, errfile):
    import sys
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HDP_K4_MATH"] = math_  # before the library loads
    torch.set_num_threads(2 if wn <= 2 else 1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from hdpissa_amd.rounding import sr_merge_bits, sr_offset
        from shard_helpers import OracleRanks, seeded_grads
        dev, dt, r, lr = torch.device("cuda:0"), torch.bfloat16, 16, 2e-3
        comm = HostComm(rank, wn)

        def build():
            model = nn.Module()
            g = torch.Generator().manual_seed(5)  # the same base weights on every rank and in both copies
            for name, out, inn in RSHAPES:
                lin = nn.Linear(inn, out, bias=False)
                with torch.no_grad():
                    lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
                setattr(model, name, lin.to(dev).to(dt).requires_grad_(False))
            return model, replace_with_custom_layer(model, [s[0] for s in RSHAPES], rank, wn, r, 16.0, comm=comm)

        (ms, ls), (mg, lg) = build(), build()
        with torch.no_grad():  # both copies on the very same factors
            lg[0]._arena.fac_all.copy_(ls[0]._arena.fac_all)
        kw = dict(merge_rounding="stochastic", sr_seed=SEED)
        ss = HDPissaStep(ms, wn, rank, comm=comm, exchange="shard", bucket_bytes=W_BUCKET_BYTES, **kw)
        sg = HDPissaStep(mg, wn, rank, comm=comm, exchange="gather", bucket_bytes=40_000, **kw)
        assert len(ss.plans[0].s_buckets) >= 3
        ref = OracleRanks(ls, wn, r, dt, lr)  # (its deltas only: the oracle's Adam for every rank)
        worst = dict(shard=0.0, gather=0.0)
        for step in (1, 2):
            for layers in (ls, lg):
                for j, L in enumerate(layers):
                    gA, gB = seeded_grads(L, j, rank, step)
                    L.A.grad, L.B.grad = gA.to(dev), gB.to(dev)
            prev = {"shard": [L.W_res.clone() for L in ls], "gather": [L.W_res.clone() for L in lg]}
            ss.step(lr, step)
            sg.step(lr, step)
            torch.cuda.synchronize()
            for name, layers in (("shard", ls), ("gather", lg)):
                for j, L in enumerate(layers):  # bitwise identical on all ranks, after every step
                    w = L.W_res.float().cpu()
                    allw = [torch.zeros_like(w) for _ in range(wn)]
                    dist.all_gather(allw, w)
                    assert all(torch.equal(allw[0], x) for x in allw), f"{name} step {step} module {j}: ranks differ"
            if math_ == "x3":
                for j, (a, b) in enumerate(zip(ls, lg)):
                    assert torch.equal(a.W_res, b.W_res), (step, j, float((a.W_res != b.W_res).float().mean()))
            for j, (L, (dA, dB)) in enumerate(zip(ls, ref.deltas(step))):
                fa = L._arena.fac_all
                A = [fa[i][L._oa:L._oa + r * L.in_features].view(r, -1).cpu().numpy() for i in range(wn)]
                B = [fa[i][L._ob:L._ob + L.out_features * r].view(-1, r).cpu().numpy() for i in range(wn)]
                exact = O.delta_w_exact(dA, dB, A, B).astype(np.float32)
                for name, M in (("shard", L), ("gather", lg[j])):
                    pb = prev[name][j].view(torch.int16).cpu().numpy().view(np.uint16)
                    want = _ordered(sr_merge_bits(pb, exact, 0, SEED, sr_offset(j, step)))
                    got = _ordered(M.W_res.view(torch.int16).cpu().numpy().view(np.uint16))
                    d = np.abs(got - want)
                    share = float(np.mean(d != 0))
                    worst[name] = max(worst[name], share)
                    assert d.max() <= 1, (name, step, j, int(d.max()))
                    assert share <= MAX_DIFF_SHARE, (name, step, j, share)
                assert not torch.equal(L.W_res, prev["shard"][j])
        if rank == 0:
            print(f"FIGURES wn={wn} {math_}: share of elements off the replica on the exact dW: {worst}", flush=True)
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("wn,math_", [(2, "auto"), (8, "auto"), (2, "x3"), (8, "x3")])
def test_ranks_on_one_gpu(wn, math_, tmp_path):
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(_worker, args=(wn, _port(), math_, errfile), nprocs=wn, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")
