"""Gradient-norm clipping with two ranks as processes on the one GPU: the global norm and the joint skip.

The pattern of tests/test_gpu_ranks_one_gpu.py (gloo on host copies of the device buffers, HostComm, test-only;
everything else the production path): per-rank gradients, then HDPissaStep.step with max_grad_norm -- one
grad_sumsq per arena, the all-gather of the per-arena sums, clip_finish, the clipped K3 and the exchange.

Both ranks must hold the same bits of sumsq, norm and coef; sumsq is the float64 sum over BOTH ranks'
regenerated gradients (within n 2^-52); each rank's m and v equal clip_ref.adam_factors_clip bit for bit; W is
bitwise identical on both ranks and within the bars of test_gpu_ranks_one_gpu.py against the oracle's rank
loop on the helper's deltas; and one inf in rank 1's gradient makes both ranks skip, W unchanged.
"""
import math
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
JOIN_SECONDS = 120


def _worker(rank, wn, port, dtname, exchange, errfile):
    import sys
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        import torch.nn as nn

        import clip_ref as R
        from helpers import rel_err
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from oracle import hdpissa_oracle as O
        from test_gpu_ranks_one_gpu import SHAPES, HostComm, _grads
        dev = torch.device("cuda:0")
        dt = getattr(torch, dtname)
        r, lr = 16, 2e-3
        model = nn.Module()
        g = torch.Generator().manual_seed(5)  # the same base weights on both ranks
        for name, out, inn in SHAPES:
            lin = nn.Linear(inn, out, bias=False)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
            setattr(model, name, lin.to(dev).to(dt).requires_grad_(False))
        comm = HostComm(rank, wn)
        layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], rank, wn, r, 16.0, comm=comm)
        ar = layers[0]._arena

        def total(step):  # float64 sum of squares over every rank's regenerated gradients
            return sum(R.sumsq(x.numpy()) for i in range(wn) for j, L in enumerate(layers) for x in _grads(L, j, i, step))

        c = 0.5 * math.sqrt(total(1))  # both steps clip (the seeded gradients have one scale)
        st = HDPissaStep(model, wn, rank, comm=comm, exchange=exchange, bucket_bytes=40_000, max_grad_norm=c)
        zeros = lambda L: [np.zeros(L.A.shape, np.float32), np.zeros(L.B.shape, np.float32)]  # noqa: E731
        mv = {(i, j): (zeros(L), zeros(L)) for i in range(wn) for j, L in enumerate(layers)}
        Wref = [L.W_res.float().cpu().numpy() for L in layers]
        if dt == torch.float32:
            Wref = [w.astype(np.float64) for w in Wref]

        def same_on_all_ranks(t, what):
            h = t.cpu()
            alls = [torch.zeros_like(h) for _ in range(wn)]
            dist.all_gather(alls, h)
            assert all(torch.equal(alls[0], x) for x in alls), f"ranks differ: {what}"

        for step in (1, 2, 3):
            for j, L in enumerate(layers):
                gA, gB = _grads(L, j, rank, step)
                if step == 3 and rank == 1 and j == 2:
                    gA[3, 5] = math.inf  # only rank 1 has a non-finite gradient: every rank must skip
                L.A.grad, L.B.grad = gA.to(dev), gB.to(dev)
            m0, v0, W0 = ar.m.clone(), ar.v.clone(), [L.W_res.clone() for L in layers]
            st.step(lr, step)
            torch.cuda.synchronize()
            info = st.clip_info()
            same_on_all_ranks(st.clip_state, "the clip record")  # sumsq, norm, coef, skip: the same bits
            for j, L in enumerate(layers):
                same_on_all_ranks(L.W_res.float(), f"W of module {j}")
            if step == 3:
                assert info["skipped"] and info["skipped_total"] == 1
                assert torch.equal(ar.m, m0) and torch.equal(ar.v, v0) and not torch.any(ar.delta)
                assert all(torch.equal(L.W_res, w) for L, w in zip(layers, W0)) and not torch.any(ar.grad)
                continue
            ss = total(step)
            assert abs(info["sumsq"] - ss) <= ss * R.sumsq_bound(wn * ar.F), (info["sumsq"], ss)
            assert np.float32(info["norm"]) == R.norm_of(info["sumsq"])
            assert np.float32(info["coef"]) == R.coef_of(info["norm"], c) and info["coef"] < 1.0 and not info["skipped"]
            for j, L in enumerate(layers):
                fa = L._arena.fac_all
                A = [fa[i][L._oa:L._oa + r * L.in_features].view(r, -1).cpu().numpy() for i in range(wn)]
                B = [fa[i][L._ob:L._ob + L.out_features * r].view(-1, r).cpu().numpy() for i in range(wn)]
                dA, dB = [], []
                for i in range(wn):
                    gA, gB = (x.numpy() for x in _grads(L, j, i, step))
                    (mA, mB), (vA, vB) = mv[(i, j)]
                    mA, vA, da = R.adam_factors_clip(gA, mA, vA, step, lr, info["coef"])
                    mB, vB, db = R.adam_factors_clip(gB, mB, vB, step, lr, info["coef"])
                    mv[(i, j)] = ([mA, mB], [vA, vB])
                    dA.append(da)
                    dB.append(db)
                (mA, mB), (vA, vB) = mv[(rank, j)]
                for got, ref in ((L.m_A, mA), (L.v_A, vA), (L.m_B, mB), (L.v_B, vB)):
                    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (step, j)
                got = L.W_res.float().cpu().numpy()
                if dt == torch.float32:
                    exact = O.delta_w_exact(dA, dB, A, B)
                    prev = Wref[j]
                    assert rel_err(got, prev + exact) < 1e-5, (step, j, rel_err(got, prev + exact))
                    assert rel_err(got - prev, exact) < 1e-4, (step, j, rel_err(got - prev, exact))
                    Wref[j] = got.astype(np.float64)
                else:
                    ref = O.merge(Wref[j], O.delta_w(dA, dB, A, B, "bfloat16"), "bfloat16")
                    upd = rel_err(got - Wref[j], ref - Wref[j])
                    diff = float(np.mean(got != ref))
                    assert upd < 2e-2 and diff < 0.02, (step, j, upd, diff)
                    Wref[j] = got
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


@pytest.mark.parametrize("dtname,exchange", [("float32", "gather"), ("bfloat16", "shard")])
def test_two_ranks_clip(dtname, exchange, tmp_path):
    """Two processes only; joined under a time limit, not retried."""
    errfile = str(tmp_path / "err.txt")
    ctx = mp.spawn(_worker, args=(2, _port(), dtname, exchange, errfile), nprocs=2, join=False)
    deadline = time.monotonic() + JOIN_SECONDS
    try:
        while not ctx.join(timeout=max(0.1, min(5.0, deadline - time.monotonic()))):
            if time.monotonic() > deadline:
                for p in ctx.processes:
                    if p.is_alive():
                        p.kill()
                pytest.fail(f"workers still running after {JOIN_SECONDS} s")
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")
