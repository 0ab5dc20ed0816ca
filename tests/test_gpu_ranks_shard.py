"""exchange="shard" with ranks as processes on the one GPU (2 and 8): the whole multi-rank path on real kernels.

As tests/test_gpu_ranks_one_gpu.py: RCCL refuses two ranks on one device, so the transport is gloo on host
copies (HostComm below, test-only); the sharded K1 init, K3, the side-stream delta all-gather, the row-block K4
plans, the grouped-copy pack and scatter and the double-buffered W buckets (four here) are the production
path.  In the same worker a second copy of the model takes the same gradients through exchange="gather".

Per step: the oracle's rank loop at the gather exchange's bars (float32 merged W 1e-5, update 1e-4; bf16
update 2e-2 with < 2 % of elements differing), W bitwise identical on all ranks (both dtypes, every math),
and, where HDP_K4_MATH pins an exact math (x3, f32), shard == gather bit for bit.

Measured (MI355X), worst over modules and steps -- see DESIGN section 3.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# o_proj 200 rows at Wn = 8: a short block and a rank with no rows; up_proj rows of 250 elements
SHAPES = [("q_proj", 256, 192), ("k_proj", 128, 192), ("o_proj", 200, 320), ("up_proj", 384, 250)]
W_BUCKET_BYTES = 100_000  # four W buckets in either dtype: both buffer pairs are reused


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


def _worker(rank, wn, port, dtname, math, errfile):
    import sys
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["HDP_K4_MATH"] = math  # before the library loads
    torch.set_num_threads(2 if wn <= 2 else 1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        import torch.nn as nn
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from shard_helpers import OracleRanks, seeded_grads
        dev = torch.device("cuda:0")
        dt = getattr(torch, dtname)
        r, lr = 16, 2e-3
        comm = HostComm(rank, wn)

        def build():
            model = nn.Module()
            g = torch.Generator().manual_seed(5)  # the same base weights on every rank and in both copies
            for name, out, inn in SHAPES:
                lin = nn.Linear(inn, out, bias=False)
                with torch.no_grad():
                    lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
                setattr(model, name, lin.to(dev).to(dt).requires_grad_(False))
            return model, replace_with_custom_layer(model, [s[0] for s in SHAPES], rank, wn, r, 16.0, comm=comm)

        (ms, ls), (mg, lg) = build(), build()
        with torch.no_grad():  # both copies on the very same factors: what follows compares the exchanges alone
            lg[0]._arena.fac_all.copy_(ls[0]._arena.fac_all)
        ss = HDPissaStep(ms, wn, rank, comm=comm, exchange="shard", bucket_bytes=W_BUCKET_BYTES)
        sg = HDPissaStep(mg, wn, rank, comm=comm, exchange="gather", bucket_bytes=40_000)
        assert len(ss.plans[0].s_buckets) >= 3
        refs, refg = OracleRanks(ls, wn, r, dt, lr), OracleRanks(lg, wn, r, dt, lr)
        for step in (1, 2):
            for layers in (ls, lg):
                for j, L in enumerate(layers):
                    gA, gB = seeded_grads(L, j, rank, step)
                    L.A.grad, L.B.grad = gA.to(dev), gB.to(dev)
            ss.step(lr, step)
            sg.step(lr, step)
            torch.cuda.synchronize()
            Ws, Wg = [L.W_res.float().cpu() for L in ls], [L.W_res.float().cpu() for L in lg]
            for j, w in enumerate(Ws):  # bitwise identical on all ranks, after every step
                allw = [torch.zeros_like(w) for _ in range(wn)]
                dist.all_gather(allw, w)
                assert all(torch.equal(allw[0], x) for x in allw), f"step {step} module {j}: ranks differ"
            if math in ("x3", "f32"):
                for j, (a, b) in enumerate(zip(Ws, Wg)):
                    assert torch.equal(a, b), (step, j, float((a != b).float().mean()))
            refs.check(step, refs.deltas(step), Ws)
            refg.check(step, refg.deltas(step), Wg)
        if rank == 0:
            print(f"FIGURES wn={wn} {dtname} {math}: shard {refs.figures} gather {refg.figures}", flush=True)
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


CASES = [(2, "float32", "auto"), (8, "bfloat16", "auto"), (8, "float32", "x3"), (2, "bfloat16", "x3"),
         (8, "bfloat16", "f32")]


@pytest.mark.parametrize("wn,dtname,math", CASES)
def test_ranks_shard(wn, dtname, math, tmp_path):
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(_worker, args=(wn, _port(), dtname, math, errfile), nprocs=wn, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")
