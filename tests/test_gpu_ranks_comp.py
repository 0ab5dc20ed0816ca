"""merge_rounding="compensated" with ranks as processes on the one GPU (the host transport of
tests/test_gpu_ranks_one_gpu.py: gloo on host copies, test-only): a bf16 four-module model, r 16, two steps, the
K4 math pinned to x3 (HDP_K4_MATH=x3: an exact math, so a row block has the whole module's bits).  Under
exchange="shard" and exchange="gather", after every step:

* W_res and W_c are bitwise equal on all ranks (shard: the bucket's pack, all-gather and scatter carry the W_c
  rows beside the W rows);
* they are bitwise equal between the two exchanges.

Each rank is a child process of its own under its own time limit; a non-zero child status fails the test and
nothing further is started.  This file is also the child's program (``python test_gpu_ranks_comp.py rank wn port``).
"""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# the shapes and bucket bounds of tests/test_gpu_ranks_shard.py: a short block, rows of 250 elements, four W buckets
RSHAPES = [("q_proj", 256, 192), ("k_proj", 128, 192), ("o_proj", 200, 320), ("up_proj", 384, 250)]
W_BUCKET_BYTES = 100_000
CHILD_SECONDS = 150


def _child(rank, wn, port):
    for p in (HERE, ROOT, os.path.join(ROOT, "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch
    import torch.distributed as dist
    import torch.nn as nn
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    assert os.environ.get("HDP_K4_MATH") == "x3"  # (read when the library first plans a K4)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from shard_helpers import seeded_grads
        from test_gpu_ranks_one_gpu import HostComm
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
        ss = HDPissaStep(ms, wn, rank, comm=comm, exchange="shard", bucket_bytes=W_BUCKET_BYTES, merge_rounding="compensated")
        sg = HDPissaStep(mg, wn, rank, comm=comm, exchange="gather", bucket_bytes=40_000, merge_rounding="compensated")
        assert len(ss.plans[0].s_buckets) >= 3 and ss.plans[0].comp and sg.plans[0].comp
        for step in (1, 2):
            for layers in (ls, lg):
                for j, L in enumerate(layers):
                    gA, gB = seeded_grads(L, j, rank, step)
                    L.A.grad, L.B.grad = gA.to(dev), gB.to(dev)
            prev = [L.W_res.clone() for L in ls]
            ss.step(lr, step)
            sg.step(lr, step)
            torch.cuda.synchronize()
            for name, layers in (("shard", ls), ("gather", lg)):
                for j, L in enumerate(layers):  # bitwise identical on all ranks, after every step
                    for what, t in (("W_res", L.W_res), ("W_c", L.W_c)):
                        x = t.view(torch.int16).to(torch.int32).cpu()
                        xs = [torch.zeros_like(x) for _ in range(wn)]
                        dist.all_gather(xs, x)
                        assert all(torch.equal(xs[0], y) for y in xs), f"{name} step {step} module {j}: {what} differs across ranks"
            for j, (a, b) in enumerate(zip(ls, lg)):  # and between the exchanges
                assert torch.equal(a.W_res.view(torch.int16), b.W_res.view(torch.int16)), \
                    (step, j, "W_res", float((a.W_res != b.W_res).float().mean()))
                assert torch.equal(a.W_c.view(torch.int16), b.W_c.view(torch.int16)), \
                    (step, j, "W_c", float((a.W_c != b.W_c).float().mean()))
                assert not torch.equal(a.W_res, prev[j]) and bool(a.W_c.any())
                rows = np.flatnonzero(a.W_c.float().abs().sum(dim=1).cpu().numpy())
                assert rows.size > 0.9 * a.out_features, (step, j, "rows of W_c left at zero", rows.size)
    finally:
        dist.destroy_process_group()


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_ranks_shard_and_gather_bitwise_equal(tmp_path):
    wn, port = 2, _port()
    env = dict(os.environ, HDP_K4_MATH="x3")
    logs = [open(str(tmp_path / f"rank{k}.log"), "w+") for k in range(wn)]
    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), str(k), str(wn), str(port)], env=env, cwd=ROOT,
                             stdout=logs[k], stderr=subprocess.STDOUT) for k in range(wn)]
    status = []
    try:
        for p in kids:  # each child under its own time limit; the first bad status ends the test
            try:
                status.append(p.wait(timeout=CHILD_SECONDS))
            except subprocess.TimeoutExpired:
                status.append("time limit")
            if status[-1] != 0:
                break
    finally:
        for p in kids:
            if p.poll() is None:
                p.kill()
                p.wait()
    out = []
    for k, f in enumerate(logs):
        f.seek(0)
        out.append(f"--- rank {k}\n" + f.read()[-4000:])
        f.close()
    assert status == [0] * wn, f"child status {status}\n" + "\n".join(out)


if __name__ == "__main__":
    _child(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
