"""exchange="shard" under gloo on CPU: the worker of test_dist_gloo.py over the same eight fixture cases at
the same bars, with the cross-rank bitwise check in BOTH dtypes (every element of W is computed by one
rank and copied to the others), plus a four-module model whose W bucket cap gives four W buckets, so that
both double buffers are reused.  (The fixtures hold at most two modules, hence at most two W buckets:
the many-bucket case builds its own model and is held to the oracle's rank loop.)
"""
import glob
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HERE = os.path.dirname(os.path.abspath(__file__))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(rank, wn, port):
    import sys
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)


def _same_on_all_ranks(layers, wn):
    for L in layers:
        w = L.W_res.float().clone()
        ws = [torch.zeros_like(w) for _ in range(wn)]
        dist.all_gather(ws, w)
        assert all(torch.equal(ws[0], x) for x in ws), "ranks hold different merged weights"


def _worker(rank, wn, port, path, errfile):
    _setup(rank, wn, port)
    try:
        from cpu_ops import CpuOps
        from helpers import build_fixture_model, rel_err
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from hdpissa_amd.comm import TorchComm

        z = np.load(path)
        case = os.path.basename(path)[5:-7]
        model, table, targets, dt = build_fixture_model(z, case)
        ops = CpuOps(table)
        comm = TorchComm(rank, wn)
        layers = replace_with_custom_layer(model, targets, rank, wn, int(z["r"]), float(z["alpha"]), comm=comm,
                                           ops=ops)
        st = HDPissaStep(model, wn, rank, comm=comm, ops=ops, exchange="shard", bucket_bytes=2048)
        for s in range(int(z["n_steps"])):
            for j, L in enumerate(layers):
                L.A.grad = torch.from_numpy(z[f"r{rank}.s{s}.{j}.gA"])
                L.B.grad = torch.from_numpy(z[f"r{rank}.s{s}.{j}.gB"])
            st.step(float(z[f"r0.s{s}.lr"]), int(z[f"r0.s{s}.t"]))
            _same_on_all_ranks(layers, wn)  # after every step, both dtypes
            for j, L in enumerate(layers):
                W_ref = z[f"r{rank}.s{s}.{j}.W"]
                W_prev = z[f"r{rank}.{j}.W0"] if s == 0 else z[f"r{rank}.s{s - 1}.{j}.W"]
                got = L.W_res.float().numpy()
                err = rel_err(got, W_ref)
                assert err < (2e-2 if dt == torch.bfloat16 else 1e-6), (s, j, err)
                upd = rel_err(got - W_prev, W_ref - W_prev)
                if dt == torch.float32:
                    assert upd < 1e-4, (s, j, upd)
                else:
                    assert upd < 2e-2 and np.mean(got != W_ref) < 0.02, (s, j, upd, float(np.mean(got != W_ref)))
                for k in ("m_A", "v_A", "m_B", "v_B"):
                    assert rel_err(getattr(L, k).numpy(), z[f"r{rank}.s{s}.{j}.{k}_out"]) < 1e-6
                with torch.no_grad():
                    L.W_res.copy_(torch.from_numpy(W_ref).to(dt))
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


CASES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "step_*_w2.npz")))] + \
        [os.path.join(GOLDEN, "step_f32_two_w4.npz"), os.path.join(GOLDEN, "step_bf16_tall_w4.npz"),
         os.path.join(GOLDEN, "step_bf16_tall_w8.npz"), os.path.join(GOLDEN, "step_f32_tall_w8.npz")]


def _spawn(fn, args, wn, tmp_path):
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(fn, args=(wn, _port()) + args + (errfile,), nprocs=wn, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p) for p in CASES])
def test_multirank_gloo_shard(path, tmp_path):
    _spawn(_worker, (path,), int(np.load(path)["world_size"]), tmp_path)


# -- four W buckets: both send / gather buffers are used twice ---------------------------------------
# out = 20 at Wn = 4: blocks of 8 rows, so rank 2 owns 4 rows and rank 3 none
SHAPES = [("q_proj", 48, 40), ("k_proj", 20, 40), ("o_proj", 64, 24), ("up_proj", 40, 56)]


def _worker_buckets(rank, wn, port, dtname, errfile):
    _setup(rank, wn, port)
    try:
        import torch.nn as nn
        from cpu_ops import CpuOps
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from hdpissa_amd.comm import TorchComm
        from shard_helpers import OracleRanks, seeded_grads

        dt = getattr(torch, dtname)
        r, lr = 4, 2e-3
        model = nn.Module()
        g = torch.Generator().manual_seed(5)  # the same base weights on every rank
        for name, out, inn in SHAPES:
            lin = nn.Linear(inn, out, bias=False)
            with torch.no_grad():
                lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
            setattr(model, name, lin.to(dt).requires_grad_(False))
        comm, ops = TorchComm(rank, wn), CpuOps()
        layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], rank, wn, r, 16.0, comm=comm, ops=ops)
        st = HDPissaStep(model, wn, rank, comm=comm, ops=ops, exchange="shard", bucket_bytes=1024)
        assert len(st.plans[0].s_buckets) == 4  # every module above 1024 B of W: one bucket each
        ref = OracleRanks(layers, wn, r, dt, lr)
        for step in (1, 2):
            for j, L in enumerate(layers):
                L.A.grad, L.B.grad = seeded_grads(L, j, rank, step)
            st.step(lr, step)
            _same_on_all_ranks(layers, wn)
            ref.check(step, ref.deltas(step), [L.W_res.float() for L in layers])
    except Exception as e:
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtname", ["float32", "bfloat16"])
def test_gloo_shard_reuses_double_buffers(dtname, tmp_path):
    _spawn(_worker_buckets, (dtname,), 4, tmp_path)
