"""Gradient-norm clipping and the non-finite-step skip: the host logic of HDPissaStep / HDPissaTrainer on
CPU, with a CPU stand-in of the three device operations (``ClipCpuOps``: torch float64 / float32 on the
host, the arithmetic of clip_ref).  What the kernels themselves compute is tests/test_gpu_clip.py's.
"""
import math
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import clip_ref as R
from cpu_ops import CpuOps
from oracle import hdpissa_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [("q_proj", 48, 40), ("k_proj", 20, 40), ("o_proj", 64, 24), ("up_proj", 40, 56)]


class ClipCpuOps(CpuOps):
    """CpuOps + grad_sumsq / clip_finish / adam(clip=) -- TEST INFRASTRUCTURE ONLY."""

    def __init__(self, factors=None):
        super().__init__(factors)
        self.log = []  # (op, arena grad data_ptr) in call order

    def grad_sumsq(self, grad, out, grad_scale=1e16):
        self.log.append(("sumsq", grad.data_ptr()))
        gs = (grad.reshape(-1) * torch.tensor(grad_scale, dtype=torch.float32)).double()
        out[0] = (gs * gs).sum()

    def clip_finish(self, sums, max_norm, state):
        from hdpissa_amd._lib import ClipState, clip_record
        self.log.append(("finish", 0))
        prev = clip_record(state.numpy().tobytes())["skipped_total"]
        rec = R.clip_record(sums.numpy(), max_norm, prev)
        s = ClipState(sumsq=rec["sumsq"], norm=rec["norm"], coef=rec["coef"], skip=int(rec["skipped"]),
                      skipped_total=rec["skipped_total"])
        state.copy_(torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8))

    def adam(self, grad, m, v, delta, t, lr, beta1, beta2, eps, zero_grad, grad_scale=1e16, clip=None):
        self.log.append(("adam", grad.data_ptr()))
        if clip is None:
            return super().adam(grad, m, v, delta, t, lr, beta1, beta2, eps, zero_grad, grad_scale)
        from hdpissa_amd._lib import clip_record
        rec = clip_record(clip.numpy().tobytes())
        if rec["skipped"]:
            delta.zero_()
        else:
            mn, vn, d = R.adam_factors_clip(grad.numpy(), m.numpy(), v.numpy(), t, lr, rec["coef"], beta1, beta2, eps,
                                            grad_scale)
            m.copy_(torch.from_numpy(mn))
            v.copy_(torch.from_numpy(vn))
            delta.copy_(torch.from_numpy(d))
        if zero_grad:
            grad.zero_()


def _model(names_shapes, dt=torch.float32, seed=5):
    model = nn.Module()
    g = torch.Generator().manual_seed(seed)
    for name, out, inn in names_shapes:
        lin = nn.Linear(inn, out, bias=False)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
        setattr(model, name, lin.to(dt).requires_grad_(False))
    return model


def _grads(L, j, rank, step, scale=1e-14):
    g = torch.Generator().manual_seed(1000 * step + 10 * j + rank)
    return torch.randn(L.A.shape, generator=g) * scale, torch.randn(L.B.shape, generator=g) * scale


def _sumsq_layers(layers, rank, step):
    return sum(R.sumsq(x.numpy()) for j, L in enumerate(layers) for x in _grads(L, j, rank, step))


# -- the helper ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 7])
def test_helper_equals_oracle_at_coef_one(t):
    g = np.random.default_rng(t)
    raw = (g.standard_normal(4099) * 1e-14).astype(np.float32)
    m = (g.standard_normal(4099) * 0.3).astype(np.float32) if t > 1 else np.zeros(4099, np.float32)
    v = (g.random(4099) * 0.2).astype(np.float32) if t > 1 else np.zeros(4099, np.float32)
    ref = O.adam_factors(raw, m, v, t, 2e-3)
    got = R.adam_factors_clip(raw, m, v, t, 2e-3, 1.0)
    for a, b in zip(got, ref):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    clipped = R.adam_factors_clip(raw, m, v, t, 2e-3, 0.25)
    assert not np.array_equal(clipped[0], ref[0]) and not np.array_equal(clipped[1], ref[1])


def test_record_arithmetic():
    rec = R.clip_record([9.0, 16.0], 1.0)
    assert rec["norm"] == 5.0 and rec["coef"] == float(np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6)))
    assert R.clip_record([9.0, 16.0], 6.0)["coef"] == 1.0 and R.clip_record([25.0], math.inf)["coef"] == 1.0
    for bad in (math.inf, math.nan):
        rec = R.clip_record([1.0, bad], 1.0, skipped_total=3)
        assert rec["skipped"] and rec["skipped_total"] == 4 and rec["coef"] == 1.0
    assert R.clip_record([], 1.0) == {"sumsq": 0.0, "norm": 0.0, "coef": 1.0, "skipped": False, "skipped_total": 0}


def test_argument_validation_without_gpu():
    """The new entry points validate before any HIP call (as tests/test_abi.py checks for the old ones)."""
    import ctypes
    from hdpissa_amd._lib import LIB_PATH, ClipState, lib
    if not os.path.exists(LIB_PATH):
        pytest.skip("libhdpissa.so not built")
    L = lib()
    assert ctypes.sizeof(ClipState) == 32
    assert L.hdp_grad_sumsq_workspace_bytes(0) == 0
    # one double per workgroup: at most the 2048-workgroup grid plus the scalar kernel's 64
    assert 8 <= L.hdp_grad_sumsq_workspace_bytes(5) <= L.hdp_grad_sumsq_workspace_bytes(40_000_000) <= 8 * (2048 + 64)
    assert L.hdp_grad_sumsq(None, 4, 1.0, 8, 8, 1 << 20, None) == 1 and b"null" in L.hdp_last_error()
    assert L.hdp_grad_sumsq(16, -1, 1.0, 8, 8, 1 << 20, None) == 1 and b"n < 0" in L.hdp_last_error()
    assert L.hdp_grad_sumsq(16, 4, 1.0, None, 8, 1 << 20, None) == 1
    assert L.hdp_grad_sumsq(16, 4, 1.0, 8, 8, 8, None) == 1 and b"workspace" in L.hdp_last_error()
    assert L.hdp_clip_finish(8, 1, 1.0, None, None) == 1 and b"null state" in L.hdp_last_error()
    assert L.hdp_clip_finish(None, 1, 1.0, 8, None) == 1
    assert L.hdp_clip_finish(8, -1, 1.0, 8, None) == 1
    for bad in (0.0, -2.0, math.nan):
        assert L.hdp_clip_finish(8, 1, bad, 8, None) == 1 and b"max_norm" in L.hdp_last_error()
    assert L.hdp_adam_factors_clip(None, None, None, None, 4, *([1.0] * 9), 1, None, None) == 1
    assert b"hdp_adam_factors_clip" in L.hdp_last_error()
    assert L.hdp_adam_factors_clip(None, None, None, None, -1, *([1.0] * 9), 1, None, None) == 1
    assert L.hdp_delta_plan_run_adam_clip(None, None, None, None, None, *([1.0] * 10), 1, None, None) == 1


# -- the step ------------------------------------------------------------------------------------------
def test_plain_ops_refuse_max_grad_norm_and_step_without_it():
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from hdpissa_amd.comm import LocalComm
    model = _model(SHAPES[:2])
    ops = CpuOps()
    layers = replace_with_custom_layer(model, ["q_proj", "k_proj"], 0, 1, 4, 16.0, ops=ops)
    with pytest.raises(NotImplementedError):
        HDPissaStep(model, 1, 0, comm=LocalComm(), ops=ops, max_grad_norm=1.0)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            HDPissaStep(model, 1, 0, comm=LocalComm(), ops=ClipCpuOps(), max_grad_norm=bad)
    st = HDPissaStep(model, 1, 0, comm=LocalComm(), ops=ops, max_grad_norm=None)
    assert st.clip_state is None and st.max_grad_norm is None
    with pytest.raises(RuntimeError):
        st.clip_info()
    for j, L in enumerate(layers):
        L.A.grad, L.B.grad = _grads(L, j, 0, 1)
    st.step(2e-3, 1)
    for j, L in enumerate(layers):  # the step as before: the oracle's unclipped Adam
        gA, gB = (x.numpy() for x in _grads(L, j, 0, 1))
        mA, vA, _ = O.adam_factors(gA, np.zeros_like(gA), np.zeros_like(gA), 1, 2e-3)
        assert np.array_equal(L.m_A.numpy(), mA) and np.array_equal(L.v_A.numpy(), vA)
        assert L.A.grad is None


@pytest.mark.parametrize("dtname", ["float32", "bfloat16"])
def test_step_wn1_clips_then_not(dtname):
    """Two steps, c between the two norms: step 1 clips (coef < 1), step 2 (10x smaller gradients) does not;
    m, v, delta equal the helper's bit for bit and W follows O.delta_w + O.merge of the helper's deltas."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from hdpissa_amd.comm import LocalComm
    from helpers import rel_err
    dt = getattr(torch, dtname)
    model, ops, r, lr = _model(SHAPES, dt), ClipCpuOps(), 4, 2e-3
    layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], 0, 1, r, 16.0, ops=ops)
    scales = {1: 1e-14, 2: 1e-15}
    n1 = math.sqrt(sum(R.sumsq(x.numpy()) for j, L in enumerate(layers) for x in _grads(L, j, 0, 1, scales[1])))
    c = 0.3 * n1
    st = HDPissaStep(model, 1, 0, comm=LocalComm(), ops=ops, max_grad_norm=c)
    mv = [[np.zeros(L.A.shape, np.float32), np.zeros(L.A.shape, np.float32), np.zeros(L.B.shape, np.float32),
           np.zeros(L.B.shape, np.float32)] for L in layers]
    for step in (1, 2):
        W0 = [L.W_res.float().numpy().copy() for L in layers]
        for j, L in enumerate(layers):
            L.A.grad, L.B.grad = _grads(L, j, 0, step, scales[step])
        st.step(lr, step)
        info = st.clip_info()
        ss = sum(R.sumsq(x.numpy()) for j, L in enumerate(layers) for x in _grads(L, j, 0, step, scales[step]))
        assert abs(info["sumsq"] - ss) <= ss * R.sumsq_bound(st.plans[0].arena.F)
        assert info["norm"] == float(R.norm_of(info["sumsq"])) and info["coef"] == float(R.coef_of(info["norm"], c))
        assert (info["coef"] < 1.0) == (step == 1) and not info["skipped"]
        for j, L in enumerate(layers):
            gA, gB = (x.numpy() for x in _grads(L, j, 0, step, scales[step]))
            mA, vA, dA = R.adam_factors_clip(gA, mv[j][0], mv[j][1], step, lr, info["coef"])
            mB, vB, dB = R.adam_factors_clip(gB, mv[j][2], mv[j][3], step, lr, info["coef"])
            mv[j] = [mA, vA, mB, vB]
            for got, ref in ((L.m_A, mA), (L.v_A, vA), (L.m_B, mB), (L.v_B, vB)):
                assert np.array_equal(got.numpy(), ref)
            da, db = L._arena.views(L._arena.delta, j)
            assert np.array_equal(da.numpy(), dA) and np.array_equal(db.numpy(), dB)
            A, B = L.A.detach().numpy(), L.B.detach().numpy()
            ref = O.merge(W0[j], O.delta_w([dA], [dB], [A], [B], dtname), dtname)
            got = L.W_res.float().numpy()
            if dt == torch.float32:
                assert rel_err(got, ref) < 1e-5
            else:
                assert rel_err(got - W0[j], ref - W0[j]) < 2e-2


def test_two_arenas_one_norm_and_order_of_operations():
    """Two replace_with_custom_layer calls = two arenas: the norm covers both, and no arena's Adam runs
    before the finish (every sum of squares, then the finish, then the Adams)."""
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from hdpissa_amd.comm import LocalComm
    model, ops = _model(SHAPES), ClipCpuOps()
    la = replace_with_custom_layer(model, ["q_proj", "k_proj"], 0, 1, 4, 16.0, ops=ops)
    lb = replace_with_custom_layer(model, ["o_proj", "up_proj"], 0, 1, 4, 16.0, ops=ops)
    layers = la + lb
    assert la[0]._arena is not lb[0]._arena
    st = HDPissaStep(model, 1, 0, comm=LocalComm(), ops=ops, max_grad_norm=1.0)
    assert len(st.plans) == 2
    for j, L in enumerate(layers):
        L.A.grad, L.B.grad = _grads(L, j, 0, 1)
    ops.log.clear()
    st.step(2e-3, 1)
    ss = _sumsq_layers(layers, 0, 1)
    info = st.clip_info()
    assert abs(info["sumsq"] - ss) <= ss * R.sumsq_bound(sum(p.arena.F for p in st.plans))
    only_a = sum(R.sumsq(x.numpy()) for j, L in enumerate(la) for x in _grads(L, j, 0, 1))
    assert info["sumsq"] > 1.5 * only_a  # (not the first arena alone)
    assert info["norm"] == float(R.norm_of(info["sumsq"])) and info["coef"] < 1.0
    kinds = [k for k, _ in ops.log]
    assert kinds == ["sumsq", "sumsq", "finish", "adam", "adam"], kinds
    ptrs = [p.arena.grad.data_ptr() for p in st.plans]
    assert [p for k, p in ops.log if k == "sumsq"] == ptrs and [p for k, p in ops.log if k == "adam"] == ptrs
    for j, L in enumerate(layers):  # both arenas were scaled by the one coefficient
        gA, _ = (x.numpy() for x in _grads(L, j, 0, 1))
        mA, vA, _ = R.adam_factors_clip(gA, np.zeros_like(gA), np.zeros_like(gA), 1, 2e-3, info["coef"])
        assert np.array_equal(L.m_A.numpy(), mA) and np.array_equal(L.v_A.numpy(), vA)


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_skip_keeps_moments_and_weights(bad):
    from hdpissa_amd import HDPissaStep, replace_with_custom_layer
    from hdpissa_amd.comm import LocalComm
    model, ops = _model(SHAPES[:2]), ClipCpuOps()
    layers = replace_with_custom_layer(model, ["q_proj", "k_proj"], 0, 1, 4, 16.0, ops=ops)
    st = HDPissaStep(model, 1, 0, comm=LocalComm(), ops=ops, max_grad_norm=math.inf)
    ar = layers[0]._arena
    for step in (1, 2, 3):
        for j, L in enumerate(layers):
            L.A.grad, L.B.grad = _grads(L, j, 0, step)
        if step == 2:
            layers[1].B.grad[3, 1] = bad
        m0, v0, W0 = ar.m.clone(), ar.v.clone(), [L.W_res.clone() for L in layers]
        st.step(2e-3, step)
        info = st.clip_info()
        assert info["skipped"] == (step == 2) and info["skipped_total"] == (0 if step == 1 else 1)
        assert not torch.any(ar.grad)
        if step == 2:
            assert torch.equal(ar.m, m0) and torch.equal(ar.v, v0) and not torch.any(ar.delta)
            assert all(torch.equal(L.W_res, w) for L, w in zip(layers, W0))
        else:
            assert info["coef"] == 1.0 and not torch.equal(ar.m, m0)


# -- the trainer ---------------------------------------------------------------------------------------
class _Toy(nn.Module):
    """Two adapter layers behind an embedding; an HF-style output (.loss)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.emb = nn.Embedding(32, 24)
        self.q_proj = nn.Linear(24, 40, bias=False)
        self.o_proj = nn.Linear(40, 16, bias=False)
        with torch.no_grad():
            self.emb.weight.copy_(torch.randn(32, 24, generator=g))
            self.q_proj.weight.copy_(torch.randn(40, 24, generator=g) * 0.1)
            self.o_proj.weight.copy_(torch.randn(16, 40, generator=g) * 0.1)
        for p in self.parameters():
            p.requires_grad = False

    def forward(self, input_ids, attention_mask=None, labels=None):
        h = self.o_proj(torch.tanh(self.q_proj(self.emb(input_ids))))
        return types.SimpleNamespace(loss=((h.sum(-1) - labels.float()) ** 2).mean())


def _batches(n):
    g = torch.Generator().manual_seed(11)
    return [dict(input_ids=torch.randint(0, 32, (2, 6), generator=g), attention_mask=torch.ones(2, 6, dtype=torch.long),
                 labels=torch.randint(0, 4, (2, 6), generator=g)) for _ in range(n)]


@pytest.mark.parametrize("loss_sync", ["step", "micro"])
def test_trainer_grad_norm_list_and_skipped_steps(loss_sync):
    from hdpissa_amd import replace_with_custom_layer
    from hdpissa_amd.comm import LocalComm
    from hdpissa_amd.train import HDPissaTrainer
    res = {}
    for c in (None, math.inf):  # the unclipped trainer gives the losses the clipped one must log too
        model, ops = _Toy(), ClipCpuOps()
        layers = replace_with_custom_layer(model, ["q_proj", "o_proj"], 0, 1, 4, 16.0, ops=ops)
        tr = HDPissaTrainer(model, 1, 0, 1e-3, 3, accumulation_steps=2, loss_sync=loss_sync, comm=LocalComm(), ops=ops,
                            max_grad_norm=c)
        norms = []
        for i, b in enumerate(_batches(6)):
            if c is not None and i == 3:  # poison the second window's gradient
                layers[0]._gA[0, 0] = math.inf
            if tr.micro_step(b) and c is not None:
                norms.append(tr.stepper.clip_info()["norm"])
        res[c] = (tr, norms)
    tr, norms = res[math.inf]
    assert tr.t == 3 and len(tr.grad_norm_list) == 3 and len(tr.loss_list) == 3 and len(tr.lr_list) == 3
    assert tr.grad_norm_list[0] == norms[0] and tr.grad_norm_list[2] == norms[2] and norms[0] > 0
    assert math.isinf(tr.grad_norm_list[1]) and math.isinf(norms[1])
    assert tr.skipped_steps == 1
    plain = res[None][0]
    assert plain.grad_norm_list == [] and plain.skipped_steps == 0
    assert tr.loss_list[0] == pytest.approx(plain.loss_list[0], rel=1e-12) and tr.lr_list == plain.lr_list


# -- two ranks under gloo ----------------------------------------------------------------------------
def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, wn, port, exchange, dtname, errfile):
    import sys
    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from hdpissa_amd import HDPissaStep, replace_with_custom_layer
        from hdpissa_amd.comm import TorchComm
        dt = getattr(torch, dtname)
        model, ops, r, lr = _model(SHAPES, dt), ClipCpuOps(), 4, 2e-3
        comm = TorchComm(rank, wn)
        layers = replace_with_custom_layer(model, [s[0] for s in SHAPES], rank, wn, r, 16.0, comm=comm, ops=ops)
        ss1 = sum(_sumsq_layers(layers, i, 1) for i in range(wn))
        c = 0.5 * math.sqrt(ss1)
        st = HDPissaStep(model, wn, rank, comm=comm, ops=ops, exchange=exchange, bucket_bytes=2048, max_grad_norm=c)
        ar = layers[0]._arena
        for step in (1, 2):
            for j, L in enumerate(layers):
                L.A.grad, L.B.grad = _grads(L, j, rank, step)
            if step == 2 and rank == 1:
                layers[2].A.grad[1, 2] = math.inf  # one rank's inf: every rank must skip
            m0, v0, W0 = ar.m.clone(), ar.v.clone(), [L.W_res.clone() for L in layers]
            st.step(lr, step)
            info = st.clip_info()
            rec = torch.tensor([info["sumsq"], info["norm"], info["coef"], float(info["skipped"])], dtype=torch.float64)
            recs = [torch.zeros_like(rec) for _ in range(wn)]
            dist.all_gather(recs, rec)
            assert all(torch.equal(recs[0].view(torch.int64), x.view(torch.int64)) for x in recs), recs
            for L in layers:
                w = L.W_res.float().clone()
                ws = [torch.zeros_like(w) for _ in range(wn)]
                dist.all_gather(ws, w)
                assert all(torch.equal(ws[0], x) for x in ws), "ranks hold different merged weights"
            if step == 1:
                assert abs(info["sumsq"] - ss1) <= ss1 * R.sumsq_bound(wn * ar.F), (info["sumsq"], ss1)
                assert info["coef"] == float(R.coef_of(info["norm"], c)) and info["coef"] < 1.0 and not info["skipped"]
                for j, L in enumerate(layers):
                    gA, gB = (x.numpy() for x in _grads(L, j, rank, 1))
                    mA, vA, _ = R.adam_factors_clip(gA, np.zeros_like(gA), np.zeros_like(gA), 1, lr, info["coef"])
                    mB, vB, _ = R.adam_factors_clip(gB, np.zeros_like(gB), np.zeros_like(gB), 1, lr, info["coef"])
                    assert np.array_equal(L.m_A.numpy(), mA) and np.array_equal(L.v_A.numpy(), vA)
                    assert np.array_equal(L.m_B.numpy(), mB) and np.array_equal(L.v_B.numpy(), vB)
                assert not all(torch.equal(L.W_res, w) for L, w in zip(layers, W0))
            else:
                assert info["skipped"] and info["skipped_total"] == 1
                assert torch.equal(ar.m, m0) and torch.equal(ar.v, v0) and not torch.any(ar.delta)
                assert all(torch.equal(L.W_res, w) for L, w in zip(layers, W0))
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("exchange,dtname", [("gather", "float32"), ("shard", "bfloat16"), ("allreduce", "float32")])
def test_gloo_two_ranks_global_norm_and_joint_skip(exchange, dtname, tmp_path):
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(_worker, args=(2, _port(), exchange, dtname, errfile), nprocs=2, join=True)
    except Exception:
        msg = open(errfile).read() if os.path.exists(errfile) else ""
        pytest.fail(f"worker failed:\n{msg}")
