"""compute_dtype=torch.bfloat16 on the host (CPU, CpuOps): float32 master weights with a bf16 compute copy.

The layer: a float32 CustomLinearLayer under bf16 autocast runs forward and backward on its copy W_lp (today
the backward dies on a bf16 x float32 matmul); y, dX and the probe gradients are held to float64 formulas on
the bf16-rounded x, W and gy at test_gpu_layer.py's bars (2e-2 relative for y and dX, which are bf16 GEMM
outputs; 1e-5 for the gradients).  The step: after two steps, at Wn = 1, at Wn = 2 over a loopback
communicator (gather, allreduce) and at Wn = 2 over gloo (all three), under each exchange, W_lp is the host replica (rounding.rne_bf16_bits) of W_res element for
element and W_res is bitwise the W_res of a twin model without the copy fed the same gradients; a counting
op set sees one shadow_group per launch site and bucket with shadowed modules, and none without a copy.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from cpu_ops import CpuOps
from helpers import rel_err
from test_clip_host import ClipCpuOps

BF = torch.bfloat16


def _replica(W: torch.Tensor) -> torch.Tensor:
    """bf16(W) by the host replica of the project's conversion."""
    from hdpissa_amd.rounding import rne_bf16_bits
    bits = rne_bf16_bits(W.detach().contiguous().cpu().numpy().view(np.uint32)).astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(BF).view(W.shape)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().cpu().view(torch.int16)


def _linear(inn, out, bias, seed, dt=torch.float32):
    g = torch.Generator().manual_seed(seed)
    lin = nn.Linear(inn, out, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(out, inn, generator=g) * 0.05)
        if bias:
            lin.bias.copy_(torch.randn(out, generator=g) * 0.1)
    return lin.to(dt).requires_grad_(False)


def test_float32_layer_under_bf16_autocast():
    """The case that raises without the feature: forward in bf16, backward bf16 x float32."""
    from hdpissa_amd import CustomLinearLayer
    inn, out, r, T = 50, 44, 4, 9
    L = CustomLinearLayer(_linear(inn, out, True, 0), "q_proj", 0, 1, r, 16.0, ops=CpuOps(), compute_dtype=BF)
    assert L.W_lp.dtype == BF and L.W_lp.shape == L.W_res.shape
    assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res)))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, T, inn, generator=g).requires_grad_(True)
    gy = torch.randn(2, T, out, generator=g)
    with torch.autocast("cpu", dtype=BF):
        y = L(x)
    assert y.dtype == BF
    y.backward(gy.to(BF))
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    xb = x.detach().to(BF).double().reshape(-1, inn)
    Wb = L.W_lp.double()
    gb = gy.to(BF).double().reshape(-1, out)
    y_ref = xb @ Wb.T + L.bias.detach().to(BF).double()
    e_y = rel_err(y.detach().float().reshape(-1, out).numpy(), y_ref.numpy())
    e_dx = rel_err(x.grad.reshape(-1, inn).numpy(), (gb @ Wb).numpy())
    A, B, s = L.A.detach().double(), L.B.detach().double(), L.probe_scale
    e_a = rel_err(L.A.grad.numpy(), (s * (gb @ B).T @ xb).numpy())
    e_b = rel_err(L.B.grad.numpy(), (s * gb.T @ (xb @ A.T)).numpy())
    print(f"y {e_y:.3e} dX {e_dx:.3e} gA {e_a:.3e} gB {e_b:.3e}")
    assert e_y < 2e-2 and e_dx < 2e-2
    assert e_a < 1e-5 and e_b < 1e-5
    # the no-grad forward runs the same GEMM
    with torch.no_grad(), torch.autocast("cpu", dtype=BF):
        assert torch.equal(L(x.detach()), y.detach())


def _qkv(compute_dtype, ops=None, dt=torch.float32):
    from hdpissa_amd import replace_with_custom_layer
    m = nn.Module()
    m.q_proj, m.k_proj, m.v_proj = _linear(40, 48, True, 1, dt), _linear(40, 24, False, 2, dt), _linear(40, 24, False, 3, dt)
    layers = replace_with_custom_layer(m, ["q_proj", "k_proj", "v_proj"], 0, 1, 4, 16.0, ops=ops or CpuOps(),
                                       compute_dtype=compute_dtype)
    return m, layers


def test_shared_activation_is_cast_once():
    """q / k / v handed one float32 x save one bf16 tensor (K2's shared-X sets are formed by pointer); the
    arena holds at most that one cast, and drops it with the backward pass and at step()."""
    from hdpissa_amd import HDPissaStep
    m, layers = _qkv(BF)
    arena = layers[0]._arena
    x = torch.randn(3, 7, 40, generator=torch.Generator().manual_seed(4))
    with torch.autocast("cpu", dtype=BF):
        ys = [L(x) for L in layers]
    saved = [y.grad_fn.saved_tensors[0] for y in ys]
    assert all(s.dtype == BF and s.data_ptr() == saved[0].data_ptr() for s in saved)
    assert arena.cast_cache is not None and arena.cast_cache[4].data_ptr() == saved[0].data_ptr()
    x2 = x.clone()  # another tensor: a new cast replaces the cached one
    with torch.autocast("cpu", dtype=BF):
        y2 = layers[0](x2)
    assert y2.grad_fn.saved_tensors[0].data_ptr() != saved[0].data_ptr()
    assert arena.cast_cache[0]() is x2
    x2.add_(1.0)  # the same object, written since: not the same activation
    with torch.autocast("cpu", dtype=BF):
        y3 = layers[1](x2)
    assert y3.grad_fn.saved_tensors[0].data_ptr() != y2.grad_fn.saved_tensors[0].data_ptr()
    sum(y.float().sum() for y in ys).backward()
    assert arena.cast_cache is None
    with torch.no_grad():
        layers[0](x)
    assert arena.cast_cache is not None
    HDPissaStep(m, 1, 0, ops=CpuOps()).step(1e-3, 1)
    assert arena.cast_cache is None
    xb = x.to(BF)  # an activation that is bf16 already is used as it is
    with torch.autocast("cpu", dtype=BF):
        yb = layers[2](xb)
    assert yb.grad_fn.saved_tensors[0].data_ptr() == xb.data_ptr()


def test_compute_dtype_values():
    from hdpissa_amd import CustomLinearLayer, replace_with_custom_layer
    from hdpissa_amd.train import HDPissaTrainer
    for bad in (torch.float16, torch.float32, "bfloat16"):
        with pytest.raises(ValueError):
            CustomLinearLayer(_linear(16, 8, False, 0), "q", 0, 1, 2, 16.0, ops=CpuOps(), compute_dtype=bad)
        with pytest.raises(ValueError):
            replace_with_custom_layer(nn.ModuleDict({"q_proj": _linear(16, 8, False, 0)}), ["q_proj"], 0, 1, 2, 16.0,
                                      ops=CpuOps(), compute_dtype=bad)
    with pytest.raises(ValueError):  # float64 master weights have no bf16 mode
        CustomLinearLayer(_linear(16, 8, False, 0, torch.float64), "q", 0, 1, 2, 16.0, ops=CpuOps(),
                          _factors=(torch.zeros(2, 16), torch.zeros(1, 8, 2)), compute_dtype=BF)
    m, _ = _qkv(None)
    with pytest.raises(ValueError):
        HDPissaTrainer(m, 1, 0, 1e-3, 4, ops=CpuOps(), compute_dtype=torch.float16)
    off = CustomLinearLayer(_linear(16, 8, False, 0), "q", 0, 1, 2, 16.0, ops=CpuOps())
    assert off.W_lp is None and off.compute_dtype is None


def test_bf16_weights_are_a_no_op():
    """compute_dtype=bfloat16 on a bf16 W_res: no copy, the plain path."""
    _, layers = _qkv(BF, dt=BF)
    x = torch.randn(5, 40, generator=torch.Generator().manual_seed(2)).to(BF)
    for L in layers:
        assert L.W_lp is None
        y = L(x)
        assert torch.equal(y, torch.nn.functional.linear(x, L.W_res, L.bias))
        y.float().sum().backward()
        assert L.A.grad is not None


def test_copy_is_not_in_the_state_dict(tmp_path):
    from hdpissa_amd.checkpoint import load_hdpissa_state, save_hdpissa_state
    m, layers = _qkv(BF)
    m0, _ = _qkv(None)
    assert sorted(m.state_dict()) == sorted(m0.state_dict())
    assert not any("W_lp" in k for k in m.state_dict())
    # a resume file written without the mode loads into a model with it, and the copy follows W_res
    with torch.no_grad():
        for L in m0.modules():
            if hasattr(L, "W_res"):
                L.W_res.mul_(1.5)
    path = str(tmp_path / "state.safetensors")
    save_hdpissa_state(m0, path, 3)
    stale = layers[0].W_lp.clone()
    assert load_hdpissa_state(m, path) == 3
    assert torch.equal(layers[0].W_lp, stale)  # (nothing has read it yet)
    x = torch.randn(4, 40)
    with torch.autocast("cpu", dtype=BF):
        for L in layers:
            L(x)
            assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res)))
    assert not torch.equal(layers[0].W_lp, stale)
    # load_state_dict and copy_ move the version counter too
    m.load_state_dict(_qkv(None)[0].state_dict())
    with torch.no_grad():
        layers[1].W_res.copy_(layers[1].W_res * 0.5)
        for L in layers:
            L(x)
            assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res)))


def test_copy_is_dropped_with_float32_master_weights():
    m, layers = _qkv(BF)
    m.to(BF)
    x = torch.randn(4, 40).to(BF)
    for L in layers:
        y = L(x)
        assert L.W_lp is None and L.compute_dtype is None
        assert torch.equal(y, torch.nn.functional.linear(x, L.W_res, L.bias))


class _LoopbackComm:
    """Single-process stand-in for a Wn-rank exchange: every rank sends what this rank sends."""
    name = "loopback"

    def __init__(self, world_size):
        self.world_size = world_size

    def allgather(self, send, recv):
        recv.view(self.world_size, -1).copy_(send.reshape(1, -1).expand(self.world_size, -1))

    allgather_any = allgather

    def allreduce_sum(self, buf):
        buf.mul_(self.world_size)

    def alltoall(self, send, recv):
        recv.copy_(send)

    def broadcast(self, t, root):
        pass


class CountingOps(ClipCpuOps):
    """The CPU op set (with the fused-norm stand-ins) and a shadow_group that casts by the host replica and records every call."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def shadow_group(self, pairs):
        assert pairs, "an empty shadow_group call"
        self.calls.append([dst.data_ptr() for dst, _ in pairs])
        for dst, src in pairs:
            assert dst.dtype == BF and src.dtype == torch.float32 and dst.shape == src.shape
            dst.copy_(_replica(src))


# q / k / v / o / up: with bucket_bytes = 6000 the W (and dW) buckets hold one or two modules each
SHAPES = [("q_proj", 24, 40), ("k_proj", 16, 40), ("v_proj", 16, 40), ("o_proj", 40, 24), ("up_proj", 56, 40)]


def _model(wn, rank, compute_dtype, ops, mixed=False):
    from hdpissa_amd import replace_with_custom_layer
    m = nn.Module()
    for j, (name, out, inn) in enumerate(SHAPES):
        setattr(m, name, _linear(inn, out, False, 10 + j, BF if mixed and j in (1, 3) else torch.float32))
    layers = replace_with_custom_layer(m, [s[0] for s in SHAPES], rank, wn, 4, 16.0, ops=ops,
                                       compute_dtype=compute_dtype)
    return m, layers


def _feed(layers, step):
    for j, L in enumerate(layers):
        g = torch.Generator().manual_seed(100 * step + j)
        L.A.grad = torch.randn(L.A.shape, generator=g) * 1e-14
        L.B.grad = torch.randn(L.B.shape, generator=g) * 1e-14


def _two_steps(wn, rank, exchange, clip, comm, comm0, model_kw=None):
    """Two steps of a shadowed model and its twin without the copy; returns the shadowed layers."""
    from hdpissa_amd import HDPissaStep
    ops = CountingOps()
    m, layers = _model(wn, rank, BF, ops, **(model_kw or {}))
    twin_ops = CountingOps()
    m0, layers0 = _model(wn, rank, None, twin_ops, **(model_kw or {}))
    kw = dict(exchange=exchange, bucket_bytes=6000, max_grad_norm=clip)
    st = HDPissaStep(m, wn, rank, ops=ops, comm=comm, **kw)
    st0 = HDPissaStep(m0, wn, rank, ops=twin_ops, comm=comm0, **kw)
    ops.calls.clear()
    for step in (1, 2):
        _feed(layers, step)
        _feed(layers0, step)
        st.step(1e-3, step)
        st0.step(1e-3, step)
        for L, L0 in zip(layers, layers0):
            assert torch.equal(L.W_res, L0.W_res), (step, L.name)
            assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res))), (step, L.name)
            assert L._shadow_version == L.W_res._version  # the next forward does not cast again
    assert not torch.equal(layers[0].W_res, _linear(SHAPES[0][2], SHAPES[0][1], False, 10).weight)  # (the steps moved W)
    assert twin_ops.calls == []  # compute_dtype=None: no call anywhere
    plan = st.plans[0]
    if exchange == "gather" or (exchange == "shard" and wn == 1):
        sites = 1 if wn == 1 else len(plan.g_buckets)
    elif exchange == "shard":
        sites = len(plan.s_buckets)
    else:
        sites = len(plan.a_buckets)
    assert sites > 1 or wn == 1
    assert len(ops.calls) == 2 * sites  # one call per launch site and bucket, per step
    per_step = [p for call in ops.calls[:sites] for p in call]
    assert sorted(per_step) == sorted(L.W_lp.data_ptr() for L in layers)  # every copy once
    return layers


# (the loopback communicator hands a rank its own rows back as the other rank's: shard at Wn = 2 runs over gloo)
@pytest.mark.parametrize("clip", [None, float("inf")])
@pytest.mark.parametrize("wn,exchange", [(1, "gather"), (1, "allreduce"), (1, "shard"), (2, "gather"), (2, "allreduce")])
def test_step_keeps_the_copy_current(wn, exchange, clip):
    _two_steps(wn, wn - 1, exchange, clip, _LoopbackComm(wn), _LoopbackComm(wn))


def _gloo_worker(rank, wn, port, errfile):
    import os
    import sys
    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "hd-pissa_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=wn)
    try:
        from hdpissa_amd.comm import TorchComm
        for exchange, clip in (("gather", None), ("allreduce", None), ("shard", None), ("shard", float("inf"))):
            layers = _two_steps(wn, rank, exchange, clip, TorchComm(rank, wn), TorchComm(rank, wn))
            for L in layers:  # the copies are bitwise equal across the ranks wherever W_res is
                w, lp = L.W_res.clone(), _bits(L.W_lp).reshape(-1).view(torch.uint8).clone()  # (gloo: no 16-bit gather)
                ws, lps = [torch.zeros_like(w) for _ in range(wn)], [torch.zeros_like(lp) for _ in range(wn)]
                dist.all_gather(ws, w)
                dist.all_gather(lps, lp)
                if exchange != "allreduce":
                    assert all(torch.equal(ws[0], x) for x in ws), (exchange, L.name)
                if all(torch.equal(ws[0], x) for x in ws):
                    assert all(torch.equal(lps[0], x) for x in lps), (exchange, L.name)
    except Exception as e:  # surface the assertion text to the parent
        import traceback
        with open(errfile, "a") as f:
            f.write(f"rank {rank}: {e!r}\n{traceback.format_exc()}\n")
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_gloo(tmp_path):
    """Wn = 2 as two processes over gloo, the three exchanges in turn (shard with and without the norm)."""
    import os
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    errfile = str(tmp_path / "err.txt")
    try:
        mp.spawn(_gloo_worker, args=(2, port, errfile), nprocs=2, join=True)
    except Exception:
        pytest.fail("worker failed:\n" + (open(errfile).read() if os.path.exists(errfile) else ""))


@pytest.mark.parametrize("exchange", ["gather", "allreduce", "shard"])
def test_mixed_model_casts_only_float32_modules(exchange):
    """bf16 modules of a mixed model keep no copy; a bucket of bf16 modules alone launches nothing."""
    from hdpissa_amd import HDPissaStep
    ops = CountingOps()
    m, layers = _model(2, 0, BF, ops, mixed=True)
    assert [L.W_lp is None for L in layers] == [False, True, False, True, False]
    st = HDPissaStep(m, 2, 0, ops=ops, comm=_LoopbackComm(2), exchange=exchange, bucket_bytes=1500)  # a module per bucket
    ops.calls.clear()
    _feed(layers, 1)
    st.step(1e-3, 1)
    assert len(ops.calls) == 3 and all(len(c) == 1 for c in ops.calls)
    for L in layers:
        if L.W_lp is not None:
            assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res)))


@pytest.mark.parametrize("exchange", ["gather", "allreduce"])
def test_skipped_step_still_leaves_the_copy_current(exchange):
    """A non-finite gradient norm: W_res stays, and the copy is cast from it all the same -- here from a W_res
    written behind the version counter's back just before the step."""
    from hdpissa_amd import HDPissaStep
    ops = CountingOps()
    m, layers = _model(2, 1, BF, ops)
    st = HDPissaStep(m, 2, 1, ops=ops, comm=_LoopbackComm(2), exchange=exchange, bucket_bytes=6000,
                     max_grad_norm=1.0)
    _feed(layers, 1)
    layers[2].A.grad[0, 0] = float("nan")
    for L in layers:
        L.W_res.data.mul_(1.25)
    W0 = [L.W_res.clone() for L in layers]
    st.step(1e-3, 1)
    assert st.clip_info()["skipped"]
    for L, w in zip(layers, W0):
        assert torch.equal(L.W_res, w)
        assert torch.equal(_bits(L.W_lp), _bits(_replica(w)))


def test_fallback_without_a_shadow_group_op():
    """An op set without shadow_group: the per-pair copy_ (torch's cast rounds to nearest even too)."""
    from hdpissa_amd import HDPissaStep
    m, layers = _model(1, 0, BF, CpuOps())
    st = HDPissaStep(m, 1, 0, ops=CpuOps())
    _feed(layers, 1)
    st.step(1e-3, 1)
    for L in layers:
        assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res)))


def test_residual_mode_refreshes_after_make_residual():
    from hdpissa_amd import replace_with_custom_layer
    m = nn.Module()
    m.q_proj = _linear(40, 24, False, 3)
    W0 = m.q_proj.weight.clone()
    (L,) = replace_with_custom_layer(m, ["q_proj"], 0, 1, 4, 16.0, ops=CpuOps(), residual=True, compute_dtype=BF)
    assert not torch.equal(L.W_res, W0)
    assert torch.equal(_bits(L.W_lp), _bits(_replica(L.W_res)))
    x = torch.randn(6, 40, generator=torch.Generator().manual_seed(0))
    with torch.autocast("cpu", dtype=BF):
        y = L(x)
    # W_lp x + the frozen components on the original x: the pretrained layer's output at bf16 accuracy
    assert rel_err(y.detach().float().numpy(), (x @ W0.T).numpy()) < 2e-2


def test_host_validation_of_the_kernel_entry():
    """hdp_shadow_group validates on the host, before any launch: testable without a GPU."""
    import ctypes
    import os
    from hdpissa_amd._lib import LIB_PATH, ShadowItem, lib
    if not os.path.exists(LIB_PATH):
        pytest.skip("libhdpissa.so not built")
    L = lib()
    assert L.hdp_shadow_group(0, None, None) == 0
    assert L.hdp_shadow_group(1, None, None) == 1
    assert L.hdp_shadow_group(-1, None, None) == 1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    items = (ShadowItem * 2)()
    items[0].dst, items[0].src, items[0].n = None, None, 0
    items[1].dst, items[1].src, items[1].n = p, p, -1
    assert L.hdp_shadow_group(2, items, None) == 1 and b"n < 0" in L.hdp_last_error()
    items[1].n = 0
    assert L.hdp_shadow_group(2, items, None) == 0  # empty items only: nothing to launch
    items[1].dst, items[1].src, items[1].n = None, p, 4
    assert L.hdp_shadow_group(2, items, None) == 1 and b"null pointer" in L.hdp_last_error()
    items[1].dst, items[1].src = p, None
    assert L.hdp_shadow_group(2, items, None) == 1 and b"null pointer" in L.hdp_last_error()
    items[1].dst, items[1].src = p + 1, p
    assert L.hdp_shadow_group(2, items, None) == 1 and b"aligned" in L.hdp_last_error()
